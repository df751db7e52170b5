"""csrc/encoder.hip on the MI355X against the float64 restatement (tests/encoder_oracle.py): ops.encoder_block at the widths,
hidden widths and row counts where a tile, a chunk or a row split ends, its dropout masks rebuilt on the host from the
saved counter, repeatable bits, the memory bound the design promises, ops.encoder_layer whole and for the last row alone,
and the refusals.

Tolerances are the kernel convention (tests/test_gpu_sasrec.py): rtol 1e-4, atol 1e-5 of the tensor's largest magnitude,
1e-4 of it for the weight matrices' gradients.  LeakyReLU's derivative jumps at 0: every case asserts that the float64
oracle alone has no pre-activation within 1e-6 of the largest magnitude of zero (the seeds below were chosen so)."""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

import encoder_oracle as EO
from test_gpu_mlp_dropout_oracle import RNG_SEED, host_keep

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")  # (the dropout state is kept per torch.device)

# (D, F, M, x strided, seed): each width edge (1, odd, half tile, tile, tile + 1, maximum), chunk edge (1, 63, 64, 65, 130 =
# two chunks + 2, 2048) and row edge (1, 63, 64, 65, 130) once; M = None: the smallest M with >= 2 row splits of two tiles
# and a ragged last one (rh_enc_nsplits)
CASES = [(1, 1, 1, False, 0), (7, 63, 63, False, 0), (32, 64, 64, False, 0), (64, 65, 65, False, 0), (65, 130, 130, False, 0),
         (128, 130, 65, False, 0), (32, 2048, 65, False, 1), (7, 1, 130, False, 0), (64, 64, 130, True, 0),
         (128, 63, 1, False, 0), (65, 64, 63, True, 0), (32, 3, None, False, 0)]
DROP_CASES = [(32, 65, 65, 0.2, 5), (65, 130, 63, 0.5, 9)]  # (D, F, M, p, first counter)
NAMES = ["attn", "x", "wo", "bo", "g1", "be1", "w1", "b1", "w2", "b2", "g2", "be2"]
MATRICES = {"wo", "w1", "w2"}


def split_rows(D, F):
    """An M (D <= 64, one chunk) whose weight kernel runs two row tiles per split and ends in a split of one."""
    from torch_rechub_amd import _lib
    ntiles, nsplits = _lib.query("rh_enc_nsplits", 64 * 511 - 5, D, F, out=(ctypes.c_int, ctypes.c_int))
    assert nsplits >= 2 and nsplits < ntiles < 2 * nsplits, (ntiles, nsplits)
    return 64 * 511 - 5


def make_case(D, F, M, seed):
    g = torch.Generator().manual_seed(1000 * D + F + seed)
    r = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    t = dict(attn=r(M, D), x=r(M, D), wo=r(D, D) / D**0.5, bo=0.1 * r(D), g1=1 + 0.1 * r(D), be1=0.1 * r(D),
             w1=r(F, D) / D**0.5, b1=0.1 * r(F), w2=r(D, F) / F**0.5, b2=0.1 * r(D), g2=1 + 0.1 * r(D), be2=0.1 * r(D))
    return t, r(M, D)


def run_oracle(t, g_out, p=0.0, keeps=(None, None, None)):
    leaves = {k: v.double().requires_grad_(True) for k, v in t.items()}
    out, u = EO.block(leaves["attn"], leaves["x"], leaves, 0.01, p, *keeps)
    out.backward(g_out.double())
    u = u.detach().abs()
    assert float(u.min()) > 1e-6 * float(u.max()), "a pre-activation at LeakyReLU's kink: take another seed"
    return out.detach(), {k: v.grad for k, v in leaves.items()}


def run_gpu(t, g_out, p=0.0, strided=False):
    from torch_rechub_amd import ops
    d = {k: v.to(DEV).requires_grad_(True) for k, v in t.items()}
    x = d["x"]
    if strided:  # rows 3 D apart: the last position of every sample of a (M, 3, D) tensor
        wide = torch.zeros(t["x"].shape[0], 3, t["x"].shape[1], device=DEV)
        wide[:, -1] = t["x"].to(DEV)
        d["x"] = wide.requires_grad_(True)
        x = d["x"][:, -1]
    out = ops.encoder_block(d["attn"], x, d["wo"], d["bo"], (d["g1"], d["be1"]), d["w1"], d["b1"], d["w2"], d["b2"],
                            (d["g2"], d["be2"]), slope=0.01, dropout_p=p, training=True)
    ctr = out.grad_fn.saved_tensors[-1]
    out.backward(g_out.to(DEV))
    ops.check_errors()
    grads = {k: v.grad for k, v in d.items()}
    if strided:
        assert not grads["x"][:, :-1].any()
        grads["x"] = grads["x"][:, -1]
    return out.detach(), grads, ctr


def miss(got, want, frac):
    """largest |got - want| / (frac max|want| + 1e-4 |want|): at most 1 when close"""
    got, want = got.detach().cpu().double().numpy(), want.detach().double().numpy()
    assert got.shape == want.shape and np.isfinite(got).all()
    return float((np.abs(got - want) / (frac * np.abs(want).max() + 1e-4 * np.abs(want) + 1e-30)).max())


def misses(out, grads, want_out, want_grads):
    res = {"out": miss(out, want_out, 1e-5)}
    res.update({"g_" + k: miss(grads[k], want_grads[k], 1e-4 if k in MATRICES else 1e-5) for k in NAMES})
    return res


@pytest.mark.parametrize("D,F,M,strided,seed", CASES, ids=lambda v: str(v))
def test_block_forward_and_every_gradient_against_float64(D, F, M, strided, seed):
    M = split_rows(D, F) if M is None else M
    t, g_out = make_case(D, F, M, seed)
    res = misses(*run_gpu(t, g_out, strided=strided)[:2], *run_oracle(t, g_out))
    assert max(res.values()) <= 1.0, res


@pytest.mark.parametrize("D,F,M,p,c0", DROP_CASES)
def test_dropout_masks_are_the_documented_ranges_of_one_counter(D, F, M, p, c0):
    from torch_rechub_amd import ops
    t, g_out = make_case(D, F, M, 0)
    ops._dropout_rng(DEV).copy_(torch.tensor([RNG_SEED, c0, 0, 0], dtype=torch.int64))
    out, grads, ctr = run_gpu(t, g_out, p=p)
    assert int(ctr) == c0 and int(ops._dropout_rng(DEV)[1]) == c0 + 1
    keep = torch.from_numpy(host_keep(RNG_SEED, c0, 2 * M * D + M * F, p))
    k_o, k_h, k_f = keep[:M * D].view(M, D), keep[M * D:M * D + M * F].view(M, F), keep[M * D + M * F:].view(M, D)
    res = misses(out, grads, *run_oracle(t, g_out, p, (k_o, k_h, k_f)))
    assert max(res.values()) <= 1.0, res
    wrong = misses(out, grads, *run_oracle(t, g_out, p, (k_f, k_h, k_o)))  # the ranges of drop_o and drop_f swapped
    assert wrong["out"] > 100 and wrong["g_attn"] > 100 and wrong["g_w2"] > 100, wrong


def test_backward_twice_gives_the_same_bits():
    D, F = 32, 3
    t, g_out = make_case(D, F, split_rows(D, F), 0)
    (_, a, _), (_, b, _) = run_gpu(t, g_out), run_gpu(t, g_out)
    assert all(torch.equal(a[k], b[k]) for k in NAMES)


def test_forward_and_backward_stay_under_one_hidden_tensor():
    """Saved tensors and workspaces are O(M D) or O(D F): the peak stays under ONE (M, F) float32 copy of the hidden."""
    M, D, F = 8448, 32, 2048
    t, g_out = make_case(D, F, M, 0)
    from torch_rechub_amd import ops
    d = {k: v.to(DEV).requires_grad_(True) for k, v in t.items()}
    g = g_out.to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ops.encoder_block(d["attn"], d["x"], d["wo"], d["bo"], (d["g1"], d["be1"]), d["w1"], d["b1"], d["w2"], d["b2"],
                      (d["g2"], d["be2"])).backward(g)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < M * F * 4


LAYERS = [(3, 8, 12, 2), (2, 65, 32, 4), (5, 1, 8, 8)]  # (B, L, D, H)


@pytest.mark.parametrize("last_only", [False, True])
@pytest.mark.parametrize("B,L,D,H", LAYERS)
def test_encoder_layer_against_the_float64_layer(B, L, D, H, last_only):
    from torch_rechub_amd import ops
    torch.manual_seed(10 * B + L)
    mod = nn.TransformerEncoderLayer(D, H, dim_feedforward=70, dropout=0.0, activation=nn.LeakyReLU(), batch_first=True)
    with torch.no_grad():
        for prm in mod.parameters():  # (the biases start at zero and the LayerNorms at one)
            prm.add_(0.1 * torch.randn_like(prm))
    mod = mod.to(DEV)
    x = torch.randn(B, L, D)
    keep = torch.ones(B, L, dtype=torch.bool)
    keep[0, :L // 2] = False      # padded at the front
    keep[1, L // 2:-1] = False    # padded at the back (the last position, BST's target, is never padding)
    keep[B - 1, :-1] = False      # only its last key
    g = torch.randn(B, D) if last_only else torch.randn(B, L, D)
    w_in, b_in, P = EO.layer_params(mod)
    x64 = x.double().requires_grad_(True)
    want, u = EO.layer(x64, w_in, b_in, H, keep, P)
    u = u.detach().abs()
    assert float(u.min()) > 1e-6 * float(u.max())
    want = want[:, -1] if last_only else want
    want.backward(g.double())
    xd = x.to(DEV).requires_grad_(True)
    got = ops.encoder_layer(xd, mod, keep.to(DEV), last_only=last_only)
    got.backward(g.to(DEV))
    ops.check_errors()
    att, mine = mod.self_attn, EO.layer_tensors(mod)
    pairs = {"out": (got, want.detach()), "g_x": (xd.grad, x64.grad), "g_w_in": (att.in_proj_weight.grad, w_in.grad),
             "g_b_in": (att.in_proj_bias.grad, b_in.grad), **{"g_" + k: (mine[k].grad, P[k].grad) for k in P}}
    # (the key bias shifts every score of a row alike: its gradient is zero in exact arithmetic, rounding noise in both)
    pairs["g_b_in"] = tuple(torch.cat([v[:D], v[2 * D:]]) for v in pairs["g_b_in"])
    res = {k: miss(a, b, 1e-4 if k in ("g_w_in", "g_wo", "g_w1", "g_w2") else 1e-5) for k, (a, b) in pairs.items()}
    assert max(res.values()) <= 1.0, res


def test_shapes_outside_the_limits_are_refused_before_any_launch():
    from torch_rechub_amd import _lib, ops
    fake, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)  # never dereferenced: the shape is checked first
    cap = (2**31 - 1) // (2 * _lib.H.RH_SASREC_MAX_D + 1)  # no cap of F's own: the workspace's int row length
    for D, F in ((129, 64), (32, cap + 1)):
        args = [fake] * 2 + [D] + [fake] * 4 + [1e-5] + [fake] * 6 + [1e-5, 0.01, 64, D, F, 0.0, null, null] + [fake] * 5 + [null]
        assert _lib.load().rh_enc_block_fwd(*args) == _lib.H.RH_E_UNSUPPORTED
    v = lambda *s: torch.zeros(*s, device=DEV)  # noqa: E731
    args = [v(4, 129), v(4, 129), v(129, 129), v(129), (v(129), v(129)), v(8, 129), v(8), v(129, 8), v(129), (v(129), v(129))]
    assert not ops.encoder_block_ok(*args)
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.encoder_block(*args)
