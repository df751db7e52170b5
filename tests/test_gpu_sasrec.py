"""SASRec on the MI355X: the four kernel pairs of csrc/sasrec.hip against the float64 restatement (tests/sasrec_oracle.py)
at the smallest shapes where each thing can go wrong, their dropout masks rebuilt on the host from the saved counter, the
LayerNorm edge rows, repeatable backwards, refused shapes, and the model against the reference's fixtures
(tools/gen_golden_sasrec.py): logits, user_tower, probe loss and gradients, three Adam steps, a captured train step under
dropout, the in-batch mode and top-k retrieval.

Widths: 1, 7 (odd k of the 2-wide MFMA step), 50 (the paper's: no multiple of 32), 64 (the tile), 65 (tile + 1: the wide
kernel), 128 (the maximum).  Rows M = B L: 1, 63, 64, 65, 130 with B = 1 and L = 1 among them; samples are unpadded, padded
at the front, padded at the back and all PAD in turn.  Inputs are N(0, 1), so no non-pad row has a variance near eps.
Tolerances are the project's kernel convention (test_gpu_sine.py, test_gpu_interest.py): rtol 1e-4, atol 1e-5 of the
tensor's largest magnitude; 1e-4 of it for the D x D weight gradients.  A ReLU input within 1e-6 of its largest magnitude
of zero (by the float64 oracle's numbers alone) would make the comparison a coin toss; such a draw is replaced by the next
seed (none of the cases below needs it).
"""
import ctypes
import json

import numpy as np
import pytest
import torch

import sasrec_oracle as O
from conftest import assert_trajectory_close, load_golden
from test_gpu_mlp_dropout_oracle import host_hash, host_keep, host_threshold  # noqa: F401  (the kernels' counter hash)

pytestmark = pytest.mark.gpu

EPS = 1e-8
WIDTHS = [1, 7, 50, 64, 65, 128]
ROWS = [(1, 1), (9, 7), (64, 1), (1, 65), (10, 13)]  # (B, L): M = 1, 63, 64, 65, 130
FEW = [(7, (9, 7)), (50, (10, 13)), (65, (1, 65)), (128, (64, 1))]  # (D, (B, L)) of the dropout / repeat tests


def dev():
    return torch.device("cuda:0")


def close(got, want, what, frac=1e-5):
    got = got.detach().cpu().numpy().astype(np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, f"{what}: {got.shape} != {want.shape}"
    assert np.isfinite(got).all(), what
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=frac * float(np.abs(want).max()) + 1e-30, err_msg=what)


def make_seq(B, L, g):
    """ids in [1, 23); sample b is full, padded at the front, padded at the back or all PAD as b % 4 says (B = 1: the
    front third is PAD)."""
    seq = torch.randint(1, 23, (B, L), generator=g)
    for b in range(B):
        kind = b % 4 if B > 1 else 1
        if kind == 1:
            seq[b, :(L // 2 if B > 1 else L // 3)] = 0
        elif kind == 2:
            seq[b, L // 2 + 1:] = 0
        elif kind == 3:
            seq[b] = 0
    return seq


def t64(t):
    return t.detach().double().cpu().numpy()


def to_dev(*ts, grad=True):
    return [t.to(dev()).requires_grad_(grad and t.is_floating_point()) for t in ts]


def rng_state():
    """(seed, next counter) of the device dropout state."""
    from torch_rechub_amd import ops
    st = ops._dropout_rng(dev()).cpu()
    return int(st[0]), int(st[1])


def keep_masks(n, p):
    """The keep-mask of element indices [0, n) of the NEXT call that draws a counter."""
    seed, ctr = rng_state()
    return host_keep(seed, ctr, n, p), ctr


# ---- input stage ---------------------------------------------------------------------------------------------------
def input_case(B, L, D, seed):
    g = torch.Generator().manual_seed(seed)
    seq = make_seq(B, L, g)
    gather = torch.randn(B, 3, L, D + 3, generator=g)  # the kernel reads a slice with both strides
    P = torch.randn(L + 2, D, generator=g)
    g_out = torch.randn(B, L, D, generator=g)
    return seq, gather, P, g_out


def run_input(seq, gather, P, g_out, p):
    from torch_rechub_amd import ops
    D = P.shape[1]
    gat, Pd = to_dev(gather, P)
    out = ops.sasrec_input(seq.to(dev()), gat[:, 0, :, :D], Pd, dropout_p=p, training=True)
    out.backward(g_out.to(dev()))
    return out, gat.grad[:, 0, :, :D], Pd.grad, gat.grad


@pytest.mark.parametrize("BL", ROWS, ids=lambda v: f"B{v[0]}L{v[1]}")
@pytest.mark.parametrize("D", WIDTHS)
def test_input_stage_against_float64(D, BL):
    B, L = BL
    seq, gather, P, g_out = input_case(B, L, D, 100 + D)
    out, g_e, g_P, g_all = run_input(seq, gather, P, g_out, 0.0)
    e = t64(gather)[:, 0, :, :D]
    close(out, O.input_fwd(seq.numpy(), e, t64(P)), "x0")
    assert (out[seq.to(dev()) == 0] == 0).all()
    want_e, want_P = O.input_bwd(seq.numpy(), t64(g_out), L + 2)
    close(g_e, want_e, "g_e")
    close(g_P, want_P, "g_P")
    assert (g_P[L:] == 0).all() and (g_all[:, 1:] == 0).all() and (g_all[..., D:] == 0).all()


@pytest.mark.parametrize("D,BL", FEW)
def test_input_stage_dropout_mask_is_the_counter_hash(D, BL):
    B, L = BL
    seq, gather, P, g_out = input_case(B, L, D, 200 + D)
    keep, ctr = keep_masks(B * L * D, 0.5)
    out, g_e, g_P, _ = run_input(seq, gather, P, g_out, 0.5)
    assert rng_state()[1] == ctr + 1
    keep = keep.reshape(B, L, D)
    e = t64(gather)[:, 0, :, :D]
    close(out, O.input_fwd(seq.numpy(), e, t64(P), keep, 0.5), "x0")
    want_e, want_P = O.input_bwd(seq.numpy(), t64(g_out), L + 2, keep, 0.5)
    close(g_e, want_e, "g_e")
    close(g_P, want_P, "g_P")


# ---- LayerNorm + in-projection ---------------------------------------------------------------------------------------
def rows_case(B, L, D, seed, n_mats):
    """x-like tensors (pad rows exactly zero where asked), LayerNorm affine, n_mats (D, D) weights with biases."""
    g = torch.Generator().manual_seed(seed)
    seq = make_seq(B, L, g)
    rn = lambda *s: torch.randn(*s, generator=g)  # noqa: E731
    gamma, beta = 1 + 0.3 * rn(D), 0.3 * rn(D)
    W = rn(n_mats * D, D) / max(D, 1)**0.5
    b = 0.3 * rn(n_mats * D)
    return g, seq, rn, gamma, beta, W, b


def attn_in_case(B, L, D, seed):
    g, seq, rn, gamma, beta, W, b = rows_case(B, L, D, seed, 3)
    x = rn(B, L, D) * (seq != 0)[..., None]
    return seq, x, gamma, beta, W, b, rn(B, L, D), rn(B, L, 3 * D)


@pytest.mark.parametrize("BL", ROWS, ids=lambda v: f"B{v[0]}L{v[1]}")
@pytest.mark.parametrize("D", WIDTHS)
def test_attention_in_against_float64(D, BL):
    from torch_rechub_amd import ops
    B, L = BL
    seq, x, gamma, beta, W, b, g_Q, g_qkv = attn_in_case(B, L, D, 300 + D)
    xd, ga, be, Wd, bd = to_dev(x, gamma, beta, W, b)
    Q, qkv = ops.sasrec_attention_in(xd, ga, be, Wd, bd, EPS)
    wQ, wqkv, cache = O.attn_in_fwd(t64(x), t64(gamma), t64(beta), t64(W), t64(b), EPS)
    close(Q, wQ, "Q")
    close(qkv, wqkv, "qkv")
    pad = (seq == 0).to(dev())
    if pad.any():  # an all-zero row gives exactly beta
        assert torch.equal(Q[pad], be.detach().expand(int(pad.sum()), D))
    torch.autograd.backward([Q, qkv], [g_Q.to(dev()), g_qkv.to(dev())])
    want = O.attn_in_bwd(t64(gamma), t64(W), cache, t64(g_qkv), t64(g_Q))
    close(xd.grad, want["x"], "g_x")
    close(ga.grad, want["gamma"], "g_gamma")
    close(be.grad, want["beta"], "g_beta")
    close(Wd.grad, want["W"], "g_in_proj_weight", 1e-4)
    close(bd.grad, want["b"], "g_in_proj_bias")


# ---- out-projection + LayerNorm + FFN --------------------------------------------------------------------------------
def ffn_case(B, L, D, seed):
    """Inputs, and a check on the oracle's numbers alone that no ReLU input sits on the kink."""
    for s in range(seed, seed + 8):
        g, seq, rn, gamma, beta, W, b = rows_case(B, L, D, s, 3)
        attn, Q, g_out = rn(B, L, D), rn(B, L, D), rn(B, L, D)
        c = dict(seq=seq, attn=attn, Q=Q, gamma=gamma, beta=beta, Wo=W[:D], W1=W[D:2 * D].reshape(D, D, 1),
                 W2=W[2 * D:].reshape(D, D, 1), bo=b[:D], b1=b[D:2 * D], b2=b[2 * D:], g_out=g_out)
        z, _ = O.ln_fwd(t64(Q) + t64(attn) @ t64(c["Wo"]).T + t64(c["bo"]), t64(gamma), t64(beta), EPS)
        h = z @ t64(c["W1"]).reshape(D, D).T + t64(c["b1"])
        if np.abs(h).min() > 1e-6 * np.abs(h).max():
            return c
    raise AssertionError("no draw without a ReLU input on the kink")


def run_ffn(c, p):
    from torch_rechub_amd import ops
    names = ("attn", "Q", "Wo", "bo", "gamma", "beta", "W1", "b1", "W2", "b2")
    t = dict(zip(names, to_dev(*(c[n] for n in names))))
    out = ops.sasrec_ffn(t["attn"], t["Q"], c["seq"].to(dev()), t["Wo"], t["bo"], t["gamma"], t["beta"], t["W1"], t["b1"],
                         t["W2"], t["b2"], EPS, dropout_p=p, training=True)
    out.backward(c["g_out"].to(dev()))
    return out, t


def ffn_oracle(c, keep1=None, keep2=None, p=0.0):
    a = {k: t64(v) for k, v in c.items() if k != "seq"}
    out, inter = O.ffn_fwd(a["attn"], a["Q"], c["seq"].numpy(), a["Wo"], a["bo"], a["gamma"], a["beta"], a["W1"], a["b1"],
                           a["W2"], a["b2"], EPS, keep1, keep2, p)
    return out, O.ffn_bwd(a["g_out"], a["gamma"], inter)


def check_ffn(c, out, t, want_out, want):
    close(out, want_out, "out")
    for n in ("attn", "Q", "bo", "gamma", "beta", "b1", "b2"):
        close(t[n].grad, want[n], "g_" + n)
    for n in ("Wo", "W1", "W2"):
        close(t[n].grad, want[n].reshape(t[n].shape), "g_" + n, 1e-4)


@pytest.mark.parametrize("BL", ROWS, ids=lambda v: f"B{v[0]}L{v[1]}")
@pytest.mark.parametrize("D", WIDTHS)
def test_ffn_against_float64(D, BL):
    B, L = BL
    c = ffn_case(B, L, D, 400 + D)
    out, t = run_ffn(c, 0.0)
    assert (out[c["seq"].to(dev()) == 0] == 0).all()
    check_ffn(c, out, t, *ffn_oracle(c))


@pytest.mark.parametrize("D,BL", FEW)
def test_ffn_dropout_masks_are_the_counter_hash_over_the_stated_ranges(D, BL):
    """dropout1 draws element indices [0, M D), dropout2 [M D, 2 M D) of ONE counter value.  The same comparison with the
    second range shifted by one element must fail: a wrong range cannot pass."""
    B, L = BL
    n = B * L * D
    c = ffn_case(B, L, D, 500 + D)
    keep, ctr = keep_masks(2 * n + 1, 0.5)
    out, t = run_ffn(c, 0.5)
    assert rng_state()[1] == ctr + 1
    k1, k2 = keep[:n].reshape(B, L, D), keep[n:2 * n].reshape(B, L, D)
    check_ffn(c, out, t, *ffn_oracle(c, k1, k2, 0.5))
    if n >= 63:  # (a single element's two masks can agree by chance)
        with pytest.raises(AssertionError):
            check_ffn(c, out, t, *ffn_oracle(c, k1, keep[n + 1:2 * n + 1].reshape(B, L, D), 0.5))


# ---- final LayerNorm + logits, and ops.layer_norm ----------------------------------------------------------------------
@pytest.mark.parametrize("BL", ROWS, ids=lambda v: f"B{v[0]}L{v[1]}")
@pytest.mark.parametrize("D", WIDTHS)
def test_head_and_layer_norm_against_float64(D, BL):
    from torch_rechub_amd import ops
    B, L = BL
    g, seq, rn, gamma, beta, _, _ = rows_case(B, L, D, 600 + D, 1)
    x = rn(B, L, D) * (seq != 0)[..., None]
    gather = rn(B, 3, L, D + 5)
    g_pos, g_neg, g_s = rn(B, L), rn(B, L), rn(B, L, D)
    xd, ga, be, gat = to_dev(x, gamma, beta, gather)
    pos, neg = ops.sasrec_head(xd, ga, be, gat[:, 1, :, :D], gat[:, 2, :, :D], EPS)
    pe, ne = t64(gather)[:, 1, :, :D], t64(gather)[:, 2, :, :D]
    s, wp, wn, cache = O.head_fwd(t64(x), t64(gamma), t64(beta), pe, ne, EPS)
    close(pos, wp, "pos_logits")
    close(neg, wn, "neg_logits")
    torch.autograd.backward([pos, neg], [g_pos.to(dev()), g_neg.to(dev())])
    want = O.head_bwd(t64(g_pos), t64(g_neg), t64(gamma), cache)
    close(xd.grad, want["x"], "g_x")
    close(gat.grad[:, 1, :, :D], want["pos_e"], "g_pos_e")
    close(gat.grad[:, 2, :, :D], want["neg_e"], "g_neg_e")
    close(ga.grad, want["gamma"], "g_gamma")
    close(be.grad, want["beta"], "g_beta")
    assert (gat.grad[:, 0] == 0).all() and (gat.grad[..., D:] == 0).all()

    xd, ga, be = to_dev(x, gamma, beta)
    out = ops.layer_norm(xd, ga, be, EPS)
    close(out, s, "layer_norm")
    pad = (seq == 0).to(dev())
    if pad.any():
        assert torch.equal(out[pad], be.detach().expand(int(pad.sum()), D))
    out.backward(g_s.to(dev()))
    g_x, g_gamma, g_beta = O.ln_bwd(t64(g_s), t64(gamma), cache[1])
    close(xd.grad, g_x, "layer_norm g_x")
    close(ga.grad, g_gamma, "layer_norm g_gamma")
    close(be.grad, g_beta, "layer_norm g_beta")


# ---- LayerNorm edge rows ---------------------------------------------------------------------------------------------
def ffn_forward_buffers(attn, Q, seq, wo, bo, gamma, beta, w1, b1, w2, b2):
    """rh_sasrec_ffn_fwd called through the C ABI at p = 0: its output buffers by the header's names (y = the LayerNorm's
    input, z = its output, a = the ReLU's output, stats, out)."""
    from torch_rechub_amd import _lib
    M, D = attn.shape
    buf = {n: torch.empty(M, D, device=dev()) for n in ("y", "z", "a", "out")}
    buf["stats"] = torch.empty(M, 2, device=dev())
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    null = ctypes.c_void_p(0)
    _lib.call("rh_sasrec_ffn_fwd", p(attn), p(Q), p(seq), p(wo), p(bo), p(gamma), p(beta), EPS, p(w1), p(b1), p(w2), p(b2), M, D,
              0.0, null, null, p(buf["y"]), p(buf["z"]), p(buf["a"]), p(buf["stats"]), p(buf["out"]),
              ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    return buf


@pytest.mark.parametrize("D", [7, 50, 128])
def test_zero_rows_give_beta_bitwise_and_constant_rows_stay_finite(D):
    """Row 0 all zero, row 1 constant 3.0 (its variance is rounding noise: no value comparison there), through every
    LayerNorm: ops.layer_norm, the query's, the FFN's (out_proj bias zero, so y is the zero row) and the head's."""
    from torch_rechub_amd import ops
    g, _, rn, gamma, beta, W, b = rows_case(4, 1, D, 700 + D, 3)
    x = rn(4, 1, D)
    x[0], x[1] = 0.0, 3.0
    xd, ga, be, Wd, bd = to_dev(x, gamma, beta, W, b, grad=False)
    xd.requires_grad_(True)
    out = ops.layer_norm(xd, ga, be, EPS)
    Q, qkv = ops.sasrec_attention_in(xd, ga, be, Wd, bd, EPS)
    assert torch.equal(out[0, 0], be) and torch.equal(Q[0, 0], be)
    seq = torch.ones(4, 1, dtype=torch.int64, device=dev())
    zero_b = torch.zeros(D, device=dev())
    wo, w1, w2 = (Wd[i * D:(i + 1) * D].contiguous() for i in range(3))
    ffn = ops.sasrec_ffn(xd, xd, seq, wo, zero_b, ga, be, w1, bd[:D].contiguous(), w2, zero_b, EPS)
    z = ffn_forward_buffers(xd.detach().view(4, D), xd.detach().view(4, D), seq, wo, zero_b, ga, be, w1, bd[:D].contiguous(),
                            w2, zero_b)["z"]
    assert torch.equal(z[0], be)
    pos, neg = ops.sasrec_head(xd, ga, be, xd, xd, EPS)
    assert pos[0, 0] == 0 and neg[0, 0] == 0
    (out.sum() + Q.sum() + qkv.sum() + ffn.sum() + pos.sum() + neg.sum()).backward()
    for t in (out, Q, qkv, ffn, z, pos, neg, xd.grad):
        assert torch.isfinite(t).all()


def test_point_wise_feed_forward_alone_against_float64():
    """The module called on its own (an unmodified reference model does that under integration.enable())."""
    from torch_rechub_amd.models.matching.sasrec import PointWiseFeedForward
    torch.manual_seed(11)
    m = PointWiseFeedForward(20, 0.0).to(dev()).train()
    x = torch.randn(3, 5, 20, device=dev(), requires_grad=True)
    out = m(x)
    w1, w2 = t64(m.conv1.weight).reshape(20, 20), t64(m.conv2.weight).reshape(20, 20)
    a = np.maximum(t64(x) @ w1.T + t64(m.conv1.bias), 0)
    close(out, a @ w2.T + t64(m.conv2.bias) + t64(x), "PointWiseFeedForward")
    out.sum().backward()
    close(x.grad, 1 + ((np.ones((3, 5, 20)) @ w2) * (a > 0)) @ w1, "g_inputs")
    m.dropout1.p = m.dropout2.p = 0.5
    assert not torch.equal(m(x), m(x))


# ---- repeatable backwards, refused shapes ------------------------------------------------------------------------------
@pytest.mark.parametrize("D,BL", FEW)
def test_backward_twice_is_bitwise_equal(D, BL):
    from torch_rechub_amd import ops
    B, L = BL
    c = ffn_case(B, L, D, 800 + D)
    seq, x, gamma, beta, W, b, g_Q, g_qkv = attn_in_case(B, L, D, 810 + D)
    iseq, gather, P, g_x0 = input_case(B, L, D, 820 + D)

    def once():
        grads = []
        _, t = run_ffn(c, 0.0)
        grads += [v.grad for v in t.values()]
        xd, ga, be, Wd, bd = to_dev(x, gamma, beta, W, b)
        Q, qkv = ops.sasrec_attention_in(xd, ga, be, Wd, bd, EPS)
        torch.autograd.backward([Q, qkv], [g_Q.to(dev()), g_qkv.to(dev())])
        grads += [xd.grad, ga.grad, be.grad, Wd.grad, bd.grad]
        xd, ga, be, pe = to_dev(x, gamma, beta, c["attn"])
        pos, neg = ops.sasrec_head(xd, ga, be, pe, pe, EPS)
        (pos * 2 + neg).sum().backward()
        grads += [xd.grad, ga.grad, be.grad, pe.grad]
        grads += list(run_input(iseq, gather, P, g_x0, 0.0)[1:3])
        return grads

    for a, b2 in zip(once(), once()):
        assert torch.equal(a, b2)


def test_unsupported_widths_raise_and_touch_nothing():
    """D = 129 is refused by the ops (before they allocate) and by the C entry points (before they launch: the output
    buffer keeps its bytes); a width the heads do not divide is refused by the model."""
    from torch_rechub_amd import _lib, ops
    from test_sasrec_host import features
    from torch_rechub_amd.models.matching import SASRec
    D = 129
    x = torch.randn(2, 3, D, device=dev())
    v, W, b = torch.ones(D, device=dev()), torch.randn(3 * D, D, device=dev()), torch.zeros(3 * D, device=dev())
    seq = torch.ones(2, 3, dtype=torch.int64, device=dev())
    for call in (lambda: ops.layer_norm(x, v, v, EPS), lambda: ops.sasrec_attention_in(x, v, v, W, b, EPS),
                 lambda: ops.sasrec_head(x, v, v, x, x, EPS), lambda: ops.sasrec_input(seq, x, x[0], 0.0),
                 lambda: ops.sasrec_ffn(x, x, seq, W[:D], v, v, v, W[:D], v, W[:D], v, EPS)):
        with pytest.raises(RuntimeError, match="no HIP kernel"):
            call()
    out = torch.full((6, D), 7.0, device=dev())
    stats = torch.full((6, 2), 7.0, device=dev())
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    null = ctypes.c_void_p(0)
    with pytest.raises(RuntimeError, match="unsupported"):
        _lib.call("rh_sasrec_head_fwd", p(x), p(v), p(v), EPS, null, 0, null, 0, 0, 6, 1, D, p(out), null, null, p(stats), st)
    with pytest.raises(RuntimeError, match="unsupported"):
        _lib.call("rh_sasrec_ffn_fwd", p(x), p(x), p(seq), p(W), p(v), p(v), p(v), EPS, p(W), p(v), p(W), p(v), 6, D, 0.0, null,
                  null, p(out), p(out), p(out), p(stats), p(out), st)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (stats == 7.0).all()
    model = SASRec(features(12), max_len=9, num_heads=1).to(dev())
    model.attention_layers[0].num_heads = 5
    ids = torch.randint(1, 23, (2, 7), device=dev())
    with pytest.raises(ValueError, match="not divisible"):
        model({"seq": ids, "pos": ids, "neg": ids})


# ---- the model against the reference's fixtures --------------------------------------------------------------------------
CFGS = ["d12h3b2", "d10h1b1"]


def load_model(cfg, dropout=0.0, item_feature=None):
    from test_sasrec_host import features
    from torch_rechub_amd.models.matching import SASRec
    gold = load_golden(f"model_sasrec_{cfg}.npz")
    c = json.loads(str(gold["cfg"]))
    model = SASRec(features(c["D"]), max_len=9, dropout_rate=dropout, num_blocks=c["blocks"], num_heads=c["H"],
                   item_feature=item_feature)
    model.load_state_dict({n[4:]: torch.from_numpy(gold[n]) for n in gold.files if n.startswith("sd0.")})
    return gold, model.to(dev())


def batch(gold, i):
    return {k: torch.from_numpy(gold[f"b{i}.{k}"]).to(dev()) for k in ("seq", "pos", "neg")}


def probe_loss(model, x):
    from torch_rechub_amd.basic.loss_func import BPRLoss
    pos, neg = model(x)
    return BPRLoss()(pos.reshape(-1), neg.reshape(-1))


@pytest.mark.parametrize("cfg", CFGS)
def test_eval_logits_and_user_tower_match_the_reference(cfg):
    gold, model = load_model(cfg)
    model.eval()
    x = batch(gold, 0)

    def tight(got, want, what):
        np.testing.assert_allclose(got.detach().cpu().numpy(), want, rtol=1e-5, atol=1e-5 * float(np.abs(want).max()),
                                   err_msg=what)

    with torch.no_grad():
        pos, neg = model(x)
        tight(pos, gold["pos_logits"], "pos_logits")
        tight(neg, gold["neg_logits"], "neg_logits")
        tight(model.user_tower(x), gold["user_tower"], "user_tower")
        model.mode = "user"
        tight(model(x), gold["user_mode"], "mode=user")


@pytest.mark.parametrize("cfg", CFGS)
def test_probe_loss_and_gradients_match_the_reference(cfg):
    gold, model = load_model(cfg)
    model.train()
    loss = probe_loss(model, batch(gold, 0))
    loss.backward()
    assert abs(loss.item() - float(gold["loss"])) <= 1e-5 * abs(float(gold["loss"]))
    sd_grads = {n: p.grad for n, p in model.named_parameters()}
    for n, g in sd_grads.items():
        want = gold["grad." + n]
        g = g[:, :want.shape[1]] if n.startswith("item_emb") else g  # (a padded table: the logical columns)
        wide = want.ndim >= 2 and "emb" not in n
        close(g, want, "grad " + n, 1e-4 if wide else 1e-5)
    # (the table's comparison above covers the rows reached only as a positive or a negative, and row 0)
    table = gold["grad.item_emb.embed_dict.seq.weight"]
    seen = set(gold["b0.seq"].reshape(-1).tolist())
    only_targets = (set(gold["b0.pos"].reshape(-1).tolist()) | set(gold["b0.neg"].reshape(-1).tolist())) - seen
    assert only_targets and all(np.abs(table[i]).max() > 0 for i in only_targets)


@pytest.mark.parametrize("cfg", CFGS)
def test_three_adam_steps_follow_the_reference_trajectory(cfg):
    """The key third of in_proj_bias only cancels inside the softmax: its gradient is noise on both sides, so it is only
    bounded, as conftest does for self_attn.in_proj_bias."""
    gold, model = load_model(cfg)
    model.train()
    lr, steps = float(gold["train.lr"]), 3
    opt = torch.optim.Adam(model.parameters(), lr=lr, weight_decay=float(gold["train.wd"]))
    losses = []
    for i in range(steps):
        loss = probe_loss(model, batch(gold, i))
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    np.testing.assert_allclose(losses, gold["train.losses"], rtol=1e-4)
    sd = model.state_dict()
    for n in (str(v) for v in gold["sd_keys"]):
        got, want = sd[n].detach().cpu().numpy(), gold["sd3." + n]
        if n.endswith("in_proj_bias"):
            d = got.shape[0] // 3
            assert np.abs(got[d:2 * d] - want[d:2 * d]).max() <= 2.1 * lr * steps, n
            got, want = np.delete(got, np.s_[d:2 * d]), np.delete(want, np.s_[d:2 * d])
        assert_trajectory_close(got, want, lr * steps, f"{cfg}: {n} after {steps} steps")


class _Listener(object):
    """A lazy optimizer's two hooks as no-ops: with a listener registered the gather looks its index buffer up in the
    descriptor cache, which may not grow during a capture."""

    def on_gather(self, record):
        pass

    def on_touch(self, record):
        pass


def test_training_under_dropout_draws_new_masks_eagerly_and_in_a_captured_step():
    from torch_rechub_amd import ops
    listener = _Listener()
    ops.add_lazy_listener(listener)  # (a weak reference: gone with this test)
    gold, model = load_model("d12h3b2", dropout=0.5)
    model.train()
    x = batch(gold, 0)
    a, b = model(x)[0].detach().clone(), model(x)[0].detach().clone()
    assert torch.isfinite(a).all() and torch.isfinite(b).all() and not torch.equal(a, b)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            model.zero_grad(set_to_none=True)
            probe_loss(model, x).backward()
    torch.cuda.current_stream().wait_stream(side)
    model.zero_grad(set_to_none=True)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        pos, neg = model(x)
        loss = (pos - neg).sigmoid().log().mean().neg()
        loss.backward()
    seen = []
    for _ in range(3):
        graph.replay()
        seen.append((pos.detach().clone(), model.last_layernorm.weight.grad.detach().clone(), loss.item()))
    for p1, g1, l1 in seen:
        assert torch.isfinite(p1).all() and torch.isfinite(g1).all() and np.isfinite(l1)
    assert not torch.equal(seen[0][0], seen[1][0]) and not torch.equal(seen[1][0], seen[2][0])
    assert not torch.equal(seen[0][1], seen[1][1])


def test_item_tower_and_in_batch_training():
    """The towers against plain indexing of our own table (the reference's item_tower cannot run), then five
    MatchTrainer(mode=0, in_batch_neg=True) steps in the trainer's captured form, which takes the model as it is: three
    eager warm-up steps, the capture, two replays."""
    from torch_rechub_amd.basic.features import SparseFeature
    from torch_rechub_amd.trainers import MatchTrainer
    from torch_rechub_amd.utils.data import DeviceDataLoader
    item = SparseFeature("item_id", vocab_size=23, embed_dim=12, shared_with="seq")
    gold, model = load_model("d12h3b2", item_feature=item)
    model.eval()
    x = dict(batch(gold, 0), item_id=torch.tensor([3, 0, 22, 7, 3], device=dev()))
    table = model.item_emb.embed_dict["seq"].weight.detach()[:, :12]
    with torch.no_grad():
        it = model.item_tower(x)
        assert it.shape == (5, 1, 12) and torch.equal(it[:, 0], table[x["item_id"]])
        user = model.user_tower(x)
        np.testing.assert_allclose(user.cpu().numpy(), gold["user_tower"], rtol=1e-5, atol=1e-5 * np.abs(gold["user_tower"]).max())
        scores = model(x)
        torch.testing.assert_close(scores, (user * it).sum(-1).squeeze())
        model.mode = "item"
        assert torch.equal(model(x), table[x["item_id"]]) and model.user_tower(x) is None
        model.mode = "user"
        assert model.item_tower(x) is None and model(x).shape == (5, 12)
        model.mode = None
    model.train()
    trainer = MatchTrainer(model, mode=0, in_batch_neg=True, optimizer_params={"lr": 1e-2}, n_epoch=1, device="cuda:0",
                           show_progress=False, use_graph=True)
    before = model.last_layernorm.weight.detach().clone()
    g = torch.Generator().manual_seed(5)
    rows = [torch.cat([torch.from_numpy(gold[f"b{i % 3}.{k}"]) for k in ("seq", "pos", "neg")], 1) for i in range(5)]
    cols = torch.cat([torch.cat(rows, 0), torch.randint(1, 23, (25, 1), generator=g)], 1).contiguous()  # five batches of 5
    loader = DeviceDataLoader(cols.to(dev()), [("seq", 7), ("pos", 7), ("neg", 7), "item_id"], None, [],
                              torch.ones(25, device=dev()), 5, shuffle=False)
    loss = trainer.train_one_epoch(loader)
    assert trainer._graph is not None and trainer._epoch_batches == 5
    assert np.isfinite(loss) and loss > 0
    assert not torch.equal(before, model.last_layernorm.weight.detach())


def test_a_block_is_three_launch_stages_on_the_hip_path():
    """Our class (the one integration.enable() binds to the reference's names) calls each of the block's three stages once
    per block and trains every block's parameters through them."""
    from torch_rechub_amd import ops
    gold, model = load_model("d12h3b2", dropout=0.25)
    model.train()
    calls = {n: 0 for n in ("sasrec_input", "sasrec_attention_in", "softmax_attention", "sasrec_ffn", "sasrec_head")}
    orig = {n: getattr(ops, n) for n in calls}

    def counted(n):
        def fn(*a, **k):
            calls[n] += 1
            return orig[n](*a, **k)
        return fn

    try:
        for n in calls:
            setattr(ops, n, counted(n))
        probe_loss(model, batch(gold, 0)).backward()
    finally:
        for n in calls:
            setattr(ops, n, orig[n])
    assert calls == {"sasrec_input": 1, "sasrec_attention_in": 2, "softmax_attention": 2, "sasrec_ffn": 2, "sasrec_head": 1}
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, n


def test_user_embeddings_through_topk_items_match_dense_topk():
    from torch_rechub_amd import ops
    gold, model = load_model("d12h3b2")
    model.eval()
    model.mode = "user"
    x = batch(gold, 0)
    live = (x["seq"] != 0).any(1)  # (the all-PAD sample's embedding is last_layernorm's bias, zero here: every score ties)
    with torch.no_grad():
        user = model(x)[live]
        table = model.item_emb.embed_dict["seq"].weight.detach()[:, :12].contiguous()
        ids, scores = ops.topk_items(user, table, 5)
        dense = user @ table.t()
        want = torch.topk(dense, 5, dim=1)
    assert torch.equal(ids, want.indices)
    torch.testing.assert_close(scores, want.values, rtol=1e-5, atol=1e-6)
