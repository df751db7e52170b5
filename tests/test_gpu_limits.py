"""Every family at the shape limit include/rechub_hip.h gives it, and one step past it.

At the limit (the limited dimension exactly ``H.RH_...``, every other one as small as the entry point takes): forward and
backward through the Python entry against the family's torch formulation evaluated in float64 on the CPU, under the rule of
the shape-range tests (test_gpu_session_hllm_shapes.compare): rtol 1e-4 plus the larger of 1e-5 of the tensor's largest
magnitude (1e-4 for a parameter gradient summed over rows) and 4 x the error of the same formulation in float32 on the CPU.

One past the limit: the Python entry refuses without a launch of the family's entry points (its ``_ok`` predicate is False,
or it raises), and the C entry point, called directly on real device tensors of that size, returns RH_E_UNSUPPORTED -- a
check that came after a launch would still touch valid memory.  Where a width must also be a multiple of 4 or a power of two,
"one past" is the next width that is wrong for the limit alone (noted per case).

Families whose shape-range tests already run at the limit read the macro there instead of a second at-limit case here: CIN
(test_gpu_cin), the residual quantizer (test_gpu_rq), the top-k scan's K (test_gpu_topk, test_gpu_ivf), the list metrics' K and
the diversity width (test_gpu_metric, test_gpu_beyond), the beam width (test_gpu_beam), attention pooling and the softmax
attention (test_gpu_session_hllm_shapes), HSTU (test_gpu_hstu), capsule routing (test_gpu_interest); AUGRU's and the gathers'
largest width is one of the widths test_gpu_sequence_shapes and test_gpu_kernels run (32 and 128 there are list entries)."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from test_gpu_session_hllm_shapes import compare, poison_small_blocks

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def limits():
    from torch_rechub_amd import _lib
    return _lib.H


def rnd(*shape, seed=0, scale=1.0):
    return scale * torch.randn(tuple(shape), generator=torch.Generator().manual_seed(seed + sum(shape)))


def at_limit(case, op, ref, inputs, params=(), const=None):
    """``op`` on the device against ``ref`` in float64 (and in float32 for the error scale), outputs and the gradients of every
    entry of ``inputs``; ``params`` names the inputs whose gradient is a sum over rows; ``const``: inputs without a gradient."""
    const = const or {}

    def run(fn, cast):
        leaves = {k: cast(v).requires_grad_(True) for k, v in inputs.items()}
        out = fn(**leaves, **{k: (cast(v) if v.is_floating_point() else v.to(cast(torch.zeros(1)).device)) for k, v in const.items()})
        outs = out if isinstance(out, tuple) else (out,)
        outs = [o for o in outs if o.is_floating_point()]
        torch.autograd.backward(outs, [cast(rnd(*o.shape, seed=7 + i)) for i, o in enumerate(outs)])
        res = {f"out{i}": o.detach() for i, o in enumerate(outs)}
        res.update({"g_" + k: v.grad for k, v in leaves.items()})
        return res

    want = run(ref, lambda t: t.detach().clone().double())
    cpu32 = run(ref, lambda t: t.detach().clone())
    poison_small_blocks()
    got = run(op, lambda t: t.detach().clone().to(dev()))
    torch.cuda.synchronize()
    from torch_rechub_amd import ops
    ops.check_errors()
    fails = []
    for name in want:
        compare(case, name, got[name], want[name], cpu32[name], 1e-4 if name[2:] in params else 1e-5, fails, rtol=1e-4)
    assert not fails, f"{case}: (tensor, error beyond rtol, bound) {fails}"


@contextlib.contextmanager
def no_launch_of(monkeypatch, prefix):
    """Fails the test when the Python side calls an entry point named ``prefix...`` (queries named *_supported excepted)."""
    from torch_rechub_amd import _lib
    real = _lib.call

    def spy(name, *args):
        assert not (name.startswith(prefix) and not name.endswith("_supported")), f"{name} was called"
        return real(name, *args)

    with monkeypatch.context() as m:
        m.setattr(_lib, "call", spy)
        yield


def refused_by_c(name, *args):
    """The C entry point itself, on real tensors: RH_E_UNSUPPORTED, and nothing was launched that could fault."""
    from torch_rechub_amd import _lib
    lib = _lib.load()
    conv = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
    rc = getattr(lib, name)(*conv)
    torch.cuda.synchronize()
    assert rc == _lib.H.RH_E_UNSUPPORTED, f"{name} returned {rc}: {lib.rh_last_error()}"


def z(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype, device=dev())


# ---- Dice ---------------------------------------------------------------------------------------------------------------
def dice_ref(x, alpha, eps=1e-3):
    c = x - x.mean(dim=1, keepdim=True)
    p = torch.sigmoid(c / torch.sqrt((c * c + eps).sum(dim=1, keepdim=True)))
    return p * x + (1 - p) * alpha * x


def test_dice_at_and_past_its_width(monkeypatch):
    from torch_rechub_amd import ops
    from torch_rechub_amd.basic.activation import Dice
    C = limits().RH_DICE_MAX_C
    at_limit("dice", lambda x, alpha: ops.dice(x, alpha, 1e-3), dice_ref, {"x": rnd(2, C), "alpha": rnd(1)}, params=("alpha",))
    mod = Dice().to(dev())
    x = rnd(2, C + 1).to(dev())
    with no_launch_of(monkeypatch, "rh_dice"):
        torch.testing.assert_close(mod(x), dice_ref(x, mod.alpha))
    refused_by_c("rh_dice_fwd", x, z(1), 1e-3, 2, C + 1, None, None, z(2, C + 1), None)
    refused_by_c("rh_dice_bwd", x, x, z(1), 1e-3, 2, C + 1, z(2, C + 1), z(64), None)


def test_batchnorm_dice_at_and_past_its_width():
    from torch_rechub_amd import ops
    C = limits().RH_BN_DICE_MAX_C

    def ref(h, gamma, beta, alpha):
        return dice_ref(F.batch_norm(h, None, None, gamma, beta, True, 0.1, 1e-5), alpha)

    def op(h, gamma, beta, alpha):
        bn = torch.nn.BatchNorm1d(C).to(dev())
        bn.weight, bn.bias = torch.nn.Parameter(gamma), torch.nn.Parameter(beta)
        assert ops.bn_dice_ok(h, bn, None)
        out = ops.bn_dice(h, bn, alpha, 1e-3)
        op.bn = bn
        return out

    leaves = {"h": rnd(3, C), "gamma": 1 + 0.1 * rnd(C, seed=1), "beta": 0.1 * rnd(C, seed=2), "alpha": rnd(1)}
    # gamma / beta become the module's Parameters: their gradients arrive on the module, so h and alpha are compared here and
    # the two affine gradients below
    want = {k: v.clone().double().requires_grad_(True) for k, v in leaves.items()}
    g = rnd(3, C, seed=9)
    ref(**want).backward(g.double())
    cpu32 = {k: v.clone().requires_grad_(True) for k, v in leaves.items()}
    ref(**cpu32).backward(g)
    got = {k: v.clone().to(dev()).requires_grad_(True) for k, v in leaves.items()}
    poison_small_blocks()
    out = op(**got)
    out.backward(g.to(dev()))
    torch.cuda.synchronize()
    fails = []
    compare("bn_dice", "out", out.detach(), ref(**{k: v.detach() for k, v in want.items()}), ref(**{k: v.detach() for k, v in cpu32.items()}),
            1e-5, fails, rtol=1e-4)
    grads = {"h": got["h"].grad, "alpha": got["alpha"].grad, "gamma": op.bn.weight.grad, "beta": op.bn.bias.grad}
    for k in leaves:
        compare("bn_dice", "g_" + k, grads[k], want[k].grad, cpu32[k].grad, 1e-5 if k == "h" else 1e-4, fails, rtol=1e-4)
    assert not fails, fails
    bn = torch.nn.BatchNorm1d(C + 1).to(dev())
    assert not ops.bn_dice_ok(z(3, C + 1), bn, None)
    lin = torch.nn.Linear(C + 1, 1).to(dev())
    assert not ops.bn_dice_head_ok(C + 1, bn, None, lin) and ops.bn_dice_head_ok(C, bn, None, torch.nn.Linear(C, 1).to(dev()))
    h = z(3, C + 1)
    refused_by_c("rh_bn_dice_bwd_stats", h, h, z(1), 1e-3, 3, C + 1, z(6, C + 1), z(C + 1), z(4096, 2, C + 1), z(4096), None)
    refused_by_c("rh_bn_dice_bwd_apply", h, h, z(1), 1e-3, 3, C + 1, z(6, C + 1), z(C + 1), z(3, C + 1), None)
    refused_by_c("rh_bn_dice_head_fwd", h, z(1), 1e-3, 3, C + 1, z(C + 1), z(C + 1), z(C + 1), z(1), z(3), None)


# ---- two-tower glue -----------------------------------------------------------------------------------------------------
def test_l2_normalize_at_and_past_its_width():
    """One past: d + 4, the next multiple of 4 (d + 1 is refused for its alignment already)."""
    from torch_rechub_amd import ops
    d = limits().RH_L2NORM_MAX_D
    at_limit("l2norm", lambda x: ops.l2_normalize(x, 1e-12), lambda x: F.normalize(x, p=2.0, dim=1, eps=1e-12), {"x": rnd(2, d)})
    x = z(2, d + 4)
    assert ops.l2_normalize_ok(z(2, d)) and not ops.l2_normalize_ok(x)
    refused_by_c("rh_l2norm_fwd", x, d + 4, 2, d + 4, 1e-12, z(2, d + 4), z(2), None)
    refused_by_c("rh_l2norm_bwd", x, z(2), x, d + 4, 2, d + 4, 1e-12, z(2, d + 4), None)


def test_cross_entropy_at_and_past_its_classes():
    from torch_rechub_amd import ops
    C = limits().RH_CE_MAX_C
    target = torch.tensor([C - 1, 0])
    at_limit("ce", lambda logits, target: ops.cross_entropy_mean(logits, target),
             lambda logits, target: F.cross_entropy(logits, target), {"logits": rnd(2, C, scale=3.0)}, const={"target": target})
    crit = torch.nn.CrossEntropyLoss()
    assert ops.cross_entropy_ok(crit, z(2, C), target.to(dev())) and not ops.cross_entropy_ok(crit, z(2, C + 1), target.to(dev()))
    t = target.to(dev())
    refused_by_c("rh_ce_fwd", z(2, C + 1), t, 2, C + 1, z(2), z(64), z(1, dtype=torch.int32), None)
    refused_by_c("rh_ce_bwd", z(2, C + 1), t, z(2), z(1), 2, C + 1, z(2, C + 1), None)


def test_inbatch_logits_at_and_past_its_width():
    from torch_rechub_amd import ops
    D = limits().RH_INBATCH_MAX_D
    neg = torch.tensor([[1], [0]])

    def ref(u, v, neg):
        return torch.cat([(u * v).sum(1, keepdim=True), (u.unsqueeze(1) * v[neg]).sum(2)], dim=1)

    at_limit("inbatch", lambda u, v, neg: ops.inbatch_logits(u, v, neg), ref, {"u": rnd(2, D), "v": rnd(2, D, seed=1)},
             const={"neg": neg})
    assert ops.inbatch_logits_ok(z(2, D), z(2, D)) and not ops.inbatch_logits_ok(z(2, D + 1), z(2, D + 1))
    u = z(2, D + 1)
    refused_by_c("rh_inbatch_logits_fwd", u, D + 1, u, D + 1, neg.to(dev()), 2, 2, D + 1, 1, 0, z(2, 2), z(1, dtype=torch.int32), None)
    refused_by_c("rh_inbatch_logits_bwd", u, D + 1, u, D + 1, neg.to(dev()), z(2, 2), 2, 2, D + 1, 1, 0, z(2, D + 1), z(2, D + 1), None)


def test_pair_cosine_and_band_logits_at_and_past_their_width():
    from torch_rechub_amd import ops
    D = limits().RH_TWOTOWER_MAX_D

    def pair_ref(hu, hp, hn):
        n = lambda t: F.normalize(t, p=2.0, dim=1, eps=1e-12)  # noqa: E731
        return (n(hu) * n(hp)).sum(1), (n(hu) * n(hn)).sum(1)

    at_limit("pair_cosine", lambda hu, hp, hn: ops.pair_cosine_scores(hu, hp, hn), pair_ref,
             {"hu": rnd(2, D), "hp": rnd(2, D, seed=1), "hn": rnd(2, D, seed=2)})

    def band_ref(u, v, w):
        s = torch.cosine_similarity(u.unsqueeze(1), v, dim=2, eps=1e-8) - torch.log(w)
        i = torch.arange(2)
        return torch.stack([s[i, (i + k) % 2] for k in range(2)], dim=1) / 0.5

    at_limit("band_logits", lambda u, v, w: ops.band_logits(u, v, w, 1, temperature=0.5), band_ref,
             {"u": rnd(2, D), "v": rnd(2, D, seed=1)}, const={"w": torch.tensor([0.3, 0.7])})
    a = z(2, D + 1)
    assert ops.pair_cosine_scores_ok(z(2, D), z(2, D), z(2, D)) and not ops.pair_cosine_scores_ok(a, a, a)
    assert ops.band_logits_ok(z(2, D), z(2, D), z(2), 1) and not ops.band_logits_ok(a, a, z(2), 1)
    refused_by_c("rh_pair_cosine_fwd", a, D + 1, a, D + 1, a, D + 1, 2, D + 1, 1e-12, z(2), z(2), z(3, 2), None)
    refused_by_c("rh_pair_cosine_bwd", a, D + 1, a, D + 1, a, D + 1, z(3, 2), z(2), z(2), 2, D + 1, 1e-12, z(2, D + 1), z(2, D + 1),
                 z(2, D + 1), None)
    refused_by_c("rh_band_logits_fwd", a, D + 1, a, D + 1, z(2) + 1, 2, D + 1, 2, 0.5, 1e-8, z(2, 2), z(2), z(2), None)
    refused_by_c("rh_band_logits_bwd", a, D + 1, a, D + 1, z(2), z(2), z(2, 2), 2, D + 1, 2, 0.5, 1e-8, z(2, D + 1), z(2, D + 1), None)


@pytest.mark.parametrize("axis", ["F", "D"])
def test_senet_at_and_past_each_limit(axis):
    from torch_rechub_amd import ops
    Fm, Dm = limits().RH_SENET_MAX_F, limits().RH_SENET_MAX_D
    Fn, D = (Fm, 1) if axis == "F" else (1, Dm)
    R = max(1, Fn // 3)

    def ref(x, w1, w2):
        return x * torch.relu(torch.relu(x.mean(-1) @ w1.T) @ w2.T).unsqueeze(-1)

    at_limit("senet_" + axis, lambda x, w1, w2: ops.senet(x, w1, w2).view(2, Fn, D), ref,
             {"x": rnd(2, Fn, D).abs(), "w1": rnd(R, Fn, seed=1).abs(), "w2": rnd(Fn, R, seed=2).abs()}, params=("w1", "w2"))
    Fn, D = (Fm + 1, 1) if axis == "F" else (1, Dm + 1)
    assert not ops.senet_ok(z(2, Fn, D), z(R, Fn), z(Fn, R))
    refused_by_c("rh_senet_fwd", z(2, Fn, D), Fn * D, z(R, Fn), z(Fn, R), 2, Fn, R, D, z(2, Fn * D), z(2, Fn), z(2, R), z(2, Fn), None)
    refused_by_c("rh_senet_bwd", z(2, Fn, D), Fn * D, z(R, Fn), z(Fn, R), z(2, Fn), z(2, R), z(2, Fn), z(2, Fn, D), Fn * D, 2, Fn, R,
                 D, z(2, Fn * D), z(64, 2 * R * Fn), None)


# ---- heads and cross layers ---------------------------------------------------------------------------------------------
def test_head_at_and_past_its_width():
    """The forward has no upper bound of its own; the backward's lane split sets the limit both sides share."""
    from torch_rechub_amd import ops
    K = limits().RH_HEAD_MAX_K
    at_limit("head", lambda h, w, b: ops.head_sigmoid(h, w, b), lambda h, w, b: torch.sigmoid((h @ w.T + b).squeeze(1)),
             {"h": rnd(2, K), "w": rnd(1, K, scale=K ** -0.5), "b": rnd(1)}, params=("w", "b"))
    assert ops.head_ok(z(2, K), torch.nn.Linear(K, 1), ()) and not ops.head_ok(z(2, K + 1), torch.nn.Linear(K + 1, 1), ())
    refused_by_c("rh_head_bwd", z(2, K + 1), K + 1, z(K + 1), z(2), z(2), 2, K + 1, z(2, K + 1), z(2), z(K + 1), z(1),
                 z(4096 * (K + 2)), None)


@pytest.mark.parametrize("axis", ["M", "d"])
def test_cross_v2_layer_at_and_past_each_limit(axis):
    from torch_rechub_amd import ops
    Mm, dm = limits().RH_CROSS_V2_MAX_M, limits().RH_CROSS_V2_MAX_D
    M, d = (Mm, 4) if axis == "M" else (1, dm)
    at_limit("cross_v2_" + axis, lambda x0, x, w, b: ops.cross_v2_layer(x0, x, w, b), lambda x0, x, w, b: x0 * (x @ w.T) + b + x,
             {"x0": rnd(M, d), "x": rnd(M, d, seed=1), "w": rnd(d, d, seed=2, scale=d ** -0.5), "b": rnd(d, seed=3)}, params=("w", "b"))
    M, d = (Mm + 1, 4) if axis == "M" else (1, dm + 1)
    assert not ops.cross_v2_shape_ok(z(M, d), z(d, d))
    refused_by_c("rh_cross_v2_fwd", z(M, d), z(M, d), z(d, d), z(d), M, d, z(M, d), z(M, d), None)
    refused_by_c("rh_cross_v2_dgrad", z(M, d), z(d, d), z(M, d), M, d, z(M, d), None)


def test_cross_network_at_and_past_its_width():
    """ops.cross_network asks rh_cross_max_layers(d) -- a query, no launch -- and refuses where it answers 0."""
    from torch_rechub_amd import ops
    d = limits().RH_CROSS_MAX_D
    at_limit("cross", lambda x, W, Bv: ops.cross_network(x, W, Bv), lambda x, W, Bv: x * (x @ W[0]).unsqueeze(1) + Bv[0] + x,
             {"x": rnd(2, d, scale=d ** -0.25), "W": rnd(1, d), "Bv": rnd(1, d, seed=1)}, params=("W", "Bv"))
    x = z(2, d + 1)
    with pytest.raises(ValueError, match=f"width {d + 1} unsupported by the HIP kernel \\(1..{d}\\)"):
        ops.cross_network(x, z(1, d + 1), z(1, d + 1))
    refused_by_c("rh_cross_fwd", x, d + 1, x, d + 1, z(1, d + 1), z(1, d + 1), 2, d + 1, 1, z(2, d + 1), d + 1, None)


@pytest.mark.parametrize("axis", ["d", "E"])
def test_cross_mix_epilogue_at_and_past_each_limit(axis, monkeypatch):
    from torch_rechub_amd import ops
    dm, Em = limits().RH_CROSS_MIX_MAX_D, limits().RH_CROSS_MIX_MAX_E
    d, E = (dm, 1) if axis == "d" else (1, Em)

    def ref(x0, xl, uv, gate, bias):
        return (gate.T.unsqueeze(2) * x0 * (uv + bias)).sum(0) + xl

    at_limit("cross_mix_" + axis, lambda x0, xl, uv, gate, bias: ops.cross_mix_epilogue(x0, xl, uv, gate, bias), ref,
             {"x0": rnd(2, d), "xl": rnd(2, d, seed=1), "uv": rnd(E, 2, d, seed=2), "gate": torch.softmax(rnd(2, E, seed=3), 1),
              "bias": rnd(d, seed=4)}, params=("bias",))
    d, E = (dm + 1, 1) if axis == "d" else (1, Em + 1)
    refused_by_c("rh_cross_mix_epilogue_fwd", z(2, d), z(2, d), z(E, 2, d), z(2, E), z(d), 2, d, E, z(2, d), None)
    refused_by_c("rh_cross_mix_epilogue_bwd", z(2, d), z(E, 2, d), z(2, E), z(d), z(2, d), 2, d, E, z(2, d), z(E, 2, d), z(2, E), None)
    # the layer (rank 3 keeps it off csrc/moe.hip) runs the tail on torch ops one past the limit, and on the kernel at it
    from torch_rechub_amd.basic.layers import CrossNetMix
    with no_launch_of(monkeypatch, "rh_cross_mix"):
        out = CrossNetMix(d, num_layers=1, low_rank=3, num_experts=E).to(dev())(rnd(2, d).to(dev()))
    assert out.shape == (2, d) and bool(torch.isfinite(out).all())
    d, E = (dm, 1) if axis == "d" else (1, Em)
    with pytest.raises(AssertionError, match="rh_cross_mix_epilogue_fwd was called"), no_launch_of(monkeypatch, "rh_cross_mix"):
        CrossNetMix(d, num_layers=1, low_rank=3, num_experts=E).to(dev())(rnd(2, d).to(dev()))


# ---- norms and attention ------------------------------------------------------------------------------------------------
def test_add_rms_norm_at_and_past_its_width():
    from torch_rechub_amd import ops
    D = limits().RH_RMS_NORM_MAX_D

    def ref(h, delta, w):
        hn = h + delta
        return hn, hn * torch.rsqrt((hn * hn).mean(-1, keepdim=True) + 1e-6) * w

    at_limit("rms", lambda h, delta, w: ops.add_rms_norm(h, delta, w, 1e-6), ref,
             {"h": rnd(2, D), "delta": rnd(2, D, seed=1), "w": 1 + 0.1 * rnd(D, seed=2)}, params=("w",))
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.add_rms_norm(z(2, D + 1), None, z(D + 1))
    refused_by_c("rh_add_rms_norm_fwd", z(2, D + 1), None, z(D + 1), 1e-6, 2, D + 1, None, z(2, D + 1), z(2), None)
    refused_by_c("rh_add_rms_norm_bwd", z(2, D + 1), z(D + 1), z(2), z(2, D + 1), None, 2, D + 1, z(2, D + 1), z(64, D + 1), None)


def test_sasrec_layer_norm_at_and_past_its_width():
    from torch_rechub_amd import ops
    D = limits().RH_SASREC_MAX_D
    at_limit("layer_norm", lambda x, w, b: ops.layer_norm(x, w, b, 1e-8), lambda x, w, b: F.layer_norm(x, (D,), w, b, 1e-8),
             {"x": rnd(2, D), "w": 1 + 0.1 * rnd(D, seed=1), "b": rnd(D, seed=2)}, params=("w", "b"))
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.layer_norm(z(2, D + 1), z(D + 1), z(D + 1), 1e-8)
    refused_by_c("rh_sasrec_head_fwd", z(2, D + 1), z(D + 1), z(D + 1), 1e-8, None, 0, None, 0, 0, 2, 1, D + 1, z(2, D + 1), None,
                 None, z(2, 2), None)
    refused_by_c("rh_sasrec_attn_in_fwd", z(2, D + 1), z(D + 1), z(D + 1), 1e-8, z(3 * (D + 1), D + 1), z(3 * (D + 1)), 2, D + 1,
                 z(2, D + 1), z(2, 3 * (D + 1)), z(2, 2), None)


def causal_ref(q, k, v):
    """One head: (B, L, dh) each."""
    L, dh = q.shape[1], q.shape[2]
    s = (q @ k.transpose(1, 2)) / dh ** 0.5
    s = s.masked_fill(torch.triu(torch.ones(L, L, dtype=torch.bool), 1), float("-inf"))
    return torch.softmax(s, dim=-1) @ v


@pytest.mark.parametrize("axis", ["L", "dh"])
def test_softmax_attention_at_and_past_each_limit(axis):
    from torch_rechub_amd import ops
    Lm, dm = limits().RH_ATTN_MAX_L, limits().RH_ATTN_MAX_DH
    L, dh = (Lm, 1) if axis == "L" else (1, dm)
    at_limit("softmax_attn_" + axis, lambda q, k, v: ops.softmax_attention(q, k, v, 1, 2 * Lm), causal_ref,
             {"q": rnd(1, L, dh), "k": rnd(1, L, dh, seed=1), "v": rnd(1, L, dh, seed=2)})
    L, dh = (Lm + 1, 1) if axis == "L" else (1, dm + 1)
    q = z(1, L, dh)
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.softmax_attention(q, q, q, 1, 2 * Lm)
    refused_by_c("rh_softmax_attn_fwd", q, q, q, dh, 1, L, 1, dh, None, 2 * Lm, 0, 1.0, 0.0, None, None, z(1, L, dh), z(1, 1, L), None)
    refused_by_c("rh_t5_attn_fwd", q, dh, q, q, dh, 1, L, L, 1, dh, None, 0, None, None, 0, 0.0, None, None, z(1, L, dh), z(1, 1, L),
                 None)


@pytest.mark.parametrize("axis", ["L", "H", "Dx"])
def test_attention_pool_at_and_past_each_limit(axis):
    from torch_rechub_amd import ops
    Lm, Wm = limits().RH_ATTN_POOL_MAX_L, limits().RH_ATTN_POOL_MAX_W
    dims = {"L": 1, "H": 1, "Dx": 1}
    dims[axis] = Lm if axis == "L" else Wm
    L, Hd, Dx = dims["L"], dims["H"], dims["Dx"]
    mask = torch.ones(2, L)
    mask[1, L // 2:] = 0 if L > 1 else 1

    def ref(P, r, w0, X, mask):
        s = (w0 * torch.sigmoid(P + r.unsqueeze(1))).sum(2)
        e = torch.exp(s) * mask
        return ((e / e.sum(1, keepdim=True)).unsqueeze(2) * X).sum(1)

    at_limit("attn_pool_" + axis, lambda P, r, w0, X, mask: ops.additive_attention_pool(P, r, w0, mask, X), ref,
             {"P": rnd(2, L, Hd), "r": rnd(2, Hd, seed=1), "w0": rnd(Hd, seed=2, scale=Hd ** -0.5), "X": rnd(2, L, Dx, seed=3)},
             params=("w0",), const={"mask": mask})
    dims[axis] += 1
    L, Hd, Dx = dims["L"], dims["H"], dims["Dx"]
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.additive_attention_pool(z(2, L, Hd), z(2, Hd), z(Hd), z(2, L) + 1, z(2, L, Dx))
    refused_by_c("rh_attn_pool_fwd", z(2, L, Hd), z(2, Hd), z(Hd), z(2, L) + 1, z(2, L, Dx), None, 2, L, Hd, Dx, 0, z(2, Dx), z(2, L),
                 z(2, 2), None)
    refused_by_c("rh_attn_pool_bwd", z(2, L, Hd), z(2, Hd), z(Hd), z(2, L, Dx), z(2, L), z(2, 2), z(2, Dx), 2, L, Hd, Dx, 0,
                 z(2, L, Hd), z(2, Hd), z(2, Hd), z(Hd), z(2, L, Dx), None)


def test_gru_at_and_past_its_hidden_size():
    from torch_rechub_amd import ops
    Hm = limits().RH_GRU_MAX_H
    torch.manual_seed(0)
    state = {k: v.detach().clone() for k, v in torch.nn.GRU(3, Hm, batch_first=True).state_dict().items()}
    x, g = rnd(2, 4, 3), rnd(2, 4, Hm, seed=1)
    res = {}
    for name, cast in (("want", lambda t: t.double()), ("cpu32", lambda t: t.clone()), ("got", lambda t: t.to(dev()))):
        mod = torch.nn.GRU(3, Hm, batch_first=True)
        mod = mod.double() if name == "want" else mod.to(dev()) if name == "got" else mod
        mod.load_state_dict({k: cast(v) for k, v in state.items()})
        xi = cast(x).requires_grad_(True)
        out = ops.gru_layers(mod, xi)[0] if name == "got" else mod(xi)[0]
        out.backward(cast(g))
        res[name] = {"out": out.detach(), "g_x": xi.grad, **{"g_" + k: p.grad for k, p in mod.named_parameters()}}
    torch.cuda.synchronize()
    fails = []
    for k in res["want"]:
        compare("gru", k, res["got"][k], res["want"][k], res["cpu32"][k], 1e-5 if k in ("out", "g_x") else 1e-4, fails, rtol=1e-4)
    assert not fails, fails
    big = torch.nn.GRU(3, Hm + 1, batch_first=True).to(dev())
    assert ops.gru_layers_ok(torch.nn.GRU(3, Hm, batch_first=True).to(dev()), z(2, 4, 3)) and not ops.gru_layers_ok(big, z(2, 4, 3))
    H1 = Hm + 1
    refused_by_c("rh_gru_fwd", z(2, 4, 3 * H1), z(3 * H1, H1), None, 2, 4, H1, z(2, 4, H1), z(2, 4, 3 * H1), None)
    refused_by_c("rh_gru_bwd", z(2, 4, 3 * H1), z(3 * H1, H1), z(2, 4, H1), z(2, 4, 3 * H1), z(2, 4, H1), 2, 4, H1, z(2, 4, 3 * H1),
                 z(2, 4, 3 * H1), None)


# ---- multi-interest towers ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", ["I", "D", "K"])
def test_listwise_at_and_past_each_limit(axis):
    from torch_rechub_amd import ops
    lim = limits()
    dims = {"I": 1, "D": 2, "K": 1}
    dims[axis] = {"I": lim.RH_LISTWISE_MAX_I, "D": lim.RH_LISTWISE_MAX_D, "K": lim.RH_LISTWISE_MAX_K}[axis]
    I, D, K = dims["I"], dims["D"], dims["K"]

    def ref(u, pos, neg):
        p, n = F.normalize(pos, dim=1, eps=1e-12), F.normalize(neg, dim=2, eps=1e-12)
        best = (u @ p.unsqueeze(2)).squeeze(2).argmax(1)
        ub = u[torch.arange(u.shape[0]), best]
        return (ub.unsqueeze(1) * torch.cat([p.unsqueeze(1), n], 1)).sum(2) / 0.7

    u = F.normalize(rnd(2, I, D), dim=2)
    at_limit("listwise_" + axis, lambda u, pos, neg: ops.listwise_logits(u, pos, neg, 0.7)[0], ref,
             {"u": u, "pos": rnd(2, D, seed=1), "neg": rnd(2, K, D, seed=2)})
    dims[axis] += 1
    I, D, K = dims["I"], dims["D"], dims["K"]
    assert not ops.listwise_ok(z(2, I, D), z(2, D), z(2, K, D))
    refused_by_c("rh_listwise_fwd", z(2, I, D), z(2, D), D, z(2, K, D), 2, I, D, K, 0.7, z(2, 1 + K), z(2, dtype=torch.int32), z(2, 1 + K),
                 None)
    refused_by_c("rh_listwise_bwd", z(2, I, D), z(2, D), D, z(2, K, D), z(2, dtype=torch.int32), z(2, 1 + K), z(2, 1 + K), 2, I, D, K,
                 0.7, z(2, I, D), z(2, D), z(2, K, D), None)


@pytest.mark.parametrize("axis", ["D", "LI", "ID"])
def test_self_attentive_pool_at_and_past_each_limit(axis):
    """L I and I D are products: the limit is met with the other factor at 1 where D's own bound allows it (I D at its limit
    needs I = 16 at D = 64, the largest D)."""
    from torch_rechub_amd import ops
    lim = limits()
    L, I, D = {"D": (1, 1, lim.RH_SA_MAX_D), "LI": (lim.RH_SA_MAX_LI, 1, 1), "ID": (1, lim.RH_SA_MAX_ID // lim.RH_SA_MAX_D, lim.RH_SA_MAX_D)}[axis]
    mask = torch.ones(2, L, dtype=torch.int32)
    mask[1, L // 2:] = 0 if L > 1 else 1

    def ref(A, E, mask):
        P = torch.softmax(A + -1e9 * (1 - mask.to(A.dtype)).unsqueeze(2), dim=1)
        return P.transpose(1, 2) @ E

    assert ops.sa_supported(L, I, D)
    at_limit("sa_" + axis, lambda A, E, mask: ops.sa_pool(A, E, mask), ref, {"A": rnd(2, L, I), "E": rnd(2, L, D, seed=1)},
             const={"mask": mask})
    L, I, D = {"D": (1, 1, D + 1), "LI": (L + 1, 1, 1), "ID": (1, I + 1, D)}[axis]
    assert not ops.sa_supported(L, I, D)
    refused_by_c("rh_sa_pool_fwd", z(2, L, I), z(2, L, D), None, 2, L, I, D, z(2, L, I), z(2, I, D), None)
    refused_by_c("rh_sa_pool_bwd", z(2, L, I), z(2, L, D), z(2, I, D), 2, L, I, D, z(2, L, I), z(2, L, D), None)


# ---- one past only: families whose shape-range tests run at the limit, or whose limit-sized launch is a whole step ----------
def test_gather_widths_one_past():
    """D = 128 is one of the widths test_gpu_kernels runs.  One past: 256, the next power-of-two multiple of 4."""
    from torch_rechub_amd import ops
    from torch_rechub_amd.basic import layers
    from torch_rechub_amd.basic.initializers import padded_dim
    lim = limits()
    assert lim.RH_EMBED_MAX_D == lim.RH_SEQ_POOL_MAX_D == lim.RH_DIN_ATT_MAX_D
    D = 2 * lim.RH_EMBED_MAX_D
    assert padded_dim(lim.RH_EMBED_MAX_D) == lim.RH_EMBED_MAX_D and padded_dim(lim.RH_EMBED_MAX_D + 1) is None
    assert layers._fusable_dim(lim.RH_SEQ_POOL_MAX_D) and not layers._fusable_dim(D)
    assert ops.din_dim_ok(lim.RH_DIN_ATT_MAX_D) and not ops.din_dim_ok(D)
    idx, flag = z(2, 2, dtype=torch.int64), z(1, dtype=torch.int32)

    def descriptors(Fn, width):
        """fdesc / idesc of Fn real tables (4, width) with real gradient buffers and real index columns, as ops.EmbedCall lays
        them out: table, gradient, vocab, padding_idx | index column, stride, slot."""
        tables, grads, cols = [z(4, width) for _ in range(Fn)], [z(4, width) for _ in range(Fn)], z(2, Fn, dtype=torch.int64)
        fdesc = torch.tensor([t.data_ptr() for t in tables] + [t.data_ptr() for t in grads] + [4] * Fn + [-1] * Fn, device=dev())
        idesc = torch.tensor([cols.data_ptr() + 8 * f for f in range(Fn)] + [Fn] * Fn + list(range(Fn)), device=dev())
        return fdesc, idesc, (tables, grads, cols)

    fdesc, idesc, keep = descriptors(1, D)
    refused_by_c("rh_embed_fwd", fdesc, idesc, 1, 2, 1, D, None, 0, D, z(2, D), D, None, None, None, None, None, 0, flag, None)
    refused_by_c("rh_seq_pool_fwd", z(4, D), 4, idx, 1, 2, 1, 2, 2, D, 0, -1, z(2, D), D, flag, None)
    refused_by_c("rh_din_att_input_fwd", z(2, 2, D), 2 * D, z(2, D), D, 2, 2, D, z(4, 4 * D), None)
    refused_by_c("rh_din_pool_fwd", z(2, 2, D), 2 * D, z(2, 2), 2, 2, D, z(2, D), None)
    # the fused LR keeps F D weights in LDS: F = limit / 4 + 1 fields of width 4
    Fn = lim.RH_EMBED_MAX_LR_FD // 4 + 1
    fdesc, idesc, keep = descriptors(Fn, 4)
    refused_by_c("rh_embed_fwd", fdesc, idesc, 1, 2, Fn, 4, None, 0, 4 * Fn, z(2, 4 * Fn), 4 * Fn, z(4 * Fn), z(1), z(2), None, None, 0,
                 flag, None)

def test_recurrences_norm_tables_and_scans_one_past():
    from torch_rechub_amd import ops
    lim = limits()
    D = 2 * lim.RH_AUGRU_MAX_D  # the next power of two: 33 is no width of the family at any limit
    assert ops.augru_ok(z(2, 3, 3 * lim.RH_AUGRU_MAX_D), lim.RH_AUGRU_MAX_D) and not ops.augru_ok(z(2, 3, 3 * D), D)
    refused_by_c("rh_augru_fwd", z(2, 3, 3 * D), None, z(D, 3 * D), None, 2, 3, D, z(2, 3, D), None)
    assert ops.topk_supported(lim.RH_TOPK_MAX_D, lim.RH_TOPK_MAX_K, lim.RH_TOPK_MAX_S)
    assert not ops.topk_supported(lim.RH_TOPK_MAX_D + 1, 1) and not ops.topk_supported(1, lim.RH_TOPK_MAX_K + 1)
    assert not ops.topk_supported(1, 1, lim.RH_TOPK_MAX_S + 1)
    assert ops.ivf_supported(1, 1, 0, lim.RH_IVF_MAX_NPROBE) and not ops.ivf_supported(1, 1, 0, lim.RH_IVF_MAX_NPROBE + 1)
    assert ops.sine_supported(lim.RH_SINE_MAX_S, lim.RH_SINE_MAX_E, lim.RH_SINE_MAX_T, lim.RH_SINE_MAX_K)
    for bad in ((lim.RH_SINE_MAX_S + 1, 1, 1, 1), (1, lim.RH_SINE_MAX_E + 1, 1, 1), (1, 1, lim.RH_SINE_MAX_T + 1, 1),
                (1, 1, lim.RH_SINE_MAX_T, lim.RH_SINE_MAX_K + 1)):
        assert not ops.sine_supported(*bad)
    assert ops.rq_supported(lim.RH_RQ_MAX_E, [lim.RH_RQ_MAX_CODES] * lim.RH_RQ_MAX_L)
    assert not ops.rq_supported(lim.RH_RQ_MAX_E + 1, [2]) and not ops.rq_supported(1, [lim.RH_RQ_MAX_CODES + 1])
    assert not ops.rq_supported(1, [2] * (lim.RH_RQ_MAX_L + 1))
    assert ops.capsule_supported(1, 1, lim.RH_CAPSULE_MAX_D, 0) and not ops.capsule_supported(1, 1, lim.RH_CAPSULE_MAX_D + 1, 0)
    V, Dq = 4, lim.RH_TOPK_MAX_D + 1
    refused_by_c("rh_topk_fwd", z(1, Dq), Dq, z(V, Dq), None, None, 0, None, 0, 1, Dq, V, 1, 1, z(64), z(1, 1, dtype=torch.int64), z(1, 1),
                 None)
    Di = lim.RH_ILD_MAX_D + 1
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.ild(z(2, 2, dtype=torch.int64), z(4, Di), [2])
    K = lim.RH_RANK_MAX_K + 1
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.coverage(z(2, K, dtype=torch.int64), 8, [1])
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.coverage(z(2, 16, dtype=torch.int64), 8, list(range(1, lim.RH_RANK_MAX_CUTOFFS + 2)))
    cut = (torch.zeros(1, dtype=torch.int32) + 1)
    import ctypes
    refused_by_c("rh_coverage", z(2, K, dtype=torch.int64), K, 2, K, 8, ctypes.c_void_p(cut.data_ptr()), 1, z(8, dtype=torch.int32),
                 z(1, dtype=torch.int64), None)


# ---- one past, on the entry points themselves: the families above whose Python side only asks a predicate -------------------
def ptrs(*tensors):
    """A HOST array of device pointers, as the entry points that take `const float* const*` read it."""
    import ctypes
    arr = (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])
    return ctypes.cast(arr, ctypes.c_void_p), arr


def ints(*values, ctype=None):
    import ctypes
    arr = ((ctype or ctypes.c_int) * len(values))(*values)
    return ctypes.cast(arr, ctypes.c_void_p), arr


def test_hstu_attention_one_past_each_limit():
    from torch_rechub_amd import ops
    lim = limits()
    for L, dqk, dv, nb in ((lim.RH_HSTU_MAX_L + 1, 1, 1, 1), (1, lim.RH_HSTU_MAX_DH + 1, 1, 1), (1, 1, lim.RH_HSTU_MAX_DH + 1, 1),
                           (1, 1, 1, lim.RH_HSTU_MAX_BUCKETS + 1)):
        N, W = 2 * lim.RH_HSTU_MAX_L, 2 * (dqk + dv)
        proj, pos_w, ts_w = z(1, L, W), z(2 * N - 1, 1), z(nb + 1, 1)
        with pytest.raises(RuntimeError, match="no HIP kernel"):
            ops.hstu_attention(proj, pos_w, ts_w, 1, dqk, dv, N, num_time_buckets=nb)
        refused_by_c("rh_hstu_attn_fwd", proj, W, 1, L, 1, dqk, dv, None, None, pos_w, ts_w, N, nb, 0, 1, 1.0, 1.0, z(1, L, dv), None)


@pytest.mark.parametrize("axis", ["F", "D"])
def test_ffm_at_and_past_each_limit(axis):
    from torch_rechub_amd import ops
    lim = limits()
    Fn, D = (lim.RH_FFM_MAX_F, 1) if axis == "F" else (2, lim.RH_FFM_MAX_D)

    def ref(x):
        i, j = torch.triu_indices(x.shape[1], x.shape[1], 1)
        return (x[:, i, j] * x[:, j, i]).reshape(x.shape[0], -1)

    at_limit("ffm_" + axis, lambda x: ops.ffm(x, reduce_sum=False).reshape(2, -1), ref, {"x": rnd(2, Fn, Fn, D)})
    Fn, D = (lim.RH_FFM_MAX_F + 1, 1) if axis == "F" else (2, lim.RH_FFM_MAX_D + 1)
    x, P = z(2, Fn, Fn, D), Fn * (Fn - 1) // 2
    with pytest.raises(RuntimeError, match="unsupported|no HIP kernel"):
        ops.ffm(x, reduce_sum=False)
    refused_by_c("rh_ffm_fwd", None, None, 1, x, Fn * Fn * D, 2, Fn, D, D, 0, z(2, P * D), P * D, z(1, dtype=torch.int32), None)


def test_cross_moe_capsule_and_din_first_layer_one_past():
    from torch_rechub_amd import ops
    lim = limits()
    E, r = lim.RH_CROSS_MOE_MAX_E, 4
    assert ops.cross_moe_ok(z(2, 8), lim.RH_CROSS_MOE_MAX_L, E, 8, r)
    for L, En, rn in ((lim.RH_CROSS_MOE_MAX_L + 1, 1, 4), (1, E + 1, 4), (1, 1, 2 * lim.RH_CROSS_MOE_MAX_R),
                      (1, lim.RH_CROSS_MOE_MAX_ER // 32 + 1, 32)):
        assert not ops.cross_moe_ok(z(2, 8), L, En, 8, rn)
        if L == 1:
            KP = (En * rn + En + 3) // 4 * 4
            refused_by_c("rh_cross_moe_mid_fwd", z(2, KP), z(En, rn, rn), 2, En, rn, z(2, En * rn), z(2, En * rn), z(2, En), z(2, KP), None)
    L = lim.RH_CROSS_MOE_MAX_L + 1
    U, keep_u = ptrs(*[z(1, 8, 4) for _ in range(L)])
    b, keep_b = ptrs(*[z(8) for _ in range(L)])
    Wg, keep_w = ptrs(z(8))
    refused_by_c("rh_cross_moe_pack", U, U, b, Wg, L, 1, 8, 4, z(L, 8, 8), z(L, 8, 8), None)
    # capsule routing: D, I D (types 0 / 1), I D D (type 2)
    Dm, IDm, IDDm = lim.RH_CAPSULE_MAX_D, lim.RH_CAPSULE_MAX_ID, lim.RH_CAPSULE_MAX_IDD
    mask = z(2, 2, dtype=torch.int32) + 1
    assert ops.capsule_supported(2, 1, Dm, 0) and ops.capsule_supported(2, IDm // Dm, Dm, 1) and ops.capsule_supported(2, IDDm // (Dm * Dm), Dm, 2)
    for I, D, kind in ((1, Dm + 1, 0), (IDm + 1, 1, 1), (IDDm // (Dm * Dm) + 1, Dm, 2)):
        assert not ops.capsule_supported(2, I, D, kind)
        Iu = 1 if kind == 0 else I
        refused_by_c("rh_capsule_fwd", z(2, 2, Iu * D), z(2, 2, D), z(2, I * D, D), mask, None, 2, 2, I, D, kind, 3, z(2, I, D), z(2, I, 2),
                     z(2, I, D), None)
    # the first layer of DIN's attention MLP: N past its limit (the next multiple of 64), D past its set (the next power of two)
    Nm, Dl = lim.RH_DIN_ATT_L1_MAX_N, lim.RH_DIN_ATT_L1_MAX_D
    for D, N in ((4, Nm + 64), (2 * Dl, 64)):
        hist, tgt, lin = z(2, 3, D), z(2, D), torch.nn.Linear(4 * D, N).to(dev())
        assert ops.din_att_l1_ok(z(2, 3, Dl), z(2, Dl), torch.nn.Linear(4 * Dl, Nm).to(dev())) and not ops.din_att_l1_ok(hist, tgt, lin)
        refused_by_c("rh_din_att_l1_fwd", hist, 3 * D, tgt, D, lin.weight, lin.bias, 2, 3, D, N, z(6, N), None, None)


def test_mlp_chain_entry_points_one_past():
    """The chain's widths and partial-row counts: ops.mlp_chain_ok is the Python side (test_gpu_tower_trips walks it)."""
    import ctypes
    from torch_rechub_amd import _lib, ops
    lim = limits()
    rng, ctr = z(4, dtype=torch.int64), z(1, dtype=torch.int64)
    K = lim.RH_HEAD_BN_MAX_K + 4  # widths are multiples of 4
    refused_by_c("rh_head_bnact_fwd", z(2, K), K, z(1, 2, K), 1, z(K), z(K), z(K), z(K), 0.1, 1e-5, 0.0, rng, ctr, z(4, K), z(K), z(1),
                 None, None, 2, K, z(2), None, None, None)
    refused_by_c("rh_head_bwd_bn", z(2, K), K, z(K), z(2), z(2), None, None, 2, K, z(2, K), z(2), z(K), z(1), z(4096 * (K + 1)), 1,
                 z(2, K), z(4, K), z(K), z(K), 0.0, rng, ctr, 1, z(4096, 2, K), None)
    K = lim.RH_LINEAR_BNACT_MAX_K + 4
    refused_by_c("rh_linear_bnact_fwd", z(2, K), K, 2, K, z(1, 2, K), 64, z(K), z(K), z(K), z(K), 0.1, 1e-5, 0.0, rng, ctr, z(4, K),
                 None, z(4, K), K, z(4), 4, z(2, 4), 4, None, None, None, None, None)
    n = lim.RH_BN_PRE_MAX_CHUNKS + 1
    refused_by_c("rh_bn_relu_dropout_bwd_pre", z(2, 4), z(2, 4), 2, 4, z(4), z(4), 0.0, rng, ctr, z(n, 2, 4), n, z(4, 4), z(2, 4), z(4),
                 z(4), 1, None)
    blocks = [(torch.nn.Linear(8, 8).to(dev()), torch.nn.BatchNorm1d(8).to(dev()), 0.0)]
    wide = lim.RH_HEAD_BN_MAX_K + 4
    assert ops.mlp_chain_ok(z(4, 8).requires_grad_(True), blocks, torch.nn.Linear(8, 1).to(dev()), ())
    assert not ops.mlp_chain_ok(z(4, 8).requires_grad_(True), [(torch.nn.Linear(8, wide).to(dev()), torch.nn.BatchNorm1d(wide).to(dev()), 0.0)],
                                torch.nn.Linear(wide, 1).to(dev()), ())
    # the grouped weight gradient: a reduction of RH_WGRAD_LONG_MIN_B rows is a long one
    B = lim.RH_WGRAD_LONG_MIN_B
    g, x = z(B, 1), z(B, 1)
    part = z(int(_lib.call("rh_linear_wgrad_workspace", B, 1, 1)) + 64)
    (pg, k1), (px, k2), (pp, k3) = ptrs(g), ptrs(x), ptrs(part)
    (ld, k4), (Bs, k5), (one, k6) = ints(1, ctype=ctypes.c_int64), ints(B), ints(1)
    refused_by_c("rh_linear_wgrad_partial_group", 1, pg, ld, px, ld, Bs, one, one, pp, None)
    # Adam: one tensor more than a launch takes
    T = lim.RH_ADAM_MAX_TENSORS + 1
    bufs = [z(4) for _ in range(4 * T)]
    tdesc = torch.tensor([t.data_ptr() for t in bufs] + [4] * T, device=dev())
    numel, k7 = ints(*([4] * T), ctype=ctypes.c_int64)
    refused_by_c("rh_adam_dense", tdesc, T, numel, z(16, dtype=torch.float64), 0, None)


def test_retrieval_and_metric_entry_points_one_past():
    import ctypes
    lim = limits()
    # residual quantizer: width, codebook size, levels
    for E, sizes in ((lim.RH_RQ_MAX_E + 1, [2]), (4, [lim.RH_RQ_MAX_CODES + 1]), (4, [2] * (lim.RH_RQ_MAX_L + 1))):
        L = len(sizes)
        C, keep_c = ptrs(*[z(n, E) for n in sizes])
        ne, keep_n = ints(*sizes)
        refused_by_c("rh_rq_fwd", z(2, E), C, ne, 2, E, L, 0, L, 0, z(2, L, dtype=torch.int32), z(2, E), z(2, E), z(4096, L), z(L), None)
    # SINE: S, E, T, K
    Sm, Em, Tm, Km = lim.RH_SINE_MAX_S, lim.RH_SINE_MAX_E, lim.RH_SINE_MAX_T, lim.RH_SINE_MAX_K
    for S, E, T, K in ((Sm + 1, 1, 1, 1), (1, Em + 1, 1, 1), (1, 1, Tm + 1, 1), (1, 1, Tm, Km + 1)):
        refused_by_c("rh_sine_interest_fwd", z(2, S, E), z(2, S, E), z(2, S), z(2, S, K), z(2, S, dtype=torch.int32) + 1, z(T, E), 2, S, E,
                     T, K, z(2, K, dtype=torch.int32), z(2, K, E), z(2, S, E), z(2, S), z(2, K, S), z(2, K, S), None)
        if T <= Tm:
            refused_by_c("rh_sine_aggregate_fwd", z(2, S, E), z(2, S), z(2, S, dtype=torch.int32) + 1, z(2, K, E), 1.0, 2, S, E, K, z(2, E),
                         None)
    # top-k scan: K, S (D is in the test above); the inverted-file scan: nprobe
    i64 = lambda *s: z(*s, dtype=torch.int64)  # noqa: E731
    i32 = lambda *s: z(*s, dtype=torch.int32)  # noqa: E731
    K = lim.RH_TOPK_MAX_K + 1
    refused_by_c("rh_topk_fwd", z(1, 4), 4, z(8, 4), None, None, 0, None, 0, 1, 4, 8, K, 1, z(2 * K + 64), i64(1, K), z(1, K), None)
    S = lim.RH_TOPK_MAX_S + 1
    refused_by_c("rh_topk_fwd", z(1, 4), 4, z(8, 4), None, i64(1, S) - 1, S, None, 0, 1, 4, 8, 1, 1, z(64), i64(1, 1), z(1, 1), None)
    P = lim.RH_IVF_MAX_NPROBE + 1
    off = torch.tensor([0, 8], dtype=torch.int32, device=dev())
    refused_by_c("rh_ivf_scan", z(1, 4), 4, z(8, 4), None, i32(8), off, 1, i32(P), i32(3), i32(3), None, 0, 1, 4, 8, 1, P, z(2 * P + 64),
                 i64(1, 1), z(1, 1), None)
    # list metrics: K, the number of cut-offs; diversity: the embedding width
    f64 = lambda *s: z(*s, dtype=torch.float64)  # noqa: E731
    cut1, keep1 = ints(1)
    cut9, keep9 = ints(*([1] * (lim.RH_RANK_MAX_CUTOFFS + 1)))
    K, n9 = lim.RH_RANK_MAX_K + 1, lim.RH_RANK_MAX_CUTOFFS + 1
    for Kn, cuts, n_k in ((K, cut1, 1), (4, cut9, n9)):
        refused_by_c("rh_rank_metrics", i64(2, Kn), Kn, 2, Kn, i64(3), i64(4), 4, cuts, n_k, f64(Kn), f64(Kn + 1), f64(1 << 16),
                     i64(n_k), i64(1), f64(n_k, 4), None, None)
        refused_by_c("rh_novelty", i64(2, Kn), Kn, 2, Kn, z(8) + 0.5, 0, 8, cuts, n_k, f64(1 << 16), f64(n_k), i64(n_k), None, None)
    D = lim.RH_ILD_MAX_D + 1
    refused_by_c("rh_ild", i64(2, 4), 4, 2, 4, z(8, D), D, 8, D, cut1, 1, f64(1 << 16), f64(1), i64(1), None, None)
    # AUGRU's backward (the forward is in the test above): the next power of two
    D = 2 * lim.RH_AUGRU_MAX_D
    refused_by_c("rh_augru_bwd", z(2, 3, 3 * D), None, z(D, 3 * D), None, z(2, 3, D), z(2, 3, D), 2, 3, D, z(2, 3, 3 * D), z(2, 3, D), None,
                 None)
