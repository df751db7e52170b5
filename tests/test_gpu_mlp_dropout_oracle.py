"""The ReLU MLP under dropout (Linear -> BatchNorm1d -> ReLU -> Dropout -> ... -> Linear(., 1) + e0 + e1 -> sigmoid) against a
float64 oracle whose dropout mask does NOT come from the kernels under test.

Both implementations are checked: the fused chain (ops._MlpChainFn: csrc/gemm.hip PRO / BNBWD, csrc/linear.hip) and the
layer-by-layer path (ops.linear_stats -> ops.bn_relu_dropout -> ops.head_sigmoid, csrc/mlp.hip; the head's backward with and
without ops.FUSE_HEAD_BN, the statistics from the epilogue's own pass or from the tile GEMM), plus ops.bn_relu_dropout called
directly.  A zero of the output may be ReLU-dead or dropped, so the mask cannot be read off the output: ``host_keep`` is a numpy
port of the counter hash documented in csrc/common.h, verified once bit for bit against ops.dropout (rh_session_dropout_fwd, a
separate kernel with its own test); from then on the oracle uses ``host_keep`` only.  Counter protocol (include/rechub_hip.h,
``saved_ctr = rng[1]++`` in the producing GEMM / epilogue): with the state set to (seed, c0, 0, 0), hidden layer l of step s
of an L-layer stack uses counter c0 + s L + l -- a p = 0 layer draws one too -- and rng[1] == c0 + steps L afterwards.

The oracle: nn.Linear / nn.BatchNorm1d in float64 on the CPU from the same initial state (BatchNorm weight in U(0.5, 1.5),
bias in U(-0.5, 0.5)), ReLU, times host_keep / (1 - p), the output Linear + e0 + e1, sigmoid; autograd gives the gradients.
Two steps with a random upstream gradient, gradients accumulated, so running statistics, num_batches_tracked and the counters
advance.  Compared after step 2: y, the gradients of x / e0 / e1 and of every parameter, running_mean, running_var,
num_batches_tracked == 2.

Tolerances = those of the PReLU epilogue against float64 (test_gpu_kernels.py::test_mlp_batchnorm_prelu_dropout_epilogue):
outputs and buffers rtol 1e-4 + atol 1e-5 max(1, max|want|); gradients 2e-4 max|want| + 2e-5 gmax (gmax = the largest
reference parameter gradient); a Linear bias in front of a BatchNorm has an exact-zero gradient and is bounded by
1e-4 max(1e-3, max|gx| sqrt(B)) as in test_mlp_chain_equals_the_layer_by_layer_kernels.  The p = 0 controls go through the
same helpers under the same numbers.

ReLU kink: a pre-activation within float32 rounding of 0 may be alive on one side and dead on the other.  That is a condition
on the inputs, not a tolerance: every ReLU case first asserts, from the float64 reference alone, min |bn_l| >= 1e-5 over
every hidden layer and both steps; the seeds below were chosen by scanning seeds 0..11 with the reference only
(``python tests/test_gpu_mlp_dropout_oracle.py`` repeats the scan on the CPU and prints the margins and the host-side
mismatch of the wrong masks).  No element is ever excluded from a comparison.

Negative controls (one per family): the kernel's result against an oracle with a deliberately wrong mask -- the counters of two
layers swapped (direct: c0 + 1 + s), or the mask indexed by row * pitch + col -- must miss by more than 100 x the tolerance.

Seed and float64 kink margin min |bn| per case (stacks are shared by the chain and the layer-by-layer tests):
  stacks  B2 [8,4] seed 3: 4.3e-01;  B32 [36,128] seed 8: 6.9e-04;  B33 [128,64,32] p (0.5, 0, 0.2) and the negative controls'
          p (0.5, 0.3, 0.2) seed 9: 1.3e-04;  B65 [256] seed 6: 2.3e-04;  B100 [36,4] seed 2, p > 0 and p = 0: 6.8e-04;
          B257 [128,256] seed 5: 2.8e-05;  B4096 [16,8] seed 7: 2.9e-05;  B5000 [8,4] seed 4: 3.3e-05;  B8200 [8] seed 9: 6.7e-05
  direct  37x32 seed 1: 2.0e-03;  1000x36 seed 8, p > 0 and p = 0: 8.3e-05;  100x36 behind the tile GEMM seed 6: 1.5e-03;
          9000x8 seed 1: 3.5e-05;  300x200 (BatchNorm -> Dropout, no kink) seed 0
Wrong masks, host side (wrong oracle against right oracle, in units of the tolerance): stack swap 6378 x, pitch 6996 x; direct
late counter 86132 x, pitch 84787 x.  float32 eager torch on the CPU through the same comparison stays below 0.004 of the
tolerance on every stack, so the bound is far from float32 rounding and far from a wrong mask.
Found by this module: with e0 and e1 both leaves the head's backward handed them two views of one buffer and the second step's
accumulation landed in both (error / tolerance 2299 on the gradients of e0 / e1 of the chain at B = 2, measured on the MI355X;
every other quantity of that case within 0.001 of its tolerance).  Fixed in ops._extra_grads; the -e2 cases are its regression.
Worst error / tolerance per path on the MI355X after the fix (the ``ORACLE`` lines each test prints): NOT MEASURED.
"""
import collections
import copy
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F64 = np.float64
STEPS = 2
RNG_SEED = 0x5DEECE66D1234  # > 2^32: the high word of the seed takes part in the hash
C0 = 7                      # call counter before the first step
KINK = 1e-5


def dev():
    return torch.device("cuda:0")


# --------------------------------------------------------------------------------------------------------------------------
# the mask, on the host
_M = 0xFFFFFFFF


def host_hash(seed, ctr, idx):
    """csrc/common.h rh_drop_hash(seed, ctr, idx) for an array of element indices: lowbias32 over
    idx ^ k0 ^ ((idx >> 32 + k1) * 0x85EBCA77), k0 = seed_lo ^ ctr_lo * 0x9E3779B1 ^ ctr_hi * 0xC2B2AE3D, k1 = seed_hi."""
    seed, ctr = int(seed) & (2 ** 64 - 1), int(ctr) & (2 ** 64 - 1)
    k0 = (seed & _M) ^ (((ctr & _M) * 0x9E3779B1) & _M) ^ (((ctr >> 32) * 0xC2B2AE3D) & _M)
    k1 = seed >> 32
    idx = np.asarray(idx, dtype=np.uint64)
    m, u = np.uint64(_M), np.uint64
    h = (idx & m) ^ u(k0) ^ (((((idx >> u(32)) + u(k1)) & m) * u(0x85EBCA77)) & m)
    h ^= h >> u(16)
    h = (h * u(0x7FEB352D)) & m
    h ^= h >> u(15)
    h = (h * u(0x846CA68B)) & m
    h ^= h >> u(16)
    return h


def host_threshold(p):
    """(uint32_t)(p * 4294967296.0) with p the C ABI's float."""
    return int(float(np.float32(p)) * 4294967296.0)


def host_keep(seed, ctr, n, p):
    """Keep flags of the n elements of call ``ctr``: hash >= uint32(float32(p) * 2^32).  Element (row, col) of a logical
    (B, C) layer is element row * C + col, whatever the pitch."""
    return host_hash(seed, ctr, np.arange(n, dtype=np.uint64)) >= np.uint64(host_threshold(p))


def _pitch(C):
    return (C // 16 + 1) * 16  # a row pitch that is never C itself


def layer_keep(ctr, B, C, p, wrong=None):
    """(B, C) float64 keep flags of one layer; wrong = "pitch": the mask a kernel would form from row * pitch + col."""
    if wrong == "pitch":
        idx = (np.arange(B, dtype=np.uint64)[:, None] * np.uint64(_pitch(C)) + np.arange(C, dtype=np.uint64)[None, :]).ravel()
        keep = host_hash(RNG_SEED, ctr, idx) >= np.uint64(host_threshold(p))
    else:
        keep = host_keep(RNG_SEED, ctr, B * C, p)
    return torch.from_numpy(keep.reshape(B, C).astype(F64))


# --------------------------------------------------------------------------------------------------------------------------
# tolerances (module docstring)
def out_ratio(got, want):
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    assert got.shape == want.shape, (got.shape, want.shape)
    atol = 1e-5 * max(1.0, float(np.abs(want).max()))
    return float((np.abs(got - want) / (atol + 1e-4 * np.abs(want))).max())


def grad_ratio(got, want, gmax):
    got, want = np.asarray(got, F64), np.asarray(want, F64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max() / (2e-4 * float(np.abs(want).max()) + 2e-5 * gmax))


def compare(got, want, B, noise=()):
    """{quantity: error / tolerance} of a kernel result against an oracle result."""
    r = {"y": out_ratio(got["y"], want["y"])}
    gmax = max(float(np.abs(v).max()) for v in want["params"].values())
    for k in ("gx", "g0", "g1"):
        if want.get(k) is not None:
            r[k] = grad_ratio(got[k], want[k], gmax)
    for n, w in want["params"].items():
        if n in noise:  # exact-zero gradient: rounding noise of a sum over B rows
            r["grad " + n] = float(np.abs(got["params"][n]).max()) / (1e-4 * max(1e-3, float(np.abs(want["gx"]).max()) * B ** 0.5))
        else:
            r["grad " + n] = grad_ratio(got["params"][n], w, gmax)
    for n, w in want["bufs"].items():
        if n.endswith("num_batches_tracked"):
            r[n] = 0.0 if int(got["bufs"][n]) == int(w) == STEPS else float("inf")
        else:
            r[n] = out_ratio(got["bufs"][n], w)
    return r


def worst(r):
    k = max(r, key=lambda q: r[q])
    return k, r[k]


def assert_within(r, what):
    k, v = worst(r)
    print(f"ORACLE {what}: worst error / tolerance {v:.3f} ({k})")
    bad = {q: round(v_, 3) for q, v_ in r.items() if not v_ <= 1.0}
    assert not bad, f"{what}: error / tolerance {bad}"


def _np(t):
    a = t.detach().double().cpu().numpy().copy()
    a.setflags(write=False)
    return a


def _collect(y, gx, g0, g1, net):
    return dict(y=_np(y), gx=_np(gx), g0=None if g0 is None else _np(g0), g1=None if g1 is None else _np(g1),
                params={n: _np(q.grad) for n, q in net.named_parameters()},
                bufs={n: _np(b) for n, b in net.named_buffers()})


# --------------------------------------------------------------------------------------------------------------------------
# the stack: cases, initial state, oracle
Stack = collections.namedtuple("Stack", "B K0 pitch dims ps extras head_bias seed")
#                 B    K0 pitch dims            ps               extras head_bias seed
S_MIN = Stack(2, 16, 16, (8, 4), (0.5, 0.2), 2, True, 3)
S_32 = Stack(32, 40, 40, (36, 128), (0.2, 0.3), 2, True, 8)
S_33 = Stack(33, 33, 48, (128, 64, 32), (0.5, 0.0, 0.2), 2, True, 9)  # K0 = 33: a column slice of a 48-wide buffer
S_65 = Stack(65, 40, 40, (256,), (0.3,), 0, False, 6)
S_100 = Stack(100, 24, 24, (36, 4), (0.1, 0.5), 1, True, 2)
S_257 = Stack(257, 64, 64, (128, 256), (0.2, 0.5), 2, True, 5)
S_4096 = Stack(4096, 20, 20, (16, 8), (0.2, 0.1), 2, True, 7)
S_CTRL = Stack(100, 24, 24, (36, 4), (0.0, 0.0), 1, True, 2)          # the p = 0 control
S_5000 = Stack(5000, 20, 20, (8, 4), (0.2, 0.5), 2, True, 4)        # past the chain; epilogue in two launches
S_8200 = Stack(8200, 12, 12, (8,), (0.3,), 1, True, 9)                # epilogue in three launches
CHAIN_CASES = [S_MIN, S_32, S_33, S_65, S_100, S_257, S_4096, S_CTRL]
#              (stack, FUSE_HEAD_BN, statistics from the tile GEMM)
LAYER_CASES = [(S_MIN, True, False), (S_33, True, False), (S_33, False, False), (S_100, True, True), (S_100, False, False),
               (S_65, True, False), (S_5000, True, False), (S_5000, False, True), (S_8200, True, False), (S_CTRL, True, False),
               (S_CTRL, False, True)]


def _sid(c):
    return f"B{c.B}-K{c.K0}-{'x'.join(map(str, c.dims))}-p{'_'.join(map(str, c.ps))}-e{c.extras}{'' if c.head_bias else '-nobias'}"


def stack_master(c):
    """The float32 initial state: [Linear, BatchNorm1d, ReLU, Dropout] per width + Linear(., 1), the layout of basic.layers.MLP."""
    torch.manual_seed(c.seed)
    mods, k = [], c.K0
    for w in c.dims:
        mods += [torch.nn.Linear(k, w), torch.nn.BatchNorm1d(w), torch.nn.ReLU(), torch.nn.Dropout(0.0)]
        k = w
    mods.append(torch.nn.Linear(k, 1, bias=c.head_bias))
    net = torch.nn.Sequential(*mods)
    with torch.no_grad():
        for m in net:
            if isinstance(m, torch.nn.BatchNorm1d):
                m.weight.uniform_(0.5, 1.5)
                m.bias.uniform_(-0.5, 0.5)
    return net.train()


def stack_inputs(c):
    g = torch.Generator().manual_seed(1000 + c.seed)
    return (torch.randn(c.B, c.pitch, generator=g), torch.randn(c.B, 1, generator=g), torch.randn(c.B, generator=g),
            torch.randn(c.B, generator=g))


def stack_noise(c):
    return tuple(f"{4 * l}.bias" for l in range(len(c.dims)))  # Linear biases in front of a BatchNorm


@functools.lru_cache(maxsize=None)
def stack_oracle(c, wrong=None):
    """float64 reference of STEPS steps.  wrong: None, "swap" (layers 0 and 1 take each other's counter) or "pitch"."""
    L = len(c.dims)
    ref = copy.deepcopy(stack_master(c)).double().train()
    x, e0, e1, gy = [t.double() for t in stack_inputs(c)]
    x = x[:, :c.K0].clone().requires_grad_()
    e0 = e0.requires_grad_() if c.extras >= 1 else None
    e1 = e1.requires_grad_() if c.extras >= 2 else None
    margin = float("inf")
    for s in range(STEPS):
        a = x
        for l in range(L):
            bn = ref[4 * l + 1](ref[4 * l](a))
            margin = min(margin, float(bn.detach().abs().min()))
            cl = {0: 1, 1: 0}.get(l, l) if wrong == "swap" else l
            keep = layer_keep(C0 + s * L + cl, c.B, c.dims[l], c.ps[l], "pitch" if wrong == "pitch" else None)
            a = torch.relu(bn) * keep / (1.0 - c.ps[l])
        z = ref[4 * L](a).squeeze(1)
        if e0 is not None:
            z = z + e0.squeeze(1)
        if e1 is not None:
            z = z + e1
        y = torch.sigmoid(z)
        y.backward(gy)
    out = _collect(y, x.grad, None if e0 is None else e0.grad, None if e1 is None else e1.grad, ref)
    out["margin"] = margin
    return out


def run_stack(c, monkeypatch, chain, fuse_head_bn=True, gemm_stats=False):
    """STEPS steps of basic.layers.MLP.sigmoid_head on the GPU from the oracle's initial state, through the chosen path."""
    from torch_rechub_amd import ops
    from torch_rechub_amd.basic.layers import MLP
    d, L = dev(), len(c.dims)
    calls = {"chain": 0, "bn": 0}
    real_chain, real_bn = ops.mlp_chain_sigmoid, ops.bn_relu_dropout

    def chain_spy(*a, **k):
        calls["chain"] += 1
        return real_chain(*a, **k)

    def bn_spy(h, bn, p, stats=None, relu=True):
        calls["bn"] += 1
        assert (stats is not None) == gemm_stats, "statistics came from the wrong place"
        return real_bn(h, bn, p, stats=stats, relu=relu)

    monkeypatch.setattr(ops, "mlp_chain_sigmoid", chain_spy)
    monkeypatch.setattr(ops, "bn_relu_dropout", bn_spy)
    monkeypatch.setattr(ops, "FUSE_MLP_CHAIN", chain)
    monkeypatch.setattr(ops, "FUSE_HEAD_BN", fuse_head_bn)
    if gemm_stats:
        monkeypatch.setattr(ops, "_GEMM_MAX_M", 16384)  # the tile GEMM whose epilogue emits the statistics and draws the counter
    mlp = MLP(c.K0, output_layer=True, dims=list(c.dims), dropout=0.0, activation="relu")
    if not c.head_bias:
        mlp.mlp[4 * L] = torch.nn.Linear(c.dims[-1], 1, bias=False)
    mlp.mlp.load_state_dict(stack_master(c).state_dict())
    for l, p in enumerate(c.ps):
        mlp.mlp[4 * l + 3].p = p  # per layer, after construction
    mlp = mlp.to(d).train()
    x, e0, e1, gy = [t.to(d) for t in stack_inputs(c)]
    xbuf = x.requires_grad_()
    extras = [t.requires_grad_() for t in (e0, e1)[:c.extras]]
    ops._dropout_rng(d).copy_(torch.tensor([RNG_SEED, C0, 0, 0], dtype=torch.int64))
    for _ in range(STEPS):
        y = mlp.sigmoid_head(xbuf[:, :c.K0], *extras)  # a row-padded view when pitch > K0, as the fused gather hands over
        if not chain:
            assert (y.grad_fn.bn_node is not None) == fuse_head_bn
        y.backward(gy)
    torch.cuda.synchronize()
    ops.check_errors()
    assert int(ops._dropout_rng(d)[1]) == C0 + STEPS * L, "dropout call counter"
    if chain:
        assert calls == {"chain": STEPS, "bn": 0}, f"the fused chain did not run: {calls}"
    else:
        assert calls == {"chain": 0, "bn": STEPS * L}, f"the layer-by-layer kernels did not run: {calls}"
    assert not xbuf.grad[:, c.K0:].any()
    g = [t.grad for t in extras] + [None, None]
    return _collect(y, xbuf.grad[:, :c.K0], g[0], g[1], mlp.mlp)


def check_stack(c, got, what):
    want = stack_oracle(c)
    assert want["margin"] >= KINK, f"seed {c.seed}: a pre-activation sits {want['margin']:.2e} from the ReLU kink"
    assert_within(compare(got, want, c.B, stack_noise(c)), f"{what} {_sid(c)}")


def check_stack_wrong_masks(c, got, what):
    assert len(c.dims) >= 2 and c.ps[0] > 0 and c.ps[1] > 0
    for wrong in ("swap", "pitch"):
        k, v = worst(compare(got, stack_oracle(c, wrong), c.B, stack_noise(c)))
        print(f"ORACLE {what} {_sid(c)} wrong mask ({wrong}): error / tolerance {v:.0f} ({k})")
        assert v > 100.0, f"{what}: a wrong mask ({wrong}) is only {v:.1f} x the tolerance away"


# --------------------------------------------------------------------------------------------------------------------------
# ops.bn_relu_dropout called directly
Direct = collections.namedtuple("Direct", "B C p relu K seed")  # K: None = h is the input; else h = Linear(K, C)(x), GEMM statistics
D_37 = Direct(37, 32, 0.5, True, None, 1)
D_1000 = Direct(1000, 36, 0.2, True, None, 8)
D_WIDE = Direct(300, 200, 0.2, False, None, 0)       # BatchNorm -> Dropout: no kink
D_WIDE_GEMM = Direct(300, 200, 0.5, False, 33, 0)
D_GEMM = Direct(100, 36, 0.2, True, 33, 6)
D_9000 = Direct(9000, 8, 0.5, True, None, 1)         # three launches
D_CTRL = Direct(1000, 36, 0.0, True, None, 8)        # the p = 0 control
DIRECT_CASES = [D_37, D_1000, D_WIDE, D_WIDE_GEMM, D_GEMM, D_9000, D_CTRL]


def _did(c):
    return f"B{c.B}-C{c.C}-p{c.p}-{'relu' if c.relu else 'bn'}-{'gemm' + str(c.K) if c.K else 'own'}"


def direct_master(c):
    torch.manual_seed(c.seed)
    mods = ([torch.nn.Linear(c.K, c.C)] if c.K else []) + [torch.nn.BatchNorm1d(c.C)]
    with torch.no_grad():
        mods[-1].weight.uniform_(0.5, 1.5)
        mods[-1].bias.uniform_(-0.5, 0.5)
    return torch.nn.Sequential(*mods).train()


def direct_inputs(c):
    g = torch.Generator().manual_seed(1000 + c.seed)
    x = torch.randn(c.B, c.K, generator=g) if c.K else torch.randn(c.B, c.C, generator=g) * 2 + torch.randn(c.C, generator=g) * 1.5
    return x, torch.randn(c.B, c.C, generator=g)


@functools.lru_cache(maxsize=None)
def direct_oracle(c, wrong=None):
    """wrong: None, "late" (call s takes counter c0 + s + 1) or "pitch"."""
    ref = copy.deepcopy(direct_master(c)).double().train()
    x, gy = [t.double() for t in direct_inputs(c)]
    x.requires_grad_()
    margin = float("inf")
    for s in range(STEPS):
        bn = ref(x)
        margin = min(margin, float(bn.detach().abs().min()))
        keep = layer_keep(C0 + s + (1 if wrong == "late" else 0), c.B, c.C, c.p, "pitch" if wrong == "pitch" else None)
        y = (torch.relu(bn) if c.relu else bn) * keep / (1.0 - c.p)
        y.backward(gy)
    out = _collect(y, x.grad, None, None, ref)
    out["margin"] = margin
    return out


def run_direct(c, monkeypatch):
    from torch_rechub_amd import ops
    d = dev()
    if c.K:
        monkeypatch.setattr(ops, "_GEMM_MAX_M", 16384)
    net = copy.deepcopy(direct_master(c)).to(d).train()
    bn = net[-1]
    x, gy = [t.to(d) for t in direct_inputs(c)]
    x.requires_grad_()
    ops._dropout_rng(d).copy_(torch.tensor([RNG_SEED, C0, 0, 0], dtype=torch.int64))
    for _ in range(STEPS):
        if c.K:
            h, stats = ops.linear_stats(x, net[0].weight, net[0].bias, bn)
            assert stats is not None, "the tile GEMM with the statistics epilogue did not run"
        else:
            h, stats = x, None
        y = ops.bn_relu_dropout(h, bn, c.p, stats=stats, relu=c.relu)
        y.backward(gy)
    torch.cuda.synchronize()
    ops.check_errors()
    assert int(ops._dropout_rng(d)[1]) == C0 + STEPS, "dropout call counter"
    return _collect(y, x.grad, None, None, net)


def direct_noise(c):
    return ("0.bias",) if c.K else ()


# --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed,ctr", [(1234, 0), (RNG_SEED, (3 << 32) + 5)])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_host_keep_is_the_device_mask_bit_for_bit(p, seed, ctr):
    from torch_rechub_amd import ops
    n, d = 70001, dev()
    ops._dropout_rng(d).copy_(torch.tensor([seed, ctr, 0, 0], dtype=torch.int64))
    y = ops.dropout(torch.ones(n, device=d), p)
    torch.cuda.synchronize()
    assert int(ops._dropout_rng(d)[1]) == ctr + 1
    got = (y != 0).cpu().numpy()
    want = host_keep(seed, ctr, n, p)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {n} keep flags differ"
    assert abs(want.mean() - (1 - p)) < 5 * (p * (1 - p) / n) ** 0.5, "keep rate"
    np.testing.assert_allclose(y.cpu().numpy()[want], 1.0 / (1.0 - p), rtol=1e-6)


@pytest.mark.parametrize("c", CHAIN_CASES, ids=_sid)
def test_mlp_chain_vs_float64_oracle(c, monkeypatch):
    check_stack(c, run_stack(c, monkeypatch, chain=True), "chain")


@pytest.mark.parametrize("c,fuse_head_bn,gemm_stats", LAYER_CASES,
                         ids=[f"{_sid(c)}-headbn{int(f)}-gemm{int(g)}" for c, f, g in LAYER_CASES])
def test_layer_by_layer_vs_float64_oracle(c, fuse_head_bn, gemm_stats, monkeypatch):
    got = run_stack(c, monkeypatch, chain=False, fuse_head_bn=fuse_head_bn, gemm_stats=gemm_stats)
    check_stack(c, got, f"layers headbn={int(fuse_head_bn)} gemm={int(gemm_stats)}")


@pytest.mark.parametrize("c", DIRECT_CASES, ids=_did)
def test_bn_relu_dropout_vs_float64_oracle(c, monkeypatch):
    got = run_direct(c, monkeypatch)
    want = direct_oracle(c)
    if c.relu:
        assert want["margin"] >= KINK, f"seed {c.seed}: a pre-activation sits {want['margin']:.2e} from the ReLU kink"
    assert_within(compare(got, want, c.B, direct_noise(c)), f"direct {_did(c)}")


S_NEG = S_33._replace(ps=(0.5, 0.3, 0.2))


def test_mlp_chain_misses_an_oracle_with_a_wrong_mask(monkeypatch):
    got = run_stack(S_NEG, monkeypatch, chain=True)
    check_stack(S_NEG, got, "chain")
    check_stack_wrong_masks(S_NEG, got, "chain")


def test_layer_by_layer_misses_an_oracle_with_a_wrong_mask(monkeypatch):
    got = run_stack(S_NEG, monkeypatch, chain=False)
    check_stack(S_NEG, got, "layers")
    check_stack_wrong_masks(S_NEG, got, "layers")


def test_bn_relu_dropout_misses_an_oracle_with_a_wrong_mask(monkeypatch):
    c = D_WIDE
    got = run_direct(c, monkeypatch)
    assert_within(compare(got, direct_oracle(c), c.B), f"direct {_did(c)}")
    for wrong in ("late", "pitch"):
        k, v = worst(compare(got, direct_oracle(c, wrong), c.B))
        print(f"ORACLE direct {_did(c)} wrong mask ({wrong}): error / tolerance {v:.0f} ({k})")
        assert v > 100.0, f"direct: a wrong mask ({wrong}) is only {v:.1f} x the tolerance away"


if __name__ == "__main__":
    # The reference side alone, no GPU: the kink margin of every case for seeds 0..11 (the chosen one marked), and how far a
    # wrong mask moves the oracle itself, in units of the tolerance.
    stacks = sorted(set(CHAIN_CASES + [c for c, _, _ in LAYER_CASES] + [S_NEG]), key=_sid)
    for c in stacks + DIRECT_CASES:
        ident, oracle = (_sid, stack_oracle) if isinstance(c, Stack) else (_did, direct_oracle)
        margins = [oracle(c._replace(seed=s))["margin"] for s in range(12)]
        ok = c.relu if isinstance(c, Direct) else True
        print(f"{ident(c)}: seed {c.seed} margin {margins[c.seed]:.2e}" +
              ("" if not ok or margins[c.seed] >= KINK else "  <-- BELOW THE KINK MARGIN") +
              f"   (seeds 0..11: {' '.join(f'{m:.1e}' for m in margins)}; {sum(m >= KINK for m in margins)} qualify)")
    for c, oracle, wrongs, noise in ((S_NEG, stack_oracle, ("swap", "pitch"), stack_noise(S_NEG)),
                                     (D_WIDE, direct_oracle, ("late", "pitch"), ())):
        for w in wrongs:
            r = compare(oracle(c, w), oracle(c), c.B, noise)
            print(f"wrong mask ({w}) against the right oracle, {c}: {worst(r)[1]:.0f} x the tolerance ({worst(r)[0]})")
