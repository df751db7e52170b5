"""The session kernels (csrc/session.hip: GRU recurrence, additive attention pooling, dropout, session lengths), the
full-catalogue mode of the streaming cross entropy (csrc/stream_ce.hip) and the causal softmax attention of HLLM
(csrc/hllm.hip) against float64 over their supported shape ranges: partly filled GRU workgroups at every sample count, the
register-width switches, second trips of every workgroup-strided loop, the largest shape each guard accepts (and the
refusal one past it), masks with holes, the F.normalize floor at a tiny non-zero sum, every (Sv, R) path of the catalogue
head with its column blocks, tile and chunk edges of the attention, many-partial bias-table sums, the attention's backward
under dropout with the mask recovered from the kernel, and the empty batch.

Bounds.  Every comparison is kernel against float64 with the bound test_gpu_session.py / test_gpu_hllm.py state for that
quantity; where the fp32 arithmetic itself cannot meet it at the larger shapes, the bound is the rule of
test_gpu_hllm.py::test_attention_kernel_against_float64: the larger of the stated bound and 4 x the error of an fp32 torch
evaluation of the same case on the CPU against the same float64 reference.  It never looks at the kernel's output.  Each
comparison prints the largest magnitude, the fp32-CPU error, the kernel's error and the bound used (pytest -s)."""
import copy

import numpy as np
import pytest
import torch

from test_gpu_session import chunked_ce64
from test_hllm_host import np_softmax_attention, np_softmax_attention_bwd, torch_attention
from test_session_host import np_attn_pool, np_attn_pool_bwd, np_catalogue_ce, np_gru, np_gru_bwd
from torch_rechub_amd._lib import H

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def to_np(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)


def compare(case, name, got, want, cpu32, floor, fails, rtol=0.0, scale_min=1e-30):
    """|got - want| <= rtol |want| + max(floor * max(max|want|, scale_min), 4 x the fp32-CPU error), printed as one line of
    the table: | case | tensor | largest magnitude | fp32-CPU error | kernel error | bound |."""
    got, want, cpu32 = (np.asarray(to_np(t), np.float64) for t in (got, want, cpu32))
    assert got.shape == want.shape == cpu32.shape, (name, got.shape, want.shape, cpu32.shape)
    scale = max(float(np.abs(want).max()), scale_min) if want.size else scale_min
    e32 = float(np.abs(cpu32 - want).max()) if want.size else 0.0
    bound = max(floor * scale, 4 * e32)
    err = np.abs(got - want)
    worst = float((err - rtol * np.abs(want)).max()) if want.size else 0.0
    print(f"| {case} | {name} | {scale:.3e} | {e32:.3e} | {float(err.max()) if want.size else 0.0:.3e} | {bound:.3e} |")
    assert np.isfinite(got).all(), f"{case} {name}: not finite"
    if worst > bound:
        fails.append((name, worst, bound))


def poison_small_blocks():
    """NaN through the caching allocator's small-block pool again: buffers of a few floats that an op takes with torch.empty
    inside a test start as NaN, whatever the test itself freed before."""
    junk = [torch.full((n,), float("nan"), device=dev()) for n in (8, 64, 512, 4096) for _ in range(16)]
    del junk


# ---- GRU ----------------------------------------------------------------------------------------------------------------
def gru_samples(B):
    """Samples per workgroup, the rule of csrc/session.hip gru_samples."""
    return min(8, max(1, -(-B // 512)))


GRU_CASES = {
    # name: (B, T, I, H, bias, samples per workgroup): S in 2..8 with a partly empty last workgroup, H at both sides of the
    # 32- and 64-register switches, and a long recurrence
    "S2_H33": (513, 5, 7, 33, True, 2),
    "S3_H64": (1025, 4, 6, 64, False, 3),
    "S7_H65": (3100, 3, 5, 65, True, 7),
    "S8_H32": (4099, 3, 4, 32, False, 8),
    "T300": (7, 300, 3, 20, True, 1),
}
GRU_NAMES = ("weight_ih_l{}", "weight_hh_l{}", "bias_ih_l{}", "bias_hh_l{}")


def gru_float64(cpu, x64, g_out, g_hn=None):
    """(out, h_n, {name: gradient}) of a batch-first nn.GRU in float64: np_gru per layer, np_gru_bwd from the top down."""
    P = {n: t.detach().double().numpy() for n, t in cpu.named_parameters()}
    nl = cpu.num_layers
    par = lambda k: [P.get(n.format(k)) for n in GRU_NAMES]  # noqa: E731
    hs, caches, inp = [], [], x64
    for k in range(nl):
        w_ih, w_hh, b_ih, b_hh = par(k)
        h, cache = np_gru(inp, w_ih, w_hh, b_ih, b_hh)
        hs.append(h)
        caches.append((inp, cache))
        inp = h
    grads = {}
    g = np.array(g_out, np.float64)
    for k in range(nl - 1, -1, -1):
        if g_hn is not None:
            g[:, -1] += g_hn[k]
        w_ih, w_hh, _, _ = par(k)
        xin, cache = caches[k]
        g, dwi, dwh, dbi, dbh = np_gru_bwd(xin, w_ih, w_hh, cache, g)
        for n, v in zip(GRU_NAMES, (dwi, dwh, dbi, dbh)):
            if n.format(k) in P:
                grads[n.format(k)] = v
    grads["x"] = g
    return hs[-1], np.stack([h[:, -1] for h in hs], 0), grads


def gru_on_cpu32(cpu, x, g_out, g_hn=None):
    ref = copy.deepcopy(cpu)
    xc = x.clone().requires_grad_(True)
    out, h_n = ref(xc)
    loss = (out * g_out).sum() if g_hn is None else (out * g_out).sum() + (h_n * g_hn).sum()
    loss.backward()
    grads = {n: p.grad for n, p in ref.named_parameters()}
    grads["x"] = xc.grad
    return out.detach(), h_n.detach(), grads


def gru_on_device(cpu, x, g_out, g_hn=None):
    from torch_rechub_amd import ops
    gru = copy.deepcopy(cpu).to(dev())
    xd = x.to(dev()).requires_grad_(True)
    out, h_n = ops.gru_layers(gru, xd)
    loss = (out * g_out.to(dev())).sum() if g_hn is None else (out * g_out.to(dev())).sum() + (h_n * g_hn.to(dev())).sum()
    loss.backward()
    grads = {n: p.grad for n, p in gru.named_parameters()}
    grads["x"] = xd.grad
    return out.detach(), h_n.detach(), grads


@pytest.mark.parametrize("name", list(GRU_CASES))
def test_gru_shapes_against_float64(name):
    B, T, I, H, bias, S = GRU_CASES[name]
    assert gru_samples(B) == S
    torch.manual_seed(B + T + H)
    cpu = torch.nn.GRU(I, H, batch_first=True, bias=bias)
    x = 0.5 * torch.randn(B, T, I)
    g = torch.randn(B, T, H)
    want, want_hn, wg = gru_float64(cpu, x.double().numpy(), g.numpy())
    c_out, _, cg = gru_on_cpu32(cpu, x, g)
    out, h_n, grads = gru_on_device(cpu, x, g)
    fails = []
    compare(name, "h_all", out, want, c_out, 2e-5, fails)
    assert torch.equal(h_n[0], out[:, -1])
    assert set(grads) == set(wg)
    for n in sorted(wg):
        compare(name, "d " + n, grads[n], wg[n], cg[n], 1e-4, fails)
    assert not fails, fails
    if S > 1:
        tail = B % S  # the last workgroup holds `tail` samples and S - tail empty slots
        assert 0 < tail < S
        assert torch.isfinite(out[B - tail:]).all() and torch.isfinite(grads["x"][B - tail:]).all()
        assert float(out[B - tail:].abs().max()) > 0 and float(grads["x"][B - tail:].abs().max()) > 0
        again = gru_on_device(cpu, x, g)[2]
        for n in grads:
            assert torch.equal(grads[n], again[n]), n


def test_gru_two_layers_biased_batch_first_forward_and_backward_against_float64():
    """Two stacked layers with all four biases; the loss reads the output AND h_n, so both layers' last states carry a
    gradient of their own."""
    B, T, I, H = 70, 12, 9, 24
    torch.manual_seed(21)
    cpu = torch.nn.GRU(I, H, num_layers=2, batch_first=True, bias=True)
    x = 0.5 * torch.randn(B, T, I)
    g, g_hn = torch.randn(B, T, H), torch.randn(2, B, H)
    want, want_hn, wg = gru_float64(cpu, x.double().numpy(), g.numpy(), g_hn.double().numpy())
    c_out, c_hn, cg = gru_on_cpu32(cpu, x, g, g_hn)
    out, h_n, grads = gru_on_device(cpu, x, g, g_hn)
    fails = []
    compare("2layers", "output", out, want, c_out, 2e-5, fails)
    compare("2layers", "h_n", h_n, want_hn, c_hn, 2e-5, fails)
    assert len(wg) == 9 and set(grads) == set(wg)
    for n in sorted(wg):
        compare("2layers", "d " + n, grads[n], wg[n], cg[n], 1e-4, fails)
    assert not fails, fails


# ---- additive attention pooling -------------------------------------------------------------------------------------------
def torch_pool(P, r, w0, mask, X, add, floor):
    """The pooling in torch (any dtype) for autograd on the CPU; clamp_min passes no gradient below the floor, as
    F.normalize's denominator."""
    e = torch.exp(torch.sigmoid(P + r[:, None]) @ w0) * mask
    tot = e.sum(1, keepdim=True)
    a = e / (tot.clamp_min(1e-12) if floor else tot)
    return torch.bmm(a[:, None, :], X)[:, 0] + (0 if add is None else add)


def holes_mask(B, L, g):
    """Row 0 full, row 1 a single kept position, the others random with holes (and at least one kept position)."""
    mask = torch.rand(B, L, generator=g) < 0.7
    mask[0] = True
    if B > 1:
        mask[1] = False
        mask[1, L // 3] = True
    for b in range(2, B):
        mask[b, (7 * b) % L] = True
    return mask


def run_pool_case(case, P, r, w0, mask, X, A, floor, gy, floors=(2e-6, 2e-5)):
    from torch_rechub_amd import ops
    ts = [t.to(dev()).requires_grad_(True) for t in (P, r, w0, X)]
    out = ops.additive_attention_pool(ts[0], ts[1], ts[2], mask.to(dev()), ts[3], None if A is None else A.to(dev()),
                                      floor=floor)
    out.backward(gy.to(dev()))
    args64 = [t.double().numpy() for t in (P, r, w0)]
    want, cache = np_attn_pool(*args64, mask.double().numpy(), X.double().numpy(), None if A is None else A.double().numpy(),
                               floor)
    refs = np_attn_pool_bwd(*args64, X.double().numpy(), cache, gy.double().numpy(), floor)
    cs = [t.clone().requires_grad_(True) for t in (P, r, w0, X)]
    c_out = torch_pool(cs[0], cs[1], cs[2], mask.float(), cs[3], A, floor)
    c_out.backward(gy)
    fails = []
    compare(case, "out", out, want, c_out.detach(), floors[0], fails)
    for t, ref, c, name in zip(ts, refs, cs, ("dP", "dr", "dw0", "dX")):
        compare(case, name, t.grad, ref, c.grad, floors[1], fails)
    assert not fails, fails
    return out.detach(), [t.grad for t in ts], cache


# (B, L, H, Dx, floor): L, H and Dx each past one trip of its 256-wide loop, alone and together, up to the guard's largest
POOL_SHAPES = {
    "L257_H257_D257": (3, 257, 257, 257, False),
    "L1024_H40_D257": (4, 1024, 40, 257, True),
    "L50_H4096_D30": (3, 50, 4096, 30, False),
    "L20_H30_D4096": (3, 20, 30, 4096, True),
    "guard_L1024_H4096_D4096": (2, H.RH_ATTN_POOL_MAX_L, H.RH_ATTN_POOL_MAX_W, H.RH_ATTN_POOL_MAX_W, False),
}


@pytest.mark.parametrize("add", [False, True])
@pytest.mark.parametrize("name", list(POOL_SHAPES))
def test_attention_pool_shapes_against_float64(name, add):
    B, L, H, Dx, floor = POOL_SHAPES[name]
    g = torch.Generator().manual_seed(B + L + H + Dx + add)
    P = torch.randn(B, L, H, generator=g)
    r = torch.randn(B, H, generator=g)
    w0 = 0.3 * min(1.0, (128 / H)**0.5) * torch.randn(H, generator=g)  # keeps s_l of the size the model shapes give
    X = torch.randn(B, L, Dx, generator=g)
    A = torch.randn(B, Dx, generator=g) if add else None
    mask = holes_mask(B, L, g)
    assert mask.any(1).all() and mask[0].all() and int(mask[1].sum()) == 1 and (B == 2 or not mask[2:].all())
    gy = torch.randn(B, Dx, generator=g)
    out, grads, _ = run_pool_case(f"{name}{'_add' if add else ''}", P, r, w0, mask, X, A, floor, gy)
    dX = grads[3]
    assert not dX[~mask.to(dev())].any()  # a masked position takes no weight: its dX row is exactly zero


def test_attention_pool_floor_with_tiny_nonzero_sums():
    """F.normalize's floor with row sums between 1e-13 and 1e-12: the weights are e / 1e-12 and the denominator passes no
    gradient (np_attn_pool_bwd's ``tot < 1e-12`` branch), although the sum is not zero.  s_l runs from about -30.5 (row
    sum ~5e-13, the weights sum to ~0.5: treating the denominator as the sum would change d s by that fraction) down to
    about -50 (exp still a normal fp32 number)."""
    B, L, H, Dx = 16, 8, 16, 12
    g = torch.Generator().manual_seed(77)
    target = torch.linspace(30.5, 50.0, B)
    w0 = -(50.0 / H) * (1 + 0.02 * torch.randn(H, generator=g))
    r = torch.logit(target / 50.0 * 0.999)[:, None] + 0.02 * torch.randn(B, H, generator=g)
    P = 0.05 * torch.randn(B, L, H, generator=g)
    X = torch.randn(B, L, Dx, generator=g)
    mask = holes_mask(B, L, g)
    gy = torch.randn(B, Dx, generator=g)
    _, _, cache = run_pool_case("floor_tiny", P, r, w0, mask, X, None, True, gy)
    sg, e, tot, den, a = cache
    assert tot.min() > 0 and tot.max() < 0.9e-12 and tot.max() > 1e-13, (tot.min(), tot.max())
    assert (den == 1e-12).all()
    kept = e[mask.numpy()]
    assert kept.min() > 1e-30 and kept.max() < 1e-12  # normal fp32 numbers, none flushed


def test_attention_pool_mask_dtypes_give_identical_bits():
    from torch_rechub_amd import ops
    B, L, H, Dx = 9, 21, 13, 17
    g = torch.Generator().manual_seed(5)
    base = [torch.randn(B, L, H, generator=g), torch.randn(B, H, generator=g), 0.3 * torch.randn(H, generator=g),
            torch.randn(B, L, Dx, generator=g)]
    mask = holes_mask(B, L, g)
    gy = torch.randn(B, Dx, generator=g).to(dev())
    runs = []
    for m in (mask, mask.to(torch.int32), mask.to(torch.float32)):
        ts = [t.to(dev()).requires_grad_(True) for t in base]
        out = ops.additive_attention_pool(ts[0], ts[1], ts[2], m.to(dev()), ts[3])
        out.backward(gy)
        runs.append([out.detach()] + [t.grad for t in ts])
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a, b)


# ---- the empty batch ------------------------------------------------------------------------------------------------------
def test_empty_batch_through_the_attention_pool_leaves_a_zero_w0_gradient():
    from torch_rechub_amd import ops
    L, H, Dx = 6, 5, 7
    P = torch.zeros(0, L, H, device=dev(), requires_grad=True)
    r = torch.zeros(0, H, device=dev(), requires_grad=True)
    w0 = torch.randn(H, device=dev(), requires_grad=True)
    X = torch.zeros(0, L, Dx, device=dev(), requires_grad=True)
    for floor in (False, True):
        out = ops.additive_attention_pool(P, r, w0, torch.zeros(0, L, dtype=torch.bool, device=dev()), X,
                                          torch.zeros(0, Dx, device=dev()), floor=floor)
        assert out.shape == (0, Dx)
        w0.grad = None
        poison_small_blocks()
        out.sum().backward()
        assert w0.grad is not None and w0.grad.shape == (H,) and torch.all(w0.grad == 0), w0.grad
    assert P.grad.shape == P.shape and r.grad.shape == r.shape and X.grad.shape == X.shape
    ops.check_errors()


def test_empty_batch_through_gru_dropout_lengths_and_the_catalogue_refusal():
    from torch_rechub_amd import ops
    for bf in (True, False):
        gru = torch.nn.GRU(5, 7, num_layers=2, batch_first=bf).to(dev())
        x = torch.zeros((0, 4, 5) if bf else (4, 0, 5), device=dev(), requires_grad=True)
        poison_small_blocks()
        out, h_n = ops.gru_layers(gru, x)
        assert out.shape == ((0, 4, 7) if bf else (4, 0, 7)) and h_n.shape == (2, 0, 7)
        (out.sum() + h_n.sum()).backward()
        assert x.grad.shape == x.shape
        for n, p in gru.named_parameters():
            assert p.grad is not None and torch.all(p.grad == 0), n
    x = torch.zeros(0, 8, device=dev(), requires_grad=True)
    rng = ops._dropout_rng(dev())
    ctr = int(rng[1])
    y = ops.dropout(x, 0.3)
    assert y.shape == (0, 8) and int(rng[1]) == ctr + 1
    y.sum().backward()
    assert x.grad.shape == (0, 8)
    for check_full in (False, True):
        counts = ops.session_lengths(torch.zeros(0, 5, dtype=torch.int64, device=dev()), check_full=check_full)
        assert counts.shape == (0,) and counts.dtype == torch.int64
    with pytest.raises(RuntimeError, match="B >= 1"):
        ops.catalogue_cross_entropy(torch.zeros(0, 8, device=dev()), torch.zeros(10, 8, device=dev()),
                                    torch.zeros(0, dtype=torch.int64, device=dev()))
    ops.check_errors()


# ---- dropout and session lengths --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.25, 0.5])
def test_dropout_grid_stride_loop_with_an_odd_tail(p):
    """n = 5 000 003 > 8192 workgroups x 256: the grid-stride loop takes a second and a partial third trip."""
    from torch_rechub_amd import ops
    n = 5000003
    assert n > 2 * 8192 * 256 and n % 256 != 0
    x = (torch.rand(n, device=dev()) + 0.5).requires_grad_(True)  # no zero: y != 0 marks the kept ones
    y = ops.dropout(x, p)
    keep = y != 0
    scale = torch.tensor(1.0, device=dev()) / (1 - torch.tensor(p, device=dev()))  # 1 / (1 - p) in float32
    assert torch.equal(y[keep], x.detach()[keep] * scale)
    frac = float(keep.double().mean())
    bound = 5 * (p * (1 - p) / n)**0.5  # five standard deviations of the binomial mean
    assert abs(frac - (1 - p)) <= bound, (frac, bound)
    # no period of the grid (8192 x 256 elements) in the mask: the hash reads the element index, not the thread's
    stride = 8192 * 256
    assert not torch.equal(keep[:stride], keep[stride:2 * stride])
    g = torch.randn(n, device=dev())
    y.backward(g)
    assert torch.equal(x.grad, torch.where(keep, g * scale, torch.zeros_like(g)))  # the forward's mask, recomputed


def _lengths_seq(B, L, seed):
    g = torch.Generator().manual_seed(seed)
    seq = torch.randint(1, 1000, (B, L), generator=g)
    seq[torch.rand(B, L, generator=g) < 0.4] = 0  # holes anywhere: the count is of non-zero ids, not a prefix length
    seq[:, 0] = torch.randint(1, 1000, (B,), generator=g)  # no empty row
    return seq


@pytest.mark.parametrize("L", [1, 19, 1024])
def test_session_lengths_over_many_rows(L):
    from torch_rechub_amd import ops
    B = 5000
    seq = _lengths_seq(B, L, L)
    if L > 1:
        seq[0, 1] = 0  # ... and row 0 not full
    want = (seq != 0).sum(1)
    assert int(want.min()) >= 1
    counts = ops.session_lengths(seq.to(dev()))
    assert counts.dtype == torch.int64 and torch.equal(counts.cpu(), want)
    assert torch.equal(ops.session_lengths(seq.to(torch.int32).to(dev())).cpu(), want)
    # the only empty row at an index above 256 (thread 225's second trip)
    empty = seq.clone()
    empty[4321] = 0
    with pytest.raises(RuntimeError, match="greater than 0"):
        ops.session_lengths(empty.to(dev()))
    ops.check_errors()  # the word was cleared
    if L > 1:
        # check_full: the only full row above 256 passes, no full row raises
        full = seq.clone()
        full[full.all(1)] = torch.cat([torch.ones(L - 1, dtype=seq.dtype), torch.zeros(1, dtype=seq.dtype)])
        assert int((full != 0).sum(1).max()) < L
        with pytest.raises(RuntimeError, match="shorter than its padded length"):
            ops.session_lengths(full.to(dev()), check_full=True)
        ops.check_errors()
        full[4000] = 7
        got = ops.session_lengths(full.to(dev()), check_full=True)
        assert torch.equal(got.cpu(), (full != 0).sum(1)) and int(got[4000]) == L


# ---- full-catalogue cross entropy -------------------------------------------------------------------------------------------
CE_CASES = [
    # (B, D, V, Sv of the dh kernel, R of the dW kernel): Sv > 1 writes (Sv, B, D) partials, R > 1 (V, D + 1) slabs; D > 256
    # adds column blocks (blockIdx.y > 0) to both
    (1, 1, 2, 1, 1),
    (63, 256, 63, 1, 1),
    (64, 257, 64, 1, 1),          # D > 256, direct dh and direct dW
    (65, 600, 65, 2, 2),          # D > 256 with dh partials and dW slabs
    (1, 600, 4097, 64, 1),        # D > 256, Sv = 64, direct dW
    (63, 257, 4097, 64, 1),
    (65, 1, 4097, 64, 2),
    (64, 256, 4097, 64, 1),
    (5000, 257, 4097, 8, 8),
    (16400, 1000, 130, 1, 32),    # Sv = 1 over three V tiles: 257 row tiles x 4 column blocks fill the chip alone
]


def test_ce_case_table_covers_every_path():
    Bs, Ds, Vs = ({c[i] for c in CE_CASES} for i in range(3))
    assert {1, 256, 257, 600} <= Ds and {1, 63, 64, 65} <= Bs and {63, 64, 65, 4097} <= Vs
    assert any(sv > 1 and D > 256 for _, D, _, sv, _ in CE_CASES)
    assert any(sv == 1 and V > 128 for _, _, V, sv, _ in CE_CASES)
    assert any(R == 1 and D > 256 for _, D, _, _, R in CE_CASES) and any(R > 1 and D > 256 for _, D, _, _, R in CE_CASES)


def ce_inputs(B, D, V, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(B, D, generator=g)
    E = 0.1 * torch.randn(V, D, generator=g)
    labels = torch.randint(0, V, (B,), generator=g)
    labels[0] = 0
    labels[-1] = V - 1
    return u, E, labels


def ce_float64(u, E, labels):
    """(loss, du, dE) in float64: the numpy restatement, or its V-chunked form on the device for the large cases."""
    if u.shape[0] * E.shape[0] <= 1 << 21:
        return np_catalogue_ce(u.double().numpy(), E.double().numpy(), labels.numpy())
    loss, du, dE = chunked_ce64(u.to(dev()), E.to(dev()), labels.to(dev()))
    return loss, du.cpu().numpy(), dE.cpu().numpy()


def run_ce_case(case, u, E, labels, upstream=1.0, label_dtype=torch.int64):
    """-> (u.grad, E.grad) on the device, after the comparison with float64."""
    from torch_rechub_amd import ops
    ud, Ed = u.to(dev()).requires_grad_(True), E.to(dev()).requires_grad_(True)
    loss = ops.catalogue_cross_entropy(ud, Ed, labels.to(label_dtype).to(dev()))
    (upstream * loss).backward()
    ops.check_errors()
    want, du, dE = ce_float64(u, E, labels)
    cu, cE = u.clone().requires_grad_(True), E.clone().requires_grad_(True)
    closs = torch.nn.functional.cross_entropy(cu @ cE.T, labels)
    (upstream * closs).backward()
    fails = []
    compare(case, "loss", loss.detach().reshape(1) * upstream, np.array([upstream * want]), closs.detach().reshape(1) * upstream,
            2e-5, fails, scale_min=1.0)
    compare(case, "du", ud.grad, upstream * du, cu.grad, 2e-5, fails)
    compare(case, "dE", Ed.grad, upstream * dE, cE.grad, 2e-5, fails)
    assert not fails, fails
    return ud.grad, Ed.grad


@pytest.mark.parametrize("B,D,V,Sv,R", CE_CASES)
def test_catalogue_ce_paths_against_float64(B, D, V, Sv, R):
    from torch_rechub_amd import _lib
    assert _lib.call("rh_catalogue_ce_vsplit", B, D, V) == Sv
    assert _lib.call("rh_hstu_head_rsplit", B, D, V) == R
    assert 1 <= _lib.call("rh_hstu_head_nsplit", B, V) <= max(1, -(-V // 64))
    u, E, labels = ce_inputs(B, D, V, seed=B + D + V)
    gu, gE = run_ce_case(f"ce_{B}_{D}_{V}", u, E, labels)
    if V >= 4097:  # bitwise repeatable
        gu2, gE2 = run_ce_case(f"ce_{B}_{D}_{V} again", u, E, labels)
        assert torch.equal(gu, gu2) and torch.equal(gE, gE2)


def test_catalogue_ce_with_logits_near_plus_and_minus_80():
    """Rows of u scaled along an item's vector so that one logit reaches +80 (rows 0..3) or -80 (rows 4..7): the running
    maximum of the online softmax jumps by tens of units between V tiles and splits."""
    B, D, V = 70, 24, 5000
    u, E, labels = ce_inputs(B, D, V, seed=9)
    items = torch.tensor([4999, 70, 2500, 64, 0, 63, 4097, 1234])
    for row, item in enumerate(items):
        u[row] = (80.0 if row < 4 else -80.0) * E[item] / (E[item] @ E[item])
    labels[1], labels[5] = 70, 63  # the spike as the label once, the dip as the label once
    z = u.double() @ E.double().T
    assert 79.9 < float(z[:4].max()) < 80.1 and -80.1 < float(z[4:8].min()) < -79.9
    run_ce_case("ce_logits_80", u, E, labels)


def test_catalogue_ce_upstream_gradient_and_int32_labels():
    u, E, labels = ce_inputs(65, 600, 65, seed=4)
    run_ce_case("ce_3x_loss", u, E, labels, upstream=3.0)
    run_ce_case("ce_int32_labels", u, E, labels, label_dtype=torch.int32)
    u, E, labels = ce_inputs(63, 257, 4097, seed=5)
    run_ce_case("ce_3x_loss_Sv64", u, E, labels, upstream=3.0)


def test_catalogue_ce_negative_label_sets_the_error_word():
    from torch_rechub_amd import ops
    u, E, labels = ce_inputs(70, 12, 300, seed=2)
    labels[66] = -1
    ops.check_errors()
    ops.catalogue_cross_entropy(u.to(dev()), E.to(dev()), labels.to(dev()))
    with pytest.raises(IndexError, match="target label"):
        ops.check_errors()
    ops.check_errors()  # the word was cleared


# ---- HLLM attention ---------------------------------------------------------------------------------------------------------
def attn_inputs(B, L, H, dh, nb, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, L, 3 * H * dh, generator=g)
    table = 0.5 * torch.randn(nb, H, generator=g) if nb else None
    gout = torch.randn(B, L, H * dh, generator=g)
    return qkv, table, gout


def run_attn(qkv, table, gout, H, N, strided, p=0.0, scale=None):
    """-> out, g_q, g_k, g_v, g_table on the CPU.  strided: q, k, v are column blocks of ONE (B, L, 3 W) tensor."""
    from torch_rechub_amd import ops
    W = qkv.shape[2] // 3
    tt = table.to(dev()).requires_grad_(True) if table is not None else None
    if strided:
        x = qkv.to(dev()).requires_grad_(True)
        q, k, v = x[..., :W], x[..., W:2 * W], x[..., 2 * W:]
    else:
        q, k, v = (qkv[..., i * W:(i + 1) * W].contiguous().to(dev()).requires_grad_(True) for i in range(3))
    out = ops.softmax_attention(q, k, v, H, N, bias_table=tt, dropout_p=p, scale=scale)
    out.backward(gout.to(dev()))
    if strided:
        gq, gk, gv = (x.grad[..., i * W:(i + 1) * W].cpu() for i in range(3))
    else:
        gq, gk, gv = q.grad.cpu(), k.grad.cpu(), v.grad.cpu()
    return out.detach().cpu(), gq, gk, gv, None if tt is None else tt.grad.cpu()


def check_attn(case, qkv, table, gout, H, N, strided, p=0.0, scale=None, keep=None):
    """The kernel against np_softmax_attention(keep=...) under the rule of test_attention_kernel_against_float64: rtol 1e-4
    and a floor of 2e-6 (1e-4 for the table's gradient) of the largest magnitude, or 4 x the fp32-CPU error."""
    B, L, W3 = qkv.shape
    W = W3 // 3
    dh = W // H
    q, k, v = (qkv[..., i * W:(i + 1) * W] for i in range(3))
    ref, cache = np_softmax_attention(q.numpy(), k.numpy(), v.numpy(), H, N, None if table is None else table.numpy(),
                                      scale=scale, keep=keep)
    wants = (ref,) + np_softmax_attention_bwd(cache, gout.numpy())
    cq, ck, cv = (t.clone().requires_grad_(True) for t in (q, k, v))
    ct = table.clone().requires_grad_(True) if table is not None else None
    f = 1.0 if scale is None else scale / dh**-0.5  # torch_attention scales by dh^-0.5: fold the rest into q
    co = torch_attention(cq * f, ck, cv, H, N, ct, None if keep is None else torch.from_numpy(keep).float())
    co.backward(gout)
    cpu32 = (co.detach(), cq.grad, ck.grad, cv.grad, None if ct is None else ct.grad)
    gots = run_attn(qkv, table, gout, H, N, strided, p=p, scale=scale)
    fails = []
    for name, got, want, c32 in zip(("out", "g_q", "g_k", "g_v", "g_table"), gots, wants, cpu32):
        if want is None:
            assert got is None
            continue
        compare(case, name, got, want, c32, 1e-4 if name == "g_table" else 2e-6, fails, rtol=1e-4)
    assert not fails, fails
    return gots


ATTN_CASES = {
    # name: (B, L, H, dh, max_seq_len, num_buckets (0: no bias), strided, scale): L at both sides of the 64-row tile edges,
    # dh at both sides of the 64-column chunk edge and below 128
    "L63_dh63": (2, 63, 2, 63, 63, 32, False, None),
    "L64_dh65": (2, 64, 3, 65, 64, 32, True, None),
    "L65_dh127": (2, 65, 2, 127, 65, 16, False, None),
    "L127_dh63": (2, 127, 1, 63, 127, 32, True, None),
    "L128_dh65_nobias": (2, 128, 2, 65, 128, 0, False, None),
    "L129_dh127": (2, 129, 2, 127, 129, 32, True, None),
    "L65_N1000_nb1500": (2, 65, 2, 16, 1000, 1500, False, None),   # buckets 0, 1, 2, 4, 5, ...: most table rows untouched
    "L129_scale": (2, 129, 2, 33, 129, 32, False, 0.37),
    "guard_L1024_dh128_nb1024": (1, H.RH_ATTN_MAX_L, 1, H.RH_ATTN_MAX_DH, H.RH_ATTN_MAX_L, 1024, False, None),
}


@pytest.mark.parametrize("name", list(ATTN_CASES))
def test_attention_edges_against_float64(name):
    B, L, H, dh, N, nb, strided, scale = ATTN_CASES[name]
    qkv, table, gout = attn_inputs(B, L, H, dh, nb, seed=L + H + dh)
    gots = check_attn(name, qkv, table, gout, H, N, strided, scale=scale)
    if nb > N:  # rows of the table no (i, j) reaches take exactly zero
        used = np.unique(np.minimum(np.arange(L), N) * (nb - 1) // N)
        rest = np.setdiff1d(np.arange(nb), used)
        assert len(rest) > 0 and not gots[4].numpy()[rest].any()


def test_attention_table_gradient_over_six_thousand_partials():
    from torch_rechub_amd import _lib
    B, L, H, dh, nb = 250, 129, 8, 4, 32
    assert B * H >= 2000 and _lib.call("rh_softmax_attn_nparts", B, L, H) >= 6000
    qkv, table, gout = attn_inputs(B, L, H, dh, nb, seed=31)
    first = check_attn("partials_6008", qkv, table, gout, H, L, False)
    again = run_attn(qkv, table, gout, H, L, False)
    for a, b in zip(first, again):
        assert torch.equal(a, b)


def test_attention_guard_refuses_one_past_each_limit():
    """L = 1024, dh = 128, num_buckets = 1024 runs (test_attention_edges_against_float64[guard_L1024_dh128_nb1024]); one past
    each limit is refused from the Python side, before any launch."""
    from torch_rechub_amd import ops

    def run(L, dh, N, p=0.0, nb=8):
        x = torch.zeros(1, L, dh, device=dev())
        return ops.softmax_attention(x, x, x, 1, N, bias_table=torch.zeros(nb, 1, device=dev()), dropout_p=p)

    assert run(8, 128, 8).shape == (1, 8, 128)
    for args in ((1025, 8, 1025), (8, 129, 8), (9, 8, 8), (8, 8, 8, 1.0)):
        with pytest.raises(RuntimeError, match="no HIP kernel"):
            run(*args)
    ops.check_errors()


def recover_keep(B, L, H, p, state0):
    """The dropout multipliers (B, H, L, L) the attention kernels draw at the (seed, counter) state ``state0``, read from the
    forward itself: q = k = 0 without a bias makes every causal weight exactly 1 / (i + 1), and v = one-hot rows of a
    128-key chunk copies the dropped weights of those keys into the output.  The mask depends on (seed, counter, b, h, i, j)
    alone, not on the head width or the values.  Leaves the state at ``state0``."""
    from torch_rechub_amd import ops
    rng = ops._dropout_rng(dev())
    dp = min(L, 128)
    z = torch.zeros(B, L, H * dp, device=dev())
    keep = np.zeros((B, H, L, L))
    rows = torch.arange(L, device=dev())
    n_kept = n_all = 0
    for c0 in range(0, L, 128):
        cols = torch.arange(c0, min(L, c0 + 128), device=dev())
        v = torch.zeros(B, L, H, dp, device=dev())
        v[:, cols, :, cols - c0] = 1.0
        v = v.view(B, L, H * dp)
        pick = lambda o: o.view(B, L, H, dp)[..., :len(cols)].permute(0, 2, 1, 3)  # noqa: E731  (B, H, queries, keys)
        rng.copy_(state0)
        w0 = pick(ops.softmax_attention(z, z, v, H, L))
        assert torch.equal(rng, state0)  # p = 0 draws nothing
        wd = pick(ops.softmax_attention(z, z, v, H, L, dropout_p=p))
        assert int(rng[1]) == int(state0[1]) + 1
        causal = (cols[None, :] <= rows[:, None])[None, None].expand(B, H, L, len(cols))
        # every causal weight before dropout is non-zero (and nothing else is): a zero in wd is a dropped weight
        assert torch.all(w0[causal] > 0) and not w0[~causal].any() and not wd[~causal].any()
        kept = (wd != 0) & causal
        np.testing.assert_allclose(wd[kept].cpu().numpy(), (w0[kept] / (1 - p)).cpu().numpy(), rtol=2e-6, atol=0)
        keep[..., c0:c0 + len(cols)] = kept.cpu().numpy() / (1 - p)
        n_kept += int(kept.sum())
        n_all += int(causal.sum())
    rng.copy_(state0)
    assert n_all == B * H * L * (L + 1) // 2
    bound = 5 * (p * (1 - p) / n_all)**0.5  # five standard deviations of the binomial mean
    assert abs(n_kept / n_all - (1 - p)) <= bound, (n_kept / n_all, bound)
    return keep


@pytest.mark.parametrize("strided", [False, True])
@pytest.mark.parametrize("L,dh", [(65, 33), (200, 128), (129, 64)])
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_attention_with_dropout_forward_and_backward_against_float64(p, L, dh, strided):
    from torch_rechub_amd import ops
    B, H, nb = 2, 3, 32
    rng = ops._dropout_rng(dev())
    state0 = rng.clone()
    keep = recover_keep(B, L, H, p, state0)
    assert torch.equal(rng, state0)
    qkv, table, gout = attn_inputs(B, L, H, dh, nb, seed=L + dh + strided)
    check_attn(f"drop_p{p}_L{L}_dh{dh}_{'strided' if strided else 'contig'}", qkv, table, gout, H, L, strided, p=p, keep=keep)
    assert int(rng[1]) == int(state0[1]) + 1 and int(rng[0]) == int(state0[0])
