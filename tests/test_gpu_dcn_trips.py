"""The DCN / DCN-v2 kernels (csrc/cross.hip, csrc/crossmix.hip, csrc/moe.hip) past their launch caps, against float64.

Every kernel in the three files is a grid-stride loop under a capped grid; past the cap a workgroup makes a second trip that
reuses its registers, its LDS staging and (the mid backward) a prefetched operand.  Each case below asks the library for the
grid of the launch it is about -- the query is the function the launch itself calls -- and asserts, before it compares
anything, that the shape is past the cap (work units > grid, the grid at its cap) with a ragged tail (work units not a
multiple of the grid).  A work unit is what one workgroup takes per trip: four rows (cross forward, mix epilogue), 1024
elements (v2 epilogue: four per thread), 256 / (E r) samples (mid kernels), 256 elements (residual backward, pack, unpack).

References: oracle/ctr_oracle.py (CrossNetwork), the float64 autograd expressions of
test_gpu_kernels.py::test_cross_mix_and_v2_epilogues_vs_reference_formula (epilogues) and
test_gpu_kernels.py::_cross_net_mix_reference (CrossNetMix end to end: output, g_x and the gradients of U, V, C, bias and the
gating weights).  Tolerances are the ones those tests use for the same quantities, |got - want| <= atol + rtol |want|:
  CrossNetMix       out rtol 2e-5, atol 2e-6 max(1, max|want|);  gradients rtol 1e-4, atol 1e-5 max(1, max|want|)
  CrossNetwork      out 2e-5 / 2e-6;  g_x, g_w, g_b 1e-4 / 1e-5
  mix epilogue      out 2e-5 / 2e-6;  gradients 1e-4 / 1e-5
  v2 epilogue       out 1e-6 / 1e-6;  gradients 2e-5 / 2e-6
No bound was widened and no element is excluded.  The weight gradients here sum up to 20485 rows in float32; float32 eager
torch on the CPU through the same comparison (``python tests/test_gpu_dcn_trips.py``) stays at or below 0.10 of the tolerance
on every CrossNetMix case but pack / unpack (0.60, the gating gradient at d = 1025 and B = 9), so the bounds above hold for
these shapes as they are.

Cases (caps as the queries answer today; B is derived from the queries, the figures in brackets are today's):
  CrossNetwork      cap 2048 workgroups = 8192 rows per trip.  B = one trip + 5 [8197]: 2 trips, 2 workgroups in the second.
                    d = 5, L = 1 (EPL 1) strided x;  d = 130, L = 3 (EPL 4, lanes 2..63 of the third 64-element group empty)
  v2 epilogue       cap 4096 workgroups x 1024 elements.  d = 1027, B = cap 1024 / d + 16 [4100 x 1027: 4113 units, 2 trips]
  mix epilogue      cap 4096 workgroups = 16384 rows.  B = one trip + 3 [16387], d = 8, E in {1, 3}
  mid, 1 per group  forward cap 2048 groups, backward cap 512.  B = 2 x forward cap + 3 [4099], d = 8, L = 1: 3 forward trips,
                    9 backward trips, a 3-group tail.  (E, r) = (4, 64), (16, 16)
  mid, 10 per group E = 3, r = 8.  B = backward cap x 10 + 3 [5123], d = 8: 513 groups, the last one with 3 of 10 samples;
                    B = forward cap x 10 + 5 [20485], d = 5: 2049 groups forward, 5 backward trips
  lane layouts      B in {37, samples per group - 1, + 1}, d = 6, L = 2: (E, r) = (5, 16) 80 threads per sample, 16 idle
                    lanes, KP = 88; (3, 32) a whole idle wavefront; (1, 64); (16, 4) KP = 80.  (under every cap by design:
                    asserted is the number of samples per group, through the backward's grid)
  g_C partial sum   E = 4, r = 64, d = 4, L = 1, B in {28, 29, 32, 33, 36, 61} = the number of partials (asserted): the
                    8-in-flight loop of a wavefront w runs once iff B > w + 28, twice iff B > w + 60
  residual backward cap 4096 workgroups x 256 elements.  d = 257, B = cap 256 / d + 19 [4099 x 257: 4116 units], E = 2, r = 4
                    (mid kernels under their caps, asserted), L in {1, 2, 3} = modes {3}, {1, 2}, {1, 0, 2}, strided x
  pack / unpack     cap 2048 workgroups x 256 elements each.  L = 2, E = 4, r = 64, B = 9, d = cap 256 / (L KP) + 17
                    [1025: pack 4165 units, unpack 4124 units, 3 trips each]
  large logits      E = 4, r = 8, d = 8, B = 64, gating weights x 60: the float64 logits span more than +-100 (asserted)
  repeatability     the 4099-row (4, 64) case backward twice: every gradient bitwise equal (no atomics)

Worst error / tolerance per case on the MI355X (the ``TRIPS`` lines each test prints; the worst quantity in brackets), every
case measured:
  CrossNetwork      d = 5: 0.013 [out];  d = 130: 0.018 [out]
  v2 epilogue       0.081 [g_b]
  mix epilogue      E = 1: 0.008 [out];  E = 3: 0.013 [out]
  mid, 1 per group  (4, 64): 0.023 [g_gating];  (16, 16): 0.022 [g_gating]
  mid, 10 per group B = 5123: 0.016 [g_C];  B = 20485: 0.054 [out]
  lane layouts      (5, 16): 0.013;  (3, 32): 0.011;  (1, 64): 0.010;  (16, 4): 0.043 [out, B = 3]
  g_C partial sum   0.007, 0.008, 0.013, 0.009, 0.011, 0.008 for B = 28, 29, 32, 33, 36, 61
  residual backward L = 1: 0.027 [g_V];  L = 2: 0.031 [g_gating];  L = 3: 0.038 [g_gating]
  pack / unpack     0.115 [g_gating]
  large logits      0.025 [g_gating], every value finite
  repeatability     bitwise equal
Found by this module: no defect -- every kernel passed as it was.  That the cases bite was tried on scratch builds with one line
of a kernel changed each (error / tolerance on the MI355X; the rest of the GPU suite passed all three):
  moe_mid_bwd_kernel without the ``fetch(grp + gridDim.x)`` refresh: the four mid cases fail (g_C 197837, g_V 47628 at (4, 64))
  moe_mid_bwd_kernel with ``acc`` zeroed on every trip:              the four mid cases fail (g_C 23160 at (4, 64))
  cross_fwd_kernel making no second trip:                            both CrossNetwork cases fail (NaN from poisoned memory)
(cross_fwd_kernel striding by ``gridDim.x`` instead of ``nwaves`` still writes every row, some of them four times: slower, not
wrong, so no comparison of values can see it.)
"""
import ctypes
import functools
import os
import sys

if __name__ == "__main__":  # python tests/test_gpu_dcn_trips.py: the float32-eager figures, on the CPU
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import pytest
import torch

from oracle import ctr_oracle as O
from test_gpu_kernels import _cross_net_mix_reference, dev

pytestmark = pytest.mark.gpu
F64 = np.float64
FAR = 1 << 22  # rows at which every launch here sits at its cap

OUT_TOL = (2e-5, 2e-6)
GRAD_TOL = (1e-4, 1e-5)


def ratio(got, want, tol, what):
    """max |got - want| / (atol + rtol |want|), atol = tol[1] max(1, max|want|): test_gpu_kernels.close as a figure."""
    got = got.detach().cpu().numpy().astype(F64) if torch.is_tensor(got) else np.asarray(got, F64)
    want = want.detach().cpu().numpy().astype(F64) if torch.is_tensor(want) else np.asarray(want, F64)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    assert np.isfinite(got).all(), f"{what}: not finite"
    atol = tol[1] * max(1.0, float(np.abs(want).max()) if want.size else 1.0)
    return float((np.abs(got - want) / (atol + tol[0] * np.abs(want))).max()) if want.size else 0.0


def check(case, pairs):
    """pairs: (what, got, want, tol).  Prints every figure, then asserts all of them."""
    figures = [(what, ratio(got, want, tol, f"{case} {what}")) for what, got, want, tol in pairs]
    worst = max(figures, key=lambda f: f[1])
    print(f"TRIPS {case}: worst {worst[1]:.3f} [{worst[0]}]  " + " ".join(f"{w}={r:.3f}" for w, r in figures))
    bad = [(w, r) for w, r in figures if not r <= 1.0]
    assert not bad, f"{case}: error / tolerance {bad}"
    return worst


# ---- the library's own grids ------------------------------------------------------------------------------------------------
def query(name, *args, n=1):
    from torch_rechub_amd import _lib
    return _lib.query(name, *args, out=(ctypes.c_int,) * n)


def mid_blocks(B, E, r, bwd):
    from torch_rechub_amd import _lib
    return _lib.call("rh_cross_moe_mid_blocks", B, E, r) if bwd else query("rh_cross_moe_mid_fwd_blocks", B, E, r)


def samples_per_group(E, r):
    """Read off the backward's grid: the smallest B that needs a second group, minus one."""
    spb = next(b for b in range(1, 258) if mid_blocks(b + 1, E, r, True) == 2)
    assert mid_blocks(spb, E, r, True) == 1 and spb == 256 // (E * r)
    return spb


def ceil_div(a, b):
    return -(-a // b)


def assert_past_cap(units, grid, cap, what):
    """The fixed condition of every trip case: the launch is at its cap, needs a second trip, and its last trip is ragged."""
    assert grid == cap, f"{what}: grid {grid} is not the cap {cap}"
    assert units > grid, f"{what}: {units} work units fit one trip of {grid} workgroups"
    assert units % grid != 0, f"{what}: {units} work units are a multiple of the grid {grid}: no ragged tail"
    return ceil_div(units, grid)


def strided(t, pad):
    """The same values as rows of a wider buffer (NaN in the padding), on the device."""
    wide = torch.full((t.shape[0], t.shape[1] + pad), float("nan"))
    wide[:, :t.shape[1]] = t
    return wide.to(dev())[:, :t.shape[1]]


# ---- CrossNetwork -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,L,stride", [(5, 1, True), (130, 3, False)])
def test_cross_network_second_trip_of_the_forward_grid(d, L, stride):
    from torch_rechub_amd import _lib, ops
    cap = query("rh_cross_fwd_nblocks", FAR)
    B = 4 * cap + 5
    trips = assert_past_cap(ceil_div(B, 4), query("rh_cross_fwd_nblocks", B), cap, "cross forward")
    nb = _lib.call("rh_cross_bwd_nblocks", B)
    assert trips == 2 and ceil_div(B, 4) > nb == _lib.call("rh_cross_bwd_nblocks", FAR) and ceil_div(B, 4) % nb != 0
    g = torch.Generator().manual_seed(B + d + L)
    x = torch.randn(B, d, generator=g)
    W = torch.randn(L, d, generator=g) / np.sqrt(d)
    Bv = torch.randn(L, d, generator=g) * 0.1
    gy = torch.randn(B, d, generator=g)
    xn, Wn, Bn, gn = (t.numpy().astype(F64) for t in (x, W, Bv, gy))
    want = O.cross_network_forward(xn, Wn, Bn)
    gx, gW, gB = O.cross_network_backward(xn, Wn, Bn, gn)
    xd = (strided(x, 3) if stride else x.to(dev())).detach().requires_grad_(True)
    assert (xd.stride(0) != d) == stride
    Wd, Bd = (t.to(dev()).requires_grad_(True) for t in (W, Bv))
    y = ops.cross_network(xd, Wd, Bd)
    y.backward(gy.to(dev()))
    check(f"cross_network B={B} d={d} L={L}", [("out", y, want, OUT_TOL), ("g_x", xd.grad, gx, GRAD_TOL),
                                               ("g_w", Wd.grad, gW, GRAD_TOL), ("g_b", Bd.grad, gB, GRAD_TOL)])


# ---- the two epilogues ------------------------------------------------------------------------------------------------------
def test_cross_v2_epilogue_past_one_trip_of_its_grid():
    from torch_rechub_amd import ops
    d = 1027
    cap = query("rh_cross_v2_epilogue_nblocks", FAR, d)
    B = cap * 1024 // d + 16
    assert d % 4 != 0
    assert_past_cap(ceil_div(B * d, 1024), query("rh_cross_v2_epilogue_nblocks", B, d), cap, "v2 epilogue")
    g = torch.Generator().manual_seed(B + d)
    x0, y, x, gy = (torch.randn(B, d, generator=g) for _ in range(4))
    b = torch.randn(d, generator=g) * 0.3
    ref_in = [t.double().requires_grad_(True) for t in (x0, y, b, x)]
    ref = ref_in[0] * ref_in[1] + ref_in[2] + ref_in[3]
    ref.backward(gy.double())
    hip_in = [t.to(dev()).requires_grad_(True) for t in (x0, y, b, x)]
    out = ops.cross_v2_epilogue(*hip_in)
    out.backward(gy.to(dev()))
    check(f"v2_epilogue {B}x{d}", [("out", out, ref.detach(), (1e-6, 1e-6))] +
          [(name, h.grad, r.grad, (2e-5, 2e-6)) for name, h, r in zip(("g_x0", "g_y", "g_b", "g_x"), hip_in, ref_in)])


@pytest.mark.parametrize("E", [1, 3])
def test_cross_mix_epilogue_past_one_trip_of_the_wave_grid(E):
    from torch_rechub_amd import _lib, ops
    d = 8
    cap = _lib.call("rh_cross_mix_nblocks", FAR)
    B = 4 * cap + 3
    assert_past_cap(ceil_div(B, 4), _lib.call("rh_cross_mix_nblocks", B), cap, "mix epilogue")
    g = torch.Generator().manual_seed(B + d + E)
    x0, xl = torch.randn(B, d, generator=g), torch.randn(B, d, generator=g)
    uv = torch.randn(E, B, d, generator=g)
    gate = torch.softmax(torch.randn(B, E, generator=g), dim=1)
    bias = torch.randn(d, generator=g) * 0.3
    gy = torch.randn(B, d, generator=g)
    ref_in = [t.double().requires_grad_(True) for t in (x0, xl, uv, gate, bias)]
    r0, rl, ruv, rg, rb = ref_in
    ref = ((r0.unsqueeze(0) * (ruv + rb.view(1, 1, d))) * rg.t().unsqueeze(2)).sum(0) + rl
    ref.backward(gy.double())
    hip_in = [t.to(dev()).requires_grad_(True) for t in (x0, xl, uv, gate, bias)]
    out = ops.cross_mix_epilogue(*hip_in)
    out.backward(gy.to(dev()))
    check(f"mix_epilogue B={B} d={d} E={E}", [("out", out, ref.detach(), OUT_TOL)] +
          [(name, h.grad, r.grad, GRAD_TOL) for name, h, r in zip(("g_x0", "g_xl", "g_uv", "g_gate", "g_bias"), hip_in, ref_in)])


# ---- CrossNetMix on the two-product form ------------------------------------------------------------------------------------
NAMES = "U V C bias gating".split()


def param_lists(mix):
    return (list(mix.u_list), list(mix.v_list), list(mix.c_list), list(mix.bias), [m.weight for m in mix.gating])


@functools.lru_cache(maxsize=None)
def mix_case(B, d, L, E, r, gate_scale):
    """The module of test_cross_net_mix_two_product_form_vs_reference_formula (biases 0.3 N(0, 1), U and V x 3), its input,
    the upstream gradient, and the float64 reference of the output and of every gradient.  Computed once per shape."""
    from torch_rechub_amd.basic.layers import CrossNetMix
    g = torch.Generator().manual_seed(B + d + 7 * E + r)
    torch.manual_seed(B + 3 * d + E + r)
    mix = CrossNetMix(d, num_layers=L, low_rank=r, num_experts=E)
    with torch.no_grad():
        for b in mix.bias:
            b.copy_(torch.randn(b.shape, generator=g) * 0.3)
        for t in list(mix.u_list) + list(mix.v_list):
            t.mul_(3.0)
        for m in mix.gating:
            m.weight.mul_(gate_scale)
    x = torch.randn(B, d, generator=g)
    gy = torch.randn(B, d, generator=g)
    want = eager(mix, x, gy, torch.float64)
    return mix, x, gy, want


def eager(mix, x, gy, dtype):
    """CrossNetMix.forward as the reference writes it, eager torch on the CPU in ``dtype``: out, g_x, parameter gradients."""
    params = [[t.detach().to(dtype).requires_grad_() for t in lst] for lst in param_lists(mix)]
    xr = x.to(dtype).requires_grad_()
    out = _cross_net_mix_reference(xr, *params)
    out.backward(gy.to(dtype))
    res = {"out": out.detach(), "g_x": xr.grad}
    for name, lst in zip(NAMES, params):
        for i, t in enumerate(lst):
            res[f"g_{name}[{i}]"] = t.grad
    return res


def logits64(mix, x):
    return x.double() @ torch.cat([m.weight.detach().double() for m in mix.gating], 0).t()


def hip(mix_cpu, x, gy, stride=False):
    import copy
    from torch_rechub_amd import ops
    mix = copy.deepcopy(mix_cpu).to(dev())
    E, r = mix.num_experts, mix.u_list[0].shape[2]
    assert ops.cross_moe_ok(x.to(dev()), mix.num_layers, E, x.shape[1], r)  # the two-product form, not the batched GEMMs
    xd = (strided(x, 16 - x.shape[1] % 16) if stride else x.to(dev())).detach().requires_grad_()
    assert (xd.stride(0) != x.shape[1]) == stride
    out = mix(xd)
    out.backward(gy.to(dev()))
    torch.cuda.synchronize()
    res = {"out": out.detach(), "g_x": xd.grad}
    for name, lst in zip(NAMES, param_lists(mix)):
        for i, t in enumerate(lst):
            res[f"g_{name}[{i}]"] = t.grad
    return res


def pairs(got, want):
    assert got.keys() == want.keys()
    return [(k, got[k], want[k], OUT_TOL if k == "out" else GRAD_TOL) for k in want]


def check_mix(B, d, L, E, r, stride=False, gate_scale=1.0):
    mix, x, gy, want = mix_case(B, d, L, E, r, gate_scale)
    got = hip(mix, x, gy, stride)
    check(f"cross_net_mix B={B} d={d} L={L} E={E} r={r}" + (" strided" if stride else ""), pairs(got, want))
    return got


def mid_trips(B, E, r):
    """(forward trips, backward trips) of the mid kernels, each asserted past its cap with a ragged tail."""
    spb = samples_per_group(E, r)
    groups = ceil_div(B, spb)
    return tuple(assert_past_cap(groups, mid_blocks(B, E, r, bwd), mid_blocks(FAR, E, r, bwd), f"mid bwd={bwd}")
                 for bwd in (False, True))


def one_per_group_rows(E, r):
    assert samples_per_group(E, r) == 1
    return 2 * mid_blocks(FAR, E, r, False) + 3


@pytest.mark.parametrize("E,r", [(4, 64), (16, 16)])
def test_mid_kernels_one_sample_per_group_three_forward_and_nine_backward_trips(E, r):
    B = one_per_group_rows(E, r)
    assert mid_trips(B, E, r) == (3, 9)
    assert ceil_div(B, 1) % mid_blocks(B, E, r, True) == 3  # the tail of both directions: 3 groups
    check_mix(B, 8, 1, E, r)


def test_mid_backward_twice_is_bitwise_equal():
    B = one_per_group_rows(4, 64)
    mix, x, gy, _ = mix_case(B, 8, 1, 4, 64, 1.0)
    first, second = hip(mix, x, gy), hip(mix, x, gy)
    for k in first:
        assert torch.equal(first[k], second[k]), k


@pytest.mark.parametrize("which,d", [("backward", 8), ("forward", 5)])
def test_mid_kernels_ten_samples_per_group_past_each_cap_with_a_partial_last_group(which, d):
    E, r = 3, 8
    spb = samples_per_group(E, r)
    assert spb == 10
    B = mid_blocks(FAR, E, r, which == "backward") * spb + (3 if which == "backward" else 5)
    assert B % spb != 0  # the last group is partial
    groups = ceil_div(B, spb)
    bwd_trips = assert_past_cap(groups, mid_blocks(B, E, r, True), mid_blocks(FAR, E, r, True), "mid backward")
    if which == "forward":
        assert assert_past_cap(groups, mid_blocks(B, E, r, False), mid_blocks(FAR, E, r, False), "mid forward") == 2
        assert bwd_trips == 5
    else:
        assert bwd_trips == 2 and mid_blocks(B, E, r, False) == groups  # (the forward: one trip)
    check_mix(B, d, 1, E, r)


@pytest.mark.parametrize("E,r,spb,kp", [(5, 16, 3, 88), (3, 32, 2, 100), (1, 64, 4, 68), (16, 4, 4, 80)])
def test_mid_kernels_lane_layouts(E, r, spb, kp):
    from torch_rechub_amd import _lib
    assert samples_per_group(E, r) == spb and _lib.call("rh_cross_moe_kp", E, r) == kp
    for B in (37, spb - 1, spb + 1):
        assert mid_blocks(B, E, r, True) == mid_blocks(B, E, r, False) == ceil_div(B, spb)
        check_mix(B, 6, 2, E, r)


@pytest.mark.parametrize("B", [28, 29, 32, 33, 36, 61])
def test_unpack_sums_the_g_c_partials_across_the_start_and_end_of_the_eight_in_flight_loop(B):
    E, r = 4, 64
    assert mid_blocks(B, E, r, True) == B  # one sample per group, under the cap: B partial rows of g_C
    check_mix(B, 4, 1, E, r)


@pytest.mark.parametrize("L", [1, 2, 3])
def test_residual_backward_past_its_cap_in_every_mode(L):
    E, r, d = 2, 4, 257
    cap = query("rh_cross_moe_res_blocks", FAR, d)
    B = cap * 256 // d + 19
    assert_past_cap(ceil_div(B * d, 256), query("rh_cross_moe_res_blocks", B, d), cap, "residual backward")
    groups = ceil_div(B, samples_per_group(E, r))
    assert mid_blocks(B, E, r, True) == mid_blocks(B, E, r, False) == groups  # the mid kernels: one trip
    check_mix(B, d, L, E, r, stride=True)


def test_pack_and_unpack_past_their_caps():
    from torch_rechub_amd import _lib
    L, E, r, B = 2, 4, 64, 9
    kp = _lib.call("rh_cross_moe_kp", E, r)
    cap = query("rh_cross_moe_pack_blocks", L, E, 1 << 16, r)
    d = cap * 256 // (L * kp) + 17
    assert assert_past_cap(ceil_div(2 * L * kp * d, 256), query("rh_cross_moe_pack_blocks", L, E, d, r), cap, "pack") >= 3
    ucap, _ = query("rh_cross_moe_unpack_blocks", L, E, 1 << 16, r, n=2)
    ugrid, cblocks = query("rh_cross_moe_unpack_blocks", L, E, d, r, n=2)
    assert cblocks == L * ceil_div(E * r * r, 64)
    assert assert_past_cap(ceil_div(L * (2 * E * d * r + d) + E * d, 256), ugrid, ucap, "unpack") >= 3
    check_mix(B, d, L, E, r)


def test_gate_softmax_with_logits_past_plus_and_minus_100():
    B, d, L, E, r, scale = 64, 8, 1, 4, 8, 60.0
    mix, x, _, _ = mix_case(B, d, L, E, r, scale)
    lg = logits64(mix, x)
    # (exp overflows float32 past 88.7: only the subtraction of the row maximum keeps the softmax finite)
    assert float(lg.max()) > 100 and float(lg.min()) < -100, (float(lg.min()), float(lg.max()))
    check_mix(B, d, L, E, r, gate_scale=scale)


if __name__ == "__main__":
    # float32 eager torch on the CPU through the same comparison, for every CrossNetMix shape above at today's caps
    shapes = [(4099, 8, 1, 4, 64, 1.0), (4099, 8, 1, 16, 16, 1.0), (5123, 8, 1, 3, 8, 1.0), (20485, 5, 1, 3, 8, 1.0),
              (4099, 257, 1, 2, 4, 1.0), (4099, 257, 2, 2, 4, 1.0), (4099, 257, 3, 2, 4, 1.0), (9, 1025, 2, 4, 64, 1.0),
              (64, 8, 1, 4, 8, 60.0)]
    shapes += [(B, 4, 1, 4, 64, 1.0) for B in (28, 29, 32, 33, 36, 61)]
    shapes += [(B, 6, 2, E, r, 1.0) for E, r, spb in ((5, 16, 3), (3, 32, 2), (1, 64, 4), (16, 4, 4)) for B in (37, spb - 1, spb + 1)]
    for shape in shapes:
        mix, x, gy, want = mix_case(*shape)
        check("float32 eager " + str(shape), pairs(eager(mix, x, gy, torch.float32), want))
