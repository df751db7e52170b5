"""The kernels every CTR step ends in -- the prediction head and its fused loss (csrc/linear.hip), the BatchNorm / activation
apply passes (csrc/mlp.hip), PReLU and Dice (csrc/din.hip) -- past their launch caps, against float64.

Each of these launches is a grid-stride loop under a capped grid; past the cap a workgroup makes a second trip that reuses its
registers (the head's weight vectors and accumulators ``lacc`` / ``wacc``, Dice's prefetched row), its LDS reduction slots and its
per-workgroup partial sums.  Every case asks the library for the grid of the launch it is about -- the query is the function the
launch itself calls -- and asserts, before it compares anything, that the grid is at its cap, that there are more work units than
workgroups and that the units are no multiple of the grid.  Rows and element counts are derived from the queries ("one trip + a
few units"); the figures in brackets are today's.  A work unit is what one workgroup takes per trip.

  launch                              query                      unit               cap     cases
  head forward (plain, + loss)        rh_head_loss_nblocks       16 rows            2048    B = 16 cap + 5 [32773]: 2 trips, one
                                                                                            workgroup (5 of its 16 rows) in the second
  head backward (every form)          rh_head_nblocks            16 rows (a pass)   256     B = 32 cap + 49 [8241]: 516 passes, 3 trips for
                                                                                            4 workgroups, 2 for the rest;  B = 64 cap + 5
                                                                                            [16389]: 1025 passes, 5 trips, one row group in
                                                                                            the last.  (B = 32773: 2049 passes, 9 trips)
  BatchNorm apply, three-launch path  rh_bn_apply_nblocks (new)  1024 elements      2048    C = 36, B = 1024 cap / C + 100 [58354 x 36:
                                                                                            2052 units, the last one half full]
  PReLU forward / backward            rh_prelu_nblocks           1024 elements      1024    n = 1024 cap + 2051 [1 050 627], 1-D: 1026 units
                                                                                            and an n % 4 = 3 remainder
  Dice, plain                         rh_dice_nblocks            4 rows             4096    N = 4 cap + 5 [16389]
  Dice folded into BatchNorm (+ head) rh_bn_dice_stats_blocks    4 rows             2048    N = 4 cap + 5 [8197] (statistics pass)

Cases
  head forward + loss   K = 5 (nv = 1: one vector lane and the K % 4 tail lane), 36 from a row-padded view (ldh = 40), 260 (lanes make
                        two passes over v); with and without bias, 0 / 1 / 2 extra logit terms; an upstream gradient of y ("gy"),
                        targets ("t": ops.fusion_begin(target) -> rh_head_loss_fwd, the mean finished by rh_step_scalars, the BCE
                        gradient formed inside rh_head_bwd_ex) or both.  The fused loss against float64 AND against the unfused
                        ops.bce_mean of the returned y.  One case gives the five rows of the second trip logits of +-200 with the
                        opposite label: each contributes exactly 100 to the float64 sum (asserted), so the -100 clamp decides the loss
  head backward         K = 5, 36 / 130 / 200 / 260 / 520 = head_bwd_kernel<1> / <2> / <4> / <8> / <16> (every instantiation the
                        dispatch can pick) at 3 ragged trips, K = 5, 130, 260 at 5; the three gradient modes; one case twice, every
                        gradient bitwise equal (no atomics)
  BatchNorm form        head_bwd_kernel<1 / 2 / 4, BN> (K = 36, 128, 256), p = 0 and 0.3 with the mask rebuilt from the counter hash on
                        the host, the layer's output given or recomputed from bn_z (h = NULL, as the fused chain calls it), g_h, g_z,
                        g_w, g_b and the two BatchNorm column sums; with the step-scalar workgroup (``sc.on``: one workgroup more, the
                        row loop strides by the grid without it) every scalar it writes -- loss mean, Adam bias corrections, ring,
                        step, two counters -- bit for bit against a separate rh_step_scalars launch on a copy of the state.  Through
                        the C interface with every output buffer NaN on entry: NOT REACHABLE past the cap through the Python
                        wrappers, as is rh_head_bnact_fwd.  ops.mlp_chain_ok refuses B > 4096 (one trip of the forward is 32768 rows)
                        and _HeadFn.backward takes rh_head_bwd_bn only while rh_head_nblocks(B) <= 128, half the cap;
                        test_wrappers_refuse_the_chain_and_the_batchnorm_form_past_one_trip asserts both and that one hidden layer of
                        32 columns at B = 32773 goes layer by layer
  BatchNorm apply       ReLU and PReLU (slope 0.25), p = 0 and 0.25, forward and backward: output, dx, dgamma, dbeta, the slope
                        gradient, running mean and (unbiased) running variance against float64 training-mode BatchNorm with the host's
                        mask; the three-launch path asserted through the row count of its statistics pass (rh_bn_prelu_nblocks)
  PReLU                 slopes 0.25 and -0.6; output and input gradient also bit-equal to the same float32 expression on the CPU
  Dice                  C = 36 (one element per lane, lanes 36 .. 63 idle), 200 (four, not FULL), 520 (sixteen; plain only: the
                        folded modes stop at C = 512), and C = 64 / 128 from a view one float into its buffer (data_ptr() % 16 == 4
                        asserted: the scalar kernel, FULL, in place of the vector kernel); forward, backward (every alpha partial
                        summed), folded BatchNorm-Dice and its head form with dgamma, dbeta, dalpha, the head's weight and bias
                        gradients and the running statistics; C = 64 / 128 aligned = the vector kernel at the cap of its statistics pass
                        with a partly filled last wavefront pass

References and tolerances.  float64 autograd of the same expression on the CPU (torch's BCELoss for the loss, the Dice formula of
test_gpu_kernels._dice_ref, training-mode BatchNorm written out, the mask from test_gpu_mlp_dropout_oracle.host_keep); the
BatchNorm form of the head's backward against what include/rechub_hip.h documents, from the launch's own inputs.  Inputs of ReLU /
PReLU cases are nudged so that every float64 pre-activation is further than 1e-5 from 0 (asserted).  |got - want| <= atol + rtol
|want| with atol = a max(1, max|want|), every element of every output, (rtol, a) from the existing test of the same quantity:
  head    test_head_sigmoid_vs_autograd: (2e-5, 2e-6), g_w and g_b (2e-5, 2e-6 sqrt(B));  loss, and fused against unfused,
          1e-5 max(1, |want|) (test_hidden_layer_and_prediction_with_two_consumers_each); the loss mean of the scalar workgroup
          (2e-6, 1e-6) (test_bce_mean_vs_torch); the BatchNorm column sums (1e-4, 1e-5) = dbeta / dgamma below
  bn+relu test_bn_relu_dropout_vs_torch_modules: out (2e-5, 2e-6), dx / dgamma / dbeta (1e-4, 1e-5), running mean (1e-5, 1e-6),
          running variance (2e-5, 1e-6); p = 0.25 under the same bounds (the dropout oracle's own are wider)
  bn+prelu test_mlp_batchnorm_prelu_dropout_epilogue: out and buffers (1e-4, 1e-5), dx and every parameter gradient (2e-4, 2e-5)
  prelu   test_prelu_single_slope_vs_torch: out and gx bit-equal to float32 eager, the slope gradient (1e-4, 1e-4); against float64
          out and gx get one float32 rounding of slope * x, (1e-7, 1e-9): 2^-24 = 0.6 of it by construction
  dice    test_dice_kernel_vs_reference_formula: (2e-5, 2e-6), gradients (1e-4, 1e-5);  folded: test_bn_dice_folded_vs_modules /
          test_bn_dice_head_vs_modules: out (2e-4, 5e-6), gradients (1e-3, 2e-5), dalpha (1e-3, 1e-4), running statistics as above
No bound was widened, none had to be derived from the float32-eager error, and no element is excluded.  float32 eager torch on the
CPU through the same comparison (``python tests/test_gpu_tower_trips.py``), worst error / tolerance per family: head forward 0.065
[g_e, K = 260], head backward 0.040 [g_e, K = 520], BatchNorm form 0.009, bn + relu 0.040 [out], bn + prelu 0.015, prelu 0.543 (the
rounding above; slope gradient 0.001), dice 0.012, folded dice 0.050 [out, C = 128]: far below 0.5 of every existing tolerance
although the sums run over up to 58354 rows.

Worst error / tolerance per case on the MI355X (the ``TRIPS`` lines; the worst quantity in brackets), all 46 tests passing:
  head forward + loss   K = 5: 0.022 [g_h], 0.009 [y];  K = 36 strided: 0.011 [y], 0.031 [g_e];  K = 260: 0.043 [g_e], 0.012 [y];
                        clamp case 0.011 [y], loss 0.000;  fused against unfused <= 0.012 everywhere
  head backward         B = 8241: K = 5 0.014, 36 0.009, 130 0.045, 200 0.030, 260 0.013, 520 0.036;  B = 16389: K = 5 0.023, 130
                        0.014, 260 0.033 (worst: g_e or y; g_w <= 0.001, g_b <= 0.002);  twice: bitwise equal
  BatchNorm form        0.005, 0.001, 0.001, 0.007, 0.007 in the order of HEAD_BN_CASES; the scalars bit-equal, loss mean <= 0.002
  BatchNorm apply       relu 0.033 [out] at both p;  prelu 0.010 [out] at both p (dslope <= 0.002)
  PReLU                 0.000 and 0.543 [out: the rounding of slope * x]; slope gradient 0.000; bit-equal to float32 eager
  Dice                  C = 36 0.011, 200 0.006, 520 0.007, 64 + 1 float 0.006, 128 + 1 float 0.006
  folded Dice (+ head)  C = 36 0.016 (0.027), 200 0.021 (0.023), 64 + 1 float 0.012 (0.021), 128 + 1 float 0.042 (0.019), vector
                        kernel C = 64 0.012 (0.021), C = 128 0.043 (0.018)
Found by this module: no defect -- every kernel passed as it was.  That the cases bite was tried on scratch builds with one line of a
kernel changed each, this module run against each (error / tolerance on the MI355X; the rest of the suite was not run on them):
  head_fwd_kernel with ``lacc`` reset inside the row loop:     the 5 cases with targets at B = 32773 fail (loss 7.0 .. 16.0, fused
                                                               against unfused the same: the first-trip terms of five rows are lost)
  head_fwd_kernel striding by ``gridDim.x * kHeadRows * 2``:   all 7 cases at B = 32773 fail (y not finite: NaN from poisoned memory)
  head_bwd_kernel with ``wacc`` zeroed on every trip:          all 21 head cases with a comparison fail (g_w 99 .. 5267)
  dice_kernel without the ``fetch(r + nw)`` refresh:           all 13 scalar-kernel cases fail (out 147 406 .. 277 661, folded dgamma
                                                               172 .. 838); the 4 vector-kernel cases pass, as they must
  prelu_bwd_kernel keeping the sum it had after its first trip: both PReLU cases fail (slope gradient 43.1)
(A mutation that only recomputes rows -- a stride shorter than the grid, say -- writes every value again, correctly: slower, not
wrong, and no comparison of values can see it.)
"""
import functools
import os
import sys

if __name__ == "__main__":  # python tests/test_gpu_tower_trips.py: the float32-eager figures, on the CPU
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import pytest
import torch

from test_gpu_dcn_trips import FAR, assert_past_cap, ceil_div, check, query, strided
from test_gpu_kernels import _dice_ref, dev
from test_gpu_mlp_dropout_oracle import host_keep

pytestmark = pytest.mark.gpu
F64 = np.float64
SEED, C0 = 0x5DEECE66D1234, 7  # the dropout stream of every case with p > 0: seed (> 2^32) and call counter before the call
KINK = 1e-5                    # every float64 pre-activation of a ReLU / PReLU case stays further than this from 0

# What the queries answer today; read by the CPU run only (no test below looks at it).
TODAY = dict(head_fwd=2048, head_bwd=256, apply=2048, prelu=1024, dice=4096, dice_stats=2048)


def caps():
    """The cap of every launch in scope, asked of the function the launch itself calls."""
    from torch_rechub_amd import _lib
    return dict(head_fwd=_lib.call("rh_head_loss_nblocks", FAR), head_bwd=_lib.call("rh_head_nblocks", FAR),
                apply=query("rh_bn_apply_nblocks", FAR * 1024), prelu=_lib.call("rh_prelu_nblocks", FAR * 1024),
                dice=_lib.call("rh_dice_nblocks", FAR), dice_stats=_lib.call("rh_bn_dice_stats_blocks", FAR))


# rows / elements of every case from the caps: "one trip + a few units"
def head_fwd_rows(c):
    return 16 * c["head_fwd"] + 5  # [32773]: 16 rows per workgroup and trip; 2049 units, 1 workgroup in the second trip


def head_bwd_rows(c, trips):
    # [8241]: 516 passes of 16 rows over 256 workgroups, 3 trips for 4 of them and 2 for the rest;  [16389]: 1025 passes, 5 trips
    return c["head_bwd"] * 32 + 16 * 3 + 1 if trips == 3 else c["head_bwd"] * 32 * 2 + 5


def apply_rows(c, C):
    return c["apply"] * 1024 // C + 100  # [58354 x 36: 2052 units of 1024 elements]


def prelu_numel(c):
    return c["prelu"] * 1024 + 1024 * 2 + 3  # [1 050 627]


def dice_rows(c, stats):
    return 4 * c["dice_stats" if stats else "dice"] + 5  # [16389; the folded modes 8197]: 4 rows per workgroup and trip


def poison(*shapes):
    """NaN into the blocks the caching allocator hands out next: the wrappers allocate their outputs themselves (torch.empty), so
    tensors of the outputs' sizes are filled with NaN and freed right before the call, and the wrapper's torch.empty of the same
    size takes such a block (on top of the suite's own fixture, which poisons the free pools before every GPU test).  An element
    no workgroup wrote then fails the finiteness check of ``ratio``."""
    junk = [torch.full(s, float("nan"), dtype=torch.float32, device=dev()) for s in shapes]
    del junk


def pairs(got, want, tols):
    assert got.keys() == want.keys(), (sorted(got), sorted(want))
    return [(k, got[k], want[k], tols[k] if k in tols else tols[k.rstrip("0123456789")]) for k in want]


def _t(x, dtype):
    return None if x is None else x.to(dtype)


# ---- the head: y = sigmoid(h w^T + b + e0 + e1), mean BCE, every gradient ---------------------------------------------------
def head_tols(B):
    """test_head_sigmoid_vs_autograd (rtol 2e-5, atol 2e-6 max(1, max|want|), x sqrt(B) for the two sums over the batch); the
    loss: test_hidden_layer_and_prediction_with_two_consumers_each (1e-5 max(1, |want|)), which is also the bound between the
    fused loss and the unfused bce_mean of the returned y."""
    return {"y": (2e-5, 2e-6), "g_h": (2e-5, 2e-6), "g_e": (2e-5, 2e-6), "g_w": (2e-5, 2e-6 * np.sqrt(B)),
            "g_b": (2e-5, 2e-6 * np.sqrt(B)), "loss": (0.0, 1e-5)}


@functools.lru_cache(maxsize=None)
def head_case(B, K, bias, nextra, mode, clamp=0):
    """mode: "gy" (an upstream gradient of y), "t" (targets: the fused loss, its gradient formed inside the head's backward)
    or "both".  clamp: that many last rows get a logit of +-200 against the opposite label."""
    g = torch.Generator().manual_seed(B + 7 * K + nextra + len(mode))
    inp = dict(h=torch.randn(B, K, generator=g), w=torch.randn(1, K, generator=g) / np.sqrt(K),
               b=torch.randn(1, generator=g) * 0.3 if bias else None,
               ex=tuple(torch.randn(B, 1, generator=g) * 0.5 for _ in range(nextra)),
               gy=torch.randn(B, generator=g) if mode in ("gy", "both") else None,
               t=(torch.rand(B, generator=g) < 0.3).float() if mode in ("t", "both") else None)
    if clamp:
        z = (inp["h"][-clamp:].double() @ inp["w"].double().t()).squeeze(1)
        z = z + (inp["b"].double() if bias else 0.0) + sum(e[-clamp:, 0].double() for e in inp["ex"][1:])
        sign = torch.tensor([1.0, -1.0] * clamp, dtype=torch.float64)[:clamp]
        inp["ex"][0][-clamp:, 0] = (200.0 * sign - z).float()
        inp["t"][-clamp:] = (sign < 0).float()
    return inp, head_eager(inp, torch.float64)


def head_eager(inp, dtype):
    h, w = inp["h"].to(dtype).requires_grad_(), inp["w"].to(dtype).requires_grad_()
    b = None if inp["b"] is None else inp["b"].to(dtype).requires_grad_()
    ex = [e.to(dtype).requires_grad_() for e in inp["ex"]]
    z = h @ w.t()
    if b is not None:
        z = z + b
    for e in ex:
        z = z + e
    y = torch.sigmoid(z.squeeze(1))
    res, total = {}, 0.0
    if inp["t"] is not None:  # torch's BCELoss: both logarithms clamped at -100, mean over the batch
        loss = torch.nn.functional.binary_cross_entropy(y, inp["t"].to(dtype))
        res["loss"] = loss.detach().reshape(1)
        total = total + loss
    if inp["gy"] is not None:
        total = total + (y * inp["gy"].to(dtype)).sum()
    total.backward()
    res.update(y=y.detach(), g_h=h.grad, g_w=w.grad)
    if b is not None:
        res["g_b"] = b.grad
    for i, e in enumerate(ex):
        res[f"g_e{i}"] = e.grad
    return res


def bce_terms64(y, t):
    y, t = y.double(), t.double()
    return -(t * torch.log(y).clamp(min=-100.0) + (1 - t) * torch.log1p(-y).clamp(min=-100.0))


def head_hip(inp, stride=False):
    """ops.head_sigmoid (+ ops.bce_mean under ops.fusion_begin(target)): rh_head_fwd / rh_head_loss_fwd + rh_step_scalars forward,
    rh_head_bwd_ex backward.  Returns the results and the unfused bce_mean of the returned y (None without targets)."""
    from torch_rechub_amd import ops
    d = dev()
    B, K = inp["h"].shape
    h = (strided(inp["h"], 4) if stride else inp["h"].to(d)).detach().requires_grad_()
    assert (h.stride(0) != K) == stride
    w = inp["w"].to(d).requires_grad_()
    b = None if inp["b"] is None else inp["b"].to(d).requires_grad_()
    ex = [e.to(d).requires_grad_() for e in inp["ex"]]
    t, gy = _t(inp["t"], d), _t(inp["gy"], d)
    res, unfused = {}, None
    poison((B,), (B,), (B, K), (ceil_div(B, 16),))
    if t is not None:
        ops.fusion_begin(target=t)
    try:
        y = ops.head_sigmoid(h, w, b, *ex)
        if t is not None:
            loss = ops.bce_mean(y, t)
            assert type(loss.grad_fn).__name__ == "_FusedBceFnBackward", "the head did not score against the targets"
    finally:
        if t is not None:
            ops.fusion_end()
    if t is not None:
        res["loss"] = loss.detach().reshape(1)
        unfused = ops.bce_mean(y.detach(), t).detach().reshape(1)
        total = loss if gy is None else loss + (y * gy).sum()
        total.backward()
    else:
        y.backward(gy)
    torch.cuda.synchronize()
    ops.check_errors()
    res.update(y=y.detach(), g_h=h.grad, g_w=w.grad)
    if b is not None:
        res["g_b"] = b.grad
    for i, e in enumerate(ex):
        res[f"g_e{i}"] = e.grad.clone()
    return res, unfused


def check_head(case_name, inp, want, stride=False):
    B = inp["h"].shape[0]
    got, unfused = head_hip(inp, stride)
    extra = []
    if unfused is not None:
        extra = [("fused == unfused", got["loss"], unfused, (0.0, 1e-5))]
    check(case_name, pairs(got, want, head_tols(B)) + extra)
    return got


def assert_head_fwd_past_cap(B, c):
    from torch_rechub_amd import _lib
    assert assert_past_cap(ceil_div(B, 16), _lib.call("rh_head_loss_nblocks", B), c["head_fwd"], "head forward") == 2


def assert_head_bwd_past_cap(B, c, trips):
    from torch_rechub_amd import _lib
    assert assert_past_cap(ceil_div(B, 16), _lib.call("rh_head_nblocks", B), c["head_bwd"], "head backward") == trips


@pytest.mark.parametrize("K,bias,nextra,mode,stride", [(5, True, 0, "gy", False), (5, False, 1, "t", False),
                                                       (36, True, 1, "t", True), (36, False, 2, "gy", True),
                                                       (260, False, 2, "both", False), (260, True, 0, "t", False)])
def test_head_forward_and_fused_loss_second_trip(K, bias, nextra, mode, stride):
    c = caps()
    B = head_fwd_rows(c)
    assert_head_fwd_past_cap(B, c)
    assert_head_bwd_past_cap(B, c, ceil_div(ceil_div(B, 16), c["head_bwd"]))  # (its backward: 2049 passes, 9 trips, 1 in the last)
    inp, want = head_case(B, K, bias, nextra, mode)
    check_head(f"head B={B} K={K} bias={bias} extras={nextra} {mode}" + (" strided" if stride else ""), inp, want, stride)


def test_fused_loss_clamps_the_logarithms_in_the_tail_rows_of_the_second_trip():
    c = caps()
    B = head_fwd_rows(c)
    assert_head_fwd_past_cap(B, c)
    tail = B - 16 * c["head_fwd"]  # the rows of the second trip
    inp, want = head_case(B, 36, True, 1, "t", clamp=tail)
    terms = bce_terms64(want["y"], inp["t"])
    assert tail == 5 and bool((terms[-tail:] == 100.0).all()), terms[-tail:]
    # the clamp decides the loss: without it the five rows would add 200 each (and -inf in float32)
    assert abs(float(want["loss"]) - float(terms.mean())) < 1e-12 and float(terms[-tail:].sum() / B) > 0.01 * float(want["loss"])
    got = check_head(f"head loss clamp B={B} K=36", inp, want)
    assert bool(((got["y"][-tail:] == 0) | (got["y"][-tail:] == 1)).all())  # float32: the sigmoid saturates at +-200


@pytest.mark.parametrize("trips,K,mode", [(3, 5, "gy"), (3, 36, "t"), (3, 130, "both"), (3, 200, "gy"), (3, 260, "t"),
                                          (3, 520, "both"), (5, 5, "both"), (5, 130, "t"), (5, 260, "gy")])
def test_head_backward_ragged_trips_at_the_cap_for_every_width_class(trips, K, mode):
    """K = 5, 36: one float4 per lane (5: the K % 4 tail lane only beside one vector); 130: two; 200: four; 260: eight; 520:
    sixteen -- head_bwd_kernel<1>, <2>, <4>, <8>, <16>."""
    c = caps()
    B = head_bwd_rows(c, trips)
    assert_head_bwd_past_cap(B, c, trips)
    inp, want = head_case(B, K, True, 1, mode)
    check_head(f"head backward B={B} K={K} {mode}", inp, want)


def test_head_backward_twice_is_bitwise_equal():
    c = caps()
    B = head_bwd_rows(c, 3)
    assert_head_bwd_past_cap(B, c, 3)
    inp, _ = head_case(B, 130, True, 1, "both")
    (first, _), (second, _) = head_hip(inp), head_hip(inp)
    for k in first:
        assert torch.equal(first[k], second[k]), k


# ---- the head's backward on a BatchNorm + ReLU + Dropout layer, with the step's scalar workgroup ------------------------------
BN_SUM_TOL = (1e-4, 1e-5)  # dbeta / dgamma of test_bn_relu_dropout_vs_torch_modules: the two column sums are exactly those


def away_from_kink(h, bn_of):
    """Nudges the few elements of h (float32, in place) whose float64 pre-activation bn_of(h) lies within 1e-3 of 0, and
    asserts the margin: a float32 kernel and the float64 reference then rectify every element the same way."""
    for _ in range(4):
        near = bn_of(h.double()).abs() < 1e-3
        if not bool(near.any()):
            break
        h[near] += 0.05
    margin = float(bn_of(h.double()).abs().min())
    assert margin > KINK, margin
    return h


@functools.lru_cache(maxsize=None)
def head_bn_case(B, K, p, mode):
    g = torch.Generator().manual_seed(B + 3 * K + int(100 * p))
    z = torch.randn(B, K, generator=g) * 1.5 + torch.randn(K, generator=g)
    gamma, beta = torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.5
    mean = z.double().mean(0).float()
    rstd = (1.0 / torch.sqrt(z.double().var(0, unbiased=False) + 1e-5)).float()
    away_from_kink(z, lambda x: (x - mean.double()) * rstd.double() * gamma.double() + beta.double())
    keep = torch.ones(B, K, dtype=torch.float64)
    if p > 0:
        keep = torch.from_numpy(host_keep(SEED, C0, B * K, p).reshape(B, K).astype(F64))
    inp = dict(z=z, mean=mean, rstd=rstd, gamma=gamma, beta=beta, keep=keep, p=p, w=torch.randn(1, K, generator=g) / np.sqrt(K),
               gy=torch.randn(B, generator=g) if mode in ("gy", "both") else None,
               t=(torch.rand(B, generator=g) < 0.3).float() if mode in ("t", "both") else None,
               g_loss=torch.tensor([0.7]))
    act = torch.relu((z.double() - mean.double()) * rstd.double() * gamma.double() + beta.double()) * keep / (1.0 - p)
    inp["y"] = torch.sigmoid(act @ inp["w"].double().t()).squeeze(1).float()  # the prediction the backward is handed
    inp["h"] = act.float()  # ... and the layer's output, when it is not recomputed
    return inp, head_bn_eager(inp, torch.float64)


def head_bn_eager(inp, dtype):
    """What rh_head_bwd_bn documents, from its own inputs: g_y = g_loss / B (y - t) / max((1 - y) y, 1e-12) (+ the upstream
    g_y), g_z = g_y y (1 - y), g_h = g_z w, g_w = g_z^T h, g_b = sum g_z, and the column sums of g1 = the gradient g_h taken
    through Dropout and ReLU, and of g1 xhat."""
    z, mean, rstd, gamma, beta, w, y = (inp[k].to(dtype) for k in ("z", "mean", "rstd", "gamma", "beta", "w", "y"))
    keep, B = inp["keep"].to(dtype) / (1.0 - inp["p"]), z.shape[0]
    gy = torch.zeros_like(y)
    if inp["t"] is not None:
        gy = gy + inp["g_loss"].to(dtype) / B * (y - inp["t"].to(dtype)) / ((1 - y) * y).clamp(min=1e-12)
    if inp["gy"] is not None:
        gy = gy + inp["gy"].to(dtype)
    gz = gy * y * (1 - y)
    xhat = (z - mean) * rstd
    bn = xhat * gamma + beta
    act = torch.relu(bn) * keep
    g_h = gz[:, None] * w
    g1 = g_h * keep * (bn > 0).to(dtype)
    return dict(g_z=gz, g_h=g_h, g_w=gz[None, :] @ act, g_b=gz.sum().reshape(1), bn_sum_g=g1.sum(0), bn_sum_gx=(g1 * xhat).sum(0))


def head_bn_hip(inp, recompute, scalars):
    """rh_head_bwd_bn / rh_head_bwd_bn_scalars through the C interface, every output buffer NaN on entry.  (The Python wrappers
    take this form only while rh_head_nblocks(B) <= 128, half the cap: see test_wrappers_refuse_...)"""
    from torch_rechub_amd import _lib, ops
    d = dev()
    p_, st = ops._p, ops._stream()
    B, K = inp["z"].shape
    nblk = _lib.call("rh_head_nblocks", B)
    z, w, y, gamma, beta = (inp[k].to(d).contiguous() for k in ("z", "w", "y", "gamma", "beta"))
    stat = torch.stack([inp["mean"], inp["rstd"]]).to(d).contiguous()
    h = None if recompute else inp["h"].to(d).contiguous()
    gy, t = _t(inp["gy"], d), _t(inp["t"], d)
    gl = inp["g_loss"].to(d) if t is not None else None
    rng = torch.tensor([SEED, C0 + 1, 0, 0], dtype=torch.int64, device=d)
    ctr = torch.tensor([C0], dtype=torch.int64, device=d)
    nan = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=d)  # noqa: E731
    g_h, g_z, g_w, g_b, partial, bn_partial = nan(B, K), nan(B), nan(1, K), nan(1), nan(nblk, K + 1), nan(nblk, 2, K)
    common = (p_(h), K, p_(w), p_(y), p_(gy), p_(t), p_(gl), B, K, p_(g_h), p_(g_z), p_(g_w), p_(g_b), p_(partial), 1, p_(z),
              p_(stat), p_(gamma), p_(beta), float(inp["p"]), p_(rng), p_(ctr), 1, p_(bn_partial))
    written = None
    if scalars:
        n = _lib.call("rh_head_loss_nblocks", B)
        gen = torch.Generator().manual_seed(B)
        lp = (torch.rand(n, generator=gen) * 16).to(d)

        def state():
            hyper = torch.zeros(16, dtype=torch.float64)
            hyper[:4] = torch.tensor([1e-3, 0.9, 0.999, 1e-8], dtype=torch.float64)
            return [nan(1), hyper.to(d), torch.tensor([41], dtype=torch.int64, device=d), torch.full((16,), -1.0, device=d),
                    torch.tensor([5], dtype=torch.int64, device=d), torch.tensor([10], dtype=torch.int64, device=d)]

        a, b = state(), state()
        tail = lambda s: (p_(s[0]), p_(s[1]), p_(s[2]), p_(s[3]), 8, p_(s[4]), 3, 7, p_(s[5]), 4, 0)  # noqa: E731
        _lib.call("rh_head_bwd_bn_scalars", *common, p_(lp), n, *tail(a), st)
        _lib.call("rh_step_scalars", p_(lp), n, B, *tail(b), st)
        torch.cuda.synchronize()
        for name, u, v in zip(("loss", "hyper", "step", "ring", "counter 0", "counter 1"), a, b):
            bits = torch.int64 if u.element_size() == 8 else torch.int32
            assert torch.equal(u.view(bits), v.view(bits)), f"the scalar workgroup and rh_step_scalars differ in {name}"
        assert int(a[2]) == 42 and int(a[4]) == 1 and int(a[5]) == 14 and float(a[3][2 * (42 & 7)]) > 0
        written = (a[0], (lp.double().sum() / B).reshape(1))
    else:
        _lib.call("rh_head_bwd_bn", *common, st)
    torch.cuda.synchronize()
    ops.check_errors()
    assert int(rng[1]) == C0 + 1 and int(ctr[0]) == C0  # the backward draws nothing
    res = dict(g_z=g_z, g_h=g_h, g_w=g_w, g_b=g_b, bn_sum_g=bn_partial[:, 0].double().sum(0),
               bn_sum_gx=bn_partial[:, 1].double().sum(0))
    # reduce = 1: g_w / g_b are the column sums of the partial rows, every one of which must have been written
    assert bool(torch.isfinite(partial).all()) and bool(torch.isfinite(bn_partial).all())
    return res, written


def head_bn_tols(B):
    tols = head_tols(B)
    return {"g_z": tols["g_e"], "g_h": tols["g_h"], "g_w": tols["g_w"], "g_b": tols["g_b"], "bn_sum_g": BN_SUM_TOL,
            "bn_sum_gx": BN_SUM_TOL}


HEAD_BN_CASES = [(3, 36, 0.0, "gy", False, False), (3, 128, 0.3, "t", True, True), (3, 256, 0.0, "t", False, True),
                 (5, 256, 0.3, "both", True, True), (5, 36, 0.3, "both", True, False)]


@pytest.mark.parametrize("trips,K,p,mode,recompute,scalars", HEAD_BN_CASES)
def test_head_backward_batchnorm_form_and_scalar_workgroup_at_the_cap(trips, K, p, mode, recompute, scalars):
    """head_bwd_kernel<1 / 2 / 4, BN>: K = 36, 128, 256.  scalars: the grid has one workgroup more, which does the step's scalar
    work; the row loop must stride by the grid WITHOUT it."""
    c = caps()
    B = head_bwd_rows(c, trips)
    assert_head_bwd_past_cap(B, c, trips)
    inp, want = head_bn_case(B, K, p, mode)
    got, written = head_bn_hip(inp, recompute, scalars)
    extra = [("loss mean", written[0], written[1], (2e-6, 1e-6))] if scalars else []  # (test_bce_mean_vs_torch's bound)
    check(f"head backward BN B={B} K={K} p={p} {mode}" + (" recompute" if recompute else "") + (" +scalars" if scalars else ""),
          pairs(got, want, head_bn_tols(B)) + extra)


def test_wrappers_refuse_the_chain_and_the_batchnorm_form_past_one_trip(monkeypatch):
    """rh_head_bnact_fwd and the BatchNorm form of the head's backward cannot make a second trip through the Python wrappers:
    ops.mlp_chain_ok refuses B > 4096 (one trip of the forward is 32768 rows), and _HeadFn.backward takes rh_head_bwd_bn only
    while rh_head_nblocks(B) <= 128, half the cap."""
    from torch_rechub_amd import _lib, ops
    from torch_rechub_amd.basic.layers import MLP
    c = caps()
    B = head_fwd_rows(c)
    assert_head_fwd_past_cap(B, c)
    torch.manual_seed(5)
    mlp = MLP(40, output_layer=True, dims=[32], dropout=0.2, activation="relu").to(dev()).train()
    mods = list(mlp.mlp)
    blocks = MLP._chain_blocks(mods[:-1])
    assert blocks and len(blocks) == 1
    x = torch.randn(B, 40, device=dev())
    assert ops.mlp_chain_ok(x[:1000], blocks, mods[-1], ())  # the same modules below the cap: the chain runs
    assert not ops.mlp_chain_ok(x, blocks, mods[-1], ())
    largest = max(b for b in (1 << s for s in range(1, 16)) if ops.mlp_chain_ok(x[:b], blocks, mods[-1], ()))
    assert ceil_div(largest, 16) < c["head_fwd"] and _lib.call("rh_head_nblocks", largest) <= 128 < c["head_bwd"]
    calls = []
    real = ops.mlp_chain_sigmoid
    monkeypatch.setattr(ops, "mlp_chain_sigmoid", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    y = mlp.sigmoid_head(x.requires_grad_())
    y.sum().backward()
    torch.cuda.synchronize()
    ops.check_errors()
    assert not calls and y.shape == (B,) and bool(torch.isfinite(y).all()) and bool(torch.isfinite(x.grad).all())


# ---- BatchNorm1d + ReLU / PReLU + Dropout on the three-launch path: the apply pass past its cap ---------------------------------
# test_bn_relu_dropout_vs_torch_modules (ReLU) and test_mlp_batchnorm_prelu_dropout_epilogue (PReLU; its parameter bound
# 2e-4 max|want| + 2e-5 max over all gradients is taken per element and per quantity here, which is never wider)
BN_RELU_TOL = {"out": (2e-5, 2e-6), "dx": (1e-4, 1e-5), "dgamma": (1e-4, 1e-5), "dbeta": (1e-4, 1e-5),
               "running_mean": (1e-5, 1e-6), "running_var": (2e-5, 1e-6)}
BN_PRELU_TOL = {"out": (1e-4, 1e-5), "dx": (2e-4, 2e-5), "dgamma": (2e-4, 2e-5), "dbeta": (2e-4, 2e-5), "dslope": (2e-4, 2e-5),
                "running_mean": (1e-4, 1e-5), "running_var": (1e-4, 1e-5)}
BN_EPS = 1e-5


@functools.lru_cache(maxsize=None)
def bn_act_case(B, C, act, p, slope=0.25):
    g = torch.Generator().manual_seed(B + C + len(act))
    h = torch.randn(B, C, generator=g) * 2 + torch.randn(C, generator=g) * 3
    gamma, beta = torch.rand(C, generator=g) + 0.5, torch.randn(C, generator=g) * 0.5

    def bn_of(x):
        return (x - x.mean(0)) / torch.sqrt(x.var(0, unbiased=False) + BN_EPS) * gamma.double() + beta.double()

    away_from_kink(h, bn_of)
    keep = torch.from_numpy(host_keep(SEED, C0, B * C, p).reshape(B, C).astype(F64)) if p > 0 else None
    inp = dict(h=h, gamma=gamma, beta=beta, gy=torch.randn(B, C, generator=g), keep=keep, p=p, act=act,
               slope=torch.tensor([slope]) if act == "prelu" else None)
    return inp, bn_act_eager(inp, torch.float64)


def batch_norm(h, gamma, beta, eps=BN_EPS):
    """nn.BatchNorm1d in training mode on fresh running statistics (0, 1; momentum 0.1): output, running mean, running variance."""
    B = h.shape[0]
    mean, var = h.mean(0), h.var(0, unbiased=False)
    bn = (h - mean) / torch.sqrt(var + eps) * gamma + beta
    return bn, 0.1 * mean.detach(), 0.9 + 0.1 * var.detach() * (B / (B - 1.0))


def bn_act_eager(inp, dtype):
    h, gamma, beta = (inp[k].to(dtype).requires_grad_() for k in ("h", "gamma", "beta"))
    bn, rm, rv = batch_norm(h, gamma, beta)
    if inp["act"] == "relu":
        a = torch.relu(bn)
    else:
        slope = inp["slope"].to(dtype).requires_grad_()
        a = torch.where(bn > 0, bn, slope * bn)
    y = a if inp["keep"] is None else a * inp["keep"].to(dtype) / (1.0 - inp["p"])
    y.backward(inp["gy"].to(dtype))
    res = dict(out=y.detach(), dx=h.grad, dgamma=gamma.grad, dbeta=beta.grad, running_mean=rm, running_var=rv)
    if inp["act"] == "prelu":
        res["dslope"] = slope.grad
    return res


def bn_module(inp, d):
    C = inp["gamma"].numel()
    bn = torch.nn.BatchNorm1d(C, eps=BN_EPS).to(d).train()
    with torch.no_grad():
        bn.weight.copy_(inp["gamma"])
        bn.bias.copy_(inp["beta"])
    return bn


def bn_act_hip(inp):
    from torch_rechub_amd import ops
    d = dev()
    B, C = inp["h"].shape
    bn = bn_module(inp, d)
    h = inp["h"].to(d).requires_grad_()
    ops._dropout_rng(d).copy_(torch.tensor([SEED, C0, 0, 0], dtype=torch.int64))
    poison((B, C), (B, C))
    if inp["act"] == "relu":
        y = ops.bn_relu_dropout(h, bn, inp["p"])
    else:
        act = torch.nn.PReLU(init=float(inp["slope"])).to(d)
        assert ops.bn_prelu_dropout_ok(h, bn, act)
        y = ops.bn_prelu_dropout(h, bn, act, inp["p"])
    y.backward(inp["gy"].to(d))
    torch.cuda.synchronize()
    ops.check_errors()
    assert int(ops._dropout_rng(d)[1]) == C0 + 1 and int(bn.num_batches_tracked) == 1
    res = dict(out=y.detach(), dx=h.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, running_mean=bn.running_mean,
               running_var=bn.running_var)
    if inp["act"] == "prelu":
        res["dslope"] = act.weight.grad
    return res


@pytest.mark.parametrize("act,p", [("relu", 0.0), ("relu", 0.25), ("prelu", 0.0), ("prelu", 0.25)])
def test_batchnorm_activation_apply_pass_past_its_cap_forward_and_backward(act, p):
    from torch_rechub_amd import _lib
    c = caps()
    C = 36
    B = apply_rows(c, C)
    assert_past_cap(ceil_div(B * C, 1024), query("rh_bn_apply_nblocks", B * C), c["apply"], "BatchNorm apply")
    assert B * C >= c["apply"] * 1024 + 1024 * 3 + 7
    # the three-launch path (not the fused finalize + apply of batch-sized inputs), through the row count: its statistics pass
    # runs at most 512 row chunks per 32-column slab, the fused path would run one per 64 rows
    slabs = ceil_div(C, 32)
    assert _lib.call("rh_bn_prelu_nblocks", B, C) <= 512 * slabs < ceil_div(B, 64) * slabs
    inp, want = bn_act_case(B, C, act, p)
    if p > 0:
        rate = 1.0 - float(inp["keep"].mean())
        assert abs(rate - p) < 4 * (p * (1 - p) / inp["keep"].numel()) ** 0.5, rate
    check(f"bn_{act}_dropout {B}x{C} p={p}", pairs(bn_act_hip(inp), want, BN_RELU_TOL if act == "relu" else BN_PRELU_TOL))


# ---- PReLU -------------------------------------------------------------------------------------------------------------------
# test_prelu_single_slope_vs_torch: output and input gradient bit-equal to the same expression in float32 (here eager torch on the
# CPU; against float64 that is one rounding of slope * x, 2^-24), the slope gradient rtol 1e-4, atol 1e-4 max(1, |want|)
PRELU_TOL = {"out": (1e-7, 1e-9), "gx": (1e-7, 1e-9), "gslope": (1e-4, 1e-4)}


@functools.lru_cache(maxsize=None)
def prelu_case(n, slope):
    g = torch.Generator().manual_seed(n)
    x = torch.randn(n, generator=g)
    x[0], x[-1] = 0.0, -1.5  # the kink (forward 0, backward the slope branch); the last element of the n % 4 remainder negative
    inp = dict(x=x, gy=torch.randn(n, generator=g), slope=torch.tensor([slope]))
    return inp, prelu_eager(inp, torch.float64)


def prelu_eager(inp, dtype):
    x, a = inp["x"].to(dtype).requires_grad_(), inp["slope"].to(dtype).requires_grad_()
    y = torch.where(x > 0, x, a * x)
    y.backward(inp["gy"].to(dtype))
    return dict(out=y.detach(), gx=x.grad, gslope=a.grad)


@pytest.mark.parametrize("slope", [0.25, -0.6])
def test_prelu_ragged_second_trip_and_remainder(slope):
    from torch_rechub_amd import _lib, ops
    c = caps()
    n = prelu_numel(c)
    assert n % 4 == 3
    assert_past_cap(ceil_div(n // 4, 256), _lib.call("rh_prelu_nblocks", n), c["prelu"], "prelu")
    inp, want = prelu_case(n, slope)
    d = dev()
    x, a = inp["x"].to(d).requires_grad_(), inp["slope"].to(d).requires_grad_()
    assert x.dim() == 1
    poison((n,), (n,), (c["prelu"],))
    y = ops.prelu(x, a)
    y.backward(inp["gy"].to(d))
    torch.cuda.synchronize()
    got = dict(out=y.detach(), gx=x.grad, gslope=a.grad)
    check(f"prelu n={n} slope={slope}", pairs(got, want, PRELU_TOL))
    same = prelu_eager(inp, torch.float32)
    assert torch.equal(got["out"].cpu(), same["out"]) and torch.equal(got["gx"].cpu(), same["gx"])


# ---- Dice ----------------------------------------------------------------------------------------------------------------------
# test_dice_kernel_vs_reference_formula, test_bn_dice_folded_vs_modules, test_bn_dice_head_vs_modules
DICE_TOL = {"out": (2e-5, 2e-6), "gx": (1e-4, 1e-5), "galpha": (1e-4, 1e-5)}
BN_DICE_TOL = {"out": (2e-4, 5e-6), "dh": (1e-3, 2e-5), "dgamma": (1e-3, 2e-5), "dbeta": (1e-3, 2e-5), "dalpha": (1e-3, 1e-4),
               "d_head_w": (1e-3, 2e-5), "d_head_b": (1e-3, 2e-5), "running_mean": (1e-5, 1e-6), "running_var": (2e-5, 1e-6)}
DICE_EPS = 1e-3


def offset_view(t, off):
    """The same (N, C) values, contiguous, starting ``off`` floats into a device buffer: off = 1 is only 4-byte aligned."""
    buf = torch.empty(t.numel() + 4, dtype=torch.float32, device=dev())
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and (v.data_ptr() % 16 != 0) == (off % 4 != 0)
    return v


@functools.lru_cache(maxsize=None)
def dice_case(N, C, kind):
    """kind: "plain" (Dice), "bn" (Dice(BatchNorm1d(h))) or "head" (Linear(C, 1) on top)."""
    g = torch.Generator().manual_seed(N + C + len(kind))
    inp = dict(x=torch.randn(N, C, generator=g) * 1.5 + (0.3 if kind == "plain" else torch.randn(C, generator=g)),
               alpha=torch.randn(1, generator=g), kind=kind,
               gy=torch.randn(N, 1 if kind == "head" else C, generator=g))
    if kind != "plain":
        inp.update(gamma=torch.rand(C, generator=g) + 0.5, beta=torch.randn(C, generator=g))
    if kind == "head":
        inp.update(w=(torch.rand(1, C, generator=g) * 2 - 1) / np.sqrt(C), b=(torch.rand(1, generator=g) * 2 - 1) / np.sqrt(C))
    return inp, dice_eager(inp, torch.float64)


def dice_eager(inp, dtype):
    x, alpha = inp["x"].to(dtype).requires_grad_(), inp["alpha"].to(dtype).requires_grad_()
    if inp["kind"] == "plain":
        y = _dice_ref(x, alpha, DICE_EPS)
        y.backward(inp["gy"].to(dtype))
        return dict(out=y.detach(), gx=x.grad, galpha=alpha.grad)
    gamma, beta = inp["gamma"].to(dtype).requires_grad_(), inp["beta"].to(dtype).requires_grad_()
    bn, rm, rv = batch_norm(x, gamma, beta)
    y = _dice_ref(bn, alpha, DICE_EPS)
    res = {}
    if inp["kind"] == "head":
        w, b = inp["w"].to(dtype).requires_grad_(), inp["b"].to(dtype).requires_grad_()
        y = y @ w.t() + b
    y.backward(inp["gy"].to(dtype))
    if inp["kind"] == "head":
        res.update(d_head_w=w.grad, d_head_b=b.grad)
    res.update(out=y.detach(), dh=x.grad, dgamma=gamma.grad, dbeta=beta.grad, dalpha=alpha.grad, running_mean=rm, running_var=rv)
    return res


def dice_hip(inp, off):
    from torch_rechub_amd import ops
    d = dev()
    N, C = inp["x"].shape
    x = offset_view(inp["x"].to(d), off).requires_grad_()
    alpha = inp["alpha"].to(d).requires_grad_()
    gy = inp["gy"].to(d)
    poison((N, C), (N, C))
    if inp["kind"] == "plain":
        y = ops.dice(x, alpha, DICE_EPS)
        assert y.data_ptr() % 16 == 0  # (only the input is misaligned: that alone must send C = 64 / 128 to the scalar kernel)
        y.backward(gy)
        torch.cuda.synchronize()
        ops.check_errors()
        return dict(out=y.detach(), gx=x.grad, galpha=alpha.grad)
    bn = bn_module(inp, d)
    res = {}
    if inp["kind"] == "bn":
        assert ops.bn_dice_ok(x, bn, None)
        y = ops.bn_dice(x, bn, alpha, DICE_EPS)
    else:
        lin = torch.nn.Linear(C, 1).to(d)
        with torch.no_grad():
            lin.weight.copy_(inp["w"])
            lin.bias.copy_(inp["b"])
        assert ops.bn_dice_ok(x, bn, None) and ops.bn_dice_head_ok(C, bn, None, lin)
        y = ops.bn_dice_head(x, bn, alpha, DICE_EPS, lin)
    y.backward(gy)
    torch.cuda.synchronize()
    ops.check_errors()
    if inp["kind"] == "head":
        res.update(d_head_w=lin.weight.grad, d_head_b=lin.bias.grad)
    res.update(out=y.detach(), dh=x.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, dalpha=alpha.grad,
               running_mean=bn.running_mean, running_var=bn.running_var)
    assert int(bn.num_batches_tracked) == 1
    return res


@pytest.mark.parametrize("C,off", [(36, 0), (200, 0), (520, 0), (64, 1), (128, 1)])
def test_dice_scalar_kernel_second_trip_forward_and_backward(C, off):
    """C = 36: one element per lane, lanes 36 .. 63 idle; 200: four, not FULL; 520: sixteen; 64 / 128 from a view that is only 4-byte
    aligned: the scalar kernel (one, two elements per lane, FULL) in place of the vector kernel."""
    from torch_rechub_amd import _lib
    c = caps()
    N = dice_rows(c, False)
    assert_past_cap(ceil_div(N, 4), _lib.call("rh_dice_nblocks", N), c["dice"], "dice")
    inp, want = dice_case(N, C, "plain")
    check(f"dice N={N} C={C} offset={off}", pairs(dice_hip(inp, off), want, DICE_TOL))


@pytest.mark.parametrize("kind", ["bn", "head"])
@pytest.mark.parametrize("C,off", [(36, 0), (200, 0), (64, 1), (128, 1), (64, 0), (128, 0)])
def test_folded_batchnorm_dice_at_the_cap_of_the_statistics_pass(C, off, kind):
    """off = 1: the scalar kernel; C = 64 / 128 with off = 0: the vector kernel (16 / 32 lanes per row), whose large cases so far
    were multiples of its rows per pass."""
    from torch_rechub_amd import _lib
    c = caps()
    N = dice_rows(c, True)
    assert_past_cap(ceil_div(N, 4), _lib.call("rh_bn_dice_stats_blocks", N), c["dice_stats"], "folded dice statistics")
    inp, want = dice_case(N, C, kind)
    check(f"bn_dice{'_head' if kind == 'head' else ''} N={N} C={C} offset={off}", pairs(dice_hip(inp, off), want, BN_DICE_TOL))


if __name__ == "__main__":
    # float32 eager torch on the CPU through the same comparison, for every shape above at today's caps
    c = TODAY
    B = head_fwd_rows(c)
    for K, bias, nextra, mode, _ in [(5, True, 0, "gy", 0), (5, False, 1, "t", 0), (36, True, 1, "t", 0), (36, False, 2, "gy", 0),
                                     (260, False, 2, "both", 0), (260, True, 0, "t", 0)]:
        inp, want = head_case(B, K, bias, nextra, mode)
        check(f"float32 eager head B={B} K={K} {mode}", pairs(head_eager(inp, torch.float32), want, head_tols(B)))
    inp, want = head_case(B, 36, True, 1, "t", clamp=5)
    check(f"float32 eager head loss clamp B={B}", pairs(head_eager(inp, torch.float32), want, head_tols(B)))
    for trips, K, mode in [(3, 5, "gy"), (3, 36, "t"), (3, 130, "both"), (3, 200, "gy"), (3, 260, "t"), (3, 520, "both"),
                           (5, 5, "both"), (5, 130, "t"), (5, 260, "gy")]:
        B = head_bwd_rows(c, trips)
        inp, want = head_case(B, K, True, 1, mode)
        check(f"float32 eager head backward B={B} K={K} {mode}", pairs(head_eager(inp, torch.float32), want, head_tols(B)))
    for trips, K, p, mode, _, _ in HEAD_BN_CASES:
        B = head_bwd_rows(c, trips)
        inp, want = head_bn_case(B, K, p, mode)
        check(f"float32 eager head backward BN B={B} K={K} p={p} {mode}",
              pairs(head_bn_eager(inp, torch.float32), want, head_bn_tols(B)))
    for act, p in [("relu", 0.0), ("relu", 0.25), ("prelu", 0.0), ("prelu", 0.25)]:
        inp, want = bn_act_case(apply_rows(c, 36), 36, act, p)
        check(f"float32 eager bn_{act}_dropout p={p}",
              pairs(bn_act_eager(inp, torch.float32), want, BN_RELU_TOL if act == "relu" else BN_PRELU_TOL))
    for slope in (0.25, -0.6):
        inp, want = prelu_case(prelu_numel(c), slope)
        check(f"float32 eager prelu slope={slope}", pairs(prelu_eager(inp, torch.float32), want, PRELU_TOL))
    for C in (36, 200, 520, 64, 128):
        inp, want = dice_case(dice_rows(c, False), C, "plain")
        check(f"float32 eager dice C={C}", pairs(dice_eager(inp, torch.float32), want, DICE_TOL))
    for kind in ("bn", "head"):
        for C in (36, 200, 64, 128):
            inp, want = dice_case(dice_rows(c, True), C, kind)
            check(f"float32 eager {kind} dice C={C}", pairs(dice_eager(inp, torch.float32), want, BN_DICE_TOL))
