"""The sequence kernels DIN and DIEN train on -- gather + masked pooling (csrc/seqpool.hip), the two memory-bound ends of the
ActivationUnit (``att_kernel`` of csrc/din.hip), its first layer on the register-built operand with the BatchNorm statistics as an
epilogue (csrc/dinmlp.hip) and the AUGRU recurrence (csrc/augru.hip) -- at every lane split and loop trip, against float64.

Every case first asks the library which split its launch takes -- ``rh_seq_pool_split`` and ``rh_din_att_split`` are wrappers of
the host functions the launches themselves take it from, ``rh_din_att_l1_chunk_rows`` is the one the first layer's launch calls --
and asserts the regime its row of the tables names before it compares anything.  LPR = D / 4 lanes on a row, LS = position groups.

  seq_pool (U = 8 positions per lane group and trip, nll = ceil(L / LS), trips = ceil(nll / 8))
    D     L    LS   nll  trips
    128   16   2    8    1      the last full single trip
    128   17   2    9    2      the second trip holds one position, for ls = 0 only
    128   40   2    20   3
    64    33   4    9    2
    32    65   8    9    2
    16    128  16   8    1
    16    129  16   9    2
    8     129  16   9    2
    4     300  16   19   3
    every row in sum / mean / concat x padding_idx 0 / None x B = 5 / 70 (neither a multiple of the samples per workgroup), int64,
    vocabulary 50 (ids repeat inside a sample and across samples: the backward's atomics of both trips meet in one row), lengths
    in [0, L] with a fully padded sample (mean = 0) and a full one (padding_idx 0; without a padding_idx nothing is masked: every
    position holds a drawn id, row 0 included -- see seq_case); (64, 33) and (16, 129) also with int32 indices and with an
    ``idx`` that is the transposed view of an (L, B) tensor (stride(1) = B); one case with an id >= vocab in the second trip

  attention ends (att_kernel<LPR, LS, MODE>, four modes), LS by (D, L):
    D \\ L       1   3   4   5   15  16  17  37
    4, 8, 16    1   1   4   4   4   16  16  16
    32, 64      1   1   4   4   4   4   4   4
    128         1   1   1   1   1   1   1   1
    every cell at B = 1 and 67, from a contiguous history / target and from the ``[:, 1]`` slice of a (B, 2, L, D) buffer; one
    pooling case whose weights are a masked softmax's (exactly 0 on the padded tail)

  first attention layer (32-row tiles folded into a chunk's (count, mean, M2) by Chan's formula; chunk = workgroup)
    R = B L             chunk rows   tiles per chunk      cases
    63   (7 x 9)        32           1 (32 and 31 rows)   all twelve (D, N): D = 4, 8, 16 x N = 64, 128, 192, 256
    1, 32               32           1                    (16, 128); also bias = None, and a history with sample stride
                                                          (L + 3) D beside a target that is a column slice
    24700 (247 x 100)   64           2, last chunk 32+28  (16, 256), (4, 64); (16, 256) with every bias + OFFSET; the
                                                          ActivationUnit on dims = [64] (rh_bn_stats_from_partial + bn_dice_head
                                                          on 64-row chunks) with the BatchNorm's running statistics
    49500 (500 x 99)    96           3, last chunk 32+28  (8, 128)

  AUGRU, attention weights AND state bias together: D = 4, 8, 16, 32 x B = SPW - 1, SPW, SPW + 1 (SPW = 64 / (D / 4) samples per
    wavefront = workgroup) x T = 1, 2, 3, 17 (T = 2: the backward's prologue reads h_all[0], the loop's prefetch nothing); sample 0
    of every case has all weights 0 (states and d_xw exactly 0); saturated gates: xw x 40 at a random third of the (sample, step,
    gate) positions, T = 17, B = SPW + 1, the float64 update gate asserted below 1e-12 and above 1 - 1e-12 somewhere

References and tolerances.  oracle/ctr_oracle.py (float64) for seq_pool and AUGRU, float64 autograd on the CPU for the attention
ends, float64 ``linear`` on the materialised [t, h, t - h, t * h] and float64 statistics over the same rows for the first layer.
|got - want| <= atol + rtol |want|, every element of every output, (rtol, a) with atol = a max(1, max|want|) from the existing test
of the same quantity:
  seq_pool   test_seq_pool_vs_oracle: out (1e-5, 1e-6), table gradient (2e-5, 2e-6); concat bit-exact (test_seq_pool_golden)
  att ends   test_din_attention_ends_vs_reference_formula: the copied halves of att_input bit-exact, att_input (1e-6, 1e-6), pooled /
             g_hist / g_w (2e-5, 2e-6), g_tgt (2e-5, 1e-5)
  att l1     test_din_att_l1_matches_linear_on_materialised_operand_and_chunk_statistics: z absolute 2e-5 max(1, max|z|), chunk sums
             rtol 1e-5 + 1e-3 absolute, chunk M2 rtol 1e-4 + 1e-3 absolute;  the ActivationUnit:
             test_activation_unit_first_layer_on_register_built_operand's, running mean (1e-5, 1e-6) / variance (2e-5, 1e-6) of
             test_bn_relu_dropout_vs_torch_modules
  augru      test_augru_recurrence_forward_and_backward_through_time: states (1e-4, 1e-5), gradients (5e-4, 1e-5); the saturated
             case under the same (its vanishing gradients are compared on the a max|want| floor)
The offset case: OFFSET = 30 on every column of the bias, the float64 statistics taken from the kernel's own z (z itself carries a
float32 rounding of a number near 30).  The float32 tile-by-tile computation on the CPU stays at 0.046 of the tolerance
there (M2; sums 0.026), under one half: 30 was not reduced.
No bound was widened and no element is excluded.

float32 eager on the CPU through the same comparison (``python tests/test_gpu_sequence_shapes.py``: numpy float32 through the oracle
for seq_pool and AUGRU, float32 torch autograd for the attention ends, float32 ``linear`` and the tile-by-tile Chan merge in float32
for the first layer), worst error / tolerance per family: seq_pool 0.390 [table gradient, D = 4, L = 300, B = 70, sum, no
padding_idx: 420 sequential additions per row], att ends 0.048 [pooled], att l1 0.031 [chunk sums, R = 24700] and 0.014 for the
running mean, the offset case 0.046 [M2], augru 0.012 [states], saturated 0.010: under one half of every existing tolerance.

Worst error / tolerance per family on the MI355X (the ``SEQS`` lines; the worst quantity in brackets), all 121 tests passing:
  seq_pool   0.148 [table gradient, D = 4, L = 300, B = 70, sum, no padding_idx]; every concat output bit-equal
  att ends   0.055 [g_w, D = 128, L = 5, B = 1, strided]; the copied halves bit-equal
  att l1     single tile 0.020 [z, bias = None]; two and three tiles per chunk 0.023 [chunk sums, (16, 256)]; the offset case 0.032
             [M2; sums 0.018, z 0.005]; running statistics behind the 64-row chunks 0.003
  augru      0.016 [d_state_bias, D = 8, T = 17, B = 32]; saturated gates 0.016 [d_xw, D = 8]
Found by this module: no defect -- every kernel passed as it was (the two split queries are new; the launches take the split
from the functions behind them).  That the cases bite was tried on scratch builds with one arithmetic line of a kernel changed
each, this module and test_gpu_kernels.py run once against each (error / tolerance on the MI355X; test_gpu_kernels.py passed all
276 of its tests on all four builds, so none of the old cases sees any of them):
  seq_pool_kernel's forward loop bounded by ``min(nll, U)``:   all 21 cases of the seven rows with 2 or 3 trips fail (out 5114 ..
                                                               235 739; concat not finite -- unwritten rows -- or not bit-equal) and
                                                               the 3 bad-id cases (the id is never read: no IndexError); the 6
                                                               cases of the two one-trip rows pass, as they must
  the same for its backward loop:                              the same 21 cases fail (table gradient 4774 .. 211 353); the bad-id
                                                               cases, forward only, pass
  din_att_l1_kernel's merge without ``dlt * dlt * (cnt * nrows / tot)``:  the four cases with 2 or 3 tiles per chunk fail (M2 8099 ..
                                                               8631, the offset case 8519) and the ActivationUnit on 64-row chunks
                                                               (attention output); the 16 single-tile cases pass
  augru_fwd_kernel reading ``ub`` only when ``attn == nullptr``:  all 16 (D, T) cases and the 4 saturated ones fail (states 4831 ..
                                                               44 374, gradients 186 .. 16 157; T = 1: the states alone, the
                                                               backward recomputes its gates with the bias)
"""
import functools
import os
import sys

if __name__ == "__main__":  # python tests/test_gpu_sequence_shapes.py: the float32-eager figures, on the CPU
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import pytest
import torch

from oracle import ctr_oracle as O
from test_gpu_dcn_trips import ceil_div, query
from test_gpu_kernels import close, dev

pytestmark = pytest.mark.gpu
F64, F32 = np.float64, np.float32
EXACT = (0.0, 0.0)


def _np(x):
    return x.detach().cpu().numpy().astype(F64) if torch.is_tensor(x) else np.asarray(x, F64)


def scaled(want, a):
    """The atol of test_gpu_kernels.close: a max(1, max|want|)."""
    want = _np(want)
    return a * max(1.0, float(np.abs(want).max()) if want.size else 1.0)


def figure(got, want, rtol, atol, what):
    """max |got - want| / (atol + rtol |want|) over every element; for rtol = atol = 0: 0 if bit-equal, else inf."""
    got, want = _np(got), _np(want)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    assert np.isfinite(got).all(), f"{what}: not finite"
    if rtol == 0.0 and atol == 0.0:
        return 0.0 if np.array_equal(got, want) else float("inf")
    return float((np.abs(got - want) / (atol + rtol * np.abs(want))).max()) if want.size else 0.0


WORST = {}  # family -> (figure, case, quantity): what the CPU run prints at its end


def check(family, case, pairs):
    """pairs: (what, got, want, (rtol, a)) with atol = a max(1, max|want|), or (what, got, want, (rtol, atol, "abs")).
    Prints every figure, then asserts all of them."""
    figures = []
    for what, got, want, tol in pairs:
        atol = tol[1] if len(tol) == 3 else (scaled(want, tol[1]) if tol[1] else 0.0)
        figures.append((what, figure(got, want, tol[0], atol, f"{case} {what}")))
    worst = max(figures, key=lambda f: f[1])
    print(f"SEQS {family} {case}: worst {worst[1]:.3f} [{worst[0]}]  " + " ".join(f"{w}={r:.3f}" for w, r in figures))
    if worst[1] >= WORST.get(family, (-1.0,))[0]:
        WORST[family] = (worst[1], case, worst[0])
    bad = [(w, r) for w, r in figures if not r <= 1.0]
    assert not bad, f"{case}: error / tolerance {bad}"
    for what, got, want, tol in pairs:  # and the suite's own comparison, where the bound has its form
        if len(tol) == 2 and tol != EXACT:
            close(got, _np(want), rtol=tol[0], atol_scale=tol[1], what=f"{case} {what}")
    return worst


def pairs(got, want, tols):
    assert got.keys() == want.keys(), (sorted(got), sorted(want))
    return [(k, got[k], want[k], tols[k]) for k in want]


def sync_and_check():
    from torch_rechub_amd import ops
    torch.cuda.synchronize()
    ops.check_errors()


def test_split_queries_refuse_what_the_launches_refuse():
    for name, n in (("rh_seq_pool_split", 3), ("rh_din_att_split", 2)):
        with pytest.raises(RuntimeError, match="embed_dim 12 unsupported"):
            query(name, 12, 5, n=n)
        with pytest.raises(RuntimeError, match=name):
            query(name, 16, 0, n=n)


# ---- seq_pool ----------------------------------------------------------------------------------------------------------------
# D, L, LS, nll, trips
SEQ_ROWS = [(128, 16, 2, 8, 1), (128, 17, 2, 9, 2), (128, 40, 2, 20, 3), (64, 33, 4, 9, 2), (32, 65, 8, 9, 2), (16, 128, 16, 8, 1),
            (16, 129, 16, 9, 2), (8, 129, 16, 9, 2), (4, 300, 16, 19, 3)]
SEQ_VARIANT_ROWS = {(64, 33), (16, 129)}  # also int32 indices and a transposed index view
SEQ_MODES = ["sum", "mean", "concat"]
SEQ_VOCAB = 50
SEQ_TOL = {"out": (1e-5, 1e-6), "grad": (2e-5, 2e-6)}
SEQ_TOL_CONCAT = {"out": EXACT, "grad": (2e-5, 2e-6)}


def assert_seq_split(D, L, LS, nll, trips):
    assert query("rh_seq_pool_split", D, L, n=3) == (D // 4, LS, trips), (D, L)
    assert ceil_div(L, LS) == nll and ceil_div(nll, 8) == trips


@functools.lru_cache(maxsize=None)
def seq_case(D, L, B, mode, pad):
    g = torch.Generator().manual_seed(D * 100000 + L * 100 + B)
    table = torch.randn(SEQ_VOCAB, D, generator=g) * 0.5
    if pad is not None:
        table[pad].zero_()
    lens = torch.randint(0, L + 1, (B,), generator=g)
    lens[0], lens[1] = 0, L  # a fully padded sample (count 0 -> mean 0) and one that is live to its last position
    if pad is not None:
        idx = torch.randint(1, SEQ_VOCAB, (B, L), generator=g)
        idx[torch.arange(L)[None, :] >= lens[:, None]] = pad
    else:
        # nothing is masked without a padding_idx: row 0 is an ordinary row and there is no tail.  (A tail of id 0 would be
        # ~4500 additions into one gradient row, which float32 numpy itself misses the gradient bound on, 1.5 - 2.6 x.)
        idx = torch.randint(0, SEQ_VOCAB, (B, L), generator=g)
    gy = torch.randn((B, L, D) if mode == "concat" else (B, D), generator=g)
    inp = dict(table=table, idx=idx, gy=gy, lens=lens)
    return inp, seq_eager(inp, mode, pad, F64)


def seq_eager(inp, mode, pad, dtype):
    table, idx = inp["table"].numpy().astype(dtype), inp["idx"].numpy()
    return dict(out=O.seq_pool(table, idx, mode, pad),
                grad=O.seq_pool_backward(table.shape, idx, mode, inp["gy"].numpy().astype(dtype), pad))


def seq_hip(inp, mode, pad, variant="int64"):
    from torch_rechub_amd import ops
    w = torch.nn.Parameter(inp["table"].to(dev()))
    idx = inp["idx"]
    if variant == "int32":
        idx = idx.to(torch.int32).to(dev())
    elif variant == "transposed":
        idx = idx.t().contiguous().to(dev()).t()
        assert idx.shape == inp["idx"].shape and idx.stride(1) == idx.shape[0] != 1 and idx.stride(0) == 1
    else:
        idx = idx.to(dev())
    y = ops.seq_pool(w, idx, mode, pad)
    y.backward(inp["gy"].to(dev()))
    sync_and_check()
    return dict(out=y.detach(), grad=w.grad)


@pytest.mark.parametrize("mode", SEQ_MODES)
@pytest.mark.parametrize("D,L,LS,nll,trips", SEQ_ROWS)
def test_seq_pool_every_trip_of_the_gather_loop(D, L, LS, nll, trips, mode):
    assert_seq_split(D, L, LS, nll, trips)
    variants = ["int64"] + (["int32", "transposed"] if (D, L) in SEQ_VARIANT_ROWS else [])
    for pad in (0, None):
        for B in (5, 70):
            assert B % (256 // 64) != 0
            inp, want = seq_case(D, L, B, mode, pad)
            lens = inp["lens"]
            assert int(lens.min()) == 0 and int(lens.max()) == L
            if trips > 1 and B == 70:  # live positions that end inside the second trip, and ids met again there
                assert bool(((lens > 8 * LS) & (lens < min(L, 16 * LS))).any()) or L - 8 * LS < 3
            for variant in variants:
                check("seq_pool", f"D={D} L={L} B={B} {mode} pad={pad} {variant}",
                      pairs(seq_hip(inp, mode, pad, variant), want, SEQ_TOL_CONCAT if mode == "concat" else SEQ_TOL))


@pytest.mark.parametrize("mode", SEQ_MODES)
def test_seq_pool_flags_an_id_past_the_vocabulary_in_the_second_trip(mode):
    """The kernel reads row 0 in place of the bad id (nothing faults) and raises the error word; without a padding_idx row 0
    is an ordinary row, so the oracle on the indices with 0 in that place is what every sample, the bad one included, must hold."""
    from torch_rechub_amd import ops
    D, L, LS, nll, trips = 64, 33, 4, 9, 2
    assert_seq_split(D, L, LS, nll, trips)
    inp, _ = seq_case(D, L, 70, mode, None)
    bad_b, bad_l = 37, 8 * LS  # the first position of the second trip, lane group ls = 0
    assert (bad_l // LS) // 8 == 1
    idx = inp["idx"].clone()
    idx[bad_b, bad_l] = SEQ_VOCAB + 3
    read = inp["idx"].clone()
    read[bad_b, bad_l] = 0
    want = O.seq_pool(inp["table"].numpy().astype(F64), read.numpy(), mode, None)
    ops.check_errors()
    y = ops.seq_pool(inp["table"].to(dev()), idx.to(dev()), mode, None)
    torch.cuda.synchronize()
    with pytest.raises(IndexError, match="out of range"):
        ops.check_errors()
    ops.check_errors()  # the word was cleared
    check("seq_pool", f"id past the vocabulary, {mode}", [("out", y, want, EXACT if mode == "concat" else SEQ_TOL["out"])])


# ---- the attention ends ------------------------------------------------------------------------------------------------------
ATT_LS = {4: (1, 1, 4, 4, 4, 16, 16, 16), 8: (1, 1, 4, 4, 4, 16, 16, 16), 16: (1, 1, 4, 4, 4, 16, 16, 16),
          32: (1, 1, 4, 4, 4, 4, 4, 4), 64: (1, 1, 4, 4, 4, 4, 4, 4), 128: (1, 1, 1, 1, 1, 1, 1, 1)}
ATT_L = (1, 3, 4, 5, 15, 16, 17, 37)
ATT_TOL = {"copies": EXACT, "att_input": (1e-6, 1e-6), "pooled": (2e-5, 2e-6), "g_hist": (2e-5, 2e-6), "g_tgt": (2e-5, 1e-5),
           "g_w": (2e-5, 2e-6)}


def assert_att_split(D, L):
    LS = ATT_LS[D][ATT_L.index(L)]
    assert query("rh_din_att_split", D, L, n=2) == (D // 4, LS), (D, L)
    return LS


@functools.lru_cache(maxsize=None)
def att_inputs(B, L, D):
    g = torch.Generator().manual_seed(B * 100000 + L * 1000 + D)
    return dict(hist_all=torch.randn(B, 2, L, D, generator=g), tgt_all=torch.randn(B, 2, D, generator=g),
                w=torch.randn(B, L, generator=g), g1=torch.randn(B * L, 4 * D, generator=g), g2=torch.randn(B, D, generator=g))


def att_layout(inp, strided, where=None):
    ha, ta = inp["hist_all"], inp["tgt_all"]
    if where is not None:
        ha, ta = ha.to(where), ta.to(where)
    if strided:
        return ha[:, 1], ta[:, 1]
    return ha[:, 0].contiguous(), ta[:, 0].contiguous()


def att_eager(inp, strided, dtype):
    """cat[t, h, t - h, t * h] and sum_l w_l h_l (models/ranking/din.py:80-81, 92) with autograd."""
    hist, tgt = att_layout(inp, strided)
    B, L, D = hist.shape
    h, t, w = (x.to(dtype).clone().requires_grad_() for x in (hist, tgt, inp["w"]))
    te = t.unsqueeze(1).expand(-1, L, -1)
    att_in = torch.cat([te, h, te - h, te * h], dim=-1).view(-1, 4 * D)
    pooled = (w.unsqueeze(-1) * h).sum(dim=1)
    torch.autograd.backward([att_in, pooled], [inp["g1"].to(dtype), inp["g2"].to(dtype)])
    return dict(copies=att_in.detach()[:, :2 * D], att_input=att_in.detach(), pooled=pooled.detach(), g_hist=h.grad,
                g_tgt=t.grad, g_w=w.grad)


@functools.lru_cache(maxsize=None)
def att_want(B, L, D, strided):
    return att_eager(att_inputs(B, L, D), strided, torch.float64)


def att_hip(inp, strided):
    from torch_rechub_amd import ops
    hist, tgt = att_layout(inp, strided, dev())
    B, L, D = hist.shape
    assert B == 1 or (hist.stride(0) == (2 if strided else 1) * L * D and hist.is_contiguous() != strided)
    h, t = hist.detach().requires_grad_(), tgt.detach().requires_grad_()
    w = inp["w"].to(dev()).requires_grad_()
    a = ops.din_att_input(h, t)
    p = ops.din_att_pool(w, h)
    torch.autograd.backward([a, p], [inp["g1"].to(dev()), inp["g2"].to(dev())])
    sync_and_check()
    return dict(copies=a.detach()[:, :2 * D], att_input=a.detach(), pooled=p.detach(), g_hist=h.grad, g_tgt=t.grad, g_w=w.grad)


@pytest.mark.parametrize("L", ATT_L)
@pytest.mark.parametrize("D", sorted(ATT_LS))
def test_din_attention_ends_at_every_lane_split(D, L):
    LS = assert_att_split(D, L)
    for B in (1, 67):
        for strided in (False, True):
            check("att ends", f"D={D} L={L} LS={LS} B={B}" + (" strided" if strided else ""),
                  pairs(att_hip(att_inputs(B, L, D), strided), att_want(B, L, D, strided), ATT_TOL))


@functools.lru_cache(maxsize=None)
def att_masked_case():
    B, L, D = 67, 37, 16
    g = torch.Generator().manual_seed(B + L + D)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0], lens[1] = 1, L
    live = torch.arange(L)[None, :] < lens[:, None]
    w = torch.randn(B, L, generator=g).masked_fill(~live, float("-inf")).softmax(dim=-1)
    assert bool((w[~live] == 0).all()) and bool((w[live] > 0).all())
    return dict(hist=torch.randn(B, L, D, generator=g), w=w, g2=torch.randn(B, D, generator=g), live=live)


def att_masked_eager(inp, dtype):
    h, w = inp["hist"].to(dtype).clone().requires_grad_(), inp["w"].to(dtype).clone().requires_grad_()
    pooled = (w.unsqueeze(-1) * h).sum(dim=1)
    pooled.backward(inp["g2"].to(dtype))
    return dict(pooled=pooled.detach(), g_hist=h.grad, g_w=w.grad)


def test_din_pooling_with_masked_softmax_weights_exactly_zero_on_the_padded_tail():
    from torch_rechub_amd import ops
    inp = att_masked_case()
    assert query("rh_din_att_split", 16, 37, n=2) == (4, 16)
    h, w = inp["hist"].to(dev()).requires_grad_(), inp["w"].to(dev()).requires_grad_()
    p = ops.din_att_pool(w, h)
    p.backward(inp["g2"].to(dev()))
    sync_and_check()
    got = dict(pooled=p.detach(), g_hist=h.grad, g_w=w.grad)
    check("att ends", "masked softmax weights", pairs(got, att_masked_eager(inp, torch.float64), ATT_TOL))
    assert bool((h.grad.cpu()[~inp["live"]] == 0).all())  # w_l = 0: the history row gets exactly nothing


# ---- the first attention layer -----------------------------------------------------------------------------------------------
OFFSET = 30.0  # the offset case's bias; see the module docstring (not reduced: float32 stays under half the tolerance)
L1_TOL = {"z": (0.0, 2e-5), "sum": (1e-5, 1e-3, "abs"), "m2": (1e-4, 1e-3, "abs")}


def materialised(hist, tgt):
    B, L, D = hist.shape
    t = tgt.unsqueeze(1).expand(-1, L, -1)
    return torch.cat([t, hist, t - hist, t * hist], dim=-1).reshape(-1, 4 * D)


@functools.lru_cache(maxsize=None)
def l1_case(B, L, D, N, bias=True, offset=0.0):
    g = torch.Generator().manual_seed(B * 1000 + L * 10 + D + N)
    inp = dict(hist=torch.randn(B, L, D, generator=g), tgt=torch.randn(B, D, generator=g),
               W=torch.randn(N, 4 * D, generator=g) * 0.2, b=torch.randn(N, generator=g) + offset if bias else None)
    return inp, l1_eager(inp, torch.float64)


def l1_eager(inp, dtype):
    b = None if inp["b"] is None else inp["b"].to(dtype)
    return torch.nn.functional.linear(materialised(inp["hist"].to(dtype), inp["tgt"].to(dtype)), inp["W"].to(dtype), b)


def chunk_stats64(z, rows):
    """(chunks, 2, N): every chunk's column sums and M2 about the chunk's own mean, float64."""
    z = _np(z)
    out = np.empty((ceil_div(z.shape[0], rows), 2, z.shape[1]), F64)
    for k in range(out.shape[0]):
        blk = z[k * rows:(k + 1) * rows]
        out[k, 0] = blk.sum(0)
        out[k, 1] = ((blk - blk.mean(0)) ** 2).sum(0)
    return out


def chunk_stats32(z, rows):
    """The same in float32 the way the kernel goes about it: 32-row tiles (sum, mean, M2 about the tile mean) merged into the
    chunk's (count, mean, M2) by Chan's formula; the sum is mean x count.  For the CPU run."""
    z = np.asarray(z, F32)
    out = np.empty((ceil_div(z.shape[0], rows), 2, z.shape[1]), F32)
    for k in range(out.shape[0]):
        blk = z[k * rows:(k + 1) * rows]
        cnt, mean, m2 = F32(0), np.zeros(z.shape[1], F32), np.zeros(z.shape[1], F32)
        for s in range(0, blk.shape[0], 32):
            t = blk[s:s + 32]
            n = F32(t.shape[0])
            tm = t.sum(0, dtype=F32) / n
            t2 = ((t - tm) ** 2).sum(0, dtype=F32)
            tot, dlt = cnt + n, tm - mean
            m2 = m2 + t2 + dlt * dlt * (cnt * n / tot)
            mean = mean + dlt * (n / tot)
            cnt = tot
        out[k, 0], out[k, 1] = mean * cnt, m2
    return out


def l1_pairs(z, part, want_z, rows, stats_of_own_z=False):
    stats = chunk_stats64(z if stats_of_own_z else want_z, rows)
    assert tuple(part.shape) == stats.shape, (tuple(part.shape), stats.shape)
    return [("z", z, want_z, L1_TOL["z"]), ("sum", part[:, 0], stats[:, 0], L1_TOL["sum"]), ("m2", part[:, 1], stats[:, 1], L1_TOL["m2"])]


def l1_hip(inp, hist=None, tgt=None):
    from torch_rechub_amd import _lib, ops
    hist = inp["hist"].to(dev()) if hist is None else hist
    tgt = inp["tgt"].to(dev()) if tgt is None else tgt
    B, L, _ = hist.shape
    z, part = ops.din_att_l1(hist, tgt, inp["W"].to(dev()), None if inp["b"] is None else inp["b"].to(dev()), True)
    sync_and_check()
    return z, part, _lib.call("rh_din_att_l1_chunk_rows", B * L)


@pytest.mark.parametrize("N", [64, 128, 192, 256])
@pytest.mark.parametrize("D", [4, 8, 16])
def test_din_att_l1_every_supported_width_pair(D, N):
    inp, want = l1_case(7, 9, D, N)
    z, part, rows = l1_hip(inp)
    assert rows == 32 and part.shape[0] == 2  # a full tile and a 31-row tile, one per chunk
    check("att l1", f"D={D} N={N} R=63", l1_pairs(z, part, want, rows))


@pytest.mark.parametrize("B,L,bias,layout", [(1, 1, True, "contiguous"), (4, 8, True, "contiguous"), (7, 9, False, "contiguous"),
                                             (7, 9, True, "strided")])
def test_din_att_l1_single_tile_edges(B, L, bias, layout):
    D, N = 16, 128
    inp, want = l1_case(B, L, D, N, bias)
    hist = tgt = None
    if layout == "strided":
        big = torch.full((B, L + 3, D), float("nan"))
        big[:, 1:L + 1] = inp["hist"]
        wide = torch.full((B, D + 8), float("nan"))
        wide[:, 4:4 + D] = inp["tgt"]
        hist, tgt = big.to(dev())[:, 1:L + 1], wide.to(dev())[:, 4:4 + D]
        assert hist.stride(0) == (L + 3) * D and tgt.stride() == (D + 8, 1)
    z, part, rows = l1_hip(inp, hist, tgt)
    assert rows == 32 and part.shape[0] == ceil_div(B * L, 32)
    check("att l1", f"D={D} N={N} R={B * L} bias={bias} {layout}", l1_pairs(z, part, want, rows))
    if B * L == 1:
        assert bool((part[:, 1] == 0).all())  # one row: M2 is exactly 0


@pytest.mark.parametrize("B,L,D,N,chunk,tiles,offset", [(247, 100, 16, 256, 64, 2, 0.0), (247, 100, 4, 64, 64, 2, 0.0),
                                                        (500, 99, 8, 128, 96, 3, 0.0), (247, 100, 16, 256, 64, 2, OFFSET)])
def test_din_att_l1_chan_merge_across_the_row_tiles_of_a_chunk(B, L, D, N, chunk, tiles, offset):
    """offset: a bias of + OFFSET on every column (mean >> spread: a sum-of-squares shortcut, or a merge without the cross term,
    loses the variance); z then carries a float32 rounding of a number near OFFSET, so the float64 statistics are the kernel's
    own z's."""
    inp, want = l1_case(B, L, D, N, True, offset)
    z, part, rows = l1_hip(inp)
    R = B * L
    assert rows == chunk == 32 * tiles and part.shape[0] == ceil_div(R, chunk) and R - (part.shape[0] - 1) * chunk == 60
    if offset:
        assert float(want.mean(0).abs().min()) > 5 * float(want.std(0).max())
    check("att l1", f"D={D} N={N} R={R} chunk={chunk} offset={offset}", l1_pairs(z, part, want, rows, stats_of_own_z=bool(offset)))


def _same(a, b, what, rtol=2e-4, atol=2e-5, floor=1.0):
    """test_activation_unit_first_layer_on_register_built_operand's comparison."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    scale = max(floor, float(b.abs().max()))
    assert bool(torch.isfinite(a).all()), what
    assert float((a - b).abs().max()) <= atol * scale + rtol * float(b.abs().max()), what


def test_activation_unit_consumes_two_tile_chunk_statistics(monkeypatch):
    """rh_bn_stats_from_partial and bn_dice_head on 64-row chunks with a ragged last one: the ActivationUnit in train mode, fused
    first layer against the materialised path, and the first BatchNorm's running statistics against float64 statistics of z."""
    from torch_rechub_amd import _lib, ops
    from torch_rechub_amd.models.ranking.din import ActivationUnit
    B, L, D, dims = 247, 100, 16, [64]
    assert _lib.call("rh_din_att_l1_chunk_rows", B * L) == 64
    g = torch.Generator().manual_seed(B + L)
    torch.manual_seed(B * L)
    au = ActivationUnit(D, dims=dims, activation="dice", use_softmax=False)
    twin = ActivationUnit(D, dims=dims, activation="dice", use_softmax=False)
    twin.load_state_dict(au.state_dict())
    lin = au.attention.mlp[0]
    hist_c, tgt_c = torch.randn(B, L, D, generator=g), torch.randn(B, D, generator=g)
    z64 = torch.nn.functional.linear(materialised(hist_c.double(), tgt_c.double()), lin.weight.detach().double(),
                                     lin.bias.detach().double())
    au, twin = au.to(dev()).train(), twin.to(dev()).train()
    hist, tgt = hist_c.to(dev()), tgt_c.to(dev())
    gy = torch.randn(B, D, generator=g).to(dev())
    assert ops.din_att_l1_ok(hist, tgt, au.attention.mlp[0])
    calls = []
    real = ops.bn_dice_head
    monkeypatch.setattr(ops, "bn_dice_head", lambda *a, **k: (calls.append((k.get("chunk_rows"), k["chunk_stats"].shape[0])),
                                                              real(*a, **k))[1])
    h1, t1 = hist.detach().clone().requires_grad_(), tgt.detach().clone().requires_grad_()
    out = au(h1, t1)
    out.backward(gy)
    assert calls == [(64, ceil_div(B * L, 64))], calls
    monkeypatch.undo()
    monkeypatch.setattr(ops, "din_att_l1_ok", lambda *a: False)
    h2, t2 = hist.detach().clone().requires_grad_(), tgt.detach().clone().requires_grad_()
    ref = twin(h2, t2)
    ref.backward(gy)
    sync_and_check()
    _same(out, ref, "attention output")
    _same(h1.grad, h2.grad, "g_history")
    _same(t1.grad, t2.grad, "g_target")
    gmax = max(float(q.grad.abs().max()) for q in twin.parameters())
    for (n, p), (_, q) in zip(au.named_parameters(), twin.named_parameters()):
        _same(p.grad, q.grad, f"g_{n}", floor=gmax)
    for (n, p), (_, q) in zip(au.named_buffers(), twin.named_buffers()):
        _same(p, q, f"buffer {n}", rtol=1e-5, atol=1e-6)
    bn = au.attention.mlp[1]
    assert type(bn) is torch.nn.BatchNorm1d and int(bn.num_batches_tracked) == 1
    check("att l1", "ActivationUnit dims=[64] R=24700: running statistics", pairs(
        dict(running_mean=bn.running_mean, running_var=bn.running_var), running_stats(z64), BN_TOL))


BN_TOL = {"running_mean": (1e-5, 1e-6), "running_var": (2e-5, 1e-6)}  # test_bn_relu_dropout_vs_torch_modules


def running_stats(z):
    """nn.BatchNorm1d's buffers after one training step from (0, 1), momentum 0.1."""
    n = z.shape[0]
    return dict(running_mean=0.1 * z.mean(0), running_var=0.9 + 0.1 * z.var(0, unbiased=False) * (n / (n - 1.0)))


# ---- AUGRU -------------------------------------------------------------------------------------------------------------------
AUGRU_TOL = {"states": (1e-4, 1e-5), "d_xw": (5e-4, 1e-5), "d_attn": (5e-4, 1e-5), "d_U": (5e-4, 1e-5), "d_state_bias": (5e-4, 1e-5)}


def spw(D):
    return 64 // (D // 4)


@functools.lru_cache(maxsize=None)
def augru_case(B, T, D, saturate=False):
    g = torch.Generator().manual_seed(B * 1000 + T * 10 + D + int(saturate))
    xw = torch.randn(B, T, 3 * D, generator=g) * 0.8
    lens = torch.randint(1, T + 1, (B,), generator=g)
    attn = torch.rand(B, T, generator=g) * (torch.arange(T)[None, :] < lens[:, None])  # 0 on padded steps
    attn[0] = 0.0  # a sample whose weights are all 0: its state never leaves 0
    if saturate:
        big = torch.rand(B, T, 3, generator=g) < 1.0 / 3.0
        xw = (xw.view(B, T, 3, D) * torch.where(big, 40.0, 1.0)[..., None]).reshape(B, T, 3 * D)
    inp = dict(xw=xw, attn=attn, U=torch.randn(D, 3 * D, generator=g) * (0.5 / D ** 0.5), ub=torch.randn(3 * D, generator=g) * 0.3,
               G=torch.randn(B, T, D, generator=g))
    return inp, augru_eager(inp, F64)


def augru_eager(inp, dtype):
    xw, attn, U, ub, G = (inp[k].numpy().astype(dtype) for k in ("xw", "attn", "U", "ub", "G"))
    d_xw, d_attn, d_U, d_b = O.augru_backward(xw, attn, U, G, ub)
    return dict(states=O.augru_forward(xw, attn, U, ub), d_xw=d_xw, d_attn=d_attn, d_U=d_U, d_state_bias=d_b)


def augru_hip(inp):
    from torch_rechub_amd import ops
    xd, ad, ud, bd = (inp[k].to(dev()).requires_grad_() for k in ("xw", "attn", "U", "ub"))
    h_all = ops.augru(xd, ad, ud, bd)
    h_all.backward(inp["G"].to(dev()))
    sync_and_check()
    return dict(states=h_all.detach(), d_xw=xd.grad, d_attn=ad.grad, d_U=ud.grad, d_state_bias=bd.grad)


def update_gate64(inp, states):
    """u of every (sample, step, element) in float64, from the reference's states."""
    xw, U, ub = (inp[k].numpy().astype(F64) for k in ("xw", "U", "ub"))
    D = U.shape[0]
    prev = np.concatenate([np.zeros_like(states[:, :1]), states[:, :-1]], axis=1)
    return 1.0 / (1.0 + np.exp(-(xw[:, :, :D] + prev @ U[:, :D] + ub[:D])))


@pytest.mark.parametrize("T", [1, 2, 3, 17])
@pytest.mark.parametrize("D", [4, 8, 16, 32])
def test_augru_attention_weights_and_state_bias_together(D, T):
    from torch_rechub_amd import _lib
    assert D <= _lib.H.RH_AUGRU_MAX_D
    for B in (spw(D) - 1, spw(D), spw(D) + 1):
        inp, want = augru_case(B, T, D)
        got = augru_hip(inp)
        check("augru", f"D={D} T={T} B={B}", pairs(got, want, AUGRU_TOL))
        assert bool((want["states"][0] == 0).all()) and bool((want["d_xw"][0] == 0).all())
        assert bool((got["states"][0] == 0).all()) and bool((got["d_xw"][0] == 0).all())  # all weights 0: exactly nothing moves


@pytest.mark.parametrize("D", [4, 8, 16, 32])
def test_augru_saturated_gates_stay_finite_and_exact_at_the_rails(D):
    """xw x 40 at a third of the (sample, step, gate) positions: exp overflows to inf in float32 and rcp(inf) has to give 0."""
    B, T = spw(D) + 1, 17
    inp, want = augru_case(B, T, D, True)
    u = update_gate64(inp, want["states"])
    assert float(u.min()) < 1e-12 and float(u.max()) > 1 - 1e-12
    assert float(np.abs(inp["xw"].numpy()).max()) > 89.0  # past float32 exp's range
    check("augru", f"saturated D={D} T={T} B={B}", pairs(augru_hip(inp), want, AUGRU_TOL))


if __name__ == "__main__":
    # float32 eager numpy / torch on the CPU through the same comparison, for every shape above
    for D, L, LS, nll, trips in SEQ_ROWS:
        for mode in SEQ_MODES:
            for pad in (0, None):
                for B in (5, 70):
                    inp, want = seq_case(D, L, B, mode, pad)
                    check("seq_pool", f"float32 eager D={D} L={L} B={B} {mode} pad={pad}",
                          pairs(seq_eager(inp, mode, pad, F32), want, SEQ_TOL_CONCAT if mode == "concat" else SEQ_TOL))
    for D in sorted(ATT_LS):
        for L in ATT_L:
            for B in (1, 67):
                for strided in (False, True):
                    check("att ends", f"float32 eager D={D} L={L} B={B} strided={strided}",
                          pairs(att_eager(att_inputs(B, L, D), strided, torch.float32), att_want(B, L, D, strided), ATT_TOL))
    check("att ends", "float32 eager masked softmax weights",
          pairs(att_masked_eager(att_masked_case(), torch.float32), att_masked_eager(att_masked_case(), torch.float64), ATT_TOL))
    l1_cases = [(7, 9, D, N, True, 0.0, 32) for D in (4, 8, 16) for N in (64, 128, 192, 256)]
    l1_cases += [(1, 1, 16, 128, True, 0.0, 32), (4, 8, 16, 128, True, 0.0, 32), (7, 9, 16, 128, False, 0.0, 32),
                 (247, 100, 16, 256, True, 0.0, 64), (247, 100, 4, 64, True, 0.0, 64), (500, 99, 8, 128, True, 0.0, 96),
                 (247, 100, 16, 256, True, OFFSET, 64)]
    for B, L, D, N, bias, offset, rows in l1_cases:
        inp, want = l1_case(B, L, D, N, bias, offset)
        z32 = l1_eager(inp, torch.float32)
        part = chunk_stats32(z32.numpy(), rows)
        check("att l1 offset" if offset else "att l1", f"float32 eager D={D} N={N} R={B * L} bias={bias} offset={offset}",
              l1_pairs(z32, part, want, rows, stats_of_own_z=bool(offset)))
        if B * L == 24700 and N == 256 and not offset:
            check("att l1", "float32 eager running statistics", pairs(running_stats(z32), running_stats(want), BN_TOL))
    for D in (4, 8, 16, 32):
        for T in (1, 2, 3, 17):
            for B in (spw(D) - 1, spw(D), spw(D) + 1):
                inp, want = augru_case(B, T, D)
                check("augru", f"float32 eager D={D} T={T} B={B}", pairs(augru_eager(inp, F32), want, AUGRU_TOL))
        inp, want = augru_case(spw(D) + 1, 17, D, True)
        u = update_gate64(inp, want["states"])
        assert float(u.min()) < 1e-12 and float(u.max()) > 1 - 1e-12
        with np.errstate(over="ignore"):
            check("augru saturated", f"float32 eager saturated D={D}", pairs(augru_eager(inp, F32), want, AUGRU_TOL))
    for family, (worst, case, what) in WORST.items():
        print(f"WORST {family}: {worst:.3f} [{what}; {case}]")
