"""ops.t5_attention under dropout (csrc/t5attn.hip: the one-wavefront path of Lq <= 8; csrc/softmax_attn_tile.h under T5Rule:
the 64 x 64 MFMA tiles) against a float64 oracle whose dropout mask does NOT come from the kernels under test.

Counter protocol (csrc/common.h drop_key, csrc/softmax_attn_tile.h attn_drop_mul): a call with p > 0 in training reads
(seed, counter) from the device state, saves the counter for its backward and advances it by one; element (b, h, i, j) of the
weights is element ((b H + h) Lq + i) Lk + j of that call, kept when hash >= uint32(float32(p) 2^32) and then scaled by the
float32 1 / (1 - p).  With the state set to (RNG_SEED, C0, 0, 0) the call uses counter C0 and leaves rng[1] == C0 + 1; p = 0
or eval draws nothing.  ``host_keep`` (tests/test_gpu_mlp_dropout_oracle.py, verified there bit for bit against ops.dropout)
rebuilds the mask; the oracle is tiger_oracle.attention with the multiplier keep * keep_scale(p) on the weights, autograd in
float64.

a. With V = identity per head the output IS the dropped weights: after asserting from the p = 0 output that every valid
   weight is > 0, the zero pattern over the valid keys must equal host_keep exactly (rectangular, both paths).
b. out, g_q, g_k, g_v and g_table against float64 under the rule of test_gpu_tiger.py::test_attention_kernel_against_float64,
   unchanged: rtol 1e-4 and a floor of max(2e-6 of the tensor's largest magnitude (1e-4 for g_table), 4 x the error of the
   same oracle with the same multiplier in float32 on the CPU).  No element is excluded; the bound never looks at the kernel.
c. Negative controls: the same kernel result against an oracle with the counter C0 + 1, or with the index
   ((b H + h) Lk + j) Lq + i, must miss that bound by more than 100 x on EVERY compared quantity.
d. p = 0.3 with training=False is the p = 0 output bitwise and leaves the state untouched.

There is no ReLU here, so no kink margin.  Kept fractions of the seven cases (host): 0.50 to 0.52 at p = 0.5, 0.90 at p = 0.1.
Wrong masks, host side (wrong oracle against right oracle, in units of the bound; ``python tests/test_gpu_t5_dropout_oracle.py``
prints them on the CPU), the smallest over the seven cases: counter C0 + 1: out, g_q, g_k, g_v 180185 x, g_table 3174 x; at
the four controls: (3, 8, 8) late out 381755 g_q 911897 g_k 1080839 g_v 527146 g_table 7868; (2, 70, 70) late out 499950 g_q
435144 g_k 429288 g_v 468705 g_table 6459; (3, 5, 80) swap out 499950 g_q 296982 g_k 346698 g_v 360580; (5, 20, 130) swap out
500000 g_q 479880 g_k 432064 g_v 573479.  The float32 oracle sits at 0.002 to 0.050 of the bound.  So 100 x is far from both.
Worst error / bound per compared quantity over the seven cases on the MI355X (the ``ORACLE`` lines): out 0.033, g_q 0.642,
g_k 0.925, g_v 0.023, g_table 0.001; every case but (3, 5, 80) and (5, 33, 33) stays below 0.1.  Those two peak (g_q 0.60 /
0.64, g_k 0.91 / 0.93) in their sample with ONE valid key, at p = 0.1: the exact g_q and g_k of such a sample are 0, because
dS = P (m dA - delta) with delta = g_out . out = m dA; the kernels take delta from the stored output, so for m = 1 / (1 - p)
that is no power of two the difference is rounding noise of size 2^-24 m |dA| (measured: error 0 in that sample at p = 0 and
p = 0.5, 1.5e-6 / 5.2e-6 on g_k at p = 0.1, the same with contiguous operands).  That is inside the bound and no bug; none was
found.  The four controls miss by 7867 x (g_table) to 1080730 x.
Broken on purpose in a scratch build (not committed), measured on the MI355X: Lq and Lk swapped in attn_drop_mul fails all four
mask tests, all seven comparisons and both whole-model modules' dropout cases (20 of 24 tests of the two modules; the p = 0
controls and the eval test pass); a backward that reads rng[1] instead of the saved counter passes the mask tests and fails all
seven comparisons and every whole-model dropout case (16 of 24).
"""
import functools

import numpy as np
import pytest
import torch

import tiger_oracle as O
from sasrec_oracle import keep_scale
from test_gpu_mlp_dropout_oracle import RNG_SEED, host_hash, host_keep, host_threshold
from test_gpu_tiger import attn_case, key_masks, run_attn

pytestmark = pytest.mark.gpu
C0 = 11
NAMES = ("out", "g_q", "g_k", "g_v", "g_table")


def dev():
    return torch.device("cuda:0")


def set_rng(ctr=C0):
    from torch_rechub_amd import ops
    rng = ops._dropout_rng(dev())
    rng.copy_(torch.tensor([RNG_SEED, ctr, 0, 0], dtype=torch.int64))
    return rng


def weight_keep(B, H, Lq, Lk, p, wrong=None):
    """(B, H, Lq, Lk) keep flags of the call with counter C0.  wrong = "late": counter C0 + 1; "swap": the index a kernel
    would form with Lq and Lk exchanged."""
    if wrong == "swap":
        bh = np.arange(B * H, dtype=np.uint64)[:, None, None]
        i = np.arange(Lq, dtype=np.uint64)[None, :, None]
        j = np.arange(Lk, dtype=np.uint64)[None, None, :]
        keep = host_hash(RNG_SEED, C0, (bh * np.uint64(Lk) + j) * np.uint64(Lq) + i) >= np.uint64(host_threshold(p))
    else:
        keep = host_keep(RNG_SEED, C0 + (1 if wrong == "late" else 0), B * H * Lq * Lk, p)
    return keep.reshape(B, H, Lq, Lk)


# ---- a. the mask, bit for bit ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("B,Lq,Lk,H", [(3, 5, 64, 3), (3, 20, 128, 2)], ids=["narrow", "tiles"])
def test_dropped_weights_are_the_hash_of_the_documented_index(B, Lq, Lk, H, p):
    from torch_rechub_amd import ops
    g = torch.Generator().manual_seed(17)
    q = (0.5 * torch.randn(B, Lq, H * Lk, generator=g)).to(dev())
    k = (0.5 * torch.randn(B, Lk, H * Lk, generator=g)).to(dev())
    v = torch.eye(Lk).repeat(B, 1, H).to(dev())  # dh = Lk: output row i of head h = the weights of query i
    mask = key_masks("right", B, Lk, g)
    mask[:, 0] = 1
    valid = (mask != 0).numpy()[:, None, None, :].repeat(H, 1).repeat(Lq, 2)  # (B, H, Lq, Lk)
    mask = mask.to(dev())
    weights = lambda out: out.detach().view(B, Lq, H, Lk).permute(0, 2, 1, 3).cpu().numpy()  # noqa: E731
    rng = set_rng()
    w0 = weights(ops.t5_attention(q, k, v, H, key_mask=mask))
    assert int(rng[1]) == C0
    assert (w0[valid] > 0).all() and (w0[~valid] == 0).all(), "inputs: a valid weight underflowed"
    wd = weights(ops.t5_attention(q, k, v, H, key_mask=mask, dropout_p=p))
    torch.cuda.synchronize()
    ops.check_errors()
    assert int(rng[1]) == C0 + 1 and int(rng[0]) == RNG_SEED
    keep = weight_keep(B, H, Lq, Lk, p)
    assert (wd[~valid] == 0).all()
    got = wd != 0
    assert np.array_equal(got[valid], keep[valid]), f"{int((got != keep)[valid].sum())} of {int(valid.sum())} keep flags differ"
    np.testing.assert_allclose(wd[valid & keep], w0[valid & keep] * keep_scale(p), rtol=2e-6, atol=0)


# ---- b. forward and backward against float64 ------------------------------------------------------------------------------
# (B, Lq, Lk, H, dh, mask, causal, num_buckets, strided, p)
CASES = [
    (3, 5, 80, 3, 50, "mixed", False, 0, True, 0.1),     # cross attention, narrow: two key chunks, no valid key, spare wavefront
    (3, 8, 8, 3, 16, None, True, 8, False, 0.5),         # decoder: the last narrow length, causal, one-sided buckets
    (5, 8, 130, 3, 4, "mixed", False, 32, False, 0.5),   # narrow path with a bias across chunk edges (the diagonal carry)
    (5, 33, 33, 3, 64, "mixed", False, 32, True, 0.1),   # encoder on the tiles, every kind of mask row, strided QKV
    (5, 20, 130, 3, 50, "mixed", False, 0, True, 0.5),   # rectangular on the tiles: three key tiles, empty tiles skipped
    (4, 70, 70, 2, 16, "left", True, 8, False, 0.1),     # causal with a mask: rows with no key left, ragged second tile
    (2, 70, 70, 1, 128, None, True, 32, True, 0.5),      # causal on the tiles, two column chunks
]
NARROW_RECT, NARROW_SQUARE, TILE_RECT, TILE_SQUARE = CASES[0], CASES[1], CASES[4], CASES[6]


@functools.lru_cache(maxsize=None)
def inputs(case):
    B, Lq, Lk, H, dh, mask, causal, nb, strided, p = case
    return attn_case(B, Lq, Lk, H, dh, mask, causal, nb, seed=Lq + Lk + H + dh)


def _oracle(case, dtype, wrong):
    B, Lq, Lk, H, dh, mask, causal, nb, strided, p = case
    c = inputs(case)
    mult = None
    if p > 0:
        mult = torch.from_numpy(weight_keep(B, H, Lq, Lk, p, wrong).astype(np.float64) * keep_scale(p)).to(dtype)
    q, k, v = (c[n].clone().to(dtype).requires_grad_(True) for n in "qkv")
    t = c["table"].clone().to(dtype).requires_grad_(True) if c["table"] is not None else None
    out = O.attention(q, k, v, H, c["mask"], causal, t, c["bidirectional"], c["md"], drop=mult)
    out.backward(c["gout"].to(dtype))
    res = [x.detach().numpy().astype(np.float64) for x in (out, q.grad, k.grad, v.grad)] + \
        [None if t is None else t.grad.numpy().astype(np.float64)]
    for a in res:
        if a is not None:
            a.setflags(write=False)
    return res


@functools.lru_cache(maxsize=None)
def oracle(case, wrong=None):
    return _oracle(case, torch.float64, wrong)


@functools.lru_cache(maxsize=None)
def bounds(case):
    """Per quantity the floor of the rule: from the float64 and the float32 oracle alone (None where there is no table)."""
    wants, cpu32 = oracle(case), _oracle(case, torch.float32, None)
    out = []
    for name, want, c32 in zip(NAMES, wants, cpu32):
        if want is None:
            out.append(None)
            continue
        scale = max(float(np.abs(want).max()), 1e-30)
        out.append(max((1e-4 if name == "g_table" else 2e-6) * scale, 4 * float(np.abs(c32 - want).max())))
    return out


def ratios(case, gots, wants):
    """{quantity: (largest |got - want| - 1e-4 |want|) / floor}: within the rule when <= 1."""
    r = {}
    for name, got, want, atol in zip(NAMES, gots, wants, bounds(case)):
        if want is None:
            assert got is None
            continue
        got = np.asarray(got, np.float64)
        assert got.shape == want.shape and np.isfinite(got).all(), name
        r[name] = float((np.abs(got - want) - 1e-4 * np.abs(want)).max()) / atol
    return r


@functools.lru_cache(maxsize=None)
def kernel(case):
    """One forward and backward of the kernel from the state (RNG_SEED, C0), shared by the comparison and its controls."""
    from torch_rechub_amd import ops
    rng = set_rng()
    gots = run_attn(inputs(case), case[8], p=case[9])
    torch.cuda.synchronize()
    ops.check_errors()
    assert int(rng[1]) == C0 + (1 if case[9] > 0 else 0), "dropout call counter"
    return [None if t is None else t.numpy().astype(np.float64) for t in gots]


@pytest.mark.parametrize("case", CASES)
def test_attention_under_dropout_against_float64(case):
    keep = weight_keep(case[0], case[3], case[1], case[2], case[9])
    assert abs(keep.mean() - (1 - case[9])) < 0.03, "inputs: kept fraction"
    r = ratios(case, kernel(case), oracle(case))
    print(f"ORACLE {case}: error / bound " + ", ".join(f"{k} {v:.3f}" for k, v in r.items()))
    bad = {k: round(v, 3) for k, v in r.items() if not v <= 1.0}
    assert not bad, f"{case}: error / bound {bad}"


# ---- c. negative controls --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,wrong", [(NARROW_SQUARE, "late"), (TILE_SQUARE, "late"), (NARROW_RECT, "swap"), (TILE_RECT, "swap")],
                         ids=["narrow-late", "tiles-late", "narrow-swap", "tiles-swap"])
def test_attention_misses_an_oracle_with_a_wrong_mask(case, wrong):
    got = kernel(case)
    assert max(ratios(case, got, oracle(case)).values()) <= 1.0
    r = ratios(case, got, oracle(case, wrong))
    print(f"ORACLE {case} wrong mask ({wrong}): error / bound " + ", ".join(f"{k} {v:.0f}" for k, v in r.items()))
    near = {k: round(v, 1) for k, v in r.items() if not v > 100.0}
    assert not near, f"{case}: a wrong mask ({wrong}) is only {near} x the bound away"


# ---- d. eval ignores p -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [NARROW_RECT, TILE_SQUARE], ids=["narrow", "tiles"])
def test_eval_ignores_p_bitwise_and_draws_nothing(case):
    c = inputs(case)
    rng = set_rng()
    plain = run_attn(c, case[8], p=0.0)
    evald = run_attn(c, case[8], p=0.3, training=False)
    torch.cuda.synchronize()
    assert torch.equal(rng.cpu(), torch.tensor([RNG_SEED, C0, 0, 0], dtype=torch.int64))
    for name, a, b in zip(NAMES, plain, evald):
        assert (a is None and b is None) or torch.equal(a, b), name


if __name__ == "__main__":
    # The reference side alone, no GPU: kept fractions, the float32 oracle inside the bound, and how far a wrong mask moves
    # the oracle itself, in units of the bound.
    for case in CASES:
        frac = weight_keep(case[0], case[3], case[1], case[2], case[9]).mean()
        r32 = ratios(case, _oracle(case, torch.float32, None), oracle(case))
        line = f"{case}: kept {frac:.3f}; float32 oracle / bound {max(r32.values()):.3f}"
        for wrong in ("late", "swap"):
            if wrong == "swap" and case[1] == case[2]:
                continue
            r = ratios(case, oracle(case, wrong), oracle(case))
            line += f"; {wrong}: " + " ".join(f"{k} {v:.0f}" for k, v in r.items())
        print(line)
