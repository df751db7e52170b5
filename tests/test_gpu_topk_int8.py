"""ops.quantize_rows_int8 / topk_items_int8 / ivf_scan_int8 and serving's quantizer="SQ8" (csrc/topk_q8.hip) against plain
numpy: the quantisation rule in float32, int64 sums of the codes, then the three float32 operations of the score,
  score[i][j] = ((float32)(sum_k qc_ik xc_jk) * qs_i) * xs_j (+ bias_j),
ranked by tests/topk_oracle.py.  Every step is exact or a single rounded float32 operation, so ids AND scores are demanded
element for element everywhere."""
import numpy as np
import pytest
import torch

import ivf_oracle as IO
import topk_oracle as O

gpu = pytest.mark.gpu
F = np.float32


def t(a, dtype=None):
    return None if a is None else torch.as_tensor(a, dtype=dtype).to("cuda:0")


def quant(x):
    """The rule in numpy float32: scale = max |x| / 127 (1 for a zero row), code = clip(rint(x / scale), -127, 127)."""
    m = np.abs(x).max(axis=1)
    scale = np.where(m == 0, F(1), m / F(127)).astype(F)
    return np.clip(np.rint(x / scale[:, None]), -127, 127).astype(np.int8), scale


def scores(q, xc, xs, bias=None):
    qc, qs = quant(q)
    s = (qc.astype(np.int64) @ xc.astype(np.int64).T).astype(F)
    s = (s * qs[:, None]) * xs[None, :]
    return (s if bias is None else s + bias[None, :]).astype(np.float64)


def run(q, xc, xs, k, **kw):
    from torch_rechub_amd import ops
    ids, sc = ops.topk_items_int8(t(q), t(xc), t(xs), k, bias=t(kw.pop("bias", None)),
                                  exclude=t(kw.pop("exclude", None), torch.int64), **kw)
    torch.cuda.synchronize()
    assert ids.dtype == torch.int64 and sc.dtype == torch.float32 and ids.shape == sc.shape == (len(q), k)
    return ids.cpu().numpy(), sc.cpu().numpy().astype(np.float64)


def assert_same(got, exp, what=""):
    np.testing.assert_array_equal(got[0], exp[0], err_msg=f"{what} ids")
    np.testing.assert_array_equal(got[1], exp[1], err_msg=f"{what} scores")


@gpu
@pytest.mark.parametrize("M", [1, 65])
@pytest.mark.parametrize("D", [1, 15, 16, 17, 64, 129, 1024])
def test_quantize_rows_is_the_numpy_rule_bit_for_bit(D, M):
    from torch_rechub_amd import ops
    x = np.random.default_rng(D + M).standard_normal((M, D)).astype(F)
    if M > 1:
        x[1] = 0  # scale 1, codes 0
        # scale exactly 1: quotients on exact midpoints over even and odd integers, both signs
        x[2] = np.resize(np.array([127, 2.5, 3.5, -2.5, -3.5, 0.5, 126.5, -127], dtype=F), D)
    wide = torch.zeros((M, D + 3), device="cuda:0")
    wide[:, :D] = t(x)
    codes, scale = quant(x)
    if M > 1 and D > 6:
        assert scale[1] == 1 and not codes[1].any() and codes[2, :7].tolist() == [127, 2, 4, -2, -4, 0, 126]
    for name, inp in (("contiguous", t(x)), ("strided", wide[:, :D])):
        c, s = ops.quantize_rows_int8(inp)
        assert c.dtype == torch.int8 and c.shape == (M, D) and s.dtype == torch.float32 and s.shape == (M,)
        np.testing.assert_array_equal(s.cpu().numpy(), scale, err_msg=name)
        np.testing.assert_array_equal(c.cpu().numpy(), codes, err_msg=name)


# M, D, V, K, nsplit, extreme: every D (byte / 16-byte loads, the 32-k step, the 128-k chunk edge, the prefetch path), V, M,
# K (RB switches at 128 / 129, K > V) and nsplit of the issue; extreme = all codes +-127 at D = 1024, the largest sum
FLAT_CASES = [(1, 1, 1, 1, 1, 0), (63, 15, 63, 10, 2, 0), (65, 16, 64, 128, 1, 0), (1, 17, 65, 129, 3, 0),
              (63, 31, 129, 256, 7, 0), (65, 32, 4097, 10, 7, 0), (1, 33, 4097, 128, 3, 0), (63, 127, 129, 129, 2, 0),
              (65, 128, 4097, 256, 1, 0), (1, 129, 65, 10, 7, 0), (63, 144, 4097, 1, 3, 0), (65, 1024, 129, 10, 2, 0),
              (65, 1024, 129, 10, 1, 1)]


@gpu
@pytest.mark.parametrize("M,D,V,K,nsplit,extreme", FLAT_CASES)
def test_flat_scan_matches_integer_arithmetic_bit_for_bit(M, D, V, K, nsplit, extreme):
    q, x, bias = O.normal_data(M + D + V + K, M, D, V, True)
    if extreme:
        q, x = np.sign(q), np.sign(x)
        q[0] = x[5]
    xc, xs = quant(x)
    if extreme:
        assert (np.abs(xc) == 127).all() and (np.abs(quant(q)[0]) == 127).all()
        assert int(xc[5].astype(np.int64) @ xc[5].astype(np.int64)) == 127 * 127 * 1024
    assert_same(run(q, xc, xs, K, bias=bias, nsplit=nsplit), O.rank(scores(q, xc, xs, bias), O.valid_mask(M, V), K))


@gpu
@pytest.mark.parametrize("D", [17, 144])
def test_ties_bias_with_minus_inf_exclude_and_invalid(D):
    """Codes in [-3, 3] under equal scales and queries from {-1, 0, 1} (codes -127, 0, 127): long runs of exact ties."""
    M, V, K, S = 65, 4097, 129, 5
    rng = np.random.default_rng(D)
    q = rng.integers(-1, 2, size=(M, D)).astype(F)
    xc, xs = rng.integers(-3, 4, size=(V, D)).astype(np.int8), np.full((V,), 0.5, dtype=F)
    bias = rng.integers(-5, 6, size=(V,)).astype(F)
    bias[::7] = -np.inf
    s = scores(q, xc, xs, bias)
    exclude = rng.integers(-1, V, size=(M, S))
    top = O.rank(s, O.valid_mask(M, V), K)[0]
    exclude[:, 0] = top[:, 0]  # the best id of every row is excluded, the second of row 0 is invalid
    invalid = [int(top[0, 1]), 64, V - 1]
    exp = O.rank(s, O.valid_mask(M, V, exclude, invalid), K)
    assert (np.diff(exp[1], axis=1) == 0).mean() > 0.5
    kw = dict(bias=bias, invalid=invalid)
    assert_same(run(q, xc, xs, K, exclude=exclude, nsplit=3, **kw), exp)
    for nsplit in (1, 7):
        assert_same(run(q, xc, xs, K, exclude=exclude, nsplit=nsplit, **kw), exp, f"nsplit {nsplit}")
    assert_same(run(q[64:], xc, xs, K, exclude=exclude[64:], **kw), (exp[0][64:], exp[1][64:]), "one row alone")


@gpu
@pytest.mark.parametrize("D", [24, 136])
def test_ivf_scan_with_every_list_probed_equals_the_flat_scan(D):
    from torch_rechub_amd import ops
    lengths = [65, 0, 1, 63, 64, 0, 130, 7]
    M, K, V, nl = 9, 129, sum(lengths), len(lengths)
    q, x, bias = O.normal_data(D, M, D, V, True)
    xc, xs = quant(x)
    lists = IO.lists_of_lengths(6, lengths)
    cs, bs, row_id, off = IO.group(xc, bias, lists)
    probe = np.stack([np.random.default_rng(i).permutation(nl) for i in range(M)]).astype(np.int32)
    ids, sc = ops.ivf_scan_int8(t(q), t(cs), t(xs[row_id]), t(row_id), t(off), t(probe), K, bias=t(bs))
    got = ids.cpu().numpy(), sc.cpu().numpy().astype(np.float64)
    assert_same(got, run(q, xc, xs, K, bias=bias), "against the flat scan")
    assert_same(got, O.rank(scores(q, xc, xs, bias), O.valid_mask(M, V), K), "against the oracle")


@gpu
@pytest.mark.parametrize("metric", ["IP", "L2"])
@pytest.mark.parametrize("index_type", ["Flat", "IVF"])
def test_serving_sq8_index_equals_the_fp32_index_on_data_the_codes_hold(index_type, metric, tmp_path):
    """Integers in [-127, 127] with a +-127 in every row (2 q has 254 and scale exactly 2): every scale is a power of two,
    the codes are the data, and every step of either index is exact."""
    from torch_rechub_amd.serving import HipBuilder
    rng = np.random.default_rng(8)
    q, x = (rng.integers(-127, 128, size=(n, 24)).astype(F) for n in (33, 300))
    q[:, 3], x[:, 5] = rng.choice([-127, 127], size=33), rng.choice([-127, 127], size=300)
    q, x = torch.as_tensor(q), torch.as_tensor(x)
    kw = dict(index_type=index_type, nlists=4, nprobe=4, niter=2, device="cuda:0")
    with HipBuilder(metric, **kw).from_embeddings(x) as ref:
        exp = ref.query(q, 20)
        ref.save(tmp_path / "f32.idx")
    builder = HipBuilder(metric, quantizer="SQ8", **kw)
    with builder.from_embeddings(x) as index:
        assert index._table.dtype == index._search.dtype == torch.int8 and index._scale.dtype == torch.float32
        assert not any(v.dtype == torch.float32 and v.numel() >= x.numel() for v in vars(index).values() if torch.is_tensor(v))
        got = index.query(q, 20)
        index.save(tmp_path / "sq8.idx")
    with builder.from_index_file(tmp_path / "sq8.idx") as index:
        assert type(index) is type(ref) and index._search.dtype == torch.int8
        again = index.query(q, 20)
    with builder.from_index_file(tmp_path / "f32.idx") as index:  # a file of the fp32 path keeps its type
        assert index._search.dtype == torch.float32 and index.quantizer is None
        old = index.query(q, 20)
    for ids, val in (got, again, old):
        assert torch.equal(ids, exp[0]) and torch.equal(val, exp[1])


def _refusals():
    from torch_rechub_amd import ops
    from torch_rechub_amd.serving import HipBuilder
    from torch_rechub_amd.utils.match import ExactIndex
    q, codes, i32 = torch.zeros(2, 8), torch.zeros((5, 8), dtype=torch.int8), torch.zeros(2, dtype=torch.int32)
    return {
        "scale shape": (lambda: ops.topk_items_int8(q, codes, torch.ones(4), 3), "one float32 scale per row"),
        "scale type": (lambda: ops.topk_items_int8(q, codes, torch.ones(5).double(), 3), "one float32 scale per row"),
        "float codes": (lambda: ops.topk_items_int8(q, codes.float(), torch.ones(5), 3), "int8 codes"),
        "ivf scale shape": (lambda: ops.ivf_scan_int8(q, codes, torch.ones(5, 1), i32, i32, i32, 3), "one float32 scale"),
        "ivf half codes": (lambda: ops.ivf_scan_int8(q, codes.half(), torch.ones(5), i32, i32, i32, 3), "int8 codes_sorted"),
        "unknown quantizer": (lambda: HipBuilder("IP", quantizer="PQ"), "quantizer must be one of"),
        "unknown quantizer of ExactIndex": (lambda: ExactIndex(quantizer="SQ4"), "quantizer must be one of"),
        "half dtype": (lambda: HipBuilder("IP", dtype=torch.float16, quantizer="SQ8"), "does not combine with dtype"),
    }


@pytest.mark.parametrize("case", ["scale shape", "scale type", "float codes", "ivf scale shape", "ivf half codes",
                                  "unknown quantizer", "unknown quantizer of ExactIndex", "half dtype"])
def test_the_new_surface_refuses_on_the_host(case):
    call, message = _refusals()[case]
    with pytest.raises(ValueError, match=message):
        call()
