"""ops.topk_items / ops.ivf_scan / serving.HipBuilder over fp16 and bf16 item tables (csrc/topk_half.hip) against the
float64 brute force of tests/topk_oracle.py and tests/ivf_oracle.py, fed q.to(T) and the table as float64:
score[i][j] = sum_k T(q_ik) x_jk (+ bias_j).  Products of two T values are exact in fp32, so on integer data ids AND
scores are demanded element for element; real-valued data are held to the fp32 accumulation bound over exact products."""
import numpy as np
import pytest
import torch

import ivf_oracle as IO
import topk_oracle as O

TYPES = [torch.float16, torch.bfloat16]
gpu = pytest.mark.gpu


def t(a, dtype=None):
    return None if a is None else torch.as_tensor(a, dtype=dtype).to("cuda:0")


def rounded(a, T):
    """The values of a.to(T), as float64."""
    return torch.as_tensor(a).to(T).double().numpy()


def ints(seed, M, D, V, lim=15):
    """q, x from the integers in [-lim, lim] and bias in [-5, 5]: every partial sum is exact in fp32 (225 D + 5 < 2^24)."""
    rng = np.random.default_rng(seed)
    draw = lambda *shape: rng.integers(-lim, lim + 1, size=shape).astype(np.float32)
    return draw(M, D), draw(V, D), rng.integers(-5, 6, size=(V,)).astype(np.float32)


def run(q, x, k, T, **kw):
    from torch_rechub_amd import ops
    q = q if torch.is_tensor(q) else t(q)
    ids, sc = ops.topk_items(q, t(x).to(T), k, bias=t(kw.pop("bias", None)), exclude=t(kw.pop("exclude", None), torch.int64), **kw)
    torch.cuda.synchronize()
    assert ids.dtype == torch.int64 and sc.dtype == torch.float32 and ids.shape == sc.shape == (q.shape[0], k)
    return ids.cpu().numpy(), sc.cpu().numpy().astype(np.float64)


def want(q, x, k, T, bias=None, ok=None):
    return O.rank(O.scores64(rounded(q, T), rounded(x, T), bias), O.valid_mask(len(q), len(x)) if ok is None else ok, k)


def assert_same(got, exp, what=""):
    np.testing.assert_array_equal(got[0], exp[0], err_msg=f"{what} ids")
    np.testing.assert_array_equal(got[1], exp[1], err_msg=f"{what} scores")


# M, D, V, K, nsplit: every D (scalar / 16-byte loads, the MFMA k step, the chunk edge), V, M, K (RB switches at 128 / 129,
# K > V) and nsplit of the issue at least twice; ranges of one, two and an odd number of tiles, ragged last tiles
INT_CASES = [(1, 1, 1, 1, 1), (1, 7, 63, 10, 2), (63, 8, 64, 128, 1), (65, 15, 65, 129, 3), (1, 16, 129, 256, 7),
             (63, 17, 4097, 10, 7), (65, 64, 4097, 128, 3), (1, 65, 4097, 129, 2), (63, 72, 129, 1, 1),
             (65, 136, 4097, 256, 7), (1, 136, 64, 10, 1), (65, 64, 129, 10, 2), (63, 64, 65, 256, 1), (1, 8, 4097, 1, 3),
             (65, 72, 63, 128, 2), (63, 1, 4097, 10, 1), (65, 16, 64, 129, 1), (1, 17, 65, 128, 2), (63, 65, 129, 129, 3),
             (65, 7, 1, 10, 1), (1, 15, 4097, 256, 1), (63, 136, 65, 10, 7), (65, 8, 129, 256, 7), (1, 64, 63, 1, 7)]


@gpu
@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("M,D,V,K,nsplit", INT_CASES)
def test_integer_data_match_the_oracle_bit_for_bit(M, D, V, K, nsplit, T):
    q, x, bias = ints(M + D + V + K, M, D, V)
    assert_same(run(q, x, K, T, bias=bias, nsplit=nsplit), want(q, x, K, T, bias))


@gpu
@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("D", [17, 72])
def test_bias_with_minus_inf_exclude_invalid_and_a_strided_q(D, T):
    M, V, K, S = 65, 4097, 129, 5
    q, x, bias = ints(D, M, D, V, lim=3)  # [-3, 3]: long runs of ties, so dropping an id moves many places
    bias[::7] = -np.inf
    rng = np.random.default_rng(1)
    exclude = rng.integers(-1, V, size=(M, S))
    top = want(q, x, K, T, bias)[0]
    exclude[:, 0] = top[:, 0]  # the best id of every row is excluded, the second of row 0 is invalid
    invalid = [int(top[0, 1]), 64, V - 1]
    wide = torch.zeros((M, D + 3), device="cuda:0")
    wide[:, :D] = t(q)
    got = run(wide[:, :D], x, K, T, bias=bias, exclude=exclude, invalid=invalid, nsplit=3)
    assert_same(got, want(q, x, K, T, bias, O.valid_mask(M, V, exclude, invalid)))


@gpu
@pytest.mark.parametrize("T,base", [(torch.float16, 1024), (torch.bfloat16, 128)])
def test_q_is_rounded_to_the_tables_type_ties_to_even(T, base):
    """q = n + j / 128 with n in [base, 2 base): T's spacing there is 1, so T drops the fraction -- j = 64 is an exact
    midpoint.  After rounding q is an integer below 2^12 and x in [-15, 15]: sums stay exact (D 2^12 15 < 2^24)."""
    M, D, V, K = 5, 24, 257, 10
    rng = np.random.default_rng(3)
    q = (rng.integers(base, 2 * base, size=(M, D)) + rng.integers(0, 128, size=(M, D)) / 128.0).astype(np.float32)
    q[0] = base + 2 + 0.5   # midpoints over an even integer: down
    q[1] = base + 3 + 0.5   # over an odd one: up
    _, x, _ = ints(4, M, D, V)
    x[0] = 15               # the best item of every (positive) query
    assert (rounded(q[0], T) == base + 2).all() and (rounded(q[1], T) == base + 4).all()
    got, exp = run(q, x, K, T), want(q, x, K, T)
    assert_same(got, exp)
    plain = O.rank(O.scores64(q, x), O.valid_mask(M, V), K)
    assert got[0][0, 0] == 0 and got[1][0, 0] < plain[1][0, 0] and got[1][1, 0] > plain[1][1, 0]


@gpu
@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("D,K", [(64, 10), (136, 200)])
def test_real_valued_data_within_the_accumulation_bound(D, K, T):
    """|score - s64| <= D 2^-24 sum_k |q~_k x_jk| (fp32 accumulation of exact products) + 2^-24 |score| (the bias add); the
    K-th returned score >= every left-out float64 score minus that id's bound (its score on the device is below the K-th
    and within the bound of its float64 score; |score| there is taken as |s64| + the first term).  No near-tie exemptions.
    nsplit 1, 3, 7 and one row alone give the same bits."""
    M, V = 65, 4097
    q, x, bias = O.normal_data(D + K, M, D, V, True)
    qr, xr = rounded(q, T), rounded(x, T)
    s64 = O.scores64(qr, xr, bias)
    acc = D * O.U * (np.abs(qr) @ np.abs(xr).T)
    ids, sc = run(q, x, K, T, bias=bias, nsplit=1)
    rows = np.arange(M)[:, None]
    assert (ids >= 0).all() and all(len(set(r)) == K for r in ids.tolist())
    err, bound = np.abs(sc - s64[rows, ids]), acc[rows, ids] + O.U * np.abs(sc)
    print(f"max |score - s64| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
    floor = s64 - acc - O.U * (np.abs(s64) + acc)
    floor[rows, ids] = -np.inf
    assert (sc[:, -1] >= floor.max(axis=1)).all()
    for nsplit in (3, 7):
        assert_same(run(q, x, K, T, bias=bias, nsplit=nsplit), (ids, sc), f"nsplit {nsplit}")
    alone = run(q[64:], x, K, T, bias=bias)
    assert_same(alone, (ids[64:], sc[64:]), "one row alone")


@gpu
@pytest.mark.parametrize("T", TYPES)
def test_ivf_scan_with_every_list_probed_equals_the_flat_scan(T):
    from torch_rechub_amd import ops
    lengths = [65, 0, 1, 63, 64, 0, 130, 7]
    M, D, K, V, nl = 9, 72, 129, sum(lengths), len(lengths)
    q, x, bias = ints(5, M, D, V, lim=3)
    lists = IO.lists_of_lengths(6, lengths)
    xs, bs, row_id, off = IO.group(x, bias, lists)
    probe = np.stack([np.random.default_rng(i).permutation(nl) for i in range(M)]).astype(np.int32)
    ids, sc = ops.ivf_scan(t(q), t(xs).to(T), t(row_id), t(off), t(probe), K, bias=t(bs), dtype=T)
    got = ids.cpu().numpy(), sc.cpu().numpy().astype(np.float64)
    assert_same(got, run(q, x, K, T, bias=bias), "against the flat scan")
    assert_same(got, want(q, x, K, T, bias), "against the oracle")


@gpu
@pytest.mark.parametrize("T", TYPES)
@pytest.mark.parametrize("metric", ["IP", "L2"])
@pytest.mark.parametrize("index_type", ["Flat", "IVF"])
def test_serving_half_index_equals_the_fp32_index_on_integer_data(index_type, metric, T, tmp_path):
    from torch_rechub_amd.serving import HipBuilder
    q, x, _ = ints(8, 33, 24, 300)
    kw = dict(index_type=index_type, nlists=4, nprobe=4, niter=2, device="cuda:0")
    with HipBuilder(metric, **kw).from_embeddings(torch.as_tensor(x)) as ref:
        exp = ref.query(torch.as_tensor(q), 20)
        ref.save(tmp_path / "f32.idx")
    builder = HipBuilder(metric, dtype=T, **kw)
    with builder.from_embeddings(torch.as_tensor(x)) as index:
        assert index._table.dtype == index._search.dtype == T and index._search.element_size() == 2
        got = index.query(torch.as_tensor(q), 20)
        index.save(tmp_path / "half.idx")
    with builder.from_index_file(tmp_path / "half.idx") as index:
        assert type(index) is type(ref) and index._search.dtype == T
        again = index.query(torch.as_tensor(q), 20)
    with builder.from_index_file(tmp_path / "f32.idx") as index:  # a file of the fp32 path keeps its type
        assert index._search.dtype == torch.float32
        old = index.query(torch.as_tensor(q), 20)
    for ids, val in (got, again, old):
        assert torch.equal(ids, exp[0]) and torch.equal(val, exp[1])


@gpu
def test_a_float32_table_takes_the_old_entry_with_the_same_bits(monkeypatch):
    from torch_rechub_amd import _lib, ops
    q, x, bias = O.int_data(2, 65, 72, 4097, True)
    called, call = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (called.append(name), call(name, *a))[1])
    ids, sc = ops.topk_items(t(q), t(x), 129, bias=t(bias), nsplit=3)
    assert "rh_topk_fwd" in called and "rh_topk_half_fwd" not in called
    assert_same((ids.cpu().numpy(), sc.cpu().numpy().astype(np.float64)),
                O.rank(O.scores64(q, x, bias), O.valid_mask(65, 4097), 129))


def test_other_table_types_are_refused_on_the_host():
    from torch_rechub_amd import ops
    from torch_rechub_amd.serving import HipBuilder
    i32 = torch.zeros(2, dtype=torch.int32)
    with pytest.raises(ValueError, match="was told dtype=torch.float32"):  # a half table has to be announced
        ops.ivf_scan(torch.zeros(2, 8), torch.zeros(5, 8).half(), i32, i32, i32, 3)
    for bad in (torch.float64, torch.int8):
        with pytest.raises(ValueError, match="float32, float16 or bfloat16"):
            ops.topk_items(torch.zeros(2, 8), torch.zeros(5, 8).to(bad), 3)
        with pytest.raises(ValueError, match="dtype must be one of"):
            HipBuilder("IP", dtype=bad)
