"""rh_ild, rh_coverage and rh_novelty through ops and basic.metric, against tests/beyond_oracle.py (the reference's loops in
float64, run on the rows with the negative entries removed).

Diversity, per user, absolute 2e-12 on values in [0, 2].  The kernel forms 1 - (||S||^2 - Q) / (n (n - 1)) with
S = sum u_i and Q = sum ||u_i||^2 in double: S carries n roundings per component, ||S||^2 another D, so the identity's
rounding is bounded by about 2 (n + D) 2^-53 n / (n - 1) <= 2.9e-13 at n = 256, D = 1024; the oracle's own BLAS product
carries the same order; together below 1e-12, and the factor of two is margin.

Novelty, per user, absolute 4e-12: a double log2 is within 3 ulp (2.1e-14 at the largest term, 33.3), summation adds
(k - 1) 2^-53 33.3 <= 9.4e-13 at k = 256: under 1e-12 in total, and the factor of four is margin.

Coverage is a count: exact.  Sums over users: the per-user bound times the number of users that contributed."""
import numpy as np
import pytest
import torch

import beyond_cases as C
import beyond_oracle as O
from conftest import load_golden
from torch_rechub_amd._lib import H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ILD_TOL, NOV_TOL = 2e-12, 4e-12
WIDTHS = [1, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, H.RH_ILD_MAX_D]
LENGTHS = [1, 2, 63, 64, 65, 128, 129, H.RH_RANK_MAX_K]
EIGHT = [7, 2, 9, 1, 9, 4, 3, 8]  # unsorted, with a duplicate


@pytest.fixture(scope="module")
def ops():
    from torch_rechub_amd import ops
    return ops


@pytest.fixture(scope="module")
def metric():
    import torch_rechub_amd.basic.metric as metric
    return metric


def dev(a):
    return torch.as_tensor(a).to(DEV)


def check_means(raw, want, tol):
    """sums and counts of an op's result against the oracle's per-user values."""
    present = ~np.isnan(want)
    counts = present.sum(0)
    assert raw["counts"].tolist() == counts.tolist()
    sums = np.where(present, want, 0.0).sum(0)
    np.testing.assert_allclose(raw["sums"].cpu().numpy(), sums, rtol=0, atol=tol * max(1, int(counts.max())))


def check_ild(ops, pred, table, cutoffs, ids=None, emb=None):
    """ops.ild with per-user values against the oracle; ``ids`` / ``emb``: the device tensors to pass (views)."""
    raw = ops.ild(dev(pred) if ids is None else ids, dev(table) if emb is None else emb, cutoffs, per_user=True)
    want = O.diversity(pred, table, cutoffs)
    got = raw["per_user"].cpu().numpy()
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=0, atol=ILD_TOL)
    check_means(raw, want, ILD_TOL)
    return raw, want


def check_novelty(ops, pred, pop, cutoffs, ids=None):
    raw = ops.novelty(dev(pred) if ids is None else ids, dev(pop), cutoffs, per_user=True)
    want = O.novelty(pred, pop, cutoffs)
    got = raw["per_user"].cpu().numpy()
    assert np.array_equal(np.isnan(got), np.isnan(want))
    np.testing.assert_allclose(got, want, rtol=0, atol=NOV_TOL)
    check_means(raw, want, NOV_TOL)
    return raw, want


def check_coverage(ops, pred, n_slots, cutoffs, ids=None):
    got = ops.coverage(dev(pred) if ids is None else ids, n_slots, cutoffs)["counts"].tolist()
    inside = np.where((pred >= 0) & (pred < n_slots), pred, -1)
    assert got == O.coverage(inside, cutoffs)
    return got


# ---- diversity -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", WIDTHS)
def test_ild_over_the_embedding_widths(ops, D):
    pred, table, _ = C.make(D, 5, 9, 50, D)
    check_ild(ops, pred, table, [2, 5, 9])


@pytest.mark.parametrize("K", LENGTHS)
def test_ild_over_the_list_lengths(ops, K):
    pred, table, _ = C.make(100 + K, 4, K, 500, 16)
    raw, _ = check_ild(ops, pred, table, sorted({1, K, max(1, K // 2)}))
    assert raw["counts"][0].item() == 0  # k = 1: nobody has a pair
    if K >= 64:  # wider rows take other lane layouts; the long walk is theirs too
        for D in (3, 64, 260):
            check_ild(ops, pred, C.make(K, 1, 1, 500, D)[1], [K, K - 1])


def test_ild_refuses_what_lies_outside_its_ranges(ops):
    ids, table = dev(np.zeros((2, 4), np.int64)), dev(np.ones((3, 4), np.float32))
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.ild(ids, dev(np.ones((3, 1025), np.float32)), [2])
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.ild(dev(np.zeros((2, 257), np.int64)), table, [2])
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.ild(ids, table, [1, 2, 3, 4, 1, 2, 3, 4, 1])  # nine cut-offs
    for bad in ([], [0], [5]):
        with pytest.raises(ValueError, match="cut-offs"):
            ops.ild(ids, table, bad)
    with pytest.raises(ValueError, match="int64"):
        ops.ild(ids.int(), table, [2])
    with pytest.raises(ValueError, match="float32"):
        ops.ild(ids, table.double(), [2])
    with pytest.raises(ValueError, match="float32"):
        ops.ild(ids, table[0], [2])


def test_ild_over_the_user_counts_and_past_the_grid_cap(ops):
    users, max_grid, _ = ops.ild_plan(1)
    for M in (1, 3, 4, 5, users * max_grid + 1):
        pred, table, _ = C.make(M, M, 2, 30, 4, pad=M <= 5)
        raw, want = check_ild(ops, pred, table, [2])
        if M > 5:
            assert raw["counts"].item() == (~np.isnan(want)).sum() > users * max_grid // 2


def test_ild_cutoffs(ops, metric):
    pred, table, _ = C.make(21, 6, 9, 40, 12)
    raw, _ = check_ild(ops, pred, table, [1])
    assert raw["counts"].tolist() == [0] and raw["sums"].tolist() == [0.0] and raw["per_user"].isnan().all()
    assert metric.diversity_score(dev(pred), dev(table), topKs=[1])["Diversity"] == ["Diversity@1: 0.0"]
    check_ild(ops, pred, table, [9])
    raw, _ = check_ild(ops, pred, table, EIGHT)
    assert torch.equal(raw["per_user"][:, 2].nan_to_num(-1.), raw["per_user"][:, 4].nan_to_num(-1.))  # the duplicate


def test_ild_ids(ops):
    """-1 tails of differing lengths, a row of -1 only, ids beyond the table, duplicates, exactly one and two known items."""
    V = 6
    table = np.random.default_rng(22).standard_normal((V, 8)).astype(np.float32)
    pred = np.array([[0, 1, 2, 3, 4, 5], [2, 3, -1, -1, -1, -1], [4, -1, -1, -1, -1, -1], [-1] * 6, [6, 7, 100, 2 ** 40, 6, 9],
                     [1, 1, 1, 5, 5, 1], [9, 3, 8, -1, -1, -1], [9, 3, 8, 0, -1, -1], [5, 2 ** 62, 2, 7, 7, 7]], dtype=np.int64)
    raw, want = check_ild(ops, pred, table, [2, 4, 6])
    assert raw["counts"].tolist() == [3, 5, 5]
    assert np.isnan(want[6]).all() and np.isnan(want[7, 0]) and not np.isnan(want[7, 1])
    assert raw["per_user"][5, 0].item() == pytest.approx(0.0, abs=ILD_TOL)  # a duplicate is at distance 0 from its twin


def test_ild_values(ops):
    """Zero rows, norms below the clamp, and float32 magnitudes near 1e30 and 1e-30 in one list."""
    rng = np.random.default_rng(23)
    table = rng.standard_normal((8, 20)).astype(np.float32)
    table[1] = 0.0
    table[2] *= np.float32(1e-12)   # norm ~ 4e-12: clamped, the unit vector is short
    table[3] *= np.float32(1e30)
    table[4] *= np.float32(1e-30)   # norm ~ 4e-30: clamped
    table[5] *= np.float32(3e-11)   # on the clamp's edge
    pred = np.array([[0, 1, 6, 7], [1, 1, 0, 2], [3, 4, 0, 3], [2, 5, 2, 6], [3, 7, 4, 1], [4, 4, 2, 2]], dtype=np.int64)
    raw, want = check_ild(ops, pred, table, [2, 3, 4])
    assert want[0, 0] == 1.0 and want[1, 0] == 1.0  # a zero row is at distance 1 from everything, itself included
    assert raw["per_user"][1, 0].item() == 1.0
    assert np.isfinite(want).all() and 0.5 < want[2, 2] < 1.5


@pytest.mark.parametrize("D", [23, 24, 300])
def test_ild_exact_cases(ops, D):
    table = np.zeros((11, D), np.float32)
    for i in range(8):
        table[i, 3 * i] = 2.0 ** (i - 4)          # pairwise-orthogonal axis vectors, power-of-two scales
    table[8, 5], table[9, 5], table[10, 5] = 2.0 ** 100, 2.0 ** -30, -4.0   # one axis, both signs, norms above the clamp
    pred = np.array([[0, 1, 2, 3, 4, 5, 6, 7], [8, 9, 8, 9, 8, 8, 9, 9], [9, 10, -1, -1, -1, -1, -1, -1],
                     [10, 8, -1, -1, -1, -1, -1, -1]], dtype=np.int64)
    got = ops.ild(dev(pred), dev(table), [2, 8], per_user=True)["per_user"].cpu().numpy()
    assert got[0].tolist() == [1.0, 1.0]
    assert got[1].tolist() == [0.0, 0.0]
    assert got[2].tolist() == [2.0, 2.0] and got[3].tolist() == [2.0, 2.0]


def test_ild_reads_strided_views_in_place(ops):
    pred, table, _ = C.make(24, 7, 40, 60, 20)
    wide_ids = dev(np.concatenate([pred, np.full((7, 9), 3)], 1))
    wide_table = dev(np.concatenate([table, np.full((60, 5), 7, np.float32)], 1))
    ids, emb = wide_ids[:, :40], wide_table[:, :20]
    assert not ids.is_contiguous() and not emb.is_contiguous()
    raw, _ = check_ild(ops, pred, table, [3, 40], ids=ids, emb=emb)
    same = ops.ild(dev(pred), dev(table), [3, 40], per_user=True)
    assert torch.equal(raw["per_user"].nan_to_num(-1.), same["per_user"].nan_to_num(-1.))
    odd = dev(np.concatenate([table, np.zeros((60, 1), np.float32)], 1))[:, :20]  # a row stride of 21 floats
    assert torch.equal(ops.ild(ids, odd, [3, 40])["sums"], same["sums"])


def test_ild_is_reproducible_and_a_user_does_not_depend_on_the_batch(ops):
    pred, table, _ = C.make(25, 37, 50, 400, 64)
    ids, emb = dev(pred), dev(table)
    a, b = ops.ild(ids, emb, [5, 20, 50], per_user=True), ops.ild(ids, emb, [5, 20, 50], per_user=True)
    assert torch.equal(a["sums"], b["sums"]) and torch.equal(a["counts"], b["counts"])
    assert torch.equal(a["per_user"].nan_to_num(-1.), b["per_user"].nan_to_num(-1.))
    for u in (0, 17, 36):
        alone = ops.ild(ids[u:u + 1], emb, [5, 20, 50], per_user=True)["per_user"]
        assert torch.equal(alone[0].nan_to_num(-1.), a["per_user"][u].nan_to_num(-1.))


def test_ild_allocates_no_gather(ops):
    M, K, D, V = 4096, 64, 64, 5000
    rng = np.random.default_rng(26)
    ids, emb = dev(rng.integers(0, V, (M, K))), dev(rng.standard_normal((V, D)).astype(np.float32))
    cut = [5, 20, 64]
    ops.ild(ids, emb, cut)  # the library is loaded, the stub allocations exist
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    raw = ops.ild(ids, emb, cut, per_user=True)
    torch.cuda.synchronize()
    declared = ops.ild_plan(M)[2] * 8 + sum(t.numel() * 8 for t in raw.values())
    assert torch.cuda.max_memory_allocated() - before <= (1 << 20) + declared
    assert M * K * D * 4 == 64 << 20 and declared < 1 << 20


# ---- coverage ------------------------------------------------------------------------------------------------------
def test_coverage_counts(ops):
    pred, _, _ = C.make(31, 9, 12, 90, 1)
    top = int(pred.max())
    for n_slots in (top + 1, top, top - 1, 40, 1):  # ids straddling n_slots - 1
        check_coverage(ops, pred, n_slots, [1, 5, 12])
    got = check_coverage(ops, pred, top + 1, EIGHT)
    assert got[2] == got[4] and got == ops.coverage(dev(pred), top + 1, EIGHT)["counts"].tolist()
    same = np.tile(np.arange(100, 164), (300, 1))  # every user recommends the same K ids
    assert check_coverage(ops, same, 164, [1, 63, 64]) == [1, 63, 64]
    assert check_coverage(ops, np.zeros((5, 3), np.int64), 1, [1, 3]) == [1, 1]
    assert check_coverage(ops, np.full((5, 3), -1), 1, [1, 3]) == [0, 0]
    assert check_coverage(ops, np.array([[3, 0], [-1, -1]]), 1, [1, 2]) == [0, 1]


def test_coverage_sees_the_first_column_of_an_item(ops):
    """Item 7 first appears at column 3: outside cut-off 3, inside cut-off 4, whichever user writes last."""
    pred = np.array([[0, 1, 2, 3, 4, 7], [0, 1, 2, 7, 4, 5], [0, 1, 2, 3, 7, 7]], dtype=np.int64)
    assert check_coverage(ops, pred, 8, [3, 4, 5, 6]) == [3, 5, 6, 7]
    assert check_coverage(ops, pred[::-1].copy(), 8, [3, 4, 5, 6]) == [3, 5, 6, 7]


def test_coverage_past_both_grid_caps(ops):
    """One row more than a full grid of the marking pass and five slots more than a full grid of the counting pass; the
    oracle here is numpy's set of the ids."""
    rows, max_grid, _ = ops.coverage_plan(1)
    M, n_slots = rows * max_grid + 1, 256 * max_grid + 5
    pred = np.random.default_rng(33).integers(-1, n_slots + 9, (M, 2))
    pred[-1] = [n_slots - 1, n_slots - 2]
    got = ops.coverage(dev(pred), n_slots, [1, 2])["counts"].tolist()
    want = [len(np.unique(part[(part >= 0) & (part < n_slots)])) for part in (pred[:, :1], pred)]
    assert got == want and want[1] > want[0] > n_slots // 2


def test_coverage_over_the_shape_edges(ops):
    users, max_grid, _ = ops.ild_plan(1)
    for K in LENGTHS:
        pred, _, _ = C.make(200 + K, 5, K, 3 * K + 5, 1)
        check_coverage(ops, pred, 3 * K + 5, sorted({1, K, max(1, K // 2)}))
    for M in (1, 3, 4, 5, 257, users * max_grid + 1):
        pred, _, _ = C.make(300 + M, M, 2, 4 * M, 1, pad=M <= 5)
        check_coverage(ops, pred, 4 * M, [1, 2])
    wide = dev(np.concatenate([C.make(32, 6, 10, 50, 1)[0], np.full((6, 4), 49)], 1))
    check_coverage(ops, wide[:, :10].cpu().numpy(), 50, [2, 10], ids=wide[:, :10])
    ids = dev(np.zeros((2, 4), np.int64))
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.coverage(dev(np.zeros((2, 257), np.int64)), 4, [2])
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.coverage(ids, 4, [1] * 9)
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.coverage(ids, 2 ** 31, [1])
    with pytest.raises(ValueError, match="n_slots"):
        ops.coverage(ids, 0, [1])


# ---- novelty -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_novelty_per_user(ops, dtype):
    pred, _, pop = C.make(41, 9, 12, 90, 1, dtype=dtype)
    pop[:4] = [0.0, 1e-12, 1.0, 1e-10]
    pred[0, :4] = [0, 1, 2, 3]
    raw, want = check_novelty(ops, pred, pop, [1, 5, 12])
    assert np.isnan(want[1]).all() and not np.isnan(want[0]).any()
    check_novelty(ops, pred, pop, EIGHT)
    again = ops.novelty(dev(pred), dev(pop), [1, 5, 12], per_user=True)
    assert torch.equal(again["sums"], raw["sums"]) and torch.equal(again["counts"], raw["counts"])
    assert torch.equal(again["per_user"].nan_to_num(-1.), raw["per_user"].nan_to_num(-1.))
    ones = ops.novelty(dev(np.array([[2, 2, -1], [2, -1, -1]])), dev(pop), [1, 3], per_user=True)
    assert ones["per_user"].tolist() == [[0.0, 0.0], [0.0, 0.0]] and ones["sums"].tolist() == [0.0, 0.0]
    clamp = ops.novelty(dev(np.array([[0, 1, 200]])), dev(pop), [3], per_user=True)["per_user"].item()
    assert clamp == pytest.approx(-np.log2(1e-10), abs=NOV_TOL)


def test_novelty_over_the_shape_edges(ops):
    users, max_grid, _ = ops.novelty_plan(1)
    for K in LENGTHS:
        pred, _, pop = C.make(400 + K, 5, K, 3 * K + 5, 1)
        check_novelty(ops, pred, pop, sorted({1, K, max(1, K // 2)}))
    for M in (1, 3, 4, 5, users * max_grid + 1):
        pred, _, pop = C.make(500 + M, M, 2, 50, 1, pad=M <= 5)
        check_novelty(ops, pred, pop, [1, 2])
    pred, _, pop = C.make(42, 6, 10, 50, 1)
    wide = dev(np.concatenate([pred, np.full((6, 4), 49)], 1))
    check_novelty(ops, pred, pop, [2, 10], ids=wide[:, :10])
    ids = dev(np.zeros((2, 4), np.int64))
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.novelty(dev(np.zeros((2, 257), np.int64)), dev(pop), [2])
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.novelty(ids, dev(pop), [1] * 9)
    with pytest.raises(ValueError, match="popularity"):
        ops.novelty(ids, dev(pop).half(), [1])
    with pytest.raises(ValueError, match="popularity"):
        ops.novelty(ids, dev(pop).reshape(5, 10), [1])


@pytest.mark.parametrize("cutoffs", [[65], [1, 2, 3, 5, 8, 13, 21, 65]])
def test_ild_and_novelty_over_a_ragged_count_of_partials(ops, cutoffs):
    """133 users are 34 workgroups, the last with one user: more partials than the final sum has parts (32) and no multiple
    of them, at one cut-off and at eight.  The other tests end in 1, 2, at most 10, 1024 or 2048 partials."""
    pred, table, pop = C.make(133, 133, 65, 400, 16)
    raw, _ = check_ild(ops, pred, table, cutoffs)
    again = ops.ild(dev(pred), dev(table), cutoffs)
    assert torch.equal(again["sums"], raw["sums"]) and torch.equal(again["counts"], raw["counts"])
    raw, _ = check_novelty(ops, pred, pop, cutoffs)
    again = ops.novelty(dev(pred), dev(pop), cutoffs)
    assert torch.equal(again["sums"], raw["sums"]) and torch.equal(again["counts"], raw["counts"])


# ---- basic.metric --------------------------------------------------------------------------------------------------
def all_cases():
    c = load_golden("metric_cases.npz")
    fixture = C.fixture_case(c)
    golden = {"Diversity": c["beyond_Diversity"].tolist(), "Coverage": c["beyond_Coverage"].tolist(),
              "Novelty": c["beyond_Novelty"].tolist()}
    return [("fixture", fixture, golden)] + [(name, C.string_case(name), None) for name in C.STRING_CASES]


def test_basic_metric_strings_on_the_device_path(ops, metric, monkeypatch):
    calls = []
    for name in ("ild", "coverage", "novelty"):
        def spy(*args, _fn=getattr(ops, name), _name=name, **kwargs):
            calls.append(_name)
            return _fn(*args, **kwargs)
        monkeypatch.setattr(ops, name, spy)
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **k: pytest.fail("a tensor was copied to the host"))
    for name, f, golden in all_cases():
        cut = f["cutoffs"]
        want = {"Diversity": O.strings("Diversity", O.means(O.diversity(f["pred"], f["table"], cut)), cut),
                "Coverage": O.coverage_strings(O.coverage(f["pred"], cut), f["catalogue"], cut),
                "Novelty": O.strings("Novelty", O.means(O.novelty(f["pred"], f["pop"], cut)), cut)}
        assert golden is None or golden == want
        ids = dev(f["pred"])
        del calls[:]
        got = metric.diversity_score(ids, dev(f["table"]), topKs=cut)
        assert got["Diversity"] == want["Diversity"] and got["missing"] == [], name
        assert metric.coverage_score(ids, range(f["catalogue"]), topKs=cut)["Coverage"] == want["Coverage"], name
        assert metric.coverage_score(ids, f["catalogue"], topKs=tuple(cut))["Coverage"] == want["Coverage"], name
        assert metric.novelty_score(ids, dev(f["pop"]), topKs=cut)["Novelty"] == want["Novelty"], name
        assert metric.novelty_score(ids, dev(f["pop"]).double(), topKs=cut)["Novelty"] == want["Novelty"], name
        assert calls == ["ild", "coverage", "coverage", "novelty", "novelty"]
    assert metric.diversity_score(dev(np.arange(12).reshape(2, 6)), dev(np.eye(12, dtype=np.float32)))["Diversity"] == \
        ["Diversity@5: 1.0"]  # the default cut-off


def test_unsupported_combinations_stay_on_the_host_path(ops, metric, monkeypatch):
    for name in ("ild", "coverage", "novelty"):
        monkeypatch.setattr(ops, name, lambda *a, **k: pytest.fail("the device op was called"))
    c = load_golden("metric_cases.npz")
    cut = [int(k) for k in c["beyond_cutoffs"]]
    ids = dev(c["beyond_pred"])
    embs = {i: row.tolist() for i, row in enumerate(c["beyond_embs"])}
    popularity = {i: p for i, p in enumerate(c["beyond_pop"])}
    assert metric.diversity_score(ids, embs, topKs=cut)["Diversity"] == c["beyond_Diversity"].tolist()  # a dict of embeddings
    assert metric.diversity_score(ids, c["beyond_embs"], topKs=cut)["Diversity"] == c["beyond_Diversity"].tolist()
    assert metric.diversity_score(ids, dev(c["beyond_embs"]).double(), topKs=cut)["Diversity"] == c["beyond_Diversity"].tolist()
    assert metric.novelty_score(ids, popularity, topKs=cut)["Novelty"] == c["beyond_Novelty"].tolist()
    host = torch.from_numpy(c["beyond_pred"])
    catalogue = set(range(int(c["beyond_catalogue"])))
    assert metric.coverage_score(host, catalogue, topKs=cut)["Coverage"] == c["beyond_Coverage"].tolist()
    assert metric.coverage_score(ids.int(), catalogue, topKs=cut)["Coverage"] == c["beyond_Coverage"].tolist()
