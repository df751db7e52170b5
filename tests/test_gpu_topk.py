"""ops.topk_items (csrc/topk.hip) on the MI355X against float64 brute force on the host (tests/topk_oracle.py).

Integer data (q, x in [-3, 3], bias in [-5, 5]) make every fp32 product and partial sum exact, so ids AND scores are
demanded element for element under the total order (score descending, id ascending); the data are full of exact ties.
Float data are checked with eps_i = 2 (D + 2) 2^-24 max_j (sum_d |q_id x_jd| + |bias_j|), the forward error bound of an
fp32 dot product counted once for each side of a comparison (topk_oracle.check_float)."""
import functools

import numpy as np
import pytest
import torch

import topk_oracle as O
from torch_rechub_amd._lib import H

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def t(a, dtype=None):
    return None if a is None else torch.as_tensor(a, dtype=dtype).to(dev())


def run(q, x, k, bias=None, exclude=None, invalid=None, nsplit=None):
    from torch_rechub_amd import ops
    ids, sc = ops.topk_items(t(q), t(x), k, bias=t(bias), exclude=t(exclude, torch.int64), invalid=invalid, nsplit=nsplit)
    torch.cuda.synchronize()
    assert ids.dtype == torch.int64 and sc.dtype == torch.float32 and ids.shape == sc.shape == (q.shape[0], k)
    return ids.cpu().numpy(), sc.cpu().numpy()


def assert_exact(got, want, what=""):
    ids, sc = got
    wi, ws = want
    np.testing.assert_array_equal(ids, wi, err_msg=f"{what} ids")
    np.testing.assert_array_equal(sc.astype(np.float64), ws, err_msg=f"{what} scores")


def ranges(V, nsplit):
    return [(V * s // nsplit, V * (s + 1) // nsplit) for s in range(nsplit)]


#             M   D    V     K    bias
INT_CASES = [(1, 1, 1, 1, False),        # the smallest problem
             (3, 7, 63, 10, True),       # less than one tile
             (65, 64, 64, 64, False),    # exactly one tile, K = V, two row blocks
             (3, 130, 65, 200, True),    # one column into the second tile, K > V, three k chunks
             (1, 130, 1, 10, False),     # K > V = 1
             (3, 1, 4097, 1, True),      # D = 1: almost every score tied
             (1, 64, 4097, 200, False),  # the examples' K; 32-row blocks
             (65, 7, 4097, H.RH_TOPK_MAX_K, True),   # the largest K, three row blocks of 32
             (3, 64, 65, H.RH_TOPK_MAX_K, False),    # K > V at the largest K
             (65, 130, 63, 64, True)]


@pytest.mark.parametrize("M,D,V,K,with_bias", INT_CASES)
def test_integer_data_match_the_oracle_bit_for_bit(M, D, V, K, with_bias):
    q, x, bias = O.int_data(100 + M + D + V + K, M, D, V, with_bias)
    want = O.rank(O.scores64(q, x, bias), O.valid_mask(M, V), K)
    assert_exact(run(q, x, K, bias), want)


def test_integer_data_at_the_planners_split():
    """V = 70001 with the planner's own nsplit (> 1 here): the top 200 of a row hold long runs of tied scores."""
    from torch_rechub_amd import ops
    M, D, V, K = 3, 130, 70001, 200
    nsplit, _ = ops.topk_plan(M, V, K)
    assert nsplit > 1
    q, x, bias = O.int_data(7, M, D, V, True)
    want = O.rank(O.scores64(q, x, bias), O.valid_mask(M, V), K)
    assert max(np.bincount(np.unique(want[1][0], return_inverse=True)[1])) > 10  # ties inside the top K
    assert_exact(run(q, x, K, bias), want)


def test_split_independence_with_ties_across_tile_and_range_boundaries():
    """nsplit 1, 2, 3, 7 at V = 4097, K = 200: copies of query 0's best row sit at ids 0, 63, 64, 4096 and at the first and
    last id of every range of every split, so that equal scores meet across tiles and ranges."""
    M, D, V, K = 3, 7, 4097, 200
    q, x, bias = O.int_data(11, M, D, V)
    best = int(O.rank(O.scores64(q, x), O.valid_mask(M, V), 1)[0][0, 0])
    plant = {0, 63, 64, V - 1}
    for n in (1, 2, 3, 7):
        for lo, hi in ranges(V, n):
            plant |= {lo, hi - 1}
    x[sorted(plant)] = x[best]
    want = O.rank(O.scores64(q, x), O.valid_mask(M, V), K)
    assert plant <= set(want[0][0].tolist())  # all tied at query 0's best score
    outs = [run(q, x, K, nsplit=n) for n in (1, 2, 3, 7)]
    for n, got in zip((1, 2, 3, 7), outs):
        assert_exact(got, want, f"nsplit={n}")
        assert got[0].tobytes() == outs[0][0].tobytes() and got[1].tobytes() == outs[0][1].tobytes()


def test_batch_independence():
    """One row queried alone, inside M = 65 and against a prefix of the table that still holds its top K: identical ids and
    score bits (a score depends on its own q_i, x_j and D only)."""
    M, D, V, K = 65, 130, 4097, 10
    q, x, _ = O.normal_data(21, M, D, V)
    ids_all, sc_all = run(q, x, K)
    i = int(np.argmin(ids_all.max(axis=1)))
    prefix = int(ids_all[i].max()) + 1
    assert prefix < V
    ids_one, sc_one = run(q[i:i + 1], x, K)
    ids_pre, sc_pre = run(q[i:i + 1], x[:prefix], K)
    for ids, sc in ((ids_one, sc_one), (ids_pre, sc_pre)):
        np.testing.assert_array_equal(ids[0], ids_all[i])
        assert sc[0].tobytes() == sc_all[i].tobytes()


@pytest.mark.parametrize("M,D,V,K,with_bias", [(3, 7, 4097, 10, False), (65, 64, 70001, 200, True), (5, 130, 4097, 256, False)])
def test_float_data_within_the_derived_tolerance(M, D, V, K, with_bias):
    q, x, bias = O.normal_data(31 + D, M, D, V, with_bias)
    ids, sc = run(q, x, K, bias)
    O.check_float(ids, sc, O.scores64(q, x, bias), O.valid_mask(M, V), O.eps_rows(q, x, bias), K, f"({M},{D},{V},{K})")


@functools.lru_cache(maxsize=None)
def exclusion_problem():
    M, D, V = 3, 7, 4097
    q, x, bias = O.int_data(41, M, D, V, True)
    s = O.scores64(q, x, bias)
    top = O.rank(s, O.valid_mask(M, V), 64)[0]
    return q, x, bias, s, top


@pytest.mark.parametrize("S", [0, 1, 50, 1024])
def test_exclusion(S):
    """exclude holds each row's own best ids, duplicates, -1 padding and ids >= V; invalid = [0]."""
    q, x, bias, s, top = exclusion_problem()
    M, V, K = q.shape[0], x.shape[0], 10
    rng = np.random.default_rng(S)
    exclude = None
    if S > 0:
        exclude = np.full((M, S), -1, dtype=np.int64)
        for i in range(M):
            own = top[i, :min(S, 20)]
            fill = np.concatenate([own, own[:5], [V, V + 5, 2 ** 40, -1], rng.integers(0, V, size=S // 3)])[:S]
            exclude[i, :len(fill)] = fill
            exclude[i] = exclude[i][rng.permutation(S)]
    ok = O.valid_mask(M, V, exclude, [0])
    want = O.rank(s, ok, K)
    got = run(q, x, K, bias, exclude, [0])
    for i in range(M):
        assert ok[i, got[0][i]].all() and 0 not in got[0][i]
    if S > 0:
        assert not (set(got[0][0].tolist()) & set(top[0, :min(S, 20)].tolist()))
    assert_exact(got, want)


def test_exclusion_leaving_fewer_than_k_candidates():
    """Everything but K - 3 ids is excluded: the tail is (-1, -inf)."""
    M, D, V, K = 3, 7, 300, 10
    q, x, bias = O.int_data(43, M, D, V, True)
    rng = np.random.default_rng(0)
    exclude = np.full((M, 1024), -1, dtype=np.int64)
    for i in range(M):
        gone = rng.permutation(np.arange(1, V))[:V - 1 - (K - 3)]  # id 0 goes through `invalid`
        exclude[i, :len(gone)] = gone
    ok = O.valid_mask(M, V, exclude, [0])
    assert (ok.sum(axis=1) == K - 3).all()
    got = run(q, x, K, bias, exclude, torch.tensor([0], device=dev()))
    assert (got[0][:, K - 3:] == -1).all() and np.isneginf(got[1][:, K - 3:]).all()
    assert_exact(got, O.rank(O.scores64(q, x, bias), ok, K))


@pytest.mark.parametrize("K", [10, 256])
def test_worst_case_order_every_element_inserts(K):
    """The table sorted by ascending score for the query: every column beats the threshold and is inserted."""
    V = 4097
    q = np.ones((1, 1), dtype=np.float32)
    x = (np.arange(V, dtype=np.float32) - 2000.0).reshape(V, 1)
    want = O.rank(O.scores64(q, x), O.valid_mask(1, V), K)
    assert want[0][0, 0] == V - 1
    for nsplit in (1, 3):
        assert_exact(run(q, x, K, nsplit=nsplit), want)


def test_two_calls_give_the_same_bits():
    q, x, bias = O.normal_data(51, 65, 64, 4097, True)
    a, b = run(q, x, 64, bias), run(q, x, 64, bias)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_memory_stays_far_below_the_logits():
    """M = 256, V = 70001, K = 10: the call's peak above what was allocated before stays below M V bytes (a quarter of
    the fp32 logits), and is exactly the planned workspace plus the two outputs, up to the allocator's 512-byte rounding."""
    from torch_rechub_amd import ops
    M, D, V, K = 256, 64, 70001, 10
    q, x, _ = O.normal_data(61, M, D, V)
    qd, xd = t(q), t(x)
    nsplit, nbytes = ops.topk_plan(M, V, K)
    assert nbytes == 8 * M * nsplit * K
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ids, sc = ops.topk_items(qd, xd, K)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise} bytes; workspace {nbytes}, outputs {M * K * 12}; M V = {M * V}")
    assert rise < M * V
    assert rise <= nbytes + M * K * 12 + 3 * 512
    O.check_float(ids.cpu().numpy()[:2], sc.cpu().numpy()[:2], O.scores64(q[:2], x), O.valid_mask(2, V),
                  O.eps_rows(q[:2], x), K, "memory case")


def test_refusals(monkeypatch):
    """D = 1025, K = 257, S = 1025, a non-contiguous table and CPU tensors raise before anything is launched."""
    from torch_rechub_amd import _lib, ops
    real, launched = _lib.call, []

    def spy(name, *a):
        if name == "rh_topk_fwd":
            launched.append(name)
        return real(name, *a)

    monkeypatch.setattr(_lib, "call", spy)
    q, x = torch.zeros(2, 8, device=dev()), torch.zeros(300, 8, device=dev())
    assert ops.topk_supported(1024, 256, 1024)
    assert not ops.topk_supported(1025, 1, 0) and not ops.topk_supported(8, 257, 0) and not ops.topk_supported(8, 1, 1025)
    assert not ops.topk_supported(0, 1, 0) and not ops.topk_supported(8, 0, 0)
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.topk_items(torch.zeros(2, 1025, device=dev()), torch.zeros(300, 1025, device=dev()), 5)
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.topk_items(q, x, 257)
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.topk_items(q, x, 5, exclude=torch.zeros(2, 1025, dtype=torch.int64, device=dev()))
    with pytest.raises(ValueError, match="contiguous"):
        ops.topk_items(q, torch.zeros(8, 300, device=dev()).t(), 5)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.topk_items(q.cpu(), x.cpu(), 5)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.topk_items(q, x.cpu(), 5)
    with pytest.raises(ValueError, match="nsplit"):
        ops.topk_items(q, x, 5, nsplit=301)
    assert not launched
    ids, sc = ops.topk_items(q[:0], x, 5)  # M = 0 returns at once
    assert ids.shape == (0, 5) and sc.shape == (0, 5) and not launched
