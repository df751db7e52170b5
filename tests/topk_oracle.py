"""Float64 brute force for the top-K retrieval tests (tests/test_gpu_topk.py, tests/test_gpu_serving.py): the scores, the
ranking under the total order (score descending, id ascending), and the derived-tolerance criterion for float data."""
import numpy as np

U = 2.0 ** -24  # unit roundoff of fp32


def int_data(seed, M, D, V, with_bias=False):
    """q, x from the integers in [-3, 3] and bias from [-5, 5], as fp32: every product and partial sum is exact in fp32
    in any order (|score| <= 9 D + 5 < 2^24), and the scores are full of exact ties."""
    rng = np.random.default_rng(seed)
    q = rng.integers(-3, 4, size=(M, D)).astype(np.float32)
    x = rng.integers(-3, 4, size=(V, D)).astype(np.float32)
    bias = rng.integers(-5, 6, size=(V,)).astype(np.float32) if with_bias else None
    return q, x, bias


def normal_data(seed, M, D, V, with_bias=False):
    rng = np.random.default_rng(seed)
    q = rng.standard_normal((M, D)).astype(np.float32)
    x = rng.standard_normal((V, D)).astype(np.float32)
    bias = rng.standard_normal((V,)).astype(np.float32) if with_bias else None
    return q, x, bias


def scores64(q, x, bias=None):
    s = q.astype(np.float64) @ x.astype(np.float64).T
    return s if bias is None else s + bias.astype(np.float64)[None, :]


def valid_mask(M, V, exclude=None, invalid=None):
    ok = np.ones((M, V), dtype=bool)
    if exclude is not None:
        for i in range(M):
            e = np.asarray(exclude[i], dtype=np.int64)
            ok[i, e[(e >= 0) & (e < V)]] = False
    if invalid is not None:
        e = np.asarray(invalid, dtype=np.int64)
        ok[:, e[(e >= 0) & (e < V)]] = False
    return ok


def rank(s, ok, k):
    """(ids (M, k) int64, scores (M, k) float64): the k best valid columns of each row of s by (score descending, id
    ascending); tail (-1, -inf)."""
    M, V = s.shape
    ids = np.full((M, k), -1, dtype=np.int64)
    out = np.full((M, k), -np.inf)
    for i in range(M):
        cand = np.nonzero(ok[i])[0]
        order = cand[np.argsort(-s[i, cand], kind="stable")][:k]  # stable: equal scores keep ascending ids
        ids[i, :len(order)] = order
        out[i, :len(order)] = s[i, order]
    return ids, out


def eps_rows(q, x, bias=None):
    """eps_i = 2 (D + 2) 2^-24 max_j (sum_d |q_id x_jd| + |bias_j|): the forward error bound of an fp32 dot product of
    length D (plus the bias add), counted once for each side of a comparison."""
    D = q.shape[1]
    mag = np.abs(q).astype(np.float64) @ np.abs(x).astype(np.float64).T
    if bias is not None:
        mag = mag + np.abs(bias).astype(np.float64)[None, :]
    return 2.0 * (D + 2) * U * mag.max(axis=1)


def check_float(ids, scores, s64, ok, eps, k, what="", tie_order=True):
    """Criterion for float data: k distinct valid ids; each returned score within eps_i / 2 of its float64 score; the
    smallest float64 score among the returned ids >= the largest among the valid others - eps_i; returned order
    non-increasing in the returned score, ascending ids on equal scores (``tie_order=False``: the scores were recovered
    from a transformed value that may merge neighbours, so equal ones say nothing about the ids)."""
    M, V = s64.shape
    for i in range(M):
        got, sc = ids[i], scores[i].astype(np.float64)
        n = min(k, int(ok[i].sum()))
        assert (got[n:] == -1).all() and np.isneginf(sc[n:]).all(), (what, i)
        got, sc = got[:n], sc[:n]
        assert ((got >= 0) & (got < V)).all() and len(set(got.tolist())) == n and ok[i, got].all(), (what, i)
        err = np.abs(sc - s64[i, got]).max() if n else 0.0
        print(f"{what} row {i}: max |score - float64| = {err:.3e} (eps / 2 = {eps[i] / 2:.3e})")
        assert err <= eps[i] / 2, (what, i, err, eps[i])
        rest = ok[i].copy()
        rest[got] = False
        if n and rest.any():
            lo, hi = s64[i, got].min(), s64[i, rest].max()
            print(f"{what} row {i}: min returned - max left out = {lo - hi:.3e} (>= -eps = {-eps[i]:.3e})")
            assert lo >= hi - eps[i], (what, i, lo, hi, eps[i])
        d = np.diff(sc)
        assert (d <= 0).all(), (what, i)
        assert not tie_order or (np.diff(got)[d == 0] > 0).all(), (what, i)
