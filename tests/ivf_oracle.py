"""Float64 numpy oracle of the inverted-file index (tests/test_ivf_host.py, tests/test_gpu_ivf.py): the grouping of a
table by explicit lists, the top K over the union of the probed lists (ranked by tests/topk_oracle.py on ORIGINAL ids),
the coarse selection, Lloyd's k-means, and the generator of the training case with its gap condition."""
import numpy as np

import topk_oracle as O

U = O.U
LLOYD_SEEDS = (0, 1, 9)  # of lloyd_data: the seeds whose gap condition tests/test_ivf_host.py asserts


def random_lists(seed, V, nlists, empty=()):
    """A random partition of range(V) into nlists lists (ascending ids each); the lists named in ``empty`` get no row."""
    rng = np.random.default_rng(seed)
    live = np.array([l for l in range(nlists) if l not in set(empty)])
    owner = live[rng.integers(0, len(live), size=V)]
    return [np.nonzero(owner == l)[0] for l in range(nlists)]


def lists_of_lengths(seed, lengths):
    """A partition of range(sum(lengths)) into lists of the given lengths, ids shuffled over the lists."""
    perm = np.random.default_rng(seed).permutation(int(sum(lengths)))
    cut = np.cumsum([0] + list(lengths))
    return [np.sort(perm[cut[i]:cut[i + 1]]) for i in range(len(lengths))]


def group(x, bias, lists):
    """(xs, bias_s, row_id int32, list_off int32): the table grouped by list, ids ascending inside each list."""
    order = np.concatenate([np.sort(np.asarray(l, dtype=np.int64)) for l in lists]) if len(lists) else np.zeros(0, np.int64)
    off = np.cumsum([0] + [len(l) for l in lists]).astype(np.int32)
    return (np.ascontiguousarray(x[order]), None if bias is None else np.ascontiguousarray(bias[order]),
            order.astype(np.int32), off)


def probed_mask(M, V, lists, probe):
    """(M, V) bool: row j lies in a list that query i probes; probe entries outside [0, len(lists)) are no list."""
    ok = np.zeros((M, V), dtype=bool)
    for i in range(M):
        for l in probe[i]:
            if 0 <= l < len(lists):
                ok[i, np.asarray(lists[l], dtype=np.int64)] = True
    return ok


def valid(M, V, lists, probe, exclude=None):
    return probed_mask(M, V, lists, probe) & O.valid_mask(M, V, exclude)


def ivf_rank(q, x, bias, lists, probe, k, exclude=None):
    """(ids (M, k) int64 original ids, scores (M, k) float64): the k best rows of the probed lists that are not excluded,
    by (score descending, id ascending); tail (-1, -inf)."""
    return O.rank(O.scores64(q, x, bias), valid(q.shape[0], x.shape[0], lists, probe, exclude), k)


def coarse(q, centroids, nprobe, metric):
    """(M, nprobe) int64: the lists a query probes, in float64: the largest q . c for "IP", else the smallest
    |q - c|^2 (the largest 2 q . c - |c|^2); ties to the lower list.  ("angular": pass unit queries.)"""
    q, c = q.astype(np.float64), centroids.astype(np.float64)
    s = q @ c.T if metric == "IP" else 2.0 * q @ c.T - (c * c).sum(1)[None, :]
    return O.rank(s, np.ones(s.shape, dtype=bool), nprobe)[0]


def assign(x, centroids):
    """(n,) int64 nearest centroid in float64, ties to the lower list; and the (n, nlists) scores 2 x . c - |c|^2."""
    x, c = x.astype(np.float64), centroids.astype(np.float64)
    s = 2.0 * x @ c.T - (c * c).sum(1)[None, :]
    return np.argmax(s, axis=1), s  # argmax: the first of equal maxima


def lists_of(a, nlists):
    return [np.nonzero(a == l)[0] for l in range(nlists)]


def list_mean(x, lists, previous):
    """float64 means of the lists' rows; an empty list keeps ``previous``."""
    out = previous.astype(np.float64).copy()
    for l, rows in enumerate(lists):
        if len(rows):
            out[l] = x[rows].astype(np.float64).mean(axis=0)
    return out


def centroid_bound(x, n):
    """What the fp32 mean of n rows may be off by per coordinate: (n + 2) 2^-24 max |x| (n - 1 additions of terms up to
    max |x| each, divided by n, plus the division's and the final rounding)."""
    return (n + 2) * U * float(np.abs(x).max())


def gap_bound(x, centroids, n):
    """What fp32 can move the difference of two of a row's scores 2 x . c - |c|^2 by: twice (once per side) the sum of
    the dot-product error in ``topk_oracle.eps_rows`` form, 2 (D + 2) 2^-24 max (2 |x| . |c| + |c|^2), and the shift of a
    score when every coordinate of c moves by d = centroid_bound: 2 d max (|x|_1 + |c|_1) + D d^2."""
    D = x.shape[1]
    ax, ac = np.abs(x).astype(np.float64), np.abs(centroids).astype(np.float64)
    dot = 2.0 * (D + 2) * U * float((2.0 * ax @ ac.T + (ac * ac).sum(1)[None, :]).max())
    d = centroid_bound(x, n)
    shift = 2.0 * d * float(ax.sum(1).max() + ac.sum(1).max()) + D * d * d
    return 2.0 * (dot + shift)


def lloyd(x, init, niter):
    """Float64 Lloyd's k-means as the device build runs it: ``niter`` rounds of assign + mean, then a final assign.
    -> dict(assign = the final partition, centroids = the final centroids (float64), ratio = the smallest
    gap / gap_bound over every row and every assign (the final one included), moved = the rounds whose assignment
    differs from the round before, sizes = the final list sizes, mean_sizes = the sizes of the lists whose means the final
    centroids are)."""
    c = init.astype(np.float64)
    nl = c.shape[0]
    ratio, moved, prev, n_prev, mean_sizes = np.inf, 0, None, 1, np.zeros(nl, dtype=np.int64)
    for r in range(niter + 1):
        a, s = assign(x, c)
        top2 = np.sort(s, axis=1)[:, -2:]
        gap = float((top2[:, 1] - top2[:, 0]).min()) if nl > 1 else np.inf
        ratio = min(ratio, gap / gap_bound(x, c, n_prev))
        if prev is not None and (a != prev).any():
            moved += 1
        prev = a
        if r < niter:
            ls = lists_of(a, nl)
            c = list_mean(x, ls, c)
            mean_sizes = np.array([len(l) for l in ls])
            n_prev = int(mean_sizes.max())
    return {"assign": a, "centroids": c, "ratio": ratio, "moved": moved, "sizes": np.bincount(a, minlength=nl),
            "mean_sizes": mean_sizes}


def lloyd_data(seed):
    """(x (222, 5) fp32, init (6, 5) fp32): six clusters of 37 rows, centres 4 N(0, 1), rows = centre + N(0, 1); the
    start is the first two rows of cluster 0 and the first row of clusters 1 .. 4 -- cluster 5 has no seed, so rows
    migrate over several rounds."""
    rng = np.random.default_rng(seed)
    centres = 4.0 * rng.standard_normal((6, 5))
    x = (centres[:, None, :] + rng.standard_normal((6, 37, 5))).reshape(6 * 37, 5).astype(np.float32)
    start = [0, 1] + [37 * c for c in range(1, 5)]
    return x, x[start].copy()
