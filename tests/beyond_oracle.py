"""Float64 restatement of the reference's three beyond-accuracy loops (diversity_score, coverage_score, novelty_score of
torch_rechub/basic/metric.py), per user and per cut-off, for the tests of basic.metric and of csrc/metric.hip.

``pred`` is an (M, K) id array whose rows are the users.  An id below 0 is an absent position (the -1 padding of
``ops.topk_items``): the user's list at cut-off k is ``[i for i in row[:k] if i >= 0]``, which for a padded tail is the
reference run on a dict of the rows with the negative entries removed.  (The reference itself would index numpy from the
end on a -1; that is not reproduced.)  Diversity keeps the reference's pairwise form: the k x k matrix of cosines.
"""
import numpy as np

from metric_oracle import rounding_margin  # noqa: F401  (shared with the tests)


def lists(pred, k):
    return [[int(i) for i in row[:k] if i >= 0] for row in np.asarray(pred)]


def diversity(pred, table, cutoffs):
    """-> (M, n_k) float64: the mean pairwise cosine distance among the known items (id < V) of the first k; nan where
    fewer than two are known."""
    table = np.asarray(table)
    V = len(table)
    out = np.full((len(pred), len(cutoffs)), np.nan)
    for q, k in enumerate(cutoffs):
        for u, items in enumerate(lists(pred, k)):
            if len(items) < 2:
                continue
            vectors = [np.array(table[i], dtype=np.float64) for i in items if i < V]
            if len(vectors) < 2:
                continue
            vectors = np.stack(vectors)
            unit = vectors / np.maximum(np.linalg.norm(vectors, axis=1, keepdims=True), 1e-10)
            n = len(vectors)
            distance = (1 - unit @ unit.T)[np.triu_indices(n, k=1)].sum()
            out[u, q] = distance / (n * (n - 1) / 2)
    return out


def coverage(pred, cutoffs):
    """-> [number of distinct ids among the users' first k] per cut-off."""
    counts = []
    for k in cutoffs:
        seen = set()
        for items in lists(pred, k):
            seen.update(items)
        counts.append(len(seen))
    return counts


def novelty(pred, pop, cutoffs):
    """-> (M, n_k) float64: the mean of -log2(max(p, 1e-10)) over the user's first k, p = 1e-10 beyond the table; nan for an
    empty list.  ``pop`` is widened to float64 first."""
    pop = np.asarray(pop).astype(np.float64)
    known = {i: pop[i] for i in range(len(pop))}
    out = np.full((len(pred), len(cutoffs)), np.nan)
    for q, k in enumerate(cutoffs):
        for u, items in enumerate(lists(pred, k)):
            if not items:
                continue
            out[u, q] = np.mean([-np.log2(max(known.get(i, 1e-10), 1e-10)) for i in items])
    return out


def means(per_user):
    """The mean over the users that contributed, per cut-off; 0.0 where nobody did."""
    out = []
    for column in np.asarray(per_user).T:
        values = column[~np.isnan(column)]
        out.append(float(np.mean(values)) if len(values) else 0.0)
    return out


def strings(name, values, cutoffs):
    """['Name@k: x', ...] rounded to the fourth decimal like the reference (a mean of nobody prints as 0.0)."""
    return [f"{name}@{k}: {round(np.float64(v), 4)}" for k, v in zip(cutoffs, values)]


def coverage_strings(counts, n_items, cutoffs):
    return [f"Coverage@{k}: {round(c / n_items, 4)}" for k, c in zip(cutoffs, counts)]
