"""Float64 / Python-int restatement of the evaluation metrics, for the tests of basic.metric and csrc/metric.hip.

* ``rank_stat``: per group the exact integers P (positives), N (negatives) and
  U2 = sum over positives of 2 #{negatives of the group below} + #{negatives of the group tied}; AUC = U2 / (2 P N).
  Ties are equal values: numpy compares float32 values on the CPU without flushing denormals, and -0.0 == +0.0.
* ``gauc``: sum_u w_u AUC_u / sum_u w_u, the users in the order of their first appearance, added one by one.
* ``log_loss``: the predictions widened to float64 first.
* ``list_metrics``: hit, mrr, recall, precision, ndcg per user and cut-off in float64, position by position, and their sums.
"""
import math

import numpy as np


def rank_stat(pred, label, group=None):
    """-> (P, N, U2): lists of Python ints of length G = max(group) + 1 (1 without groups)."""
    pred = np.asarray(pred, dtype=np.float32).astype(np.float64) + 0.0  # -0.0 + 0.0 = +0.0: one value, one sort key
    pos = np.asarray(label).astype(np.float64) == 1.0
    n = pred.shape[0]
    group = np.zeros(n, dtype=np.int64) if group is None else np.asarray(group, dtype=np.int64)
    G = int(group.max()) + 1 if n else 1
    P, N, U2 = [0] * G, [0] * G, [0] * G
    order = np.lexsort((pred, group))
    sg, sp, spos = group[order], pred[order], pos[order]
    starts = np.flatnonzero(np.r_[True, sg[1:] != sg[:-1]])
    ends = np.r_[starts[1:], n]
    for lo, hi in zip(starts, ends):
        g = int(sg[lo])
        v, is_pos = sp[lo:hi], spos[lo:hi]
        negs = v[~is_pos]  # ascending
        below = np.searchsorted(negs, v[is_pos], side="left")
        through = np.searchsorted(negs, v[is_pos], side="right")
        P[g] = int(is_pos.sum())
        N[g] = int(hi - lo) - P[g]
        U2[g] = int(below.astype(np.int64).sum()) + int(through.astype(np.int64).sum())  # 2 below + tied = below + through
    return P, N, U2


def auc(pred, label):
    P, N, U2 = rank_stat(pred, label)
    return U2[0] / (2 * P[0] * N[0])


def gauc(pred, label, users, weights=None):
    """``weights``: anything indexable by user id, or None for the users' sample counts.  nan with a single-class user."""
    users = np.asarray(users)
    seen = {}
    for u in users.tolist():
        seen.setdefault(u, len(seen))
    dense = np.array([seen[u] for u in users.tolist()], dtype=np.int64)
    P, N, U2 = rank_stat(pred, label, dense)
    num, den = 0.0, 0.0
    for u, g in seen.items():
        if P[g] == 0 or N[g] == 0:
            return float("nan")
        w = float(P[g] + N[g]) if weights is None else float(weights[u])
        num += (U2[g] / (2 * P[g] * N[g])) * w
        den += w
    return num / den


def log_loss(pred, label):
    p = np.asarray(pred, dtype=np.float32).astype(np.float64)
    y = np.asarray(label).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        terms = y * np.log(p) + (1.0 - y) * np.log(1.0 - p)
    return float(-terms.sum() / len(p))


def list_metrics(pred, truth, cutoffs):
    """``pred``: (M, K) ids, ``truth``: M id lists.  -> dict: per_user (M, n_k, 5) float64 = hit, mrr, recall, precision,
    ndcg; hits [n_k] ints; gts int; sums (n_k, 4) float64 = mrr, recall, precision, ndcg added user by user."""
    pred = np.asarray(pred)
    M = pred.shape[0]
    per_user = np.zeros((M, len(cutoffs), 5), dtype=np.float64)
    hits, gts = [0] * len(cutoffs), 0
    sums = np.zeros((len(cutoffs), 4), dtype=np.float64)
    for u in range(M):
        wanted = list(truth[u])
        if not wanted:
            continue
        gts += len(wanted)
        members = set(wanted)
        row = pred[u].tolist()
        for q, k in enumerate(cutoffs):
            hit, first, dcg, idcg = 0, None, 0.0, 0.0
            for j in range(k):
                gain = 1.0 / float(np.log2(j + 2))
                if row[j] in members:
                    hit += 1
                    first = j if first is None else first
                    dcg += gain
                if j < len(wanted):
                    idcg += gain
            values = (float(hit), 0.0 if first is None else 1.0 / (1 + first), hit / len(wanted), hit / k, dcg / idcg)
            per_user[u, q] = values
            hits[q] += hit
            sums[q] += values[1:]
    return {"per_user": per_user, "hits": hits, "gts": gts, "sums": sums}


def list_strings(result, cutoffs, n_users):
    """{'NDCG': ['NDCG@k: x', ...], ...} from ``list_metrics``' result, rounded to the fourth decimal like the reference."""
    out = {name: [] for name in ("NDCG", "MRR", "Recall", "Hit", "Precision")}
    for q, k in enumerate(cutoffs):
        mrr, recall, precision, ndcg = (float(v) for v in result["sums"][q])
        values = {"Hit": result["hits"][q] / result["gts"], "MRR": mrr / n_users, "Recall": recall / n_users,
                  "Precision": precision / n_users, "NDCG": ndcg / n_users}
        for name in out:
            out[name].append(f"{name}@{k}: {round(values[name], 4)}")
    return out


def unrounded(result, cutoffs, n_users):
    """The values ``list_strings`` rounds, flat."""
    vals = []
    for q in range(len(cutoffs)):
        vals.append(result["hits"][q] / result["gts"])
        vals.extend(float(v) / n_users for v in result["sums"][q])
    return vals


def rounding_margin(value, digits=4):
    """Distance of ``value`` from the nearest rounding boundary of its ``digits``-th decimal."""
    scaled = abs(value) * 10 ** digits
    return abs(scaled - math.floor(scaled) - 0.5) / 10 ** digits
