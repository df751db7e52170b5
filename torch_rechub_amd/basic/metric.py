"""Evaluation metrics: ``auc_score``, ``gauc_score``, ``log_loss``, ``topk_metrics`` and its five wrappers, and the
beyond-accuracy trio ``diversity_score`` / ``coverage_score`` / ``novelty_score`` (reference torch_rechub/basic/metric.py).

Every function takes the reference's host inputs (arrays, dicts of lists) and then returns what the reference returns,
down to the ``defaultdict`` of ``'NDCG@5: 0.1234'`` strings.  ``auc_score``, ``gauc_score``, ``log_loss`` and
``topk_metrics`` (with ``ndcg_score``, ``hit_score``, ``mrr_score``, ``recall_score``, ``precision_score``) also take HIP
tensors and then run on the kernels of csrc/metric.hip through ``ops`` -- no copy of the predictions to the host, no
Python loop over users -- and return the same Python objects:

* ``auc_score(y_true, y_pred)`` / ``gauc_score(y_true, y_pred, users, weights)``: 1-D device tensors; the AUC is the exact
  rational U2 / (2 P N) (``roc_auc_score`` differs from it by float64 summation order only);
* ``topk_metrics(y_true, y_pred, topKs)``: ``y_pred`` an (M, K) int64 id tensor (what ``ops.topk_items`` leaves on the
  device), ``y_true`` an ``(offsets, ids)`` CSR pair of device tensors or a row-aligned list of id lists.

The beyond-accuracy trio runs on the device too when ``y_pred`` is such an (M, K) int64 HIP id tensor (rows are users; an
id below 0 is an absent position, the -1 padding of ``ops.topk_items``: that user's list is shorter there):

* ``diversity_score(y_pred, item_embeddings, topKs)`` with ``item_embeddings`` a 2-D float32 HIP tensor indexed by item id:
  ``ops.ild``, O(k D) per user, no (M, K, D) gather and no k x k matrix;
* ``novelty_score(y_pred, item_popularity, topKs)`` with ``item_popularity`` a 1-D HIP tensor indexed by item id;
* ``coverage_score(y_pred, all_items, topKs)`` with ``all_items`` anything with a ``len``, or the catalogue size as an int.

The oracle of each is the reference run on a dict of the rows with the negative entries removed.  Every other combination
of inputs (dicts, host tensors, a dict of embeddings beside a device ``y_pred``) takes the host loops below.
"""
from collections import defaultdict

import numpy as np

_LIST_METRICS = ("NDCG", "MRR", "Recall", "Hit", "Precision")


def _on_device(x):
    import torch
    return torch.is_tensor(x) and x.is_cuda


def _host(x):
    """A device or host tensor as a numpy array; anything else unchanged."""
    import torch
    return x.detach().cpu().numpy() if torch.is_tensor(x) else x


def auc_score(y_true, y_pred):
    if _on_device(y_pred) or _on_device(y_true):
        from .. import ops
        return ops.auc(y_pred, y_true)
    from sklearn.metrics import roc_auc_score
    return roc_auc_score(y_true, y_pred)


def get_user_pred(y_true, y_pred, users):
    """{user id: {'y_true': [...], 'y_pred': [...]}} in the order in which the users first appear."""
    y_true, y_pred, users = _host(y_true), _host(y_pred), _host(users)
    by_user = {}
    for label, score, user in zip(y_true, y_pred, users):
        entry = by_user.get(user)
        if entry is None:
            entry = by_user[user] = {"y_true": [], "y_pred": []}
        entry["y_true"].append(label)
        entry["y_pred"].append(score)
    return by_user


def gauc_score(y_true, y_pred, users, weights=None):
    """The users' AUCs averaged under ``weights`` ({user id: weight}; on the device a 1-D tensor indexed by user id), by
    default under the number of samples of each user."""
    if _on_device(y_pred) or _on_device(y_true) or _on_device(users):
        from .. import ops
        return ops.gauc(y_pred, y_true, users, weights)
    assert len(y_true) == len(y_pred) and len(y_true) == len(users)
    total, norm = 0, 0
    for user, entry in get_user_pred(y_true, y_pred, users).items():
        w = len(entry["y_true"]) if weights is None else weights[user]
        total += auc_score(entry["y_true"], entry["y_pred"]) * w
        norm += w
    return total / norm


def _topk_strings(topKs, hits, gts, sums, n_users):
    """The reference's result object from the raw sums: per cut-off hits / gts and the four per-user sums over the users."""
    rows = []
    for q in range(len(topKs)):
        mrr, recall, precision, ndcg = sums[q]
        rows.append({"Hit": round(hits[q] / gts, 4), "MRR": round(mrr / n_users, 4), "Recall": round(recall / n_users, 4),
                     "Precision": round(precision / n_users, 4), "NDCG": round(ndcg / n_users, 4)})
    results = defaultdict(list)
    for k, row in zip(topKs, rows):
        for name in _LIST_METRICS:
            results[name].append(f"{name}@{k}: {row[name]}")
    return results


def _topk_host_sums(truth, pred, topKs):
    hits, sums, gts = [], [], 0
    for q, k in enumerate(topKs):
        n_hit, mrr, recall, precision, ndcg, gts = 0, 0, 0, 0, 0, 0
        for wanted, ranked in zip(truth, pred):
            if len(wanted) == 0:
                continue
            found, first, dcg, idcg = 0., None, 0, 0
            for j in range(k):
                gain = 1. / np.log2(j + 2)
                if ranked[j] in wanted:
                    found += 1.
                    if first is None:
                        first = j
                    dcg += gain
                if j < len(wanted):
                    idcg += gain
            gts += len(wanted)
            n_hit += found
            mrr += 0 if first is None else 1. / (1 + first)
            recall += found / len(wanted)
            precision += found / k
            if idcg != 0:
                ndcg += dcg / idcg
        hits.append(n_hit)
        sums.append((mrr, recall, precision, ndcg))
    return hits, gts, sums


def topk_metrics(y_true, y_pred, topKs=None):
    """NDCG, MRR, Recall, Hit and Precision at every cut-off of ``topKs`` -> {'NDCG': ['NDCG@5: 0.1234', ...], ...}.

    Host form: ``y_true`` {user: interacted ids}, ``y_pred`` {user: recommended ids}.  Device form: ``y_pred`` an (M, K)
    int64 HIP tensor, ``y_true`` an (offsets, ids) pair of HIP tensors or a row-aligned list of id lists."""
    if topKs is None:
        topKs = [5]
    if _on_device(y_pred):
        if not isinstance(topKs, (tuple, list)):
            raise ValueError("topKs wrong, it should be tuple or list")
        from .. import ops
        raw = ops.rank_metrics(y_pred, y_true, topKs)
        return _topk_strings(topKs, raw["hits"].tolist(), int(raw["gts"]), raw["sums"].tolist(), int(y_pred.shape[0]))
    assert len(y_true) == len(y_pred)
    if not isinstance(topKs, (tuple, list)):
        raise ValueError("topKs wrong, it should be tuple or list")
    users = list(y_true.keys())
    hits, gts, sums = _topk_host_sums([y_true[u] for u in users], [y_pred[u] for u in users], topKs)
    return _topk_strings(topKs, hits, gts, sums, len(users))


def ndcg_score(y_true, y_pred, topKs=None):
    return topk_metrics(y_true, y_pred, topKs)["NDCG"]


def hit_score(y_true, y_pred, topKs=None):
    return topk_metrics(y_true, y_pred, topKs)["Hit"]


def mrr_score(y_true, y_pred, topKs=None):
    return topk_metrics(y_true, y_pred, topKs)["MRR"]


def recall_score(y_true, y_pred, topKs=None):
    return topk_metrics(y_true, y_pred, topKs)["Recall"]


def precision_score(y_true, y_pred, topKs=None):
    return topk_metrics(y_true, y_pred, topKs)["Precision"]


def log_loss(y_true, y_pred):
    if _on_device(y_pred) or _on_device(y_true):
        from .. import ops
        return ops.log_loss(y_pred, y_true)
    terms = y_true * np.log(y_pred) + (1 - y_true) * np.log(1 - y_pred)
    return -terms.sum() / len(y_true)


def _host_lists(y_pred):
    """{user: [item ids]} of a recommendation given as a dict or as an (M, K) tensor (rows become users 0 .. M - 1)."""
    import torch
    if torch.is_tensor(y_pred):
        return dict(enumerate(y_pred.detach().cpu().tolist()))
    return y_pred


def _mean_score(values):
    return round(np.mean(values), 4) if values else 0.0


def _device_lists(y_pred):
    """True for the device form of a recommendation: an (M, K) int64 HIP tensor."""
    import torch
    return _on_device(y_pred) and y_pred.dim() == 2 and y_pred.dtype == torch.int64


def _device_table(x):
    import torch
    return _on_device(x) and x.dim() == 2 and x.dtype == torch.float32


def _device_means(name, topKs, raw):
    """The reference's result object from the raw sums of ``ops.ild`` / ``ops.novelty``: the mean over the users that
    contributed, 0.0 when nobody did."""
    results = defaultdict(list)
    for k, total, count in zip(topKs, raw["sums"].tolist(), raw["counts"].tolist()):
        results[name].append(f"{name}@{k}: {round(np.float64(total) / count, 4) if count else 0.0}")
    return results


def diversity_score(y_pred, item_embeddings, topKs=None):
    """Intra-list diversity: the mean pairwise cosine distance inside each user's top-k list, averaged over the users whose
    list has at least two items with a known embedding.  ``item_embeddings``: {item id: vector} or a 2-D array indexed by
    item id.  -> {'Diversity': ['Diversity@5: 0.xxxx', ...]}.

    Device form: ``y_pred`` an (M, K) int64 HIP tensor, ``item_embeddings`` a (V, D) float32 HIP tensor; the result is the
    reference's on a dict of the rows with the negative entries (absent positions) removed."""
    if topKs is None:
        topKs = [5]
    if _device_lists(y_pred) and _device_table(item_embeddings):
        from .. import ops
        return _device_means("Diversity", topKs, ops.ild(y_pred, item_embeddings, topKs))
    y_pred, item_embeddings = _host_lists(y_pred), _host(item_embeddings)
    known = (lambda i: i in item_embeddings) if isinstance(item_embeddings, dict) else (lambda i: i < len(item_embeddings))
    results = defaultdict(list)
    for k in topKs:
        per_user = []
        for items in y_pred.values():
            items = items[:k]
            if len(items) < 2:
                continue
            vectors = [np.array(item_embeddings[i], dtype=np.float64) for i in items if known(i)]
            if len(vectors) < 2:
                continue
            vectors = np.stack(vectors)
            unit = vectors / np.maximum(np.linalg.norm(vectors, axis=1, keepdims=True), 1e-10)
            n = len(vectors)
            distance = (1 - unit @ unit.T)[np.triu_indices(n, k=1)].sum()
            per_user.append(distance / (n * (n - 1) / 2))
        results["Diversity"].append(f"Diversity@{k}: {_mean_score(per_user)}")
    return results


def coverage_score(y_pred, all_items, topKs=None):
    """Catalogue coverage: the share of ``all_items`` that appears in at least one user's top-k list.
    -> {'Coverage': ['Coverage@5: 0.xxxx', ...]}.

    Device form: ``y_pred`` an (M, K) int64 HIP tensor, ``all_items`` anything with a ``len`` or the catalogue size as an
    int; the result is the reference's on a dict of the rows with the negative entries (absent positions) removed."""
    if topKs is None:
        topKs = [5]
    if _device_lists(y_pred):
        from .. import ops
        n_items = all_items if isinstance(all_items, int) else len(all_items)
        n_slots = max(int(y_pred.max()), 0) + 1  # every id >= 0 counts, inside ``all_items`` or not, as in the reference
        counts = ops.coverage(y_pred, n_slots, topKs)["counts"].tolist()
        results = defaultdict(list)
        for k, count in zip(topKs, counts):
            results["Coverage"].append(f"Coverage@{k}: {round(count / n_items, 4)}")
        return results
    y_pred = _host_lists(y_pred)
    results = defaultdict(list)
    for k in topKs:
        seen = set()
        for items in y_pred.values():
            seen.update(items[:k])
        results["Coverage"].append(f"Coverage@{k}: {round(len(seen) / len(all_items), 4)}")
    return results


def novelty_score(y_pred, item_popularity, topKs=None):
    """Mean self-information -log2(popularity) of the recommended items, per user and then over users; an unknown item
    and a popularity below 1e-10 count as 1e-10.  -> {'Novelty': ['Novelty@5: x.xxxx', ...]}.

    Device form: ``y_pred`` an (M, K) int64 HIP tensor, ``item_popularity`` a 1-D float32 or float64 HIP tensor indexed by
    item id; the result is the reference's on a dict of the rows with the negative entries (absent positions) removed."""
    if topKs is None:
        topKs = [5]
    if _device_lists(y_pred) and _on_device(item_popularity) and item_popularity.dim() == 1:
        from .. import ops
        return _device_means("Novelty", topKs, ops.novelty(y_pred, item_popularity, topKs))
    y_pred = _host_lists(y_pred)
    results = defaultdict(list)
    for k in topKs:
        per_user = []
        for items in y_pred.values():
            items = items[:k]
            if not items:
                continue
            per_user.append(np.mean([-np.log2(max(item_popularity.get(i, 1e-10), 1e-10)) for i in items]))
        results["Novelty"].append(f"Novelty@{k}: {_mean_score(per_user)}")
    return results
