"""Evaluation metrics (csrc/metric.hip): exact AUC / GAUC, log loss, top-K list metrics, and the beyond-accuracy metrics
(intra-list diversity, catalogue coverage, novelty)."""
import ctypes

import torch

from .. import _lib
from .._opcore import _p, _stream, require_hip


_LABEL_DTYPES = {torch.float32: 0, torch.float64: 1, torch.int64: 2, torch.uint8: 3, torch.bool: 3}


_rank_tables = {}


_PLAN_OUT = (ctypes.c_int, ctypes.c_int, ctypes.c_int64)  # what the metric kernels' plans answer with


def auc_plan(n):
    """(chunk, max_grid, workspace_bytes) of rh_auc_groups over n samples: the sorted elements a workgroup takes per trip,
    the grid cap (more chunks than that are further trips) and the scratch size."""
    return _lib.query("rh_auc_plan", int(n), out=_PLAN_OUT)


def _metric_inputs(what, pred, label, *more):
    """The guards of the pointwise metrics, before anything is allocated or launched.  -> (pred 1-D, possibly strided;
    label 1-D contiguous; n)."""
    require_hip(pred, label, *more)
    if pred.dtype != torch.float32:
        raise ValueError(f"torch_rechub_amd: {what} takes float32 predictions, got {pred.dtype}")
    if label.dtype not in _LABEL_DTYPES:
        raise ValueError(f"torch_rechub_amd: {what} takes float32, float64, int64, uint8 or bool labels, got {label.dtype}")
    if pred.numel() != label.numel() or any(t.numel() != pred.numel() for t in more):
        raise ValueError(f"torch_rechub_amd: {what}: {[tuple(t.shape) for t in (pred, label) + more]} do not agree")
    n = int(pred.numel())
    if n == 0:
        raise ValueError(f"torch_rechub_amd: {what} of an empty input")
    if n >= 2 ** 31:
        raise ValueError(f"torch_rechub_amd: {what} takes fewer than 2**31 samples, got {n}")
    pred = pred.detach()
    if pred.dim() != 1:
        pred = pred.reshape(-1)
    return pred, label.detach().reshape(-1).contiguous(), n


def _auc_groups(pred, label, g, G, n):
    dev = pred.device
    ps = int(pred.stride(0)) if n > 1 else 1
    keys = torch.empty((n,), dtype=torch.int64, device=dev)
    _lib.call("rh_auc_keys", _p(pred), ps, _p(g), n, _p(keys), _stream())
    order = torch.sort(keys).indices  # the permutation is plumbing: the counting below is the metric
    del keys
    work = torch.empty((auc_plan(n)[2],), dtype=torch.uint8, device=dev)
    out = torch.empty((3, G), dtype=torch.int64, device=dev)
    bad = torch.empty((2,), dtype=torch.int64, device=dev)
    _lib.call("rh_auc_groups", _p(pred), ps, _p(label), _LABEL_DTYPES[label.dtype], _p(g), _p(order), n, G, _p(work), _p(out),
              _p(bad), _stream())
    nonfinite, badlabel = bad.tolist()
    if nonfinite:
        raise ValueError(f"torch_rechub_amd: {nonfinite} predictions are NaN or infinite")
    if badlabel:
        raise ValueError(f"torch_rechub_amd: {badlabel} labels are neither 0 nor 1")
    return out


def auc_groups(pred, label, group=None):
    """(P, N, U2), int64 tensors of length G: per group the positives, the negatives and the rank statistic
    U2 = sum over positives of 2 #{negatives below} + #{negatives tied}, so that AUC_g = U2 / (2 P N) exactly.  ``group``:
    dense int64 ids in [0, G) with G = max + 1, or None for one group.  Ties are equal VALUES (-0.0 == +0.0, distinct
    denormals distinct).  NaN / infinite predictions and labels other than 0 / 1 raise ValueError.  No autograd; current
    stream."""
    more = () if group is None else (group,)
    pred, label, n = _metric_inputs("auc_groups", pred, label, *more)
    G, g = 1, None
    if group is not None:
        if group.dtype != torch.int64:
            raise ValueError(f"torch_rechub_amd: auc_groups takes int64 group ids, got {group.dtype}")
        g = group.detach().reshape(-1).contiguous()
        lo, hi = int(g.min()), int(g.max())
        if lo < 0 or hi >= 2 ** 31 - 1:
            raise ValueError(f"torch_rechub_amd: auc_groups takes dense group ids in [0, G), G < 2**31; got [{lo}, {hi}]")
        G = hi + 1
    out = _auc_groups(pred, label, g, G, n)
    return out[0], out[1], out[2]


def auc(pred, label):
    """roc_auc_score(label, pred) as a Python float: the exact rational U2 / (2 P N), correctly rounded."""
    P, N, U2 = (int(t) for t in auc_groups(pred, label))
    if P == 0 or N == 0:
        raise ValueError("Only one class present in y_true. ROC AUC score is not defined in that case.")
    return U2 / (2 * P * N)


def gauc(pred, label, users, weights=None):
    """sum_u w_u AUC_u / sum_u w_u over the distinct values u of ``users`` (any int64 tensor); w_u = the samples of u, or
    ``weights[u]`` (a 1-D tensor indexed by user id).  nan when a user holds one class only."""
    pred, label, n = _metric_inputs("gauc", pred, label, users)
    if users.dtype != torch.int64:
        raise ValueError(f"torch_rechub_amd: gauc takes int64 user ids, got {users.dtype}")
    if weights is not None:
        require_hip(weights)
        if weights.dim() != 1:
            raise ValueError("torch_rechub_amd: gauc takes a 1-D weight tensor indexed by user id")
    uniq, g = torch.unique(users.detach().reshape(-1), return_inverse=True)
    G = int(uniq.numel())
    w = None
    if weights is not None:
        if int(uniq[0]) < 0 or int(uniq[-1]) >= weights.numel():
            raise ValueError("torch_rechub_amd: gauc: a user id lies outside the weight tensor")
        w = weights.detach()[uniq].to(torch.float64).contiguous()
    stats = _auc_groups(pred, label, g.contiguous(), G, n)
    dev = pred.device
    partial = torch.empty((3072,), dtype=torch.float64, device=dev)
    result = torch.empty((2,), dtype=torch.float64, device=dev)
    single = torch.empty((1,), dtype=torch.int64, device=dev)
    _lib.call("rh_gauc_reduce", _p(stats), _p(w), G, _p(partial), _p(result), _p(single), _stream())
    if int(single):
        return float("nan")
    num, den = result.tolist()
    return num / den


def log_loss(pred, label):
    """-mean(y log p + (1 - y) log(1 - p)) as a Python float; p is widened to double before the logarithms."""
    pred, label, n = _metric_inputs("log_loss", pred, label)
    dev = pred.device
    partial = torch.empty((1024,), dtype=torch.float64, device=dev)
    result = torch.empty((1,), dtype=torch.float64, device=dev)
    _lib.call("rh_log_loss", _p(pred), int(pred.stride(0)) if n > 1 else 1, _p(label), _LABEL_DTYPES[label.dtype], n,
              _p(partial), _p(result), _stream())
    return float(result)


def rank_metrics_plan(M):
    """(stage, users_per_workgroup, max_grid, partial_doubles) of rh_rank_metrics over M users."""
    return _lib.query("rh_rank_metrics_plan", int(M), out=(ctypes.c_int,) + _PLAN_OUT)


def rank_gain_tables(K):
    """(gain (K,), ideal (K + 1,)) as float64 numpy arrays: gain[j] = 1 / log2(j + 2) position by position, ideal its
    sequential prefix sums from 0 -- the operands and the order of additions of the host loop."""
    import numpy as np
    gain = np.array([1. / np.log2(j + 2) for j in range(K)], dtype=np.float64)
    ideal = np.zeros(K + 1, dtype=np.float64)
    for j in range(K):
        ideal[j + 1] = ideal[j] + gain[j]
    return gain, ideal


def pack_truth(truth, device):
    """A list of id lists as the CSR pair (offsets (M + 1,), ids) of int64 tensors on ``device``: packed once, on the host."""
    import numpy as np
    lens = np.fromiter((len(t) for t in truth), dtype=np.int64, count=len(truth))
    off = np.zeros(len(truth) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    ids = np.fromiter((i for t in truth for i in t), dtype=np.int64, count=int(off[-1]))
    return torch.from_numpy(off).to(device), torch.from_numpy(ids).to(device)


def rank_metrics(pred_ids, truth, cutoffs, per_user=False):
    """The raw sums behind the top-K list metrics.  ``pred_ids`` (M, K) int64 (what ``topk_items`` returns; a strided
    ``ids[:, :k]`` view is read in place), ``truth`` an (offsets, ids) pair of int64 device tensors or a row-aligned list of
    id lists, ``cutoffs`` at most 8 ints in [1, K].  -> dict: ``hits`` (n_k,) int64, ``gts`` (1,) int64, ``sums`` (n_k, 4)
    float64 = mrr, recall, precision, ndcg summed over users, ``per_user`` (M, n_k, 5) float64 = hit, mrr, recall,
    precision, ndcg or None.  No autograd; current stream."""
    cutoffs = [int(k) for k in cutoffs]
    if len(cutoffs) > _lib.H.RH_RANK_MAX_CUTOFFS:  # the newer list metrics answer this with "no HIP kernel"; here it stays a ValueError
        raise ValueError(f"torch_rechub_amd: rank_metrics takes 1 to {_lib.H.RH_RANK_MAX_CUTOFFS} cut-offs, got {cutoffs}")
    pred_ids, ld, M, K, cuts, n_k = _list_inputs("rank_metrics", pred_ids, cutoffs)
    if isinstance(truth, (tuple, list)) and len(truth) == 2 and all(torch.is_tensor(t) for t in truth):
        off, ids = truth
        require_hip(off, ids)
        if off.dtype != torch.int64 or ids.dtype != torch.int64 or off.dim() != 1 or ids.dim() != 1:
            raise ValueError("torch_rechub_amd: rank_metrics takes int64 1-D truth offsets and ids")
        off, ids = off.contiguous(), ids.contiguous()
    else:
        if len(truth) != M:
            raise ValueError(f"torch_rechub_amd: rank_metrics: {len(truth)} truth lists for {M} users")
        off, ids = pack_truth(truth, pred_ids.device)
    if off.numel() != M + 1:
        raise ValueError(f"torch_rechub_amd: rank_metrics: {off.numel()} truth offsets for {M} users (M + 1 expected)")
    dev = pred_ids.device
    tables = _rank_tables.get((K, dev))
    if tables is None:
        tables = _rank_tables[(K, dev)] = tuple(torch.from_numpy(t).to(dev) for t in rank_gain_tables(K))
    partial = torch.empty((rank_metrics_plan(M)[3],), dtype=torch.float64, device=dev)
    hits = torch.empty((n_k,), dtype=torch.int64, device=dev)
    gts = torch.empty((1,), dtype=torch.int64, device=dev)
    sums = torch.empty((n_k, 4), dtype=torch.float64, device=dev)
    users = torch.empty((M, n_k, 5), dtype=torch.float64, device=dev) if per_user else None
    _lib.call("rh_rank_metrics", _p(pred_ids), ld, M, K, _p(off), _p(ids), int(ids.numel()),
              ctypes.c_void_p(ctypes.addressof(cuts)), n_k, _p(tables[0]), _p(tables[1]), _p(partial), _p(hits), _p(gts),
              _p(sums), _p(users), _stream())
    return {"hits": hits, "gts": gts, "sums": sums, "per_user": users}


# beyond-accuracy metrics (rh_ild, rh_coverage, rh_novelty): intra-list diversity, catalogue coverage, novelty
_POP_DTYPES = {torch.float32: 0, torch.float64: 1}


def ild_plan(M):
    """(users_per_workgroup, max_grid, partial_doubles) of rh_ild over M users."""
    return _lib.query("rh_ild_plan", int(M), out=_PLAN_OUT)


def novelty_plan(M):
    """(users_per_workgroup, max_grid, partial_doubles) of rh_novelty over M users."""
    return _lib.query("rh_novelty_plan", int(M), out=_PLAN_OUT)


def coverage_plan(n_slots):
    """(rows_per_workgroup, max_grid, workspace_bytes) of rh_coverage over n_slots item slots: the rows a workgroup marks
    per trip, the grid cap of both passes (the counting pass takes 256 slots per workgroup and trip) and the scratch size."""
    return _lib.query("rh_coverage_plan", int(n_slots), out=_PLAN_OUT)


def _list_inputs(what, pred_ids, cutoffs, *more):
    """The guards the list metrics share, before anything is allocated or launched.  -> (pred_ids readable in place, ld, M,
    K, the cut-offs as a C array, n_k)."""
    require_hip(pred_ids, *more)
    if pred_ids.dim() != 2 or pred_ids.dtype != torch.int64:
        raise ValueError(f"torch_rechub_amd: {what} takes an (M, K) int64 id tensor")
    M, K = (int(v) for v in pred_ids.shape)
    if M == 0 or K == 0:
        raise ValueError(f"torch_rechub_amd: {what} of an empty input")
    if K > _lib.H.RH_RANK_MAX_K:
        from ..models.matching._listwise import no_kernel
        raise no_kernel(f"{what} over K={K} recommendations (1 <= K <= {_lib.H.RH_RANK_MAX_K})")
    cutoffs = [int(k) for k in cutoffs]
    if not cutoffs or any(not 1 <= k <= K for k in cutoffs):
        raise ValueError(f"torch_rechub_amd: {what} takes cut-offs within [1, K={K}], got {cutoffs}")
    if len(cutoffs) > _lib.H.RH_RANK_MAX_CUTOFFS:
        from ..models.matching._listwise import no_kernel
        raise no_kernel(f"{what} at {len(cutoffs)} cut-offs (1 to {_lib.H.RH_RANK_MAX_CUTOFFS})")
    pred_ids = pred_ids.detach()
    if pred_ids.stride(1) != 1 or (M > 1 and pred_ids.stride(0) < K):
        pred_ids = pred_ids.contiguous()
    ld = int(pred_ids.stride(0)) if M > 1 else K
    return pred_ids, ld, M, K, (ctypes.c_int * len(cutoffs))(*cutoffs), len(cutoffs)


def ild(pred_ids, table, cutoffs, per_user=False):
    """The raw sums behind intra-list diversity.  ``pred_ids`` (M, K) int64 (what ``topk_items`` returns; a strided
    ``ids[:, :k]`` view is read in place; an id below 0 is an absent position), ``table`` (V, D) float32, read in place
    under a row stride, ``cutoffs`` at most 8 ints in [1, K].  Per user and cut-off k the mean over the pairs i < j of
    1 - cos(e_i, e_j) among the first k entries with 0 <= id < V (norms clamped at 1e-10, in double), for users with at
    least two such entries -- the reference run on the rows with the negative entries removed.  -> dict: ``sums`` (n_k,)
    float64 over the users, ``counts`` (n_k,) int64 = the users that contributed, ``per_user`` (M, n_k) float64 (nan where
    the user was left out) or None.  O(k D) per user; no (M, K, D) gather.  No autograd; current stream."""
    pred_ids, ld, M, K, cuts, n_k = _list_inputs("ild", pred_ids, cutoffs, table)
    if table.dim() != 2 or table.dtype != torch.float32:
        raise ValueError("torch_rechub_amd: ild takes a (V, D) float32 embedding table")
    V, D = (int(v) for v in table.shape)
    if V == 0 or D == 0:
        raise ValueError("torch_rechub_amd: ild of an empty embedding table")
    if D > _lib.H.RH_ILD_MAX_D:
        from ..models.matching._listwise import no_kernel
        raise no_kernel(f"intra-list diversity over embeddings of width {D} (1 <= D <= {_lib.H.RH_ILD_MAX_D})")
    table = table.detach()
    if table.stride(1) != 1 or (V > 1 and table.stride(0) < D):
        table = table.contiguous()
    lt = int(table.stride(0)) if V > 1 else D
    dev = pred_ids.device
    partial = torch.empty((ild_plan(M)[2],), dtype=torch.float64, device=dev)
    sums = torch.empty((n_k,), dtype=torch.float64, device=dev)
    counts = torch.empty((n_k,), dtype=torch.int64, device=dev)
    users = torch.empty((M, n_k), dtype=torch.float64, device=dev) if per_user else None
    _lib.call("rh_ild", _p(pred_ids), ld, M, K, _p(table), lt, V, D, ctypes.c_void_p(ctypes.addressof(cuts)), n_k,
              _p(partial), _p(sums), _p(counts), _p(users), _stream())
    return {"sums": sums, "counts": counts, "per_user": users}


def coverage(pred_ids, n_slots, cutoffs):
    """The distinct ids in [0, n_slots) among ``pred_ids[:, :k]`` for every cut-off, in one pass: -> dict ``counts`` (n_k,)
    int64.  Ids outside [0, n_slots) -- the -1 padding among them -- are ignored.  Exact.  No autograd; current stream."""
    pred_ids, ld, M, K, cuts, n_k = _list_inputs("coverage", pred_ids, cutoffs)
    n_slots = int(n_slots)
    if n_slots < 1:
        raise ValueError(f"torch_rechub_amd: coverage takes n_slots >= 1, got {n_slots}")
    if n_slots >= 2 ** 31:
        from ..models.matching._listwise import no_kernel
        raise no_kernel(f"coverage over {n_slots} item slots (fewer than 2**31)")
    dev = pred_ids.device
    first = torch.empty((coverage_plan(n_slots)[2] // 4,), dtype=torch.int32, device=dev)
    counts = torch.empty((n_k,), dtype=torch.int64, device=dev)
    _lib.call("rh_coverage", _p(pred_ids), ld, M, K, n_slots, ctypes.c_void_p(ctypes.addressof(cuts)), n_k, _p(first),
              _p(counts), _stream())
    return {"counts": counts}


def novelty(pred_ids, popularity, cutoffs, per_user=False):
    """The raw sums behind novelty.  ``popularity`` (V,) float32 or float64, indexed by item id.  An id >= 0 adds
    -log2(max(p, 1e-10)) in double, p = 1e-10 for an id >= V; an id below 0 is an absent position.  Per user and cut-off k
    the mean over the present positions among the first k; a user with none is left out -- the reference run on the rows
    with the negative entries removed.  -> dict like ``ild``'s.  No autograd; current stream."""
    pred_ids, ld, M, K, cuts, n_k = _list_inputs("novelty", pred_ids, cutoffs, popularity)
    if popularity.dim() != 1 or popularity.dtype not in _POP_DTYPES:
        raise ValueError("torch_rechub_amd: novelty takes a 1-D float32 or float64 popularity tensor indexed by item id")
    V = int(popularity.numel())
    if V == 0:
        raise ValueError("torch_rechub_amd: novelty of an empty popularity tensor")
    popularity = popularity.detach().contiguous()
    dev = pred_ids.device
    partial = torch.empty((novelty_plan(M)[2],), dtype=torch.float64, device=dev)
    sums = torch.empty((n_k,), dtype=torch.float64, device=dev)
    counts = torch.empty((n_k,), dtype=torch.int64, device=dev)
    users = torch.empty((M, n_k), dtype=torch.float64, device=dev) if per_user else None
    _lib.call("rh_novelty", _p(pred_ids), ld, M, K, _p(popularity), _POP_DTYPES[popularity.dtype], V,
              ctypes.c_void_p(ctypes.addressof(cuts)), n_k, _p(partial), _p(sums), _p(counts), _p(users), _stream())
    return {"sums": sums, "counts": counts, "per_user": users}
