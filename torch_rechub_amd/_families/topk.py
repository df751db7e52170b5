"""Exact top-K item retrieval (csrc/topk.hip; fp16 / bf16 tables: csrc/topk_half.hip)."""
import ctypes

import torch

from .. import _lib
from .._opcore import _NULL, _p, _stream, require_hip


def topk_supported(D, K, S=0):
    """Whether csrc/topk.hip takes width D, K results and S exclusions per query (D <= RH_TOPK_MAX_D, K <= RH_TOPK_MAX_K,
    S <= RH_TOPK_MAX_S)."""
    return bool(_lib.query("rh_topk_supported", int(D), int(K), int(S)))


def topk_plan(M, V, K):
    """(nsplit, workspace_bytes): the default number of item ranges for M queries over V items and the size of the
    partial lists for it (8 M nsplit K bytes)."""
    return _lib.query("rh_topk_plan", int(M), int(V), int(K), out=(ctypes.c_int, ctypes.c_int64))


HALF_TABLES = {torch.float16: 0, torch.bfloat16: 1}  # the half table types and the kernels' is_bf16 for them


def _table_dtype(what, tname, table):
    """Refuses a table of another type than the three the scans read (a host-side check, made before anything else)."""
    if table.dtype != torch.float32 and table.dtype not in HALF_TABLES:
        raise ValueError(f"torch_rechub_amd: {what} takes a float32, float16 or bfloat16 {tname}, got {table.dtype}")


def _scan_inputs(what, tname, q, table, k, bias, exclude, refuse):
    """What ``topk_items`` and ``ivf_scan`` check and prepare alike: the table (V, D; ``tname`` in the messages) float32,
    float16 or bfloat16 and contiguous, q (M, D) float32 or of the table's type (handed on as float32, which holds every
    value of either half type; the half kernels round it back), bias (V,) float32, exclude (M, S).  ``refuse(M, D, V, k, S)`` makes the
    caller's own checks and raises where there is no kernel, before anything is allocated.  Returns q with unit column
    stride and its row stride, bias and exclude as the kernels read them, S and the empty (ids, scores) (M, k)."""
    if q.dim() != 2 or table.dim() != 2 or q.shape[1] != table.shape[1]:
        raise ValueError(f"{what}: q (M, D) and {tname} (V, D) expected")
    _table_dtype(what, tname, table)
    if q.dtype not in (torch.float32, table.dtype) or (bias is not None and bias.dtype != torch.float32):
        raise ValueError(f"torch_rechub_amd: {what} takes float32 tensors (q may have the {tname}'s type)")
    if not table.is_contiguous():
        raise ValueError(f"{what}: the table must be contiguous")
    M, D = (int(v) for v in q.shape)
    V, k = int(table.shape[0]), int(k)
    if exclude is not None and (exclude.dim() != 2 or exclude.shape[0] != M):
        raise ValueError(f"{what}: exclude (M, S) expected")
    S = 0 if exclude is None else int(exclude.shape[1])
    if bias is not None and tuple(bias.shape) != (V,):
        raise ValueError(f"{what}: bias (V,) expected")
    refuse(M, D, V, k, S)
    q = q.detach().float()
    if M > 0 and (q.stride(1) != 1 or q.stride(0) < D):
        q = q.contiguous()
    ldq = int(q.stride(0)) if M > 1 else D
    if bias is not None:
        bias = bias.detach().contiguous()
    if S > 0:
        exclude = exclude.to(torch.int64).contiguous()
    ids = torch.empty((M, k), dtype=torch.int64, device=q.device)
    scores = torch.empty((M, k), dtype=torch.float32, device=q.device)
    return q, ldq, bias, exclude, S, ids, scores


def topk_items(q, table, k, bias=None, exclude=None, invalid=None, nsplit=None):
    """(ids (M, k) int64, scores (M, k) float32): the k best items of ``table`` (V, D) for every row of ``q`` (M, D) by
    q_i . x_j (+ bias[j]), best first, exact ties to the lower id; the (M, V) scores are never formed.  ``exclude`` (M, S)
    int64: ids that may not be returned to query i (entries outside [0, V) are ignored: pad with -1, or pass a 0-padded
    history to drop id 0 with it); ``invalid``: ids dropped for every query.  With fewer than k candidates the tail is
    id -1, score -inf.  ``nsplit`` forces the number of item ranges (the result does not depend on it).  A float16 or
    bfloat16 ``table`` (half the bytes per item) scores sum_k T(q_ik) x_jk: q is rounded to the table's type T as
    ``q.to(T)`` does, the products are exact and the sum is float32.  No autograd; runs on the current stream."""
    if invalid is not None and not torch.is_tensor(invalid):
        invalid = torch.as_tensor(list(invalid), dtype=torch.int64, device=q.device)
    _table_dtype("topk_items", "table", table)
    require_hip(q, table, bias, exclude, invalid)

    def refuse(M, D, V, k, S):
        if V < 1 or not topk_supported(D, k, S):
            from ..models.matching._listwise import no_kernel
            raise no_kernel(f"top-k retrieval at D={D}, k={k}, {S} exclusions per query, V={V} "
                            f"(1 <= D <= {_lib.H.RH_TOPK_MAX_D}, 1 <= k <= {_lib.H.RH_TOPK_MAX_K}, S <= {_lib.H.RH_TOPK_MAX_S}, V >= 1)")

    q, ldq, bias, exclude, S, ids, scores = _scan_inputs("topk_items", "table", q, table, k, bias, exclude, refuse)
    (M, D), V, k = q.shape, int(table.shape[0]), int(k)
    n_inv = 0
    if invalid is not None:
        invalid = invalid.to(torch.int64).reshape(-1).contiguous()
        n_inv = int(invalid.numel())
    if nsplit is None:
        nsplit, _ = topk_plan(M, V, k)
    nsplit = int(nsplit)
    if not 1 <= nsplit <= min(V, _lib.H.RH_TOPK_MAX_SPLIT):
        raise ValueError(f"topk_items: nsplit={nsplit} outside [1, min(V, {_lib.H.RH_TOPK_MAX_SPLIT})]")
    if M == 0:
        return ids, scores
    work = torch.empty((8 * M * nsplit * k,), dtype=torch.uint8, device=q.device)
    tail = (_p(bias), _p(exclude) if S > 0 else _NULL, S, _p(invalid) if n_inv > 0 else _NULL, n_inv, M, D, V, k, nsplit,
            _p(work), _p(ids), _p(scores), _stream())
    if table.dtype == torch.float32:
        _lib.call("rh_topk_fwd", _p(q), ldq, _p(table.detach()), *tail)
    else:
        _lib.call("rh_topk_half_fwd", _p(q), ldq, _p(table.detach()), HALF_TABLES[table.dtype], *tail)
    return ids, scores
