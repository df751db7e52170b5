"""Exact top-K item retrieval (csrc/topk.hip; fp16 / bf16 tables: csrc/topk_half.hip; int8 tables: csrc/topk_q8.hip;
(M, I, D) multi-interest queries, one list per user: csrc/topk_multi.hip)."""
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
    return _scan_prepare(what, q, table, k, bias, exclude, refuse)


def _scan_prepare(what, q, table, k, bias, exclude, refuse):
    """The part of ``_scan_inputs`` that does not ask for the table's type (the int8 entries check theirs themselves)."""
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


def _as_ids(invalid, device):
    """``invalid`` as the kernels read it, (n_inv,) int64 contiguous, or None; the caller keeps it until it has launched."""
    if invalid is None:
        return None
    if not torch.is_tensor(invalid):
        invalid = torch.as_tensor(list(invalid), dtype=torch.int64, device=device)
    return invalid.to(torch.int64).reshape(-1).contiguous()


def _flat_refuse(M, D, V, k, S):
    if V < 1 or not topk_supported(D, k, S):
        from ..models.matching._listwise import no_kernel
        raise no_kernel(f"top-k retrieval at D={D}, k={k}, {S} exclusions per query, V={V} "
                        f"(1 <= D <= {_lib.H.RH_TOPK_MAX_D}, 1 <= k <= {_lib.H.RH_TOPK_MAX_K}, S <= {_lib.H.RH_TOPK_MAX_S}, V >= 1)")


def _flat_tail(what, M, D, V, k, bias, exclude, S, invalid, nsplit, ids, scores):
    """(tail, work): the arguments every flat entry point takes after its table, from ``bias`` on (nsplit checked or
    planned), and the tensor of the partial lists, which the caller keeps until it has launched -- the tail holds only
    its address; (None, None) for M = 0."""
    n_inv = 0 if invalid is None else int(invalid.numel())
    if nsplit is None:
        nsplit, _ = topk_plan(M, V, k)
    nsplit = int(nsplit)
    if not 1 <= nsplit <= min(V, _lib.H.RH_TOPK_MAX_SPLIT):
        raise ValueError(f"{what}: nsplit={nsplit} outside [1, min(V, {_lib.H.RH_TOPK_MAX_SPLIT})]")
    if M == 0:
        return None, None
    work = torch.empty((8 * M * nsplit * k,), dtype=torch.uint8, device=ids.device)
    return (_p(bias), _p(exclude) if S > 0 else _NULL, S, _p(invalid) if n_inv > 0 else _NULL, n_inv, M, D, V, k, nsplit,
            _p(work), _p(ids), _p(scores), _stream()), work


def topk_items(q, table, k, bias=None, exclude=None, invalid=None, nsplit=None):
    """(ids (M, k) int64, scores (M, k) float32): the k best items of ``table`` (V, D) for every row of ``q`` (M, D) by
    q_i . x_j (+ bias[j]), best first, exact ties to the lower id; the (M, V) scores are never formed.  ``exclude`` (M, S)
    int64: ids that may not be returned to query i (entries outside [0, V) are ignored: pad with -1, or pass a 0-padded
    history to drop id 0 with it); ``invalid``: ids dropped for every query.  With fewer than k candidates the tail is
    id -1, score -inf.  ``nsplit`` forces the number of item ranges (the result does not depend on it).  A float16 or
    bfloat16 ``table`` (half the bytes per item) scores sum_k T(q_ik) x_jk: q is rounded to the table's type T as
    ``q.to(T)`` does, the products are exact and the sum is float32.  No autograd; runs on the current stream."""
    invalid = _as_ids(invalid, q.device)
    _table_dtype("topk_items", "table", table)
    require_hip(q, table, bias, exclude, invalid)
    q, ldq, bias, exclude, S, ids, scores = _scan_inputs("topk_items", "table", q, table, k, bias, exclude, _flat_refuse)
    (M, D), V, k = q.shape, int(table.shape[0]), int(k)
    tail, work = _flat_tail("topk_items", M, D, V, k, bias, exclude, S, invalid, nsplit, ids, scores)
    if tail is None:
        return ids, scores
    if table.dtype == torch.float32:
        _lib.call("rh_topk_fwd", _p(q), ldq, _p(table.detach()), *tail)
    else:
        _lib.call("rh_topk_half_fwd", _p(q), ldq, _p(table.detach()), HALF_TABLES[table.dtype], *tail)
    return ids, scores


def topk_multi_supported(D, K, S=0, I=1):
    """Whether csrc/topk_multi.hip takes I interests per user at width D, K results and S exclusions per user
    (``topk_supported`` and 1 <= I <= RH_LISTWISE_MAX_I)."""
    return bool(_lib.query("rh_topk_multi_supported", int(D), int(K), int(S), int(I)))


def topk_multi_plan(M, I, V, K):
    """(nsplit, workspace_bytes) for M users of I interests: ``topk_plan``'s rule over the users' row tiles; the partial
    lists are per user (8 M nsplit K bytes)."""
    return _lib.query("rh_topk_multi_plan", int(M), int(I), int(V), int(K), out=(ctypes.c_int, ctypes.c_int64))


def topk_items_multi(q, table, k, qbias=None, bias=None, exclude=None, invalid=None, nsplit=None):
    """(ids (M, k) int64, scores (M, k) float32): for ``q`` (M, I, D), one vector per interest of a user, the k best items
    of ``table`` (V, D) for every USER by max_i (q[u, i] . x_j + qbias[u, i]) + bias[j] -- the merged, de-duplicated union
    of the I per-interest ``topk_items`` lists, formed in one scan with one list per user (csrc/topk_multi.hip).  ``qbias``
    (M, I) float32: -inf marks an absent interest; a user without any interest gets the (-1, -inf) tail.  ``exclude`` (M, S)
    is per user.  Order, ties (to the lower id), ``invalid``, the tail, ``nsplit`` and a float16 / bfloat16 ``table`` are
    ``topk_items``'; with I = 1 and no ``qbias`` the result is ``topk_items(q[:, 0])`` bit for bit.  An int8 table is not
    built.  No autograd; runs on the current stream."""
    what = "topk_items_multi"
    invalid = _as_ids(invalid, q.device)
    if table.dtype == torch.int8:
        raise ValueError(f"torch_rechub_amd: {what} over an int8 (SQ8) table is not built; use a float32, float16 or "
                         "bfloat16 table")
    _table_dtype(what, "table", table)
    if q.dim() != 3 or table.dim() != 2 or q.shape[2] != table.shape[1]:
        raise ValueError(f"{what}: q (M, I, D) and table (V, D) expected")
    if q.dtype not in (torch.float32, table.dtype) or (bias is not None and bias.dtype != torch.float32):
        raise ValueError(f"torch_rechub_amd: {what} takes float32 tensors (q may have the table's type)")
    if not table.is_contiguous():
        raise ValueError(f"{what}: the table must be contiguous")
    (M, I, D), V, k = (int(v) for v in q.shape), int(table.shape[0]), int(k)
    if qbias is not None and (tuple(qbias.shape) != (M, I) or qbias.dtype != torch.float32):
        raise ValueError(f"{what}: qbias (M, I) float32 expected")
    if exclude is not None and (exclude.dim() != 2 or exclude.shape[0] != M):
        raise ValueError(f"{what}: exclude (M, S) expected, one row per user")
    S = 0 if exclude is None else int(exclude.shape[1])
    if bias is not None and tuple(bias.shape) != (V,):
        raise ValueError(f"{what}: bias (V,) expected")
    if V < 1 or not topk_multi_supported(D, k, S, I):
        from ..models.matching._listwise import no_kernel
        raise no_kernel(f"multi-interest top-k retrieval at I={I}, D={D}, k={k}, {S} exclusions per user, V={V} "
                        f"(1 <= I <= {_lib.H.RH_LISTWISE_MAX_I}, 1 <= D <= {_lib.H.RH_TOPK_MAX_D}, 1 <= k <= "
                        f"{_lib.H.RH_TOPK_MAX_K}, S <= {_lib.H.RH_TOPK_MAX_S}, V >= 1)")
    require_hip(q, table, qbias, bias, exclude, invalid)
    q = q.detach().float()
    # one stride ldq from an interest row to the next, over users and interests alike; anything else is copied
    ldq = int(q.stride(1)) if I > 1 else (int(q.stride(0)) if M > 1 else D)
    if M > 0 and (q.stride(2) != 1 or ldq < D or (I > 1 and M > 1 and q.stride(0) != I * ldq)):
        q, ldq = q.contiguous(), D
    qbias = None if qbias is None else qbias.detach().contiguous()
    bias = None if bias is None else bias.detach().contiguous()
    if S > 0:
        exclude = exclude.to(torch.int64).contiguous()
    ids = torch.empty((M, k), dtype=torch.int64, device=q.device)
    scores = torch.empty((M, k), dtype=torch.float32, device=q.device)
    if nsplit is None:
        nsplit, _ = topk_multi_plan(M, I, V, k)
    # work, invalid and qbias stay alive in this frame until the launch: the argument tuple holds only their addresses
    tail, work = _flat_tail(what, M, D, V, k, bias, exclude, S, invalid, nsplit, ids, scores)
    if tail is None:
        return ids, scores
    if table.dtype == torch.float32:
        _lib.call("rh_topk_multi_fwd", _p(q), ldq, I, _p(qbias), _p(table.detach()), *tail)
    else:
        _lib.call("rh_topk_multi_half_fwd", _p(q), ldq, I, _p(qbias), _p(table.detach()), HALF_TABLES[table.dtype], *tail)
    return ids, scores


def _q8_table(what, cname, codes, scale):
    """Refuses what is not a quantised table (host-side, made before anything else): ``codes`` (V, D) int8 and ``scale``
    (V,) float32, as ``quantize_rows_int8`` returns them."""
    if codes.dtype != torch.int8 or codes.dim() != 2:
        raise ValueError(f"torch_rechub_amd: {what} takes (V, D) int8 {cname}, got {codes.dtype} {tuple(codes.shape)}")
    if scale.dtype != torch.float32 or tuple(scale.shape) != (codes.shape[0],):
        raise ValueError(f"torch_rechub_amd: {what} takes one float32 scale per row of {cname} (V,), got {scale.dtype} "
                         f"{tuple(scale.shape)}")


def _q8_scan_inputs(what, cname, q, codes, k, bias, exclude, refuse):
    """``_scan_inputs`` for a quantised table: q (M, D) float32 and bias (V,) float32 only."""
    if q.dim() != 2 or q.shape[1] != codes.shape[1]:
        raise ValueError(f"{what}: q (M, D) and {cname} (V, D) expected")
    if q.dtype != torch.float32 or (bias is not None and bias.dtype != torch.float32):
        raise ValueError(f"torch_rechub_amd: {what} takes float32 q and bias")
    return _scan_prepare(what, q, codes, k, bias, exclude, refuse)


def _quantize_rows(x, ldc):
    """``quantize_rows_int8`` of x (M, D) float32 with unit column stride into codes (M, ldc), zero from column D on."""
    M, D = (int(v) for v in x.shape)
    codes = torch.empty((M, ldc), dtype=torch.int8, device=x.device)
    scale = torch.empty((M,), dtype=torch.float32, device=x.device)
    if M > 0:
        _lib.call("rh_quantize_rows_q8", _p(x), int(x.stride(0)) if M > 1 else D, M, D, _p(codes), ldc, _p(scale), _stream())
    return codes, scale


def quantize_rows_int8(x):
    """(codes (M, D) int8, scale (M,) float32) of ``x`` (M, D) float32, one scale per row: with m = max_k |x_k|,
    scale = m / 127 and code_k = clamp(rint(x_k / scale), -127, 127), rounding to nearest even, both divisions correctly
    rounded float32 divisions (numpy float32 gives the same bits); a zero row has scale 1 and codes 0.  x_k is about
    scale * code_k, off by at most scale / 2.  The one rule of the int8 index: it builds the table and quantises every
    batch of queries.  NaN and inf are out of scope.  No autograd; runs on the current stream."""
    if x.dim() != 2 or x.shape[1] < 1 or x.dtype != torch.float32:
        raise ValueError(f"torch_rechub_amd: quantize_rows_int8 takes a float32 (M, D) tensor with D >= 1, got {x.dtype} "
                         f"{tuple(x.shape)}")
    require_hip(x)
    x = x.detach()
    if x.shape[0] > 0 and (x.stride(1) != 1 or x.stride(0) < x.shape[1]):
        x = x.contiguous()
    return _quantize_rows(x, int(x.shape[1]))


def topk_items_int8(q, codes, scale, k, bias=None, exclude=None, invalid=None, nsplit=None):
    """``topk_items`` over a quantised table (csrc/topk_q8.hip): ``codes`` (V, D) int8 contiguous and ``scale`` (V,)
    float32 as ``quantize_rows_int8`` makes them, a quarter of the float32 bytes per item.  ``q`` (M, D) float32 is
    quantised per call by the same rule (qc, qs), and
      score[i][j] = ((float32)(sum_k qc_ik xc_jk) * qs_i) * scale_j (+ bias_j):
    the integer sum is exact, the two multiplications and the addition are single float32 operations in that order, so
    the answer is defined bit for bit and does not depend on ``nsplit``.  Order, ties, ``exclude``, ``invalid`` and the
    (-1, -inf) tail are ``topk_items``'.  No autograd; runs on the current stream."""
    invalid = _as_ids(invalid, q.device)
    _q8_table("topk_items_int8", "codes", codes, scale)
    require_hip(q, codes, scale, bias, exclude, invalid)
    q, _, bias, exclude, S, ids, scores = _q8_scan_inputs("topk_items_int8", "codes", q, codes, k, bias, exclude, _flat_refuse)
    (M, D), V, k = q.shape, int(codes.shape[0]), int(k)
    tail, work = _flat_tail("topk_items_int8", M, D, V, k, bias, exclude, S, invalid, nsplit, ids, scores)
    if tail is None:
        return ids, scores
    ldqc = (D + 15) // 16 * 16
    qc, qs = _quantize_rows(q, ldqc)
    _lib.call("rh_topk_q8_fwd", _p(qc), ldqc, _p(qs), _p(codes.detach()), _p(scale.detach().contiguous()), *tail)
    return ids, scores
