"""Inverted-file index: the list scan and the k-means update (csrc/ivf.hip; int8 tables: csrc/topk_q8.hip)."""
import ctypes

import torch

from .. import _lib
from .._opcore import _NULL, _p, _stream, require_hip
from .topk import HALF_TABLES, _q8_scan_inputs, _q8_table, _quantize_rows, _scan_inputs, _table_dtype


def ivf_supported(D, K, S=0, nprobe=1):
    """Whether csrc/ivf.hip takes width D, K results, S exclusions per query and nprobe lists per query (the limits of
    ops.topk_supported and nprobe <= RH_IVF_MAX_NPROBE)."""
    return bool(_lib.query("rh_ivf_supported", int(D), int(K), int(S), int(nprobe)))


def ivf_plan(M, nlists, nprobe, K):
    """(rows_per_tile, grid, workspace_bytes) of ``ivf_scan``: the (query, slot) pairs one workgroup takes, the fixed grid
    bound ceil(M nprobe / rows_per_tile) + nlists + 1, and 8 M nprobe K bytes of partial lists + 4 M nprobe of pair
    indices + 8 (nlists + 2) of group and tile offsets."""
    return _lib.query("rh_ivf_plan", int(M), int(nlists), int(nprobe), int(K),
                      out=(ctypes.c_int, ctypes.c_int64, ctypes.c_int64))


def ivf_scan(q, table_sorted, row_ids, list_offsets, probe, k, bias=None, exclude=None, dtype=torch.float32):
    """(ids (M, k) int64, scores (M, k) float32): the k best rows for every row of ``q`` (M, D) by q_i . x_j (+ bias[j])
    among the lists it probes, best first, exact ties to the lower id; ``topk_items`` restricted to a union of lists.
    ``table_sorted`` (V, D) holds the table's rows grouped by list, ``bias`` (V,) alike, ``row_ids`` (V,) int32 the original
    id of every grouped row (ascending inside each list: a stable sort by list gives that), ``list_offsets`` (nlists + 1,)
    int32 the lists' offsets.  ``probe`` (M, nprobe) int32: the lists of each query, distinct per row; an entry outside
    [0, nlists) (-1) is no list.  ``exclude`` (M, S) int64: original ids that may not be returned to query i (anything
    else is padding).  The returned ids are original ids; with fewer than k candidates the tail is id -1, score -inf.
    With every list probed the result is ``topk_items``' on the un-grouped table, bit for bit.  ``dtype``: the type
    ``table_sorted`` is stored in, float32 unless the caller names torch.float16 or torch.bfloat16 (with the score
    ``topk_items`` gives such a table); a table of any other type than the one named is refused.  The pairs are grouped by
    list with a stable ``torch.sort``; nothing synchronises with the host.  No autograd; runs on the current stream."""
    _table_dtype("ivf_scan", "table_sorted", table_sorted)
    if table_sorted.dtype != dtype:
        raise ValueError(f"torch_rechub_amd: ivf_scan was told dtype={dtype} and given a {table_sorted.dtype} table_sorted")
    require_hip(q, table_sorted, row_ids, list_offsets, probe, bias, exclude)

    def launch(q, ldq, table, tail):
        if table.dtype == torch.float32:
            _lib.call("rh_ivf_scan", _p(q), ldq, _p(table), *tail)
        else:
            _lib.call("rh_ivf_scan_half", _p(q), ldq, _p(table), HALF_TABLES[table.dtype], *tail)

    return _list_scan("ivf_scan", "table_sorted", _scan_inputs, launch, q, table_sorted, row_ids, list_offsets, probe, k, bias,
                      exclude)


def ivf_scan_int8(q, codes_sorted, scale_sorted, row_ids, list_offsets, probe, k, bias=None, exclude=None):
    """``ivf_scan`` over a quantised table (csrc/topk_q8.hip): ``codes_sorted`` (V, D) int8 and ``scale_sorted`` (V,)
    float32, the rows of ``ops.quantize_rows_int8`` grouped by list, with the score ``ops.topk_items_int8`` gives (``q``
    float32, quantised per call by the same rule).  With every list probed the result is ``topk_items_int8``'s on the
    un-grouped table, bit for bit.  No autograd; runs on the current stream."""
    _q8_table("ivf_scan_int8", "codes_sorted", codes_sorted, scale_sorted)
    require_hip(q, codes_sorted, scale_sorted, row_ids, list_offsets, probe, bias, exclude)

    def launch(q, ldq, codes, tail):
        ldqc = (int(q.shape[1]) + 15) // 16 * 16
        qc, qs = _quantize_rows(q, ldqc)
        _lib.call("rh_ivf_scan_q8", _p(qc), ldqc, _p(qs), _p(codes), _p(scale_sorted.detach().contiguous()), *tail)

    return _list_scan("ivf_scan_int8", "codes_sorted", _q8_scan_inputs, launch, q, codes_sorted, row_ids, list_offsets, probe,
                      k, bias, exclude)


def _list_scan(what, tname, inputs, launch, q, table_sorted, row_ids, list_offsets, probe, k, bias, exclude):
    """What the list-scan entry points share: the checks (``inputs`` = the ``_scan_inputs`` of the table's kind), the
    pairs grouped by list, the partials; ``launch(q, ldq, table, tail)`` calls the kernel."""
    def refuse(M, D, V, k, S):
        if row_ids.dtype != torch.int32 or list_offsets.dtype != torch.int32 or probe.dtype != torch.int32:
            raise ValueError(f"{what}: row_ids, list_offsets and probe are int32 tensors")
        if tuple(row_ids.shape) != (V,) or list_offsets.dim() != 1 or list_offsets.shape[0] < 2:
            raise ValueError(f"{what}: row_ids (V,) and list_offsets (nlists + 1,) expected")
        if probe.dim() != 2 or probe.shape[0] != M:
            raise ValueError(f"{what}: probe (M, nprobe) expected")
        nlists, nprobe = int(list_offsets.shape[0]) - 1, int(probe.shape[1])
        if V < 1 or M * nprobe >= 2 ** 31 - 64 * (nlists + 2) or not ivf_supported(D, k, S, nprobe):
            from ..models.matching._listwise import no_kernel
            raise no_kernel(f"the inverted-file scan at D={D}, k={k}, {S} exclusions per query, nprobe={nprobe}, V={V} "
                            f"(1 <= D <= {_lib.H.RH_TOPK_MAX_D}, 1 <= k <= {_lib.H.RH_TOPK_MAX_K}, S <= {_lib.H.RH_TOPK_MAX_S}, "
                            f"1 <= nprobe <= {_lib.H.RH_IVF_MAX_NPROBE}, V >= 1, M nprobe < 2^31)")

    q, ldq, bias, exclude, S, ids, scores = inputs(what, tname, q, table_sorted, k, bias, exclude, refuse)
    (M, D), V, k, dev = q.shape, int(table_sorted.shape[0]), int(k), q.device
    nlists, nprobe = int(list_offsets.shape[0]) - 1, int(probe.shape[1])
    if M == 0:
        return ids, scores
    table_sorted, row_ids, list_offsets = table_sorted.detach(), row_ids.contiguous(), list_offsets.contiguous()
    rb = ivf_plan(M, nlists, nprobe, k)[0]
    # the pairs grouped by list: group 0 = no list, group l + 1 = list l (a stable sort: reproducible pair order)
    key = torch.where((probe >= 0) & (probe < nlists), probe + 1, torch.zeros_like(probe)).reshape(-1)
    key, order = torch.sort(key, stable=True)
    pair = order.to(torch.int32)
    del order
    bounds = torch.arange(nlists + 2, dtype=torch.int32, device=dev)
    pair_off = torch.searchsorted(key, bounds, out_int32=True)
    del key, bounds
    tile_off = torch.zeros_like(pair_off)
    tile_off[1:] = torch.cumsum((pair_off[1:] - pair_off[:-1] + (rb - 1)) // rb, 0)
    part = torch.empty((8 * M * nprobe * k,), dtype=torch.uint8, device=dev)
    launch(q, ldq, table_sorted, (_p(bias), _p(row_ids), _p(list_offsets), nlists, _p(pair), _p(pair_off), _p(tile_off),
                                  _p(exclude) if S > 0 else _NULL, S, M, D, V, k, nprobe, _p(part), _p(ids), _p(scores),
                                  _stream()))
    return ids, scores


def ivf_list_mean(x_sorted, list_offsets, previous):
    """(nlists, D) float32: row l = the mean of the rows [list_offsets[l], list_offsets[l + 1]) of ``x_sorted`` (V, D),
    summed in a fixed order (two runs give the same bits) and divided once; an empty list keeps ``previous[l]``.  The
    update step of k-means over rows grouped by list.  No autograd; runs on the current stream."""
    require_hip(x_sorted, list_offsets, previous)
    if x_sorted.dim() != 2 or previous.dim() != 2 or previous.shape[1] != x_sorted.shape[1] or previous.shape[0] < 1 or \
            x_sorted.shape[1] < 1:
        raise ValueError("ivf_list_mean: x_sorted (V, D) and previous (nlists, D) expected")
    if x_sorted.dtype != torch.float32 or previous.dtype != torch.float32:
        raise ValueError("torch_rechub_amd: ivf_list_mean takes float32 tensors")
    nlists = int(previous.shape[0])
    if list_offsets.dtype != torch.int32 or tuple(list_offsets.shape) != (nlists + 1,):
        raise ValueError("ivf_list_mean: list_offsets (nlists + 1,) int32 expected")
    if not x_sorted.is_contiguous():
        raise ValueError("ivf_list_mean: the rows must be contiguous")
    V, D = (int(v) for v in x_sorted.shape)
    if V >= 2 ** 31:
        from ..models.matching._listwise import no_kernel
        raise no_kernel(f"the list mean over V={V} rows (V < 2^31)")
    previous, list_offsets = previous.detach().contiguous(), list_offsets.contiguous()
    out = torch.empty_like(previous)
    _lib.call("rh_ivf_list_mean", _p(x_sorted.detach()), _p(list_offsets), _p(previous), V, D, nlists, _p(out), _stream())
    return out
