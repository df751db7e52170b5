"""Autograd bindings of the gfx950 kernels (C ABI in ``include/rechub_hip.h``).

Each op hands raw device pointers + the current HIP stream to ``librechub_hip.so`` through ctypes.
PyTorch is only the allocator / stream / autograd plumbing here.  There is no CPU path: tensors that
are not on a HIP device raise ``RuntimeError``.

Gradient convention for embedding tables (replaces ``embedding_dense_backward`` + ``model.zero_grad``,
reference trainers/ctr_trainer.py:97-98): every table owns ONE persistent dense gradient buffer
(``grad_buffer(weight)``), zero outside the rows touched since the last optimizer step.  The fused
backward scatter-adds into it and publishes it as ``weight.grad``; ``FusedDenseAdam`` re-zeroes the
touched rows inside its own pass.  A stock ``torch.optim`` optimizer sees an ordinary dense ``.grad``.
"""
import ctypes
import math
import os
from collections import OrderedDict

import torch

from . import _lib

_NULL = ctypes.c_void_p(0)


_empty_stub = {}


def _p(t):
    """Device pointer of a tensor for the C ABI.  An EMPTY tensor has a null data_ptr(); the entry points check their
    pointers before they look at the sizes (and then return at once for B = 0), so empties are passed as a pointer to
    a small per-device stub allocation."""
    if t is None:
        return _NULL
    if t.numel() == 0:
        stub = _empty_stub.get(t.device)
        if stub is None:
            stub = torch.zeros(64, dtype=torch.float32, device=t.device)
            _empty_stub[t.device] = stub
        return ctypes.c_void_p(stub.data_ptr())
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


_BRANCH_STREAMS = {}


def run_beside(fn_main, fn_side, side_inputs=()):
    """(fn_main(), fn_side()) with fn_side on a second HIP stream: fork after everything enqueued so far, join before
    returning.  Inside a hipGraph capture the two become concurrent branches of the graph (tools/probe/branch_probe.cpp:
    captured branches do run side by side on this runtime); autograd runs each op's backward on the stream of its forward,
    so the backward forks and joins the same way.  For two independent chains of small kernels (the towers of a two-tower
    model: each launch fills a fraction of the 256 CUs)."""
    cur = torch.cuda.current_stream()
    key = cur.device.index
    side = _BRANCH_STREAMS.get(key)
    if side is None:
        from . import graphs
        side = _BRANCH_STREAMS[key] = graphs.role_stream("branch", cur.device)
    side.wait_stream(cur)
    for t in side_inputs:
        t.record_stream(side)
    with torch.cuda.stream(side):
        b = fn_side()
    a = fn_main()
    cur.wait_stream(side)
    for t in (b if isinstance(b, (tuple, list)) else (b,)):
        if torch.is_tensor(t):
            t.record_stream(cur)
    return a, b


def require_hip(*tensors):
    """Fail loudly for anything that is not a HIP tensor (there is no CPU fallback)."""
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("torch_rechub_amd: this op runs only on a HIP device (MI355X); got a "
                               f"{t.device} tensor. There is no CPU fallback by design.")
    _lib.load()


# --------------------------------------------------------------------------------------------
# persistent per-table state
# --------------------------------------------------------------------------------------------
def grad_buffer(weight):
    """The persistent dense gradient buffer of a table (allocated zeroed on first use)."""
    buf = getattr(weight, "_rh_grad", None)
    if buf is None or buf.device != weight.device or buf.shape != weight.shape:
        buf = torch.zeros_like(weight, memory_format=torch.contiguous_format)
        weight._rh_grad = buf
        weight._rh_dirty = False
    return buf


def _publish_grad(weight):
    """Make ``weight.grad`` the persistent buffer (folding in a foreign dense grad if one exists)."""
    buf = weight._rh_grad
    g = weight.grad
    if g is None:
        weight.grad = buf
    elif g.data_ptr() != buf.data_ptr():
        buf.add_(g)
        weight.grad = buf
    weight._rh_dirty = True


def _prepare_grad(weight):
    """Called before a scatter: drop stale contents if the user reset ``.grad`` since the last backward."""
    buf = grad_buffer(weight)
    if weight._rh_dirty:
        g = weight.grad
        if g is None or g.data_ptr() != buf.data_ptr():
            buf.zero_()  # zero_grad(set_to_none=True) happened: the buffer holds last step's rows
            weight._rh_dirty = False
    return buf


_err_flags = {}


def err_flag(device):
    """Per-device int32 word the kernels OR error bits into (index out of range ...)."""
    f = _err_flags.get(device)
    if f is None:
        f = torch.zeros(1, dtype=torch.int32, device=device)
        _err_flags[device] = f
    return f


def check_errors(device=None):
    """Synchronising check of the kernel error word; raises IndexError like the reference's CPU path."""
    for dev, f in list(_err_flags.items()):
        if device is not None and dev != device:
            continue
        v = int(f.item())
        if v:
            f.zero_()
            if v & _lib.H.RH_FLAG_INDEX_OOB:
                raise IndexError("torch_rechub_amd: an embedding index was out of range (index < 0 or >= vocab_size)")
            if v & _lib.H.RH_FLAG_TARGET_OOB:
                raise IndexError("torch_rechub_amd: a target label was out of range (label < 0 or >= the number of classes)")
            if v & _lib.H.RH_FLAG_SESSION_EMPTY:
                raise RuntimeError("torch_rechub_amd: Length of all samples has to be greater than 0 (a session holds no item)")
            if v & _lib.H.RH_FLAG_SESSION_SHORT:
                raise RuntimeError("torch_rechub_amd: the longest session of the batch is shorter than its padded length L "
                                   "(the reference NARM fails to broadcast its states against the mask)")
            if v & _lib.H.RH_ERR_GATE_TIMEOUT:
                raise RuntimeError("torch_rechub_amd: a deferred table sweep waited 2 s for a training step that never started "
                                   "(rh_adam_sweep_gate); the tables may be inconsistent")
            raise RuntimeError(f"torch_rechub_amd: kernel error flag {v}")


class _DescCache(object):
    """LRU of host tuples -> device int64 descriptor tensors (no upload when pointers repeat).

    An entry that was looked up while a hipGraph was being captured is PINNED: the graph keeps reading that device
    tensor on every replay, so it must never be evicted (freed) afterwards."""

    def __init__(self, cap=1024):
        self.cap = cap
        self.d = OrderedDict()
        self.pinned = {}

    def get(self, key, device):
        k = (key, device)
        t = self.pinned.get(k)
        if t is not None:
            return t
        capturing = device.type == "cuda" and torch.cuda.is_current_stream_capturing()
        t = self.d.get(k)
        if t is None:
            if capturing:
                raise RuntimeError("torch_rechub_amd: a descriptor table would have to be uploaded during hipGraph "
                                   "capture; run the step eagerly once with the same (static) buffers first")
            t = torch.tensor(key, dtype=torch.int64).to(device)
            self.d[k] = t
            if len(self.d) > self.cap:
                self.d.popitem(last=False)
        else:
            self.d.move_to_end(k)
        if capturing:
            self.pinned[k] = t
        return t


class EmbedCall(object):
    """Everything one fused gather needs besides the autograd inputs: descriptors + shapes.

    weights : table weights per field (a weight may repeat: shared tables)
    pads    : padding_idx per field (-1 = none)
    idx     : index tensors per field, shape (B,), int64 or int32, on the device
    dense   : dense value tensors (B,), float32, appended after the sparse block
    """
    _fcache = _DescCache()
    _icache = _DescCache()
    _dcache = _DescCache()

    def __init__(self, weights, pads, idx, dense=(), want_fm=False, want_lr=False, slots=None, width=None,
                 field_split=0, samples_per_block=0, local_grads=False, replay=True):
        self.local_grads = bool(local_grads)
        # False: the index columns are computed inside the step (x * F + j of a field-aware lookup), so an optimizer must
        # not replay this gather's record ahead of the step that recomputes them (optim.TableAdam: ordinary refresh only)
        self.replay = bool(replay)  # True: never hand the gradient rows to the data-parallel exchange
        self.weights = list(weights)
        self.idx = list(idx)
        self.dense = list(dense)
        F = len(self.weights)
        if F == 0 or len(self.idx) != F or len(pads) != F:
            raise ValueError("EmbedCall: need one weight, padding_idx and index tensor per field")
        require_hip(*self.weights, *self.idx, *self.dense)
        self.F = F
        self.D = int(self.weights[0].shape[1])
        for w in self.weights:
            if w.dim() != 2 or w.shape[1] != self.D or w.dtype != torch.float32 or not w.is_contiguous():
                raise ValueError("EmbedCall: tables must be contiguous float32 (vocab, D) with one common D")
        self.B = int(self.idx[0].shape[0])
        idt = self.idx[0].dtype
        if idt not in (torch.int64, torch.int32):
            raise ValueError(f"EmbedCall: index dtype {idt} unsupported (int64 / int32)")
        for t in self.idx:
            if t.dim() != 1 or t.shape[0] != self.B or t.dtype != idt:
                raise ValueError("EmbedCall: every index tensor must be (B,) with one common integer dtype")
        for t in self.dense:
            if t.dim() != 1 or t.shape[0] != self.B or t.dtype != torch.float32:
                raise ValueError("EmbedCall: dense values must be float32 (B,)")
        self.idx_is_i64 = 1 if idt == torch.int64 else 0
        self.pads = [(-1 if p is None else int(p)) for p in pads]
        self.slots = list(range(F)) if slots is None else list(slots)
        self.dense_col = (max(self.slots) + 1) * self.D
        self.width = self.dense_col + len(self.dense) if width is None else int(width)
        self.want_fm = bool(want_fm)
        self.want_lr = bool(want_lr)
        if self.want_lr and self.slots != list(range(F)):
            raise ValueError("EmbedCall: fused LR needs slot f == field f")
        self.field_split = field_split
        self.samples_per_block = samples_per_block
        self.device = self.weights[0].device

    # descriptor tables ------------------------------------------------------------------
    def fdesc(self, with_grads):
        ptrs = [w.data_ptr() for w in self.weights]
        if with_grads:
            gp = [(_prepare_grad(w).data_ptr() if w.requires_grad else 0) for w in self.weights]
        else:
            gp = [0] * self.F
        key = tuple(ptrs + gp + [int(w.shape[0]) for w in self.weights] + self.pads)
        return EmbedCall._fcache.get(key, self.device)

    def idesc(self):
        key = tuple([t.data_ptr() for t in self.idx] + [t.stride(0) for t in self.idx] + self.slots)
        return EmbedCall._icache.get(key, self.device)

    def ddesc(self):
        if not self.dense:
            return None
        key = tuple([t.data_ptr() for t in self.dense] + [t.stride(0) for t in self.dense])
        return EmbedCall._dcache.get(key, self.device)


# Fusions that have an unfused twin kept for A/B parity tests (tests flip these module attributes; they are not
# environment switches): the head's backward forming the BatchNorm sums of the layer below, the Dice + output-layer pass of
# DIN's attention MLP, BatchNorm + PReLU + Dropout as one launch pair.
FUSE_HEAD_BN = True
FUSE_DICE_HEAD = True
FUSE_BN_PRELU = True


# Lazy optimizers (optim.TableAdam(lazy_k > 1)) listen to two events, through weak references:
#   on_gather(record): rows are about to be READ -> bring them up to date first (a row that was not in recent batches
#                      lags behind the dense semantics until someone looks at it);
#   on_touch(record):  (table, index column) pairs received gradient -> the next step must claim those rows.
# A record keeps the index tensors alive until the listener consumed it.
_lazy_listeners = []


def add_lazy_listener(obj):
    import weakref
    _lazy_listeners.append(weakref.ref(obj))


def _listeners():
    live = [r for r in _lazy_listeners if r() is not None]
    if len(live) != len(_lazy_listeners):
        _lazy_listeners[:] = live
    return [r() for r in live]


def _log_touch(weights, pads, idesc, idx_is_i64, B, F, D, keep):
    for lst in _listeners():
        lst.on_touch(dict(weights=list(weights), pads=list(pads), idesc=idesc, idx_is_i64=idx_is_i64, B=B, F=F, D=D,
                          keep=keep))


def _pre_gather(weights, pads, idesc, idx_is_i64, B, F, D, training=None, keep=None, replay=True):
    """``training``: the lookup is part of a differentiated forward (a backward / optimizer step follows).  Inside an
    autograd.Function.forward grad mode is off, so the callers pass ctx.needs_input_grad; None = ask grad mode.
    ``keep``: the index tensor(s) behind ``idesc`` -- a listener that keeps the record (TableAdam's refresh-ahead replays the
    previous step's records) keeps the memory the descriptor points at alive with it.
    ``replay``: False when the index buffer behind ``idesc`` is computed inside the step (EmbedCall.replay)."""
    if training is None:
        training = torch.is_grad_enabled()
    for lst in _listeners():
        lst.on_gather(dict(weights=list(weights), pads=list(pads), idesc=idesc, idx_is_i64=idx_is_i64, B=B, F=F, D=D,
                           training=bool(training), keep=keep, replay=bool(replay)))


# data-parallel exchange hook: set by torch_rechub_amd.distributed when world_size > 1
_sparse_exchange = None
_row_gather = None


def set_sparse_exchange(fn, row_gather=None):
    """fn(call, rows_local (B,F,D)) -> (idx_all (W*B,F) int, rows_all (W*B,F,D)), or None when fn keeps the rows and
    runs the exchange + scatter itself after the backward.  row_gather(t) -> the rows of ``t`` from every rank in rank
    order (used by the sequence-feature backward, which scatters the gathered batch in line).
    set_sparse_exchange(None) disables both."""
    global _sparse_exchange, _row_gather
    _sparse_exchange = fn
    _row_gather = row_gather if fn is not None else None


_pre_backward_hooks = []


def add_pre_embed_backward_hook(fn):
    """fn() runs at the start of every fused-embedding backward (used to kick the dense all-reduce early)."""
    _pre_backward_hooks.append(fn)
    return fn


def remove_pre_embed_backward_hook(fn):
    if fn in _pre_backward_hooks:
        _pre_backward_hooks.remove(fn)


class _EmbedFused(torch.autograd.Function):
    """out (B,width), fm (B,1)|None, lr (B,1)|None = fused_embedding(call, lr_w, lr_b, *table weights)."""

    @staticmethod
    def forward(ctx, call, lr_w, lr_b, *weights):
        B, F, D = call.B, call.F, call.D
        dev = call.device
        # row pitch rounded up to 64 bytes: with 13 dense columns a (B, 429) row is 1716 B, every 64-byte field chunk
        # straddles two cache lines and every store is a partial-line write; at pitch 432 the chunks ARE lines.  The
        # result is the (B, width) view of the padded buffer (row stride 432): GEMMs take a leading dimension.
        pitch = (call.width + 15) // 16 * 16
        out = torch.empty((B, pitch), dtype=torch.float32, device=dev)[:, :call.width]
        fm = torch.empty((B, 1), dtype=torch.float32, device=dev) if call.want_fm else None
        lr = torch.empty((B, 1), dtype=torch.float32, device=dev) if call.want_lr else None
        s_sum = torch.empty((B, D), dtype=torch.float32, device=dev) if call.want_fm else None
        if call.want_lr:
            if lr_w is None or lr_w.numel() != F * D or not lr_w.is_contiguous() or lr_w.dtype != torch.float32:
                raise ValueError("fused LR weight must be contiguous float32 with F*D elements")
            require_hip(lr_w, lr_b)
        ddesc = call.ddesc()
        _pre_gather(call.weights, call.pads, call.idesc(), call.idx_is_i64, B, F, D, training=any(ctx.needs_input_grad),
                    keep=call.idx, replay=call.replay)
        _lib.call("rh_embed_fwd", _p(call.fdesc(False)), _p(call.idesc()), call.idx_is_i64, B, F, D, _p(ddesc),
                  len(call.dense), call.dense_col, _p(out), out.stride(0), _p(lr_w if call.want_lr else None),
                  _p(lr_b if call.want_lr else None), _p(lr), _p(fm), _p(s_sum), call.field_split,
                  _p(err_flag(dev)), _stream())
        ctx.call = call
        ctx.has_lr_b = lr_b is not None
        ctx.lr_params = (lr_w, lr_b)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(out, s_sum, lr_w if call.want_lr else None)
        return out, fm, lr

    @staticmethod
    def backward(ctx, g_out, g_fm, g_lr):
        call = ctx.call
        out, s_sum, lr_w = ctx.saved_tensors
        B, F, D = call.B, call.F, call.D
        dev = call.device
        for hook in list(_pre_backward_hooks):
            hook()
        if g_out is not None and (g_out.stride(1) != 1 or g_out.stride(0) < call.width):
            g_out = g_out.contiguous()
        g_fm = None if g_fm is None else g_fm.reshape(-1).contiguous()
        g_lr = None if g_lr is None else g_lr.reshape(-1).contiguous()
        any_table = any(w.requires_grad for w in call.weights)
        want_wgrad = g_lr is not None and lr_w is not None and ctx.needs_input_grad[1]
        nchunks = _lib.call("rh_embed_bwd_nchunks", B, call.samples_per_block)
        partial = torch.empty((nchunks, F * D), dtype=torch.float32, device=dev) if want_wgrad else None
        # local_grads: a lookup over row-sharded tables already holds the gradient rows of the global batch
        exchange = _sparse_exchange if (any_table and not call.local_grads) else None
        if any_table or want_wgrad:
            if exchange is None:
                fdesc = call.fdesc(True)
                rows = None
                sink = 0
            else:
                fdesc = call.fdesc(False)
                rows = torch.empty((B, F, D), dtype=torch.float32, device=dev)
                sink = 1
            _lib.call("rh_embed_bwd", _p(fdesc), _p(call.idesc()), call.idx_is_i64, B, F, D, _p(g_out),
                      0 if g_out is None else g_out.stride(0), _p(out), out.stride(0), _p(s_sum), _p(g_fm), _p(g_lr),
                      _p(lr_w), _p(partial), 1.0, sink, _p(rows), call.samples_per_block, _p(err_flag(dev)),
                      _stream())
            if exchange is not None:
                gathered = exchange(call, rows)
                if gathered is not None:  # None: the exchange is deferred to after the backward (split-graph step)
                    scatter_rows(call, gathered[0], gathered[1])
            elif any_table:
                _log_touch(call.weights, call.pads, call.idesc(), call.idx_is_i64, B, F, D, call.idx)
            if any_table:
                for w in {id(w): w for w in call.weights if w.requires_grad}.values():
                    _publish_grad(w)
        want_b = g_lr is not None and ctx.has_lr_b and ctx.needs_input_grad[2]
        wp, bp = ctx.lr_params
        armed = deferred.armed
        if B > 0 and want_wgrad and armed is not None and id(wp) in armed and (not want_b or id(bp) in armed):
            # the per-block partial rows (and, for the bias, the per-sample g_lr) go to the step's packing launch
            g_w = deferred.offer(wp, partial.data_ptr(), nchunks, F * D, F * D, lambda: partial.sum(0).view_as(lr_w), partial)
            g_b = None
            if want_b:
                glc = g_lr.contiguous()
                g_b = deferred.offer(bp, glc.data_ptr(), glc.numel(), 1, 1, lambda: glc.sum().view(1), glc)
            return (None, g_w, g_b) + (None,) * len(call.weights)
        g_w = torch.empty_like(lr_w) if want_wgrad else None
        g_b = torch.empty((1,), dtype=torch.float32, device=dev) if want_b else None
        if B == 0:  # empty batch: nothing was launched; the parameter gradients are exact zeros
            g_w = None if g_w is None else g_w.zero_()
            g_b = None if g_b is None else g_b.zero_()
        elif want_wgrad or want_b:  # one launch: column sums of the per-block LR partials + sum of g_lr
            glc = g_lr.contiguous() if want_b else None
            _lib.call("rh_colsum", _p(partial), nchunks if want_wgrad else 0, F * D, _p(g_w), _p(glc),
                      glc.numel() if want_b else 0, _p(g_b), _stream())
        return (None, g_w, g_b) + (None,) * len(call.weights)


def fused_embedding(call, lr_w=None, lr_b=None):
    """Run the fused gather (+FM, +LR); returns (out, fm, lr) with fm / lr None when not requested."""
    return _EmbedFused.apply(call, lr_w, lr_b, *call.weights)


_row_ids = {}


def _row_index(B, F, device):
    """int32 (B, F) with entry b * F + f: the lookup (b, f) of a (B, F*D) row block read as a (B*F, D) table."""
    key = (B, F, str(device))
    t = _row_ids.get(key)
    if t is None:
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("torch_rechub_amd: run the step eagerly once before capturing a hipGraph")
        t = torch.arange(B * F, dtype=torch.int32, device=device).view(B, F)
        _row_ids[key] = t
    return t


class _RowsFused(torch.autograd.Function):
    """The fused gather's second half on rows that are already in HBM: ``emb`` (B, F*D) -- the result of a row-sharded
    lookup (sharding.lookup) -- goes through the SAME kernels as a (B*F, D) table indexed by b*F + f, so that one launch
    emits the flattened MLP input (sparse block + dense values, Q1), the FM scalar and the LR scalar, and one launch
    computes the gradient of all three with respect to every row (``sink = 1``: per-lookup gradient rows, the form the
    row exchange carries) plus the per-block LR weight partials.  Keep ``emb`` at a fixed address from step to step
    (sharding.lookup does): the descriptor tables are cached by address."""

    @staticmethod
    def forward(ctx, emb, F, dense, lr_w, lr_b, want_fm):
        require_hip(emb, *dense)
        if emb.dim() != 2 or emb.dtype != torch.float32 or not emb.is_contiguous() or emb.shape[1] % F:
            raise ValueError("fused_rows: rows must be a contiguous float32 (B, F*D) matrix")
        B, D = int(emb.shape[0]), int(emb.shape[1]) // F
        dev = emb.device
        want_lr = lr_w is not None
        if want_lr:
            if lr_w.numel() != F * D or not lr_w.is_contiguous() or lr_w.dtype != torch.float32:
                raise ValueError("fused LR weight must be contiguous float32 with F*D elements")
            require_hip(lr_w, lr_b)
        for t in dense:
            if t.dim() != 1 or t.shape[0] != B or t.dtype != torch.float32:
                raise ValueError("fused_rows: dense values must be float32 (B,)")
        ids = _row_index(B, F, dev)
        fdesc = EmbedCall._fcache.get(tuple([emb.data_ptr()] * F + [0] * F + [B * F] * F + [-1] * F), dev)
        idesc = EmbedCall._icache.get(tuple([ids.data_ptr() + 4 * f for f in range(F)] + [F] * F + list(range(F))), dev)
        ddesc = None
        if dense:
            ddesc = EmbedCall._dcache.get(tuple([t.data_ptr() for t in dense] + [t.stride(0) for t in dense]), dev)
        out = torch.empty((B, F * D + len(dense)), dtype=torch.float32, device=dev)
        fm = torch.empty((B, 1), dtype=torch.float32, device=dev) if want_fm else None
        lr = torch.empty((B, 1), dtype=torch.float32, device=dev) if want_lr else None
        s_sum = torch.empty((B, D), dtype=torch.float32, device=dev) if want_fm else None
        _lib.call("rh_embed_fwd", _p(fdesc), _p(idesc), 0, B, F, D, _p(ddesc), len(dense), F * D, _p(out), out.stride(0),
                  _p(lr_w), _p(lr_b if want_lr else None), _p(lr), _p(fm), _p(s_sum), 0, _p(err_flag(dev)), _stream())
        ctx.meta = (B, F, D, fdesc, idesc, lr_b is not None)
        ctx.set_materialize_grads(False)
        ctx.save_for_backward(out, s_sum, lr_w)
        return out, fm, lr

    @staticmethod
    def backward(ctx, g_out, g_fm, g_lr):
        out, s_sum, lr_w = ctx.saved_tensors
        B, F, D, fdesc, idesc, has_b = ctx.meta
        dev = out.device
        for hook in list(_pre_backward_hooks):
            hook()
        if g_out is not None and (g_out.stride(1) != 1 or g_out.stride(0) < out.shape[1]):
            g_out = g_out.contiguous()
        g_fm = None if g_fm is None else g_fm.reshape(-1).contiguous()
        g_lr = None if g_lr is None else g_lr.reshape(-1).contiguous()
        want_wgrad = g_lr is not None and lr_w is not None and ctx.needs_input_grad[3]
        want_b = g_lr is not None and has_b and ctx.needs_input_grad[4]
        nchunks = _lib.call("rh_embed_bwd_nchunks", B, 0)
        partial = torch.empty((nchunks, F * D), dtype=torch.float32, device=dev) if want_wgrad else None
        rows = torch.empty((B, F * D), dtype=torch.float32, device=dev)
        g_w = torch.empty_like(lr_w) if want_wgrad else None
        g_b = torch.empty((1,), dtype=torch.float32, device=dev) if want_b else None
        if B == 0:
            g_w = None if g_w is None else g_w.zero_()
            g_b = None if g_b is None else g_b.zero_()
            return rows, None, None, g_w, g_b, None
        _lib.call("rh_embed_bwd", _p(fdesc), _p(idesc), 0, B, F, D, _p(g_out), 0 if g_out is None else g_out.stride(0),
                  _p(out), out.stride(0), _p(s_sum), _p(g_fm), _p(g_lr), _p(lr_w), _p(partial), 1.0, 1, _p(rows), 0,
                  _p(err_flag(dev)), _stream())
        if want_wgrad or want_b:
            glc = g_lr.contiguous() if want_b else None
            _lib.call("rh_colsum", _p(partial), nchunks if want_wgrad else 0, F * D, _p(g_w), _p(glc),
                      glc.numel() if want_b else 0, _p(g_b), _stream())
        return rows, None, None, g_w, g_b, None


def fused_rows(emb, n_fields, dense=(), lr_w=None, lr_b=None, want_fm=False):
    """(out (B, F*D + n_dense), fm (B,1)|None, lr (B,1)|None) from rows already gathered into ``emb`` (B, F*D)."""
    return _RowsFused.apply(emb, int(n_fields), tuple(dense), lr_w, lr_b, bool(want_fm))


def scatter_rows(call, idx_all, rows_all):
    """Scatter-add gradient rows (N,F,D) for packed indices idx_all (N,F) into the tables' grad buffers."""
    require_hip(idx_all, rows_all)
    N = int(idx_all.shape[0])
    F, D = call.F, call.D
    ptrs = [idx_all.data_ptr() + f * idx_all.element_size() for f in range(F)]
    key = tuple(ptrs + [idx_all.stride(0)] * F + list(range(F)))
    idesc = EmbedCall._icache.get(key, call.device)
    _lib.call("rh_embed_scatter_rows", _p(call.fdesc(True)), _p(idesc), 1 if idx_all.dtype == torch.int64 else 0,
              N, F, D, _p(rows_all), 1.0, call.samples_per_block, _p(err_flag(call.device)), _stream())
    _log_touch(call.weights, call.pads, idesc, 1 if idx_all.dtype == torch.int64 else 0, N, F, D, [idx_all])


# --------------------------------------------------------------------------------------------
# field-aware FM (DeepFFM / FAT-DeepFFM, csrc/ffm.hip)
_ffm_xv = OrderedDict()
_ffm_xv_pinned = {}


def _ffm_index_buffer(idesc, B, V, dtype, device):
    """The (B, F(F-1)) expanded-index buffer of one set of raw index columns (keyed by their descriptor tensor, itself cached
    by the columns' addresses): its contents are a function of those columns alone, and its address stays fixed from the
    eager steps into a hipGraph capture (its own descriptor is then already uploaded).  Buffers a capture used are kept."""
    key = (idesc.data_ptr(), B, V, dtype, str(device))
    t = _ffm_xv_pinned.get(key)
    if t is None:
        t = _ffm_xv.get(key)
        capturing = device.type == "cuda" and torch.cuda.is_current_stream_capturing()
        if t is None:
            if capturing:
                raise RuntimeError("torch_rechub_amd: run the step eagerly once before capturing a hipGraph")
            t = _ffm_xv[key] = torch.empty((B, V), dtype=dtype, device=device)
            if len(_ffm_xv) > 16:
                _ffm_xv.popitem(last=False)
        else:
            _ffm_xv.move_to_end(key)
        if capturing:
            _ffm_xv_pinned[key] = t
    return t


class FfmCall(object):
    """The fused field-aware lookup of F fields: tables (vocab_f, Dp) whose row x_f * F + j is field f's embedding towards
    field j, the raw (B,) index columns (EmbedCall's rules) and the logical width D <= Dp."""

    def __init__(self, weights, pads, idx, embed_dim):
        self.base = EmbedCall(weights, pads, idx)
        self.F, self.B, self.Dp = self.base.F, self.base.B, self.base.D
        self.D = int(embed_dim)
        if not 2 <= self.F <= _lib.H.RH_FFM_MAX_F or not 1 <= self.D <= min(self.Dp, _lib.H.RH_FFM_MAX_D):
            raise RuntimeError(f"torch_rechub_amd: field-aware FM with {self.F} fields of width {self.D} (row {self.Dp}) "
                               f"has no HIP kernel (2 .. {_lib.H.RH_FFM_MAX_F} fields, width 1 .. {_lib.H.RH_FFM_MAX_D})")
        self.P = self.F * (self.F - 1) // 2
        self.V = self.F * (self.F - 1)
        self.device = self.base.device
        self.weights = self.base.weights

    def virtual_call(self):
        """(EmbedCall over the F(F-1) virtual fields v(i, j) = i (F-1) + (j < i ? j : j - 1), xv): the lookups of the fused
        kernel as ordinary index columns x_i * F + j (rh_ffm_expand_index), for the optimizer's records and the exchange."""
        F, V, B = self.F, self.V, self.B
        base = self.base
        xv = _ffm_index_buffer(base.idesc(), B, V, base.idx[0].dtype, self.device)
        _lib.call("rh_ffm_expand_index", _p(base.idesc()), base.idx_is_i64, B, F, _p(xv), _stream())
        owner = [i for i in range(F) for _ in range(F - 1)]
        vcall = EmbedCall([base.weights[i] for i in owner], [base.pads[i] for i in owner], list(xv.unbind(1)),
                          replay=False)
        return vcall, xv


class _FfmFused(torch.autograd.Function):
    """em (B, P*D) = the pairwise field-aware products read straight from the tables (rh_ffm_fwd, table mode)."""

    @staticmethod
    def forward(ctx, call, *weights):
        B, F, D, Dp, P = call.B, call.F, call.D, call.Dp, call.P
        dev = call.device
        base = call.base
        training = any(ctx.needs_input_grad)
        vcall = xv = None
        if _listeners() or (training and _sparse_exchange is not None):
            vcall, xv = call.virtual_call()
            _pre_gather(vcall.weights, vcall.pads, vcall.idesc(), vcall.idx_is_i64, B, call.V, Dp, training=training,
                        keep=[xv], replay=False)
        em = torch.empty((B, P * D), dtype=torch.float32, device=dev)
        _lib.call("rh_ffm_fwd", _p(base.fdesc(False)), _p(base.idesc()), base.idx_is_i64, _NULL, 0, B, F, D, Dp, 0, _p(em),
                  em.stride(0), _p(err_flag(dev)), _stream())
        ctx.call, ctx.vcall, ctx.xv = call, vcall, xv
        return em

    @staticmethod
    def backward(ctx, g_em):
        call, vcall, xv = ctx.call, ctx.vcall, ctx.xv
        base = call.base
        B, F, D, Dp = call.B, call.F, call.D, call.Dp
        dev = call.device
        nones = (None,) * (1 + len(base.weights))
        if g_em is None or not any(w.requires_grad for w in base.weights):
            return nones
        for hook in list(_pre_backward_hooks):
            hook()
        if g_em.stride(1) != 1:
            g_em = g_em.contiguous()
        exchange = _sparse_exchange
        if exchange is not None and vcall is None:
            raise RuntimeError("torch_rechub_amd: the data-parallel exchange was switched on between forward and backward")
        rows = None
        if exchange is None:
            fdesc = base.fdesc(True)
        else:
            fdesc = base.fdesc(False)
            rows = torch.empty((B, call.V, Dp), dtype=torch.float32, device=dev)
        _lib.call("rh_ffm_bwd", _p(fdesc), _p(base.idesc()), base.idx_is_i64, _NULL, 0, B, F, D, Dp, 0, _p(g_em),
                  g_em.stride(0), _NULL, 0, 0 if rows is None else 1, _p(rows), _p(err_flag(dev)), _stream())
        if exchange is not None:
            gathered = exchange(vcall, rows)
            if gathered is not None:
                scatter_rows(vcall, gathered[0], gathered[1])
        elif vcall is not None:
            _log_touch(vcall.weights, vcall.pads, vcall.idesc(), vcall.idx_is_i64, B, call.V, Dp, [xv])
        for w in {id(w): w for w in base.weights if w.requires_grad}.values():
            _publish_grad(w)
        return nones


def ffm_fused(call):
    """em (B, P*D) of a FfmCall: the MLP input of DeepFFM (deepffm.py:57-65 of the reference) without the (B, F, F, D)
    lookup; the backward scatters into the tables' gradient buffers (or hands rows to the data-parallel exchange)."""
    return _FfmFused.apply(call, *call.weights)


class _FfmDenseFn(torch.autograd.Function):
    """FFM.forward on a (B, F, F, D) tensor (rh_ffm_fwd / rh_ffm_bwd, dense mode): (B, P, D) or (B, P, 1)."""

    @staticmethod
    def forward(ctx, x, reduce_sum):
        require_hip(x)
        B, F, F2, D = (int(v) for v in x.shape)
        if F != F2 or x.dtype != torch.float32:
            raise ValueError("ffm: input must be float32 (B, F, F, D)")
        if x.stride(3) != 1 or x.stride(2) != D or x.stride(1) != F * D:
            x = x.contiguous()
        P = F * (F - 1) // 2
        out = torch.empty((B, P, 1 if reduce_sum else D), dtype=torch.float32, device=x.device)
        _lib.call("rh_ffm_fwd", _NULL, _NULL, 0, _p(x), x.stride(0), B, F, D, D, int(reduce_sum), _p(out), out.stride(0),
                  _NULL, _stream())
        ctx.reduce_sum = bool(reduce_sum)
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, g):
        x, = ctx.saved_tensors
        B, F, _, D = (int(v) for v in x.shape)
        g = g.contiguous()
        gx = torch.empty((B, F, F, D), dtype=torch.float32, device=x.device)
        _lib.call("rh_ffm_bwd", _NULL, _NULL, 0, _p(x), x.stride(0), B, F, D, D, int(ctx.reduce_sum), _p(g), g.stride(0),
                  _p(gx), gx.stride(0), 0, _NULL, _NULL, _stream())
        return gx, None


def ffm(x, reduce_sum=True):
    """The reference's FFM layer (basic/layers.py:736-746) on a (B, F, F, D) input."""
    return _FfmDenseFn.apply(x, bool(reduce_sum))


def _em_2d(em, P, D):
    """(B, P*D) view with unit column stride of a (B, P, D) / (B, P*D) tensor, and its row stride."""
    if em.dim() == 3:
        em = em.reshape(em.shape[0], P * D)
    if em.stride(1) != 1:
        em = em.contiguous()
    return em


class _CenDescFn(torch.autograd.Function):
    """d (B, P) = relu(sum_d u * em) (CEN.forward, basic/layers.py:779 of the reference); u gradient without atomics."""

    @staticmethod
    def forward(ctx, em, u):
        require_hip(em, u)
        P, D = int(u.shape[0]), int(u.shape[1])
        ctx.in_shape = em.shape
        em = _em_2d(em, P, D)
        u = u.contiguous()
        B = int(em.shape[0])
        d = torch.empty((B, P), dtype=torch.float32, device=em.device)
        _lib.call("rh_cen_desc_fwd", _p(em), em.stride(0), _p(u), B, P, D, _p(d), _stream())
        ctx.save_for_backward(em, u, d)
        return d

    @staticmethod
    def backward(ctx, g_d):
        em, u, d = ctx.saved_tensors
        B, P, D = int(em.shape[0]), int(u.shape[0]), int(u.shape[1])
        g_d = g_d.contiguous()
        g_em = torch.empty((B, P * D), dtype=torch.float32, device=em.device)
        nch = _lib.call("rh_cen_nchunks", B)
        part = torch.empty((max(nch, 1), P * D), dtype=torch.float32, device=em.device)
        _lib.call("rh_cen_desc_bwd", _p(em), em.stride(0), _p(u), _p(d), _p(g_d), B, P, D, _p(g_em), _p(part), _stream())
        g_u = torch.empty((P, D), dtype=torch.float32, device=em.device)
        if B == 0:
            g_u.zero_()
        else:
            _lib.call("rh_colsum", _p(part), nch, P * D, _p(g_u), _NULL, 0, _NULL, _stream())
        return g_em.view(ctx.in_shape), g_u


class _CenRescaleFn(torch.autograd.Function):
    """aem (B, P*D) = s[b, p] * em[b, p, :] (CEN.forward, basic/layers.py:785-786 of the reference)."""

    @staticmethod
    def forward(ctx, em, s, P, D):
        require_hip(em, s)
        ctx.in_shape = em.shape
        em = _em_2d(em, P, D)
        s = s.contiguous()
        B = int(em.shape[0])
        out = torch.empty((B, P * D), dtype=torch.float32, device=em.device)
        _lib.call("rh_cen_rescale_fwd", _p(em), em.stride(0), _p(s), B, P, D, _p(out), _stream())
        ctx.dims = (P, D)
        ctx.save_for_backward(em, s)
        return out

    @staticmethod
    def backward(ctx, g):
        em, s = ctx.saved_tensors
        P, D = ctx.dims
        B = int(em.shape[0])
        if g.stride(1) != 1:
            g = g.contiguous()
        g_em = torch.empty((B, P * D), dtype=torch.float32, device=em.device)
        g_s = torch.empty((B, P), dtype=torch.float32, device=em.device)
        _lib.call("rh_cen_rescale_bwd", _p(em), em.stride(0), _p(s), _p(g), g.stride(0), B, P, D, _p(g_em), _p(g_s),
                  _stream())
        return g_em.view(ctx.in_shape), g_s, None, None


def cen_descriptor(em, u):
    """relu(sum_d u * em): (B, P) from em (B, P, D) or (B, P*D)."""
    return _CenDescFn.apply(em, u)


def cen_rescale(em, s):
    """s.unsqueeze(-1) * em, flattened to (B, P*D)."""
    B, P = int(s.shape[0]), int(s.shape[1])
    return _CenRescaleFn.apply(em, s, P, int(em.shape[-1]) if em.dim() == 3 else int(em.shape[1]) // P)


# --------------------------------------------------------------------------------------------
class _FMFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, reduce_sum):
        require_hip(x)
        if x.dim() != 3 or x.dtype != torch.float32:
            raise ValueError("FM expects a float32 (B, num_features, embed_dim) tensor")
        if x.stride(2) != 1 or x.stride(1) != x.shape[2]:
            x = x.contiguous()
        B, F, D = x.shape
        out = torch.empty((B, 1) if reduce_sum else (B, D), dtype=torch.float32, device=x.device)
        _lib.call("rh_fm_fwd", _p(x), x.stride(0), B, F, D, 1 if reduce_sum else 0, _p(out), _stream())
        ctx.reduce_sum = reduce_sum
        ctx.save_for_backward(x)
        return out

    @staticmethod
    def backward(ctx, g):
        (x,) = ctx.saved_tensors
        B, F, D = x.shape
        g = g.contiguous()
        gx = torch.empty((B, F, D), dtype=torch.float32, device=x.device)
        _lib.call("rh_fm_bwd", _p(x), x.stride(0), B, F, D, 1 if ctx.reduce_sum else 0, _p(g), _p(gx), gx.stride(0),
                  _stream())
        return gx, None


def fm(x, reduce_sum=True):
    return _FMFn.apply(x, reduce_sum)


# --------------------------------------------------------------------------------------------
_POOL_MODES = {"sum": 0, "mean": 1, "concat": 2}


class _SeqPoolFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, weight, idx, mode, sentinel, padding_idx, local_grads=False):
        ctx.local_grads = local_grads
        require_hip(weight, idx)
        if idx.dim() != 2 or idx.dtype not in (torch.int64, torch.int32):
            raise ValueError("sequence feature values must be an integer (B, L) tensor")
        B, L = idx.shape
        V, D = weight.shape
        out = torch.empty((B, L, D) if mode == 2 else (B, D), dtype=torch.float32, device=weight.device)
        if _lazy_listeners:
            flat = idx.reshape(-1) if idx.is_contiguous() else idx.contiguous().view(-1)
            # (the padding positions of a post-padded history all carry padding_idx: the refresh skips those lookups and
            # keeps the padding row itself current once per launch -- csrc/optim.hip)
            _pre_gather([weight], [padding_idx], EmbedCall._icache.get((flat.data_ptr(), 1, 0), weight.device),
                        1 if idx.dtype == torch.int64 else 0, B * L, 1, D, training=any(ctx.needs_input_grad), keep=[flat])
        _lib.call("rh_seq_pool_fwd", _p(weight), V, _p(idx), 1 if idx.dtype == torch.int64 else 0, idx.stride(0),
                  idx.stride(1), B, L, D, mode, sentinel, _p(out), out.stride(0), _p(err_flag(weight.device)),
                  _stream())
        ctx.meta = (mode, sentinel, -1 if padding_idx is None else int(padding_idx))
        ctx.weight = weight
        ctx.save_for_backward(idx)
        return out

    @staticmethod
    def backward(ctx, g):
        (idx,) = ctx.saved_tensors
        weight = ctx.weight
        mode, sentinel, pad = ctx.meta
        if weight.requires_grad:
            g = g.contiguous()
            if _row_gather is not None and not ctx.local_grads:
                # replicated table under data parallelism: every replica applies the gradient rows of the global batch
                idx, g = _row_gather(idx.contiguous()), _row_gather(g)
            B, L = idx.shape
            V, D = weight.shape
            buf = _prepare_grad(weight)
            _lib.call("rh_seq_pool_bwd", _p(buf), V, _p(idx), 1 if idx.dtype == torch.int64 else 0, idx.stride(0),
                      idx.stride(1), B, L, D, mode, sentinel, pad, _p(g), g.stride(0), 1.0,
                      _p(err_flag(weight.device)), _stream())
            _publish_grad(weight)
            if _lazy_listeners:  # the (B, L) positions are B*L lookups of one field
                flat = idx.reshape(-1) if idx.is_contiguous() else idx.contiguous().view(-1)
                idesc = EmbedCall._icache.get((flat.data_ptr(), 1, 0), weight.device)
                _log_touch([weight], [pad], idesc, 1 if idx.dtype == torch.int64 else 0, B * L, 1, D, [flat])
        return None, None, None, None, None, None


def seq_pool(weight, idx, pooling, padding_idx, local_grads=False):
    """Gather + masked pooling of one sequence feature (mask sentinel = padding_idx, or -1 when unset).
    ``local_grads``: the caller already feeds the gradient of the global batch (row-sharded tables)."""
    if pooling not in _POOL_MODES:
        raise ValueError("Sequence pooling method supports only pooling in %s, got %s." % (["sum", "mean"], pooling))
    sentinel = -1 if padding_idx is None else int(padding_idx)
    return _SeqPoolFn.apply(weight, idx, _POOL_MODES[pooling], sentinel, padding_idx, local_grads)


# --------------------------------------------------------------------------------------------
class _CrossFn(torch.autograd.Function):
    """CrossNetwork: x_{l+1} = x0 * (w_l . x_l) + b_l + x_l, W and Bv stacked (L, d)."""

    @staticmethod
    def forward(ctx, x, W, Bv):
        require_hip(x, W, Bv)
        if x.dim() != 2 or x.dtype != torch.float32:
            raise ValueError("CrossNetwork expects a float32 (B, d) tensor")
        if x.stride(1) != 1:
            x = x.contiguous()
        W = W.contiguous()
        Bv = Bv.contiguous()
        B, d = x.shape
        L = W.shape[0]
        seg = _lib.call("rh_cross_max_layers", d)
        if seg <= 0:
            raise ValueError(f"CrossNetwork width {d} unsupported by the HIP kernel (1..{_lib.H.RH_CROSS_MAX_D})")
        xs = [x]
        cur = x
        for l0 in range(0, L, seg):
            n = min(seg, L - l0)
            out = torch.empty((B, d), dtype=torch.float32, device=x.device)
            _lib.call("rh_cross_fwd", _p(x), x.stride(0), _p(cur), cur.stride(0), _p(W[l0:l0 + n]), _p(Bv[l0:l0 + n]),
                      B, d, n, _p(out), out.stride(0), _stream())
            cur = out
            xs.append(cur)
        ctx.seg = seg
        ctx.save_for_backward(W, Bv, *xs[:-1])
        return cur

    @staticmethod
    def backward(ctx, g):
        W, Bv, *xs = ctx.saved_tensors
        x = xs[0]
        B, d = x.shape
        L = W.shape[0]
        seg = ctx.seg
        g = g.contiguous()
        if B == 0:
            return g, torch.zeros_like(W), torch.zeros_like(Bv)
        gW = torch.empty_like(W)
        gB = torch.empty_like(Bv)
        nblocks = _lib.call("rh_cross_bwd_nblocks", B)
        starts = list(range(0, L, seg))
        gx0_total = None
        for si in reversed(range(len(starts))):
            l0 = starts[si]
            n = min(seg, L - l0)
            cur = xs[si]
            first = si == 0
            partial = torch.empty((nblocks, 2, n, d), dtype=torch.float32, device=x.device)
            gx = torch.empty((B, d), dtype=torch.float32, device=x.device)
            gx0 = None if first else torch.empty((B, d), dtype=torch.float32, device=x.device)
            _lib.call("rh_cross_bwd", _p(x), x.stride(0), _p(cur), cur.stride(0), _p(W[l0:l0 + n]), _p(Bv[l0:l0 + n]),
                      B, d, n, _p(g), g.stride(0), _p(gx0), _p(gx), gx.stride(0), 1 if first else 0, _p(partial),
                      _stream())
            red = partial.sum(0)
            gW[l0:l0 + n] = red[0]
            gB[l0:l0 + n] = red[1]
            if not first:
                gx0_total = gx0 if gx0_total is None else gx0_total + gx0
            g = gx
        if gx0_total is not None:
            g = g + gx0_total
        return g, gW, gB


def cross_network(x, W, Bv):
    return _CrossFn.apply(x, W, Bv)


# --------------------------------------------------------------------------------------------
_rng_state = {}


def _dropout_rng(device):
    """Device-resident (seed, call counter) of the fused dropout; seeded from torch's generator on first use."""
    st = _rng_state.get(device)
    if st is None:
        st = torch.tensor([torch.initial_seed() & 0x7FFFFFFFFFFFFFFF, 0, 0, 0], dtype=torch.int64).to(device)
        _rng_state[device] = st
    return st


class _BnReluDropoutFn(torch.autograd.Function):
    """y = dropout(relu(batch_norm(h))) for one MLP hidden layer (training mode); see csrc/mlp.hip.
    ``stats`` / ``stats_ctr``: per-slab (sum, M2) of h and the dropout counter drawn by the GEMM that produced h
    (ops.linear_stats), or None."""

    @staticmethod
    def forward(ctx, h, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, p_drop, stats,
                stats_ctr, relu):
        require_hip(h, gamma, beta)
        h = h.contiguous()
        B, C = h.shape
        dev = h.device
        out = torch.empty_like(h)
        if stats is not None:
            partial, prow = stats, _lib.call("rh_gemm_stats_rows", B, C)  # the slab height rh_linear_fwd used
            if tuple(stats.shape) != (-(-B // prow), 2, C):
                raise ValueError("BatchNorm statistics slabs do not match the activations")
        else:
            partial = torch.empty((_lib.call("rh_bn_act_nchunks", B), 2, C), dtype=torch.float32, device=dev)
            prow = 0
        stat = torch.empty((4, C), dtype=torch.float32, device=dev)
        # with GEMM-provided statistics the GEMM already drew this call's dropout counter (and counted the batch)
        saved_ctr = stats_ctr if stats is not None else torch.empty(1, dtype=torch.int64, device=dev)
        rng = _dropout_rng(dev)
        _lib.call("rh_bn_relu_dropout_fwd", _p(h), B, C, _p(gamma), _p(beta), _p(running_mean), _p(running_var),
                  _p(num_batches_tracked), float(momentum), float(eps), float(p_drop), 1, _p(rng), _p(saved_ctr),
                  _p(partial), prow, _p(stat), _p(out), 1 if relu else 0, _stream())
        ctx.p_drop = float(p_drop)
        ctx.relu = bool(relu)
        ctx.save_for_backward(h, gamma, beta, stat, saved_ctr)
        return out

    @staticmethod
    def backward(ctx, dy):
        h, gamma, beta, stat, saved_ctr = ctx.saved_tensors
        B, C = h.shape
        dev = h.device
        dy = dy.contiguous()
        dx = torch.empty_like(h)
        dgamma = torch.empty_like(gamma)
        dbeta = torch.empty_like(beta)
        pre = getattr(ctx, "rh_pre", None)
        ctx.rh_pre = None
        if pre is not None and pre[0].data_ptr() == dy.data_ptr() and pre[0].shape == dy.shape and \
                dy._version == pre[1]:
            # dy is exactly the tensor the output head's backward produced (the head was the only consumer of this
            # layer): its launch already summed (g1, g1 * xhat) per column -> finalize + apply only.  ``pre`` HOLDS that
            # tensor: autograd can then neither sum a second consumer's gradient into it in place (InputBuffer only
            # reuses a buffer it owns alone -> the sum is a new tensor with another address) nor recycle its memory
            # for another gradient; the version counter covers any other in-place writer.
            _lib.call("rh_bn_relu_dropout_bwd_pre", _p(h), _p(dy), B, C, _p(gamma), _p(beta), ctx.p_drop,
                      _p(_dropout_rng(dev)), _p(saved_ctr), _p(pre[2]), pre[3], _p(stat), _p(dx), _p(dgamma), _p(dbeta),
                      1 if ctx.relu else 0, _stream())
            return dx, dgamma, dbeta, None, None, None, None, None, None, None, None, None
        partial = torch.empty((_lib.call("rh_bn_act_nchunks", B), 2, C), dtype=torch.float32, device=dev)
        _lib.call("rh_bn_relu_dropout_bwd", _p(h), _p(dy), B, C, _p(gamma), _p(beta), ctx.p_drop, _p(_dropout_rng(dev)),
                  _p(saved_ctr), _p(partial), _p(stat), _p(dx), _p(dgamma), _p(dbeta), 1 if ctx.relu else 0, _stream())
        return dx, dgamma, dbeta, None, None, None, None, None, None, None, None, None


class _BnPreluDropoutFn(torch.autograd.Function):
    """y = dropout(prelu(batch_norm(h))) for one hidden layer of a two-tower MLP (training mode; one slope, nn.PReLU())."""

    @staticmethod
    def forward(ctx, h, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, eps, p_drop, slope):
        require_hip(h, gamma, beta, slope)
        h = h.contiguous()
        B, C = h.shape
        dev = h.device
        out = torch.empty_like(h)
        partial = torch.empty((_lib.call("rh_bn_act_nchunks", B), 2, C), dtype=torch.float32, device=dev)
        stat = torch.empty((4, C), dtype=torch.float32, device=dev)
        saved_ctr = torch.empty(1, dtype=torch.int64, device=dev)
        _lib.call("rh_bn_prelu_dropout_fwd", _p(h), B, C, _p(gamma), _p(beta), _p(running_mean), _p(running_var),
                  _p(num_batches_tracked), float(momentum), float(eps), float(p_drop), 1, _p(_dropout_rng(dev)), _p(saved_ctr),
                  _p(partial), 0, _p(stat), _p(out), _p(slope), _stream())
        ctx.p_drop = float(p_drop)
        ctx.param = slope
        ctx.save_for_backward(h, gamma, beta, stat, saved_ctr, slope)
        return out

    @staticmethod
    def backward(ctx, dy):
        h, gamma, beta, stat, saved_ctr, slope = ctx.saved_tensors
        B, C = h.shape
        dev = h.device
        dy = dy.contiguous()
        dx = torch.empty_like(h)
        dgamma = torch.empty_like(gamma)
        dbeta = torch.empty_like(beta)
        partial = torch.empty((_lib.call("rh_bn_act_nchunks", B), 2, C), dtype=torch.float32, device=dev)
        nb = _lib.call("rh_bn_prelu_nblocks", B, C)
        sp = torch.empty((nb,), dtype=torch.float32, device=dev)
        _lib.call("rh_bn_prelu_dropout_bwd", _p(h), _p(dy), B, C, _p(gamma), _p(beta), ctx.p_drop, _p(_dropout_rng(dev)),
                  _p(saved_ctr), _p(partial), _p(stat), _p(dx), _p(dgamma), _p(dbeta), _p(slope), _p(sp), _stream())
        g_slope = deferred.offer(ctx.param, sp.data_ptr(), nb, 1, 1, lambda: sp.sum().reshape(1), sp)
        return dx, dgamma, dbeta, None, None, None, None, None, None, g_slope


def bn_prelu_dropout_ok(h, bn, act):
    return (bn.training and type(act) is torch.nn.PReLU and act.weight.numel() == 1 and h.is_cuda and
            h.dtype == torch.float32 and h.dim() == 2 and h.shape[0] > 1 and FUSE_BN_PRELU)


def bn_prelu_dropout(h, bn, act, p_drop):
    """Fused BatchNorm1d + nn.PReLU() + Dropout of one hidden layer (training mode), driven by the modules."""
    return _BnPreluDropoutFn.apply(h, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                   bn.momentum, bn.eps, p_drop, act.weight)


def bn_relu_dropout(h, bn, p_drop, stats=None, relu=True):
    """Fused BatchNorm1d + ReLU + Dropout of one MLP hidden layer, driven by the nn.BatchNorm1d module ``bn``
    (``relu=False``: BatchNorm1d + Dropout only, for layers whose activation is Dice / PReLU / ...).
    ``stats``: the (statistics, counter) pair ops.linear_stats returned for this very ``bn``, or None."""
    if bn.training:
        st, ctr = stats if stats is not None else (None, None)
        return _BnReluDropoutFn.apply(h, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                      bn.momentum, bn.eps, p_drop, st, ctr, relu)
    require_hip(h)
    h = h.contiguous()
    out = torch.empty_like(h)
    _lib.call("rh_bn_relu_dropout_fwd", _p(h), h.shape[0], h.shape[1], _p(bn.weight), _p(bn.bias), _p(bn.running_mean),
              _p(bn.running_var), _p(None), 0.0, float(bn.eps), 0.0, 0, _p(None), _p(None), _p(None), 0, _p(None), _p(out),
              1 if relu else 0, _stream())
    return out


# --------------------------------------------------------------------------------------------
# MLP GEMM backward (weight gradient), output head and loss (csrc/linear.hip)
_MAX_WGRAD_TILES = 4096


def _offer_wgrad_slabs(weight, bias, partial, B):
    """Register the per-split slabs rh_linear_wgrad_partial(_group) left in ``partial`` -- S x (N, K), then S x (N,) -- as
    the gradient sources of ``weight`` / ``bias`` (None: no bias) with the armed ops.deferred."""
    N, K = weight.shape
    S = _lib.call("rh_linear_wgrad_splits", B, N, K)

    def reduce_w():
        flush_wgrad_rider()  # (the slabs may still be waiting for the optimizer's end-of-step launch)
        return partial[:S * N * K].view(S, N, K).sum(0)

    def reduce_b():
        flush_wgrad_rider()
        return partial[S * N * K:S * N * K + S * N].view(S, N).sum(0)

    dW = deferred.offer(weight, partial.data_ptr(), S, N * K, N * K, reduce_w, partial)
    db = None
    if bias is not None:
        db = deferred.offer(bias, partial.data_ptr() + 4 * S * N * K, S, N, N, reduce_b, partial)
    return dW, db


def linear_wgrad(g, x, want_bias=True, weight=None, bias=None, out=None):
    """(dW (N, K), db (N,) | None) = (g^T x, colsum(g)) for g (B, N), x (B, K): split-batch f32 MFMA kernel.

    ``weight`` / ``bias``: the parameters these are the gradients of.  While the trainer's fast path has armed
    ``ops.deferred`` for them, the per-split slabs are NOT reduced here: they are registered and the function returns
    None for that gradient (the step's packing launch sums them into the flat bucket).

    ``out`` = (dW, db): contiguous buffers (slices of a larger gradient, say) the result is written into and returned as;
    for gradients assembled from several products, which therefore cannot be deferred (``weight`` / ``bias`` are not taken)."""
    require_hip(g, x)
    if out is not None and (weight is not None or bias is not None or not want_bias):
        raise ValueError("linear_wgrad: out=(dW, db) goes without weight / bias and with want_bias")
    if g.stride(1) != 1:
        g = g.contiguous()
    if x.stride(1) != 1:
        x = x.contiguous()
    B, N = g.shape
    K = x.shape[1]
    dev = g.device
    if out is not None:
        dW, db = out
        if tuple(dW.shape) != (N, K) or tuple(db.shape) != (N,) or not (dW.is_contiguous() and db.is_contiguous()):
            raise ValueError(f"linear_wgrad: out must be contiguous ({N}, {K}) and ({N},) buffers")
    if B == 0:
        if out is not None:
            return dW.zero_(), db.zero_()
        return (torch.zeros((N, K), dtype=torch.float32, device=dev),
                torch.zeros((N,), dtype=torch.float32, device=dev) if want_bias else None)
    partial = torch.empty(_lib.call("rh_linear_wgrad_workspace", B, N, K), dtype=torch.float32, device=dev)
    armed = deferred.armed
    if armed is not None and weight is not None and id(weight) in armed and (not want_bias or
                                                                              (bias is not None and id(bias) in armed)):
        # (step-ahead graph being captured: the slabs feed nothing but the packing launch at the end of the step, so the launch
        # rides in the optimizer's end-of-step launch with the other weight gradients of the step -- wgrad_rider below)
        rider = wgrad_rider
        if not (rider is not None and B < _lib.H.RH_WGRAD_LONG_MIN_B and rider([(g, g.stride(0), x, x.stride(0), N, K, partial)], B)):
            _lib.call("rh_linear_wgrad_partial", _p(g), g.stride(0), _p(x), x.stride(0), B, N, K, _p(partial), _stream())
        return _offer_wgrad_slabs(weight, bias if want_bias else None, partial, B)
    if out is None:
        dW = torch.empty((N, K), dtype=torch.float32, device=dev)
        db = torch.empty((N,), dtype=torch.float32, device=dev) if want_bias else None
    _lib.call("rh_linear_wgrad", _p(g), g.stride(0), _p(x), x.stride(0), B, N, K, _p(dW), _p(db), _p(partial),
              _stream())
    return dW, db


def linear_ok(x, weight):
    return (x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and weight.dtype == torch.float32 and
            _lib.call("rh_linear_wgrad_tiles", weight.shape[0], weight.shape[1]) <= _MAX_WGRAD_TILES)


# Forward / input-gradient GEMMs: hipBLASLt by default.  RECHUB_OWN_GEMM=1 (or "fwd": forward only) routes batch-sized
# problems (M <= 16384, N, K <= 1024) through the f32-MFMA tile kernel of csrc/gemm.hip, whose epilogue also emits the
# BatchNorm statistics (one BN launch less per layer).  Measured on MI355X at B = 4096 (round 1, same box A/B): the
# whole step is within +-0.5 % of the library path (0.4331 vs 0.4325 ms) -- parity, not yet a win, so it stays opt-in
# (DESIGN.md 3.8).
_GEMM_MAX_M = 16384 if os.environ.get("RECHUB_OWN_GEMM", "0") in ("1", "fwd") else 0
_GEMM_MAX_NK = 1024
_GEMM_DGRAD = os.environ.get("RECHUB_OWN_GEMM", "0") != "fwd"  # "fwd": own forward GEMMs only


def _own_gemm(M, N, K):
    return 0 < M <= _GEMM_MAX_M and N <= _GEMM_MAX_NK and K <= _GEMM_MAX_NK


# Round 6: the FORWARD of an nn.Linear over (B L) rows (DIN's attention MLP: 409 600 x 256 -> 128) on the tile kernel too -- on
# those shapes it is faster than the library GEMM it replaced (configs[3] 5.02-5.17 -> 4.91-4.92 ms per step, same box; the input
# gradient is not: 5.18-5.44 with both), and its epilogue hands the BatchNorm that follows the per-slab statistics of the output
# (no statistics pass over the (B L, C) tensor).  RECHUB_AB=tallgemm=0: the library GEMM + the statistics pass.
TALL_GEMM_FWD = _lib.ab("tallgemm")
_TALL_MIN_M = 65536
_STATS_ONLY = object()  # _LinearFn: per-slab statistics of the output WITHOUT the BatchNorm bookkeeping of rh_linear_fwd


def _tall_fwd(M, N, K):
    # (the measured territory: the attention MLP's widths; wide layers stay with the library's larger tiles)
    return TALL_GEMM_FWD and M >= _TALL_MIN_M and N <= 256 and K <= 512


class _LinearFn(torch.autograd.Function):
    """nn.Linear: forward and input gradient on the f32-MFMA tile kernel at CTR batch sizes (library GEMM otherwise),
    weight + bias gradient on the split-batch MFMA kernel.  With ``want_stats`` the forward also returns the per-slab
    (sum, M2) of its output for the BatchNorm that follows."""

    @staticmethod
    def forward(ctx, x, weight, bias, bn_batches):
        want_stats = bn_batches is not None
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        ctx.params = (weight, bias)  # the parameter objects themselves (ops.deferred keys gradients by identity)
        M, K = x.shape
        N = weight.shape[0]
        stats = ctr = None
        stats_only = bn_batches is _STATS_ONLY
        if (_own_gemm(M, N, K) or _tall_fwd(M, N, K)) and weight.is_contiguous() and x.stride(1) == 1:
            y = torch.empty((M, N), dtype=torch.float32, device=x.device)
            rng = None
            if want_stats:
                rows = _lib.call("rh_gemm_stats_rows", M, N)
                stats = torch.empty((-(-M // rows), 2, N), dtype=torch.float32, device=x.device)
                if not stats_only:
                    ctr = torch.empty(1, dtype=torch.int64, device=x.device)
                    rng = _dropout_rng(x.device)
            _lib.call("rh_linear_fwd", _p(x), x.stride(0), _p(weight), K, _p(bias), M, N, K, _p(y), N, _p(stats), _p(rng),
                      _p(ctr), _p(bn_batches if want_stats and not stats_only else None), _stream())
        else:
            y = torch.nn.functional.linear(x, weight, bias)
        if want_stats:
            if stats is None:
                return y, None, None
            if stats_only:
                ctx.mark_non_differentiable(stats)
                return y, stats, None
            ctx.mark_non_differentiable(stats, ctr)
            return y, stats, ctr
        return y

    @staticmethod
    def backward(ctx, g, *unused):
        x, weight = ctx.saved_tensors
        gx = None
        if ctx.needs_input_grad[0]:
            M, N = g.shape
            K = weight.shape[1]
            if _GEMM_DGRAD and _own_gemm(M, K, N) and weight.is_contiguous() and g.stride(1) == 1:
                gx = torch.empty((M, K), dtype=torch.float32, device=g.device)
                _lib.call("rh_linear_dgrad", _p(g), g.stride(0), _p(weight), K, M, N, K, _p(gx), K, _stream())
            else:
                gx = g.mm(weight)
        dW = db = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            dW, db = linear_wgrad(g, x, want_bias=ctx.has_bias, weight=ctx.params[0], bias=ctx.params[1])
        return gx, dW, db, None


def linear_chunk_stats(x, weight, bias=None):
    """(h, chunk_stats, chunk_rows) for a Linear in front of a training-mode BatchNorm1d whose statistics the consumer finalises
    itself (``bn_dice`` / ``bn_dice_head`` with ``chunk_stats``: rh_bn_stats_from_partial does the BatchNorm bookkeeping): on
    (B L)-row inputs the tile GEMM's epilogue emits the per-slab (sum, M2) of h; otherwise (h, None, 0)."""
    if linear_ok(x, weight) and x.dim() == 2 and _tall_fwd(x.shape[0], weight.shape[0], weight.shape[1]) and \
            weight.is_contiguous() and x.stride(1) == 1:
        h, st, _ = _LinearFn.apply(x, weight, bias, _STATS_ONLY)
        if st is not None:
            return h, st, _lib.call("rh_gemm_stats_rows", int(x.shape[0]), int(weight.shape[0]))
        return h, None, 0
    return linear(x, weight, bias), None, 0


def linear(x, weight, bias=None):
    """F.linear for 2-D fp32 HIP activations; see _LinearFn."""
    if linear_ok(x, weight) and (_own_gemm(x.shape[0], weight.shape[0], weight.shape[1]) or _tall_fwd(
            x.shape[0], weight.shape[0], weight.shape[1]) or (
            torch.is_grad_enabled() and (weight.requires_grad or (bias is not None and bias.requires_grad)))):
        return _LinearFn.apply(x, weight, bias, None)
    return torch.nn.functional.linear(x, weight, bias)


def linear_stats(x, weight, bias, bn):
    """The Linear in front of the training-mode BatchNorm1d ``bn``: returns (h, stats) where stats is None or the pair
    (per-slab (sum, M2) of h, dropout counter) to hand to ``bn_relu_dropout(h, bn, p, stats=stats)`` -- the GEMM then
    has already counted the batch for ``bn`` and drawn the dropout counter of that call."""
    if linear_ok(x, weight):
        h, st, ctr = _LinearFn.apply(x, weight, bias, bn.num_batches_tracked)
        return h, (None if st is None else (st, ctr))
    return torch.nn.functional.linear(x, weight, bias), None


def _col(t, B):
    """(B,) contiguous view of a (B,) / (B, 1) tensor."""
    if t is None:
        return None
    if t.numel() != B:
        raise ValueError(f"head term of {tuple(t.shape)} does not match batch {B}")
    return t.reshape(B).contiguous()


def _leaf_extra(*extras):
    """Is one of the head's extra terms a leaf that wants a gradient?  (see _extra_grads)"""
    return any(e is not None and e.requires_grad and e.grad_fn is None for e in extras)


def _extra_grads(g_z, s0, s1, leaf):
    """The gradients of the head's extra terms e0 / e1: both are g_z.  Handed on as two views of ONE buffer they are safe for
    graph-interior terms (the wide / FM outputs: autograd adds a second gradient into a buffer in place only when it owns its
    storage alone), but a LEAF keeps the very tensor it is handed as its .grad and adds every later backward into it in
    place -- with two leaves on one buffer each accumulation landed in both (e.grad = g(1) + 2 g(2) after two backwards).
    ``leaf``: e1 then gets a buffer of its own."""
    g0 = None if s0 is None else g_z.view(s0)
    g1 = None if s1 is None else g_z.view(s1)
    if leaf and g0 is not None and g1 is not None:
        g1 = g1.clone()
    return g0, g1


class DeferredGrads(object):
    """Parameter gradients that exist only as per-block / per-split partial slabs until the step's ONE packing launch
    (rh_pack_grads) sums them straight into the flat gradient bucket.

    Armed by the single-GPU fast path of the trainers for the parameters of their bucket.  While armed, the backward of
    the weight-gradient, head and fused-embedding kernels skips its trailing reduction launch, registers
    ``(slab, rows, row stride)`` for the parameter and hands autograd ``None`` for it.  A parameter that is used twice in
    one step (second registration) falls back to the immediate reduction for BOTH uses; a gradient produced by any
    other op (``p.grad`` set by autograd) is added on top by the packing launch."""

    def __init__(self):
        self.armed = None  # {id(param): param} of the parameters whose gradients may be deferred
        self.items = {}    # id(param) -> dict(param, slab, nparts, stride, numel, reduce_now)

    def arm(self, params, root=None):
        """``root``: the tensor ``backward()`` is about to be called on.  Given (the data-parallel step: its bucket packs slabs
        and starts their all-reduce IN THE MIDDLE of the backward, DenseGradBucket.flush from the pre-embedding-backward hook),
        the uses of every armed parameter in the autograd graph are counted, and ``final(p)`` says whether all of them have
        reported -- a slab registered by the first of two uses (a Linear shared by two towers, with an embedding backward in
        between) is not the parameter's gradient yet (round-5 advisor finding: the second contribution was lost)."""
        self.armed = {id(p): p for p in params}
        self.items = {}
        self.uses = None
        if root is not None and root.grad_fn is not None:
            self.uses = self._count_uses(root.grad_fn, self.armed)

    @staticmethod
    def _count_uses(root_fn, want):
        """{id(param): edges into its AccumulateGrad node} over the graph below ``root_fn`` (one edge per use of the leaf)."""
        counts, seen, stack = {}, set(), [root_fn]
        while stack:
            fn = stack.pop()
            if fn in seen:
                continue
            seen.add(fn)
            for nxt, _ in fn.next_functions:
                if nxt is None:
                    continue
                v = getattr(nxt, "variable", None)  # AccumulateGrad
                if v is not None:
                    if id(v) in want:
                        counts[id(v)] = counts.get(id(v), 0) + 1
                else:
                    stack.append(nxt)
        return counts

    uses = None

    def final(self, param):
        """Have all uses of ``param`` in this backward produced their gradient?  (True when uses are not tracked: the
        single-GPU step packs once, after the backward.)"""
        return self.uses is None or self.uses.get(id(param), 0) <= 0

    def backward_done(self):
        self.uses = None  # the backward has returned: whatever exists now is final

    def disarm(self):
        items, self.items, self.armed = self.items, {}, None
        self.uses = None
        return items

    def offer(self, param, slab_ptr, nparts, stride, numel, reduce_now, keep):
        """Called from a backward: returns the gradient to hand to autograd (None = deferred)."""
        if self.uses is not None and param is not None and id(param) in self.uses:
            self.uses[id(param)] -= 1
        if self.armed is None or param is None or id(param) not in self.armed:
            return reduce_now()
        first = self.items.pop(id(param), None)
        if first is not None:  # second use of this parameter in the step: both reduce now, autograd accumulates
            g1 = first["reduce_now"]()
            param.grad = g1 if param.grad is None else param.grad + g1
            self.armed.pop(id(param))  # no more deferral for it in this step
            return reduce_now()
        self.items[id(param)] = dict(param=param, src=slab_ptr, nparts=int(nparts), stride=int(stride), numel=int(numel),
                                     reduce_now=reduce_now, keep=keep)
        return None


deferred = DeferredGrads()


class StepFusion(object):
    """Cross-op state of ONE fused training step, armed by the trainers around ``model(x)`` + criterion.

    The reference's step ends with  y = sigmoid(...);  loss = BCELoss()(y, t);  loss.backward();  optimizer.step()
    (models/ranking/deepfm.py:43, trainers/ctr_trainer.py:88-99): five tiny launches here (head, BCE forward, BCE
    backward, Adam bias corrections, loader position) that are pure launch latency at B = 4096.  While a trainer has
    armed ``target`` (the labels of the batch), the output head also emits the per-block BCE terms, ``bce_mean`` on that
    very output finishes the mean inside ``rh_step_scalars`` -- the one single-block launch that also does the Adam
    bias corrections of the coming optimizer step and advances the registered device counters -- and the head's
    backward forms the BCE gradient inline.  Nothing changes numerically (same per-row arithmetic); any other use of
    the head's output (another criterion, no trainer) takes the unfused kernels."""

    def __init__(self):
        self.clear()

    def clear(self):
        self.target = None     # (B,) float32 labels the head may score against
        self.optimizer = None  # optim.TableAdam: its prepare() rides in rh_step_scalars
        self.counters = []     # [(int64 device tensor of one element, increment, modulus)]
        self.head = None       # dict(y_ptr, partial, t) of the head launch that computed BCE terms
        self.g_loss = None     # (1,) gradient of the loss, handed from the fused BCE backward to the head backward
        self.defer_scalars = False  # armed by a trainer whose backward follows the forward at once (train_step)
        self.pending = None    # scalar work a fused-BCE forward left to the chain's head backward (see _FusedBceFn)


fusion = StepFusion()


def _flush_pending_scalars():
    """A fused-BCE forward left its scalar work to a head backward that never ran (an abandoned step): run it now, so that
    the loader's position and the loss buffer are what they would have been."""
    pend, fusion.pending = fusion.pending, None
    if pend is not None:
        _lib.call("rh_step_scalars", _p(pend["partial"]), pend["partial"].numel(), pend["B"], _p(pend["loss"]), _p(None),
                  _p(None), _p(None), 0, *pend["flat"], _stream())


def fusion_begin(target=None, optimizer=None, counters=(), defer_scalars=False):
    _flush_pending_scalars()
    fusion.clear()
    fusion.defer_scalars = bool(defer_scalars)
    if target is not None and target.is_cuda and target.dtype == torch.float32 and target.dim() == 1 and \
            target.is_contiguous():
        fusion.target = target
    fusion.optimizer = optimizer
    fusion.counters = list(counters)


def fusion_end():
    """Disarm; returns the device counters nobody advanced (the caller launches rh_batch_advance for them)."""
    left = fusion.counters
    g, pend = fusion.g_loss, fusion.pending
    fusion.clear()
    fusion.g_loss = g  # the backward of this step has not run yet
    fusion.pending = pend  # ... and may carry the step's scalar work (_FusedBceFn, defer_scalars)
    return left


def advance_counters(counters):
    for t, inc, mod in counters:
        _lib.call("rh_batch_advance", _p(t), int(inc), int(mod), _stream())


class _HeadFn(torch.autograd.Function):
    """y = sigmoid(h w^T + b + e0 + e1): the MLP's Linear(K, 1), the wide / FM terms and the sigmoid in one launch each way."""

    @staticmethod
    def forward(ctx, h, weight, bias, e0, e1):
        require_hip(h, weight)
        if h.stride(1) != 1:
            h = h.contiguous()
        B, K = h.shape
        c0, c1 = _col(e0, B), _col(e1, B)
        y = torch.empty((B,), dtype=torch.float32, device=h.device)
        t = fusion.target
        ctx.fused_t = None
        if t is not None and t.numel() == B and t.device == h.device and B > 0 and any(ctx.needs_input_grad):
            partial = torch.empty((_lib.call("rh_head_loss_nblocks", B),), dtype=torch.float32, device=h.device)
            _lib.call("rh_head_loss_fwd", _p(h), h.stride(0), _p(weight), _p(bias), _p(c0), _p(c1), B, K, _p(y), _p(t),
                      _p(partial), _stream())
            fusion.head = dict(y_ptr=y.data_ptr(), partial=partial, t=t)
            ctx.fused_t = t
        else:
            _lib.call("rh_head_fwd", _p(h), h.stride(0), _p(weight), _p(bias), _p(c0), _p(c1), B, K, _p(y), _stream())
        ctx.save_for_backward(h, weight, y)
        ctx.shapes = (None if e0 is None else e0.shape, None if e1 is None else e1.shape, bias is not None)
        ctx.leaf_extra = _leaf_extra(e0, e1)
        ctx.params = (weight, bias)
        # h straight out of a BatchNorm1d + ReLU + Dropout layer (the MLP's last hidden layer): the backward below then
        # also forms that layer's BatchNorm-backward column sums (one statistics launch less per step)
        node = h.grad_fn
        ctx.bn_node = node if (node is not None and type(node).__name__ == "_BnReluDropoutFnBackward" and
                               FUSE_HEAD_BN) else None
        return y

    @staticmethod
    def backward(ctx, g_y):
        h, weight, y = ctx.saved_tensors
        s0, s1, has_bias = ctx.shapes
        B, K = h.shape
        dev = h.device
        g_h = torch.empty((B, K), dtype=torch.float32, device=dev)
        g_z = torch.empty((B,), dtype=torch.float32, device=dev)
        nblk = _lib.call("rh_head_nblocks", B)
        partial = torch.empty((nblk, K + 1), dtype=torch.float32, device=dev)
        wp, bp = ctx.params
        armed = deferred.armed
        defer = armed is not None and id(wp) in armed and (not has_bias or id(bp) in armed)
        g_w = None if defer else torch.empty_like(weight)
        g_b = torch.empty((1,), dtype=torch.float32, device=dev) if (has_bias and not defer) else None
        g_loss = fusion.g_loss
        t = gl = None
        if ctx.fused_t is not None and g_loss is not None and g_loss[1] == y.data_ptr():
            # y went into the fused BCE: that gradient is formed per row inside this launch.  The loss's backward
            # returned a persistent all-zero placeholder (which it keeps a reference to, so autograd cannot sum into it
            # in place): if g_y still IS that tensor the loss was the only consumer of y, otherwise g_y = 0 + the other
            # consumers' gradient and rides along
            fusion.g_loss = None
            t, gl = ctx.fused_t, g_loss[0]
            zero = g_loss[2]
            if g_y.data_ptr() == zero.data_ptr() and g_y._version == g_loss[3]:
                g_y = None
            else:
                g_y = g_y.contiguous()
        else:
            g_y = g_y.contiguous()
        bn = ctx.bn_node
        if bn is not None and K % 4 == 0 and K <= _lib.H.RH_HEAD_BN_MAX_K and nblk <= _lib.H.RH_BN_PRE_MAX_CHUNKS and h.stride(0) == K:
            z, gamma, beta, stat, saved_ctr = bn.saved_tensors
            bn_partial = torch.empty((nblk, 2, K), dtype=torch.float32, device=dev)
            _lib.call("rh_head_bwd_bn", _p(h), h.stride(0), _p(weight), _p(y), _p(g_y), _p(t), _p(gl), B, K, _p(g_h),
                      _p(g_z), _p(g_w), _p(g_b), _p(partial), 0 if defer else 1, _p(z), _p(stat), _p(gamma), _p(beta),
                      float(bn.p_drop), _p(_dropout_rng(dev)), _p(saved_ctr), 1 if bn.relu else 0, _p(bn_partial), _stream())
            # valid only if the layer's upstream gradient IS this g_h, unmodified: the tensor itself + its version
            bn.rh_pre = (g_h, g_h._version, bn_partial, nblk)
        else:
            _lib.call("rh_head_bwd_ex", _p(h), h.stride(0), _p(weight), _p(y), _p(g_y), _p(t), _p(gl), B, K, _p(g_h),
                      _p(g_z), _p(g_w), _p(g_b), _p(partial), 0 if defer else 1, _stream())
        if defer:
            g_w = deferred.offer(wp, partial.data_ptr(), nblk, K + 1, K, lambda: partial[:, :K].sum(0).view_as(weight),
                                 partial)
            if has_bias:
                g_b = deferred.offer(bp, partial.data_ptr() + 4 * K, nblk, K + 1, 1, lambda: partial[:, K].sum().view(1),
                                     partial)
        return (g_h, g_w, g_b) + _extra_grads(g_z, s0, s1, ctx.leaf_extra)


# Fused MLP chain (round 4): [Linear -> BatchNorm1d -> ReLU -> Dropout] x L -> Linear(., 1) (+ wide / FM terms)
# -> sigmoid of torch_rechub/basic/layers.py:276-292 + models/ranking/deepfm.py:39-43 as ONE autograd node over L + 1 forward
# launches and 3 L + 1 backward launches.  A/B switch for benchmarks: RECHUB_AB=chain=0 (tests flip the attribute).
FUSE_MLP_CHAIN = _lib.ab("chain")
# The chain's L weight gradients as ONE grouped launch behind its last input-gradient GEMM (A/B: RECHUB_AB=chainwgroup=0).
# Bit-equal to the per-layer launches (same body, same split plan).  Measured on the headline step, same box, 200 steps, two
# rounds: 0.2422 / 0.2424 -> 0.2411 / 0.2411 ms (profiles/r05_ab_chain_wgroup_same_box.txt): one launch less on a chain that is
# co-critical with the deferred sweep, so most of the 5 us it saves on the chain is not a shorter step.
CHAIN_WGRAD_GROUP = _lib.ab("chainwgroup")
chain_gate = None      # the gate words of the optimizer whose step-ahead graph is being captured (optim.TableAdam), or None
chain_gate_used = []   # ... and a mark per rh_linear_fwd_gate launch captured for it
# Round 6: while optim.TableAdam captures a step-ahead graph, the chain's grouped weight gradients are not launched where the
# backward produces them but handed to the optimizer, whose end-of-step launch carries them as its first workgroups
# (rh_adam_lazy_step_ahead_wgrad): nothing on the step's critical chain reads their slabs.  wgrad_rider(problems, B) -> True
# when the optimizer took them (it launches them itself if its step then ends differently: TableAdam._flush_rider).
wgrad_rider = None
wgrad_rider_flush = None  # the rider's owner launches what it holds NOW (whoever reads weight-gradient slabs calls flush_wgrad_rider)


def flush_wgrad_rider():
    """Weight gradients handed to the optimizer's end-of-step launch that has not run yet are launched on their own, now: called
    by everything that reads their slabs (the packing launches, an immediate reduction) -- a step whose packing launch comes
    BEFORE optimizer.step() (no dense-parameter Adam riding in it) must not read slabs that are still to be written."""
    f = wgrad_rider_flush
    if f is not None:
        f()


def _reset_capture_state():
    """chain_gate / chain_gate_used / wgrad_rider belong to ONE capture (optim.TableAdam arms them at the head of a step-ahead
    capture and disarms them at its last launch).  A capture that is abandoned in between must not leave them armed for
    whatever is captured next -- another trainer's MLP chain would bake rh_linear_fwd_gate with THIS optimizer's gate words
    into its graph, or hand its weight gradients to a launch that never comes (round-5 advisor finding)."""
    global chain_gate, wgrad_rider, wgrad_rider_flush
    chain_gate = None
    wgrad_rider = None
    wgrad_rider_flush = None
    del chain_gate_used[:]


from . import graphs as _graphs  # noqa: E402  (graphs imports torch only)

_graphs.capture_end_hooks.append(_reset_capture_state)
_CHAIN_MAX_K = min(_GEMM_MAX_NK, _lib.H.RH_LINEAR_BNACT_MAX_K)  # the tile GEMM's policy width and rh_linear_bnact_fwd's K limit
_CHAIN_MAX_B = 4096  # rh_head_bwd_bn hands over rh_head_nblocks(B) <= RH_BN_PRE_MAX_CHUNKS partial rows up to here


class _MlpChainFn(torch.autograd.Function):
    """y (B,) = sigmoid(head(hidden_L(... hidden_1(x))) + e0 + e1), hidden_l = Dropout(ReLU(BatchNorm1d(Linear_l(.)))) in
    training mode.  No hidden layer's BatchNorm / ReLU / Dropout runs as a pass of its own: the statistics are a by-product
    of the GEMM that produced the pre-activations (csrc/gemm.hip, STATS), the normalisation + activation + mask are applied
    where the NEXT layer (rh_linear_bnact_fwd) or the head (rh_head_bnact_fwd) reads them; in the backward the BatchNorm sums
    come from the head's backward (rh_head_bwd_bn, h = NULL) / the input-gradient GEMM's epilogue (rh_linear_dgrad_bnbwd).
    Saved for the backward: x, the pre-activations h_l, the activations a_l of all but the last hidden layer (written by the
    consuming GEMM for the weight gradient), per-layer (mean, rstd) and dropout counters, y.
    params = [W_l, b_l, gamma_l, beta_l] * L + [head_w, head_b]."""

    @staticmethod
    def forward(ctx, x, e0, e1, cfg, *params):
        bns, ps = cfg["bns"], cfg["p"]
        L = len(bns)
        require_hip(x, *[t for t in params if t is not None])
        B = x.shape[0]
        dev = x.device
        rng = _dropout_rng(dev)
        hs, stats, rows, ctrs, stat, acts = [], [], [], [], [], []
        inp = x
        for l in range(L):
            W, b, gamma, beta = params[4 * l:4 * l + 4]
            N, K = W.shape
            h = torch.empty((B, N), dtype=torch.float32, device=dev)
            r = _lib.call("rh_gemm_stats_rows", B, N) if l == 0 else _lib.call("rh_gemm_chain_stats_rows", B)
            st = torch.empty((-(-B // r), 2, N), dtype=torch.float32, device=dev)
            ctr = torch.empty(1, dtype=torch.int64, device=dev)
            if l == 0 and chain_gate is not None and torch.cuda.is_current_stream_capturing():
                # the first own GEMM of a step-ahead graph counts the chain start that releases the optimizer's deferred sweep
                # (optim.TableAdam sets ops.chain_gate while it captures such a step; csrc/optim.hip::stream_gate_kernel)
                _lib.call("rh_linear_fwd_gate", _p(inp), inp.stride(0), _p(W), K, _p(b), B, N, K, _p(h), N, _p(st), _p(rng),
                          _p(ctr), _p(bns[0].num_batches_tracked), _p(chain_gate), _stream())
                chain_gate_used.append(1)
            elif l == 0:
                _lib.call("rh_linear_fwd", _p(inp), inp.stride(0), _p(W), K, _p(b), B, N, K, _p(h), N, _p(st), _p(rng),
                          _p(ctr), _p(bns[0].num_batches_tracked), _stream())
            else:
                pb, pg, pbt = bns[l - 1], params[4 * (l - 1) + 2], params[4 * (l - 1) + 3]
                so = torch.empty((4, K), dtype=torch.float32, device=dev)
                act = torch.empty((B, K), dtype=torch.float32, device=dev)
                _lib.call("rh_linear_bnact_fwd", _p(hs[-1]), K, B, K, _p(stats[-1]), rows[-1], _p(pg), _p(pbt),
                          _p(pb.running_mean), _p(pb.running_var), float(pb.momentum), float(pb.eps), float(ps[l - 1]),
                          _p(rng), _p(ctrs[-1]), _p(so), _p(act), _p(W), K, _p(b), N, _p(h), N, _p(st), _p(rng), _p(ctr),
                          _p(bns[l].num_batches_tracked), _stream())
                stat.append(so)
                acts.append(act)
            hs.append(h)
            stats.append(st)
            rows.append(r)
            ctrs.append(ctr)
        hw, hb = params[4 * L], params[4 * L + 1]
        K = hs[-1].shape[1]
        lb, lg, lbt = bns[-1], params[4 * (L - 1) + 2], params[4 * (L - 1) + 3]
        so = torch.empty((4, K), dtype=torch.float32, device=dev)
        c0, c1 = _col(e0, B), _col(e1, B)
        y = torch.empty((B,), dtype=torch.float32, device=dev)
        t = fusion.target
        partial = None
        ctx.fused_t = None
        if t is not None and t.numel() == B and t.device == dev and any(ctx.needs_input_grad):
            partial = torch.empty((_lib.call("rh_head_loss_nblocks", B),), dtype=torch.float32, device=dev)
            ctx.fused_t = t
        _lib.call("rh_head_bnact_fwd", _p(hs[-1]), K, _p(stats[-1]), rows[-1], _p(lg), _p(lbt), _p(lb.running_mean),
                  _p(lb.running_var), float(lb.momentum), float(lb.eps), float(ps[-1]), _p(rng), _p(ctrs[-1]), _p(so), _p(hw),
                  _p(hb), _p(c0), _p(c1), B, K, _p(y), _p(ctx.fused_t), _p(partial), _stream())
        if ctx.fused_t is not None:
            fusion.head = dict(y_ptr=y.data_ptr(), partial=partial, t=t)
        stat.append(so)
        ctx.L, ctx.ps = L, [float(v) for v in ps]
        ctx.params = params  # the parameter objects themselves (ops.deferred keys gradients by identity)
        ctx.shapes = (None if e0 is None else e0.shape, None if e1 is None else e1.shape)
        ctx.leaf_extra = _leaf_extra(e0, e1)
        ctx.save_for_backward(x, y, *hs, *acts, *stat, *ctrs)
        return y

    @staticmethod
    def backward(ctx, g_y):
        L, ps, params = ctx.L, ctx.ps, ctx.params
        saved = ctx.saved_tensors
        x, y = saved[0], saved[1]
        hs = saved[2:2 + L]
        acts = saved[2 + L:2 + L + (L - 1)]
        stat = saved[2 + L + (L - 1):2 + L + (L - 1) + L]
        ctrs = saved[2 + L + (L - 1) + L:]
        B = x.shape[0]
        dev = x.device
        rng = _dropout_rng(dev)
        hw, hb = params[4 * L], params[4 * L + 1]
        K = hs[-1].shape[1]
        # ---- head: d loss / d y -> g of the last hidden layer's OUTPUT + that layer's BatchNorm-backward sums
        g_a = torch.empty((B, K), dtype=torch.float32, device=dev)
        g_z = torch.empty((B,), dtype=torch.float32, device=dev)
        nblk = _lib.call("rh_head_nblocks", B)
        partial = torch.empty((nblk, K + 1), dtype=torch.float32, device=dev)
        armed = deferred.armed
        has_bias = hb is not None
        defer = armed is not None and id(hw) in armed and (not has_bias or id(hb) in armed)
        g_w = None if defer else torch.empty_like(hw)
        g_b = torch.empty((1,), dtype=torch.float32, device=dev) if (has_bias and not defer) else None
        g_loss = fusion.g_loss
        t = gl = None
        if ctx.fused_t is not None and g_loss is not None and g_loss[1] == y.data_ptr():
            fusion.g_loss = None  # (see _HeadFn.backward: the fused BCE's gradient is formed per row inside the launch)
            t, gl = ctx.fused_t, g_loss[0]
            zero = g_loss[2]
            if g_y.data_ptr() == zero.data_ptr() and g_y._version == g_loss[3]:
                g_y = None
            else:
                g_y = g_y.contiguous()
        else:
            g_y = g_y.contiguous()
        bn_partial = torch.empty((nblk, 2, K), dtype=torch.float32, device=dev)
        pend = fusion.pending
        if pend is not None and pend["y_ptr"] == y.data_ptr():
            fusion.pending = None
            opt = pend["opt"]
            hyper = step = ring = None
            ring_size = 0
            if opt is not None and opt.can_fuse_prepare():
                hyper, step, ring, ring_size = opt.fuse_prepare()
            _lib.call("rh_head_bwd_bn_scalars", _p(None), K, _p(hw), _p(y), _p(g_y), _p(t), _p(gl), B, K, _p(g_a), _p(g_z),
                      _p(g_w), _p(g_b), _p(partial), 0 if defer else 1, _p(hs[-1]), _p(stat[-1]), _p(params[4 * (L - 1) + 2]),
                      _p(params[4 * (L - 1) + 3]), ps[-1], _p(rng), _p(ctrs[-1]), 1, _p(bn_partial), _p(pend["partial"]),
                      pend["partial"].numel(), _p(pend["loss"]), _p(hyper), _p(step), _p(ring), ring_size, *pend["flat"],
                      _stream())
        else:
            _lib.call("rh_head_bwd_bn", _p(None), K, _p(hw), _p(y), _p(g_y), _p(t), _p(gl), B, K, _p(g_a), _p(g_z), _p(g_w),
                      _p(g_b), _p(partial), 0 if defer else 1, _p(hs[-1]), _p(stat[-1]), _p(params[4 * (L - 1) + 2]),
                      _p(params[4 * (L - 1) + 3]), ps[-1], _p(rng), _p(ctrs[-1]), 1, _p(bn_partial), _stream())
        if defer:
            g_w = deferred.offer(hw, partial.data_ptr(), nblk, K + 1, K, lambda: partial[:, :K].sum(0).view_as(hw), partial)
            if has_bias:
                g_b = deferred.offer(hb, partial.data_ptr() + 4 * K, nblk, K + 1, 1, lambda: partial[:, K].sum().view(1),
                                     partial)
        grads = [None] * (4 * L + 2)
        grads[4 * L], grads[4 * L + 1] = g_w, g_b
        nchunks = nblk
        g_x = None
        # The L weight gradients depend on nothing later in this backward and nothing later depends on them (their slabs are
        # summed by the step's packing launch): with ops.deferred armed for every Linear of the chain they run as ONE
        # rh_linear_wgrad_partial_group launch behind the last input-gradient GEMM instead of one launch per layer between
        # the GEMMs -- same kernel body, same split plan per problem, hence the same slabs bit for bit.
        group = (CHAIN_WGRAD_GROUP and 2 <= L <= 8 and armed is not None and B < _lib.H.RH_WGRAD_LONG_MIN_B and
                 all(id(params[4 * l]) in armed and (params[4 * l + 1] is None or id(params[4 * l + 1]) in armed)
                     for l in range(L)))
        problems = []
        for l in range(L - 1, -1, -1):
            W, b, gamma, beta = params[4 * l:4 * l + 4]
            N, Kin = W.shape
            # BatchNorm + ReLU + Dropout backward of layer l from the sums its consumer formed: finalize + apply
            g_h = torch.empty((B, N), dtype=torch.float32, device=dev)
            dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(beta)
            _lib.call("rh_bn_relu_dropout_bwd_pre", _p(hs[l]), _p(g_a), B, N, _p(gamma), _p(beta), ps[l], _p(rng),
                      _p(ctrs[l]), _p(bn_partial), nchunks, _p(stat[l]), _p(g_h), _p(dgamma), _p(dbeta), 1, _stream())
            grads[4 * l + 2], grads[4 * l + 3] = dgamma, dbeta
            inp = acts[l - 1] if l > 0 else x
            if l > 0:
                r = _lib.call("rh_gemm_stats_rows", B, Kin)
                nchunks = -(-B // r)
                bn_partial = torch.empty((nchunks, 2, Kin), dtype=torch.float32, device=dev)
                g_a = torch.empty((B, Kin), dtype=torch.float32, device=dev)
                _lib.call("rh_linear_dgrad_bnbwd", _p(g_h), N, _p(W), Kin, B, N, Kin, _p(g_a), Kin, _p(hs[l - 1]), Kin,
                          _p(stat[l - 1]), _p(params[4 * (l - 1) + 2]), _p(params[4 * (l - 1) + 3]), ps[l - 1], _p(rng),
                          _p(ctrs[l - 1]), _p(bn_partial), _stream())
            elif ctx.needs_input_grad[0]:
                g_x = torch.empty((B, Kin), dtype=torch.float32, device=dev)
                _lib.call("rh_linear_dgrad", _p(g_h), N, _p(W), Kin, B, N, Kin, _p(g_x), Kin, _stream())
            if group:
                problems.append((l, g_h, inp, W, b))
            else:
                grads[4 * l], grads[4 * l + 1] = linear_wgrad(g_h, inp, want_bias=b is not None, weight=W, bias=b)
        if group:
            problems.reverse()  # layer 0 first: the widest problem's workgroups are dispatched first
            recs = []
            for l, g_h, inp, W, b in problems:
                N, Kin = W.shape
                part = torch.empty(_lib.call("rh_linear_wgrad_workspace", B, N, Kin), dtype=torch.float32, device=dev)
                recs.append((g_h, g_h.stride(0), inp, inp.stride(0), N, Kin, part))
            rider = wgrad_rider
            if not (rider is not None and rider(recs, B)):
                linear_wgrad_partial_group(recs, B)
            for (l, g_h, inp, W, b), rec in zip(problems, recs):
                grads[4 * l], grads[4 * l + 1] = _offer_wgrad_slabs(W, b, rec[6], B)
        s0, s1 = ctx.shapes
        return (g_x,) + _extra_grads(g_z, s0, s1, ctx.leaf_extra) + (None,) + tuple(grads)


def mlp_chain_ok(x, blocks, head, extras):
    """blocks = [(nn.Linear, nn.BatchNorm1d, p_drop)] of consecutive Linear -> BatchNorm1d -> ReLU -> Dropout layers in
    training mode, head = the closing nn.Linear(., 1): can _MlpChainFn run them?"""
    if not (FUSE_MLP_CHAIN and blocks and torch.is_grad_enabled() and x.is_cuda and x.dim() == 2 and
            x.dtype == torch.float32 and x.stride(1) == 1 and 2 <= x.shape[0] <= _CHAIN_MAX_B and len(extras) <= 2 and
            type(head) is torch.nn.Linear and head.out_features == 1 and head.weight.dtype == torch.float32 and
            all(e.numel() == x.shape[0] for e in extras)):
        return False
    width = x.shape[1]
    for lin, bn, p in blocks:
        if not (type(lin) is torch.nn.Linear and type(bn) is torch.nn.BatchNorm1d and bn.training and bn.affine and
                bn.track_running_stats and bn.momentum is not None and lin.in_features == width and
                lin.weight.is_contiguous() and lin.weight.dtype == torch.float32 and lin.out_features % 4 == 0 and
                lin.out_features <= _CHAIN_MAX_K and width <= _CHAIN_MAX_K and 0.0 <= p < 1.0 and linear_ok(x, lin.weight)):
            return False
        width = lin.out_features
    return (width <= _lib.H.RH_HEAD_BN_MAX_K and head.in_features == width and
            _lib.call("rh_head_nblocks", x.shape[0]) <= _lib.H.RH_BN_PRE_MAX_CHUNKS)


def mlp_chain_sigmoid(x, blocks, head, *extras):
    """sigmoid((head(hidden(x)) + sum(extras)).squeeze(1)) through _MlpChainFn; see mlp_chain_ok."""
    e = list(extras) + [None, None]
    cfg = {"bns": [bn for _, bn, _ in blocks], "p": [p for _, _, p in blocks]}
    params = []
    for lin, bn, _ in blocks:
        params += [lin.weight, lin.bias, bn.weight, bn.bias]
    return _MlpChainFn.apply(x, e[0], e[1], cfg, *params, head.weight, head.bias)


def head_ok(h, lin, extras):
    K = lin.in_features
    return (h.is_cuda and h.dim() == 2 and h.dtype == torch.float32 and lin.out_features == 1 and 1 <= K <= _lib.H.RH_HEAD_MAX_K and
            len(extras) <= 2 and h.shape[0] > 0 and all(e.numel() == h.shape[0] for e in extras))


def head_sigmoid(h, weight, bias, *extras):
    """sigmoid((h @ weight.T + bias + sum(extras)).squeeze(1)) -> (B,)"""
    e = list(extras) + [None, None]
    return _HeadFn.apply(h, weight, bias, e[0], e[1])


class _BceFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, y, t):
        require_hip(y, t)
        y, t = y.contiguous(), t.contiguous()
        loss = torch.empty((1,), dtype=torch.float32, device=y.device)
        _lib.call("rh_bce_fwd", _p(y), _p(t), y.numel(), _p(loss), _stream())
        ctx.save_for_backward(y, t)
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        y, t = ctx.saved_tensors
        g = g.contiguous().view(1)
        g_y = torch.empty_like(y)
        _lib.call("rh_bce_bwd", _p(y), _p(t), _p(g), y.numel(), _p(g_y), _stream())
        return g_y, None


def bce_ok(criterion, y, t):
    return (type(criterion) is torch.nn.BCELoss and criterion.reduction == "mean" and criterion.weight is None and
            y.is_cuda and y.dtype == torch.float32 and t.dtype == torch.float32 and y.dim() == 1 and
            y.shape == t.shape and 0 < y.numel() <= (1 << 22) and not t.requires_grad)


_zero_cache = {}


def _zero_placeholder(shape, dev):
    """A persistent, never-written all-zero float32 tensor per (shape, device) (no memset launch per step)."""
    key = (tuple(shape), str(dev))
    z = _zero_cache.get(key)
    if z is None:
        z = torch.zeros(shape, dtype=torch.float32, device=dev)
        if torch.cuda.is_current_stream_capturing():
            return z  # lives in the graph's pool, re-zeroed by the captured fill on every replay: not cached
        _zero_cache[key] = z
    return z


class _FusedBceFn(torch.autograd.Function):
    """Mean BCE of a head output whose per-block terms were computed by rh_head_loss_fwd: the forward is the step's
    ONE scalar launch (rh_step_scalars: mean of the terms + Adam bias corrections + device counters), the backward only
    hands the loss gradient to the head's backward (which forms dL/dy inline, rh_head_loss_bwd)."""

    @staticmethod
    def forward(ctx, y, t, partial):
        loss = torch.empty((1,), dtype=torch.float32, device=y.device)
        opt = fusion.optimizer
        cs = fusion.counters[:2]
        fusion.counters = fusion.counters[2:]
        flat = []
        for c, inc, mod in cs:
            flat += [_p(c), int(inc), int(mod)]
        while len(flat) < 6:
            flat += [_NULL, 0, 0]
        if fusion.defer_scalars and y.grad_fn is not None and y.grad_fn.__class__.__name__ == "_MlpChainFnBackward":
            # the chain's head backward carries this scalar work as one extra workgroup of its own launch (the loss value
            # is then written during the backward; the trainer that armed defer_scalars reads it only afterwards)
            fusion.pending = dict(partial=partial, B=y.numel(), loss=loss, flat=flat, y_ptr=y.data_ptr(), opt=opt,
                                  keep=[c for c, _, _ in cs])
        else:
            hyper = step = ring = None
            ring_size = 0
            if opt is not None and opt.can_fuse_prepare():
                hyper, step, ring, ring_size = opt.fuse_prepare()
            _lib.call("rh_step_scalars", _p(partial), partial.numel(), y.numel(), _p(loss), _p(hyper), _p(step), _p(ring),
                      ring_size, *flat, _stream())
        ctx.y_ptr = y.data_ptr()
        ctx.shape = y.shape
        ctx.dev = y.device
        return loss.view(())

    @staticmethod
    def backward(ctx, g):
        # dL/dy itself is formed inside the head's backward (from y, t and g); what goes back through autograd is a
        # persistent all-zero tensor, so a second consumer of y adds its gradient to 0 (and not to uninitialised memory)
        zero = _zero_placeholder(ctx.shape, ctx.dev)
        fusion.g_loss = (g.contiguous().view(1), ctx.y_ptr, zero, zero._version)
        return zero, None, None


def bce_mean(y, t):
    """torch.nn.BCELoss()(y, t) (mean reduction, log clamped at -100) in one launch each way; when ``y`` is the output
    of a head that already scored against ``t`` (StepFusion), the mean is finished by the step's scalar launch."""
    head = fusion.head
    if head is not None and head["y_ptr"] == y.data_ptr() and head["t"].data_ptr() == t.data_ptr() and \
            y.grad_fn is not None and y.grad_fn.__class__.__name__ in ("_HeadFnBackward", "_MlpChainFnBackward"):
        fusion.head = None
        return _FusedBceFn.apply(y, t, head["partial"])
    return _BceFn.apply(y, t)


# --------------------------------------------------------------------------------------------
class _DiceFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, alpha, eps):
        require_hip(x, alpha)
        if x.dim() != 2 or x.dtype != torch.float32:
            raise ValueError("Dice expects a float32 (N, num_neurons) tensor")
        x = x.contiguous()
        N, C = x.shape
        out = torch.empty_like(x)
        _lib.call("rh_dice_fwd", _p(x), _p(alpha), float(eps), N, C, _p(None), _p(None), _p(out), _stream())
        ctx.eps = float(eps)
        ctx.save_for_backward(x, alpha)
        return out

    @staticmethod
    def backward(ctx, g):
        x, alpha = ctx.saved_tensors
        N, C = x.shape
        g = g.contiguous()
        gx = torch.empty_like(x)
        partial = torch.empty(_lib.call("rh_dice_nblocks", N), dtype=torch.float32, device=x.device)
        _lib.call("rh_dice_bwd", _p(x), _p(g), _p(alpha), ctx.eps, N, C, _p(gx), _p(partial), _stream())
        return gx, partial.sum().reshape(1), None


def dice(x, alpha, eps):
    return _DiceFn.apply(x, alpha, eps)


class _PReluFn(torch.autograd.Function):
    """nn.PReLU() with one slope: one pass each way (csrc/din.hip); the slope gradient leaves as per-block partials
    (summed by the step's packing launch when the trainer armed ops.deferred for the parameter)."""

    @staticmethod
    def forward(ctx, x, weight):
        require_hip(x, weight)
        x = x.contiguous()
        out = torch.empty_like(x)
        _lib.call("rh_prelu_fwd", _p(x), _p(weight), x.numel(), _p(out), _stream())
        ctx.save_for_backward(x, weight)
        ctx.param = weight
        return out

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g = g.contiguous()
        gx = torch.empty_like(x)
        nb = _lib.call("rh_prelu_nblocks", x.numel())
        partial = torch.empty((nb,), dtype=torch.float32, device=x.device)
        _lib.call("rh_prelu_bwd", _p(x), _p(g), _p(weight), x.numel(), _p(gx), _p(partial), _stream())
        return gx, deferred.offer(ctx.param, partial.data_ptr(), nb, 1, 1, lambda: partial.sum().reshape(1), partial)


class _L2NormFn(torch.autograd.Function):
    """F.normalize(x, p=2, dim=1, eps): one launch each way (csrc/match.hip)."""

    @staticmethod
    def forward(ctx, x, eps):
        require_hip(x)
        if x.stride(1) != 1 or x.stride(0) % 4:
            x = x.contiguous()
        B, d = x.shape
        y = torch.empty((B, d), dtype=torch.float32, device=x.device)
        nrm = torch.empty((B,), dtype=torch.float32, device=x.device)
        _lib.call("rh_l2norm_fwd", _p(x), x.stride(0), B, d, float(eps), _p(y), _p(nrm), _stream())
        ctx.eps = float(eps)
        ctx.save_for_backward(y, nrm)
        return y

    @staticmethod
    def backward(ctx, g):
        y, nrm = ctx.saved_tensors
        B, d = y.shape
        if g.stride(1) != 1 or g.stride(0) % 4:
            g = g.contiguous()
        gx = torch.empty_like(y)
        _lib.call("rh_l2norm_bwd", _p(y), _p(nrm), _p(g), g.stride(0), B, d, ctx.eps, _p(gx), _stream())
        return gx, None


def l2_normalize_ok(x):
    return x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] > 0 and x.shape[1] % 4 == 0 and \
        _lib.H.RH_L2NORM_MIN_D <= x.shape[1] <= _lib.H.RH_L2NORM_MAX_D


def l2_normalize(x, eps=1e-12):
    """torch.nn.functional.normalize(x, p=2, dim=1, eps=eps) for a float32 (B, d) HIP tensor, d % 4 == 0."""
    return _L2NormFn.apply(x, eps)


class _CrossEntropyFn(torch.autograd.Function):
    """torch.nn.CrossEntropyLoss() (mean) over (B, C) logits, int64 targets (None = class 0 everywhere)."""

    @staticmethod
    def forward(ctx, logits, target):
        require_hip(logits)
        if target is not None and (target.dtype != torch.int64 or target.shape != (logits.shape[0],) or not target.is_cuda):
            raise ValueError("cross-entropy targets must be an int64 (B,) tensor on the device of the logits")
        logits = logits.contiguous()
        B, C = logits.shape
        dev = logits.device
        lse = torch.empty((B,), dtype=torch.float32, device=dev)
        nb = _lib.call("rh_ce_nblocks", B)
        partial = torch.empty((nb,), dtype=torch.float32, device=dev)
        _lib.call("rh_ce_fwd", _p(logits), _p(target), B, C, _p(lse), _p(partial), _p(err_flag(dev)), _stream())
        loss = torch.empty((1,), dtype=torch.float32, device=dev)
        _lib.call("rh_colsum", _p(partial), nb, 1, _p(loss), _NULL, 0, _NULL, _stream())
        ctx.save_for_backward(logits, lse) if target is None else ctx.save_for_backward(logits, lse, target)
        ctx.has_target = target is not None
        return (loss / B).view(())

    @staticmethod
    def backward(ctx, g):
        saved = ctx.saved_tensors
        logits, lse = saved[0], saved[1]
        target = saved[2] if ctx.has_target else None
        B, C = logits.shape
        gx = torch.empty_like(logits)
        _lib.call("rh_ce_bwd", _p(logits), _p(target), _p(lse), _p(g.contiguous().view(1)), B, C, _p(gx), _stream())
        return gx, None


def cross_entropy_ok(criterion, logits, target):
    return (type(criterion) is torch.nn.CrossEntropyLoss and criterion.reduction == "mean" and criterion.weight is None and
            criterion.label_smoothing == 0.0 and criterion.ignore_index == -100 and logits.is_cuda and
            logits.dtype == torch.float32 and logits.dim() == 2 and 1 <= logits.shape[1] <= _lib.H.RH_CE_MAX_C and logits.shape[0] > 0 and
            (target is None or (target.dtype == torch.int64 and target.shape == (logits.shape[0],) and target.is_cuda)))


def cross_entropy_mean(logits, target=None):
    return _CrossEntropyFn.apply(logits, None if target is None else target.contiguous())


def prelu_ok(mod, x):
    return (type(mod) is torch.nn.PReLU and mod.weight.numel() == 1 and x.is_cuda and x.dtype == torch.float32 and
            x.numel() >= 1)


def prelu(x, weight):
    return _PReluFn.apply(x, weight)


class _BnDiceFn(torch.autograd.Function):
    """Dice(BatchNorm1d(h)) with the normalisation folded into the Dice passes (csrc/din.hip, csrc/mlp.hip): the
    normalised tensor is never written.  Training mode; running statistics and num_batches_tracked updated in place."""

    @staticmethod
    def forward(ctx, h, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, bn_eps, alpha, eps,
                chunk_stats=None, chunk_rows=0):
        require_hip(h, gamma, beta, alpha)
        h = h.contiguous()
        N, C = h.shape
        dev = h.device
        stat = torch.empty((6, C), dtype=torch.float32, device=dev)
        if chunk_stats is not None:  # the producer of h already emitted per-chunk (sum, M2): no pass over h
            _lib.call("rh_bn_stats_from_partial", _p(chunk_stats), int(chunk_rows), N, C, _p(gamma), _p(beta),
                      _p(running_mean), _p(running_var), _p(num_batches_tracked), float(momentum), float(bn_eps), _p(stat),
                      _stream())
        else:
            partial = torch.empty((_lib.call("rh_bn_act_nchunks", N), 2, C), dtype=torch.float32, device=dev)
            _lib.call("rh_bn_stats_fwd", _p(h), N, C, _p(gamma), _p(beta), _p(running_mean), _p(running_var),
                      _p(num_batches_tracked), float(momentum), float(bn_eps), 1, _p(partial), _p(stat), _stream())
        out = torch.empty_like(h)
        _lib.call("rh_dice_fwd", _p(h), _p(alpha), float(eps), N, C, _p(stat[4]), _p(stat[5]), _p(out), _stream())
        ctx.eps = float(eps)
        ctx.save_for_backward(h, gamma, alpha, stat)
        return out

    @staticmethod
    def backward(ctx, g):
        h, gamma, alpha, stat = ctx.saved_tensors
        N, C = h.shape
        dev = h.device
        g = g.contiguous()
        nb = _lib.call("rh_bn_dice_stats_blocks", N)
        col_partial = torch.empty((nb, 2, C), dtype=torch.float32, device=dev)
        alpha_partial = torch.empty((nb,), dtype=torch.float32, device=dev)
        _lib.call("rh_bn_dice_bwd_stats", _p(h), _p(g), _p(alpha), ctx.eps, N, C, _p(stat), _p(gamma), _p(col_partial),
                  _p(alpha_partial), _stream())
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        d_alpha = torch.empty((1,), dtype=torch.float32, device=dev)
        # (the finalize launch also sums Dice's alpha partials: no framework reduction launch behind the apply pass)
        _lib.call("rh_bn_finalize_bwd_tail", _p(col_partial), nb, C, _p(stat), _p(dgamma), _p(dbeta), _p(None), _p(None),
                  _p(alpha_partial), 1, _p(d_alpha), _stream())
        dh = torch.empty_like(h)
        _lib.call("rh_bn_dice_bwd_apply", _p(h), _p(g), _p(alpha), ctx.eps, N, C, _p(stat), _p(gamma), _p(dh), _stream())
        return dh, dgamma, dbeta, None, None, None, None, None, d_alpha, None, None, None


def bn_dice_ok(h, bn, dice_mod):
    return (h.is_cuda and h.dim() == 2 and h.dtype == torch.float32 and h.shape[1] <= _lib.H.RH_BN_DICE_MAX_C and h.shape[0] > 1 and
            bn.affine and bn.track_running_stats and bn.momentum is not None)


def bn_dice(h, bn, alpha, eps, chunk_stats=None, chunk_rows=0):
    """Dice(bn(h)) for a Linear -> BatchNorm1d -> Dice block: folded into two passes over h (training) or one (eval).
    ``chunk_stats`` / ``chunk_rows``: per-chunk (sum, M2) of h from its producer (din_att_l1), replacing the statistics pass."""
    if bn.training:
        return _BnDiceFn.apply(h, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.momentum,
                               bn.eps, alpha, eps, chunk_stats, chunk_rows)
    require_hip(h)
    h = h.contiguous()
    N, C = h.shape
    stat = torch.empty((6, C), dtype=torch.float32, device=h.device)
    _lib.call("rh_bn_stats_fwd", _p(h), N, C, _p(bn.weight), _p(bn.bias), _p(bn.running_mean), _p(bn.running_var), _p(None),
              0.0, float(bn.eps), 0, _p(None), _p(stat), _stream())
    out = torch.empty_like(h)
    _lib.call("rh_dice_fwd", _p(h), _p(alpha), float(eps), N, C, _p(stat[4]), _p(stat[5]), _p(out), _stream())
    return out


class _BnDiceHeadFn(torch.autograd.Function):
    """Linear(C, 1)(Dice(BatchNorm1d(h))) -- the tail of the ActivationUnit's MLP (layers.py:281-288) -- without the Dice
    output: forward one pass over h writing (N, 1); backward two passes over h with the rank-1 gradient g[r] * w[c] formed in
    registers, the head's weight / bias gradients as per-block partials of the statistics pass (csrc/din.hip, HEAD)."""

    @staticmethod
    def forward(ctx, h, gamma, beta, running_mean, running_var, num_batches_tracked, momentum, bn_eps, alpha, eps, head_w,
                head_b, chunk_stats=None, chunk_rows=0):
        require_hip(h, gamma, beta, alpha, head_w)
        h = h.contiguous()
        N, C = h.shape
        dev = h.device
        stat = torch.empty((6, C), dtype=torch.float32, device=dev)
        if chunk_stats is not None:
            _lib.call("rh_bn_stats_from_partial", _p(chunk_stats), int(chunk_rows), N, C, _p(gamma), _p(beta),
                      _p(running_mean), _p(running_var), _p(num_batches_tracked), float(momentum), float(bn_eps), _p(stat),
                      _stream())
        else:
            partial = torch.empty((_lib.call("rh_bn_act_nchunks", N), 2, C), dtype=torch.float32, device=dev)
            _lib.call("rh_bn_stats_fwd", _p(h), N, C, _p(gamma), _p(beta), _p(running_mean), _p(running_var),
                      _p(num_batches_tracked), float(momentum), float(bn_eps), 1, _p(partial), _p(stat), _stream())
        head_w = head_w.contiguous()
        out = torch.empty((N, 1), dtype=torch.float32, device=dev)
        _lib.call("rh_bn_dice_head_fwd", _p(h), _p(alpha), float(eps), N, C, _p(stat[4]), _p(stat[5]), _p(head_w),
                  _p(head_b), _p(out), _stream())
        ctx.eps = float(eps)
        ctx.has_bias = head_b is not None
        ctx.save_for_backward(h, gamma, alpha, stat, head_w)
        return out

    @staticmethod
    def backward(ctx, g):
        h, gamma, alpha, stat, head_w = ctx.saved_tensors
        N, C = h.shape
        dev = h.device
        g = g.contiguous()
        nb = _lib.call("rh_bn_dice_stats_blocks", N)
        col_partial = torch.empty((nb, 2, C), dtype=torch.float32, device=dev)
        scalar_partial = torch.empty((2, nb), dtype=torch.float32, device=dev)
        head_partial = torch.empty((nb, C), dtype=torch.float32, device=dev)
        _lib.call("rh_bn_dice_head_bwd_stats", _p(h), _p(g), _p(alpha), ctx.eps, N, C, _p(stat), _p(gamma), _p(head_w),
                  _p(col_partial), _p(scalar_partial), _p(head_partial), _stream())
        dgamma, dbeta = torch.empty_like(gamma), torch.empty_like(gamma)
        scalars = torch.empty((2,), dtype=torch.float32, device=dev)
        d_head_w = torch.empty((1, C), dtype=torch.float32, device=dev)
        # (the finalize launch also sums the head's weight-gradient partials and the two scalar rows -- Dice's alpha, the head's
        # bias: three framework reduction launches + a fill per attention unit less on the backward's critical path)
        _lib.call("rh_bn_finalize_bwd_tail", _p(col_partial), nb, C, _p(stat), _p(dgamma), _p(dbeta), _p(head_partial),
                  _p(d_head_w), _p(scalar_partial), 2, _p(scalars), _stream())
        dh = torch.empty_like(h)
        _lib.call("rh_bn_dice_head_bwd_apply", _p(h), _p(g), _p(alpha), ctx.eps, N, C, _p(stat), _p(gamma), _p(head_w),
                  _p(dh), _stream())
        return (dh, dgamma, dbeta, None, None, None, None, None, scalars[0:1], None, d_head_w,
                scalars[1:2] if ctx.has_bias else None, None, None)


def bn_dice_head_ok(h_cols, bn, dice_mod, lin):
    return (type(lin) is torch.nn.Linear and lin.out_features == 1 and lin.in_features == h_cols and h_cols <= _lib.H.RH_BN_DICE_MAX_C and
            lin.weight.dtype == torch.float32 and FUSE_DICE_HEAD)


def bn_dice_head(h, bn, alpha, eps, lin, chunk_stats=None, chunk_rows=0):
    """lin(Dice(bn(h))) for Linear -> BatchNorm1d -> Dice -> Linear(C, 1); (N, 1)."""
    if bn.training:
        return _BnDiceHeadFn.apply(h, bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                   bn.momentum, bn.eps, alpha, eps, lin.weight, lin.bias, chunk_stats, chunk_rows)
    require_hip(h)
    h = h.contiguous()
    N, C = h.shape
    stat = torch.empty((6, C), dtype=torch.float32, device=h.device)
    _lib.call("rh_bn_stats_fwd", _p(h), N, C, _p(bn.weight), _p(bn.bias), _p(bn.running_mean), _p(bn.running_var), _p(None),
              0.0, float(bn.eps), 0, _p(None), _p(stat), _stream())
    out = torch.empty((N, 1), dtype=torch.float32, device=h.device)
    _lib.call("rh_bn_dice_head_fwd", _p(h), _p(alpha), float(eps), N, C, _p(stat[4]), _p(stat[5]),
              _p(lin.weight.detach().contiguous()), _p(None if lin.bias is None else lin.bias.detach()), _p(out), _stream())
    return out


def _hist_layout(history):
    """(B, L, D) view whose rows are contiguous over (L, D); returns (tensor, batch stride in floats)."""
    if history.stride(2) != 1 or history.stride(1) != history.shape[2]:
        history = history.contiguous()
    return history, history.stride(0)


class _AttInputFn(torch.autograd.Function):
    """cat[t, h, t-h, t*h] over (B*L, 4D) without the expand / sub / mul / cat temporaries."""

    @staticmethod
    def forward(ctx, history, target):
        require_hip(history, target)
        history, hs = _hist_layout(history)
        if target.stride(1) != 1:
            target = target.contiguous()
        B, L, D = history.shape
        out = torch.empty((B * L, 4 * D), dtype=torch.float32, device=history.device)
        _lib.call("rh_din_att_input_fwd", _p(history), hs, _p(target), target.stride(0), B, L, D, _p(out), _stream())
        ctx.save_for_backward(history, target)
        return out

    @staticmethod
    def backward(ctx, g):
        history, target = ctx.saved_tensors
        B, L, D = history.shape
        g = g.contiguous()
        g_hist = torch.empty((B, L, D), dtype=torch.float32, device=g.device)
        g_tgt = torch.empty((B, D), dtype=torch.float32, device=g.device)
        _lib.call("rh_din_att_input_bwd", _p(history), history.stride(0), _p(target), target.stride(0), _p(g), B, L, D,
                  _p(g_hist), _p(g_tgt), _stream())
        return g_hist, g_tgt


class _AttPoolFn(torch.autograd.Function):
    """(att_weight.unsqueeze(-1) * history).sum(dim=1)."""

    @staticmethod
    def forward(ctx, weight, history):
        require_hip(weight, history)
        history, hs = _hist_layout(history)
        weight = weight.contiguous()
        B, L, D = history.shape
        out = torch.empty((B, D), dtype=torch.float32, device=history.device)
        _lib.call("rh_din_pool_fwd", _p(history), hs, _p(weight), B, L, D, _p(out), _stream())
        ctx.save_for_backward(weight, history)
        return out

    @staticmethod
    def backward(ctx, g):
        weight, history = ctx.saved_tensors
        B, L, D = history.shape
        g = g.contiguous()
        g_hist = torch.empty((B, L, D), dtype=torch.float32, device=g.device)
        g_w = torch.empty((B, L), dtype=torch.float32, device=g.device)
        _lib.call("rh_din_pool_bwd", _p(history), history.stride(0), _p(weight), _p(g), B, L, D, _p(g_hist), _p(g_w),
                  _stream())
        return g_w, g_hist


class _AttL1Fn(torch.autograd.Function):
    """z (B*L, N) = [t, h, t-h, t*h] W^T + b with the operand built in registers (csrc/dinmlp.hip) and, when asked, the
    per-chunk BatchNorm statistics of z as an epilogue.  Backward: the operand is rebuilt once (rh_din_att_input_fwd) for
    the split-batch weight gradient; input gradient = library GEMM + rh_din_att_input_bwd."""

    @staticmethod
    def forward(ctx, history, target, weight, bias, want_stats):
        require_hip(history, target, weight)
        history, hs = _hist_layout(history)
        if target.stride(1) != 1:
            target = target.contiguous()
        weight_c = weight.contiguous()
        B, L, D = history.shape
        N = weight.shape[0]
        dev = history.device
        z = torch.empty((B * L, N), dtype=torch.float32, device=dev)
        partial = None
        if want_stats:
            rows = _lib.call("rh_din_att_l1_chunk_rows", B * L)
            partial = torch.empty((-(-(B * L) // rows), 2, N), dtype=torch.float32, device=dev)
        _lib.call("rh_din_att_l1_fwd", _p(history), hs, _p(target), target.stride(0), _p(weight_c),
                  _p(None if bias is None else bias.contiguous()), B, L, D, N, _p(z), _p(partial), _stream())
        ctx.save_for_backward(history, target, weight_c)
        ctx.params = (weight, bias)
        if partial is None:
            return z, None
        ctx.mark_non_differentiable(partial)
        return z, partial

    @staticmethod
    def backward(ctx, g, _unused):
        history, target, weight = ctx.saved_tensors
        B, L, D = history.shape
        wp, bp = ctx.params
        g = g.contiguous()
        dev = g.device
        dW = db = None
        if ctx.needs_input_grad[2] or (bp is not None and ctx.needs_input_grad[3]):
            att = torch.empty((B * L, 4 * D), dtype=torch.float32, device=dev)
            _lib.call("rh_din_att_input_fwd", _p(history), history.stride(0), _p(target), target.stride(0), B, L, D, _p(att),
                      _stream())
            dW, db = linear_wgrad(g, att, want_bias=bp is not None, weight=wp, bias=bp)
        g_hist = g_tgt = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            # (B*L, N) x (N, 4D): the tile kernel of csrc/gemm.hip runs this tall, narrow-output product at 184 us against
            # the library's 260 us at configs[3] (tools/gemm_tall_probe.py)
            g_att = torch.empty((B * L, 4 * D), dtype=torch.float32, device=dev)
            _lib.call("rh_linear_dgrad", _p(g), g.stride(0), _p(weight), 4 * D, B * L, weight.shape[0], 4 * D, _p(g_att),
                      4 * D, _stream())
            g_hist = torch.empty((B, L, D), dtype=torch.float32, device=dev)
            g_tgt = torch.empty((B, D), dtype=torch.float32, device=dev)
            _lib.call("rh_din_att_input_bwd", _p(history), history.stride(0), _p(target), target.stride(0), _p(g_att), B, L,
                      D, _p(g_hist), _p(g_tgt), _stream())
        return g_hist, g_tgt, dW, db, None


def din_att_l1_ok(history, target, lin):
    return (history.is_cuda and history.dtype == torch.float32 and history.dim() == 3 and history.shape[0] >= 1 and
            type(lin) is torch.nn.Linear and lin.in_features == 4 * history.shape[2] and
            _lib.call("rh_din_att_l1_supported", history.shape[2], lin.out_features) == 1)


def din_att_l1(history, target, weight, bias, want_stats):
    """(z, chunk_stats | None): the ActivationUnit's first Linear on the never-materialised [t, h, t-h, t*h] operand."""
    return _AttL1Fn.apply(history, target, weight, bias, want_stats)


def din_att_input(history, target):
    return _AttInputFn.apply(history, target)


def din_att_pool(weight, history):
    return _AttPoolFn.apply(weight, history)


def din_dim_ok(d):
    q = d // 4
    return d % 4 == 0 and 4 <= d <= _lib.H.RH_DIN_ATT_MAX_D and (q & (q - 1)) == 0


# --------------------------------------------------------------------------------------------
class _CrossV2Epilogue(torch.autograd.Function):
    """out = x0 * y + b + x  (y = W_l x): Hadamard + bias + residual of one CrossNetV2 layer in one pass."""

    @staticmethod
    def forward(ctx, x0, y, b, x):
        require_hip(x0, y, b, x)
        x0, y, b, x = x0.contiguous(), y.contiguous(), b.contiguous(), x.contiguous()
        B, d = x.shape
        out = torch.empty_like(x)
        _lib.call("rh_cross_v2_epilogue_fwd", _p(x0), _p(y), _p(b), _p(x), B, d, _p(out), _stream())
        ctx.save_for_backward(x0, y)
        return out

    @staticmethod
    def backward(ctx, g):
        x0, y = ctx.saved_tensors
        B, d = x0.shape
        g = g.contiguous()
        g_x0 = torch.empty_like(x0)
        g_y = torch.empty_like(y)
        _lib.call("rh_cross_v2_epilogue_bwd", _p(x0), _p(y), _p(g), B, d, _p(g_x0), _p(g_y), _stream())
        return g_x0, g_y, g.sum(0), g


def cross_v2_epilogue(x0, y, b, x):
    return _CrossV2Epilogue.apply(x0, y, b, x)


class _CrossV2LayerFn(torch.autograd.Function):
    """out = x0 * (x W^T) + b + x: ONE CrossNetV2 layer (torch_rechub/basic/layers.py:440-444) as one launch each for the
    forward (rh_cross_v2_fwd: tile GEMM whose epilogue is the Hadamard + bias + residual) and the input gradient
    (rh_cross_v2_dgrad: g_y W + g), plus rh_cross_v2_epilogue_bwd (g_x0 = g * y, g_y = g * x0) and the split-batch weight
    gradient.  Round 5; before: library GEMM + epilogue pass forward, epilogue pass + two library products + autograd's residual
    add backward."""

    @staticmethod
    def forward(ctx, x0, x, weight, bias):
        require_hip(x0, x, weight, bias)
        x0, x = x0.contiguous(), x.contiguous()
        B, d = x.shape
        y = torch.empty_like(x)
        out = torch.empty_like(x)
        _lib.call("rh_cross_v2_fwd", _p(x0), _p(x), _p(weight), _p(bias), B, d, _p(y), _p(out), _stream())
        ctx.save_for_backward(x0, x, y, weight)
        ctx.params = (weight, bias)
        return out

    @staticmethod
    def backward(ctx, g):
        x0, x, y, weight = ctx.saved_tensors
        B, d = x.shape
        g = g.contiguous()
        g_x0 = torch.empty_like(x0)
        g_y = torch.empty_like(y)
        _lib.call("rh_cross_v2_epilogue_bwd", _p(x0), _p(y), _p(g), B, d, _p(g_x0), _p(g_y), _stream())
        g_x = None
        if ctx.needs_input_grad[1]:
            g_x = torch.empty_like(x)
            _lib.call("rh_cross_v2_dgrad", _p(g_y), _p(weight), _p(g), B, d, _p(g_x), _stream())
        g_w = None
        if ctx.needs_input_grad[2]:
            g_w, _ = linear_wgrad(g_y, x, want_bias=False, weight=ctx.params[0])
        g_b = g.sum(0) if ctx.needs_input_grad[3] else None
        return (g_x0 if ctx.needs_input_grad[0] else None), g_x, g_w, g_b


def cross_v2_shape_ok(x, weight):
    """THE predicate of the fused CrossNetV2 layer (ops.cross_v2_layer_ok and torch.ops.rechub_hip.cross_net_v2 share it):
    contiguous f32 x (B, d) and W (d, d) within the entry points' limits."""
    return (x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and weight.dtype == torch.float32 and
            1 <= x.shape[0] <= _lib.H.RH_CROSS_V2_MAX_M and 1 <= x.shape[1] <= _lib.H.RH_CROSS_V2_MAX_D and
            tuple(weight.shape[-2:]) == (x.shape[1], x.shape[1]))


def cross_v2_layer_ok(x, lin):
    """Can one CrossNetV2 layer run on the tile GEMM (f32, square weight without bias up to the GEMM's widths)?"""
    return (type(lin) is torch.nn.Linear and lin.bias is None and x.dim() == 2 and cross_v2_shape_ok(x, lin.weight) and
            x.shape[1] <= _GEMM_MAX_NK and lin.weight.is_contiguous() and linear_ok(x, lin.weight))


def cross_v2_layer(x0, x, weight, bias):
    return _CrossV2LayerFn.apply(x0, x, weight, bias)


class _CrossMixEpilogue(torch.autograd.Function):
    """out = sum_e gate_e * x0 * (uv_e + bias) + xl: bias + Hadamard + gated expert mix + residual in one pass."""

    @staticmethod
    def forward(ctx, x0, xl, uv, gate, bias):
        require_hip(x0, xl, uv, gate, bias)
        ctx.bias_param, ctx.bias_shape = bias, bias.shape  # the (d, 1) / (d,) parameter itself (ops.deferred keys by identity)
        x0, xl, uv, gate = x0.contiguous(), xl.contiguous(), uv.contiguous(), gate.contiguous()
        bias = bias.reshape(-1).contiguous()
        E, B, d = uv.shape
        out = torch.empty_like(x0)
        _lib.call("rh_cross_mix_epilogue_fwd", _p(x0), _p(xl), _p(uv), _p(gate), _p(bias), B, d, E, _p(out), _stream())
        ctx.save_for_backward(x0, uv, gate, bias)
        return out

    @staticmethod
    def backward(ctx, g):
        x0, uv, gate, bias = ctx.saved_tensors
        E, B, d = uv.shape
        g = g.contiguous()
        g_x0 = torch.empty_like(x0)
        g_uv = torch.empty_like(uv)
        g_gate = torch.empty_like(gate)
        nblk = _lib.call("rh_cross_mix_nblocks", B)
        partial = torch.empty((nblk, d), dtype=torch.float32, device=g.device)
        _lib.call("rh_cross_mix_epilogue_bwd_b", _p(x0), _p(uv), _p(gate), _p(bias), _p(g), B, d, E, _p(g_x0), _p(g_uv),
                  _p(g_gate), _p(partial), _stream())
        # d/d bias = sum_b g x0 sum_e gate_e: per-block partial rows from the same pass (was 2 multiplies + 2 reductions)
        shape = ctx.bias_shape
        g_bias = deferred.offer(ctx.bias_param, partial.data_ptr(), nblk, d, d, lambda: partial.sum(0).view(shape), partial)
        return g_x0, g, g_uv, g_gate, g_bias


def cross_mix_epilogue(x0, xl, uv, gate, bias):
    return _CrossMixEpilogue.apply(x0, xl, uv, gate, bias)


# --------------------------------------------------------------------------------------------
def _ptr_array(tensors):
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _int_array(values):
    import ctypes
    return (ctypes.c_int * len(values))(*values)


def cross_moe_ok(x, L, E, d, r):
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 2 and x.shape[0] >= 1 and x.stride(1) == 1 and
            _lib.call("rh_cross_moe_supported", L, E, d, r) == 1)


class _CrossMoeFn(torch.autograd.Function):
    """CrossNetMix.forward (reference basic/layers.py:470-506) for ALL its layers: per layer two library GEMMs
    (B, d) x (d, KP) and (B, KP) x (KP, d), the mid pass between them and one addcmul (csrc/moe.hip); the backward is two
    GEMMs + two split-batch weight-gradient launches + two fused passes per layer, and ONE launch that turns the
    weight-gradient slabs of all layers into the gradients of u_list / v_list / c_list / bias / gating.

    inputs: x, then L x U, L x V, L x C, L x bias, E x gating weight."""

    @staticmethod
    def forward(ctx, x, L, E, *params):
        import ctypes
        require_hip(x, *params)
        U, V, C, bias, Wg = (params[0:L], params[L:2 * L], params[2 * L:3 * L], params[3 * L:4 * L], params[4 * L:4 * L + E])
        B, d = x.shape
        r = U[0].shape[2]
        KP = _lib.call("rh_cross_moe_kp", E, r)
        dev = x.device
        cont = [t.contiguous() for t in params]
        Uc, Vc, Cc, bc, Wgc = cont[0:L], cont[L:2 * L], cont[2 * L:3 * L], cont[3 * L:4 * L], cont[4 * L:4 * L + E]
        VgT = torch.empty((L, KP, d), dtype=torch.float32, device=dev)
        UTb = torch.empty((L, d, KP), dtype=torch.float32, device=dev)
        _lib.call("rh_cross_moe_pack", ctypes.cast(_ptr_array(Uc), ctypes.c_void_p), ctypes.cast(_ptr_array(Vc), ctypes.c_void_p),
                  ctypes.cast(_ptr_array(bc), ctypes.c_void_p), ctypes.cast(_ptr_array(Wgc), ctypes.c_void_p), L, E, d, r,
                  _p(VgT), _p(UTb), _stream())
        xl, saved = x, []
        for l in range(L):
            PG = torch.mm(xl, VgT[l].t())
            v1 = torch.empty((B, E * r), dtype=torch.float32, device=dev)
            v2 = torch.empty_like(v1)
            gate = torch.empty((B, E), dtype=torch.float32, device=dev)
            wp = torch.empty((B, KP), dtype=torch.float32, device=dev)
            _lib.call("rh_cross_moe_mid_fwd", _p(PG), _p(Cc[l]), B, E, r, _p(v1), _p(v2), _p(gate), _p(wp), _stream())
            Y = torch.mm(wp, UTb[l].t())
            nxt = torch.addcmul(xl, x, Y)
            saved += [xl, v1, v2, gate, wp, Y]
            xl = nxt
        ctx.dims = (L, E, B, d, r, KP)
        ctx.shapes = [t.shape for t in params]
        ctx.save_for_backward(x, VgT, UTb, *Cc, *saved)
        return xl

    @staticmethod
    def backward(ctx, G):
        import ctypes
        L, E, B, d, r, KP = ctx.dims
        x, VgT, UTb = ctx.saved_tensors[:3]
        Cc = ctx.saved_tensors[3:3 + L]
        saved = ctx.saved_tensors[3 + L:]
        dev = x.device
        if G.stride(1) != 1:
            G = G.contiguous()
        acc = torch.empty((B, d), dtype=torch.float32, device=dev)  # running gradient of x0
        nb = _lib.call("rh_cross_moe_mid_blocks", B, E, r)
        s1 = _lib.call("rh_linear_wgrad_splits", B, KP, d)
        s2 = _lib.call("rh_linear_wgrad_splits", B, d, KP)
        ws1 = _lib.call("rh_linear_wgrad_workspace", B, KP, d)
        ws2 = _lib.call("rh_linear_wgrad_workspace", B, d, KP)
        slabV, slabU, gC = [], [], []
        # The two weight gradients of a layer (g_UTb = g_Y^T wp, g_VgT = g_PG^T x_l) feed nothing but the final unpack: they
        # are collected and run as grouped launches of <= 8 problems after the loop (round 4: 2 L launches of ~16.5 us -> 1)
        group = WGRAD_GROUP and B < _lib.H.RH_WGRAD_LONG_MIN_B
        problems = []
        own_G = False
        for l in reversed(range(L)):
            xl, v1, v2, gate, wp, Y = saved[6 * l:6 * l + 6]
            g_Y = torch.empty((B, d), dtype=torch.float32, device=dev)
            # (l == 0: acc also takes G, the closing product below accumulates into it -- that IS the gradient of x)
            _lib.call("rh_cross_moe_res_bwd", _p(G), G.stride(0), _p(x), x.stride(0), _p(Y), B, d,
                      (1 if l == L - 1 else 0) | (2 if l == 0 else 0), _p(g_Y), _p(acc), _stream())
            pu = torch.empty((ws2,), dtype=torch.float32, device=dev)  # g_UTb (d, KP) = g_Y^T wp
            if group:
                problems.append((g_Y, d, wp, KP, d, KP, pu))
            else:
                _lib.call("rh_linear_wgrad_partial", _p(g_Y), d, _p(wp), KP, B, d, KP, _p(pu), _stream())
            g_wp = torch.mm(g_Y, UTb[l])
            g_PG = torch.empty((B, KP), dtype=torch.float32, device=dev)
            pc = torch.empty((nb, E * r * r), dtype=torch.float32, device=dev)
            _lib.call("rh_cross_moe_mid_bwd", _p(g_wp), _p(v1), _p(v2), _p(gate), _p(Cc[l]), B, E, r, _p(g_PG), _p(pc),
                      _stream())
            pv = torch.empty((ws1,), dtype=torch.float32, device=dev)  # g_VgT (KP, d) = g_PG^T x_l
            if group:
                problems.append((g_PG, KP, xl, xl.stride(0), KP, d, pv))
            else:
                _lib.call("rh_linear_wgrad_partial", _p(g_PG), KP, _p(xl), xl.stride(0), B, KP, d, _p(pv), _stream())
            # gradient of x_l: residual + through the first product.  Only the first of the backward copies (the incoming
            # gradient is not ours to overwrite); the others accumulate in place, the last one into acc
            if l == 0:
                g_x = acc.addmm_(g_PG, VgT[l])  # x is both x_0 (Hadamard factor of every layer) and the first x_l
            elif own_G:
                G.addmm_(g_PG, VgT[l])
            else:
                G, own_G = torch.addmm(G, g_PG, VgT[l]), True
            slabV.append(pv), slabU.append(pu), gC.append(pc)
        for i in range(0, len(problems), 8):
            linear_wgrad_partial_group(problems[i:i + 8], B)
        slabV.reverse(), slabU.reverse(), gC.reverse()
        g_U = [torch.empty(ctx.shapes[l], dtype=torch.float32, device=dev) for l in range(L)]
        g_V = [torch.empty(ctx.shapes[L + l], dtype=torch.float32, device=dev) for l in range(L)]
        g_C = [torch.empty(ctx.shapes[2 * L + l], dtype=torch.float32, device=dev) for l in range(L)]
        g_b = [torch.empty(ctx.shapes[3 * L + l], dtype=torch.float32, device=dev) for l in range(L)]
        g_W = [torch.empty(ctx.shapes[4 * L + e], dtype=torch.float32, device=dev) for e in range(E)]
        cast = lambda arr: ctypes.cast(arr, ctypes.c_void_p)
        _lib.call("rh_cross_moe_unpack", cast(_ptr_array(slabV)), cast(_int_array([s1] * L)), cast(_ptr_array(slabU)),
                  cast(_int_array([s2] * L)), cast(_ptr_array(gC)), cast(_int_array([nb] * L)), L, E, d, r,
                  cast(_ptr_array(g_U)), cast(_ptr_array(g_V)), cast(_ptr_array(g_b)), cast(_ptr_array(g_C)),
                  cast(_ptr_array(g_W)), _stream())
        return (g_x, None, None) + tuple(g_U) + tuple(g_V) + tuple(g_C) + tuple(g_b) + tuple(g_W)


WGRAD_GROUP = _lib.ab("wgroup")  # False (RECHUB_AB=wgroup=0, tests): one rh_linear_wgrad_partial launch per problem


def wgrad_group_args(problems, B):
    """The nine array arguments of a grouped weight-gradient launch (n, g, ldg, x, ldx, B, N, K, partial) + what must stay
    alive until the call returns.  problems = [(g (B, N), ldg, x (B, K), ldx, N, K, partial workspace)]."""
    import ctypes
    n = len(problems)
    g = (ctypes.c_void_p * n)(*[p_[0].data_ptr() for p_ in problems])
    ldg = (ctypes.c_int64 * n)(*[int(p_[1]) for p_ in problems])
    x = (ctypes.c_void_p * n)(*[p_[2].data_ptr() for p_ in problems])
    ldx = (ctypes.c_int64 * n)(*[int(p_[3]) for p_ in problems])
    Bs = (ctypes.c_int * n)(*[int(B)] * n)
    Ns = (ctypes.c_int * n)(*[int(p_[4]) for p_ in problems])
    Ks = (ctypes.c_int * n)(*[int(p_[5]) for p_ in problems])
    part = (ctypes.c_void_p * n)(*[p_[6].data_ptr() for p_ in problems])
    cast = lambda a: ctypes.cast(a, ctypes.c_void_p)
    return (n, cast(g), cast(ldg), cast(x), cast(ldx), cast(Bs), cast(Ns), cast(Ks), cast(part)), (g, ldg, x, ldx, Bs, Ns, Ks, part)


def linear_wgrad_partial_group(problems, B):
    """ONE launch for <= 8 independent weight-gradient problems (g (B, N) ld, x (B, K) ld, N, K, partial workspace)."""
    args, keep = wgrad_group_args(problems, B)
    _lib.call("rh_linear_wgrad_partial_group", *args, _stream())
    del keep


def cross_moe(x, u_list, v_list, c_list, bias_list, gating_weights):
    """The whole CrossNetMix stack (all layers) through csrc/moe.hip; check ``cross_moe_ok`` first."""
    L, E = len(u_list), len(gating_weights)
    return _CrossMoeFn.apply(x, L, E, *u_list, *v_list, *c_list, *bias_list, *gating_weights)


# --------------------------------------------------------------------------------------------
class _AugruFn(torch.autograd.Function):
    """h_all (B, T, D) = gated recurrence over xw (B, T, 3D), attn (B, T) | None, U (D, 3D), state_bias (3D) | None
    (csrc/augru.hip)."""

    @staticmethod
    def forward(ctx, xw, attn, U, ub):
        require_hip(xw, U)
        B, T, D3 = xw.shape
        D = D3 // 3
        xw, U = xw.contiguous(), U.contiguous()
        attn = None if attn is None else attn.contiguous()
        ub = None if ub is None else ub.contiguous()
        h_all = torch.empty((B, T, D), dtype=torch.float32, device=xw.device)
        _lib.call("rh_augru_fwd", _p(xw), _p(attn), _p(U), _p(ub), B, T, D, _p(h_all), _stream())
        ctx.save_for_backward(xw, attn, U, ub, h_all)
        return h_all

    @staticmethod
    def backward(ctx, g):
        xw, attn, U, ub, h_all = ctx.saved_tensors
        B, T, D3 = xw.shape
        D = D3 // 3
        g = g.contiguous()
        d_xw = torch.empty_like(xw)
        d_huh = torch.empty((B, T, D), dtype=torch.float32, device=xw.device)
        d_attn = None if attn is None else torch.empty((B, T), dtype=torch.float32, device=xw.device)
        _lib.call("rh_augru_bwd", _p(xw), _p(attn), _p(U), _p(ub), _p(h_all), _p(g), B, T, D, _p(d_xw), _p(d_huh),
                  _p(d_attn), _stream())
        d_U = d_ub = None
        if ctx.needs_input_grad[2] or (ub is not None and ctx.needs_input_grad[3]):
            # gradient of s = h_{t-1} U + state_bias: [d pre_u | d pre_r | d s_h] for every (sample, step); dU^T =
            # d_s^T h_prev sums over B*T rows -- the split-batch MFMA weight-gradient kernel's shape (a library GEMM
            # with K = B*T = 409600 took 580 us here), which also returns the column sums = d state_bias
            d_s = torch.cat([d_xw[:, :, :2 * D], d_huh], dim=2).reshape(B * T, D3)
            h_prev = torch.cat([h_all.new_zeros(B, 1, D), h_all[:, :-1]], dim=1).reshape(B * T, D)
            d_Ut, d_ub = linear_wgrad(d_s, h_prev, want_bias=ub is not None)
            d_U = d_Ut.t()
        return d_xw, d_attn, d_U, d_ub


def augru_ok(xw, D):
    return (xw.is_cuda and xw.dtype == torch.float32 and xw.dim() == 3 and xw.shape[1] >= 1 and
            4 <= D <= _lib.H.RH_AUGRU_MAX_D and D & (D - 1) == 0 and xw.shape[2] == 3 * D)


def augru(xw, attn, U, state_bias=None):
    """States h_1 .. h_T (B, T, D) of the attentional-update GRU (reference dien.py:30-36, 60-66) in one launch each
    way; ``xw`` holds the input halves of the three gates for every step, ``U`` = [Uu | Ur | Uh]."""
    return _AugruFn.apply(xw, attn, U, state_bias)


def gru_ok(gru, x):
    return (isinstance(gru, torch.nn.GRU) and gru.num_layers == 1 and not gru.bidirectional and gru.batch_first and
            gru.bias and gru.input_size == x.shape[-1] and x.dim() == 3 and x.is_cuda and x.dtype == torch.float32 and
            x.shape[1] >= 1 and gru.hidden_size in (4, 8, 16, 32))


def gru(gru_mod, x):
    """Outputs (B, T, H) of a one-layer ``nn.GRU(batch_first=True)`` from the zero state, through the same recurrence
    kernel: PyTorch's cell is r, z, n with h' = (1 - z) n + z h, i.e. the kernel's update gate is 1 - z = sigmoid of
    the NEGATED z pre-activation, its weight a = 1, and bias_hh rides on the state product."""
    H = gru_mod.hidden_size
    w_ih, w_hh, b_ih, b_hh = gru_mod.weight_ih_l0, gru_mod.weight_hh_l0, gru_mod.bias_ih_l0, gru_mod.bias_hh_l0

    def gates(m):  # rows (r, z, n) of a (3H, ...) parameter -> kernel order (1 - z, r, n)
        return torch.cat([-m[H:2 * H], m[:H], m[2 * H:]], dim=0)

    B, T, _ = x.shape
    xw = linear(x.reshape(B * T, -1), gates(w_ih), gates(b_ih)).view(B, T, 3 * H)
    return _AugruFn.apply(xw, None, gates(w_hh).t(), gates(b_hh))


# --------------------------------------------------------------------------------------------
_sample_rng = {}


class _InbatchLogitsFn(torch.autograd.Function):
    """(B, 1 + K) in-batch logits straight from the tower outputs (csrc/match.hip): no (B, C) score matrix."""

    @staticmethod
    def forward(ctx, u, v, neg, row0):
        require_hip(u, v, neg)
        if u.dim() != 2 or v.dim() != 2 or u.shape[1] != v.shape[1]:
            raise ValueError("in-batch logits expect (B, D) user and (C, D) item embeddings of one width")
        if neg.dtype != torch.int64 or neg.dim() != 2 or neg.shape[0] != u.shape[0]:
            # (the kernel reads int64 words: a narrower index tensor would be read past its end)
            raise ValueError("in-batch negatives must be an int64 (B, K) tensor")
        if u.stride(1) != 1:
            u = u.contiguous()
        if v.stride(1) != 1:
            v = v.contiguous()
        neg = neg.contiguous()
        B, D = u.shape
        C, K = v.shape[0], neg.shape[1]
        logits = torch.empty((B, 1 + K), dtype=torch.float32, device=u.device)
        _lib.call("rh_inbatch_logits_fwd", _p(u), u.stride(0), _p(v), v.stride(0), _p(neg), B, C, D, K, int(row0),
                  _p(logits), _p(err_flag(u.device)), _stream())
        ctx.save_for_backward(u, v, neg)
        ctx.row0 = int(row0)
        return logits

    @staticmethod
    def backward(ctx, g):
        u, v, neg = ctx.saved_tensors
        B, D = u.shape
        C, K = v.shape[0], neg.shape[1]
        g = g.contiguous()
        g_u = torch.empty((B, D), dtype=torch.float32, device=u.device)
        g_v = torch.zeros((C, D), dtype=torch.float32, device=u.device)
        _lib.call("rh_inbatch_logits_bwd", _p(u), u.stride(0), _p(v), v.stride(0), _p(neg), _p(g), B, C, D, K, ctx.row0,
                  _p(g_u), _p(g_v), _stream())
        return g_u, g_v, None, None


def inbatch_logits_ok(u, v):
    return (u.is_cuda and v.is_cuda and u.dtype == torch.float32 and v.dtype == torch.float32 and u.dim() == 2 and
            v.dim() == 2 and u.shape[1] == v.shape[1] and 1 <= u.shape[1] <= _lib.H.RH_INBATCH_MAX_D and u.shape[0] >= 1)


def inbatch_logits(u, v, neg, row0=0):
    """logits[i, 0] = u_i . v_(row0 + i), logits[i, 1 + k] = u_i . v_neg[i, k]  (== gather_inbatch_logits(u @ v.T, neg))."""
    return _InbatchLogitsFn.apply(u, v, neg, row0)


def inbatch_sample(batch_size, k, device, seed=None, cols=None, row0=0):
    """(B, K) int64: per row K distinct in-batch negatives (never the row itself), uniformly at random; hipGraph-safe.

    ``cols`` / ``row0``: the rows are rows [row0, row0 + B) of a (cols x cols) problem (cross-rank negatives): row r
    draws from {0..cols-1} minus {row0 + r}, with the random stream of global row row0 + r."""
    key = (str(device), seed)
    st = _sample_rng.get(key)
    if st is None:
        s = torch.initial_seed() if seed is None else int(seed)
        st = torch.tensor([s & 0x7FFFFFFFFFFFFFFF, 0], dtype=torch.int64).to(device)
        _sample_rng[key] = st
    out = torch.empty((batch_size, k), dtype=torch.int64, device=device)
    if cols is None:
        _lib.call("rh_inbatch_sample", _p(st), batch_size, k, _p(out), _stream())
    else:
        _lib.call("rh_inbatch_sample_rows", _p(st), batch_size, int(cols), int(row0), k, _p(out), _stream())
    _lib.call("rh_batch_advance", ctypes.c_void_p(st.data_ptr() + 8), 1, 0, _stream())
    return out


def shard_narrow(idx, out):
    """``out`` (N, F) int32, contiguous <- the int64 index matrix ``idx`` (N, F) (rows contiguous, any row stride), saturating
    (``rh_shard_narrow``: what ``idx.clamp(-1, 2**31 - 1).to(torch.int32)`` computes, written where the caller says)."""
    require_hip(idx, out)
    if idx.dim() != 2 or idx.dtype != torch.int64 or idx.stride(1) != 1 or out.shape != idx.shape or \
            out.dtype != torch.int32 or not out.is_contiguous():
        raise ValueError("shard_narrow: idx (N, F) int64 with contiguous rows, out (N, F) contiguous int32")
    _lib.call("rh_shard_narrow", _p(idx), idx.stride(0), int(idx.shape[0]), int(idx.shape[1]), _p(out), _stream())
    return out


def shard_localize(idx, desc, world, rank, out=None):
    """int32 (N, F): the index matrix ``idx`` (N, F) of a global batch rewritten for this rank's table shards
    (``rh_shard_localize``; desc = device int64 [vocab | pad | sink] per field, see sharding.RowShard)."""
    require_hip(idx, desc)
    if idx.dim() != 2 or not idx.is_contiguous() or idx.dtype not in (torch.int64, torch.int32):
        raise ValueError("shard_localize: indices must be a contiguous (N, F) int64 / int32 matrix")
    N, F = int(idx.shape[0]), int(idx.shape[1])
    if desc.numel() != 3 * F or desc.dtype != torch.int64:
        raise ValueError("shard_localize: descriptor must hold 3 * F int64 entries")
    if out is None:
        out = torch.empty((N, F), dtype=torch.int32, device=idx.device)
    elif out.shape != (N, F) or out.dtype != torch.int32 or not out.is_contiguous():
        raise ValueError("shard_localize: out must be a contiguous int32 (N, F) tensor")
    _lib.call("rh_shard_localize", _p(idx), 1 if idx.dtype == torch.int64 else 0, N, F, _p(desc), int(world),
              int(rank), _p(out), _p(err_flag(idx.device)), _stream())
    return out


# --------------------------------------------------------------------------------------------
# multi-interest user towers and list-wise scoring (csrc/interest.hip)
class _CapsuleFn(torch.autograd.Function):
    """CapsuleNetwork routing (reference basic/layers.py:657-712).  Types 0 / 1: x = the Linear's output U (B, L, Iu*D);
    type 2: x = the history E (B, L, D) and w the (1, L, I*D, D) weight.  Gradient through the last iteration only."""

    @staticmethod
    def forward(ctx, x, w, mask, init, kind, I, D, iters):
        B, L = int(mask.shape[0]), int(mask.shape[1])
        x = x.contiguous()
        w = w.contiguous() if w is not None else None
        dev = x.device
        cap = torch.empty((B, I, D), dtype=torch.float32, device=dev)
        sw = torch.empty((B, I, L), dtype=torch.float32, device=dev)
        s = torch.empty((B, I, D), dtype=torch.float32, device=dev)
        U, E = (None, x) if kind == 2 else (x, None)
        _lib.call("rh_capsule_fwd", _p(U), _p(E), _p(w), _p(mask), _p(init), B, L, I, D, kind, iters, _p(cap), _p(sw), _p(s),
                  _stream())
        ctx.dims = (B, L, I, D, kind)
        ctx.save_for_backward(x, w, sw, s)
        return cap

    @staticmethod
    def backward(ctx, g):
        x, w, sw, s = ctx.saved_tensors
        B, L, I, D, kind = ctx.dims
        g = g.contiguous()
        dev = g.device
        if kind != 2:
            g_u = torch.empty(x.shape, dtype=torch.float32, device=dev)
            _lib.call("rh_capsule_bwd", _p(g), _p(s), _p(sw), _NULL, B, L, I, D, kind, _p(g_u), _NULL, _NULL, _stream())
            return g_u, None, None, None, None, None, None, None
        g_e = torch.empty((B, L, D), dtype=torch.float32, device=dev)
        g_s = torch.empty((B, I, D), dtype=torch.float32, device=dev)
        _lib.call("rh_capsule_bwd", _p(g), _p(s), _p(sw), _p(w), B, L, I, D, 2, _NULL, _p(g_e), _p(g_s), _stream())
        g_w = None
        if ctx.needs_input_grad[1]:
            g_w = torch.empty(w.shape, dtype=torch.float32, device=dev)
            if B == 0:
                g_w.zero_()
            else:
                nch = _lib.call("rh_capsule_wgrad_nchunks", B)
                part = torch.empty((nch, L * I * D * D), dtype=torch.float32, device=dev)
                _lib.call("rh_capsule_wgrad", _p(g_s), _p(sw), _p(x), B, L, I, D, _p(part), _stream())
                _lib.call("rh_colsum", _p(part), nch, L * I * D * D, _p(g_w), _NULL, 0, _NULL, _stream())
        return g_e, g_w, None, None, None, None, None, None


def capsule_supported(L, I, D, kind):
    return bool(_lib.call("rh_capsule_supported", int(L), int(I), int(D), int(kind)))


def capsule_routing(x, w, mask, init, kind, interest_num, embed_dim, routing_times):
    """(B, I, D) interest capsules; ``mask`` (B, L) int32 (nonzero = kept), ``init`` (B, I, L) initial logits or None."""
    require_hip(x, w, mask, init)
    return _CapsuleFn.apply(x, w, mask, init, int(kind), int(interest_num), int(embed_dim), int(routing_times))


class _SaPoolFn(torch.autograd.Function):
    """MultiInterestSA after A = tanh(E W1) W2: softmax over L of A + -1e9 (1 - mask), then A^T E (layers.py:601-608)."""

    @staticmethod
    def forward(ctx, A, E, mask):
        A, E = A.contiguous(), E.contiguous()
        B, L, I = (int(v) for v in A.shape)
        D = int(E.shape[2])
        P = torch.empty((B, L, I), dtype=torch.float32, device=A.device)
        out = torch.empty((B, I, D), dtype=torch.float32, device=A.device)
        _lib.call("rh_sa_pool_fwd", _p(A), _p(E), _p(mask), B, L, I, D, _p(P), _p(out), _stream())
        ctx.save_for_backward(P, E)
        return out

    @staticmethod
    def backward(ctx, g):
        P, E = ctx.saved_tensors
        B, L, I = (int(v) for v in P.shape)
        D = int(E.shape[2])
        g = g.contiguous()
        gA = torch.empty((B, L, I), dtype=torch.float32, device=g.device)
        gE = torch.empty((B, L, D), dtype=torch.float32, device=g.device)
        _lib.call("rh_sa_pool_bwd", _p(P), _p(E), _p(g), B, L, I, D, _p(gA), _p(gE), _stream())
        return gA, gE, None


def sa_supported(L, I, D):
    return bool(_lib.call("rh_sa_supported", int(L), int(I), int(D)))


def sa_pool(A, E, mask=None):
    """(B, I, D) = softmax_L(A + -1e9 (1 - mask))^T E for A (B, L, I), E (B, L, D), mask (B, L) int32 or None."""
    require_hip(A, E, mask)
    return _SaPoolFn.apply(A, E, mask)


class _ListwiseFn(torch.autograd.Function):
    """(B, 1 + K) logits of the list-wise retrieval models: normalised item rows, best interest by the positive."""

    @staticmethod
    def forward(ctx, u, pos, neg, temperature):
        u, neg = u.contiguous(), neg.contiguous()
        if pos.stride(1) != 1:
            pos = pos.contiguous()
        B, I, D = (int(v) for v in u.shape)
        K = int(neg.shape[1])
        dev = u.device
        logits = torch.empty((B, 1 + K), dtype=torch.float32, device=dev)
        best = torch.empty((B,), dtype=torch.int32, device=dev)
        nrm = torch.empty((B, 1 + K), dtype=torch.float32, device=dev)
        _lib.call("rh_listwise_fwd", _p(u), _p(pos), pos.stride(0), _p(neg), B, I, D, K, float(temperature), _p(logits),
                  _p(best), _p(nrm), _stream())
        ctx.temperature = float(temperature)
        ctx.save_for_backward(u, pos, neg, best, nrm)
        ctx.mark_non_differentiable(best)
        return logits, best

    @staticmethod
    def backward(ctx, g, _unused):
        u, pos, neg, best, nrm = ctx.saved_tensors
        B, I, D = (int(v) for v in u.shape)
        K = int(neg.shape[1])
        g = g.contiguous()
        dev = g.device
        g_u = torch.empty((B, I, D), dtype=torch.float32, device=dev)
        g_pos = torch.empty((B, D), dtype=torch.float32, device=dev)
        g_neg = torch.empty((B, K, D), dtype=torch.float32, device=dev)
        _lib.call("rh_listwise_bwd", _p(u), _p(pos), pos.stride(0), _p(neg), _p(best), _p(nrm), _p(g), B, I, D, K,
                  ctx.temperature, _p(g_u), _p(g_pos), _p(g_neg), _stream())
        return g_u, g_pos, g_neg, None


def listwise_ok(u, pos, neg):
    return (u.is_cuda and u.dtype == pos.dtype == neg.dtype == torch.float32 and u.dim() == 3 and pos.dim() == 2 and
            neg.dim() == 3 and 1 <= u.shape[1] <= _lib.H.RH_LISTWISE_MAX_I and 1 <= u.shape[2] <= _lib.H.RH_LISTWISE_MAX_D and
            pos.shape == (u.shape[0], u.shape[2])
            and neg.shape[0] == u.shape[0] and neg.shape[2] == u.shape[2] and neg.shape[1] <= _lib.H.RH_LISTWISE_MAX_K)


def listwise_logits(u, pos, neg, temperature=1.0):
    """(logits (B, 1 + K), best (B,) int32): logits = u_best . normalize([pos, neg]) / temperature, u (B, I, D) the
    normalised user vectors, pos (B, D) / neg (B, K, D) the raw item rows; best = first argmax_i u_i . normalize(pos)."""
    require_hip(u, pos, neg)
    if not listwise_ok(u, pos, neg):
        raise RuntimeError(f"torch_rechub_amd: list-wise scoring of user {tuple(u.shape)}, items {tuple(pos.shape)} / "
                           f"{tuple(neg.shape)} has no HIP kernel (I <= {_lib.H.RH_LISTWISE_MAX_I}, D <= {_lib.H.RH_LISTWISE_MAX_D}, "
                           f"K <= {_lib.H.RH_LISTWISE_MAX_K}, float32)")
    return _ListwiseFn.apply(u, pos, neg, float(temperature))


# --------------------------------------------------------------------------------------------
# SINE's sparse-interest chain (csrc/sine.hip)
class _SineInterestFn(torch.autograd.Function):
    """sine.py:94-118 between the w_1 / w_k1 / w_3 products and h_3: (phi (B, K, E), xhat (B, S, E), idx (B, K) int32)."""

    @staticmethod
    def forward(ctx, X, Y, a1, a2, mask, C):
        X, Y, a1, a2, C = X.contiguous(), Y.contiguous(), a1.contiguous(), a2.contiguous(), C.contiguous()
        B, S, E = (int(v) for v in X.shape)
        K, T = int(a2.shape[2]), int(C.shape[0])
        dev = X.device
        idx = torch.empty((B, K), dtype=torch.int32, device=dev)
        phi = torch.empty((B, K, E), dtype=torch.float32, device=dev)
        xhat = torch.empty((B, S, E), dtype=torch.float32, device=dev)
        P1 = torch.empty((B, S), dtype=torch.float32, device=dev)
        P2 = torch.empty((B, K, S), dtype=torch.float32, device=dev)
        PU = torch.empty((B, K, S), dtype=torch.float32, device=dev)
        _lib.call("rh_sine_interest_fwd", _p(X), _p(Y), _p(a1), _p(a2), _p(mask), _p(C), B, S, E, T, K, _p(idx), _p(phi),
                  _p(xhat), _p(P1), _p(P2), _p(PU), _stream())
        ctx.save_for_backward(X, Y, C, mask, idx, P1, P2, PU)
        ctx.mark_non_differentiable(idx)
        return phi, xhat, idx

    @staticmethod
    def backward(ctx, g_phi, g_xhat, _unused):
        X, Y, C, mask, idx, P1, P2, PU = ctx.saved_tensors
        B, S, E = (int(v) for v in X.shape)
        K, T = int(idx.shape[1]), int(C.shape[0])
        dev = X.device
        g_phi, g_xhat = g_phi.contiguous(), g_xhat.contiguous()  # (autograd materialises an unused output's as zeros)
        g_X = torch.empty((B, S, E), dtype=torch.float32, device=dev)
        g_Y = torch.empty((B, S, E), dtype=torch.float32, device=dev)
        g_a1 = torch.empty((B, S), dtype=torch.float32, device=dev)
        g_a2 = torch.empty((B, S, K), dtype=torch.float32, device=dev)
        g_C = torch.empty((T, E), dtype=torch.float32, device=dev)
        if B == 0:
            g_C.zero_()
        else:
            nch = _lib.query("rh_sine_nchunks", B)
            rows = torch.empty((B, K, E), dtype=torch.float32, device=dev)
            part = torch.empty((nch, T * E), dtype=torch.float32, device=dev)
            _lib.call("rh_sine_interest_bwd", _p(X), _p(Y), _p(C), _p(idx), _p(P1), _p(P2), _p(PU), _p(g_phi), _p(g_xhat), B,
                      S, E, T, K, _p(g_X), _p(g_Y), _p(g_a1), _p(g_a2), _p(rows), _p(part), _stream())
            _lib.call("rh_colsum", _p(part), nch, T * E, _p(g_C), _NULL, 0, _NULL, _stream())
        return g_X, g_Y, g_a1, g_a2, None, g_C


class _SineAggregateFn(torch.autograd.Function):
    """sine.py:122-128 after h_3 w_5: v (B, E).  The backward recomputes the chain from the inputs (in fp64, csrc/sine.hip)."""

    @staticmethod
    def forward(ctx, xhat, a3, mask, phi, inv_t):
        xhat, a3, phi = xhat.contiguous(), a3.contiguous(), phi.contiguous()
        B, S, E = (int(v) for v in xhat.shape)
        K = int(phi.shape[1])
        v = torch.empty((B, E), dtype=torch.float32, device=xhat.device)
        _lib.call("rh_sine_aggregate_fwd", _p(xhat), _p(a3), _p(mask), _p(phi), inv_t, B, S, E, K, _p(v), _stream())
        ctx.inv_t = inv_t
        ctx.save_for_backward(xhat, a3, mask, phi)
        return v

    @staticmethod
    def backward(ctx, g_v):
        xhat, a3, mask, phi = ctx.saved_tensors
        B, S, E = (int(v) for v in xhat.shape)
        K = int(phi.shape[1])
        dev = xhat.device
        g_v = g_v.contiguous()
        g_xhat = torch.empty((B, S, E), dtype=torch.float32, device=dev)
        g_a3 = torch.empty((B, S), dtype=torch.float32, device=dev)
        g_phi = torch.empty((B, K, E), dtype=torch.float32, device=dev)
        _lib.call("rh_sine_aggregate_bwd", _p(xhat), _p(a3), _p(mask), _p(phi), _p(g_v), ctx.inv_t, B, S, E, K, _p(g_xhat),
                  _p(g_a3), _p(g_phi), _stream())
        return g_xhat, g_a3, None, g_phi, None


def sine_supported(S, E, T, K):
    return bool(_lib.query("rh_sine_supported", int(S), int(E), int(T), int(K)))


def _sine_check(what, tensors, mask, S, E, T, K):
    if any(t.dtype != torch.float32 for t in tensors) or mask.dtype != torch.int32 or not mask.is_contiguous():
        raise ValueError(f"torch_rechub_amd: {what} takes float32 tensors and a contiguous int32 mask")
    if not sine_supported(S, E, T, K):
        from .models.matching._listwise import no_kernel
        raise no_kernel(f"{what} at seq_max_len {S}, embedding_dim {E}, num_concept {T}, num_intention {K} "
                        f"(S <= {_lib.H.RH_SINE_MAX_S}, E <= {_lib.H.RH_SINE_MAX_E}, T <= {_lib.H.RH_SINE_MAX_T}, "
                        f"K <= min(T, {_lib.H.RH_SINE_MAX_K}))")


def sine_interests(X, Y, a1, a2, mask, C):
    """(phi (B, K, E), xhat (B, S, E), idx (B, K) int32) of SINE's sparse-interest extraction (sine.py:94-118) from
    X = x_u and Y = X w_3 (B, S, E), a1 (B, S) = tanh(X w_1) w_2, a2 (B, S, K) = tanh(X w_k1) w_k2, mask (B, S) int32
    (1 = kept) and the concept table C (T, E).  idx are the chosen concepts in descending score order."""
    require_hip(X, Y, a1, a2, mask, C)
    B, S, E = (int(v) for v in X.shape)
    if Y.shape != X.shape or a1.shape != (B, S) or a2.dim() != 3 or a2.shape[:2] != (B, S) or mask.shape != (B, S) or \
            C.dim() != 2 or C.shape[1] != E:
        raise ValueError("sine_interests: X, Y (B, S, E), a1 (B, S), a2 (B, S, K), mask (B, S), C (T, E) expected")
    _sine_check("SINE's interest extraction", (X, Y, a1, a2, C), mask, S, E, int(C.shape[0]), int(a2.shape[2]))
    return _SineInterestFn.apply(X, Y, a1, a2, mask, C)


def sine_aggregate(xhat, a3, mask, phi, temperature):
    """v (B, E) of SINE's interest aggregation (sine.py:122-128) from xhat (B, S, E), a3 (B, S) = tanh(xhat w_4) w_5,
    mask (B, S) int32 and phi (B, K, E)."""
    require_hip(xhat, a3, mask, phi)
    B, S, E = (int(v) for v in xhat.shape)
    if a3.shape != (B, S) or mask.shape != (B, S) or phi.dim() != 3 or phi.shape[0] != B or phi.shape[2] != E:
        raise ValueError("sine_aggregate: xhat (B, S, E), a3 (B, S), mask (B, S), phi (B, K, E) expected")
    K = int(phi.shape[1])
    _sine_check("SINE's interest aggregation", (xhat, a3, phi), mask, S, E, max(K, 1), K)
    return _SineAggregateFn.apply(xhat, a3, mask, phi, 1.0 / float(temperature))


# --------------------------------------------------------------------------------------------
# RQ-VAE's residual quantizer (csrc/rq.hip)
def rq_supported(E, sizes):
    """Whether csrc/rq.hip takes rows of width E against codebooks of these sizes (E <= RH_RQ_MAX_E, sizes <= RH_RQ_MAX_CODES, <= RH_RQ_MAX_L
    levels)."""
    sizes = [int(v) for v in sizes]
    arr = _int_array(sizes)
    return bool(_lib.query("rh_rq_supported", int(E), len(sizes), ctypes.cast(arr, ctypes.c_void_p)))


def _rq_check(x, codebooks):
    require_hip(x, *codebooks)
    if x.dim() != 2 or not codebooks or any(c.dim() != 2 or c.shape[1] != x.shape[1] for c in codebooks):
        raise ValueError("residual quantizer: rows (N, E) and codebooks (n_e, E) expected")
    if x.dtype != torch.float32 or any(c.dtype != torch.float32 for c in codebooks):
        raise ValueError("torch_rechub_amd: the residual quantizer takes float32 tensors")
    sizes = [int(c.shape[0]) for c in codebooks]
    if not rq_supported(int(x.shape[1]), sizes):
        from .models.matching._listwise import no_kernel
        raise no_kernel(f"the residual quantizer at e_dim {int(x.shape[1])} with codebook sizes {sizes} "
                        f"(e_dim <= {_lib.H.RH_RQ_MAX_E}, sizes <= {_lib.H.RH_RQ_MAX_CODES}, at most {_lib.H.RH_RQ_MAX_L} levels)")
    return sizes


def rq_forward(r_in, codebooks, l0=0, l1=None, given=0, idx=None, sse=None):
    """The levels [l0, l1) of the residual quantizer on r_in (N, E), the residual entering level l0: (idx (N, L) int32,
    r_out (N, E), x_q = r_in - r_out, sse (L,)).  Level l takes its index from ``idx`` instead of searching it when bit l of
    ``given`` is set.  ``idx`` and ``sse`` of an earlier call are continued in place.  No autograd."""
    codebooks = [c.detach().contiguous() for c in codebooks]
    r_in = r_in.detach().contiguous()
    sizes = _rq_check(r_in, codebooks)
    N, E = (int(v) for v in r_in.shape)
    L = len(sizes)
    l1 = L if l1 is None else int(l1)
    if not 0 <= l0 < l1 <= L:
        raise ValueError(f"residual quantizer: level range [{l0}, {l1}) of {L}")
    dev = r_in.device
    whole = l0 == 0 and l1 == L  # every element of idx and sse is written by this call
    if idx is None:
        if given:
            raise ValueError("residual quantizer: given levels need their indices")
        idx = (torch.empty if whole and N else torch.zeros)((N, L), dtype=torch.int32, device=dev)
    if sse is None:
        sse = (torch.empty if whole and N else torch.zeros)((L,), dtype=torch.float32, device=dev)
    r_out = torch.empty((N, E), dtype=torch.float32, device=dev)
    x_q = torch.empty((N, E), dtype=torch.float32, device=dev)
    if N:
        blocks, _ = _lib.query("rh_rq_nchunks", N, out=(ctypes.c_int, ctypes.c_int))
        part = torch.empty((blocks, l1 - l0), dtype=torch.float32, device=dev)
        _lib.call("rh_rq_fwd", _p(r_in), ctypes.cast(_ptr_array(codebooks), ctypes.c_void_p),
                  ctypes.cast(_int_array(sizes), ctypes.c_void_p), N, E, L, int(l0), l1, int(given), _p(idx), _p(r_out),
                  _p(x_q), _p(part), _p(sse), _stream())
    return idx, r_out, x_q, sse


def _sinkhorn_level(r, C, epsilon, iters):
    """Index of every row at a Sinkhorn level, as torch ops on the device (rqvae.py:248-258)."""
    from .models.generative.rqvae import VectorQuantizer, sinkhorn_algorithm
    d = torch.sum(r**2, dim=1, keepdim=True) + torch.sum(C**2, dim=1, keepdim=True).t() - 2 * torch.matmul(r, C.t())
    d = VectorQuantizer.center_distance_for_constraint(d).double()
    Q = sinkhorn_algorithm(d, epsilon, iters)
    if torch.isnan(Q).any() or torch.isinf(Q).any():
        print("Sinkhorn Algorithm returns nan/inf values.")
    return torch.argmax(Q, dim=-1).to(torch.int32)


class _ResidualQuantizeFn(torch.autograd.Function):
    """(x_q (N, E), loss (), idx (N, L) int64) of rqvae.py:382-398 on x (N, E); sk = ((level, epsilon, iterations), ...)."""

    @staticmethod
    def forward(ctx, x, beta, sk, *codebooks):
        x = x.contiguous()
        cbs = [c.detach().contiguous() for c in codebooks]
        N, E = (int(v) for v in x.shape)
        L = len(cbs)
        idx, sse, r, l0, given, x_q = None, None, x, 0, 0, None
        for level, eps, iters in sk:  # the cold path: the levels before a Sinkhorn level, then its index as torch ops
            if level > l0:
                idx, r, _, sse = rq_forward(r, cbs, l0, level, given, idx, sse)
            if idx is None:
                idx = torch.zeros((N, L), dtype=torch.int32, device=x.device)
            idx[:, level] = _sinkhorn_level(r, cbs[level], eps, iters)
            l0, given = level, given | (1 << level)
        idx, r, x_q, sse = rq_forward(r, cbs, l0, L, given, idx, sse)
        if l0 > 0:
            x_q = x - r
        loss = sse.sum() * ((1.0 + beta) / (float(N) * E * L)) if N else sse.sum() * float("nan")
        ctx.beta = beta
        ctx.save_for_backward(x, idx, *cbs)
        out_idx = idx.to(torch.int64)
        ctx.mark_non_differentiable(out_idx)
        return x_q, loss, out_idx

    @staticmethod
    def backward(ctx, g_xq, g_loss, _unused):
        x, idx, *cbs = ctx.saved_tensors
        N, E = (int(v) for v in x.shape)
        sizes = [int(c.shape[0]) for c in cbs]
        dev = x.device
        total = sum(sizes) * E
        g_x = torch.empty((N, E), dtype=torch.float32, device=dev)
        g_C = torch.empty((total,), dtype=torch.float32, device=dev)
        if N == 0:
            g_C.zero_()
        else:
            _, nch = _lib.query("rh_rq_nchunks", N, out=(ctypes.c_int, ctypes.c_int))
            part = torch.empty((nch, total), dtype=torch.float32, device=dev)
            g_loss, g_xq = g_loss.to(torch.float32).contiguous(), g_xq.contiguous()
            _lib.call("rh_rq_bwd", _p(x), ctypes.cast(_ptr_array(cbs), ctypes.c_void_p),
                      ctypes.cast(_int_array(sizes), ctypes.c_void_p), _p(idx), _p(g_xq), _p(g_loss),
                      float(ctx.beta), N, E, len(cbs), _p(g_x), _p(part), _p(g_C), _stream())
        grads, off = [], 0
        for n in sizes:
            grads.append(g_C[off:off + n * E].view(n, E))
            off += n * E
        return (g_x, None, None, *grads)


def residual_quantize(x, codebooks, beta, sk_epsilons=None, sk_iters=100, use_sk=True):
    """(x_q, loss, indices) of the RQ-VAE's residual quantizer (rqvae.py:241-274 per level, :382-398 across levels) on x
    (..., E) and the codebooks [(n_e, E), ...]: x_q = x + (sum of the chosen codes - x).detach(), loss = the mean over
    levels of codebook_loss + beta commitment_loss, indices int64 of shape x.shape[:-1] + (L,).  A level with ``use_sk`` and
    ``sk_epsilons[l] > 0`` takes its index from the Sinkhorn assignment (torch ops on the device; ``sk_iters`` an int or one
    per level); every other level, the distances, arg-min, gathers, losses and the backward are csrc/rq.hip."""
    codebooks = list(codebooks)
    if not codebooks:
        raise ValueError("residual_quantize: at least one codebook expected")
    flat = x.reshape(-1, x.shape[-1])
    _rq_check(flat, codebooks)
    L = len(codebooks)
    eps = [0.0] * L if sk_epsilons is None else [float(e) for e in sk_epsilons]
    if len(eps) != L:
        raise ValueError(f"residual_quantize: {len(eps)} sk_epsilons for {L} codebooks")
    iters = [int(sk_iters)] * L if isinstance(sk_iters, int) else [int(v) for v in sk_iters]
    sk = tuple((l, eps[l], iters[l]) for l in range(L) if use_sk and eps[l] > 0)
    x_q, loss, idx = _ResidualQuantizeFn.apply(flat, float(beta), sk, *codebooks)
    return x_q.view(x.shape), loss, idx.view(tuple(x.shape[:-1]) + (L,))


# --------------------------------------------------------------------------------------------
# HSTU: pointwise relative-bias attention (csrc/hstu.hip) and the next-token head (csrc/stream_ce.hip)
# --------------------------------------------------------------------------------------------
class _HstuAttnFn(torch.autograd.Function):
    """(B, L, H dv) = (silu(alpha q k^T + rab) / N, causal and key-padding masked) v, q / k / v read from proj."""

    @staticmethod
    def forward(ctx, proj, pos_w, ts_w, td, kmask, cfg):
        proj = proj.contiguous()
        B, L, ld = (int(v) for v in proj.shape)
        H, dqk, dv, N, nb, fn_log, minutes, divisor, alpha = cfg
        out = torch.empty((B, L, H * dv), dtype=torch.float32, device=proj.device)
        _lib.call("rh_hstu_attn_fwd", _p(proj), ld, B, L, H, dqk, dv, _p(td), _p(kmask), _p(pos_w), _p(ts_w), N, nb,
                  fn_log, minutes, divisor, alpha, _p(out), _stream())
        ctx.cfg = cfg
        ctx.save_for_backward(proj, pos_w, ts_w, td, kmask)
        return out

    @staticmethod
    def backward(ctx, g):
        proj, pos_w, ts_w, td, kmask = ctx.saved_tensors
        B, L, ld = (int(v) for v in proj.shape)
        H, dqk, dv, N, nb, fn_log, minutes, divisor, alpha = ctx.cfg
        g = g.contiguous()
        dev = g.device
        g_proj = torch.zeros((B, L, ld), dtype=torch.float32, device=dev)  # the u columns stay zero
        if B == 0:
            return g_proj, torch.zeros_like(pos_w), torch.zeros_like(ts_w), None, None, None
        nparts = _lib.call("rh_hstu_attn_nparts", B, L, H)
        pos_part = torch.empty((nparts, L), dtype=torch.float32, device=dev)
        ts_part = torch.empty((nparts, nb + 1), dtype=torch.float32, device=dev) if td is not None else None
        g_pos = torch.empty_like(pos_w)
        g_ts = torch.empty_like(ts_w)
        _lib.call("rh_hstu_attn_bwd", _p(proj), ld, B, L, H, dqk, dv, _p(td), _p(kmask), _p(pos_w), _p(ts_w), N, nb,
                  fn_log, minutes, divisor, alpha, _p(g), _p(g_proj), _p(pos_part), _p(ts_part), _p(g_pos), _p(g_ts),
                  _stream())
        return g_proj, g_pos, g_ts, None, None, None


def hstu_attention(proj, pos_w, ts_w, n_heads, dqk, dv, max_seq_len, time_diffs=None, padding_mask=None,
                   num_time_buckets=128, time_bucket_fn="sqrt", time_bucket_divisor=1.0, time_bucket_unit="minutes"):
    """HSTU attention output (B, L, H dv) from ``proj`` (B, L, 2 H (dqk + dv)) = silu(proj1(LN(x))) laid out [q | k | u | v],
    the rab tables pos_w (2 N - 1, H) / ts_w (nb + 1, H), time_diffs (B, L) int64 seconds or None (position-only bias) and
    padding_mask (B, L) bool (True = valid key) or None."""
    require_hip(proj, pos_w, ts_w, time_diffs, padding_mask)
    if proj.dtype != torch.float32 or pos_w.dtype != torch.float32 or ts_w.dtype != torch.float32:
        raise RuntimeError("torch_rechub_amd: HSTU attention runs in float32 only")
    B, L, W = (int(v) for v in proj.shape)
    if W != 2 * n_heads * (dqk + dv):
        raise RuntimeError(f"torch_rechub_amd: HSTU projection width {W} != 2 * {n_heads} * ({dqk} + {dv})")
    if not (1 <= L <= min(int(max_seq_len), _lib.H.RH_HSTU_MAX_L) and 1 <= dqk <= _lib.H.RH_HSTU_MAX_DH and
            1 <= dv <= _lib.H.RH_HSTU_MAX_DH and
            num_time_buckets <= _lib.H.RH_HSTU_MAX_BUCKETS):
        raise RuntimeError(f"torch_rechub_amd: HSTU attention with L={L}, dqk={dqk}, dv={dv}, "
                           f"num_time_buckets={num_time_buckets} has no HIP kernel (L <= min(max_seq_len, "
                           f"{_lib.H.RH_HSTU_MAX_L}), dqk, dv <= {_lib.H.RH_HSTU_MAX_DH}, "
                           f"num_time_buckets <= {_lib.H.RH_HSTU_MAX_BUCKETS})")
    if time_bucket_fn not in ("sqrt", "log") or time_bucket_unit not in ("minutes", "seconds"):
        raise ValueError(f"Unsupported time bucketing {time_bucket_fn!r} / {time_bucket_unit!r}")
    td = None if time_diffs is None else time_diffs.to(torch.int64).contiguous()
    km = None if padding_mask is None else padding_mask.to(torch.int32).contiguous()
    cfg = (int(n_heads), int(dqk), int(dv), int(max_seq_len), int(num_time_buckets), int(time_bucket_fn == "log"),
           int(time_bucket_unit == "minutes"), float(time_bucket_divisor), 1.0 / math.sqrt(dqk))
    return _HstuAttnFn.apply(proj, pos_w.contiguous(), ts_w.contiguous(), td, km, cfg)


def _head_fwd_workspaces(M, V, dev):
    """part, zlab, lse, wrow, loss of the streaming cross entropy's forward over M rows and V items."""
    nsplit = _lib.call("rh_hstu_head_nsplit", M, V)
    return (torch.empty((M, nsplit, 2), dtype=torch.float32, device=dev), torch.empty((M,), dtype=torch.float32, device=dev),
            torch.empty((M,), dtype=torch.float32, device=dev), torch.empty((M,), dtype=torch.float32, device=dev),
            torch.empty((), dtype=torch.float32, device=dev))


def _head_dw_slab(M, D, V, dev):
    """The (R, V, D + 1) dW / d_bias partials of the streaming cross entropy's backward; unused when R is 1."""
    R = _lib.call("rh_hstu_head_rsplit", M, D, V)
    return torch.empty((R, V, D + 1) if R > 1 else (1,), dtype=torch.float32, device=dev)


class _NextTokenLossFn(torch.autograd.Function):
    """Mean next-token cross entropy over the item table without the (M, V) logits."""

    @staticmethod
    def forward(ctx, h, w, bias, labels, t1, t2, nce):
        h, w = h.contiguous(), w.contiguous()
        M, D = (int(v) for v in h.shape)
        V = int(w.shape[0])
        part, zlab, lse, wrow, loss = _head_fwd_workspaces(M, V, h.device)
        _lib.call("rh_hstu_head_fwd", _p(h), _p(w), _p(bias), _p(labels), M, D, V, t1, t2, int(nce), _p(part), _p(zlab),
                  _p(lse), _p(wrow), _p(loss), _p(err_flag(h.device)), _stream())
        ctx.t = (t1, t2)
        ctx.has_bias = bias is not None
        ctx.save_for_backward(h, w, bias, labels, lse, wrow)
        return loss

    @staticmethod
    def backward(ctx, g):
        h, w, bias, labels, lse, wrow = ctx.saved_tensors
        M, D = (int(v) for v in h.shape)
        V = int(w.shape[0])
        t1, t2 = ctx.t
        dev = h.device
        g_h = torch.empty_like(h)
        if not (ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2])):
            # a frozen head (HLLM's item embeddings): no (V, D) gradient, no partials, no dW kernel
            _lib.call("rh_hstu_head_bwd", _p(h), _p(w), _p(bias), _p(labels), _p(lse), _p(wrow),
                      _p(g.reshape(1).contiguous()), M, D, V, t1, t2, _NULL, _p(g_h), _NULL, _NULL, _stream())
            return g_h, None, None, None, None, None, None
        part = _head_dw_slab(M, D, V, dev)
        g_w = torch.empty_like(w)
        g_b = torch.empty((V,), dtype=torch.float32, device=dev) if ctx.has_bias else None
        _lib.call("rh_hstu_head_bwd", _p(h), _p(w), _p(bias), _p(labels), _p(lse), _p(wrow), _p(g.reshape(1).contiguous()),
                  M, D, V, t1, t2, _p(part), _p(g_h), _p(g_w), _p(g_b), _stream())
        return g_h, g_w, g_b, None, None, None, None


def next_token_loss(h, weight, bias, labels, temperature=1.0, nce_temperature=None):
    """Mean cross entropy of the next-token logits z = ((h weight^T + bias) / temperature) [/ nce_temperature] over the
    rows whose label is not 0, column 0 excluded (SeqTrainer._compute_next_token_loss with ignore_index 0).  h (M, D),
    weight (V, D), bias (V,) or None, labels (M,) int64.  nce_temperature given: NCELoss (mean over every row when no
    label is set); else nn.CrossEntropyLoss (NaN then)."""
    require_hip(h, weight, bias, labels)
    if h.dim() != 2 or weight.dim() != 2 or h.shape[1] != weight.shape[1] or weight.shape[0] < 2 or h.shape[0] < 1:
        raise RuntimeError(f"torch_rechub_amd: next-token head of h {tuple(h.shape)} and weight {tuple(weight.shape)} "
                           "unsupported (h (M, D), weight (V, D), M >= 1, V >= 2)")
    if h.dtype != torch.float32 or weight.dtype != torch.float32:
        raise RuntimeError("torch_rechub_amd: the next-token head runs in float32 only")
    nce = nce_temperature is not None
    return _NextTokenLossFn.apply(h, weight, bias, labels.to(torch.int64).contiguous(), float(temperature),
                                  float(nce_temperature) if nce else 1.0, nce)


# --------------------------------------------------------------------------------------------
# HLLM: causal softmax attention with the bucketed relative-position bias and dropout (csrc/hllm.hip)
# --------------------------------------------------------------------------------------------
class _SoftmaxAttnFn(torch.autograd.Function):
    """(B, L, H dh) = dropout(softmax_j(scale q k^T + bias, causal)) v; keeps the rows' log-sum-exp, never the weights."""

    @staticmethod
    def forward(ctx, q, k, v, bias, cfg):
        H, dh, N, nb, scale, p = cfg
        B, L = int(q.shape[0]), int(q.shape[1])
        ld = int(q.stride(1))
        dev = q.device
        out = torch.empty((B, L, H * dh), dtype=torch.float32, device=dev)
        lse = torch.empty((B, H, L), dtype=torch.float32, device=dev)
        rng = _dropout_rng(dev) if p > 0 else None
        ctr = torch.empty(1, dtype=torch.int64, device=dev) if p > 0 else None
        _lib.call("rh_softmax_attn_fwd", _p(q), _p(k), _p(v), ld, B, L, H, dh, _p(bias), N, nb, scale, p, _p(rng), _p(ctr),
                  _p(out), _p(lse), _stream())
        ctx.cfg = cfg
        ctx.save_for_backward(q, k, v, bias, out, lse, rng, ctr)
        return out

    @staticmethod
    def backward(ctx, g):
        q, k, v, bias, out, lse, rng, ctr = ctx.saved_tensors
        H, dh, N, nb, scale, p = ctx.cfg
        B, L = int(q.shape[0]), int(q.shape[1])
        dev = q.device
        g = g.contiguous()
        g_qkv = torch.empty((3, B, L, H * dh), dtype=torch.float32, device=dev)
        g_bias = torch.empty_like(bias) if bias is not None else None
        if B == 0:
            return g_qkv[0], g_qkv[1], g_qkv[2], None if bias is None else torch.zeros_like(bias), None
        delta = torch.empty((B, H, L), dtype=torch.float32, device=dev)
        part = None
        if bias is not None:
            part = torch.empty((_lib.call("rh_softmax_attn_nparts", B, L, H), L), dtype=torch.float32, device=dev)
        _lib.call("rh_softmax_attn_bwd", _p(q), _p(k), _p(v), int(q.stride(1)), B, L, H, dh, _p(bias), N, nb, scale, p,
                  _p(rng), _p(ctr), _p(out), _p(lse), _p(g), _p(delta), _p(g_qkv[0]), _p(g_qkv[1]), _p(g_qkv[2]), H * dh,
                  _p(part), _p(g_bias), _stream())
        return g_qkv[0], g_qkv[1], g_qkv[2], g_bias, None


def _attn_view_ok(t, B, L, W):
    """(B, L, W) with unit column stride and rows B L apart by one stride (a contiguous tensor or a column block of one)."""
    return t.stride(2) == 1 and t.stride(1) >= W and (B <= 1 or t.stride(0) == L * t.stride(1))


def softmax_attention(q, k, v, n_heads, max_seq_len, bias_table=None, dropout_p=0.0, training=True, scale=None):
    """Causal multi-head softmax attention (B, L, H dh) of q, k, v (B, L, H dh): three contiguous projections, or three
    column blocks of one (B, L, 3 H dh) product (fed without a copy when they share the row stride).  ``bias_table``
    (num_buckets, H): RelPosBias's table, added as table[min(|i - j|, max_seq_len) * (num_buckets - 1) // max_seq_len, h].
    Dropout with probability ``dropout_p`` on the attention weights when ``training``.  No padding mask."""
    require_hip(q, k, v, bias_table)
    if q.dim() != 3 or q.shape != k.shape or q.shape != v.shape or q.shape[2] % n_heads != 0:
        raise RuntimeError(f"torch_rechub_amd: softmax attention of q {tuple(q.shape)}, k {tuple(k.shape)}, "
                           f"v {tuple(v.shape)} with {n_heads} heads unsupported (three (B, L, H dh) tensors)")
    if q.dtype != torch.float32 or k.dtype != torch.float32 or v.dtype != torch.float32 or (
            bias_table is not None and bias_table.dtype != torch.float32):
        raise RuntimeError("torch_rechub_amd: softmax attention runs in float32 only")
    B, L, W = (int(x) for x in q.shape)
    H = int(n_heads)
    dh = W // H
    nb = int(bias_table.shape[0]) if bias_table is not None else 0
    if not (1 <= L <= min(int(max_seq_len), _lib.H.RH_ATTN_MAX_L) and 1 <= dh <= _lib.H.RH_ATTN_MAX_DH) or (bias_table is not None and (
            nb < 1 or bias_table.dim() != 2 or bias_table.shape[1] != H)):
        raise RuntimeError(f"torch_rechub_amd: softmax attention with L={L}, head width {dh}, bias table "
                           f"{None if bias_table is None else tuple(bias_table.shape)} has no HIP kernel "
                           f"(1 <= L <= min(max_seq_len, {_lib.H.RH_ATTN_MAX_L}), 1 <= head width <= {_lib.H.RH_ATTN_MAX_DH}, table "
                           "(num_buckets >= 1, H))")
    p = float(dropout_p) if training else 0.0
    if not 0.0 <= p < 1.0:
        raise RuntimeError(f"torch_rechub_amd: attention dropout p={p} has no HIP kernel (0 <= p < 1)")
    if not (_attn_view_ok(q, B, L, W) and _attn_view_ok(k, B, L, W) and _attn_view_ok(v, B, L, W) and
            q.stride(1) == k.stride(1) == v.stride(1)):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
    cfg = (H, dh, int(max_seq_len), nb, float(dh**-0.5 if scale is None else scale), p)
    return _SoftmaxAttnFn.apply(q, k, v, None if bias_table is None else bias_table.contiguous(), cfg)


# --------------------------------------------------------------------------------------------
# Session-based retrieval: general GRU, additive attention pooling, full-catalogue cross entropy
# (csrc/session.hip, csrc/stream_ce.hip)
# --------------------------------------------------------------------------------------------
class _GruLayerFn(torch.autograd.Function):
    """h_all (B, T, H) of one nn.GRU layer from the zero state; xw (B, T, 3H) = x W_ih^T (+ b_ih), rows r | z | n."""

    @staticmethod
    def forward(ctx, xw, w_hh, b_hh):
        B, T, H3 = (int(v) for v in xw.shape)
        H = H3 // 3
        xw, w_hh = xw.contiguous(), w_hh.contiguous()
        b_hh = None if b_hh is None else b_hh.contiguous()
        h_all = torch.empty((B, T, H), dtype=torch.float32, device=xw.device)
        hu = torch.empty((B, T, H3), dtype=torch.float32, device=xw.device)
        _lib.call("rh_gru_fwd", _p(xw), _p(w_hh), _p(b_hh), B, T, H, _p(h_all), _p(hu), _stream())
        ctx.has_bias = b_hh is not None
        ctx.save_for_backward(xw, w_hh, h_all, hu)
        return h_all

    @staticmethod
    def backward(ctx, g):
        xw, w_hh, h_all, hu = ctx.saved_tensors
        B, T, H3 = (int(v) for v in xw.shape)
        H = H3 // 3
        g = g.contiguous()
        d_xw = torch.empty_like(xw)
        d_s = torch.empty_like(xw)
        _lib.call("rh_gru_bwd", _p(xw), _p(w_hh), _p(h_all), _p(hu), _p(g), B, T, H, _p(d_xw), _p(d_s), _stream())
        d_w = d_b = None
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            # dW_hh = d_s^T h_prev over the B T rows (split-batch MFMA kernel), d b_hh its column sums
            h_prev = torch.cat([h_all.new_zeros(B, 1, H), h_all[:, :-1]], dim=1).reshape(B * T, H)
            d_w, d_b = linear_wgrad(d_s.view(B * T, H3), h_prev, want_bias=ctx.has_bias)
        return d_xw, d_w, d_b


def gru_layers_ok(gru_mod, x, batch_first=None):
    bf = gru_mod.batch_first if batch_first is None else batch_first
    return (isinstance(gru_mod, torch.nn.GRU) and not gru_mod.bidirectional and x.dim() == 3 and x.is_cuda and
            x.dtype == torch.float32 and gru_mod.input_size == x.shape[-1] and gru_mod.proj_size == 0 and
            1 <= gru_mod.hidden_size <= _lib.H.RH_GRU_MAX_H and x.shape[1 if bf else 0] >= 1)


def gru_layers(gru_mod, x, batch_first=None):
    """(output, h_n) of a multi-layer ``nn.GRU`` from the zero state, as the module returns them (``batch_first`` either way,
    with or without bias; ``batch_first`` given: the layout of ``x`` and of the output instead of the module's): per layer the input halves of all steps are one ops.linear product and the recurrence one launch
    each way (csrc/session.hip).  1 <= hidden_size <= RH_GRU_MAX_H; inter-layer dropout is not supported in training."""
    require_hip(x)
    bf = gru_mod.batch_first if batch_first is None else batch_first
    if not gru_layers_ok(gru_mod, x, bf):
        raise RuntimeError(f"torch_rechub_amd: nn.GRU(input {gru_mod.input_size}, hidden {gru_mod.hidden_size}, "
                           f"bidirectional={gru_mod.bidirectional}) on {tuple(x.shape)} has no HIP kernel "
                           f"(float32, unidirectional, 1 <= hidden_size <= {_lib.H.RH_GRU_MAX_H})")
    if gru_mod.dropout > 0 and gru_mod.training and gru_mod.num_layers > 1:
        raise RuntimeError("torch_rechub_amd: nn.GRU inter-layer dropout has no HIP kernel")
    h = x if bf else x.transpose(0, 1)
    B, T, _ = (int(v) for v in h.shape)
    H = gru_mod.hidden_size
    last = []
    for k in range(gru_mod.num_layers):
        w_ih, w_hh = getattr(gru_mod, f"weight_ih_l{k}"), getattr(gru_mod, f"weight_hh_l{k}")
        b_ih = getattr(gru_mod, f"bias_ih_l{k}") if gru_mod.bias else None
        b_hh = getattr(gru_mod, f"bias_hh_l{k}") if gru_mod.bias else None
        xw = linear(h.reshape(B * T, h.shape[-1]), w_ih, b_ih).view(B, T, 3 * H)  # (B = 0: -1 would be ambiguous)
        h = _GruLayerFn.apply(xw, w_hh, b_hh)
        last.append(h[:, -1])
    h_n = torch.stack(last, 0)
    return (h if bf else h.transpose(0, 1)), h_n


class _AttnPoolFn(torch.autograd.Function):
    """out (B, Dx) = sum_l a_l X_l (+ add), a = exp(w0 . sigmoid(P + r)) mask / den (csrc/session.hip)."""

    @staticmethod
    def forward(ctx, P, r, w0, mask, X, add, floor_):
        B, L, H = (int(v) for v in P.shape)
        Dx = int(X.shape[2])
        dev = P.device
        out = torch.empty((B, Dx), dtype=torch.float32, device=dev)
        e = torch.empty((B, L), dtype=torch.float32, device=dev)
        sums = torch.empty((B, 2), dtype=torch.float32, device=dev)
        _lib.call("rh_attn_pool_fwd", _p(P), _p(r), _p(w0), _p(mask), _p(X), _p(add), B, L, H, Dx, int(floor_), _p(out), _p(e),
                  _p(sums), _stream())
        ctx.floor_ = int(floor_)
        ctx.has_add = add is not None
        ctx.save_for_backward(P, r, w0, X, e, sums)
        return out

    @staticmethod
    def backward(ctx, g):
        P, r, w0, X, e, sums = ctx.saved_tensors
        B, L, H = (int(v) for v in P.shape)
        Dx = int(X.shape[2])
        dev = P.device
        g = g.contiguous()
        dP = torch.empty_like(P)
        dr = torch.empty((B, H), dtype=torch.float32, device=dev)
        dw0_part = torch.empty((B, H), dtype=torch.float32, device=dev)
        dw0 = torch.empty((H,), dtype=torch.float32, device=dev)
        dX = torch.empty_like(X)
        _lib.call("rh_attn_pool_bwd", _p(P), _p(r), _p(w0), _p(X), _p(e), _p(sums), _p(g), B, L, H, Dx, ctx.floor_, _p(dP),
                  _p(dr), _p(dw0_part), _p(dw0), _p(dX), _stream())
        return dP, dr, dw0.view(w0.shape), None, dX, (g if ctx.has_add else None), None


def additive_attention_pool(P, r, w0, mask, X, add=None, floor=False):
    """Additive attention pooling of NARM / STAMP: s_l = sum_h w0_h sigmoid(P_lh + r_h), a_l = exp(s_l) mask_l / den,
    out (B, Dx) = sum_l a_l X_l (+ add).  den = sum_l exp(s_l) mask_l, or max(that, 1e-12) with ``floor`` (F.normalize(p=1)).
    P (B, L, H), r (B, H), w0 (H,) or (H, 1), mask (B, L) (bool / 0-1), X (B, L, Dx), add (B, Dx) or None."""
    require_hip(P, r, w0, mask, X, add)
    if P.dim() != 3 or X.dim() != 3 or P.shape[:2] != X.shape[:2] or r.shape != (P.shape[0], P.shape[2]) or \
            w0.numel() != P.shape[2] or mask.shape != P.shape[:2] or (add is not None and add.shape != (X.shape[0], X.shape[2])):
        raise RuntimeError(f"torch_rechub_amd: attention pooling shapes P {tuple(P.shape)}, r {tuple(r.shape)}, "
                           f"w0 {tuple(w0.shape)}, mask {tuple(mask.shape)}, X {tuple(X.shape)} do not agree")
    if not (1 <= P.shape[1] <= _lib.H.RH_ATTN_POOL_MAX_L and 1 <= P.shape[2] <= _lib.H.RH_ATTN_POOL_MAX_W and
            1 <= X.shape[2] <= _lib.H.RH_ATTN_POOL_MAX_W):
        raise RuntimeError(f"torch_rechub_amd: attention pooling with L={P.shape[1]}, H={P.shape[2]}, Dx={X.shape[2]} has "
                           f"no HIP kernel (1 <= L <= {_lib.H.RH_ATTN_POOL_MAX_L}, 1 <= H, Dx <= {_lib.H.RH_ATTN_POOL_MAX_W})")
    if any(t.dtype != torch.float32 for t in (P, r, w0, X) + (() if add is None else (add,))):
        raise RuntimeError("torch_rechub_amd: attention pooling runs in float32 only")
    m = mask.to(torch.float32).contiguous()
    return _AttnPoolFn.apply(P.contiguous(), r.contiguous(), w0.contiguous(), m, X.contiguous(),
                             None if add is None else add.contiguous(), bool(floor))


class _CatalogueCEFn(torch.autograd.Function):
    """Mean nn.CrossEntropyLoss of u E^T against labels without the (B, V) logits."""

    @staticmethod
    def forward(ctx, u, E, labels):
        u, E = u.contiguous(), E.contiguous()
        B, D = (int(v) for v in u.shape)
        V = int(E.shape[0])
        part, zlab, lse, wrow, loss = _head_fwd_workspaces(B, V, u.device)
        _lib.call("rh_catalogue_ce_fwd", _p(u), _p(E), _p(labels), B, D, V, _p(part), _p(zlab), _p(lse), _p(wrow), _p(loss),
                  _p(err_flag(u.device)), _stream())
        ctx.save_for_backward(u, E, labels, lse, wrow)
        return loss

    @staticmethod
    def backward(ctx, g):
        u, E, labels, lse, wrow = ctx.saved_tensors
        B, D = (int(v) for v in u.shape)
        V = int(E.shape[0])
        dev = u.device
        Sv = _lib.call("rh_catalogue_ce_vsplit", B, D, V)
        part = _head_dw_slab(B, D, V, dev)
        part_h = torch.empty((Sv, B, D) if Sv > 1 else (1,), dtype=torch.float32, device=dev)
        g_u = torch.empty_like(u)
        g_E = torch.empty_like(E)
        _lib.call("rh_catalogue_ce_bwd", _p(u), _p(E), _p(labels), _p(lse), _p(wrow), _p(g.reshape(1).contiguous()), B, D, V,
                  _p(part), _p(part_h), _p(g_u), _p(g_E), _stream())
        return g_u, g_E, None


def catalogue_cross_entropy(u, weight, labels):
    """torch.nn.CrossEntropyLoss()(u @ weight.T, labels) (mean over every row, every column a class) without forming the
    (B, V) logits.  u (B, D), weight (V, D), labels (B,) integer in [0, V) (out of range: the device error word is set,
    ops.check_errors raises).  The backward returns du and the dense d weight."""
    require_hip(u, weight, labels)
    if u.dim() != 2 or weight.dim() != 2 or u.shape[1] != weight.shape[1] or u.shape[0] < 1 or \
            not (2 <= weight.shape[0] <= 1 << 30) or labels.shape != (u.shape[0],):
        raise RuntimeError(f"torch_rechub_amd: catalogue cross entropy of u {tuple(u.shape)}, weight {tuple(weight.shape)}, "
                           f"labels {tuple(labels.shape)} unsupported (u (B, D), weight (V, D), labels (B,), B >= 1, "
                           "2 <= V <= 2^30)")
    if u.dtype != torch.float32 or weight.dtype != torch.float32:
        raise RuntimeError("torch_rechub_amd: the catalogue cross entropy runs in float32 only")
    return _CatalogueCEFn.apply(u, weight, labels.to(torch.int64).contiguous())


class _DropoutFn(torch.autograd.Function):

    @staticmethod
    def forward(ctx, x, p):
        x = x.contiguous()
        y = torch.empty_like(x)
        rng = _dropout_rng(x.device)
        ctr = torch.empty(1, dtype=torch.int64, device=x.device)
        _lib.call("rh_session_dropout_fwd", _p(x), x.numel(), float(p), _p(rng), _p(ctr), _p(y), _stream())
        ctx.p = float(p)
        ctx.save_for_backward(rng, ctr)
        return y

    @staticmethod
    def backward(ctx, g):
        rng, ctr = ctx.saved_tensors
        g = g.contiguous()
        dx = torch.empty_like(g)
        _lib.call("rh_session_dropout_bwd", _p(g), g.numel(), ctx.p, _p(rng), _p(ctr), _p(dx), _stream())
        return dx, None


def dropout(x, p, training=True):
    """nn.Dropout(p) with the project's counter-hash mask (the fused MLP dropout's stream): identity at p = 0 or in eval;
    the mask is recomputed in the backward, never stored."""
    if not training or p == 0:
        return x
    require_hip(x)
    if not (0 < p < 1) or x.dtype != torch.float32:
        raise RuntimeError(f"torch_rechub_amd: dropout p={p} on {x.dtype} has no HIP kernel (0 <= p < 1, float32)")
    return _DropoutFn.apply(x, p)


def session_lengths(seq, check_full=False):
    """(B,) int64 number of non-zero ids per row of a (B, L) id matrix, one launch.  A row without items (and, with
    ``check_full``, a batch whose longest row is shorter than L) sets the device error word: outside a hipGraph capture this
    checks it at once and raises RuntimeError, inside one the replayed step leaves it for the trainer's error check."""
    require_hip(seq)
    seq = seq.to(torch.int64).contiguous()
    B, L = (int(v) for v in seq.shape)
    counts = torch.empty((B,), dtype=torch.int64, device=seq.device)
    _lib.call("rh_session_lengths", _p(seq), B, L, int(bool(check_full)), _p(counts), _p(err_flag(seq.device)), _stream())
    if not torch.cuda.is_current_stream_capturing():
        check_errors(seq.device)
    return counts


# --------------------------------------------------------------------------------------------
# Exact top-K item retrieval (csrc/topk.hip)
# --------------------------------------------------------------------------------------------
def topk_supported(D, K, S=0):
    """Whether csrc/topk.hip takes width D, K results and S exclusions per query (D <= RH_TOPK_MAX_D, K <= RH_TOPK_MAX_K,
    S <= RH_TOPK_MAX_S)."""
    return bool(_lib.query("rh_topk_supported", int(D), int(K), int(S)))


def topk_plan(M, V, K):
    """(nsplit, workspace_bytes): the default number of item ranges for M queries over V items and the size of the
    partial lists for it (8 M nsplit K bytes)."""
    return _lib.query("rh_topk_plan", int(M), int(V), int(K), out=(ctypes.c_int, ctypes.c_int64))


def _scan_inputs(what, tname, q, table, k, bias, exclude, refuse):
    """What ``topk_items`` and ``ivf_scan`` check and prepare alike: q (M, D) and the table (V, D; ``tname`` in the
    messages) float32, the table contiguous, bias (V,) float32, exclude (M, S).  ``refuse(M, D, V, k, S)`` makes the
    caller's own checks and raises where there is no kernel, before anything is allocated.  Returns q with unit column
    stride and its row stride, bias and exclude as the kernels read them, S and the empty (ids, scores) (M, k)."""
    if q.dim() != 2 or table.dim() != 2 or q.shape[1] != table.shape[1]:
        raise ValueError(f"{what}: q (M, D) and {tname} (V, D) expected")
    if q.dtype != torch.float32 or table.dtype != torch.float32 or (bias is not None and bias.dtype != torch.float32):
        raise ValueError(f"torch_rechub_amd: {what} takes float32 tensors")
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
    q = q.detach()
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
    id -1, score -inf.  ``nsplit`` forces the number of item ranges (the result does not depend on it).  No autograd;
    runs on the current stream."""
    if invalid is not None and not torch.is_tensor(invalid):
        invalid = torch.as_tensor(list(invalid), dtype=torch.int64, device=q.device)
    require_hip(q, table, bias, exclude, invalid)

    def refuse(M, D, V, k, S):
        if V < 1 or not topk_supported(D, k, S):
            from .models.matching._listwise import no_kernel
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
    _lib.call("rh_topk_fwd", _p(q), ldq, _p(table.detach()), _p(bias), _p(exclude) if S > 0 else _NULL, S,
              _p(invalid) if n_inv > 0 else _NULL, n_inv, M, D, V, k, nsplit, _p(work), _p(ids), _p(scores), _stream())
    return ids, scores


# --------------------------------------------------------------------------------------------
# Inverted-file index: the list scan and the k-means update (csrc/ivf.hip)
# --------------------------------------------------------------------------------------------
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


def ivf_scan(q, table_sorted, row_ids, list_offsets, probe, k, bias=None, exclude=None):
    """(ids (M, k) int64, scores (M, k) float32): the k best rows for every row of ``q`` (M, D) by q_i . x_j (+ bias[j])
    among the lists it probes, best first, exact ties to the lower id; ``topk_items`` restricted to a union of lists.
    ``table_sorted`` (V, D) holds the table's rows grouped by list, ``bias`` (V,) alike, ``row_ids`` (V,) int32 the original
    id of every grouped row (ascending inside each list: a stable sort by list gives that), ``list_offsets`` (nlists + 1,)
    int32 the lists' offsets.  ``probe`` (M, nprobe) int32: the lists of each query, distinct per row; an entry outside
    [0, nlists) (-1) is no list.  ``exclude`` (M, S) int64: original ids that may not be returned to query i (anything
    else is padding).  The returned ids are original ids; with fewer than k candidates the tail is id -1, score -inf.
    With every list probed the result is ``topk_items``' on the un-grouped table, bit for bit.  The pairs are grouped by
    list with a stable ``torch.sort``; nothing synchronises with the host.  No autograd; runs on the current stream."""
    require_hip(q, table_sorted, row_ids, list_offsets, probe, bias, exclude)

    def refuse(M, D, V, k, S):
        if row_ids.dtype != torch.int32 or list_offsets.dtype != torch.int32 or probe.dtype != torch.int32:
            raise ValueError("ivf_scan: row_ids, list_offsets and probe are int32 tensors")
        if tuple(row_ids.shape) != (V,) or list_offsets.dim() != 1 or list_offsets.shape[0] < 2:
            raise ValueError("ivf_scan: row_ids (V,) and list_offsets (nlists + 1,) expected")
        if probe.dim() != 2 or probe.shape[0] != M:
            raise ValueError("ivf_scan: probe (M, nprobe) expected")
        nlists, nprobe = int(list_offsets.shape[0]) - 1, int(probe.shape[1])
        if V < 1 or M * nprobe >= 2 ** 31 - 64 * (nlists + 2) or not ivf_supported(D, k, S, nprobe):
            from .models.matching._listwise import no_kernel
            raise no_kernel(f"the inverted-file scan at D={D}, k={k}, {S} exclusions per query, nprobe={nprobe}, V={V} "
                            f"(1 <= D <= {_lib.H.RH_TOPK_MAX_D}, 1 <= k <= {_lib.H.RH_TOPK_MAX_K}, S <= {_lib.H.RH_TOPK_MAX_S}, "
                            f"1 <= nprobe <= {_lib.H.RH_IVF_MAX_NPROBE}, V >= 1, M nprobe < 2^31)")

    q, ldq, bias, exclude, S, ids, scores = _scan_inputs("ivf_scan", "table_sorted", q, table_sorted, k, bias, exclude,
                                                         refuse)
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
    _lib.call("rh_ivf_scan", _p(q), ldq, _p(table_sorted), _p(bias), _p(row_ids), _p(list_offsets), nlists, _p(pair),
              _p(pair_off), _p(tile_off), _p(exclude) if S > 0 else _NULL, S, M, D, V, k, nprobe, _p(part), _p(ids),
              _p(scores), _stream())
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
        from .models.matching._listwise import no_kernel
        raise no_kernel(f"the list mean over V={V} rows (V < 2^31)")
    previous, list_offsets = previous.detach().contiguous(), list_offsets.contiguous()
    out = torch.empty_like(previous)
    _lib.call("rh_ivf_list_mean", _p(x_sorted.detach()), _p(list_offsets), _p(previous), V, D, nlists, _p(out), _stream())
    return out


# --------------------------------------------------------------------------------------------
# SASRec: the transformer block around ops.softmax_attention, fused per row tile (csrc/sasrec.hip)
# --------------------------------------------------------------------------------------------
def _sasrec_check(what, D, *tensors):
    """Before anything is allocated or launched: float32 tensors and a width the kernels take."""
    if any(t is not None and t.dtype != torch.float32 for t in tensors):
        raise ValueError(f"torch_rechub_amd: {what} takes float32 tensors")
    if not 1 <= int(D) <= _lib.H.RH_SASREC_MAX_D:
        from .models.matching._listwise import no_kernel
        raise no_kernel(f"{what} at width {int(D)} (1 <= D <= {_lib.H.RH_SASREC_MAX_D})")


def _sasrec_ntiles(M, D):
    return _lib.query("rh_sasrec_ntiles", int(M), int(D))


def _ln_param_grads(part, D):
    """(g_gamma, g_beta) (D,) from the per-workgroup partials (n, 2, D), summed in a fixed order."""
    out = torch.empty((2 * D,), dtype=torch.float32, device=part.device)
    _lib.call("rh_colsum", _p(part), int(part.shape[0]), 2 * D, _p(out), _NULL, 0, _NULL, _stream())
    return out[:D], out[D:]


def _sample_view(t, B, L, D):
    """A (B, L, D) tensor as the kernels read it: unit column stride, rows and samples one stride apart each (a slice of
    the (B, 3, L, >= D) gather, or a contiguous tensor) -> (tensor, sample stride, row stride)."""
    if not (t.stride(2) == 1 and t.stride(1) >= D and t.stride(0) >= L * t.stride(1)):
        t = t.contiguous()
    return t, int(t.stride(0)), int(t.stride(1))


class _SasrecInputFn(torch.autograd.Function):
    """x0 (B, L, D) = m dropout(e sqrt(D) + P[l]), m = seq != 0."""

    @staticmethod
    def forward(ctx, seq, e, P, p):
        B, L, D = (int(v) for v in e.shape)
        dev = e.device
        e, ebs, ers = _sample_view(e, B, L, D)
        x0 = torch.empty((B, L, D), dtype=torch.float32, device=dev)
        rng = _dropout_rng(dev) if p > 0 else None
        ctr = torch.empty(1, dtype=torch.int64, device=dev) if p > 0 else None
        scale = float(torch.tensor(float(D)**0.5, dtype=torch.float32))
        _lib.call("rh_sasrec_input_fwd", _p(seq), _p(e), ebs, ers, _p(P), B, L, D, int(P.shape[0]), scale, p, _p(rng), _p(ctr),
                  _p(x0), _stream())
        ctx.cfg = (B, L, D, int(P.shape[0]), scale, p)
        ctx.save_for_backward(seq, rng, ctr)
        return x0

    @staticmethod
    def backward(ctx, g):
        seq, rng, ctr = ctx.saved_tensors
        B, L, D, max_len, scale, p = ctx.cfg
        g = g.contiguous()
        g_e = torch.empty((B, L, D), dtype=torch.float32, device=g.device)
        g_P = torch.empty((max_len, D), dtype=torch.float32, device=g.device)
        _lib.call("rh_sasrec_input_bwd", _p(seq), _p(g), B, L, D, max_len, scale, p, _p(rng), _p(ctr), _p(g_e), _p(g_P),
                  _stream())
        return None, g_e, g_P, None


def _seq_ids(seq, B, L):
    if seq.dim() != 2 or tuple(seq.shape) != (B, L):
        raise ValueError(f"torch_rechub_amd: the history ids must be (B, L) = ({B}, {L}), got {tuple(seq.shape)}")
    return seq.to(torch.int64).contiguous()


def _drop_p(p, training):
    p = float(p) if training else 0.0
    if not 0.0 <= p < 1.0:
        raise RuntimeError(f"torch_rechub_amd: dropout p={p} has no HIP kernel (0 <= p < 1)")
    return p


def sasrec_input(seq, e, P, dropout_p=0.0, training=True):
    """SASRec's input stage x0 (B, L, D) = m dropout(e sqrt(D) + P[:L]) from the history ids seq (B, L) (0 = pad, m = seq
    != 0), their gathered rows e (B, L, D) (a slice of the (B, 3, L, D) gather is read in place) and the position table P
    (max_len, D), L <= max_len."""
    require_hip(seq, e, P)
    if e.dim() != 3 or P.dim() != 2 or P.shape[1] != e.shape[2]:
        raise ValueError("sasrec_input: e (B, L, D) and P (max_len, D) expected")
    B, L, D = (int(v) for v in e.shape)
    _sasrec_check("SASRec's input stage", D, e, P)
    if L > P.shape[0]:
        raise IndexError("index out of range in self")  # the reference's position lookup fails with this error
    return _SasrecInputFn.apply(_seq_ids(seq, B, L), e, P.contiguous(), _drop_p(dropout_p, training))


class _SasrecAttnInFn(torch.autograd.Function):
    """(Q (M, D), qkv (M, 3 D)) = (LN(x), [Q Wq^T + bq | x Wk^T + bk | x Wv^T + bv])."""

    @staticmethod
    def forward(ctx, x, gamma, beta, w, b, eps):
        M, D = (int(v) for v in x.shape)
        dev = x.device
        Q = torch.empty((M, D), dtype=torch.float32, device=dev)
        qkv = torch.empty((M, 3 * D), dtype=torch.float32, device=dev)
        stats = torch.empty((M, 2), dtype=torch.float32, device=dev)
        _lib.call("rh_sasrec_attn_in_fwd", _p(x), _p(gamma), _p(beta), eps, _p(w), _p(b), M, D, _p(Q), _p(qkv), _p(stats),
                  _stream())
        ctx.save_for_backward(x, gamma, w, Q, stats)
        return Q, qkv

    @staticmethod
    def backward(ctx, g_Q, g_qkv):
        x, gamma, w, Q, stats = ctx.saved_tensors
        M, D = (int(v) for v in x.shape)
        dev = x.device
        g_Q, g_qkv = g_Q.contiguous(), g_qkv.contiguous()
        g_x = torch.empty((M, D), dtype=torch.float32, device=dev)
        g_w = torch.empty((3 * D, D), dtype=torch.float32, device=dev)
        g_b = torch.empty((3 * D,), dtype=torch.float32, device=dev)
        if M == 0:
            z = torch.zeros((D,), dtype=torch.float32, device=dev)
            return g_x, z, z.clone(), g_w.zero_(), g_b.zero_(), None
        part = torch.empty((_sasrec_ntiles(M, D), 2, D), dtype=torch.float32, device=dev)
        _lib.call("rh_sasrec_attn_in_bwd", _p(x), _p(gamma), _p(w), _p(stats), _p(g_qkv), _p(g_Q), M, D, _p(g_x), _p(part),
                  _stream())
        g_gamma, g_beta = _ln_param_grads(part, D)
        linear_wgrad(g_qkv[:, :D], Q, out=(g_w[:D], g_b[:D]))
        linear_wgrad(g_qkv[:, D:], x, out=(g_w[D:], g_b[D:]))
        return g_x, g_gamma, g_beta, g_w, g_b, None


def sasrec_attention_in(x, ln_weight, ln_bias, in_proj_weight, in_proj_bias, eps=1e-8):
    """(Q, qkv) for one SASRec block from x (..., D): Q = LayerNorm(x) (the attention's query input and the block's
    residual) and qkv (..., 3 D) = the in-projection of nn.MultiheadAttention with query Q and key = value = x.  The three
    column blocks of qkv feed ops.softmax_attention without a copy."""
    require_hip(x, ln_weight, ln_bias, in_proj_weight, in_proj_bias)
    D = int(x.shape[-1])
    _sasrec_check("SASRec's LayerNorm + in-projection", D, x, ln_weight, ln_bias, in_proj_weight, in_proj_bias)
    if tuple(in_proj_weight.shape) != (3 * D, D) or tuple(in_proj_bias.shape) != (3 * D,) or \
            tuple(ln_weight.shape) != (D,) or tuple(ln_bias.shape) != (D,):
        raise ValueError("sasrec_attention_in: LayerNorm (D,), in_proj_weight (3 D, D), in_proj_bias (3 D,) expected")
    lead = tuple(x.shape[:-1])
    Q, qkv = _SasrecAttnInFn.apply(x.reshape(-1, D).contiguous(), ln_weight.contiguous(), ln_bias.contiguous(),
                                   in_proj_weight.contiguous(), in_proj_bias.contiguous(), float(eps))
    return Q.view(lead + (D,)), qkv.view(lead + (3 * D,))


class _SasrecFfnFn(torch.autograd.Function):
    """out = m (z + dropout2(W2 relu(dropout1(W1 z + b1)) + b2)), z = LN(Q + attn Wo^T + bo); one launch each way, the
    D x D weight gradients by rh_linear_wgrad on the operands the backward emits."""

    @staticmethod
    def forward(ctx, attn, Q, seq, wo, bo, gamma, beta, w1, b1, w2, b2, eps, p):
        M, D = (int(v) for v in attn.shape)
        dev = attn.device
        y, z, a, out = (torch.empty((M, D), dtype=torch.float32, device=dev) for _ in range(4))
        stats = torch.empty((M, 2), dtype=torch.float32, device=dev)
        rng = _dropout_rng(dev) if p > 0 else None
        ctr = torch.empty(1, dtype=torch.int64, device=dev) if p > 0 else None
        _lib.call("rh_sasrec_ffn_fwd", _p(attn), _p(Q), _p(seq), _p(wo), _p(bo), _p(gamma), _p(beta), eps, _p(w1), _p(b1),
                  _p(w2), _p(b2), M, D, p, _p(rng), _p(ctr), _p(y), _p(z), _p(a), _p(stats), _p(out), _stream())
        ctx.p = p
        ctx.save_for_backward(attn, seq, wo, gamma, w1, w2, y, z, a, stats, rng, ctr)
        return out

    @staticmethod
    def backward(ctx, g):
        attn, seq, wo, gamma, w1, w2, y, z, a, stats, rng, ctr = ctx.saved_tensors
        M, D = (int(v) for v in attn.shape)
        dev = attn.device
        g = g.contiguous()
        g_f, g_h, g_Q, g_attn = (torch.empty((M, D), dtype=torch.float32, device=dev) for _ in range(4))
        g_w = torch.empty((3, D, D), dtype=torch.float32, device=dev)  # Wo, W1, W2
        g_b = torch.empty((3, D), dtype=torch.float32, device=dev)
        if M == 0:
            zero = torch.zeros((D,), dtype=torch.float32, device=dev)
            g_w.zero_(), g_b.zero_()
            return (g_attn, g_Q, None, g_w[0], g_b[0], zero, zero.clone(), g_w[1].view(w1.shape), g_b[1],
                    g_w[2].view(w2.shape), g_b[2], None, None)
        part = torch.empty((_sasrec_ntiles(M, D), 2, D), dtype=torch.float32, device=dev)
        _lib.call("rh_sasrec_ffn_bwd", _p(seq), _p(wo), _p(gamma), _p(w1), _p(w2), _p(y), _p(a), _p(stats), _p(g), M, D, ctx.p,
                  _p(rng), _p(ctr), _p(g_f), _p(g_h), _p(g_Q), _p(g_attn), _p(part), _stream())
        g_gamma, g_beta = _ln_param_grads(part, D)
        linear_wgrad(g_Q, attn, out=(g_w[0], g_b[0]))
        linear_wgrad(g_h, z, out=(g_w[1], g_b[1]))
        linear_wgrad(g_f, a, out=(g_w[2], g_b[2]))
        return (g_attn, g_Q, None, g_w[0], g_b[0], g_gamma, g_beta, g_w[1].view(w1.shape), g_b[1], g_w[2].view(w2.shape),
                g_b[2], None, None)


def sasrec_ffn(attn, Q, seq, out_proj_weight, out_proj_bias, ln_weight, ln_bias, w1, b1, w2, b2, eps=1e-8, dropout_p=0.0,
               training=True):
    """The second half of a SASRec block, (B, L, D): y = Q + attn Wo^T + bo, z = LayerNorm(y), out = m (z + dropout(W2
    relu(dropout(W1 z + b1)) + b2)) with m = seq != 0.  attn (B, L, D) is the heads' output (ops.softmax_attention), Q the
    normalised query (ops.sasrec_attention_in); w1 / w2 are (D, D) or Conv1d's (D, D, 1)."""
    require_hip(attn, Q, seq, out_proj_weight, out_proj_bias, ln_weight, ln_bias, w1, b1, w2, b2)
    if attn.dim() != 3 or attn.shape != Q.shape:
        raise ValueError("sasrec_ffn: attn and Q (B, L, D) expected")
    B, L, D = (int(v) for v in attn.shape)
    _sasrec_check("SASRec's out-projection + FFN", D, attn, Q, out_proj_weight, out_proj_bias, ln_weight, ln_bias, w1, b1, w2,
                  b2)
    if any(w.numel() != D * D for w in (out_proj_weight, w1, w2)) or any(
            tuple(v.shape) != (D,) for v in (out_proj_bias, ln_weight, ln_bias, b1, b2)):
        raise ValueError("sasrec_ffn: three (D, D) weights and five (D,) vectors expected")
    out = _SasrecFfnFn.apply(attn.reshape(B * L, D).contiguous(), Q.reshape(B * L, D).contiguous(), _seq_ids(seq, B, L),
                             out_proj_weight.contiguous(), out_proj_bias.contiguous(), ln_weight.contiguous(),
                             ln_bias.contiguous(), w1.contiguous(), b1.contiguous(), w2.contiguous(), b2.contiguous(),
                             float(eps), _drop_p(dropout_p, training))
    return out.view(B, L, D)


class _SasrecHeadFn(torch.autograd.Function):
    """(pos_logits, neg_logits) (B, L) = LN(x) . pos_e, LN(x) . neg_e."""

    @staticmethod
    def forward(ctx, x, gamma, beta, pos_e, neg_e, eps):
        B, L, D = (int(v) for v in x.shape)
        dev = x.device
        pos_e, pbs, prs = _sample_view(pos_e, B, L, D)
        neg_e, nbs, nrs = _sample_view(neg_e, B, L, D)
        if prs != nrs:
            pos_e, pbs, prs = pos_e.contiguous(), L * D, D
            neg_e, nbs, nrs = neg_e.contiguous(), L * D, D
        pos = torch.empty((B, L), dtype=torch.float32, device=dev)
        neg = torch.empty((B, L), dtype=torch.float32, device=dev)
        stats = torch.empty((B * L, 2), dtype=torch.float32, device=dev)
        _lib.call("rh_sasrec_head_fwd", _p(x), _p(gamma), _p(beta), eps, _p(pos_e), pbs, _p(neg_e), nbs, prs, B, L, D, _NULL,
                  _p(pos), _p(neg), _p(stats), _stream())
        ctx.strides = (pbs, nbs, prs)
        ctx.save_for_backward(x, gamma, beta, pos_e, neg_e, stats)
        return pos, neg

    @staticmethod
    def backward(ctx, g_pos, g_neg):
        x, gamma, beta, pos_e, neg_e, stats = ctx.saved_tensors
        B, L, D = (int(v) for v in x.shape)
        dev = x.device
        g_pos, g_neg = g_pos.contiguous(), g_neg.contiguous()
        g_x, g_pe, g_ne = (torch.empty((B, L, D), dtype=torch.float32, device=dev) for _ in range(3))
        if B * L == 0:
            z = torch.zeros((D,), dtype=torch.float32, device=dev)
            return g_x, z, z.clone(), g_pe, g_ne, None
        part = torch.empty((-(-B * L // 64), 2, D), dtype=torch.float32, device=dev)
        _lib.call("rh_sasrec_head_bwd", _p(x), _p(gamma), _p(beta), _p(stats), _p(pos_e), ctx.strides[0], _p(neg_e),
                  ctx.strides[1], ctx.strides[2], _NULL, _p(g_pos), _p(g_neg), B, L, D, _p(g_x), _p(g_pe), _p(g_ne), _p(part), _stream())
        g_gamma, g_beta = _ln_param_grads(part, D)
        return g_x, g_gamma, g_beta, g_pe, g_ne, None


class _LayerNormFn(torch.autograd.Function):
    """LayerNorm over the last axis of (M, D) (the head kernels without their products)."""

    @staticmethod
    def forward(ctx, x, gamma, beta, eps):
        M, D = (int(v) for v in x.shape)
        s = torch.empty((M, D), dtype=torch.float32, device=x.device)
        stats = torch.empty((M, 2), dtype=torch.float32, device=x.device)
        _lib.call("rh_sasrec_head_fwd", _p(x), _p(gamma), _p(beta), eps, _NULL, 0, _NULL, 0, 0, M, 1, D, _p(s), _NULL, _NULL,
                  _p(stats), _stream())
        ctx.save_for_backward(x, gamma, beta, stats)
        return s

    @staticmethod
    def backward(ctx, g):
        x, gamma, beta, stats = ctx.saved_tensors
        M, D = (int(v) for v in x.shape)
        dev = x.device
        g = g.contiguous()
        g_x = torch.empty((M, D), dtype=torch.float32, device=dev)
        if M == 0:
            z = torch.zeros((D,), dtype=torch.float32, device=dev)
            return g_x, z, z.clone(), None
        part = torch.empty((-(-M // 64), 2, D), dtype=torch.float32, device=dev)
        _lib.call("rh_sasrec_head_bwd", _p(x), _p(gamma), _p(beta), _p(stats), _NULL, 0, _NULL, 0, 0, _p(g), _NULL, _NULL, M, 1,
                  D, _p(g_x), _NULL, _NULL, _p(part), _stream())
        g_gamma, g_beta = _ln_param_grads(part, D)
        return g_x, g_gamma, g_beta, None


def layer_norm(x, weight, bias, eps=1e-5):
    """F.layer_norm(x, (D,), weight, bias, eps) over the last axis of a float32 (..., D) tensor, D <= RH_SASREC_MAX_D: two-pass
    variance, so an all-zero row gives exactly ``bias``; the weight and bias gradients are summed in a fixed order."""
    require_hip(x, weight, bias)
    D = int(x.shape[-1])
    _sasrec_check("LayerNorm", D, x, weight, bias)
    if tuple(weight.shape) != (D,) or tuple(bias.shape) != (D,):
        raise ValueError("layer_norm: weight and bias (D,) expected")
    out = _LayerNormFn.apply(x.reshape(-1, D).contiguous(), weight.contiguous(), bias.contiguous(), float(eps))
    return out.view(x.shape)


def sasrec_head(x, ln_weight, ln_bias, pos_e, neg_e, eps=1e-8):
    """SASRec's training head: (pos_logits, neg_logits) (B, L) = sum_d LayerNorm(x) pos_e, sum_d LayerNorm(x) neg_e for x,
    pos_e, neg_e (B, L, D); pos_e / neg_e may be slices of the (B, 3, L, D) gather (read in place)."""
    require_hip(x, ln_weight, ln_bias, pos_e, neg_e)
    if x.dim() != 3 or pos_e.shape != x.shape or neg_e.shape != x.shape:
        raise ValueError("sasrec_head: x, pos_e, neg_e (B, L, D) expected")
    D = int(x.shape[2])
    _sasrec_check("SASRec's final LayerNorm + logits", D, x, ln_weight, ln_bias, pos_e, neg_e)
    if tuple(ln_weight.shape) != (D,) or tuple(ln_bias.shape) != (D,):
        raise ValueError("sasrec_head: LayerNorm weight and bias (D,) expected")
    return _SasrecHeadFn.apply(x.contiguous(), ln_weight.contiguous(), ln_bias.contiguous(), pos_e, neg_e, float(eps))


# --------------------------------------------------------------------------------------------
# two-tower score tails and the SENET field gate (csrc/twotower.hip)
# --------------------------------------------------------------------------------------------
def _rows(t):
    """A float32 (B, D) tensor whose rows are contiguous (any row stride), as the row-strided entry points read it."""
    return t if t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()


class _BandLogitsFn(torch.autograd.Function):
    """YoutubeSBC's (B, 1 + n_neg) scores straight from the tower outputs: no (B, B) tensor; the item gradient is a gather."""

    @staticmethod
    def forward(ctx, u, v, w, K1, temperature, eps):
        require_hip(u, v, w)
        u, v, w = _rows(u), _rows(v), w.contiguous()
        B, D = u.shape
        dev = u.device
        logits = torch.empty((B, K1), dtype=torch.float32, device=dev)
        norms = torch.empty((2, B), dtype=torch.float32, device=dev)
        _lib.call("rh_band_logits_fwd", _p(u), u.stride(0), _p(v), v.stride(0), _p(w), B, D, K1, temperature, eps, _p(logits),
                  _p(norms[0]), _p(norms[1]), _stream())
        ctx.save_for_backward(u, v, norms)
        ctx.cfg = (K1, temperature, eps)
        return logits

    @staticmethod
    def backward(ctx, g):
        u, v, norms = ctx.saved_tensors
        K1, temperature, eps = ctx.cfg
        B, D = u.shape
        g = g.contiguous()
        g_u = torch.empty((B, D), dtype=torch.float32, device=u.device)
        g_v = torch.empty((B, D), dtype=torch.float32, device=u.device)
        _lib.call("rh_band_logits_bwd", _p(u), u.stride(0), _p(v), v.stride(0), _p(norms[0]), _p(norms[1]), _p(g), B, D, K1,
                  temperature, eps, _p(g_u), _p(g_v), _stream())
        return g_u, g_v, None, None, None, None


def _f32_rows(*tensors):
    first = tensors[0]
    return all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape == first.shape for t in tensors) and \
        first.shape[0] >= 1 and 1 <= first.shape[1] <= _lib.H.RH_TWOTOWER_MAX_D


def band_logits_ok(u, v, w, n_neg):
    return (_f32_rows(u, v) and w.is_cuda and w.dtype == torch.float32 and tuple(w.shape) == (u.shape[0],) and
            0 <= int(n_neg) < u.shape[0])


def band_logits(u, v, w, n_neg, temperature=1.0, eps=1e-8):
    """logits[i, k] = (cosine_similarity(u_i, v_j, eps) - log w_j) / temperature with j = (i + k) mod B, k = 0..n_neg:
    ``((torch.cosine_similarity(u.unsqueeze(1), v, dim=2) - torch.log(w))[index0, index1] / temperature).view(B, -1)`` for
    YoutubeSBC's band ``index1 = (i + k) mod B``.  ``w`` gets no gradient (it is a DenseFeature input)."""
    return _BandLogitsFn.apply(u, v, w, int(n_neg) + 1, float(temperature), float(eps))


class _PairCosineFn(torch.autograd.Function):
    """(sum(n(hu) n(hp)), sum(n(hu) n(hn))), n = F.normalize(., p=2, dim=1, eps): one launch each way."""

    @staticmethod
    def forward(ctx, hu, hp, hn, eps):
        require_hip(hu, hp, hn)
        hu, hp, hn = _rows(hu), _rows(hp), _rows(hn)
        B, D = hu.shape
        dev = hu.device
        score = torch.empty((2, B), dtype=torch.float32, device=dev)
        nrm = torch.empty((3, B), dtype=torch.float32, device=dev)
        _lib.call("rh_pair_cosine_fwd", _p(hu), hu.stride(0), _p(hp), hp.stride(0), _p(hn), hn.stride(0), B, D, eps,
                  _p(score[0]), _p(score[1]), _p(nrm), _stream())
        ctx.save_for_backward(hu, hp, hn, nrm)
        ctx.eps = eps
        return score[0], score[1]

    @staticmethod
    def backward(ctx, g_pos, g_neg):
        hu, hp, hn, nrm = ctx.saved_tensors
        B, D = hu.shape
        g_pos, g_neg = g_pos.contiguous(), g_neg.contiguous()
        grads = torch.empty((3, B, D), dtype=torch.float32, device=hu.device)
        _lib.call("rh_pair_cosine_bwd", _p(hu), hu.stride(0), _p(hp), hp.stride(0), _p(hn), hn.stride(0), _p(nrm), _p(g_pos),
                  _p(g_neg), B, D, ctx.eps, _p(grads[0]), _p(grads[1]), _p(grads[2]), _stream())
        return grads[0], grads[1], grads[2], None


def pair_cosine_scores_ok(hu, hp, hn):
    return _f32_rows(hu, hp, hn)


def pair_cosine_scores(hu, hp, hn, eps=1e-12):
    """(pos, neg) (B,) each: the cosine of every user row with its positive and its negative item row, from the RAW tower
    outputs -- ``(F.normalize(hu) * F.normalize(hp)).sum(1), (F.normalize(hu) * F.normalize(hn)).sum(1)``."""
    return _PairCosineFn.apply(hu, hp, hn, float(eps))


class _SenetFn(torch.autograd.Function):
    """SENETLayer.forward over the (B, F, D) field block; the weight gradients through per-workgroup partials + rh_colsum."""

    @staticmethod
    def forward(ctx, x, w1, w2):
        require_hip(x, w1, w2)
        B, F, D = x.shape
        if x.stride(2) != 1 or x.stride(1) != D or x.stride(0) < F * D:
            x = x.contiguous()
        w1, w2 = w1.contiguous(), w2.contiguous()
        R = w1.shape[0]
        dev = x.device
        y = torch.empty((B, F, D), dtype=torch.float32, device=dev)
        z = torch.empty((B, F), dtype=torch.float32, device=dev)
        h = torch.empty((B, R), dtype=torch.float32, device=dev)
        a = torch.empty((B, F), dtype=torch.float32, device=dev)
        _lib.call("rh_senet_fwd", _p(x), x.stride(0), _p(w1), _p(w2), B, F, R, D, _p(y), _p(z), _p(h), _p(a), _stream())
        ctx.save_for_backward(x, w1, w2, z, h, a)
        return y

    @staticmethod
    def backward(ctx, g):
        x, w1, w2, z, h, a = ctx.saved_tensors
        B, F, D = x.shape
        R = w1.shape[0]
        dev = x.device
        if g.stride(2) != 1 or g.stride(1) != D or g.stride(0) < F * D:
            g = g.contiguous()
        g_x = torch.empty((B, F, D), dtype=torch.float32, device=dev)
        nb = _lib.query("rh_twotower_nblocks", B)
        partial = torch.empty((nb, 2 * R * F), dtype=torch.float32, device=dev)
        _lib.call("rh_senet_bwd", _p(x), x.stride(0), _p(w1), _p(w2), _p(z), _p(h), _p(a), _p(g), g.stride(0), B, F, R, D,
                  _p(g_x), _p(partial), _stream())
        g_w = torch.empty((2, R * F), dtype=torch.float32, device=dev)
        _lib.call("rh_colsum", _p(partial), nb, 2 * R * F, _p(g_w), _NULL, 0, _NULL, _stream())
        return g_x, g_w[0].view(R, F), g_w[1].view(F, R)


def senet_ok(x, w1, w2):
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[0] >= 1 and
            1 <= x.shape[1] <= _lib.H.RH_SENET_MAX_F and 1 <= x.shape[2] <= _lib.H.RH_SENET_MAX_D and
            w1.is_cuda and w2.is_cuda and w1.dtype == torch.float32 and
            w2.dtype == torch.float32 and w1.dim() == 2 and w1.shape[1] == x.shape[1] and 1 <= w1.shape[0] <= x.shape[1] and
            tuple(w2.shape) == (x.shape[1], w1.shape[0]))


def senet(x, w1, w2):
    """``x * relu(relu(x.mean(-1) @ w1.T) @ w2.T).unsqueeze(-1)`` for x (B, F, D) -- a view of the fused gather's (B, F D)
    output is read in place --, w1 (R, F), w2 (F, R): SENETLayer.forward as one launch each way."""
    return _SenetFn.apply(x, w1, w2)


# --------------------------------------------------------------------------------------------
# TIGER / T5: masked, biased, rectangular softmax attention and the residual RMS norm (csrc/t5attn.hip)
# --------------------------------------------------------------------------------------------
_t5_bucket_cache = {}


def _t5_bucket_of(rel, bidirectional, num_buckets, max_distance):
    """T5Attention._relative_position_bucket's rule, in its own order of operations (int64 positions, float32 logarithm,
    truncation to int64) on the CPU, so a bucket boundary falls where the reference's falls."""
    rel = rel.to(torch.int64)
    buckets = torch.zeros_like(rel)
    nb = int(num_buckets)
    if nb == 1:  # one bucket holds every distance (the reference's rule divides by zero here)
        return buckets
    if nb // (4 if bidirectional else 2) == 0:
        raise ValueError(f"t5_relative_buckets: num_buckets={nb} leaves no exact bucket (the reference's rule divides by "
                         "zero): 1, or at least 4 bidirectional / 2 one-sided")
    if bidirectional:
        nb //= 2
        buckets = buckets + (rel > 0).to(torch.int64) * nb
        rel = rel.abs()
    else:
        rel = -torch.minimum(rel, torch.zeros_like(rel))
    max_exact = nb // 2
    small = rel < max_exact
    with torch.no_grad():
        big = max_exact + (torch.log(rel.to(torch.float32) / max_exact) / math.log(max_distance / max_exact) *
                           (nb - max_exact)).to(torch.int64)
    big = torch.minimum(big, torch.full_like(big, nb - 1))
    return buckets + torch.where(small, rel, big)


def t5_relative_buckets(Lq, Lk, bidirectional, num_buckets, max_distance, device=None):
    """The int32 table of T5's relative-position buckets for Lq queries against Lk keys: entry (j - i) + (Lq - 1) is the
    bucket of key j seen from query i.  Built once per (Lq, Lk, bidirectional, num_buckets, max_distance) on the host and
    cached (per device when ``device`` is given)."""
    key = (int(Lq), int(Lk), bool(bidirectional), int(num_buckets), int(max_distance))
    table = _t5_bucket_cache.get(key)
    if table is None:
        rel = torch.arange(-(key[0] - 1), key[1], dtype=torch.int64)
        table = _t5_bucket_of(rel, key[2], key[3], key[4]).to(torch.int32).contiguous()
        if int(table.min()) < 0 or int(table.max()) >= key[3]:  # the kernel indexes the bias table with it
            raise ValueError(f"t5_relative_buckets{key}: a bucket outside [0, num_buckets)")
        _t5_bucket_cache[key] = table
    if device is None or torch.device(device).type == "cpu":
        return table
    dkey = key + (str(device),)
    dev_table = _t5_bucket_cache.get(dkey)
    if dev_table is None:
        dev_table = _t5_bucket_cache[dkey] = table.to(device)
    return dev_table


class _T5AttnFn(torch.autograd.Function):
    """(B, Lq, H dh) = dropout(softmax_j(q k^T + bias, mask)) v; keeps the rows' log-sum-exp, never the weights."""

    @staticmethod
    def forward(ctx, q, k, v, bias, mask, bucket, cfg):
        H, dh, causal, nb, p = cfg
        B, Lq, Lk = int(q.shape[0]), int(q.shape[1]), int(k.shape[1])
        dev = q.device
        out = torch.empty((B, Lq, H * dh), dtype=torch.float32, device=dev)
        lse = torch.empty((B, H, Lq), dtype=torch.float32, device=dev)
        rng = _dropout_rng(dev) if p > 0 else None
        ctr = torch.empty(1, dtype=torch.int64, device=dev) if p > 0 else None
        _lib.call("rh_t5_attn_fwd", _p(q), int(q.stride(1)), _p(k), _p(v), int(k.stride(1)), B, Lq, Lk, H, dh, _p(mask),
                  causal, _p(bias), _p(bucket), nb, p, _p(rng), _p(ctr), _p(out), _p(lse), _stream())
        ctx.cfg = cfg
        ctx.save_for_backward(q, k, v, bias, mask, bucket, out, lse, rng, ctr)
        return out

    @staticmethod
    def backward(ctx, g):
        q, k, v, bias, mask, bucket, out, lse, rng, ctr = ctx.saved_tensors
        H, dh, causal, nb, p = ctx.cfg
        B, Lq, Lk = int(q.shape[0]), int(q.shape[1]), int(k.shape[1])
        dev = q.device
        g = g.contiguous()
        W = H * dh
        g_q = torch.empty((B, Lq, W), dtype=torch.float32, device=dev)
        if k.stride(1) >= 2 * W:  # column blocks of a fused product: its gradient's blocks, side by side
            g_kv = torch.empty((B, Lk, 2 * W), dtype=torch.float32, device=dev)
            g_k, g_v = g_kv[:, :, :W], g_kv[:, :, W:]
        else:
            g_kv = torch.empty((2, B, Lk, W), dtype=torch.float32, device=dev)
            g_k, g_v = g_kv[0], g_kv[1]
        g_bias = torch.empty_like(bias) if bias is not None else None
        if B == 0:
            return g_q, g_k, g_v, None if bias is None else torch.zeros_like(bias), None, None, None
        delta = torch.empty((B, H, Lq), dtype=torch.float32, device=dev)
        part = None
        if bias is not None:
            part = torch.empty((_lib.query("rh_t5_attn_nparts", B, Lq, H), Lq + Lk - 1), dtype=torch.float32, device=dev)
        _lib.call("rh_t5_attn_bwd", _p(q), int(q.stride(1)), _p(k), _p(v), int(k.stride(1)), B, Lq, Lk, H, dh, _p(mask),
                  causal, _p(bias), _p(bucket), nb, p, _p(rng), _p(ctr), _p(out), _p(lse), _p(g), _p(delta), _p(g_q), W,
                  _p(g_k), _p(g_v), int(g_k.stride(1)), _p(part), _p(g_bias), _stream())
        return g_q, g_k, g_v, g_bias, None, None, None


def t5_attention(q, k, v, n_heads, key_mask=None, causal=False, bias_table=None, bidirectional=True, max_distance=128,
                 dropout_p=0.0, training=True):
    """T5's multi-head attention (B, Lq, H dh) of q (B, Lq, H dh) against k, v (B, Lk, H dh), with no scale on q . k:
    separate projections, or column blocks of one fused QKV / KV product (read in place when k and v share a row stride).
    ``key_mask`` (B, Lk), non-zero = attend; a row with no key left weighs all Lk keys equally, as the reference's additive
    mask does.  ``causal`` excludes j > i and needs Lq == Lk.  ``bias_table`` (num_buckets, H): the stack's
    relative_attention_bias weight, added by T5's bucket rule (``bidirectional``, ``max_distance``).  Dropout with
    probability ``dropout_p`` on the weights when ``training``."""
    require_hip(q, k, v, key_mask, bias_table)
    if (q.dim() != 3 or k.dim() != 3 or k.shape != v.shape or q.shape[0] != k.shape[0] or q.shape[2] != k.shape[2] or
            q.shape[2] % n_heads != 0):
        raise RuntimeError(f"torch_rechub_amd: T5 attention of q {tuple(q.shape)}, k {tuple(k.shape)}, v {tuple(v.shape)} "
                           f"with {n_heads} heads unsupported (q (B, Lq, H dh), k and v (B, Lk, H dh))")
    if q.dtype != torch.float32 or k.dtype != torch.float32 or v.dtype != torch.float32 or (
            bias_table is not None and bias_table.dtype != torch.float32):
        raise RuntimeError("torch_rechub_amd: T5 attention runs in float32 only")
    B, Lq, W = (int(x) for x in q.shape)
    Lk = int(k.shape[1])
    H = int(n_heads)
    dh = W // H
    nb = int(bias_table.shape[0]) if bias_table is not None else 0
    if bias_table is not None and (bias_table.dim() != 2 or nb < 1 or bias_table.shape[1] != H):
        raise RuntimeError(f"torch_rechub_amd: T5 attention bias table {tuple(bias_table.shape)} unsupported "
                           "((num_buckets >= 1, H))")
    if key_mask is not None and tuple(key_mask.shape) != (B, Lk):
        raise RuntimeError(f"torch_rechub_amd: T5 attention key mask {tuple(key_mask.shape)} is not (B, Lk) = ({B}, {Lk})")
    p = float(dropout_p) if training else 0.0
    if not 0.0 <= p < 1.0:
        raise RuntimeError(f"torch_rechub_amd: attention dropout p={p} has no HIP kernel (0 <= p < 1)")
    if not _attn_view_ok(q, B, Lq, W):
        q = q.contiguous()
    if not (_attn_view_ok(k, B, Lk, W) and _attn_view_ok(v, B, Lk, W) and k.stride(1) == v.stride(1)):
        k, v = k.contiguous(), v.contiguous()
    mask = None if key_mask is None else (key_mask != 0).to(torch.uint8).contiguous()
    bucket = None
    if bias_table is not None and 1 <= Lq <= _lib.H.RH_ATTN_MAX_L and 1 <= Lk <= _lib.H.RH_ATTN_MAX_L:
        bucket = t5_relative_buckets(Lq, Lk, bidirectional, nb, max_distance, device=q.device)
    cfg = (H, dh, 1 if causal else 0, nb, p)
    # (shapes outside the kernel's range are refused by the entry point itself, before any launch)
    return _T5AttnFn.apply(q, k, v, None if bias_table is None else bias_table.contiguous(), mask, bucket, cfg)


class _AddRmsNormFn(torch.autograd.Function):
    """(h + delta, RMSNorm(h + delta) * w) over the rows of (M, D); g_w through per-workgroup partials and rh_colsum."""

    @staticmethod
    def forward(ctx, h, delta, w, eps):
        M, D = (int(x) for x in h.shape)
        dev = h.device
        y = torch.empty((M, D), dtype=torch.float32, device=dev)
        rstd = torch.empty((M,), dtype=torch.float32, device=dev)
        hn = torch.empty((M, D), dtype=torch.float32, device=dev) if delta is not None else None
        _lib.call("rh_add_rms_norm_fwd", _p(h), _p(delta), _p(w), eps, M, D, _p(hn), _p(y), _p(rstd), _stream())
        ctx.has_delta = delta is not None
        ctx.save_for_backward(h if hn is None else hn, w, rstd)
        if hn is None:  # no sum was formed: the caller keeps h; a placeholder stands in the output tuple
            hn = torch.empty((0,), dtype=torch.float32, device=dev)
            ctx.mark_non_differentiable(hn)
        return hn, y

    @staticmethod
    def backward(ctx, g_hn, g_y):
        hn, w, rstd = ctx.saved_tensors
        M, D = (int(x) for x in hn.shape)
        dev = hn.device
        if g_y is None:
            return g_hn, (g_hn if ctx.has_delta else None), torch.zeros_like(w), None
        g_y = g_y.contiguous()
        g_hn = g_hn.contiguous() if (ctx.has_delta and g_hn is not None) else None  # (else: the placeholder's)
        g_h = torch.empty((M, D), dtype=torch.float32, device=dev)
        g_w = torch.zeros((D,), dtype=torch.float32, device=dev)
        if M > 0:
            n = _lib.query("rh_add_rms_norm_nparts", M)
            part = torch.empty((n, D), dtype=torch.float32, device=dev)
            _lib.call("rh_add_rms_norm_bwd", _p(hn), _p(w), _p(rstd), _p(g_y), _p(g_hn), M, D, _p(g_h), _p(part), _stream())
            _lib.call("rh_colsum", _p(part), n, D, _p(g_w), _NULL, 0, _NULL, _stream())
        return g_h, (g_h if ctx.has_delta else None), g_w, None


def add_rms_norm(h, delta, weight, eps=1e-6):
    """(h_new, y): h_new = h + delta (``delta`` None: h itself), y = h_new * rsqrt(mean(h_new^2, -1) + eps) * weight --
    T5LayerNorm behind the residual add of the sub-layer before it, in one pass.  float32 (..., D), D <= RH_RMS_NORM_MAX_D; the weight
    gradient is summed in a fixed order."""
    require_hip(h, delta, weight)
    D = int(h.shape[-1])
    if h.dtype != torch.float32 or weight.dtype != torch.float32 or (delta is not None and delta.dtype != torch.float32):
        raise RuntimeError("torch_rechub_amd: add_rms_norm runs in float32 only")
    if not 1 <= D <= _lib.H.RH_RMS_NORM_MAX_D or tuple(weight.shape) != (D,) or (delta is not None and delta.shape != h.shape):
        raise RuntimeError(f"torch_rechub_amd: add_rms_norm of h {tuple(h.shape)}, weight {tuple(weight.shape)} has no HIP "
                           f"kernel (1 <= D <= {_lib.H.RH_RMS_NORM_MAX_D}, weight (D,), delta like h)")
    hn, y = _AddRmsNormFn.apply(h.reshape(-1, D).contiguous(), None if delta is None else delta.reshape(-1, D).contiguous(),
                                weight.contiguous(), float(eps))
    return (h if delta is None else hn.view(h.shape)), y.view(h.shape)


def beam_step(logits, running, node, trie):
    """One step of the constrained beam search (csrc/beam.hip): ``logits`` (B K, V) float32 the beams' next-token logits
    (rows may be strided: the ``[:, -1, :]`` view of a decoder output is read in place), ``running`` (B, K) float32 their
    scores, ``node`` (B, K) int32 their nodes in ``trie`` (a ``utils.data.DeviceTrie`` on the same device), -1 = dead beam.
    Returns ``(running, parent, token, node, short)``: per query the K best continuations running + log_softmax(logits)[tok]
    over the children of the beams' nodes, by (score descending, beam ascending, token ascending) -- (B, K) float32 and
    three (B, K) int32 -- and ``short`` (B,) int32, 1 where fewer than K continuations exist (the unused slots are -inf,
    -1, -1, -1).  No autograd; no host synchronisation; runs on the current stream."""
    require_hip(logits, running, node, trie.child_off)
    if logits.dim() != 2 or running.dim() != 2 or tuple(node.shape) != tuple(running.shape):
        raise ValueError(f"beam_step: logits {tuple(logits.shape)}, running {tuple(running.shape)}, node {tuple(node.shape)}: "
                         "(B K, V), (B, K) and (B, K) expected")
    if logits.dtype != torch.float32 or running.dtype != torch.float32 or node.dtype != torch.int32:
        raise ValueError("beam_step: float32 logits and running and int32 node expected")
    B, K = (int(v) for v in running.shape)
    V = int(logits.shape[1])
    if int(logits.shape[0]) != B * K:
        raise ValueError(f"beam_step: {int(logits.shape[0])} logits rows for B K = {B} x {K} beams")
    if not (logits.device == running.device == node.device == trie.child_off.device):
        raise ValueError("beam_step: logits, running, node and the trie must be on one device")
    if not 1 <= K <= _lib.H.RH_BEAM_MAX_K or V < 1:
        raise ValueError(f"beam_step: K={K}, V={V} unsupported (1 <= K <= {_lib.H.RH_BEAM_MAX_K}, V >= 1)")
    if trie.max_token >= V:
        raise ValueError(f"beam_step: the trie holds token {trie.max_token}, outside the vocabulary V={V}")
    logits = logits.detach()
    if B * K > 0 and (logits.stride(1) != 1 or (B * K > 1 and logits.stride(0) < V)):
        logits = logits.contiguous()
    ld = int(logits.stride(0)) if B * K > 1 else V
    running, node = running.detach().contiguous(), node.contiguous()
    dev = logits.device
    out_run = torch.empty((B, K), dtype=torch.float32, device=dev)
    parent, tok, child = (torch.empty((B, K), dtype=torch.int32, device=dev) for _ in range(3))
    short = torch.empty((B,), dtype=torch.int32, device=dev)
    if B > 0:
        _lib.call("rh_beam_step", _p(logits), ld, _p(running), _p(node), _p(trie.child_off), _p(trie.child_tok),
                  _p(trie.child_node), int(trie.n_nodes), B, K, V, _p(out_run), _p(parent), _p(tok), _p(child), _p(short),
                  _stream())
    return out_run, parent, tok, child, short


# --------------------------------------------------------------------------------------------
# CIN: one Compressed Interaction Network layer (csrc/cin.hip)
# --------------------------------------------------------------------------------------------


def _cin_views(x0, h):
    """(x0, sample stride, field stride, h, sample stride) as the kernels read them: d contiguous, x0's fields at least D
    apart, a sample of h contiguous.  Anything else is copied here."""
    D = int(x0.shape[2])
    if (x0.stride(2) != 1 and D > 1) or (x0.shape[1] > 1 and x0.stride(1) < D):
        x0 = x0.contiguous()
    if (h.stride(2) != 1 and D > 1) or (h.shape[1] > 1 and h.stride(1) != D):
        h = h.contiguous()
    xf = int(x0.stride(1)) if x0.shape[1] > 1 else D
    return x0, int(x0.stride(0)), max(xf, D), h, int(h.stride(0))


class _CinLayerFn(torch.autograd.Function):
    """relu(conv1d(x0 (x) h)) of one CIN layer; the (B, F Hp, D) product exists only in registers, both ways."""

    @staticmethod
    def forward(ctx, x0, h, weight, bias):
        B, F, D = (int(s) for s in x0.shape)
        Hp, Ho = int(h.shape[1]), int(weight.shape[0])
        x0, xs, xf, h, hs = _cin_views(x0, h)
        weight, bias = weight.contiguous(), bias.contiguous()  # (Ho, F Hp, 1): read as (Ho, F Hp)
        y = torch.empty((B, Ho, D), dtype=torch.float32, device=x0.device)
        _lib.call("rh_cin_fwd", _p(x0), xs, xf, _p(h), hs, _p(weight), _p(bias), B, D, F, Hp, Ho, _p(y), _stream())
        ctx.save_for_backward(x0, h, weight, y)
        ctx.strides = (xs, xf, hs)
        return y

    @staticmethod
    def backward(ctx, g):
        x0, h, weight, y = ctx.saved_tensors
        xs, xf, hs = ctx.strides
        B, F, D = (int(s) for s in x0.shape)
        Hp, Ho = int(h.shape[1]), int(weight.shape[0])
        K = F * Hp
        dev = x0.device
        g = g.contiguous()
        need_x0, need_h, need_w, need_b = ctx.needs_input_grad
        g_x0 = torch.empty((B, F, D), dtype=torch.float32, device=dev) if need_x0 else None
        g_h = torch.empty((B, Hp, D), dtype=torch.float32, device=dev) if need_h else None
        if need_x0 or need_h:
            _lib.call("rh_cin_bwd", _p(x0), xs, xf, _p(h), hs, _p(weight), _p(y), _p(g), B, D, F, Hp, Ho, _p(g_x0), _p(g_h),
                      _stream())
        g_w = g_b = None
        if need_w or need_b:
            if B == 0:  # nothing is launched: the parameter gradients are exact zeros
                both = torch.zeros((Ho * K + Ho,), dtype=torch.float32, device=dev)
            else:
                nch = _lib.query("rh_cin_wgrad_chunks", B, D, F, Hp, Ho)
                part = torch.empty((nch, Ho * K + Ho), dtype=torch.float32, device=dev)
                _lib.call("rh_cin_wgrad", _p(x0), xs, xf, _p(h), hs, _p(y), _p(g), B, D, F, Hp, Ho, _p(part), _stream())
                both = torch.empty((Ho * K + Ho,), dtype=torch.float32, device=dev)
                _lib.call("rh_colsum", _p(part), nch, Ho * K + Ho, _p(both), _NULL, 0, _NULL, _stream())
            g_w = both[:Ho * K].view(Ho, K, 1) if need_w else None
            g_b = both[Ho * K:] if need_b else None
        return g_x0, g_h, g_w, g_b


def cin_layer_ok(x0, h, weight, bias):
    """True when the HIP kernels take this layer: float32 HIP tensors inside the ranges of rh_cin_* (RH_CIN_MAX_*)."""
    ts = (x0, h, weight, bias)
    if not all(t.is_cuda and t.dtype == torch.float32 for t in ts) or x0.dim() != 3 or h.dim() != 3 or weight.dim() != 3:
        return False
    (B, F, D), Hp, Ho = x0.shape, h.shape[1], weight.shape[0]
    return (h.shape[0] == B and h.shape[2] == D and tuple(weight.shape) == (Ho, F * Hp, 1) and tuple(bias.shape) == (Ho,) and
            1 <= D <= _lib.H.RH_CIN_MAX_D and 1 <= F <= _lib.H.RH_CIN_MAX_F and 1 <= Hp <= _lib.H.RH_CIN_MAX_HP and
            1 <= Ho <= _lib.H.RH_CIN_MAX_HO)


def cin_layer(x0, h, weight, bias):
    """``relu(conv1d((x0.unsqueeze(2) * h.unsqueeze(1)).view(B, F * Hp, D), weight, bias))`` for x0 (B, F, D), h (B, Hp, D),
    weight (Ho, F * Hp, 1) -- the Conv1d parameter, used in place --, bias (Ho,): one CIN layer as one MFMA GEMM launch
    (csrc/cin.hip) whose operand is formed from x0 and h in registers.  x0 may be a strided view (the sparse block of the
    fused gather's output) and h the second half of the previous layer's output; the backward is deterministic.  Shapes
    outside the kernel's ranges are refused by the entry points, before any launch."""
    require_hip(x0, h, weight, bias)
    if any(t.dtype != torch.float32 for t in (x0, h, weight, bias)):
        raise RuntimeError("torch_rechub_amd: cin_layer runs in float32 only")
    if (x0.dim() != 3 or h.dim() != 3 or h.shape[0] != x0.shape[0] or h.shape[2] != x0.shape[2] or
            tuple(weight.shape) != (weight.shape[0], x0.shape[1] * h.shape[1], 1) or tuple(bias.shape) != (weight.shape[0],)):
        raise RuntimeError(f"torch_rechub_amd: cin_layer of x0 {tuple(x0.shape)}, h {tuple(h.shape)}, weight "
                           f"{tuple(weight.shape)}, bias {tuple(bias.shape)}: need x0 (B, F, D), h (B, Hp, D), weight "
                           "(Ho, F * Hp, 1), bias (Ho,)")
    return _CinLayerFn.apply(x0, h, weight, bias)


# --------------------------------------------------------------------------------------------
# Evaluation metrics (csrc/metric.hip): exact AUC / GAUC, log loss, top-K list metrics
# --------------------------------------------------------------------------------------------
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
        from .models.matching._listwise import no_kernel
        raise no_kernel(f"{what} over K={K} recommendations (1 <= K <= {_lib.H.RH_RANK_MAX_K})")
    cutoffs = [int(k) for k in cutoffs]
    if not cutoffs or any(not 1 <= k <= K for k in cutoffs):
        raise ValueError(f"torch_rechub_amd: {what} takes cut-offs within [1, K={K}], got {cutoffs}")
    if len(cutoffs) > _lib.H.RH_RANK_MAX_CUTOFFS:
        from .models.matching._listwise import no_kernel
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
        from .models.matching._listwise import no_kernel
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
        from .models.matching._listwise import no_kernel
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
