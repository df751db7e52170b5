"""Session-based retrieval (csrc/session.hip): additive attention pooling and the stand-alone dropout.  The general GRU,
the full-catalogue cross entropy and session_lengths call the core of ops.py and live there."""
import torch

from .. import _lib
from .._opcore import _p, _stream, require_hip, _dropout_rng


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
