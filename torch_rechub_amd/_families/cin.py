"""CIN: one Compressed Interaction Network layer (csrc/cin.hip)."""
import torch

from .. import _lib
from .._opcore import _NULL, _p, _stream, require_hip


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
