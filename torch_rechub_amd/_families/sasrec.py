"""SASRec: the transformer block around softmax_attention, fused per row tile (csrc/sasrec.hip): the input stage, the
head and layer_norm.  The attention-input and feed-forward stages end in ops.linear_wgrad and live in ops.py."""
import torch

from .. import _lib
from .._opcore import _NULL, _p, _stream, require_hip, _dropout_rng


def _sasrec_check(what, D, *tensors):
    """Before anything is allocated or launched: float32 tensors and a width the kernels take."""
    if any(t is not None and t.dtype != torch.float32 for t in tensors):
        raise ValueError(f"torch_rechub_amd: {what} takes float32 tensors")
    if not 1 <= int(D) <= _lib.H.RH_SASREC_MAX_D:
        from ..models.matching._listwise import no_kernel
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
