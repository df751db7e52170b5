"""TIGER / T5: masked, biased, rectangular softmax attention and the residual RMS norm (csrc/t5attn.hip)."""
import math

import torch

from .. import _lib
from .._opcore import _NULL, _p, _stream, require_hip, _dropout_rng, _attn_view_ok


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
