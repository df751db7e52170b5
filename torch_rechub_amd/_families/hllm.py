"""HLLM: causal softmax attention with the bucketed relative-position bias and dropout (csrc/hllm.hip), in float32 and,
on the half-precision MFMA tile of csrc/softmax_attn_half_tile.h, in float16 / bfloat16."""
import torch

from .. import _lib
from .._opcore import _p, _stream, require_hip, _dropout_rng, _attn_view_ok

HALF_TYPES = {torch.float16: 0, torch.bfloat16: 1}  # the half operand types and the kernels' is_bf16 for them


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


class _SoftmaxAttnHalfFn(torch.autograd.Function):
    """_SoftmaxAttnFn on float16 / bfloat16 q, k, v: out and the three gradients in that type, the log-sum-exp, the row
    dots and the bias table's gradient in float32."""

    @staticmethod
    def forward(ctx, q, k, v, bias, cfg):
        H, dh, N, nb, scale, p = cfg
        B, L = int(q.shape[0]), int(q.shape[1])
        dev = q.device
        out = torch.empty((B, L, H * dh), dtype=q.dtype, device=dev)
        lse = torch.empty((B, H, L), dtype=torch.float32, device=dev)
        rng = _dropout_rng(dev) if p > 0 else None
        ctr = torch.empty(1, dtype=torch.int64, device=dev) if p > 0 else None
        _lib.call("rh_softmax_attn_half_fwd", _p(q), _p(k), _p(v), HALF_TYPES[q.dtype], int(q.stride(1)), B, L, H, dh,
                  _p(bias), N, nb, scale, p, _p(rng), _p(ctr), _p(out), _p(lse), _stream())
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
        g_qkv = torch.empty((3, B, L, H * dh), dtype=q.dtype, device=dev)
        g_bias = torch.empty_like(bias) if bias is not None else None
        if B == 0:
            return g_qkv[0], g_qkv[1], g_qkv[2], None if bias is None else torch.zeros_like(bias), None
        delta = torch.empty((B, H, L), dtype=torch.float32, device=dev)
        part = None
        if bias is not None:
            part = torch.empty((_lib.call("rh_softmax_attn_nparts", B, L, H), L), dtype=torch.float32, device=dev)
        _lib.call("rh_softmax_attn_half_bwd", _p(q), _p(k), _p(v), HALF_TYPES[q.dtype], int(q.stride(1)), B, L, H, dh,
                  _p(bias), N, nb, scale, p, _p(rng), _p(ctr), _p(out), _p(lse), _p(g), _p(delta), _p(g_qkv[0]),
                  _p(g_qkv[1]), _p(g_qkv[2]), H * dh, _p(part), _p(g_bias), _stream())
        return g_qkv[0], g_qkv[1], g_qkv[2], g_bias, None


def softmax_attention(q, k, v, n_heads, max_seq_len, bias_table=None, dropout_p=0.0, training=True, scale=None):
    """Causal multi-head softmax attention (B, L, H dh) of q, k, v (B, L, H dh): three contiguous projections, or three
    column blocks of one (B, L, 3 H dh) product (fed without a copy when they share the row stride).  ``bias_table``
    (num_buckets, H): RelPosBias's table, added as table[min(|i - j|, max_seq_len) * (num_buckets - 1) // max_seq_len, h].
    Dropout with probability ``dropout_p`` on the attention weights when ``training``.  No padding mask.

    q, k, v all float32, all float16 or all bfloat16; ``bias_table`` is float32 either way.  Half operands run on the
    half-precision MFMA with float32 scores, statistics and sums: the result and the gradients of q, k, v come back in
    that type, the table's gradient in float32."""
    require_hip(q, k, v, bias_table)
    if q.dim() != 3 or q.shape != k.shape or q.shape != v.shape or q.shape[2] % n_heads != 0:
        raise RuntimeError(f"torch_rechub_amd: softmax attention of q {tuple(q.shape)}, k {tuple(k.shape)}, "
                           f"v {tuple(v.shape)} with {n_heads} heads unsupported (three (B, L, H dh) tensors)")
    if not (q.dtype == k.dtype == v.dtype and (q.dtype == torch.float32 or q.dtype in HALF_TYPES)) or (
            bias_table is not None and bias_table.dtype != torch.float32):
        raise RuntimeError(f"torch_rechub_amd: softmax attention of q {q.dtype}, k {k.dtype}, v {v.dtype}, bias table "
                           f"{None if bias_table is None else bias_table.dtype} has no HIP kernel (q, k, v all float32, "
                           "all float16 or all bfloat16; the bias table float32)")
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
    fn = _SoftmaxAttnHalfFn if q.dtype in HALF_TYPES else _SoftmaxAttnFn
    return fn.apply(q, k, v, None if bias_table is None else bias_table.contiguous(), cfg)
