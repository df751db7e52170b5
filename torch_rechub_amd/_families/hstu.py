"""HSTU: pointwise relative-bias attention (csrc/hstu.hip).  Its next-token head (csrc/stream_ce.hip) writes the kernel
error word and therefore lives in ops.py."""
import math

import torch

from .. import _lib
from .._opcore import _p, _stream, require_hip


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
