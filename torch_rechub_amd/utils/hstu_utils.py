"""HSTU bias modules with the reference's constructor signatures, parameter names and init (torch_rechub/utils/hstu_utils.py).

``RelativeBucketedTimeAndPositionBias`` keeps its dense ``forward`` (the (B, H, L, L) bias, for API users); ``HSTULayer``
never calls it: the attention kernel (``ops.hstu_attention``, csrc/hstu.hip) reads ``pos_w`` / ``ts_w`` directly and
forms each bias term in registers with the same bucket arithmetic (``bucketize_time`` below).  ``RelPosBias`` and
``VocabMask`` are plain mirrors.
"""
import math

import torch
import torch.nn as nn


def bucketize_time(dt, num_time_buckets, time_bucket_fn="sqrt", time_bucket_divisor=1.0, time_bucket_unit="minutes"):
    """Signed int64 second deltas -> bucket ids in [0, num_time_buckets]: float32 |dt| [/ 60], floored at 1e-6, sqrt or
    log, / divisor, clamped, truncated (the arithmetic the attention kernel repeats per score)."""
    dt = dt.float().abs()
    if time_bucket_unit == "minutes":
        dt = dt / 60.0
    dt = torch.clamp(dt, min=1e-6)
    v = torch.sqrt(dt) if time_bucket_fn == "sqrt" else torch.log(dt)
    return (v / time_bucket_divisor).clamp(min=0, max=num_time_buckets).long()


class RelPosBias(nn.Module):
    """Legacy bucketed relative-position bias (1, H, L, L) over ``num_buckets`` buckets of |i - j|."""

    def __init__(self, n_heads, max_seq_len, num_buckets=32):
        super().__init__()
        self.n_heads = n_heads
        self.max_seq_len = max_seq_len
        self.num_buckets = num_buckets
        bound = math.sqrt(1.0 / num_buckets)
        self.rel_pos_bias_table = nn.Parameter(torch.empty(num_buckets, n_heads).uniform_(-bound, bound))

    def _relative_position_bucket(self, relative_position):
        dist = relative_position.abs().clamp(max=self.max_seq_len)
        return (dist * (self.num_buckets - 1) // self.max_seq_len).long()

    def forward(self, seq_len):
        pos = torch.arange(seq_len, dtype=torch.long, device=self.rel_pos_bias_table.device)
        buckets = self._relative_position_bucket(pos[None, :] - pos[:, None])
        return self.rel_pos_bias_table[buckets].permute(2, 0, 1).unsqueeze(0)


class RelativeBucketedTimeAndPositionBias(nn.Module):
    """HSTU rab^{p,t}: per-head bias pos_w[j - i + N - 1] + ts_w[bucket(t_i - t_j)] added to the attention scores."""

    def __init__(self, n_heads, max_seq_len, num_time_buckets=128, time_bucket_fn='sqrt', time_bucket_divisor=1.0,
                 time_bucket_unit='minutes'):
        super().__init__()
        if time_bucket_fn not in ('sqrt', 'log'):
            raise ValueError(f"Unsupported time_bucket_fn: {time_bucket_fn}")
        if time_bucket_unit not in ('minutes', 'seconds'):
            raise ValueError(f"Unsupported time_bucket_unit: {time_bucket_unit}")
        self.n_heads = n_heads
        self.max_seq_len = max_seq_len
        self.num_time_buckets = num_time_buckets
        self.time_bucket_fn = time_bucket_fn
        self.time_bucket_divisor = time_bucket_divisor
        self.time_bucket_unit = time_bucket_unit
        npos, nts = 2 * max_seq_len - 1, num_time_buckets + 1
        self.pos_w = nn.Parameter(torch.empty(npos, n_heads).uniform_(-math.sqrt(1.0 / npos), math.sqrt(1.0 / npos)))
        self.ts_w = nn.Parameter(torch.empty(nts, n_heads).uniform_(-math.sqrt(1.0 / nts), math.sqrt(1.0 / nts)))

    def _bucketize_time(self, dt):
        return bucketize_time(dt, self.num_time_buckets, self.time_bucket_fn, self.time_bucket_divisor,
                              self.time_bucket_unit)

    def forward(self, time_diffs=None, seq_len=None):
        """Dense bias: (B, H, L, L) with ``time_diffs`` (B, L), else (1, H, L, L) from ``seq_len``."""
        if time_diffs is None:
            if seq_len is None:
                raise ValueError("Provide either `time_diffs` or `seq_len`.")
            L, device = seq_len, self.pos_w.device
        else:
            L, device = time_diffs.shape[1], time_diffs.device
        if L > self.max_seq_len:
            raise ValueError(f"seq_len ({L}) exceeds max_seq_len ({self.max_seq_len}).")
        pos = torch.arange(L, device=device)
        pos_bias = self.pos_w[pos[None, :] - pos[:, None] + (self.max_seq_len - 1)].permute(2, 0, 1)
        if time_diffs is None:
            return pos_bias.unsqueeze(0)
        buckets = self._bucketize_time(time_diffs[:, :, None] - time_diffs[:, None, :])
        return pos_bias.unsqueeze(0) + self.ts_w[buckets].permute(0, 3, 1, 2)


class VocabMask(nn.Module):
    """Pushes invalid item columns (fixed ``invalid_items`` and optional per-row ids) of a logits tensor to -1e9."""

    def __init__(self, vocab_size, invalid_items=None):
        super().__init__()
        self.vocab_size = vocab_size
        self.register_buffer('mask', torch.ones(vocab_size, dtype=torch.bool))
        for item in invalid_items or ():
            if 0 <= item < vocab_size:
                self.mask[item] = False

    def apply_mask(self, logits, invalid_ids=None):
        out = logits.clone()
        out[..., ~self.mask] = -1e9
        if invalid_ids is None:
            return out
        ids = invalid_ids.to(device=out.device, dtype=torch.long)
        if ids.dim() == 1:
            ids = ids.unsqueeze(0).expand(out.size(0), -1)
        if out.dim() != 2 or ids.dim() != 2:
            raise ValueError("dynamic invalid_ids masking expects logits (B, V) and invalid_ids (B, N)")
        if ids.size(0) != out.size(0):
            raise ValueError("invalid_ids batch size must match logits batch size")
        ok = (ids >= 0) & (ids < self.vocab_size)
        out.scatter_(dim=-1, index=ids.masked_fill(~ok, 0), value=-1e9)
        return out
