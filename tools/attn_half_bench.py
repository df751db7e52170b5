"""Forward + backward of ops.softmax_attention alone: float32 against float16 and bfloat16 on the same seeded values.

    python tools/attn_half_bench.py [--min-ms 300] [--repeats 3]

Per shape (B, L, H, dh) every variant is warmed up first; then the variants alternate, each timed with device events around
enough calls to fill ``--min-ms`` of work, ``--repeats`` times.  Reports the median time per call, the spread (max - min
over the repeats, relative to the median), the ratio to the float32 kernels of the same build, and the peak memory of one
call above its resident inputs.  With the bias table (32 buckets) and no dropout; q, k, v are column blocks of one
(B, L, 3 H dh) tensor, as a fused projection would hand them over."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from torch_rechub_amd import ops  # noqa: E402

SHAPES = [(64, 200, 8, 64), (64, 256, 8, 64), (16, 1024, 8, 64), (16, 1024, 16, 128)]
DTYPES = [torch.float32, torch.float16, torch.bfloat16]


def make_step(shape, dtype, dev):
    B, L, H, dh = shape
    g = torch.Generator().manual_seed(L + H + dh)
    W = H * dh
    x = torch.randn(B, L, 3 * W, generator=g).to(dev, dtype).requires_grad_(True)
    table = (0.5 * torch.randn(32, H, generator=g)).to(dev).requires_grad_(True)
    gout = torch.randn(B, L, W, generator=g).to(dev, dtype)

    def step():
        out = ops.softmax_attention(x[..., :W], x[..., W:2 * W], x[..., 2 * W:], H, L, bias_table=table)
        out.backward(gout)
        x.grad = table.grad = None

    return step


def timed(step, calls):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        step()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--min-ms", type=float, default=300.0)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    print(f"device {torch.cuda.get_device_name(0)}; forward + backward of ops.softmax_attention, ms per call")
    for shape in SHAPES:
        steps = {dt: make_step(shape, dt, dev) for dt in DTYPES}
        calls, peak = {}, {}
        for dt, step in steps.items():  # warm-up, the call count and the peak memory of every variant
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            calls[dt] = max(3, int(a.min_ms / timed(step, 3)) + 1)
            peak[dt] = (torch.cuda.max_memory_allocated() - base) / 2**20
        times = {dt: [] for dt in DTYPES}
        for _ in range(a.repeats):
            for dt in DTYPES:
                times[dt].append(timed(steps[dt], calls[dt]))
        med = {dt: statistics.median(times[dt]) for dt in DTYPES}
        for dt in DTYPES:
            spread = (max(times[dt]) - min(times[dt])) / med[dt]
            print(f"(B, L, H, dh) = {shape}  {str(dt):15s} {med[dt]:8.3f} ms  spread {100 * spread:4.1f} %  "
                  f"x{med[dt] / med[torch.float32]:5.2f} of float32  peak +{peak[dt]:7.1f} MiB  ({calls[dt]} calls x {a.repeats})",
                  flush=True)
    ops.check_errors()


if __name__ == "__main__":
    main()
