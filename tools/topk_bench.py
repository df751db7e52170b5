"""Top-K retrieval timings on the device: ops.topk_items (csrc/topk.hip) against the eager chain the reference's examples
run, torch.topk(q @ x.T + mask, k), same process, same tensors, the two alternating:

  catalogue   V = 2^20 items, D = 64, M = 1024 queries, K = 10 and K = 200
  movielens   V = 4096 items, D = 64, M = 4096 queries, K = 200

mask is a (V,) row of zeros with -inf at the PAD id (examples/generative/run_hstu_movielens.py:109-114 masks column 0); the
kernel gets the same thing as ``invalid=[0]``.  Each figure is the median over ROUNDS windows of ``iters`` calls between
two device events (a window ends in a synchronise), warm-up first; min and max of the windows are printed beside it.  Peak
memory is torch.cuda.max_memory_allocated above what was allocated before one call.  The share of rows whose id lists are
identical on the two paths is printed (their fp32 scores differ in the last bits, so near-ties may swap).  One JSON line
at the end."""
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from torch_rechub_amd import ops  # noqa: E402

ROUNDS = 5
SHAPES = [("catalogue", 1024, 64, 1 << 20, 10, 20), ("catalogue", 1024, 64, 1 << 20, 200, 20),
          ("movielens", 4096, 64, 4096, 200, 100)]


def windows_ms(fns, iters, warmup=3):
    for fn in fns.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    out = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for name, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(iters):
                fn()
            b.record()
            torch.cuda.synchronize()
            out[name].append(a.elapsed_time(b) / iters)
    return out


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    del out
    return peak


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    result = {}
    for name, M, D, V, K, iters in SHAPES:
        q = torch.randn(M, D, device=dev)
        x = torch.randn(V, D, device=dev)
        mask = torch.zeros(V, device=dev)
        mask[0] = float("-inf")
        invalid = torch.tensor([0], device=dev)

        def fused():
            return ops.topk_items(q, x, K, invalid=invalid)

        def eager():
            return torch.topk(q @ x.t() + mask, K, dim=1)

        ids, _ = fused()
        ref = eager().indices
        same = float((ids == ref).all(dim=1).float().mean())
        w = windows_ms({"kernel": fused, "eager": eager}, iters)
        what = f"{name} (M {M}, D {D}, V {V}, K {K})"
        res = {}
        for n, ts in w.items():
            res[n + "_ms"] = statistics.median(ts)
            print(f"{what}: {n:7s} {res[n + '_ms']:9.3f} ms  (min {min(ts):.3f}, max {max(ts):.3f})")
        res["eager_over_kernel"] = res["eager_ms"] / res["kernel_ms"]
        res["kernel_peak_bytes"], res["eager_peak_bytes"] = peak_bytes(fused), peak_bytes(eager)
        res["nsplit"] = ops.topk_plan(M, V, K)[0]
        res["rows_with_identical_ids"] = same
        print(f"{what}: eager / kernel = {res['eager_over_kernel']:.2f}x; peak memory kernel {res['kernel_peak_bytes'] / 2**20:.1f} MiB, "
              f"eager {res['eager_peak_bytes'] / 2**20:.1f} MiB; nsplit {res['nsplit']}; rows with identical ids {same:.4f}")
        result[f"{name}_M{M}_V{V}_K{K}"] = res
        del q, x, mask, ids, ref
    print(json.dumps(result))


if __name__ == "__main__":
    main()
