"""Inverted-file index timings on the device: serving.HipIvfIndexer (ops.ivf_scan, csrc/ivf.hip) against the flat
serving.HipIndexer (ops.topk_items, csrc/topk.hip), same process, same table and queries, the two alternating:

  D = 64, M = 1024 queries, V = 2^20 rows of a Gaussian mixture (1024 centres 4 N(0, 1), rows and queries = a centre +
  N(0, 1)), metric "L2", K = 10 and 200, nlists = 1024, nprobe = 1, 8, 32, 256 and 1024

Each figure is the median over ROUNDS windows of ``iters`` queries between two device events (a window ends in a
synchronise), warm-up first; min and max of the windows are printed beside it.  recall@K is the share of the flat index's
ids (the exact answer) that the IVF answer holds.  A setting the kernel refuses (nprobe above its limit of 256) is reported
as refused.  Build time is one wall-clock build (k-means of 10 rounds, final assignment, grouping) after a warm-up build of
a small index; peak memory is torch.cuda.max_memory_allocated above what was allocated before.  The lines are also
written to ``--out`` (default profiles/ivf_bench.txt); one JSON line at the end."""
import argparse
import json
import statistics
import sys
import time

import torch

sys.path.insert(0, ".")
from torch_rechub_amd.serving import builder_factory  # noqa: E402

ROUNDS = 5
M, D, V, NLISTS = 1024, 64, 1 << 20, 1024
KS = (10, 200)
NPROBES = (1, 8, 32, 256, 1024)


def windows_ms(fns, iters, warmup=2):
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
    return out, peak


def mixture(n, centres, g):
    pick = torch.randint(0, centres.shape[0], (n,), generator=g, device=centres.device)
    return centres[pick] + torch.randn(n, centres.shape[1], generator=g, device=centres.device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/ivf_bench.txt")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(0)
    centres = 4.0 * torch.randn(NLISTS, D, generator=g, device=dev)
    x, q = mixture(V, centres, g), mixture(M, centres, g)
    lines, result = [], {}

    def say(line):
        print(line, flush=True)
        lines.append(line)

    say(f"ivf_bench: M {M}, D {D}, V {V}, nlists {NLISTS}, metric L2, Gaussian mixture of {NLISTS} centres; "
        f"median of {ROUNDS} windows (min - max)")
    with builder_factory("hip", index_type="IVF", nlists=8, niter=2).from_embeddings(x[:4096]):
        pass  # warm-up: loads the library, sizes the allocator's first blocks
    with builder_factory("hip").from_embeddings(x) as flat:
        def build():
            t0 = time.perf_counter()
            cm = builder_factory("hip", index_type="IVF", nlists=NLISTS, nprobe=1, niter=10).from_embeddings(x)
            index = cm.__enter__()
            torch.cuda.synchronize()
            return index, time.perf_counter() - t0

        (ivf, build_s), build_peak = peak_bytes(build)
        sizes = ivf.list_sizes().float()
        result["build_s"], result["build_peak_bytes"] = build_s, build_peak
        result["list_rows_min_mean_max"] = [float(sizes.min()), float(sizes.mean()), float(sizes.max())]
        say(f"build (10 rounds of k-means + final assignment + grouping): {build_s:.3f} s, peak memory {build_peak / 2**20:.1f} MiB "
            f"above the {V * D * 4 / 2**20:.0f} MiB table; rows per list min {sizes.min():.0f}, mean {sizes.mean():.0f}, "
            f"max {sizes.max():.0f}, empty lists {int((sizes == 0).sum())}")
        for K in KS:
            (want, _), flat_peak = peak_bytes(lambda: flat.query(q, K))
            for nprobe in NPROBES:
                what = f"K {K:3d} nprobe {nprobe:4d}"
                try:
                    (got, _), ivf_peak = peak_bytes(lambda: ivf.query(q, K, nprobe=nprobe))
                except RuntimeError as e:
                    say(f"{what}: refused ({str(e)[:150]})")
                    result[f"K{K}_nprobe{nprobe}"] = {"refused": True}
                    continue
                hit = (got.unsqueeze(2) == want.unsqueeze(1)).any(dim=2) & (got >= 0)
                recall = float(hit.sum()) / float((want >= 0).sum())
                same = bool(torch.equal(got, want))
                iters = 10 if nprobe <= 32 else 3
                w = windows_ms({"ivf": lambda: ivf.query(q, K, nprobe=nprobe), "flat": lambda: flat.query(q, K)}, iters)
                res = {n + "_ms": statistics.median(ts) for n, ts in w.items()}
                res.update(flat_over_ivf=res["flat_ms"] / res["ivf_ms"], recall=recall, ids_equal_flat=same,
                           ivf_peak_bytes=ivf_peak, flat_peak_bytes=flat_peak)
                say(f"{what}: ivf {res['ivf_ms']:9.3f} ms ({min(w['ivf']):.3f} - {max(w['ivf']):.3f}), flat {res['flat_ms']:9.3f} ms "
                    f"({min(w['flat']):.3f} - {max(w['flat']):.3f}), flat / ivf = {res['flat_over_ivf']:.2f}x, recall@{K} {recall:.4f}"
                    f"{' (ids equal the flat index)' if same else ''}, peak memory ivf {ivf_peak / 2**20:.1f} MiB, "
                    f"flat {flat_peak / 2**20:.1f} MiB")
                result[f"K{K}_nprobe{nprobe}"] = res
    say(json.dumps(result))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
