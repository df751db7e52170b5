"""Time the device forms of diversity_score, coverage_score and novelty_score on an MI355X and write
profiles/beyond_metric_bench.txt.

  python tools/beyond_metric_bench.py [--out profiles/beyond_metric_bench.txt] [--repeat 10]

The three device metrics at M = 1 M users, K = 100, cut-offs (10, 50, 100), D = 64, V = 1 M items: the median wall time of
``--repeat`` calls after two warm-up calls; a call ends in the copy of its result to the host, so the clock covers the
kernels and that copy.  Two comparisons beside them:

  host        the host loops of this module (the reference's) at sizes they finish in about a second, and whether the
              device returns the same strings on the same data
  gather+bmm  diversity as table[ids[:, :k]] -> normalise -> bmm -> sum over pairs on torch ops, in float64 like the
              reference, at the largest M its (M, k, D) and (M, k, k) temporaries fit into, with its peak memory

No GPU: the script fails, it does not fall back.  The host timings belong to the CPU of the machine it ran on.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from torch_rechub_amd.basic import metric  # noqa: E402

M, K, D, V, CUT = 1_000_000, 100, 64, 1_000_000, (10, 50, 100)


def timed(fn, repeat, warmup=2):
    for _ in range(warmup):
        fn()
    times = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return statistics.median(times), min(times), max(times)


def once(fn):
    t0 = time.perf_counter()
    out = fn()
    return time.perf_counter() - t0, out


def gather_bmm_diversity(ids, table, cut):
    """The reference's computation on torch ops: per cut-off an (M, k, D) gather, unit rows, the (M, k, k) Gram matrices
    and the sum over their pairs i < j = (sum of all - trace) / 2.  Every id is known and present.  -> the users' means."""
    out = []
    for k in cut:
        e = table[ids[:, :k]].double()
        e /= e.norm(dim=2, keepdim=True).clamp_min(1e-10)
        gram = torch.bmm(e, e.transpose(1, 2))
        pairs = (gram.sum((1, 2)) - gram.diagonal(dim1=1, dim2=2).sum(1)) / 2
        out.append((1 - pairs / (k * (k - 1) / 2)).mean().item())
    return out


def gather_bmm_bytes_per_user(k, d):
    """float32 gather, its float64 copy, the norm's square, the Gram matrix and its reduction's temporaries."""
    return k * d * (4 + 8 + 8) + 2 * k * k * 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beyond_metric_bench.txt"))
    ap.add_argument("--repeat", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("beyond_metric_bench: no HIP device")
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(2022)
    ids = torch.randint(0, V, (M, K), device=dev, generator=gen)
    table = torch.randn((V, D), device=dev, generator=gen)
    pop = torch.rand((V,), device=dev, generator=gen)
    lines = [f"beyond_metric_bench on {torch.cuda.get_device_name(0)}; median (min .. max) of {args.repeat} calls, 2 warm-up "
             "calls", "a device call = kernels + the result's copy to the host; host timings: this machine's CPU, one call",
             f"M = {M} users, K = {K}, cut-offs {CUT}, D = {D}, V = {V} items (table {V * D * 4 / 2**20:.0f} MiB), ids uniform",
             ""]

    med, lo, hi = timed(lambda: metric.diversity_score(ids, table, topKs=CUT), args.repeat)
    row_bytes = M * max(CUT) * D * 4
    lines += [f"diversity  device {med * 1e3:.2f} ms ({lo * 1e3:.2f} .. {hi * 1e3:.2f}); {M * max(CUT)} rows of {D * 4} B "
              f"gathered = {row_bytes / 1e9:.1f} GB -> {row_bytes / med / 1e12:.2f} TB/s of row bytes over the call time"]
    med, lo, hi = timed(lambda: metric.coverage_score(ids, V, topKs=CUT), args.repeat)
    lines += [f"coverage   device {med * 1e3:.2f} ms ({lo * 1e3:.2f} .. {hi * 1e3:.2f}), with the max() that sizes the slots"]
    med, lo, hi = timed(lambda: metric.novelty_score(ids, pop, topKs=CUT), args.repeat)
    lines += [f"novelty    device {med * 1e3:.2f} ms ({lo * 1e3:.2f} .. {hi * 1e3:.2f})", ""]

    # the host loops on the first rows of the same data
    m_div, m_cov, m_nov = 2_000, 50_000, 4_000
    h_ids, h_table, h_pop = ids[:m_cov].cpu(), table.cpu().numpy(), pop.cpu().numpy()
    rec = dict(enumerate(h_ids[:m_div].tolist()))
    host_s, host_res = once(lambda: metric.diversity_score(rec, h_table, topKs=CUT))
    same = dict(metric.diversity_score(ids[:m_div], table, topKs=CUT)) == dict(host_res)
    lines += [f"diversity  host path at M = {m_div}: {host_s:.2f} s; device strings on the same data "
              f"{'equal' if same else 'DIFFER'}"]
    rec = dict(enumerate(h_ids.tolist()))
    host_s, host_res = once(lambda: metric.coverage_score(rec, range(V), topKs=CUT))
    same = dict(metric.coverage_score(ids[:m_cov], V, topKs=CUT)) == dict(host_res)
    lines += [f"coverage   host path at M = {m_cov}: {host_s:.2f} s; device strings on the same data "
              f"{'equal' if same else 'DIFFER'}"]
    rec = dict(enumerate(h_ids[:m_nov].tolist()))
    popularity = {i: float(h_pop[i]) for i in np.unique(h_ids[:m_nov].numpy()).tolist()}
    host_s, host_res = once(lambda: metric.novelty_score(rec, popularity, topKs=CUT))
    same = dict(metric.novelty_score(ids[:m_nov], pop, topKs=CUT)) == dict(host_res)
    lines += [f"novelty    host path at M = {m_nov}: {host_s:.2f} s; device strings on the same data "
              f"{'equal' if same else 'DIFFER'}", ""]
    del rec, popularity, h_table

    # gather + bmm on torch ops at the largest M that fits
    torch.cuda.synchronize()
    free = torch.cuda.mem_get_info()[0] + torch.cuda.memory_reserved() - torch.cuda.memory_allocated()
    m_fit = min(M, int(0.5 * free / gather_bmm_bytes_per_user(max(CUT), D)))
    while True:
        try:
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.memory_allocated()
            means = gather_bmm_diversity(ids[:m_fit], table, CUT)
            break
        except torch.cuda.OutOfMemoryError:
            torch.cuda.empty_cache()
            m_fit //= 2
    peak = torch.cuda.max_memory_allocated() - before
    med, lo, hi = timed(lambda: gather_bmm_diversity(ids[:m_fit], table, CUT), min(args.repeat, 5), warmup=1)
    raw = metric.diversity_score(ids[:m_fit], table, topKs=CUT)["Diversity"]
    dmed, dlo, dhi = timed(lambda: metric.diversity_score(ids[:m_fit], table, topKs=CUT), args.repeat)
    lines += [f"diversity  gather + bmm on torch ops (float64) at M = {m_fit} ({free / 2**30:.0f} GiB free): {med * 1e3:.1f} ms "
              f"({lo * 1e3:.1f} .. {hi * 1e3:.1f}), peak memory above the inputs {peak / 2**30:.1f} GiB",
              f"           the device metric at the same M = {m_fit}: {dmed * 1e3:.2f} ms ({dlo * 1e3:.2f} .. {dhi * 1e3:.2f}); "
              f"means {[round(v, 6) for v in means]} against {raw}"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
