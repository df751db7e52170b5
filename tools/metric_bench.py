"""Time the device metrics of basic.metric on an MI355X and write profiles/metric_bench.txt.

  python tools/metric_bench.py [--out profiles/metric_bench.txt] [--repeat 10]

Three measurements, each the median wall time of ``--repeat`` calls after two warm-up calls; a call ends in the copy of
its result to the host, so the clock covers the sort, the kernels and that copy:

  AUC           N = 4.5 M float32 predictions, against sklearn's roc_auc_score on the same arrays on this host's CPU
  GAUC          N = 4.5 M over 200 k users; the host path of this module (pinned to the reference by
                tests/test_metric_host.py) is timed at N = 100 k over 2.5 k users -- a size it finishes in seconds
  list metrics  M = 1 M users, K = 100, cut-offs (10, 50, 100), truth lists of 1 to 30 ids; the host path at M = 5 k

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metric_bench.txt"))
    ap.add_argument("--repeat", type=int, default=10)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("metric_bench: no HIP device")
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(2022)
    lines = [f"metric_bench on {torch.cuda.get_device_name(0)}; median (min .. max) of {args.repeat} calls, 2 warm-up calls",
             "a device call = sort + kernels + the result's copy to the host; host timings: this machine's CPU, one call", ""]

    # AUC
    N = 4_500_000
    pred, label = rng.random(N).astype(np.float32), (rng.random(N) < 0.25).astype(np.float32)
    dp, dl = torch.from_numpy(pred).to(dev), torch.from_numpy(label).to(dev)
    med, lo, hi = timed(lambda: metric.auc_score(dl, dp), args.repeat)
    from sklearn.metrics import roc_auc_score
    host_s, host_auc = once(lambda: roc_auc_score(label, pred))
    got = metric.auc_score(dl, dp)
    lines += [f"AUC   N = {N}: device {med * 1e3:.2f} ms ({lo * 1e3:.2f} .. {hi * 1e3:.2f}); roc_auc_score on the host "
              f"{host_s * 1e3:.0f} ms; |device - host| = {abs(got - host_auc):.2e}"]

    # GAUC
    U = 200_000
    # every user holds both classes: one positive, one negative, and a random share of the rest
    users = np.concatenate([np.arange(U), np.arange(U), rng.integers(0, U, N - 2 * U)]).astype(np.int64)
    glabel = np.concatenate([np.ones(U, np.float32), np.zeros(U, np.float32), label[2 * U:]])
    perm = rng.permutation(N)
    users, glabel = users[perm], glabel[perm]
    du, dg = torch.from_numpy(users).to(dev), torch.from_numpy(glabel).to(dev)
    med, lo, hi = timed(lambda: metric.gauc_score(dg, dp, du), args.repeat)
    got = metric.gauc_score(dg, dp, du)
    n_small, u_small = 100_000, 2_500
    su = rng.integers(0, u_small, n_small).astype(np.int64)
    # every user of the small case holds both classes, so the host path returns a number
    sl = label[:n_small].copy()
    first = np.unique(su, return_index=True)[1]
    sl[first] = 1.0
    second = np.array([np.flatnonzero(su == u)[1] for u in su[first]])
    sl[second] = 0.0
    host_s, host_g = once(lambda: metric.gauc_score(sl, pred[:n_small], su))
    small = metric.gauc_score(torch.from_numpy(sl).to(dev), dp[:n_small], torch.from_numpy(su).to(dev))
    lines += [f"GAUC  N = {N} over {U} users: device {med * 1e3:.2f} ms ({lo * 1e3:.2f} .. {hi * 1e3:.2f}), value {got!r}",
              f"      host path at N = {n_small} over {u_small} users: {host_s:.2f} s; device on the same data differs by "
              f"{abs(small - host_g):.2e}"]

    # list metrics
    M, K, cut = 1_000_000, 100, (10, 50, 100)
    ids = torch.randint(0, 5000, (M, K), device=dev)
    lens = torch.randint(1, 31, (M,), device=dev)
    off = torch.zeros(M + 1, dtype=torch.int64, device=dev)
    off[1:] = torch.cumsum(lens, 0)
    truth = torch.randint(0, 5000, (int(off[-1]),), device=dev)
    med, lo, hi = timed(lambda: metric.topk_metrics((off, truth), ids, topKs=cut), args.repeat)
    m_small = 5_000
    h_off, h_truth, h_ids = off[:m_small + 1].cpu().numpy(), truth[:int(off[m_small])].cpu().numpy(), ids[:m_small].cpu()
    y_true = {u: h_truth[h_off[u]:h_off[u + 1]].tolist() for u in range(m_small)}
    y_pred = {u: row for u, row in enumerate(h_ids.tolist())}
    host_s, host_res = once(lambda: metric.topk_metrics(y_true, y_pred, topKs=cut))
    small = metric.topk_metrics((off[:m_small + 1], truth), ids[:m_small], topKs=cut)
    lines += [f"lists M = {M}, K = {K}, cut-offs {cut}, truth lists of 1-30 ids: device {med * 1e3:.2f} ms "
              f"({lo * 1e3:.2f} .. {hi * 1e3:.2f})",
              f"      host path at M = {m_small}: {host_s:.2f} s; device strings on the same data "
              f"{'equal' if dict(small) == dict(host_res) else 'DIFFER'}"]
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()
