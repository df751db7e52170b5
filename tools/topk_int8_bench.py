"""int8 (SQ8) item tables against fp32 and fp16 ones on the device (csrc/topk_q8.hip, topk_half.hip, topk.hip), same
process, same tensors, the paths alternating (the windows of tools/topk_bench.py):

  catalogue   V = 2^20 items, D = 64, M = 1024 queries, K = 10         unit-Gaussian rows
  movielens   V = 4096 items, D = 64, M = 4096 queries, K = 200        unit-Gaussian rows
  ivf         the Gaussian mixture of tools/ivf_bench.py (V = 2^20, D = 64, M = 1024, 1024 lists), "L2", K = 10, nprobe = 8

The int8 time is a whole query, ``ops.topk_items_int8`` with its quantise launch; ``quantise`` is that launch alone
(``ops.quantize_rows_int8`` of the queries).  Each figure is the median over ROUNDS windows of ``iters`` calls between two
device events, warm-up first, min - max beside it.  Resident bytes are the tensors an index keeps (table or codes + scales;
bias and lists are the same for all).  recall@K is the share of the fp32 flat answer's ids the int8 answer holds.  The lines
are also written to ``--out`` (default profiles/topk_int8_bench.txt); one JSON line at the end."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from tools.ivf_bench import M as IVF_M, D as IVF_D, V as IVF_V, NLISTS, mixture  # noqa: E402
from tools.topk_bench import windows_ms  # noqa: E402
from torch_rechub_amd import ops  # noqa: E402
from torch_rechub_amd.serving import builder_factory  # noqa: E402

SHAPES = [("catalogue", 1024, 64, 1 << 20, 10, 20), ("movielens", 4096, 64, 4096, 200, 100)]


def recall(got, want):
    hit = (got.unsqueeze(2) == want.unsqueeze(1)).any(dim=2) & (got >= 0)
    return float(hit.sum()) / float((want >= 0).sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/topk_int8_bench.txt")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    result, lines = {}, []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    def report(what, w, base):
        res = {}
        for n, ts in w.items():
            res[n + "_ms"] = statistics.median(ts)
            say(f"{what}: {n:9s} {res[n + '_ms']:9.3f} ms  (min {min(ts):.3f}, max {max(ts):.3f})")
        for n in w:
            if n not in (base, "quantise"):
                res[n + "_over_" + base] = res[n + "_ms"] / res[base + "_ms"]
        say(f"{what}: " + ", ".join(f"{k.replace('_over_', ' / ')} = {v:.3f}" for k, v in res.items() if "_over_" in k))
        return res

    for name, M, D, V, K, iters in SHAPES:
        q, x = torch.randn(M, D, device=dev), torch.randn(V, D, device=dev)
        xh = x.half()
        codes, scale = ops.quantize_rows_int8(x)
        fns = {"fp32": lambda: ops.topk_items(q, x, K), "fp16": lambda: ops.topk_items(q, xh, K),
               "int8": lambda: ops.topk_items_int8(q, codes, scale, K), "quantise": lambda: ops.quantize_rows_int8(q)}
        what = f"{name} (M {M}, D {D}, V {V}, K {K})"
        res = report(what, windows_ms(fns, iters), "fp32")
        res["recall"] = recall(fns["int8"]()[0], fns["fp32"]()[0])
        res["resident_bytes"] = {"fp32": x.numel() * 4, "fp16": xh.numel() * 2, "int8": codes.numel() + scale.numel() * 4}
        say(f"{what}: recall@{K} of int8 against fp32 (unit-Gaussian rows) {res['recall']:.4f}; resident bytes "
            + ", ".join(f"{n} {b / 2**20:.1f} MiB" for n, b in res["resident_bytes"].items()))
        result[f"{name}_K{K}"] = res
        del q, x, xh, codes, scale, fns

    g = torch.Generator(device=dev).manual_seed(0)
    centres = 4.0 * torch.randn(NLISTS, IVF_D, generator=g, device=dev)
    x, q = mixture(IVF_V, centres, g), mixture(IVF_M, centres, g)
    K, nprobe = 10, 8
    with builder_factory("hip").from_embeddings(x) as flat, \
            builder_factory("hip", index_type="IVF", nlists=NLISTS, nprobe=nprobe, niter=10).from_embeddings(x) as ivf:
        half = type(ivf)(x, ivf.centroids, "L2", dev, nprobe, torch.float16)
        sq8 = type(ivf)(x, ivf.centroids, "L2", dev, nprobe, None, "SQ8")
        flat8 = type(flat)(x, "L2", dev, None, "SQ8")
        what = f"ivf (M {IVF_M}, D {IVF_D}, V {IVF_V}, nlists {NLISTS}, L2, K {K}, nprobe {nprobe})"
        fns = {"fp32": lambda: ivf.query(q, K), "fp16": lambda: half.query(q, K), "int8": lambda: sq8.query(q, K)}
        res = report(what, windows_ms(fns, 10), "fp32")
        want = flat.query(q, K)[0]
        res["recall"] = {"fp32_ivf": recall(ivf.query(q, K)[0], want), "int8_ivf": recall(sq8.query(q, K)[0], want),
                         "int8_flat": recall(flat8.query(q, K)[0], want)}
        say(f"{what}: recall@{K} against the fp32 flat index (mixture): "
            + ", ".join(f"{n} {r:.4f}" for n, r in res["recall"].items()))
        result["ivf"] = res
    say(json.dumps(result))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
