"""Multi-interest top-K retrieval on the device: ``ops.topk_items_multi`` (csrc/topk_multi.hip, one K-list per user) against
the formulation a user had before it, on kernels that were already there -- ``ops.topk_items`` over the flattened (M I, D)
queries, then the merge in torch: reshape to (M, I K), keep the best entry of every id, order by (score descending, id
ascending), first K.  Same process, same tensors, the two alternating (the windows of tools/topk_bench.py):

  comirec     M = 4096 users, I = 4, V = 4096 items, K = 200     (ComiRec / MIND on MovieLens-size data)
  catalogue   M = 1024, I = 4 and 8, V = 2^20, K = 10
  sine        M = 1024, I = 8, V = 2^20, K = 50

all at D = 64, unit-Gaussian rows, for an fp32 and an fp16 table.  Each figure is the median over ROUNDS windows of ``iters``
calls between two device events (a window ends in a synchronise), warm-up first, min - max beside it.  Peak memory is
torch.cuda.max_memory_allocated above what was allocated before one call.  The ids and scores of the two sides are compared
on the timed inputs.  The lines are also written to ``--out`` (default profiles/topk_multi_bench.txt); one JSON line at
the end."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, ".")
from tools.topk_bench import peak_bytes, windows_ms  # noqa: E402
from torch_rechub_amd import ops  # noqa: E402

SHAPES = [("comirec", 4096, 4, 4096, 200, 20), ("catalogue", 1024, 4, 1 << 20, 10, 5),
          ("catalogue", 1024, 8, 1 << 20, 10, 5), ("sine", 1024, 8, 1 << 20, 50, 5)]


def flat_then_merge(q, x, K):
    M, I, D = q.shape
    ids, sc = ops.topk_items(q.reshape(M * I, D), x, K)
    ids, sc = ids.reshape(M, I * K), sc.reshape(M, I * K)
    o = torch.argsort(sc, dim=1, descending=True, stable=True)
    ids, sc = ids.gather(1, o), sc.gather(1, o)
    o = torch.argsort(ids, dim=1, stable=True)  # by id, the best score of an id first
    ids, sc = ids.gather(1, o), sc.gather(1, o)
    repeated = torch.zeros_like(ids, dtype=torch.bool)
    repeated[:, 1:] = ids[:, 1:] == ids[:, :-1]
    ids, sc = ids.masked_fill(repeated, -1), sc.masked_fill(repeated, float("-inf"))
    o = torch.argsort(sc, dim=1, descending=True, stable=True)[:, :K]  # ids already ascend: (score descending, id ascending)
    return ids.gather(1, o), sc.gather(1, o)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="profiles/topk_multi_bench.txt")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    result, lines = {}, []

    def say(line):
        print(line, flush=True)
        lines.append(line)

    for name, M, I, V, K, iters in SHAPES:
        q, x32 = torch.randn(M, I, 64, device=dev), torch.randn(V, 64, device=dev)
        for x in (x32, x32.half()):
            what = f"{name} (M {M}, I {I}, D 64, V {V}, K {K}, {str(x.dtype)[6:]})"
            fns = {"multi": lambda: ops.topk_items_multi(q, x, K), "flat+merge": lambda: flat_then_merge(q, x, K)}
            res = {}
            for n, ts in windows_ms(fns, iters).items():
                res[n + "_ms"] = statistics.median(ts)
                res[n + "_peak_bytes"] = peak_bytes(fns[n])
                say(f"{what}: {n:10s} {res[n + '_ms']:9.3f} ms  (min {min(ts):.3f}, max {max(ts):.3f})  peak "
                    f"{res[n + '_peak_bytes'] / 2**20:8.1f} MiB")
            (mi, ms), (fi, fs) = fns["multi"](), fns["flat+merge"]()
            res["multi_over_flat"] = res["multi_ms"] / res["flat+merge_ms"]
            res["equal"] = bool(torch.equal(mi, fi) and torch.equal(ms, fs))
            say(f"{what}: multi / flat+merge = {res['multi_over_flat']:.3f}; ids and scores of the two sides equal: "
                f"{res['equal']}")
            result[f"{name}_I{I}_K{K}_{str(x.dtype)[6:]}"] = res
        del q, x32, x, fns
    say(json.dumps(result))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
