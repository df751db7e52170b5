"""MMOE / PLE train step and expert bank alone, the grouped kernels of csrc/experts.hip against the per-expert path they
replace (``ops.expert_bank_ok`` forced false: the parent's code, untouched).  The two paths run in alternating fresh child
processes on one device; the table goes to profiles/experts_bench.txt.

    python tools/mtl_bench.py                 # all shapes, both paths, writes the table
    python tools/mtl_bench.py --child fused   # one process, one path: a JSON line per shape
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
B = 4096
SHAPES = {  # name -> (model, kwargs)
    "mmoe 8x[16] T2": ("mmoe", dict(n_expert=8, dims=[16])),
    "mmoe 8x[512,256] T2": ("mmoe", dict(n_expert=8, dims=[512, 256])),
    "ple L2 4+4x[512,256] T2": ("ple", dict(n_level=2, specific=4, shared=4, dims=[512, 256])),
    "ple L1 2+1x[16] T2": ("ple", dict(n_level=1, specific=2, shared=1, dims=[16])),
}


def build(kind, kw):
    from torch_rechub_amd.basic.features import SparseFeature
    from torch_rechub_amd.models.multi_task import MMOE, PLE
    feats = [SparseFeature(f"f{i}", 1000, 16) for i in range(16)]  # input width 256
    types, towers = ["classification"] * 2, [{"dims": [8]}, {"dims": [8]}]
    body = {"dims": kw["dims"], "dropout": 0.0, "activation": "relu"}
    if kind == "mmoe":
        return MMOE(feats, types, kw["n_expert"], body, towers), feats
    return PLE(feats, types, kw["n_level"], kw["specific"], kw["shared"], body, towers), feats


def timed(fn, warmup, steps, repeats):
    import torch
    for _ in range(warmup):
        fn()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(steps):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / steps)
    return out


def child(path, warmup, steps, repeats):
    import torch
    from torch_rechub_amd import ops
    if path == "parent":
        ops.expert_bank_ok = lambda *a: False
    dev = torch.device("cuda:0")
    for name, (kind, kw) in SHAPES.items():
        torch.manual_seed(0)
        model, feats = build(kind, kw)
        model = model.to(dev).train()
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        x = {f.name: torch.randint(0, 1000, (B,), device=dev) for f in feats}
        y = (torch.rand(B, 2, device=dev) < 0.3).float()
        emb = torch.randn(B, 256, device=dev, requires_grad=True)

        def step():
            opt.zero_grad(set_to_none=True)
            torch.nn.functional.binary_cross_entropy(model(x), y).backward()
            opt.step()

        def bank():  # the experts, gates and mixtures alone, forward + backward, from a given (B, 256) input
            if kind == "mmoe":
                E, T = model.n_expert, model.n_task
                args = ([emb], list(model.experts), [0] * E, list(model.gates), [0] * T, [list(range(E))] * T)
                if ops.expert_bank_ok(*args):
                    outs = ops.expert_bank(*args)
                else:
                    from torch_rechub_amd.models.multi_task._common import gate_mix
                    ex = torch.stack([e(emb) for e in model.experts], dim=1)
                    outs = [gate_mix(g(emb), ex) for g in model.gates]
            else:
                outs = [emb] * (model.n_task + 1)
                for layer in model.cgc_layers:
                    outs = layer(outs)
            torch.cat(outs, 1).sum().backward()

        torch.cuda.reset_peak_memory_stats()
        t_step = timed(step, warmup, steps, repeats)
        peak = torch.cuda.max_memory_allocated() / 2 ** 20
        t_bank = timed(bank, warmup, steps, repeats)
        print(json.dumps(dict(shape=name, path=path, step_ms=t_step, bank_ms=t_bank, peak_mib=peak)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", choices=["fused", "parent"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "experts_bench.txt"))
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.warmup, a.steps, a.repeats)
    rows = {}
    for _ in range(a.rounds):
        for path in ("parent", "fused"):  # alternating fresh processes
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", path, "--warmup", str(a.warmup), "--steps",
                                str(a.steps), "--repeats", str(a.repeats)], capture_output=True, text=True, timeout=600)
            if r.returncode != 0:
                sys.exit(f"child {path} failed ({r.returncode}):\n{r.stderr[-2000:]}")
            for line in r.stdout.splitlines():
                if line.startswith("{"):
                    d = json.loads(line)
                    e = rows.setdefault((d["shape"], d["path"]), dict(step=[], bank=[], peak=[]))
                    e["step"] += d["step_ms"]
                    e["bank"] += d["bank_ms"]
                    e["peak"].append(d["peak_mib"])
    lines = [f"B = {B}, 16 sparse features x 16 (input width 256), 2 tasks, eager Adam step; {a.rounds} alternating processes per path, "
             f"{a.repeats} x {a.steps} steps each; median [min .. max] ms", ""]
    for name in SHAPES:
        for what in ("step", "bank"):
            p, f = rows[(name, "parent")][what], rows[(name, "fused")][what]
            lines.append(f"{name:26s} {what:4s}  parent {statistics.median(p):7.3f} [{min(p):7.3f} .. {max(p):7.3f}]   "
                         f"grouped {statistics.median(f):7.3f} [{min(f):7.3f} .. {max(f):7.3f}]   "
                         f"x{statistics.median(p) / statistics.median(f):.2f}")
        lines.append(f"{name:26s} peak  parent {max(rows[(name, 'parent')]['peak']):8.1f} MiB   grouped "
                     f"{max(rows[(name, 'fused')]['peak']):8.1f} MiB")
    text = "\n".join(lines) + "\n"
    print(text)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
