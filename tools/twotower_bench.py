"""The three two-tower tails of csrc/twotower.hip against the reference's formulation on torch ops, same device, same
process, same inputs.  Timed is the TAIL alone, forward + backward from given tower outputs (the towers in front of it are the
same code on both sides):

  YoutubeSBC   ops.band_logits  vs  cosine_similarity(u.unsqueeze(1), v, dim=2) - log(w), [index0, index1], / T
               at B in {512, 4096}, D in {16, 64}, n_neg = 3; also the peak device memory of ONE forward on each side
  FaceBookDSSM ops.pair_cosine_scores  vs  three F.normalize + two multiply-sums, B in {512, 4096}, D in {16, 64}
  SENet        ops.senet  vs  mean, Linear, ReLU, Linear, ReLU, scale, B in {512, 4096}, (F, D) in {(6, 16), (26, 16)}

After a warm-up of both sides the two take turns, ROUNDS times each: one HIP-event pair around a window of back-to-back
steps, the window sized (from a calibration run) to about WINDOW_MS.  Printed per side: the median window's time per step
and the spread (fastest .. slowest window).  Run:  python tools/twotower_bench.py [out.txt]"""
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from torch_rechub_amd import ops  # noqa: E402

ROUNDS, WARMUP, WINDOW_MS = 7, 10, 200.0
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def window_ms(fn, steps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def alternate(fns):
    """Per function (median, fastest, slowest) time per step in ms over ROUNDS windows, the functions taking turns."""
    steps = []
    for fn in fns:
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        steps.append(max(5, min(2000, int(WINDOW_MS / max(window_ms(fn, 5), 1e-3)))))
    times = [[] for _ in fns]
    for _ in range(ROUNDS):
        for t, fn, n in zip(times, fns, steps):
            t.append(window_ms(fn, n))
    return [(statistics.median(t), min(t), max(t)) for t in times]


def report(what, fused, torch_side):
    (mf, lf, hf), (mt, lt, ht) = alternate([fused, torch_side])
    say(f"{what}: fused {mf * 1e3:.1f} us ({lf * 1e3:.1f} .. {hf * 1e3:.1f}), torch ops {mt * 1e3:.1f} us "
        f"({lt * 1e3:.1f} .. {ht * 1e3:.1f}), torch / fused {mt / mf:.2f}x")


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return peak / 2**20


def leaf(*shape):
    return torch.randn(*shape, device="cuda").requires_grad_(True)


def step_of(forward, leaves):
    """forward + backward of a scalar made from every output, gradients dropped before each step."""
    def step():
        for t in leaves:
            t.grad = None
        out = forward()
        out = out if isinstance(out, tuple) else (out,)
        sum(o.sum() for o in out).backward()
    return step


def bench_band(B, D, n_neg=3, temp=0.05):
    u, v = leaf(B, D), leaf(B, D)
    w = torch.rand(B, device="cuda") * 0.95 + 0.05
    rows = np.repeat(np.arange(B), n_neg + 1)
    index0 = torch.from_numpy(rows).cuda()
    index1 = torch.from_numpy((rows + np.tile(np.arange(n_neg + 1), B)) % B).cuda()

    def fused():
        return ops.band_logits(u, v, w, n_neg, temp)

    def torch_side():
        pred = torch.cosine_similarity(u.unsqueeze(1), v, dim=2)
        return ((pred - torch.log(w))[index0, index1] / temp).view(-1, n_neg + 1)

    torch.testing.assert_close(fused(), torch_side(), rtol=1e-4, atol=1e-4)
    with torch.no_grad():
        mem_f, mem_t = peak_mib(fused), peak_mib(torch_side)
    say(f"YoutubeSBC tail B={B} D={D} n_neg={n_neg}: peak memory of one forward: fused {mem_f:.2f} MiB, torch ops {mem_t:.2f} MiB")
    report(f"YoutubeSBC tail B={B} D={D} n_neg={n_neg} forward + backward", step_of(fused, (u, v)), step_of(torch_side, (u, v)))


def bench_pair(B, D):
    hs = [leaf(B, D) for _ in range(3)]

    def fused():
        return ops.pair_cosine_scores(*hs)

    def torch_side():
        u, p, n = (F.normalize(h, p=2, dim=1) for h in hs)
        return torch.mul(u, p).sum(dim=1), torch.mul(u, n).sum(dim=1)

    report(f"FaceBookDSSM tail B={B} D={D} forward + backward", step_of(fused, hs), step_of(torch_side, hs))


def bench_senet(B, Fn, D, ratio=3):
    x = leaf(B, Fn, D)
    R = max(1, Fn // ratio)
    w1, w2 = leaf(R, Fn), leaf(Fn, R)

    def fused():
        return ops.senet(x, w1, w2)

    def torch_side():
        a = torch.relu(F.linear(torch.relu(F.linear(torch.mean(x, dim=-1), w1)), w2))
        return x * a.unsqueeze(-1)

    report(f"SENet gate B={B} F={Fn} R={R} D={D} forward + backward", step_of(fused, (x, w1, w2)), step_of(torch_side, (x, w1, w2)))


def main():
    torch.manual_seed(0)
    say(f"device: {torch.cuda.get_device_name(0)}; {ROUNDS} alternating windows of ~{WINDOW_MS:.0f} ms per side")
    for B in (512, 4096):
        for D in (16, 64):
            bench_band(B, D)
    for B in (512, 4096):
        for D in (16, 64):
            bench_pair(B, D)
    for B in (512, 4096):
        for Fn in (6, 26):
            bench_senet(B, Fn, 16)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
