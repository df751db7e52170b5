"""One CIN layer of csrc/cin.hip against the reference's formulation on torch ops, same device, same process, same inputs,
and one xDeepFM train step beside DeepFM's.

  layer   ops.cin_layer  vs  relu(conv1d((x0.unsqueeze(2) * h.unsqueeze(1)).view(B, F * Hp, D), W, b)), forward + backward
          through autograd at B = 4096, D = 16, (F, Hp, Ho) in {(39, 39, 200), (39, 100, 200)}: time per step and the peak
          device memory of one forward + backward above the inputs (``max_memory_allocated``)
  step    one eager ``CTRTrainer.train_step`` of xDeepFM with cin_size [200, 200] and of DeepFM on the same 26 tables of
          width 16 + 13 dense features, B = 4096

Timing as tools/twotower_bench.py: after a warm-up of both sides the two take turns, ROUNDS times each, one HIP-event pair
around a window of back-to-back steps; printed per side: the median window's time per step and the spread.
Run:  python tools/cin_bench.py [out.txt]"""
import sys

import torch

sys.path.insert(0, ".")
from tools.twotower_bench import LINES, ROUNDS, WINDOW_MS, alternate, leaf, say, step_of  # noqa: E402
from torch_rechub_amd import ops  # noqa: E402


def torch_layer(x0, h, w, b):
    z = x0.unsqueeze(2) * h.unsqueeze(1)
    return torch.relu(torch.nn.functional.conv1d(z.reshape(z.shape[0], z.shape[1] * z.shape[2], z.shape[3]), w, b))


def peak_mib(step):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    step()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def bench_layer(B, D, F, Hp, Ho):
    x0, h = leaf(B, F, D), leaf(B, Hp, D)
    w = (torch.randn(Ho, F * Hp, 1, device="cuda") / (F * Hp) ** 0.5).requires_grad_(True)
    b = leaf(Ho)
    leaves = (x0, h, w, b)
    fused = step_of(lambda: ops.cin_layer(x0, h, w, b), leaves)
    torch_side = step_of(lambda: torch_layer(x0, h, w, b), leaves)
    torch.testing.assert_close(ops.cin_layer(x0, h, w, b), torch_layer(x0, h, w, b), rtol=1e-4, atol=1e-4)
    what = f"CIN layer B={B} D={D} F={F} Hp={Hp} Ho={Ho} forward + backward"
    for t in leaves:
        t.grad = None
    mem_f = peak_mib(fused)
    for t in leaves:
        t.grad = None
    mem_t = peak_mib(torch_side)
    say(f"{what}: peak memory above the inputs: fused {mem_f:.1f} MiB, torch ops {mem_t:.1f} MiB "
        f"(one (B, F Hp, D) tensor: {B * F * Hp * D * 4 / 2**20:.1f} MiB)")
    (mf, lf, hf), (mt, lt, ht) = alternate([fused, torch_side])
    flop = 6.0 * B * D * F * Hp * Ho
    say(f"{what}: fused {mf:.3f} ms ({lf:.3f} .. {hf:.3f}; {flop / mf * 1e-9:.1f} TF/s), torch ops {mt:.3f} ms "
        f"({lt:.3f} .. {ht:.3f}), torch / fused {mt / mf:.2f}x")


def bench_step(B=4096, D=16, cin_size=(200, 200)):
    from torch_rechub_amd.basic.features import DenseFeature, SparseFeature
    from torch_rechub_amd.models.ranking import DeepFM, xDeepFM
    from torch_rechub_amd.trainers import CTRTrainer
    vocabs = [3, 4, 10, 27, 105, 305, 583, 1460, 5000, 20000, 40, 24, 633] * 2
    g = torch.Generator().manual_seed(0)
    x = {f"C{i}": torch.randint(0, v, (B,), generator=g).cuda() for i, v in enumerate(vocabs)}
    x.update({f"I{i}": torch.rand(B, generator=g).cuda() for i in range(13)})
    y = (torch.rand(B, generator=g) < 0.25).float().cuda()
    mlp = {"dims": [256, 128], "dropout": 0.0, "activation": "relu"}
    steps = []
    for cls in (xDeepFM, DeepFM):
        dense = [DenseFeature(f"I{i}") for i in range(13)]
        sparse = [SparseFeature(f"C{i}", v, D) for i, v in enumerate(vocabs)]
        args = (dense + sparse, sparse, mlp) + ((list(cin_size),) if cls is xDeepFM else ())
        trainer = CTRTrainer(cls(*args), device="cuda:0", show_progress=False)
        steps.append(lambda t=trainer: t.train_step(x, y))
    (mx, lx, hx), (md, ld, hd) = alternate(steps)
    say(f"CTRTrainer eager step B={B}, 26 tables of width {D} + 13 dense, MLP [256, 128]: xDeepFM cin_size {list(cin_size)} "
        f"{mx:.3f} ms ({lx:.3f} .. {hx:.3f}), DeepFM {md:.3f} ms ({ld:.3f} .. {hd:.3f})")


def main():
    torch.manual_seed(0)
    say("# python tools/cin_bench.py -- one MI355X, one process, both sides on the same inputs")
    say(f"device: {torch.cuda.get_device_name(0)}; {ROUNDS} alternating windows of ~{WINDOW_MS:.0f} ms per side")
    for F, Hp, Ho in ((39, 39, 200), (39, 100, 200)):
        bench_layer(4096, 16, F, Hp, Ho)
    bench_step()
    ops.check_errors()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
