"""AutoInt's interacting layer of csrc/interact.hip against the torch formulation the layer keeps as its fallback
(``InteractingLayer.forward_torch``), same device, same process, same parameters and inputs, and one AutoInt train step
through each.

  layer   forward + backward of one layer at (B, F, D, H) in {(4096, 39, 16, 2), (4096, 13, 64, 4), (65536, 39, 16, 2)}: time
          per step and the peak device memory of one forward + backward above the inputs (``max_memory_allocated``)
  step    one eager ``CTRTrainer.train_step`` of AutoInt (26 tables of width 16 + 13 dense fields = 39 fields, three layers of
          two heads, MLP [256, 128]) at B = 4096, with the layers on the kernel and with ``forward`` bound to
          ``forward_torch`` (the step before this kernel)

Timing as tools/twotower_bench.py: after a warm-up of both sides the two take turns, ROUNDS times each, one HIP-event pair
around a window of back-to-back steps; printed per side: the median window's time per step and the spread.
Run:  python tools/autoint_bench.py [out.txt]"""
import sys

import torch

sys.path.insert(0, ".")
from tools.twotower_bench import LINES, ROUNDS, WINDOW_MS, alternate, leaf, say, step_of  # noqa: E402
from tools.cin_bench import peak_mib  # noqa: E402
from torch_rechub_amd import ops  # noqa: E402
from torch_rechub_amd.basic.layers import InteractingLayer  # noqa: E402


def bench_layer(B, F, D, H):
    layer = InteractingLayer(D, num_heads=H).cuda()
    x = leaf(B, F, D)
    leaves = (x,) + tuple(layer.parameters())
    fused = step_of(lambda: layer(x), leaves)
    torch_side = step_of(lambda: layer.forward_torch(x), leaves)
    torch.testing.assert_close(layer(x), layer.forward_torch(x), rtol=1e-4, atol=1e-4)
    what = f"InteractingLayer B={B} F={F} D={D} H={H} forward + backward"
    for t in leaves:
        t.grad = None
    mem_f = peak_mib(fused)
    for t in leaves:
        t.grad = None
    mem_t = peak_mib(torch_side)
    say(f"{what}: peak memory above the inputs: fused {mem_f:.1f} MiB, torch ops {mem_t:.1f} MiB "
        f"(x: {B * F * D * 4 / 2**20:.1f} MiB, one (B, H, F, F) tensor: {B * H * F * F * 4 / 2**20:.1f} MiB)")
    (mf, lf, hf), (mt, lt, ht) = alternate([fused, torch_side])
    say(f"{what}: fused {mf:.3f} ms ({lf:.3f} .. {hf:.3f}), torch ops {mt:.3f} ms ({lt:.3f} .. {ht:.3f}), "
        f"torch / fused {mt / mf:.2f}x")


def bench_step(B=4096, D=16):
    from torch_rechub_amd.basic.features import DenseFeature, SparseFeature
    from torch_rechub_amd.models.ranking import AutoInt
    from torch_rechub_amd.trainers import CTRTrainer
    vocabs = [3, 4, 10, 27, 105, 305, 583, 1460, 5000, 20000, 40, 24, 633] * 2
    g = torch.Generator().manual_seed(0)
    x = {f"C{i}": torch.randint(0, v, (B,), generator=g).cuda() for i, v in enumerate(vocabs)}
    x.update({f"I{i}": torch.rand(B, generator=g).cuda() for i in range(13)})
    y = (torch.rand(B, generator=g) < 0.25).float().cuda()
    steps = []
    for kernel in (True, False):
        dense = [DenseFeature(f"I{i}") for i in range(13)]
        sparse = [SparseFeature(f"C{i}", v, D) for i, v in enumerate(vocabs)]
        model = AutoInt(sparse, dense, num_layers=3, num_heads=2,
                        mlp_params={"dims": [256, 128], "dropout": 0.0, "activation": "relu"})
        if not kernel:
            for layer in model.interacting_layers:
                layer.forward = layer.forward_torch
        trainer = CTRTrainer(model, device="cuda:0", show_progress=False)
        steps.append(lambda t=trainer: t.train_step(x, y))
    (mk, lk, hk), (mt, lt, ht) = alternate(steps)
    say(f"CTRTrainer eager step of AutoInt B={B}, 39 fields of width {D}, 3 layers x 2 heads, MLP [256, 128]: layers on the "
        f"kernel {mk:.3f} ms ({lk:.3f} .. {hk:.3f}), on torch ops {mt:.3f} ms ({lt:.3f} .. {ht:.3f})")


def main():
    torch.manual_seed(0)
    say("# python tools/autoint_bench.py -- one MI355X, one process, both sides on the same inputs")
    say(f"device: {torch.cuda.get_device_name(0)}; {ROUNDS} alternating windows of ~{WINDOW_MS:.0f} ms per side")
    for shape in ((4096, 39, 16, 2), (4096, 13, 64, 4), (65536, 39, 16, 2)):
        bench_layer(*shape)
    bench_step()
    ops.check_errors()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
