"""FiBiNET's bilinear interaction of csrc/bilinear.hip against the torch formulation the layer keeps as its fallback
(``BiLinearInteractionLayer.forward_torch``: the raw and the gated branch and their ``cat``, FiBiNet's forward before the
kernel), same device, same process, same parameters and inputs, and one FiBiNet train step through each.

  layer   forward + backward of one layer call with a gate, both branches, at (B, F, D) in {(4096, 26, 16), (4096, 24, 40),
          (65536, 26, 16)} for each bilinear type: time per step and the peak device memory of one forward + backward above
          the inputs (``max_memory_allocated``).  The upstream gradient is a dense tensor made once.
  step    one eager ``CTRTrainer.train_step`` of FiBiNet (26 tables of width 16, MLP [256, 128]) at B = 4096, with the layer
          on the kernel and with ``forward`` bound to ``forward_torch`` (the step before this kernel)

Timing as tools/twotower_bench.py: after a warm-up of both sides the two take turns, ROUNDS times each, one HIP-event pair
around a window of back-to-back steps; printed per side: the median window's time per step and the spread.
Run:  python tools/bilinear_bench.py [out.txt] [--layer-only]"""
import sys

import torch

sys.path.insert(0, ".")
from tools.twotower_bench import LINES, ROUNDS, WINDOW_MS, alternate, leaf, say  # noqa: E402
from tools.cin_bench import peak_mib  # noqa: E402
from torch_rechub_amd import ops  # noqa: E402
from torch_rechub_amd.basic.layers import BiLinearInteractionLayer  # noqa: E402


def bench_layer(B, F, D, kind):
    layer = BiLinearInteractionLayer(D, F, kind).cuda()
    x = leaf(B, F, D)
    gate = torch.relu(torch.randn(B, F, device="cuda")).requires_grad_(True)
    P = F * (F - 1) // 2
    gy = torch.randn(B, 2 * P, D, device="cuda")
    leaves = (x, gate) + tuple(layer.parameters())

    def step_of(forward):
        def step():
            for t in leaves:
                t.grad = None
            forward(x, gate).backward(gy)
        return step

    fused, torch_side = step_of(layer), step_of(layer.forward_torch)
    assert ops.bilinear_interaction_ok(x, layer.stacked_weight(), kind, gate)
    torch.testing.assert_close(layer(x, gate), layer.forward_torch(x, gate), rtol=1e-4, atol=1e-4)
    what = f"BiLinearInteractionLayer {kind} B={B} F={F} D={D} both branches forward + backward"
    mem = []
    for side in (fused, torch_side):
        side()
        for t in leaves:
            t.grad = None
        mem.append(peak_mib(side))
    say(f"{what}: peak memory above the inputs: fused {mem[0]:.1f} MiB, torch ops {mem[1]:.1f} MiB "
        f"(the (B, 2 P, D) result: {B * 2 * P * D * 4 / 2**20:.1f} MiB)")
    (mf, lf, hf), (mt, lt, ht) = alternate([fused, torch_side])
    say(f"{what}: fused {mf:.3f} ms ({lf:.3f} .. {hf:.3f}), torch ops {mt:.3f} ms ({lt:.3f} .. {ht:.3f}), "
        f"torch / fused {mt / mf:.2f}x")


def bench_step(B=4096, D=16):
    from torch_rechub_amd.basic.features import SparseFeature
    from torch_rechub_amd.models.ranking import FiBiNet
    from torch_rechub_amd.trainers import CTRTrainer
    vocabs = [3, 4, 10, 27, 105, 305, 583, 1460, 5000, 20000, 40, 24, 633] * 2
    g = torch.Generator().manual_seed(0)
    x = {f"C{i}": torch.randint(0, v, (B,), generator=g).cuda() for i, v in enumerate(vocabs)}
    y = (torch.rand(B, generator=g) < 0.25).float().cuda()
    steps = []
    for kernel in (True, False):
        sparse = [SparseFeature(f"C{i}", v, D) for i, v in enumerate(vocabs)]
        model = FiBiNet(sparse, {"dims": [256, 128], "dropout": 0.0, "activation": "relu"})
        if not kernel:
            model.bilinear_interaction.forward = model.bilinear_interaction.forward_torch
        trainer = CTRTrainer(model, device="cuda:0", show_progress=False)
        steps.append(lambda t=trainer: t.train_step(x, y))
    (mk, lk, hk), (mt, lt, ht) = alternate(steps)
    say(f"CTRTrainer eager step of FiBiNet B={B}, 26 fields of width {D}, field_interaction, MLP [256, 128]: layer on the "
        f"kernel {mk:.3f} ms ({lk:.3f} .. {hk:.3f}), on torch ops {mt:.3f} ms ({lt:.3f} .. {ht:.3f})")


def main():
    torch.manual_seed(0)
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    say("# python tools/bilinear_bench.py -- one MI355X, one process, both sides on the same inputs")
    say(f"device: {torch.cuda.get_device_name(0)}; {ROUNDS} alternating windows of ~{WINDOW_MS:.0f} ms per side")
    for shape in ((4096, 26, 16), (4096, 24, 40), (65536, 26, 16)):
        for kind in ops.BILINEAR_KINDS:
            bench_layer(*shape, kind)
    if "--layer-only" not in sys.argv:
        bench_step()
    ops.check_errors()
    if args:
        with open(args[0], "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
