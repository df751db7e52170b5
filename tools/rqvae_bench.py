"""RQ-VAE timings on the device, fused path against the reference's chain written as eager torch here, same process, same
weights, the two alternating:

  quantizer   ops.residual_quantize forward + backward at the training shape (N 512, E 32, three codebooks of 256)
  id pass     the quantizer's forward alone (no grad) over a catalogue of 2^18 rows
  step        the example's model (in_dim 2048, layers 2048 ... 64, e_dim 32, B 512, Adam): Trainer eager and captured,
              against the whole step as eager torch (nn.Linear / BatchNorm1d / ReLU, the eager quantizer, torch Adam)

Each figure is the median over ROUNDS windows of 1000 / 2000 / 100 / 100 iterations between two device events (a window
ends in a synchronise and lasts a tenth of a second or more), warm-up first; min and max of the windows are printed beside it.  One JSON line at the end."""
import json
import statistics
import sys

import torch
import torch.nn.functional as F
from torch import nn

sys.path.insert(0, ".")
from torch_rechub_amd import ops  # noqa: E402
from torch_rechub_amd.models.generative import RQVAEModel  # noqa: E402
from torch_rechub_amd.trainers.rqvae_trainer import Trainer  # noqa: E402

E, SIZES, BETA = 32, [256, 256, 256], 0.25
IN_DIM, LAYERS, B = 2048, [2048, 1024, 512, 256, 128, 64], 512
ROUNDS = 7


def windows_ms(fns, iters, warmup=10):
    """{name: [ms per iteration of each window]} for the named callables, their windows alternating."""
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


def report(what, w, base):
    res = {}
    for name, ts in w.items():
        res[name] = statistics.median(ts)
        print(f"{what}: {name:22s} {res[name] * 1e3:9.1f} us  (min {min(ts) * 1e3:.1f}, max {max(ts) * 1e3:.1f})")
    for name in res:
        if name != base:
            print(f"{what}: {base} / {name} = {res[base] / res[name]:.2f}x")
    return res


def eager_rq(x, codebooks, beta):
    """rqvae.py:241-274 and :382-398 with every epsilon 0, as the reference composes them from ATen ops."""
    all_losses, all_indices, x_q, residual = [], [], 0, x
    for C in codebooks:
        d = torch.sum(residual**2, dim=1, keepdim=True) + torch.sum(C**2, dim=1, keepdim=True).t() - 2 * torch.matmul(residual, C.t())
        indices = torch.argmin(d, dim=-1)
        q = F.embedding(indices, C)
        loss = F.mse_loss(q, residual.detach()) + beta * F.mse_loss(q.detach(), residual)
        q = residual + (q - residual).detach()
        residual = residual - q
        x_q = x_q + q
        all_losses.append(loss)
        all_indices.append(indices)
    return x_q, torch.stack(all_losses).mean(), torch.stack(all_indices, dim=-1)


class EagerRQVAE(nn.Module):
    """The reference's model as plain torch modules."""

    def __init__(self):
        super().__init__()

        def mlp(dims):
            mods = []
            for a, b in zip(dims[:-1], dims[1:]):
                mods += [nn.Linear(a, b), nn.BatchNorm1d(b), nn.ReLU(), nn.Dropout(0.0)]
            return nn.Sequential(*mods)
        dims = [IN_DIM] + LAYERS + [E]
        self.encoder, self.decoder = mlp(dims), mlp(dims[::-1])
        self.codebooks = nn.ParameterList([nn.Parameter(torch.randn(n, E) * 0.5) for n in SIZES])

    def forward(self, x):
        x_q, rq_loss, indices = eager_rq(self.encoder(x), list(self.codebooks), BETA)
        return self.decoder(x_q), rq_loss, indices


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    result = {}

    x = torch.randn(512, E, device=dev, requires_grad=True)
    cbs = [(0.5 * torch.randn(n, E, device=dev)).requires_grad_(True) for n in SIZES]
    g_xq, g_loss = torch.randn(512, E, device=dev), torch.tensor(1.0, device=dev)

    def both(fn):
        def run():
            x.grad = None
            for c in cbs:
                c.grad = None
            x_q, loss, _ = fn(x, cbs, BETA)
            torch.autograd.backward([x_q, loss], [g_xq, g_loss])
        return run

    w = windows_ms({"fused": both(ops.residual_quantize), "eager": both(eager_rq)}, iters=1000)
    result["quantizer_fwd_bwd_512x32_3x256_ms"] = report("quantizer fwd+bwd (512, 32, [256]x3)", w, "eager")
    with torch.no_grad():
        w = windows_ms({"fused": lambda: ops.residual_quantize(x, cbs, BETA), "eager": lambda: eager_rq(x, cbs, BETA)}, iters=2000)
    result["quantizer_fwd_512x32_3x256_ms"] = report("quantizer fwd (512, 32, [256]x3)", w, "eager")

    big = torch.randn(1 << 18, E, device=dev)
    with torch.no_grad():
        a, b = ops.residual_quantize(big, cbs, BETA), eager_rq(big, cbs, BETA)
        agree = float((a[2] == b[2]).all(1).float().mean())
        w = windows_ms({"fused": lambda: ops.residual_quantize(big, cbs, BETA), "eager": lambda: eager_rq(big, cbs, BETA)},
                       iters=100, warmup=3)
    print(f"id pass: rows with the same IDs on both paths: {agree:.6f}")
    result["id_pass_262144x32_3x256_ms"] = report("id pass (2^18, 32, [256]x3)", w, "eager")
    result["id_pass_rows_agreeing"] = agree

    def build():
        torch.manual_seed(1)
        m = RQVAEModel(in_dim=IN_DIM, num_emb_list=list(SIZES), e_dim=E, layers=list(LAYERS), beta=BETA, kmeans_init=False,
                       sk_epsilons=[0.0, 0.0, 0.0])
        with torch.no_grad():
            for vq in m.rq.vq_layers:
                vq.embedding.weight.normal_(0, 0.5)
        return m

    opt = {"lr": 1e-3, "weight_decay": 1e-5}
    t_eager, t_graph = Trainer(build(), device="cuda:0", optimizer_params=dict(opt)), \
        Trainer(build(), device="cuda:0", optimizer_params=dict(opt), use_graph=True)
    t_eager.model.train(), t_graph.model.train()
    ref = EagerRQVAE().to(dev).train()
    ref_opt = torch.optim.Adam(ref.parameters(), **opt)
    data = torch.randn(B, IN_DIM, device=dev)

    def ref_step():
        ref_opt.zero_grad()
        out, rq_loss, _ = ref(data)
        loss = F.mse_loss(out, data, reduction="mean") + rq_loss
        loss.backward()
        ref_opt.step()

    w = windows_ms({"Trainer eager": lambda: t_eager.train_step(data), "Trainer captured": lambda: t_graph.train_step(data),
                    "eager torch step": ref_step}, iters=100)
    assert len(t_graph._graphs) == 1
    result["step_B512_ms"] = report("train step (B 512, in_dim 2048)", w, "eager torch step")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
