"""SINE's user tower at the example's configuration (S = 50, E = 128, hidden_dim 512, T = 10, K = 2, temperature 0.1) at
B = 256 and 4096, forward + backward: the fused path (models/matching/sine.py on csrc/sine.hip) against the reference's
own chain (sine.py:86-128) written as eager torch on the same device and the same weights.  One process, warm-up, the
median of HIP-event timings of single iterations; and the four fused kernels alone."""
import statistics
import sys

import torch
import torch.nn.functional as F
from torch import einsum

sys.path.insert(0, ".")
from torch_rechub_amd import ops  # noqa: E402
from torch_rechub_amd.models.matching import SINE  # noqa: E402

S, E, H, T, K, V, TEMP = 50, 128, 512, 10, 2, 4000, 0.1


def median_ms(fn, iters=30, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def eager_user_tower(m, hist):
    """The reference's user tower as it composes it from ATen ops."""
    x_u = m.item_embedding(hist) + m.position_embedding.weight.unsqueeze(0)
    mask = (hist > 0).long()
    h_1 = einsum("bse, ed -> bsd", x_u, m.w_1).tanh()
    a_hist = F.softmax(einsum("bsd, dh -> bsh", h_1, m.w_2) + -1.e9 * (1 - mask.unsqueeze(-1).float()), dim=1)
    z_u = einsum("bse, bsh -> be", x_u, a_hist)
    s_u = einsum("be, te -> bt", z_u, m.concept_embedding.weight)
    top = torch.topk(s_u, m.num_intention)
    c_u = einsum("bk, bke -> bke", torch.sigmoid(top.values), m.concept_embedding(top.indices))
    p_u = F.softmax(einsum("bse, bke -> bks", F.normalize(x_u @ m.w_3, dim=-1), F.normalize(c_u, p=2, dim=-1)), dim=1)
    h_2 = einsum("bse, ed -> bsd", x_u, m.w_k1).tanh()
    a_k = F.softmax(einsum("bsd, dk -> bsk", h_2, m.w_k2) + -1.e9 * (1 - mask.unsqueeze(-1).float()), dim=1)
    phi_u = einsum("bks, bse -> bke", p_u * a_k.permute(0, 2, 1), x_u)
    x_hat = einsum("bks, bke -> bse", p_u, c_u)
    h_3 = einsum("bse, ed -> bsd", x_hat, m.w_4).tanh()
    c_apt = F.normalize(einsum("bs, bse -> be", F.softmax(einsum("bsd, dh -> bsh", h_3, m.w_5).reshape(-1, m.seq_max_len) +
                                                             -1.e9 * (1 - mask.float()), dim=1), x_hat), -1)
    e_u = F.softmax(einsum("be, bke -> bk", c_apt, phi_u) / m.temperature, dim=1)
    return einsum("bk, bke -> be", e_u, phi_u)


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    model = SINE(["hist"], ["item"], ["neg"], V, E, H, T, K, S, temperature=TEMP).to(dev)
    with torch.no_grad():
        for table in (model.item_embedding, model.concept_embedding, model.position_embedding):
            table.weight.normal_(0, 0.1)
    model.mode = "user"
    for B in (256, 4096):
        hist = torch.randint(1, V, (B, S), device=dev)
        lens = torch.randint(1, S + 1, (B,), device=dev)
        hist[torch.arange(S, device=dev)[None, :] < (S - lens)[:, None]] = 0
        g = torch.randn(B, E, device=dev)

        def fused():
            model.zero_grad(set_to_none=True)
            model({"hist": hist}).backward(g)

        def eager():
            model.zero_grad(set_to_none=True)
            eager_user_tower(model, hist).backward(g)

        tf, te = median_ms(fused), median_ms(eager)
        print(f"SINE user tower fwd+bwd B={B} S={S} E={E} H={H} T={T} K={K}: fused {tf:.3f} ms, eager reference chain "
              f"{te:.3f} ms ({te / tf:.2f}x)")
        X = 0.5 * torch.randn(B, S, E, device=dev)
        Y = 0.5 * torch.randn(B, S, E, device=dev)
        a1, a2, a3 = torch.randn(B, S, device=dev), torch.randn(B, S, K, device=dev), torch.randn(B, S, device=dev)
        mask = (hist > 0).to(torch.int32)
        C = model.concept_embedding.weight.detach()
        t_if = median_ms(lambda: ops.sine_interests(X, Y, a1, a2, mask, C))
        Xg, Yg = X.clone().requires_grad_(True), Y.clone().requires_grad_(True)
        gp, gx = torch.randn(B, K, E, device=dev), torch.randn(B, S, E, device=dev)

        def interests_both():
            phi, xhat, _ = ops.sine_interests(Xg, Yg, a1, a2, mask, C)
            torch.autograd.backward([phi, xhat], [gp, gx])

        t_ib = median_ms(interests_both)
        phi, xhat, _ = ops.sine_interests(X, Y, a1, a2, mask, C)
        t_af = median_ms(lambda: ops.sine_aggregate(xhat, a3, mask, phi, TEMP))
        xg = xhat.clone().requires_grad_(True)
        t_ab = median_ms(lambda: ops.sine_aggregate(xg, a3, mask, phi, TEMP).backward(g))
        print(f"  kernels alone: interest fwd {t_if * 1e3:.0f} us, fwd + bwd {t_ib * 1e3:.0f} us; aggregate fwd "
              f"{t_af * 1e3:.0f} us, fwd + bwd {t_ab * 1e3:.0f} us")


if __name__ == "__main__":
    main()
