"""One SASRec train step at the paper's shape (B 128, L 200, D 50, 2 blocks, 1 head, dropout 0.5; V 3417): our model
(models/matching/sasrec.py on csrc/sasrec.hip and csrc/hllm.hip) against the same model composed from library ops
(F.embedding, F.layer_norm, nn.MultiheadAttention, F.linear, F.dropout) on the same device, with equal initial weights.
A step = zero_grad, forward, the BPR probe loss over the (B, L) logit pairs, backward, torch.optim.Adam.step.  One process;
after a warm-up of both sides the two are timed in turn, ROUNDS times each: one HIP-event pair around a window of STEPS
back-to-back steps (a few hundred ms), so clock and temperature drift meets both alike.  Printed per side: the median
window's time per step and the spread (fastest .. slowest window); forward + backward alone as well."""
import copy
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from torch_rechub_amd.basic.features import SequenceFeature  # noqa: E402
from torch_rechub_amd.models.matching import SASRec  # noqa: E402

B, L, D, BLOCKS, HEADS, P, V = 128, 200, 50, 2, 1, 0.5, 3417


ROUNDS, STEPS, WARMUP = 9, 60, 20


def window_ms(fn):
    """Time per step of one window of STEPS steps."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(STEPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / STEPS


def alternate(fns):
    """Per function the sorted per-step times of its ROUNDS windows, the functions taking turns."""
    for fn in fns:
        for _ in range(WARMUP):
            fn()
    torch.cuda.synchronize()
    times = [[] for _ in fns]
    for _ in range(ROUNDS):
        for t, fn in zip(times, fns):
            t.append(window_ms(fn))
    return [sorted(t) for t in times]


def library_forward(m, x):
    """The reference's pairwise forward as it composes it from library ops, batch-first."""
    table = m.item_emb.embed_dict["seq"].weight[:, :D]
    seq = x["seq"]
    emb = F.embedding(torch.stack([x["seq"], x["pos"], x["neg"]], 1), table)  # (B, 3, L, D)
    keep = (seq != 0).unsqueeze(-1)
    h = F.dropout(emb[:, 0] * D**0.5 + m.position_emb.weight[:seq.shape[1]], m.emb_dropout.p, m.training) * keep
    causal = ~torch.tril(torch.ones((seq.shape[1], seq.shape[1]), dtype=torch.bool, device=seq.device))
    for ln_a, mha, ln_f, ffn in zip(m.attention_layernorms, m.attention_layers, m.forward_layernorms, m.forward_layers):
        ht = h.transpose(0, 1)
        q = ln_a(ht)
        h = (q + mha(q, ht, ht, attn_mask=causal)[0]).transpose(0, 1)
        z = ln_f(h)
        a = F.relu(F.dropout(F.linear(z, ffn.conv1.weight.squeeze(-1), ffn.conv1.bias), ffn.dropout1.p, m.training))
        h = (z + F.dropout(F.linear(a, ffn.conv2.weight.squeeze(-1), ffn.conv2.bias), ffn.dropout2.p, m.training)) * keep
    s = m.last_layernorm(h)
    return (s * emb[:, 1]).sum(-1), (s * emb[:, 2]).sum(-1)


def main():
    dev = torch.device("cuda:0")
    torch.manual_seed(0)
    feas = [SequenceFeature("seq", vocab_size=V, embed_dim=D, pooling="concat"),
            SequenceFeature("pos", vocab_size=V, embed_dim=D, pooling="concat", shared_with="seq"),
            SequenceFeature("neg", vocab_size=V, embed_dim=D, pooling="concat", shared_with="seq")]
    ours = SASRec(feas, max_len=L, dropout_rate=P, num_blocks=BLOCKS, num_heads=HEADS)
    with torch.no_grad():
        ours.item_emb.embed_dict["seq"].weight[:, :D].normal_(0, 0.1)
    lib = copy.deepcopy(ours)
    ours, lib = ours.to(dev).train(), lib.to(dev).train()
    lens = torch.randint(1, L + 1, (B,), device=dev)
    keep = torch.arange(L, device=dev)[None, :] >= (L - lens)[:, None]  # padded at the front, as the paper's loader pads
    x = {k: torch.randint(1, V, (B, L), device=dev) * keep for k in ("seq", "pos", "neg")}

    def make(model, forward, with_step):
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)

        def step():
            opt.zero_grad(set_to_none=True)
            pos, neg = forward(x)
            (-(pos - neg).sigmoid().log().mean()).backward()
            if with_step:
                opt.step()
        return step

    for what, with_step in (("train step", True), ("forward + backward", False)):
        t_ours, t_lib = alternate([make(ours, ours, with_step), make(lib, lambda xb: library_forward(lib, xb), with_step)])
        m_ours, m_lib = statistics.median(t_ours), statistics.median(t_lib)
        print(f"SASRec {what} B={B} L={L} D={D} blocks={BLOCKS} heads={HEADS} p={P}, {ROUNDS} alternating windows of {STEPS} "
              f"steps: ours {m_ours:.3f} ms ({t_ours[0]:.3f} .. {t_ours[-1]:.3f}), library ops {m_lib:.3f} ms "
              f"({t_lib[0]:.3f} .. {t_lib[-1]:.3f}), library / ours {m_lib / m_ours:.2f}x")


if __name__ == "__main__":
    main()
