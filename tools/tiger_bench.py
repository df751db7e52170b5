"""TIGER's attention kernels (csrc/t5attn.hip) and one whole train step against the same computation on torch ops, same
device, same process, same inputs.

  attention   ops.t5_attention, forward + backward from given q, k, v (fp32), against matmul, the gathered bias, the
              additive mask, softmax and matmul, at B = 256, dh = 64, H in {6, 8}:
                encoder  Lq = Lk = 80, key-padding mask, bidirectional bias table (32 buckets)
                decoder  Lq = Lk = 4, causal, one-sided bias table
                cross    Lq = 4, Lk = 80, key-padding mask, no bias
  train step  TIGERModel at the t5-small shape (d_model 512, d_kv 64, 8 heads, d_ff 2048, 6 + 6 layers, vocab 32128,
              dropout 0.1), B = 256, 80 input tokens, 4 target tokens: forward, loss, backward, AdamW step; the fused path
              against the same model with ops.t5_attention and ops.add_rms_norm replaced by torch ops.

After a warm-up of both sides the two take turns, ROUNDS times each: one HIP-event pair around a window of back-to-back
steps, the window sized (from a calibration run) to about WINDOW_MS.  Printed per side: the median window's time per step
and the spread (fastest .. slowest window).  These are wall times of enqueued work: where a step is a handful of tiny
launches (the decoder shapes) they measure the host's launch cost, and the line says so.  Not measured: kernel times from a
trace, other batch sizes, bf16.  Run:  python tools/tiger_bench.py [out.txt]"""
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, ".")
from torch_rechub_amd import ops  # noqa: E402
from torch_rechub_amd.models.generative import TIGERConfig, TIGERModel  # noqa: E402

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
        steps.append(max(3, min(2000, int(WINDOW_MS / max(window_ms(fn, 3), 1e-3)))))
    times = [[] for _ in fns]
    for _ in range(ROUNDS):
        for t, fn, n in zip(times, fns, steps):
            t.append(window_ms(fn, n))
    return [(statistics.median(t), min(t), max(t)) for t in times]


def report(what, fused, torch_side, note=""):
    (mf, lf, hf), (mt, lt, ht) = alternate([fused, torch_side])
    say(f"{what}: fused {mf * 1e3:.1f} us ({lf * 1e3:.1f} .. {hf * 1e3:.1f}), torch ops {mt * 1e3:.1f} us "
        f"({lt * 1e3:.1f} .. {ht * 1e3:.1f}), torch / fused {mt / mf:.2f}x{note}")


def torch_attention(q, k, v, n_heads, key_mask=None, causal=False, bias_table=None, bidirectional=True, max_distance=128,
                    dropout_p=0.0, training=True):
    """ops.t5_attention's contract on torch ops, the way the reference's eager attention computes it."""
    B, Lq, W = q.shape
    Lk = k.shape[1]
    dh = W // n_heads
    qh, kh, vh = (t.reshape(B, -1, n_heads, dh).transpose(1, 2) for t in (q, k, v))
    s = torch.matmul(qh, kh.transpose(2, 3))
    if bias_table is not None:
        bucket = ops.t5_relative_buckets(Lq, Lk, bidirectional, bias_table.shape[0], max_distance, device=q.device)
        idx = (torch.arange(Lk, device=q.device)[None, :] - torch.arange(Lq, device=q.device)[:, None]) + (Lq - 1)
        s = s + bias_table[bucket.long()[idx]].permute(2, 0, 1)[None]
    fmin = torch.finfo(s.dtype).min
    if key_mask is not None:
        s = s + torch.where(key_mask != 0, 0.0, fmin)[:, None, None, :]
    if causal:
        s = s + torch.where(torch.tril(torch.ones(Lq, Lk, dtype=torch.bool, device=q.device)), 0.0, fmin)[None, None]
    p = F.dropout(torch.softmax(s, -1), dropout_p, training)
    return torch.matmul(p, vh).transpose(1, 2).reshape(B, Lq, W)


def torch_add_rms_norm(h, delta, weight, eps=1e-6):
    hn = h if delta is None else h + delta
    return hn, weight * (hn * torch.rsqrt(hn.pow(2).mean(-1, keepdim=True) + eps))


def attention_step(fn, q, k, v, gout, **kw):
    def step():
        for t in (q, k, v, kw.get("bias_table")):
            if t is not None:
                t.grad = None
        fn(q, k, v, **kw).backward(gout)
    return step


def bench_attention():
    B, dh, Ls, Lt = 256, 64, 80, 4
    g = torch.Generator(device="cuda").manual_seed(0)
    for H in (6, 8):
        W = H * dh
        mask = (torch.arange(Ls, device="cuda")[None, :] < torch.randint(20, Ls + 1, (B, 1), device="cuda", generator=g)).long()
        forms = {"encoder 80 x 80, mask, bias": (Ls, Ls, dict(key_mask=mask, bidirectional=True), True),
                 "decoder 4 x 4, causal, bias": (Lt, Lt, dict(causal=True, bidirectional=False), True),
                 "cross 4 x 80, mask": (Lt, Ls, dict(key_mask=mask), False)}
        for name, (Lq, Lk, kw, with_bias) in forms.items():
            q = (torch.randn(B, Lq, W, device="cuda", generator=g) / 8).requires_grad_(True)
            k, v = (torch.randn(B, Lk, W, device="cuda", generator=g).requires_grad_(True) for _ in range(2))
            gout = torch.randn(B, Lq, W, device="cuda", generator=g)
            if with_bias:
                kw = dict(kw, bias_table=torch.randn(32, H, device="cuda", generator=g).requires_grad_(True))
            a = ops.t5_attention(q, k, v, H, **kw)
            b = torch_attention(q, k, v, H, **kw)
            say(f"  (max |fused - torch| of the output {float((a - b).abs().max()):.2e})")
            note = "  [both sides a few tiny launches: host launch cost]" if Lq * Lk <= 1024 else ""
            report(f"attention fwd+bwd B {B} H {H} dh {dh} {name}", attention_step(ops.t5_attention, q, k, v, gout, n_heads=H, **kw),
                   attention_step(torch_attention, q, k, v, gout, n_heads=H, **kw), note)


def bench_train_step():
    cfg = TIGERConfig(vocab_size=32128, d_model=512, d_kv=64, d_ff=2048, num_layers=6, num_decoder_layers=6, num_heads=8,
                      dropout_rate=0.1)
    B, Ls, Lt = 256, 80, 4
    g = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    model = TIGERModel(cfg).cuda().train()
    opt = torch.optim.AdamW(model.parameters(), lr=1e-4)
    ids = torch.randint(2, cfg.vocab_size, (B, Ls), generator=g).cuda()
    lengths = torch.randint(20, Ls + 1, (B, 1), generator=g).cuda()
    mask = (torch.arange(Ls, device="cuda")[None, :] < lengths).long()
    ids = ids * mask
    labels = torch.randint(2, cfg.vocab_size, (B, Lt), generator=g).cuda()
    labels[:, -1] = 1
    fused_ops = (ops.t5_attention, ops.add_rms_norm)

    def step_with(attn, norm):
        def step():
            ops.t5_attention, ops.add_rms_norm = attn, norm
            try:
                opt.zero_grad(set_to_none=True)
                loss = model(ids, attention_mask=mask, labels=labels).loss
                loss.backward()
                opt.step()
            finally:
                ops.t5_attention, ops.add_rms_norm = fused_ops
            return loss
        return step

    fused, plain = step_with(*fused_ops), step_with(torch_attention, torch_add_rms_norm)
    model.eval()  # the two paths on the same weights, no dropout
    with torch.no_grad():
        a = float(model(ids, attention_mask=mask, labels=labels).loss)
        ops.t5_attention, ops.add_rms_norm = torch_attention, torch_add_rms_norm
        try:
            b = float(model(ids, attention_mask=mask, labels=labels).loss)
        finally:
            ops.t5_attention, ops.add_rms_norm = fused_ops
    model.train()
    say(f"  (eval loss on the same weights: fused {a:.6f}, torch ops {b:.6f})")
    report(f"train step t5-small shape B {B} inputs {Ls} targets {Lt} dropout 0.1 (fwd, loss, bwd, AdamW)", fused, plain)


def main():
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; ROUNDS {ROUNDS} WARMUP {WARMUP} "
        f"window {WINDOW_MS:.0f} ms; times are per step, median (fastest .. slowest window)")
    bench_attention()
    bench_train_step()
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
