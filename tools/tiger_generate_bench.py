"""TIGERModel.generate with the constraint as a Python callback (Trie.get per beam row, a dense (B K, V) mask built on the
host, log_softmax and torch.topk over (B, K V), three host reads per step) against generate with the constraint as a
DeviceTrie (ops.beam_step, csrc/beam.hip: one launch per step, one host read per call).  Same weights, same inputs, one
process.

  model       the t5-small shape (d_model 512, d_kv 64, 8 heads, d_ff 2048, 6 + 6 layers, vocab 32128), random weights, eval
  candidates  10 000 distinct items of 4 code levels, 256 codes per level (tokens 2 + 256 l + c), each behind the start
              token and before EOS: 5 decoding steps
  search      20 beams, 20 returned, 80 input tokens, B = 1, 32, 256

After a warm-up of both sides the two take turns, ROUNDS times each: one HIP-event pair around a window of back-to-back
calls (generate ends with a host read, so a window is also wall time), the window sized from a calibration call to about
WINDOW_MS, at least one call.  Printed per side: the median window's time per call, the spread (fastest .. slowest window)
and the peak of torch.cuda.max_memory_allocated above what was allocated before the call (the model and the inputs).
The decoder has no KV cache on either side: every step recomputes the prefix.
``--trie-only B`` runs only the device path at batch B, a few calls: the run to trace for the kernel's own time
(rocprofv3 --kernel-trace --stats).  Run:  python tools/tiger_generate_bench.py [out.txt]"""
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, ".")
from torch_rechub_amd.models.generative import TIGERConfig, TIGERModel  # noqa: E402
from torch_rechub_amd.utils.data import DeviceTrie, Trie  # noqa: E402

ROUNDS, WARMUP, WINDOW_MS = 5, 2, 500.0
BEAMS, LEVELS, CODES, ITEMS, INPUT_TOKENS = 20, 4, 256, 10000, 80
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def window_ms(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / calls


def alternate(fns):
    """Per function (median, fastest, slowest) time per call in ms over ROUNDS windows, the functions taking turns."""
    calls = []
    for fn in fns:
        for _ in range(WARMUP):
            fn()
        torch.cuda.synchronize()
        calls.append(max(1, min(200, int(WINDOW_MS / max(window_ms(fn, 1), 1e-3)))))
    times = [[] for _ in fns]
    for r in range(ROUNDS):
        for t, fn, n in zip(times, fns, calls):
            t.append(window_ms(fn, n))
        print(f"  (round {r + 1} of {ROUNDS})", flush=True)
    return [(statistics.median(t), min(t), max(t)) for t in times], calls


def peak_above(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2**20


def setup():
    cfg = TIGERConfig(vocab_size=32128, d_model=512, d_kv=64, d_ff=2048, num_layers=6, num_decoder_layers=6, num_heads=8,
                      dropout_rate=0.1)
    torch.manual_seed(0)
    model = TIGERModel(cfg).cuda().eval()
    rng = np.random.default_rng(0)
    codes = np.unique(rng.integers(0, CODES, size=(ITEMS + ITEMS // 10, LEVELS)), axis=0)
    codes = codes[rng.permutation(len(codes))[:ITEMS]]
    items = [[cfg.decoder_start_token_id] + [int(2 + CODES * l + c) for l, c in enumerate(row)] + [cfg.eos_token_id]
             for row in codes]
    return cfg, model, items


def inputs(cfg, B):
    g = torch.Generator().manual_seed(B)
    lengths = torch.randint(20, INPUT_TOKENS + 1, (B, 1), generator=g)
    mask = (torch.arange(INPUT_TOKENS)[None, :] < lengths).long()
    ids = torch.randint(2, cfg.vocab_size, (B, INPUT_TOKENS), generator=g) * mask
    return ids.cuda(), mask.cuda()


def main():
    args = sys.argv[1:]
    cfg, model, items = setup()
    host_trie = Trie(items)
    callback = host_trie.def_prefix_allowed_tokens_fn(host_trie)
    trie = DeviceTrie(items, "cuda")
    kw = dict(max_new_tokens=LEVELS + 1, num_beams=BEAMS, num_return_sequences=BEAMS)
    if args and args[0] == "--trie-only":
        ids, mask = inputs(cfg, int(args[1]))
        for _ in range(5):
            model.generate(ids, mask, constraint=trie, **kw)
        torch.cuda.synchronize()
        return
    say(f"device: {torch.cuda.get_device_name(0)}; torch {torch.__version__}; ROUNDS {ROUNDS} WARMUP {WARMUP} window "
        f"{WINDOW_MS:.0f} ms; times are per generate call, median (fastest .. slowest window)")
    say(f"t5-small shape, vocab {cfg.vocab_size}, {len(items)} items of {LEVELS} levels x {CODES} codes + EOS "
        f"({trie.n_nodes} trie nodes, {trie.n_edges} edges, {LEVELS + 1} steps), {BEAMS} beams, {INPUT_TOKENS} input tokens")
    for B in (1, 32, 256):
        ids, mask = inputs(cfg, B)

        def with_callback():
            return model.generate(ids, mask, prefix_allowed_tokens_fn=callback, **kw)

        def with_trie():
            return model.generate(ids, mask, constraint=trie, **kw)

        a, b = with_callback(), with_trie()
        same = float((a["sequences"] == b["sequences"]).all(dim=1).float().mean())
        diff = float((a["sequences_scores"] - b["sequences_scores"]).abs().max())
        say(f"B {B}: {same * 100:.1f}% of the {B * BEAMS} returned sequences equal, max |score difference| {diff:.2e}")
        ((mc, lc, hc), (mt, lt, ht)), calls = alternate([with_callback, with_trie])
        pc, pt = peak_above(with_callback), peak_above(with_trie)
        say(f"B {B}: callback {mc:.1f} ms ({lc:.1f} .. {hc:.1f}; {calls[0]} calls per window), peak {pc:.0f} MiB; DeviceTrie "
            f"{mt:.1f} ms ({lt:.1f} .. {ht:.1f}; {calls[1]} calls per window), peak {pt:.0f} MiB; callback / DeviceTrie "
            f"{mc / mt:.2f}x")
    if args:
        with open(args[0], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
