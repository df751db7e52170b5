"""Generate the TIGER fixtures of tests/golden/ from the UNMODIFIED reference (CPU; needs ``transformers``).

Run where the reference checkout exists:  ``python tools/gen_golden_tiger.py``

  tiger_layers.npz   T5Attention._relative_position_bucket at relative positions -1100..1100 for (num_buckets,
                     max_distance) in {(32, 128), (8, 16), (4, 6)}, both directions; one attention module of each kind
                     (encoder self-attention, decoder self-attention, cross attention; d_model 16, d_kv 8, 2 heads, 8
                     buckets up to distance 16) taken out of a reference TIGERModel, with its weights, inputs, additive
                     mask, output and every gradient.  The key masks hold a full row, a right-padded row with ONE valid
                     key, a row with NO valid key and a left-padded row.
  model_tiger_a.npz  TIGERModel at vocab 40, d_model 16, d_kv 8, 2 heads, d_ff 24, 2 + 2 layers, 8 buckets / distance 16,
                     dropout 0, tied embeddings: the seeded state_dict, a batch of ragged right-padded inputs with a -100
                     label, logits, the loss at temperature 1.0 and 0.7, every parameter's gradient (temperature 0.7), the
                     losses of three torch.optim.AdamW steps (lr 1e-2) and ``generate`` with num_beams = 3 under a
                     six-candidate trie (sequences and sequences_scores).
  model_tiger_b.npz  the same with d_model 24, 3 heads, d_kv 5 (!= d_model / heads), 1 + 2 layers, and
                     ``tie_word_embeddings=False`` ASKED for: transformers >= 5 ties T5's embeddings whatever the config
                     says (T5Config.__post_init__ forces the field to True), so the recorded model is tied and rescaled,
                     and the recorded ``cfg`` holds what the reference's config holds after construction.  An untied head
                     cannot be recorded from the reference with this transformers; tests check it against the oracle.

The reference runs in float64 (``model.double()``) on float32-valued parameters and inputs, so the recorded outputs and
gradients are exact to ~1e-15 and a float64 restatement can be held to 1e-9.  Neighbouring recorded beam scores of a query differ by more than 1e-3 (asserted), so the compared order is not a matter
of rounding.  The archives are written with a fixed member timestamp: the files regenerate byte-identically.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_golden_ffm import _save_fixed  # noqa: E402
from oracle import gen_golden as G  # noqa: E402
from oracle.ref_import import import_reference  # noqa: E402

BUCKET_CFGS = ((32, 128), (8, 16), (4, 6))
MODEL_CFGS = {
    "a": dict(vocab_size=40, d_model=16, d_kv=8, num_heads=2, d_ff=24, num_layers=2, num_decoder_layers=2,
              relative_attention_num_buckets=8, relative_attention_max_distance=16, tie_word_embeddings=True),
    "b": dict(vocab_size=40, d_model=24, d_kv=5, num_heads=3, d_ff=24, num_layers=1, num_decoder_layers=2,
              relative_attention_num_buckets=8, relative_attention_max_distance=16, tie_word_embeddings=False),
}
SEEDS = {"a": G.SEED, "b": G.SEED + 1}
TEMPERATURE, LR, BEAMS = 0.7, 1e-2, 3
CANDIDATES = [[0, 5, 11, 21, 1], [0, 5, 12, 22, 1], [0, 6, 11, 23, 1], [0, 6, 13, 21, 1], [0, 7, 12, 24, 1], [0, 7, 13, 22, 1]]
FMIN = torch.finfo(torch.float64).min  # what the reference's mask builder adds at the model's dtype


def build(cfg_kw, seed):
    from transformers.models.t5.configuration_t5 import T5Config

    from torch_rechub.models.generative.tiger import TIGERModel
    torch.manual_seed(seed)
    cfg = T5Config(dropout_rate=0.0, feed_forward_proj="relu", layer_norm_epsilon=1e-6, pad_token_id=0, eos_token_id=1,
                   decoder_start_token_id=0, **cfg_kw)
    cfg._attn_implementation = "eager"
    model = TIGERModel(cfg)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():  # norm weights away from their all-one init, a livelier bias table
        for name, p in model.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
            if "relative_attention_bias" in name:
                p.copy_(0.5 * torch.randn(p.shape, generator=g))
    return model.double(), cfg  # float32 values, float64 arithmetic: the recording is the reference at double precision


def f32(t):
    """The float32 array of a tensor whose values are float32 numbers (inputs and parameters): exact."""
    a = G.npy(t)
    assert np.array_equal(a.astype(np.float32).astype(np.float64), a)
    return a.astype(np.float32)


def gen_layers():
    from transformers.models.t5.modeling_t5 import T5Attention
    out = {"bucket.cfgs": np.array(BUCKET_CFGS), "bucket.rel": np.arange(-1100, 1101, dtype=np.int32)}
    rel = torch.arange(-1100, 1101, dtype=torch.long)
    for nb, md in BUCKET_CFGS:
        for bi in (True, False):
            got = T5Attention._relative_position_bucket(rel, bidirectional=bi, num_buckets=nb, max_distance=md)
            out[f"bucket.{nb}_{md}_{int(bi)}"] = G.npy(got).astype(np.int32)
    model, cfg = build(MODEL_CFGS["a"], G.SEED + 7)
    model.train()
    g = torch.Generator().manual_seed(G.SEED + 8)
    D, Ls, Lt = cfg.d_model, 9, 5
    key_mask = torch.tensor([[1] * 9, [1] + [0] * 8, [0] * 9, [0, 0, 0, 1, 1, 1, 1, 1, 1]])
    zero, fmin = torch.zeros((), dtype=torch.float64), torch.full((), FMIN, dtype=torch.float64)
    add_mask = torch.where(key_mask.bool(), zero, fmin)[:, None, None, :]
    causal_add = torch.where(torch.tril(torch.ones(Lt, Lt, dtype=torch.bool)), zero, fmin)[None, None]
    kinds = {
        "enc": (model.encoder.block[0].layer[0].SelfAttention, (4, Ls), None, add_mask),
        "dec": (model.decoder.block[0].layer[0].SelfAttention, (2, Lt), None, causal_add),
        "cross": (model.decoder.block[0].layer[1].EncDecAttention, (4, 3), (4, Ls), add_mask),
    }
    out["attn.key_mask"] = G.npy(key_mask).astype(np.uint8)
    out["attn.cfg"] = np.array(json.dumps(dict(d_model=D, d_kv=cfg.d_kv, num_heads=cfg.num_heads, num_buckets=8, max_distance=16)))
    for kind, (mod, (B, L), kv_shape, mask) in kinds.items():
        x = torch.randn(B, L, D, generator=g).double().requires_grad_(True)
        kv = torch.randn(*kv_shape, D, generator=g).double().requires_grad_(True) if kv_shape else None
        res = mod(x, mask=mask, key_value_states=kv)
        y = res[0]
        gout = torch.randn(y.shape, generator=g).double()
        mod.zero_grad()
        (y * gout).sum().backward()
        out[f"attn.{kind}.x"] = f32(x)
        out[f"attn.{kind}.out"] = G.npy(y)
        out[f"attn.{kind}.weights"] = G.npy(res[2]) if res[2] is not None else np.zeros(0)
        out[f"attn.{kind}.gout"] = f32(gout)
        out[f"attn.{kind}.g_x"] = G.npy(x.grad)
        if kv is not None:
            out[f"attn.{kind}.kv"] = f32(kv)
            out[f"attn.{kind}.g_kv"] = G.npy(kv.grad)
        for name, p in mod.named_parameters():
            out[f"attn.{kind}.param.{name}"] = f32(p)
            out[f"attn.{kind}.grad.{name}"] = G.npy(p.grad)
    return out


def gen_model(tag):
    from torch_rechub.utils.data import Trie
    model, cfg = build(MODEL_CFGS[tag], SEEDS[tag])
    g = torch.Generator().manual_seed(SEEDS[tag] + 100)
    B, L = 4, 9
    lengths = [9, 4, 6, 1]
    ids = torch.randint(2, cfg.vocab_size, (B, L), generator=g)
    mask = torch.zeros(B, L, dtype=torch.long)
    for r, n in enumerate(lengths):
        mask[r, :n] = 1
        ids[r, n:] = 0
    labels = torch.tensor([c[1:] for c in (CANDIDATES[0], CANDIDATES[3], CANDIDATES[4], CANDIDATES[1])])
    labels[2, 3] = -100
    said = cfg.to_dict()  # what the reference's config holds after construction, not what was asked for
    names = ("vocab_size", "d_model", "d_kv", "d_ff", "num_layers", "num_decoder_layers", "num_heads",
             "relative_attention_num_buckets", "relative_attention_max_distance", "dropout_rate", "layer_norm_epsilon",
             "feed_forward_proj", "tie_word_embeddings", "pad_token_id", "eos_token_id", "decoder_start_token_id")
    out = {"cfg": np.array(json.dumps({k: said[k] for k in names})),
           "keys": np.array(json.dumps({k: list(v.shape) for k, v in model.state_dict().items()})),
           "input_ids": G.npy(ids), "attention_mask": G.npy(mask), "labels": G.npy(labels),
           "temperature": np.array(TEMPERATURE), "lr": np.array(LR)}
    for k, v in model.named_parameters():  # (the tied state_dict keys are "shared.weight" again: see "keys")
        out["param/" + k] = f32(v)
    model.train()
    res = model(input_ids=ids, attention_mask=mask, labels=labels)
    out["logits"] = G.npy(res.logits)
    out["loss_t1"] = G.npy(res.loss)
    model.set_hyper(TEMPERATURE)
    res = model(input_ids=ids, attention_mask=mask, labels=labels)
    out["loss_t"] = G.npy(res.loss)
    model.zero_grad()
    res.loss.backward()
    for name, p in model.named_parameters():
        out["grad/" + name] = G.npy(p.grad)
    model.zero_grad()
    # constrained beam search, before the optimizer moves the weights
    model.eval()
    trie = Trie(CANDIDATES)
    fn = trie.def_prefix_allowed_tokens_fn(trie)
    with torch.no_grad():
        gen = model.generate(input_ids=ids, attention_mask=mask, max_new_tokens=10, prefix_allowed_tokens_fn=fn,
                             num_beams=BEAMS, num_return_sequences=BEAMS, output_scores=True, return_dict_in_generate=True,
                             early_stopping=True, use_cache=False)
    seqs, scores = G.npy(gen["sequences"]), G.npy(gen["sequences_scores"])
    gaps = np.abs(np.diff(scores.reshape(B, BEAMS), axis=1))
    assert gaps.min() > 1e-3, f"model {tag}: neighbouring beam scores {scores} closer than 1e-3: pick another seed"
    out["beam.candidates"] = np.array(CANDIDATES)
    out["beam.sequences"] = seqs
    out["beam.scores"] = scores
    model.train()
    opt = torch.optim.AdamW(model.parameters(), lr=LR)
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = model(input_ids=ids, attention_mask=mask, labels=labels).loss
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    out["step_losses"] = np.array(losses)
    return out


def main():
    import_reference()
    _save_fixed(os.path.join(G.OUT, "tiger_layers.npz"), gen_layers())
    print("tiger_layers.npz")
    for tag in MODEL_CFGS:
        _save_fixed(os.path.join(G.OUT, f"model_tiger_{tag}.npz"), gen_model(tag))
        print(f"model_tiger_{tag}.npz")


if __name__ == "__main__":
    main()
