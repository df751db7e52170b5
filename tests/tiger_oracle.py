"""float64 restatement of TIGER's T5 (reference models/generative/tiger.py over transformers' T5): the relative-position
buckets, the attention in its three forms, the RMS norm, the whole forward with its loss, and the constrained beam
search.  torch.double with autograd, so every backward is autograd's over the restated forward.  ``dtype`` lets the same
code run in float32 on the CPU: that is the error yardstick of the GPU tests' tolerance rule.

Excluded scores: the reference ADDS finfo(float32).min to a float32 score, which rounds to finfo.min itself, so a row with
no key left is uniform over all keys and its gradient still reaches the scores through the addition.  Here an excluded
score is set to that value with the identity as its derivative (``s + (fmin - s).detach()``), which is the same function
in any precision."""
import math

import numpy as np
import torch

FMIN = float(torch.finfo(torch.float32).min)


def buckets(rel, bidirectional, num_buckets, max_distance):
    """T5's bucket of relative position ``rel`` = key position - query position (int array)."""
    rel = np.asarray(rel, dtype=np.int64)
    out = np.zeros_like(rel)
    nb = num_buckets
    if nb == 1:  # (the reference's rule divides by zero; one bucket holds every distance)
        return out
    if bidirectional:
        nb //= 2
        out += (rel > 0).astype(np.int64) * nb
        rel = np.abs(rel)
    else:
        rel = -np.minimum(rel, 0)
    max_exact = nb // 2
    small = rel < max_exact
    with np.errstate(divide="ignore", invalid="ignore"):
        x = np.log(rel.astype(np.float32) / np.float32(max_exact)) / np.float32(math.log(max_distance / max_exact))
        x = x.astype(np.float32) * np.float32(nb - max_exact)
    big = np.where(np.isfinite(x), x, 0).astype(np.int64) + max_exact
    big = np.minimum(big, nb - 1)
    return out + np.where(small, rel, big)


def bucket_table(Lq, Lk, bidirectional, num_buckets, max_distance):
    """entry (j - i) + (Lq - 1)"""
    return buckets(np.arange(-(Lq - 1), Lk), bidirectional, num_buckets, max_distance)


def attention(q, k, v, H, key_mask=None, causal=False, table=None, bidirectional=True, max_distance=128, drop=None):
    """q (B, Lq, H dh), k, v (B, Lk, H dh) -> (B, Lq, H dh); no scale.  key_mask (B, Lk) bool-like; table (nb, H);
    drop (B, H, Lq, Lk) multiplier on the weights or None."""
    B, Lq, W = q.shape
    Lk = k.shape[1]
    dh = W // H
    qh = q.reshape(B, Lq, H, dh).permute(0, 2, 1, 3)
    kh = k.reshape(B, Lk, H, dh).permute(0, 2, 1, 3)
    vh = v.reshape(B, Lk, H, dh).permute(0, 2, 1, 3)
    s = qh @ kh.transpose(2, 3)
    if table is not None:
        i = np.arange(Lq)[:, None]
        j = np.arange(Lk)[None, :]
        bk = torch.as_tensor(buckets(j - i, bidirectional, table.shape[0], max_distance))
        s = s + table[bk].permute(2, 0, 1)[None]
    ok = torch.ones(B, 1, Lq, Lk, dtype=torch.bool)
    if key_mask is not None:
        ok = ok & (torch.as_tensor(key_mask) != 0)[:, None, None, :]
    if causal:
        ok = ok & torch.tril(torch.ones(Lq, Lk, dtype=torch.bool))[None, None]
    ok = ok.expand(B, H, Lq, Lk)
    s = torch.where(ok, s, s + (FMIN - s).detach())
    p = torch.softmax(s, dim=-1)
    if drop is not None:
        p = p * drop
    return (p @ vh).permute(0, 2, 1, 3).reshape(B, Lq, W)


def rms_norm(h, w, eps, vdt=None):
    """T5LayerNorm.  The reference takes the variance and its rsqrt in float32 whatever the model's dtype, and autograd
    differentiates through that cast; ``vdt`` = torch.float32 restates exactly that, which is what reproduces a float64
    recording of the reference to 1e-9.  None keeps the row's own dtype: the plain function the kernels are measured
    against."""
    x = h if vdt is None else h.to(vdt)
    return w * (h * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps))


def _attn_layer(P, pre, y, kv, H, key_mask, causal, table, bidirectional, maxd, drop=None):
    q = y @ P[pre + ".q.weight"].T
    k = kv @ P[pre + ".k.weight"].T
    v = kv @ P[pre + ".v.weight"].T
    w = None if drop is None else drop((y.shape[0], H, y.shape[1], kv.shape[1]))
    a = attention(q, k, v, H, key_mask, causal, table, bidirectional, maxd, w)
    return a @ P[pre + ".o.weight"].T


def _dropped(x, drop):
    return x if drop is None else x * drop(tuple(x.shape))


def stack(P, cfg, name, ids, key_mask=None, enc=None, enc_mask=None, vdt=None, drop=None, kink=None):
    """drop: None, or a callable that is called once per dropout site in the model's program order (T5Stack.forward: the
    token dropout; per block the self-attention weights, the attention delta, (decoder: the cross-attention weights and
    their delta,) relu(wi) and wo; the final dropout) with the site's logical shape -- (B, H, Lq, Lk) for attention
    weights, the tensor's own shape elsewhere -- and returns the multiplier.  kink: a list that receives, per ReLU, the
    smallest |pre-activation| over the units its dropout keeps."""
    dec = name == "decoder"
    n = cfg["num_decoder_layers"] if dec else cfg["num_layers"]
    H, eps, maxd = cfg["num_heads"], cfg["layer_norm_epsilon"], cfg["relative_attention_max_distance"]
    h = _dropped(P["shared.weight"][torch.as_tensor(ids)], drop)
    table = P[f"{name}.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]
    for b in range(n):
        pre = f"{name}.block.{b}.layer."
        y = rms_norm(h, P[pre + "0.layer_norm.weight"], eps, vdt)
        h = h + _dropped(_attn_layer(P, pre + "0.SelfAttention", y, y, H, key_mask, dec, table, not dec, maxd, drop), drop)
        f = 1
        if dec:
            y = rms_norm(h, P[pre + "1.layer_norm.weight"], eps, vdt)
            h = h + _dropped(_attn_layer(P, pre + "1.EncDecAttention", y, enc, H, enc_mask, False, None, True, maxd, drop), drop)
            f = 2
        y = rms_norm(h, P[pre + f"{f}.layer_norm.weight"], eps, vdt)
        pre_act = y @ P[pre + f"{f}.DenseReluDense.wi.weight"].T
        w = None if drop is None else drop(tuple(pre_act.shape))
        if kink is not None:
            live = pre_act.detach().abs() if w is None else pre_act.detach().abs()[torch.as_tensor(w) != 0]
            kink.append(float(live.min()) if live.numel() else float("inf"))
        mid = torch.relu(pre_act) if w is None else torch.relu(pre_act) * w
        h = h + _dropped(mid @ P[pre + f"{f}.DenseReluDense.wo.weight"].T, drop)
    return _dropped(rms_norm(h, P[f"{name}.final_layer_norm.weight"], eps, vdt), drop)


def shift_right(labels, cfg):
    labels = np.asarray(labels)
    out = np.zeros_like(labels)
    out[:, 1:] = labels[:, :-1]
    out[:, 0] = cfg["decoder_start_token_id"]
    out[out == -100] = cfg["pad_token_id"]
    return out


def decode(P, cfg, dec_ids, enc, mask, vdt=None, drop=None, kink=None):
    out = stack(P, cfg, "decoder", dec_ids, None, enc, mask, vdt, drop, kink)
    if cfg["tie_word_embeddings"]:
        out = out * cfg["d_model"]**-0.5
    return out @ P["lm_head.weight"].T


def forward(P, cfg, ids, mask, labels, temperature=1.0, vdt=None, drop=None, kink=None):
    """-> (logits (B, T, V), loss); drop, kink: see ``stack`` (the encoder's sites come first)."""
    enc = stack(P, cfg, "encoder", ids, mask, vdt=vdt, drop=drop, kink=kink)
    logits = decode(P, cfg, shift_right(labels, cfg), enc, mask, vdt, drop, kink)
    lab = torch.as_tensor(np.asarray(labels)).reshape(-1)
    loss = torch.nn.functional.cross_entropy((logits / temperature).reshape(-1, logits.shape[-1]), lab, ignore_index=-100)
    return logits, loss


def params(arrays, tied, dtype=torch.float64, requires_grad=False):
    """{state_dict key: tensor} from a fixture's arrays; both embed_tokens keys, and lm_head when ``tied``
    (tie_word_embeddings), are the ``shared.weight`` leaf."""
    P = {key: torch.tensor(np.asarray(a), dtype=dtype) for key, a in arrays.items()}
    for k in ("encoder.embed_tokens.weight", "decoder.embed_tokens.weight") + (("lm_head.weight",) if tied else ()):
        P[k] = P["shared.weight"]
    if requires_grad:
        for t in {id(t): t for t in P.values()}.values():
            t.requires_grad_(True)
    return P


def beam_search(P, cfg, ids, mask, allowed_fn, num_beams, max_new_tokens=10, vdt=None):
    """The reference's constrained beam search where all candidates have one length: -> (sequences (B K, 1 + n), scores
    (B K,)), per query by descending score; score = sum(log p) / n generated tokens.  As in the reference's ``generate``,
    the last position's logits are cast to float32 and the log-softmax, the -inf of the disallowed tokens, the running
    sums and the final division are float32, whatever the model's dtype."""
    with torch.no_grad():
        B, K, V = len(ids), num_beams, cfg["vocab_size"]
        enc = stack(P, cfg, "encoder", ids, mask, vdt=vdt).repeat_interleave(K, 0)
        m = None if mask is None else np.repeat(np.asarray(mask), K, 0)
        seqs = np.full((B * K, 1), cfg["decoder_start_token_id"], dtype=np.int64)
        running = torch.zeros(B, K, dtype=torch.float32)
        running[:, 1:] = -1e9
        for step in range(max_new_tokens):
            logp = torch.log_softmax(decode(P, cfg, seqs, enc, m, vdt)[:, -1, :].float(), -1)
            allow = torch.full((B * K, V), float("-inf"), dtype=torch.float32)
            for r in range(B * K):
                allow[r, allowed_fn(r // K, torch.as_tensor(seqs[r]))] = 0.0
            cand = (running.reshape(B * K, 1) + logp + allow).reshape(B, K * V)
            top, idx = torch.topk(cand, K, dim=1)
            beam, tok = (idx // V).numpy(), (idx % V).numpy()
            rows = (np.arange(B)[:, None] * K + beam).reshape(-1)
            seqs = np.concatenate([seqs[rows], tok.reshape(-1, 1)], 1)
            running = top
            if (tok == cfg["eos_token_id"]).all():
                return seqs, (running / (step + 1)).reshape(-1).numpy()
    raise AssertionError("no beam ended")
