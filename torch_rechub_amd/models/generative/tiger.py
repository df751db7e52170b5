"""TIGER (generative retrieval over semantic IDs): a stand-alone T5 encoder-decoder on the fused attention kernels.

Reference ``torch_rechub/models/generative/tiger.py`` subclasses ``transformers.T5ForConditionalGeneration`` and adds a
temperature on the logits before the cross entropy.  This is the same network written out, with the reference's
``state_dict`` keys, so a reference checkpoint loads with ``strict=True`` and ``transformers`` is not needed:

* pre-norm blocks with T5's RMS norm, no biases anywhere, a ReLU feed-forward;
* attention without the 1/sqrt(d) scale; one log-bucketed relative-position table per stack, owned by block 0;
* tied embeddings (``shared``, both ``embed_tokens`` and ``lm_head`` are one parameter) with the ``d_model ** -0.5`` rescale
  before the head.

Each sub-layer is ``ops.add_rms_norm`` (the residual add of the sub-layer before it and the norm, one pass), one fused
QKV (or, for cross attention, KV) product, ``ops.t5_attention`` reading its column blocks in place, and the output
product.  The products, the head and the loss are library GEMMs and torch ops.
"""
from dataclasses import dataclass, fields

import torch
import torch.nn.functional as F
from torch import nn

from ... import ops


@dataclass
class TIGERConfig:
    """The T5Config fields the model reads."""
    vocab_size: int = 32128
    d_model: int = 512
    d_kv: int = 64
    d_ff: int = 2048
    num_layers: int = 6
    num_decoder_layers: int = None
    num_heads: int = 8
    relative_attention_num_buckets: int = 32
    relative_attention_max_distance: int = 128
    dropout_rate: float = 0.1
    layer_norm_epsilon: float = 1e-6
    feed_forward_proj: str = "relu"
    tie_word_embeddings: bool = True
    pad_token_id: int = 0
    eos_token_id: int = 1
    decoder_start_token_id: int = 0

    def __post_init__(self):
        if self.num_decoder_layers is None:
            self.num_decoder_layers = self.num_layers
        if self.feed_forward_proj != "relu":
            raise ValueError(f"TIGERConfig: feed_forward_proj={self.feed_forward_proj!r} is not supported (only 'relu'; "
                             "the gated-GELU T5 variants have no implementation here)")

    @classmethod
    def from_dict(cls, d):
        """From a T5 ``config.json`` dict (or ``T5Config.to_dict()``): unknown keys are ignored."""
        names = {f.name for f in fields(cls)}
        kw = {k: v for k, v in dict(d).items() if k in names and v is not None}
        return cls(**kw)

    def to_dict(self):
        return {f.name: getattr(self, f.name) for f in fields(self)}


class ModelOutput(dict):
    """{"loss", "logits"} with attribute access."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None


class T5LayerNorm(nn.Module):
    """Holds the RMS norm's weight; the norm itself runs inside ``ops.add_rms_norm``."""

    def __init__(self, d, eps):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(d))
        self.variance_epsilon = eps


class T5Attention(nn.Module):

    def __init__(self, cfg, has_relative_attention_bias):
        super().__init__()
        inner = cfg.num_heads * cfg.d_kv
        self.n_heads = cfg.num_heads
        self.q = nn.Linear(cfg.d_model, inner, bias=False)
        self.k = nn.Linear(cfg.d_model, inner, bias=False)
        self.v = nn.Linear(cfg.d_model, inner, bias=False)
        self.o = nn.Linear(inner, cfg.d_model, bias=False)
        if has_relative_attention_bias:
            self.relative_attention_bias = nn.Embedding(cfg.relative_attention_num_buckets, cfg.num_heads)
        d = cfg.d_model
        nn.init.normal_(self.q.weight, std=(d * cfg.d_kv)**-0.5)
        nn.init.normal_(self.k.weight, std=d**-0.5)
        nn.init.normal_(self.v.weight, std=d**-0.5)
        nn.init.normal_(self.o.weight, std=inner**-0.5)
        if has_relative_attention_bias:
            nn.init.normal_(self.relative_attention_bias.weight, std=d**-0.5)


class T5DenseActDense(nn.Module):

    def __init__(self, cfg):
        super().__init__()
        self.wi = nn.Linear(cfg.d_model, cfg.d_ff, bias=False)
        self.wo = nn.Linear(cfg.d_ff, cfg.d_model, bias=False)
        nn.init.normal_(self.wi.weight, std=cfg.d_model**-0.5)
        nn.init.normal_(self.wo.weight, std=cfg.d_ff**-0.5)


class _SubLayer(nn.Module):

    def __init__(self, cfg, name, inner):
        super().__init__()
        setattr(self, name, inner)
        self.layer_norm = T5LayerNorm(cfg.d_model, cfg.layer_norm_epsilon)


class T5Block(nn.Module):
    """``layer`` = [self attention, (cross attention,) feed-forward], named as the reference names them."""

    def __init__(self, cfg, is_decoder, has_relative_attention_bias):
        super().__init__()
        layers = [_SubLayer(cfg, "SelfAttention", T5Attention(cfg, has_relative_attention_bias))]
        if is_decoder:
            layers.append(_SubLayer(cfg, "EncDecAttention", T5Attention(cfg, False)))
        layers.append(_SubLayer(cfg, "DenseReluDense", T5DenseActDense(cfg)))
        self.layer = nn.ModuleList(layers)


class T5Stack(nn.Module):

    def __init__(self, cfg, embed_tokens, is_decoder):
        super().__init__()
        self.cfg = cfg
        self.is_decoder = is_decoder
        self.embed_tokens = embed_tokens
        n = cfg.num_decoder_layers if is_decoder else cfg.num_layers
        self.block = nn.ModuleList([T5Block(cfg, is_decoder, i == 0) for i in range(n)])
        self.final_layer_norm = T5LayerNorm(cfg.d_model, cfg.layer_norm_epsilon)

    def _attend(self, att, y, kv_src, key_mask, causal, table):
        cfg = self.cfg
        W = cfg.num_heads * cfg.d_kv
        if kv_src is None:  # self attention: one product for q, k and v
            qkv = F.linear(y, torch.cat((att.q.weight, att.k.weight, att.v.weight), 0))
            q, k, v = qkv[..., :W], qkv[..., W:2 * W], qkv[..., 2 * W:]
        else:  # cross attention: q from the decoder, one product for k and v of the encoded history
            q = F.linear(y, att.q.weight)
            kv = F.linear(kv_src, torch.cat((att.k.weight, att.v.weight), 0))
            k, v = kv[..., :W], kv[..., W:]
        a = ops.t5_attention(q, k, v, cfg.num_heads, key_mask=key_mask, causal=causal, bias_table=table,
                             bidirectional=not self.is_decoder, max_distance=cfg.relative_attention_max_distance,
                             dropout_p=cfg.dropout_rate, training=self.training)
        return F.linear(a, att.o.weight)

    def forward(self, input_ids, key_mask=None, encoder_hidden=None, encoder_mask=None):
        cfg = self.cfg
        p, tr = cfg.dropout_rate, self.training
        eps = cfg.layer_norm_epsilon
        h = ops.dropout(self.embed_tokens(input_ids), p, tr)
        delta = None
        table = self.block[0].layer[0].SelfAttention.relative_attention_bias.weight if len(self.block) else None
        for blk in self.block:
            sa = blk.layer[0]
            h, y = ops.add_rms_norm(h, delta, sa.layer_norm.weight, eps)
            delta = ops.dropout(self._attend(sa.SelfAttention, y, None, key_mask, self.is_decoder, table), p, tr)
            if self.is_decoder:
                ca = blk.layer[1]
                h, y = ops.add_rms_norm(h, delta, ca.layer_norm.weight, eps)
                delta = ops.dropout(self._attend(ca.EncDecAttention, y, encoder_hidden, encoder_mask, False, None), p, tr)
            ff = blk.layer[-1]
            h, y = ops.add_rms_norm(h, delta, ff.layer_norm.weight, eps)
            mid = ops.dropout(torch.relu(F.linear(y, ff.DenseReluDense.wi.weight)), p, tr)
            delta = ops.dropout(F.linear(mid, ff.DenseReluDense.wo.weight), p, tr)
        _, y = ops.add_rms_norm(h, delta, self.final_layer_norm.weight, eps)
        return ops.dropout(y, p, tr)


class TIGERModel(nn.Module):
    """T5 for conditional generation with TIGER's temperature on the training logits.

    ``forward(input_ids, attention_mask=None, labels=None, decoder_input_ids=None)`` returns ``{"loss", "logits"}`` (also as
    attributes); ``generate`` is the constrained beam search of the reference's examples.  HIP device only."""

    def __init__(self, config):
        super().__init__()
        if isinstance(config, dict):
            config = TIGERConfig.from_dict(config)
        self.config = config
        self.model_dim = config.d_model
        self.shared = nn.Embedding(config.vocab_size, config.d_model)
        nn.init.normal_(self.shared.weight, std=1.0)
        self.encoder = T5Stack(config, self.shared, False)
        self.decoder = T5Stack(config, self.shared, True)
        self.lm_head = nn.Linear(config.d_model, config.vocab_size, bias=False)
        if config.tie_word_embeddings:
            self.lm_head.weight = self.shared.weight
        else:
            nn.init.normal_(self.lm_head.weight, std=1.0)
        self.temperature = 1.0

    def set_hyper(self, temperature):
        self.temperature = temperature

    @classmethod
    def from_t5(cls, ref_model):
        """A TIGERModel with the config, the weights and the temperature of the reference's TIGERModel.  A plain
        ``transformers`` T5ForConditionalGeneration is accepted where it computes the same function -- it rescales the
        decoder output exactly when its embeddings are tied -- and refused otherwise."""
        cfg = ref_model.config
        if getattr(cfg, "scale_decoder_outputs", None) is False and cfg.tie_word_embeddings and not hasattr(ref_model, "ranking_loss"):
            raise ValueError("TIGERModel.from_t5: this T5 ties its embeddings but does not rescale the decoder output "
                             "(scale_decoder_outputs=False, a T5 v1.1-style config); the reference TIGERModel, which this "
                             "class mirrors, rescales whenever tie_word_embeddings is set, so the copy would differ")
        model = cls(TIGERConfig.from_dict(cfg.to_dict() if hasattr(cfg, "to_dict") else dict(cfg)))
        model.load_state_dict({k: v.detach().clone() for k, v in ref_model.state_dict().items()}, strict=True)
        model.temperature = getattr(ref_model, "temperature", 1.0)
        return model

    def _shift_right(self, labels):
        cfg = self.config
        shifted = labels.new_zeros(labels.shape)
        shifted[..., 1:] = labels[..., :-1]
        shifted[..., 0] = cfg.decoder_start_token_id
        return shifted.masked_fill(shifted == -100, cfg.pad_token_id)

    def encode(self, input_ids, attention_mask=None):
        return self.encoder(input_ids, key_mask=attention_mask)

    def decode(self, decoder_input_ids, encoder_hidden, attention_mask=None):
        out = self.decoder(decoder_input_ids, encoder_hidden=encoder_hidden, encoder_mask=attention_mask)
        if self.config.tie_word_embeddings:
            out = out * (self.model_dim**-0.5)
        return self.lm_head(out)

    def ranking_loss(self, lm_logits, labels):
        if labels is None:
            return None
        t_logits = lm_logits / self.temperature
        return F.cross_entropy(t_logits.view(-1, t_logits.size(-1)), labels.reshape(-1), ignore_index=-100)

    def forward(self, input_ids, attention_mask=None, labels=None, decoder_input_ids=None):
        hidden = self.encode(input_ids, attention_mask)
        if decoder_input_ids is None:
            if labels is None:
                raise ValueError("TIGERModel.forward: labels or decoder_input_ids expected")
            decoder_input_ids = self._shift_right(labels)
        logits = self.decode(decoder_input_ids, hidden, attention_mask)
        return ModelOutput(loss=self.ranking_loss(logits, labels), logits=logits)

    @torch.no_grad()
    def generate(self, input_ids, attention_mask=None, max_new_tokens=10, num_beams=1, num_return_sequences=1,
                 prefix_allowed_tokens_fn=None, constraint=None):
        """Constrained beam search as the reference's examples run it (``early_stopping=True``, length penalty 1): the
        encoder runs once, the decoder is recomputed on the growing prefix; tokens outside
        ``prefix_allowed_tokens_fn(batch_id, prefix)`` get -inf on their log-probabilities (which are not renormalised);
        a hypothesis ends with EOS and scores sum(log p) / number of generated tokens.  Returns ``{"sequences": (B *
        num_return_sequences, 1 + n) int64, "sequences_scores": (B * num_return_sequences,)}``, per query by descending score.

        Supported: every candidate of the constraint has the same length (the semantic-ID case: all beams end at the same
        step) and there are at least ``num_beams`` candidates; anything else raises.

        ``constraint``: the candidates as a ``utils.data.DeviceTrie`` (each starting with ``decoder_start_token_id`` and
        ending with EOS) instead of the callback.  The search then stays on the device -- one ``ops.beam_step`` per step
        over the children of the beams' trie nodes, no callback, no (B K, V) mask, one host read after the last step -- and
        the result also holds ``"item_index"``: (B, num_return_sequences) int64, the candidates' indices in the trie's
        order, which ``basic.metric.topk_metrics`` takes as it is."""
        cfg = self.config
        K = int(num_beams)
        R = int(num_return_sequences)
        if not 1 <= R <= K:
            raise ValueError(f"generate: num_return_sequences={R} must be in [1, num_beams={K}]")
        if constraint is not None:
            if prefix_allowed_tokens_fn is not None:
                raise ValueError("generate: constraint and prefix_allowed_tokens_fn are two forms of one thing: give one")
            return self._generate_on_trie(input_ids, attention_mask, int(max_new_tokens), K, R, constraint)
        B = int(input_ids.shape[0])
        dev = input_ids.device
        V = cfg.vocab_size
        was_training = self.training
        self.eval()
        try:
            hidden = self.encode(input_ids, attention_mask)
            hidden = hidden.repeat_interleave(K, 0)
            mask = None if attention_mask is None else attention_mask.repeat_interleave(K, 0)
            seqs = torch.full((B * K, 1), cfg.decoder_start_token_id, dtype=torch.int64, device=dev)
            # as the reference's search starts: only the first of a query's (identical) beams counts at step one
            running = torch.zeros((B, K), dtype=torch.float32, device=dev)
            running[:, 1:] = -1e9
            done = None
            for step in range(int(max_new_tokens)):
                logits = self.decode(seqs, hidden, mask)[:, -1, :]
                logp = torch.log_softmax(logits.float(), dim=-1)
                if prefix_allowed_tokens_fn is not None:
                    allow = torch.full((B * K, V), float("-inf"), dtype=torch.float32)
                    host = seqs.cpu()
                    n_allowed = []
                    for r in range(B * K):
                        toks = list(prefix_allowed_tokens_fn(r // K, host[r]))
                        n_allowed.append(len(toks))
                        allow[r, toks] = 0.0
                    if any(n == 0 for n in n_allowed):
                        raise ValueError("generate: a live beam has no allowed continuation and has not ended with EOS: the "
                                         "candidates of the constraint differ in length, which is not supported")
                    logp = logp + allow.to(dev)
                cand = (running.view(B * K, 1) + logp).view(B, K * V)
                top, idx = torch.topk(cand, K, dim=1)
                if bool(torch.isinf(top).any()):
                    raise ValueError(f"generate: fewer than num_beams={K} continuations are allowed: the constraint has "
                                     "fewer candidates than beams, which is not supported")
                beam = idx // V
                tok = idx % V
                rows = (torch.arange(B, device=dev).view(B, 1) * K + beam).view(-1)
                seqs = torch.cat((seqs[rows], tok.view(-1, 1)), 1)
                running = top
                ended = tok == cfg.eos_token_id
                if bool(ended.all()):
                    done = step + 1
                    break
                if bool(ended.any()):
                    raise ValueError("generate: some beams ended with EOS and others did not at the same step: the "
                                     "candidates of the constraint differ in length, which is not supported")
            if done is None:
                raise ValueError(f"generate: no candidate ended within max_new_tokens={int(max_new_tokens)}")
            if bool((running < -1e8).any()):
                raise ValueError(f"generate: the constraint has fewer than num_beams={K} candidates, which is not supported")
            scores = running / float(done)
            seqs = seqs.view(B, K, -1)[:, :R].reshape(B * R, -1)
            return {"sequences": seqs, "sequences_scores": scores[:, :R].reshape(-1)}
        finally:
            self.train(was_training)

    def _generate_on_trie(self, input_ids, attention_mask, max_new_tokens, K, R, trie):
        """``generate`` with the candidates as a DeviceTrie: decode, ``ops.beam_step``, reorder -- all on the device.

        Nothing is read back inside the loop, so a query that runs short of candidates is noticed only after the last
        step: until then its unused slots (parent -1, token -1) stay dead in the kernel, and the decoder is fed row 0 of
        the query and token 0 for them on every remaining step.  That work is wasted, never returned: the one host read
        behind the loop raises for such a query."""
        cfg = self.config
        steps = trie.depth - 1  # a candidate is the start token, the codes and EOS
        if trie.find([cfg.decoder_start_token_id]) < 0 or steps < 1:
            raise ValueError(f"generate: the constraint's candidates do not start with decoder_start_token_id="
                             f"{cfg.decoder_start_token_id} followed by at least one token")
        if steps > max_new_tokens:
            raise ValueError(f"generate: no candidate ended within max_new_tokens={max_new_tokens}: the constraint's "
                             f"candidates take {steps} steps")
        if trie.last_tokens_equal != cfg.eos_token_id:
            raise ValueError(f"generate: the constraint's candidates do not all end with eos_token_id={cfg.eos_token_id}")
        if trie.max_token >= cfg.vocab_size:
            raise ValueError(f"generate: the constraint holds token {trie.max_token}, outside vocab_size={cfg.vocab_size}")
        B = int(input_ids.shape[0])
        dev = input_ids.device
        was_training = self.training
        self.eval()
        try:
            hidden = self.encode(input_ids, attention_mask).repeat_interleave(K, 0)
            mask = None if attention_mask is None else attention_mask.repeat_interleave(K, 0)
            seqs = torch.full((B * K, 1), cfg.decoder_start_token_id, dtype=torch.int64, device=dev)
            node = torch.full((B, K), trie.find([cfg.decoder_start_token_id]), dtype=torch.int32, device=dev)
            running = torch.zeros((B, K), dtype=torch.float32, device=dev)
            running[:, 1:] = -1e9  # as the callback path starts
            short = torch.zeros((B,), dtype=torch.int32, device=dev)
            first = torch.arange(B, device=dev).view(B, 1) * K
            for _ in range(steps):
                logits = self.decode(seqs, hidden, mask)[:, -1, :].float()
                running, parent, tok, node, short_now = ops.beam_step(logits, running, node, trie)
                short |= short_now
                # (an unused slot holds -1, -1: it stays dead in the kernel, the decoder is given row 0 / token 0 for it)
                rows = (first + parent.clamp_min(0)).view(-1)
                seqs = torch.cat((seqs[rows], tok.clamp_min(0).view(-1, 1).to(torch.int64)), 1)
            bad = torch.stack((short.any(), (running < -1e8).any())).tolist()  # the search's one host read
            if bad[0]:
                raise ValueError(f"generate: fewer than num_beams={K} continuations are allowed: the constraint has "
                                 "fewer candidates than beams, which is not supported")
            if bad[1]:
                raise ValueError(f"generate: the constraint has fewer than num_beams={K} candidates, which is not supported")
            scores = running / float(steps)
            items = trie.leaf_item[node[:, :R].reshape(-1).to(torch.int64)].view(B, R).to(torch.int64)
            seqs = seqs.view(B, K, -1)[:, :R].reshape(B * R, -1)
            return {"sequences": seqs, "sequences_scores": scores[:, :R].reshape(-1), "item_index": items}
        finally:
            self.train(was_training)
