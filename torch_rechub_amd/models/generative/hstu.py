"""HSTUModel (reference torch_rechub/models/generative/hstu.py): token + position (+ time-bucket) embeddings, an
HSTUBlock on the HIP attention kernel, and next-item logits over the (tied or untied) item table.

``forward`` returns the (B, L, V) logits as the reference does (one library GEMM).  ``hidden_and_head`` returns the final
hidden states and the head's (weight, bias) without forming the logits: SeqTrainer feeds them to the fused next-token
loss (ops.next_token_loss), so training never materialises (B, L, V).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ...basic.layers import HSTUBlock


class HSTUModel(nn.Module):

    def __init__(self, vocab_size, d_model=512, n_heads=8, n_layers=4, dqk=64, dv=64, max_seq_len=256, dropout=0.1,
                 use_time_embedding=True, num_time_buckets=128, time_bucket_fn='sqrt', time_bucket_divisor=1.0,
                 time_bucket_unit='minutes', tie_embeddings=True, score_norm='none', temperature=1.0, use_output_bias=True,
                 scale_input_embedding=False, l2_norm_eps=1e-6):
        super().__init__()
        if score_norm not in ('none', 'l2'):
            raise ValueError("score_norm must be 'none' or 'l2'")
        if temperature <= 0:
            raise ValueError("temperature must be positive")
        self.vocab_size = vocab_size
        self.d_model = d_model
        self.n_heads = n_heads
        self.n_layers = n_layers
        self.max_seq_len = max_seq_len
        self.use_time_embedding = use_time_embedding
        self.num_time_buckets = num_time_buckets
        self.time_bucket_fn = time_bucket_fn
        self.time_bucket_divisor = time_bucket_divisor
        self.time_bucket_unit = time_bucket_unit
        self.tie_embeddings = tie_embeddings
        self.score_norm = score_norm
        self.temperature = temperature
        self.use_output_bias = use_output_bias
        self.scale_input_embedding = scale_input_embedding
        self.l2_norm_eps = l2_norm_eps

        self.token_embedding = nn.Embedding(vocab_size, d_model, padding_idx=0)
        self.position_embedding = nn.Embedding(max_seq_len, d_model)
        if use_time_embedding:
            self.time_embedding = nn.Embedding(num_time_buckets, d_model)
        self.hstu_block = HSTUBlock(d_model=d_model, n_heads=n_heads, n_layers=n_layers, dqk=dqk, dv=dv, dropout=dropout,
                                    max_seq_len=max_seq_len, num_time_buckets=num_time_buckets,
                                    time_bucket_fn=time_bucket_fn, time_bucket_divisor=time_bucket_divisor,
                                    time_bucket_unit=time_bucket_unit)
        if tie_embeddings:
            self.output_bias = nn.Parameter(torch.zeros(vocab_size)) if use_output_bias else None
            self.output_projection = None
        else:
            self.output_projection = nn.Linear(d_model, vocab_size, bias=use_output_bias)
            self.output_bias = None
        self.dropout = nn.Dropout(dropout)
        self._init_weights()

    def _init_weights(self):
        """Xavier-uniform for matrices, zero biases, then the padding row of the token table back to zero."""
        for name, param in self.named_parameters():
            if 'weight' in name and len(param.shape) > 1:
                nn.init.xavier_uniform_(param)
            elif 'bias' in name:
                nn.init.constant_(param, 0)
        with torch.no_grad():
            self.token_embedding.weight[0].zero_()

    def _time_diff_to_bucket(self, time_diffs):
        """Input-side time buckets in [0, num_time_buckets - 1] (no abs: the deltas are non-negative by convention)."""
        t = time_diffs.float()
        if self.time_bucket_unit == 'minutes':
            t = t / 60.0
        t = torch.clamp(t, min=1e-6)
        if self.time_bucket_fn == 'sqrt':
            v = torch.sqrt(t)
        elif self.time_bucket_fn == 'log':
            v = torch.log(t)
        else:
            raise ValueError(f"Unsupported time_bucket_fn: {self.time_bucket_fn}")
        return (v / self.time_bucket_divisor).clamp(min=0, max=self.num_time_buckets - 1).long()

    def hidden_and_head(self, x, time_diffs=None):
        """(hidden (B, L, D), weight (V, D), bias (V,) or None): the logits are hidden @ weight^T + bias, / temperature;
        both sides already L2-normalised when score_norm == 'l2'."""
        batch_size, seq_len = x.shape
        if seq_len > self.max_seq_len:
            raise ValueError(f"Input seq_len ({seq_len}) exceeds max_seq_len ({self.max_seq_len}). "
                             f"Either truncate the input or rebuild the model with a larger max_seq_len.")
        padding_mask = x.ne(0)
        tok = self.token_embedding(x)
        if self.scale_input_embedding:
            tok = tok * (self.d_model**0.5)
        emb = tok + self.position_embedding(torch.arange(seq_len, dtype=torch.long, device=x.device)).unsqueeze(0)
        if self.use_time_embedding:
            if time_diffs is None:
                time_diffs = torch.zeros(batch_size, seq_len, dtype=torch.long, device=x.device)
            emb = emb + self.time_embedding(self._time_diff_to_bucket(time_diffs))
        emb = self.dropout(emb * padding_mask.unsqueeze(-1).to(emb.dtype))
        h = self.hstu_block(emb, padding_mask=padding_mask, time_diffs=time_diffs)
        h = h * padding_mask.unsqueeze(-1).to(h.dtype)
        if self.tie_embeddings:
            weight, bias = self.token_embedding.weight, self.output_bias
        else:
            weight, bias = self.output_projection.weight, self.output_projection.bias
        if self.score_norm == 'l2':
            h = F.normalize(h, p=2, dim=-1, eps=self.l2_norm_eps)
            weight = F.normalize(weight, p=2, dim=-1, eps=self.l2_norm_eps)
        return h, weight, bias

    def forward(self, x, time_diffs=None):
        h, weight, bias = self.hidden_and_head(x, time_diffs)
        logits = F.linear(h, weight, bias)
        if self.temperature != 1.0:
            logits = logits / self.temperature
        return logits

