"""HLLMModel (reference torch_rechub/models/generative/hllm.py): frozen, pre-computed item embeddings + position (+ time
bucket) embeddings, pre-norm transformer blocks on the HIP causal softmax attention kernel, cosine logits over the items.

``HLLMTransformerBlock`` keeps the reference's four projections, FFN and LayerNorms on the library (F.linear /
F.layer_norm); the attention between them is ONE launch each way (ops.softmax_attention, csrc/hllm.hip) that reads the
relative-position bias table directly and never forms the (B, H, L, L) scores, softmax or dropout mask.  The two
nn.Dropout applications of the reference (on the attention weights and on the projected attention output) draw from
the project's counter hash, so a captured train step draws a new mask on every replay.

``forward`` returns the (B, L, V) logits as the reference does.  ``hidden_and_head`` returns the normalised hidden
states and the frozen item table without forming the logits: SeqTrainer feeds them to the fused next-token loss
(csrc/stream_ce.hip), whose backward then computes no (V, D) gradient at all.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from ... import ops
from ...utils.hstu_utils import RelPosBias


class HLLMTransformerBlock(nn.Module):
    """One pre-norm block: x + dropout(W_O attention(LN(x))), then x + FFN(LN(x)) (reference hllm.py:12-101)."""

    def __init__(self, d_model=512, n_heads=8, dropout=0.1):
        super().__init__()
        self.d_model = d_model
        self.n_heads = n_heads
        assert d_model % n_heads == 0, "d_model must be divisible by n_heads"
        self.head_dim = d_model // n_heads
        self.scale = self.head_dim**-0.5
        self.W_Q = nn.Linear(d_model, d_model)
        self.W_K = nn.Linear(d_model, d_model)
        self.W_V = nn.Linear(d_model, d_model)
        self.W_O = nn.Linear(d_model, d_model)
        ffn_hidden = 4 * d_model
        self.ffn = nn.Sequential(nn.Linear(d_model, ffn_hidden), nn.ReLU(), nn.Dropout(dropout), nn.Linear(ffn_hidden, d_model),
                                 nn.Dropout(dropout))
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x, rel_pos_bias=None):
        """x (B, L, D).  ``rel_pos_bias``: a ``RelPosBias`` module (its table is read by the kernel) or None.  A dense
        (1, H, L, L) tensor, as the reference's signature takes, has no kernel and is refused."""
        if rel_pos_bias is not None and not isinstance(rel_pos_bias, RelPosBias):
            raise RuntimeError("torch_rechub_amd: HLLMTransformerBlock takes the RelPosBias module, not its dense "
                               "(1, H, L, L) output: the attention kernel forms the bias from the table")
        table, max_len = None, x.shape[1]
        if rel_pos_bias is not None:
            table, max_len = rel_pos_bias.rel_pos_bias_table, rel_pos_bias.max_seq_len
            if x.shape[1] > max_len:
                raise ValueError(f"seq_len ({x.shape[1]}) exceeds max_seq_len ({max_len}).")
        p = self.dropout.p
        h = self.norm1(x)
        attn = ops.softmax_attention(self.W_Q(h), self.W_K(h), self.W_V(h), self.n_heads, max_len, bias_table=table,
                                     dropout_p=p, training=self.training, scale=self.scale)
        x = x + ops.dropout(self.W_O(attn), p, self.training)
        h = self.norm2(x)
        h = ops.dropout(F.relu(self.ffn[0](h)), self.ffn[2].p, self.training)
        return x + ops.dropout(self.ffn[3](h), self.ffn[4].p, self.training)


class HLLMModel(nn.Module):

    def __init__(self, item_embeddings, vocab_size, d_model=512, n_heads=8, n_layers=4, max_seq_len=256, dropout=0.1,
                 use_rel_pos_bias=True, use_time_embedding=True, num_time_buckets=2048, time_bucket_fn='sqrt',
                 temperature=0.07):
        super().__init__()
        self.vocab_size = vocab_size
        self.d_model = d_model
        self.n_heads = n_heads
        self.n_layers = n_layers
        self.max_seq_len = max_seq_len
        self.use_time_embedding = use_time_embedding
        self.num_time_buckets = num_time_buckets
        self.time_bucket_fn = time_bucket_fn
        self.temperature = temperature
        if isinstance(item_embeddings, str):
            item_embeddings = torch.load(item_embeddings)
        if item_embeddings.shape[0] != vocab_size:
            raise ValueError(f"item_embeddings.shape[0]={item_embeddings.shape[0]} "
                             f"!= vocab_size={vocab_size}. "
                             "Embedding tensor must be indexed by token_id "
                             "(row i = embedding of vocab token i, row 0 = PAD).")
        if item_embeddings.shape[1] != d_model:
            raise ValueError(f"item_embeddings.shape[1]={item_embeddings.shape[1]} != d_model={d_model}")
        # frozen, so normalised once
        self.register_buffer('item_embeddings', F.normalize(item_embeddings.float(), dim=-1, eps=1e-8))
        self.position_embedding = nn.Embedding(max_seq_len, d_model)
        if use_time_embedding:
            self.time_embedding = nn.Embedding(num_time_buckets + 1, d_model, padding_idx=0)
        self.transformer_blocks = nn.ModuleList(
            [HLLMTransformerBlock(d_model=d_model, n_heads=n_heads, dropout=dropout) for _ in range(n_layers)])
        self.use_rel_pos_bias = use_rel_pos_bias
        if use_rel_pos_bias:
            self.rel_pos_bias = RelPosBias(n_heads, max_seq_len)
        self.dropout = nn.Dropout(dropout)
        self._init_weights()

    def _init_weights(self):
        """Xavier-uniform for matrices (the time table's padding row included, as in the reference), zero biases."""
        for name, param in self.named_parameters():
            if 'weight' in name and len(param.shape) > 1:
                nn.init.xavier_uniform_(param)
            elif 'bias' in name:
                nn.init.constant_(param, 0)

    def _time_diff_to_bucket(self, time_diffs):
        """Seconds -> minutes -> sqrt | log, truncated, clamped to [0, num_time_buckets - 1]."""
        t = torch.clamp(time_diffs.float() / 60.0, min=1e-6)
        if self.time_bucket_fn == 'sqrt':
            buckets = torch.sqrt(t).long()
        elif self.time_bucket_fn == 'log':
            buckets = torch.log(t).long()
        else:
            raise ValueError(f"Unsupported time_bucket_fn: {self.time_bucket_fn}")
        return torch.clamp(buckets, min=0, max=self.num_time_buckets - 1)

    def hidden_and_head(self, seq_tokens, time_diffs=None):
        """(normalised hidden (B, L, D), item_embeddings (V, D), None): the logits are hidden @ item_embeddings^T /
        temperature."""
        batch_size, seq_len = seq_tokens.shape
        if seq_len > self.max_seq_len:  # the reference's position lookup fails with this error
            raise IndexError("index out of range in self")
        positions = torch.arange(seq_len, dtype=torch.long, device=seq_tokens.device)
        emb = self.item_embeddings[seq_tokens] + self.position_embedding(positions).unsqueeze(0)
        if self.use_time_embedding:
            if time_diffs is None:
                time_diffs = torch.zeros(batch_size, seq_len, dtype=torch.long, device=seq_tokens.device)
            emb = emb + self.time_embedding(self._time_diff_to_bucket(time_diffs))
        x = ops.dropout(emb, self.dropout.p, self.training)
        bias = self.rel_pos_bias if self.use_rel_pos_bias else None
        for block in self.transformer_blocks:
            x = block(x, rel_pos_bias=bias)
        return F.normalize(x, dim=-1, eps=1e-8), self.item_embeddings, None

    def forward(self, seq_tokens, time_diffs=None):
        h, emb, _ = self.hidden_and_head(seq_tokens, time_diffs)
        return torch.matmul(h, emb.t()) / self.temperature
