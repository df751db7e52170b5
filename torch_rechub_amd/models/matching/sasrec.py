"""SASRec (API mirror of torch_rechub/models/matching/sasrec.py, "Self-Attentive Sequential Recommendation"): one gather of
the seq / pos / neg ids from the shared item table -> ops.sasrec_input (scale, position rows, dropout, pad mask) -> per
block three launches: ops.sasrec_attention_in (LayerNorm of the query + the in-projection), ops.softmax_attention
(causal, dropout on the weights) and ops.sasrec_ffn (out-projection, residual from the NORMALISED query, LayerNorm,
point-wise FFN with its two dropouts, residual, pad mask) -> ops.sasrec_head (final LayerNorm + the two logit sums), all
in csrc/sasrec.hip and csrc/hllm.hip.  nn.MultiheadAttention, nn.Conv1d and nn.LayerNorm only hold the parameters under the
reference's names; their forwards are never called.

Three things the reference cannot do work here:
  * ``item_tower`` with an ``item_feature``: the reference reads ``self.item_emb.embedding``, which does not exist
    (AttributeError), so its in-batch ``forward`` and MatchTrainer(in_batch_neg=True) cannot run.  This one does what the
    reference's comments state: it looks ``x[item_feature.name]`` up in ``item_emb.embed_dict[features[0].name]`` and
    returns (B, 1, D), or (B, D) in item mode.
  * a batch of one sample and a history of one position (the reference's ``squeeze()`` drops those axes): every stage
    works on (B, L, D) for any B, L >= 1.
  * ``user_tower`` picks the last valid row first and normalises B rows, not B L.

Limits, refused before anything launches: embed_dim <= RH_SASREC_MAX_D, embed_dim divisible by num_heads, and a history of at
most min(max_len, RH_ATTN_MAX_L) positions (the attention kernel's bound; max_len itself may be larger).
"""
import torch

from ... import _lib, ops
from ._listwise import no_kernel


class PointWiseFeedForward(torch.nn.Module):
    """inputs + dropout2(conv2(relu(dropout1(conv1(inputs))))) over the last axis (kernel-size-1 convolutions = two D x D
    products).  Inside SASRec the parameters are read by ops.sasrec_ffn; called on its own it runs the products through
    ops.linear and the dropouts through ops.dropout."""

    def __init__(self, hidden_units, dropout_rate):
        super().__init__()
        self.conv1 = torch.nn.Conv1d(hidden_units, hidden_units, kernel_size=1)
        self.dropout1 = torch.nn.Dropout(p=dropout_rate)
        self.relu = torch.nn.ReLU()
        self.conv2 = torch.nn.Conv1d(hidden_units, hidden_units, kernel_size=1)
        self.dropout2 = torch.nn.Dropout(p=dropout_rate)

    def forward(self, inputs):
        ops.require_hip(inputs)
        D = inputs.shape[-1]
        rows = inputs.reshape(-1, D)
        h = ops.linear(rows, self.conv1.weight.view(D, D), self.conv1.bias)
        h = torch.relu(ops.dropout(h, self.dropout1.p, self.training))
        out = ops.dropout(ops.linear(h, self.conv2.weight.view(D, D), self.conv2.bias), self.dropout2.p, self.training)
        return out.view(inputs.shape) + inputs


class SASRec(torch.nn.Module):
    """features: the history, positive and negative SequenceFeatures, in this order, sharing the history's table
    (pooling="concat").  max_len: rows of the position table (a batch may be shorter).  item_feature: the target item's
    feature for the in-batch mode."""

    def __init__(self, features, max_len=50, dropout_rate=0.5, num_blocks=2, num_heads=1, item_feature=None):
        super().__init__()
        from ...basic.layers import EmbeddingLayer
        self.features = features
        self.item_feature = item_feature
        self.mode = None
        self.max_len = max_len
        self.item_num = self.features[0].vocab_size
        self.embed_dim = self.features[0].embed_dim

        self.item_emb = EmbeddingLayer(self.features)
        self.position_emb = torch.nn.Embedding(max_len, self.embed_dim)
        self.position_emb._rh_dense = True  # read as one slice, stepped whole
        self.emb_dropout = torch.nn.Dropout(p=dropout_rate)

        self.attention_layernorms = torch.nn.ModuleList()
        self.attention_layers = torch.nn.ModuleList()
        self.forward_layernorms = torch.nn.ModuleList()
        self.forward_layers = torch.nn.ModuleList()
        self.last_layernorm = torch.nn.LayerNorm(self.embed_dim, eps=1e-8)
        for _ in range(num_blocks):
            self.attention_layernorms.append(torch.nn.LayerNorm(self.embed_dim, eps=1e-8))
            self.attention_layers.append(torch.nn.MultiheadAttention(self.embed_dim, num_heads, dropout_rate))
            self.forward_layernorms.append(torch.nn.LayerNorm(self.embed_dim, eps=1e-8))
            self.forward_layers.append(PointWiseFeedForward(self.embed_dim, dropout_rate))

    # -- helpers -------------------------------------------------------------------------------
    def _check(self, L):
        """Everything that can be refused is refused before the first launch."""
        D = self.embed_dim
        if not 1 <= D <= _lib.H.RH_SASREC_MAX_D:
            raise no_kernel(f"SASRec at embed_dim {D} (1 <= D <= {_lib.H.RH_SASREC_MAX_D})")
        for mha in self.attention_layers:
            if D % mha.num_heads != 0:
                raise ValueError(f"SASRec: embed_dim {D} is not divisible by num_heads {mha.num_heads}")
        if L > self.max_len:  # the reference's position lookup fails with this error
            raise IndexError("index out of range in self")
        if L < 1:
            raise ValueError("SASRec: the history holds no position")
        if L > _lib.H.RH_ATTN_MAX_L:  # ops.softmax_attention's limit, met here so that no stage before it has launched
            raise no_kernel(f"SASRec on a history of {L} positions (the causal attention kernel takes L <= "
                            f"{_lib.H.RH_ATTN_MAX_L})")
        if self.item_emb.is_sharded(self.features):
            raise RuntimeError("torch_rechub_amd: SASRec on a row-sharded item table is not supported")

    def _seq_ids(self, x):
        seq = x[self.features[0].name]
        if seq.dim() != 2:
            raise ValueError(f"SASRec: the history must be (B, L) ids, got {tuple(seq.shape)}")
        self._check(int(seq.shape[1]))
        return seq

    # -- reference API -------------------------------------------------------------------------
    def seq_forward(self, x, embed_x_feature, normalize=True):
        """The blocks over the gathered history rows embed_x_feature (B, L, D) -> (B, L, D): normalised by last_layernorm as
        in the reference, or (``normalize=False``) the last block's output for callers that normalise fewer rows."""
        seq = self._seq_ids(x)
        B, L = (int(v) for v in seq.shape)
        D = self.embed_dim
        e = embed_x_feature.reshape(B, L, D) if embed_x_feature.dim() != 3 else embed_x_feature
        h = ops.sasrec_input(seq, e, self.position_emb.weight, self.emb_dropout.p, self.training)
        for ln_a, mha, ln_f, ffn in zip(self.attention_layernorms, self.attention_layers, self.forward_layernorms,
                                        self.forward_layers):
            Q, qkv = ops.sasrec_attention_in(h, ln_a.weight, ln_a.bias, mha.in_proj_weight, mha.in_proj_bias, ln_a.eps)
            attn = ops.softmax_attention(qkv[..., :D], qkv[..., D:2 * D], qkv[..., 2 * D:], mha.num_heads, self.max_len,
                                         dropout_p=mha.dropout, training=self.training)
            h = ops.sasrec_ffn(attn, Q, seq, mha.out_proj.weight, mha.out_proj.bias, ln_f.weight, ln_f.bias, ffn.conv1.weight,
                               ffn.conv1.bias, ffn.conv2.weight, ffn.conv2.bias, ln_f.eps, ffn.dropout1.p, self.training)
        if not normalize:
            return h
        return ops.layer_norm(h, self.last_layernorm.weight, self.last_layernorm.bias, self.last_layernorm.eps)

    def user_tower(self, x):
        """The normalised output at the last non-pad position (position 0 for an all-pad history): (B, 1, D), or (B, D)
        in user mode."""
        if self.mode == "item":
            return None
        seq = self._seq_ids(x)
        h = self.seq_forward(x, self.item_emb.shared_rows(x, self.features[:1]), normalize=False)
        last = ((seq != 0).sum(dim=1) - 1).clamp(min=0)
        picked = h[torch.arange(h.size(0), device=h.device), last]
        user_emb = ops.layer_norm(picked, self.last_layernorm.weight, self.last_layernorm.bias, self.last_layernorm.eps)
        if self.mode == "user":
            return user_emb
        return user_emb.unsqueeze(1)

    def item_tower(self, x):
        """The target item's row of the shared table: (B, 1, D), or (B, D) in item mode; None without an item_feature."""
        if self.mode == "user":
            return None
        if self.item_feature is None:
            return None
        item_emb = self.item_emb.shared_rows(x, [self.item_feature], table=self.item_emb.table_of(self.features[0]))
        if self.mode == "item":
            return item_emb.squeeze(1)
        return item_emb

    def forward(self, x):
        if self.mode == "user":
            return self.user_tower(x)
        if self.mode == "item":
            return self.item_tower(x)
        if self.item_feature is not None:  # in-batch mode: (B,) scores of each user against its own target
            return torch.mul(self.user_tower(x), self.item_tower(x)).sum(dim=-1).squeeze()
        seq = self._seq_ids(x)
        B, L = (int(v) for v in seq.shape)
        emb = self.item_emb.shared_rows(x, self.features).unflatten(1, (len(self.features), L))  # (B, 3, L, D): one launch
        h = self.seq_forward(x, emb[:, 0], normalize=False)
        return ops.sasrec_head(h, self.last_layernorm.weight, self.last_layernorm.bias, emb[:, 1], emb[:, 2],
                               self.last_layernorm.eps)
