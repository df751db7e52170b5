"""NARM (API mirror of torch_rechub/models/matching/narm.py): item lookup -> GRU (csrc/session.hip, one launch each way
over the padded block, states from the row's length on zeroed as pack_padded_sequence leaves them) -> additive attention
over the states (ops.additive_attention_pool) -> [c_g | c_l] -> bilinear head.  ``forward`` returns the (B, V) scores
against the whole item table as the reference does; ``catalogue_head`` returns (user vector, item table) so that
MatchTrainer trains through ops.catalogue_cross_entropy without forming them.

The item table is a plain nn.Embedding with a dense gradient every step (the scores reach every row, row 0 included);
it is flagged ``_rh_dense`` so the optimizer takes the reference's dense-Adam trajectory for it."""
import torch
import torch.nn as nn
from torch.nn import GRU, Dropout, Embedding, Parameter

from ... import ops
from ._session import check_dense_table, lookup, session_counts


class NARM(nn.Module):

    def __init__(self, item_history_feature, hidden_dim, emb_dropout_p, session_rep_dropout_p, item_feature=None):
        super(NARM, self).__init__()
        self.item_history_feature = item_history_feature
        self.item_feature = item_feature
        self.item_emb = Embedding(item_history_feature.vocab_size, item_history_feature.embed_dim, padding_idx=0)
        self.item_emb._rh_dense = True
        self.mode = None
        self.emb_dropout = Dropout(emb_dropout_p)
        self.gru = GRU(input_size=item_history_feature.embed_dim, hidden_size=hidden_dim)
        self.a_1, self.a_2 = Parameter(torch.randn(hidden_dim, hidden_dim)), Parameter(torch.randn(hidden_dim, hidden_dim))
        self.v = Parameter(torch.randn(hidden_dim, 1))
        self.session_rep_dropout = Dropout(session_rep_dropout_p)
        self.b = Parameter(torch.randn(item_history_feature.embed_dim, hidden_dim * 2))

    def _compute_session_repr(self, input_dict):
        """c (B, 2H) = dropout([h_t | c_l]) (narm.py:47-66)."""
        check_dense_table(self)
        seq = input_dict[self.item_history_feature.name]
        B, L = (int(v) for v in seq.shape)
        mask, counts = session_counts(seq, check_full=True)
        emb = ops.dropout(lookup(self.item_emb, seq), self.emb_dropout.p, self.training)
        h, _ = ops.gru_layers(self.gru, emb, batch_first=True)
        H = h.shape[2]
        live = torch.arange(L, device=seq.device).unsqueeze(0) < counts.unsqueeze(1)
        h = h * live.unsqueeze(-1).to(h.dtype)  # pad_packed_sequence: zeros from the row's length on
        h_t = h.gather(1, (counts - 1).clamp(min=0).view(B, 1, 1).expand(B, 1, H)).squeeze(1)
        P = ops.linear(h.reshape(B * L, H), self.a_2).view(B, L, H)
        r = ops.linear(h_t, self.a_1)
        c_l = ops.additive_attention_pool(P, r, self.v, mask, h)
        return ops.dropout(torch.cat((h_t, c_l), dim=1), self.session_rep_dropout.p, self.training)

    def user_tower(self, x):
        if self.mode == "item":
            return None
        user_emb = ops.linear(self._compute_session_repr(x), self.b)  # c @ b^T
        if self.mode == "user":
            return user_emb
        return user_emb.unsqueeze(1)

    def item_tower(self, x):
        if self.mode == "user":
            return None
        if self.item_feature is not None:
            item_emb = lookup(self.item_emb, x[self.item_feature.name])
            if self.mode == "item":
                return item_emb
            return item_emb.unsqueeze(1)
        return None

    def catalogue_head(self, x):
        """(u (B, D), item table (V, D)): the full-catalogue scores are u @ table^T; None outside the full-catalogue mode."""
        if self.mode is not None or self.item_feature is not None:
            return None
        return ops.linear(self._compute_session_repr(x), self.b), self.item_emb.weight

    def forward(self, input_dict):
        if self.mode == "user":
            return self.user_tower(input_dict)
        if self.mode == "item":
            return self.item_tower(input_dict)
        if self.item_feature is not None:
            user_emb = self.user_tower(input_dict)
            item_emb = self.item_tower(input_dict)
            return torch.mul(user_emb, item_emb).sum(dim=-1).squeeze()
        u, table = self.catalogue_head(input_dict)
        return u @ table.T
