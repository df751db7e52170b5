"""STAMP (API mirror of torch_rechub/models/matching/stamp.py): masked item lookup, the session's mean m_s and last item
x_t, additive attention over the items with ``+ m_s`` and F.normalize(p=1)'s floor (ops.additive_attention_pool), then
the two tanh-Linear heads.  ``forward`` returns the (B, V) scores against the whole item table; ``catalogue_head`` hands
(user vector, item table) to ops.catalogue_cross_entropy.  The item table is flagged ``_rh_dense`` (see narm.py)."""
import torch
import torch.nn as nn

from ... import ops
from ._session import check_dense_table, lookup, session_counts


class STAMP(nn.Module):

    def __init__(self, item_history_feature, weight_std, emb_std, item_feature=None):
        super(STAMP, self).__init__()
        self.item_history_feature = item_history_feature
        self.item_feature = item_feature
        n_items, item_emb_dim, = item_history_feature.vocab_size, item_history_feature.embed_dim
        self.item_emb = nn.Embedding(n_items, item_emb_dim, padding_idx=0)
        self.item_emb._rh_dense = True
        self.mode = None
        self.w_0 = nn.Parameter(torch.zeros(item_emb_dim, 1))
        self.w_1_t = nn.Parameter(torch.zeros(item_emb_dim, item_emb_dim))
        self.w_2_t = nn.Parameter(torch.zeros(item_emb_dim, item_emb_dim))
        self.w_3_t = nn.Parameter(torch.zeros(item_emb_dim, item_emb_dim))
        self.b_a = nn.Parameter(torch.zeros(item_emb_dim))
        self._init_parameter_weights(weight_std)
        self.f_s = nn.Sequential(nn.Tanh(), nn.Linear(item_emb_dim, item_emb_dim))
        self.f_t = nn.Sequential(nn.Tanh(), nn.Linear(item_emb_dim, item_emb_dim))
        self.emb_std = emb_std
        self.apply(self._init_module_weights)

    def _init_parameter_weights(self, weight_std):
        nn.init.normal_(self.w_0, std=weight_std)
        nn.init.normal_(self.w_1_t, std=weight_std)
        nn.init.normal_(self.w_2_t, std=weight_std)
        nn.init.normal_(self.w_3_t, std=weight_std)

    def _init_module_weights(self, module):
        if isinstance(module, nn.Linear):
            module.weight.data.normal_(std=self.emb_std)
            if module.bias is not None:
                module.bias.data.zero_()
        elif isinstance(module, nn.Embedding):
            module.weight.data.normal_(std=self.emb_std)  # (row 0 too: the padding row is not zero)

    def _compute_user_repr(self, input_dict):
        """h_s * h_t (B, D) (stamp.py:55-71)."""
        check_dense_table(self)
        seq = input_dict[self.item_history_feature.name]
        B, L = (int(v) for v in seq.shape)
        mask, counts = session_counts(seq)
        counts = counts.unsqueeze(1)
        items = lookup(self.item_emb, seq) * mask.unsqueeze(-1)
        D = items.shape[2]
        # (an empty row has set the error word; its clamped index keeps the gather in bounds)
        x_t = lookup(self.item_emb, torch.gather(seq, 1, (counts - 1).clamp(min=0))).squeeze(1)
        m_s = items.sum(1) / counts
        P = ops.linear(items.reshape(B * L, D), self.w_1_t.t()).view(B, L, D)
        r = ops.linear(x_t, self.w_2_t.t()) + ops.linear(m_s, self.w_3_t.t(), self.b_a)
        m_a = ops.additive_attention_pool(P, r, self.w_0, mask, items, add=m_s, floor=True)
        return self.f_s(m_a) * self.f_t(x_t)

    def user_tower(self, x):
        if self.mode == "item":
            return None
        user_emb = self._compute_user_repr(x)
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
        """(u (B, D), item table (V, D)); None outside the full-catalogue mode."""
        if self.mode is not None or self.item_feature is not None:
            return None
        return self._compute_user_repr(x), self.item_emb.weight

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
