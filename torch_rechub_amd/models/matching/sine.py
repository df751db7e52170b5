"""SINE (API mirror of torch_rechub/models/matching/sine.py, "Sparse-Interest Network for Sequential Recommendation"):
item + position embeddings -> the w_1 / w_k1 / w_3 products (ops.linear over the B S rows, tanh and the thin w_2 / w_k2
products) -> ops.sine_interests (concept scores, top-k, gated prototypes, intention assignment, interest encoding:
csrc/sine.hip) -> the w_4 / w_5 product -> ops.sine_aggregate.  Scoring against the positive and the negatives stays a
tensor expression, as the reference writes it.

The three tables are plain nn.Embedding modules flagged ``_rh_dense``: the item table has no padding row (row 0 receives
gradient like any other, unlike NARM / STAMP) and the reference steps all of it with dense Adam; the position table is
read as one slice and the concept table through the kernels."""
import torch
import torch.nn.functional as F

from ... import ops


class SINE(torch.nn.Module):

    def __init__(self, history_features, item_features, neg_item_features, num_items, embedding_dim, hidden_dim, num_concept,
                 num_intention, seq_max_len, num_heads=1, temperature=1.0):
        super().__init__()
        self.item_features = item_features
        self.history_features = history_features
        self.neg_item_features = neg_item_features
        self.temperature = temperature
        self.num_concept = num_concept
        self.num_intention = num_intention
        self.seq_max_len = seq_max_len
        self.num_heads = num_heads

        std = 1e-4
        self.item_embedding = torch.nn.Embedding(num_items, embedding_dim)
        torch.nn.init.normal_(self.item_embedding.weight, 0, std)
        self.concept_embedding = torch.nn.Embedding(num_concept, embedding_dim)
        torch.nn.init.normal_(self.concept_embedding.weight, 0, std)
        self.position_embedding = torch.nn.Embedding(seq_max_len, embedding_dim)
        torch.nn.init.normal_(self.position_embedding.weight, 0, std)
        for table in (self.item_embedding, self.concept_embedding, self.position_embedding):
            table._rh_dense = True

        self.w_1 = torch.nn.Parameter(torch.rand(embedding_dim, hidden_dim), requires_grad=True)
        self.w_2 = torch.nn.Parameter(torch.rand(hidden_dim, num_heads), requires_grad=True)

        self.w_3 = torch.nn.Parameter(torch.rand(embedding_dim, embedding_dim), requires_grad=True)

        self.w_k1 = torch.nn.Parameter(torch.rand(embedding_dim, hidden_dim), requires_grad=True)
        self.w_k2 = torch.nn.Parameter(torch.rand(hidden_dim, num_intention), requires_grad=True)

        self.w_4 = torch.nn.Parameter(torch.rand(embedding_dim, hidden_dim), requires_grad=True)
        self.w_5 = torch.nn.Parameter(torch.rand(hidden_dim, num_heads), requires_grad=True)

        self.mode = None

    def _check(self):
        if self.num_heads != 1:
            raise ValueError(f"SINE: num_heads={self.num_heads} is not supported: the reference's own forward reshapes the "
                             "(B, seq_max_len, num_heads) attention against the (B, seq_max_len) mask (sine.py:122) and "
                             "fails for num_heads != 1")
        for table in (self.item_embedding, self.concept_embedding, self.position_embedding):
            if getattr(table, "_rh_shard", None) is not None:
                raise RuntimeError("torch_rechub_amd: SINE on a row-sharded table is not supported")

    def forward(self, x):
        user_embedding = self.user_tower(x)
        item_embedding = self.item_tower(x)
        if self.mode == "user":
            return user_embedding
        if self.mode == "item":
            return item_embedding
        return torch.mul(user_embedding, item_embedding).sum(dim=-1)

    def user_tower(self, x):
        if self.mode == "item":
            return None
        self._check()
        hist_item = x[self.history_features[0]]
        B, S = (int(v) for v in hist_item.shape)
        if S != self.seq_max_len:
            raise ValueError(f"SINE: the history holds {S} positions, seq_max_len is {self.seq_max_len}")
        x_u = F.embedding(hist_item, self.item_embedding.weight) + self.position_embedding.weight.unsqueeze(0)
        mask = (hist_item > 0).to(torch.int32)
        E = int(x_u.shape[2])
        rows = x_u.reshape(B * S, E)
        a1 = (torch.tanh(ops.linear(rows, self.w_1.t())) @ self.w_2).view(B, S)
        a2 = (torch.tanh(ops.linear(rows, self.w_k1.t())) @ self.w_k2).view(B, S, self.num_intention)
        y = ops.linear(rows, self.w_3.t()).view(B, S, E)
        phi_u, x_u_hat, _ = ops.sine_interests(x_u, y, a1, a2, mask, self.concept_embedding.weight)
        a3 = (torch.tanh(ops.linear(x_u_hat.reshape(B * S, E), self.w_4.t())) @ self.w_5).view(B, S)
        v_u = ops.sine_aggregate(x_u_hat, a3, mask, phi_u, self.temperature)
        if self.mode == "user":
            return v_u
        return v_u.unsqueeze(1)

    def item_tower(self, x):
        if self.mode == "user":
            return None
        self._check()
        pos_embedding = F.embedding(x[self.item_features[0]], self.item_embedding.weight).unsqueeze(1)
        if self.mode == "item":  # inference embedding mode
            return pos_embedding.squeeze(1)  # [batch_size, embed_dim]
        neg_embeddings = F.embedding(x[self.neg_item_features[0]], self.item_embedding.weight).squeeze(1)
        return torch.cat((pos_embedding, neg_embeddings), dim=1)  # [batch_size, 1+n_neg_items, embed_dim]

    def gen_mask(self, x):
        name = self.history_features[0]  # (a feature name here; the reference's copy of this helper asks it for ``.name``)
        his_list = x[getattr(name, "name", name)]
        return (his_list > 0).long()
