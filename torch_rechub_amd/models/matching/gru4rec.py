"""GRU4Rec (API mirror of torch_rechub/models/matching/gru4rec.py): a two-layer bias-free GRU over the history (csrc/
session.hip, all L steps, trailing padding included) whose last state joins the user features in the MLP user tower;
list-wise training on the positive and the ``neg_items`` rows.  As in the reference, ``forward`` returns
y (B, D) = sum over dim 1 of u * [pos | neg] -- u times the SUM of the normalised item rows, not one dot product per
item -- with no temperature, and user_params["num_layers"] reaches the MLP (which then raises a TypeError)."""
import torch
from torch import nn

from ... import ops
from ...basic.layers import MLP, EmbeddingLayer
from ._listwise import ListwiseItems, normalize_rows


class GRU4Rec(ListwiseItems, nn.Module):

    def __init__(self, user_features, history_features, item_features, neg_item_feature, user_params, temperature=1.0):
        super().__init__()
        self.user_features = user_features
        self.item_features = item_features
        self.history_features = history_features
        self.neg_item_feature = neg_item_feature
        self.temperature = temperature
        self.user_dims = sum([fea.embed_dim for fea in user_features + history_features])
        self.embedding = EmbeddingLayer(user_features + item_features + history_features)
        self.gru = nn.GRU(input_size=history_features[0].embed_dim, hidden_size=history_features[0].embed_dim,
                          num_layers=user_params.get('num_layers', 2), batch_first=True, bias=False)
        self.user_mlp = MLP(self.user_dims, output_layer=False, **user_params)
        self.mode = None

    def forward(self, x):
        user_embedding = self.user_tower(x)
        item_embedding = self.item_tower(x)
        if self.mode == "user":
            return user_embedding
        if self.mode == "item":
            return item_embedding
        return torch.mul(user_embedding, item_embedding).sum(dim=1)

    def user_tower(self, x):
        if self.mode == "item":
            return None
        self._check_tables()
        input_user = self.embedding(x, self.user_features, squeeze_dim=True)
        hist = self.embedding(x, self.history_features, as_list=True)[0]
        _, h_n = ops.gru_layers(self.gru, hist)
        u = normalize_rows(self.user_mlp(torch.cat([input_user, h_n[-1]], dim=-1)))
        return u if self.mode == "user" else u.unsqueeze(1)
