"""YoutubeDNN (API mirror of torch_rechub/models/matching/youtube_dnn.py): user tower EmbeddingLayer -> MLP -> L2
normalise; the item side is the positive and ``neg_items`` rows, normalised and scored inside one list-wise HIP launch
(ops.listwise_logits: no (B, 1 + K, D) concatenation).  ``forward`` returns (B, 1 + K) logits / temperature."""
from torch import nn

from ...basic.layers import MLP, EmbeddingLayer
from ._listwise import ListwiseItems, normalize_rows


class YoutubeDNN(ListwiseItems, nn.Module):

    def __init__(self, user_features, item_features, neg_item_feature, user_params, temperature=1.0):
        super().__init__()
        self.user_features = user_features
        self.item_features = item_features
        self.neg_item_feature = neg_item_feature
        self.temperature = temperature
        self.user_dims = sum([fea.embed_dim for fea in user_features])
        self.embedding = EmbeddingLayer(user_features + item_features)
        self.user_mlp = MLP(self.user_dims, output_layer=False, **user_params)
        self.mode = None

    def user_tower(self, x):
        """(B, 1, D), or (B, D) in "user" mode."""
        if self.mode == "item":
            return None
        u = normalize_rows(self.user_mlp(self.embedding(x, self.user_features, squeeze_dim=True)))
        return u if self.mode == "user" else u.unsqueeze(1)

    def forward(self, x):
        user_embedding = self.user_tower(x)
        if self.mode == "user":
            return user_embedding
        if self.mode == "item":
            return self.item_tower(x)
        return self._logits(x, user_embedding, self.temperature)
