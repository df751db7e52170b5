"""FaceBookDSSM: the pair-wise two-tower model of "Embedding-based Retrieval in Facebook Search" (API mirror of
torch_rechub/models/matching/dssm_facebook.py:15-77).

One user tower and one item tower that is applied to the positive and to the negative item features; ``forward`` returns
``(pos_score, neg_score)``, the cosines of the user embedding with the two item embeddings, for a pair-wise loss
(``MatchTrainer(mode=1)``: BPRLoss; the reference's docstring names ``basic.loss_func.HingeLoss``).  Kept from the
reference as it is:

  * the item MLP runs twice in a training forward, positive first, so its BatchNorm layers see two batches and update their
    running statistics twice per step;
  * ``item_tower`` returns a pair, ``(None, None)`` in user mode;
  * ``mode == "item"`` returns ``item_mlp(pos)`` WITHOUT the L2 normalisation (:71-72), ``mode == "user"`` the normalised
    user embedding;
  * ``temperature`` is stored and never applied.

On a HIP tensor the three F.normalize calls and the two multiply-sum reductions of the training forward are ONE launch each
way from the raw tower outputs (``ops.pair_cosine_scores``, csrc/twotower.hip).  The three gathers and the three MLP runs
stay in order on the calling stream; running the user MLP beside the item MLP's two runs (``ops.run_beside``, as
``DSSM.towers`` does) is not done here: its gain for this model is unmeasured.
"""
import torch.nn.functional as F
from torch import nn

from ... import ops
from ...basic.layers import MLP, EmbeddingLayer


def _normalize(h):
    return ops.l2_normalize(h) if ops.l2_normalize_ok(h) else F.normalize(h, p=2, dim=1)


class FaceBookDSSM(nn.Module):

    def __init__(self, user_features, pos_item_features, neg_item_features, user_params, item_params, temperature=1.0):
        super().__init__()
        self.user_features = user_features
        self.pos_item_features = pos_item_features
        self.neg_item_features = neg_item_features
        self.temperature = temperature
        self.user_dims = sum(fea.embed_dim for fea in user_features)
        self.item_dims = sum(fea.embed_dim for fea in pos_item_features)
        self.embedding = EmbeddingLayer(user_features + pos_item_features + neg_item_features)
        self.user_mlp = MLP(self.user_dims, output_layer=False, **user_params)
        self.item_mlp = MLP(self.item_dims, output_layer=False, **item_params)
        self.mode = None

    def _raw(self, x):
        """The three tower outputs before normalisation, in the reference's order (user, positive, negative)."""
        hu = self.user_mlp(self.embedding(x, self.user_features, squeeze_dim=True))
        hp = self.item_mlp(self.embedding(x, self.pos_item_features, squeeze_dim=True))
        hn = self.item_mlp(self.embedding(x, self.neg_item_features, squeeze_dim=True))
        return hu, hp, hn

    def forward(self, x):
        if self.mode not in ("user", "item"):
            hu, hp, hn = self._raw(x)
            if ops.pair_cosine_scores_ok(hu, hp, hn):
                return ops.pair_cosine_scores(hu, hp, hn)
            u, p, n = _normalize(hu), _normalize(hp), _normalize(hn)
            return (u * p).sum(dim=1), (u * n).sum(dim=1)
        user_embedding = self.user_tower(x)
        pos_item_embedding, _ = self.item_tower(x)
        return user_embedding if self.mode == "user" else pos_item_embedding

    def user_tower(self, x):
        if self.mode == "item":
            return None
        return _normalize(self.user_mlp(self.embedding(x, self.user_features, squeeze_dim=True)))

    def item_tower(self, x):
        if self.mode == "user":
            return None, None
        pos = self.embedding(x, self.pos_item_features, squeeze_dim=True)
        if self.mode == "item":  # the reference's inference mode: not normalised
            return self.item_mlp(pos), None
        neg = self.embedding(x, self.neg_item_features, squeeze_dim=True)
        hp, hn = self.item_mlp(pos), self.item_mlp(neg)
        return _normalize(hp), _normalize(hn)
