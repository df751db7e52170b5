"""DSSM with a SENET field gate in front of each tower (API mirror of torch_rechub/models/matching/dssm_senet.py:15-87; the
class is called ``DSSM`` there too -- ``models.matching`` exports it as ``DSSMSENet``).

Each tower: EmbeddingLayer(squeeze_dim=True) -> view (B, num_features, -1) -> SENETLayer -> MLP(no output layer) -> L2
normalise.  ``forward`` returns ``sigmoid(sum(user * item) / temperature)`` -- unlike the plain DSSM, whose reference never
applies its temperature, this one does (:54) --, or one tower's embedding when ``mode`` is "user" / "item".

``user_num_features`` / ``item_num_features`` follow the reference's counting rule verbatim (:37-38), operator precedence
included: every SparseFeature counts, shared or not, and a SequenceFeature counts only when it owns its table; the gather's
(B, sum of widths) output is viewed as that many fields of equal width.

On a HIP tensor the gate (mean, two bias-free Linear + ReLU, scale) is ONE launch each way over the gather's output, read in
place (``ops.senet``, csrc/twotower.hip); the normalisation is ``ops.l2_normalize`` as in DSSM.  ``towers`` runs the two
towers one after the other (``MatchTrainer(in_batch_neg=True)`` calls it).
"""
import torch
import torch.nn.functional as F
from torch import nn

from ... import ops
from ...basic.features import SequenceFeature, SparseFeature
from ...basic.layers import MLP, EmbeddingLayer, SENETLayer


def _count_fields(features):
    return len([fea.embed_dim for fea in features
                if isinstance(fea, SparseFeature) or isinstance(fea, SequenceFeature) and fea.shared_with is None])


class DSSM(nn.Module):

    def __init__(self, user_features, item_features, user_params, item_params, temperature=1.0):
        super().__init__()
        self.user_features = user_features
        self.item_features = item_features
        self.temperature = temperature
        self.user_dims = sum(fea.embed_dim for fea in user_features)
        self.item_dims = sum(fea.embed_dim for fea in item_features)
        self.embedding = EmbeddingLayer(user_features + item_features)
        self.user_mlp = MLP(self.user_dims, output_layer=False, **user_params)
        self.item_mlp = MLP(self.item_dims, output_layer=False, **item_params)
        self.user_num_features = _count_fields(user_features)
        self.item_num_features = _count_fields(item_features)
        self.user_senet = SENETLayer(self.user_num_features)
        self.item_senet = SENETLayer(self.item_num_features)
        self.user_senet.fused = self.item_senet.fused = True
        self.mode = None

    def _tower(self, x, features, num_features, senet, mlp):
        h = self.embedding(x, features, squeeze_dim=True)
        h = senet(h.view(h.size(0), num_features, -1))
        h = mlp(h.view(h.size(0), -1))
        return ops.l2_normalize(h) if ops.l2_normalize_ok(h) else F.normalize(h, p=2, dim=1)

    def user_tower(self, x):
        if self.mode == "item":
            return None
        return self._tower(x, self.user_features, self.user_num_features, self.user_senet, self.user_mlp)

    def item_tower(self, x):
        if self.mode == "user":
            return None
        return self._tower(x, self.item_features, self.item_num_features, self.item_senet, self.item_mlp)

    def towers(self, x):
        return self.user_tower(x), self.item_tower(x)

    def forward(self, x):
        user_embedding = self.user_tower(x)
        item_embedding = self.item_tower(x)
        if self.mode == "user":
            return user_embedding
        if self.mode == "item":
            return item_embedding
        y = torch.mul(user_embedding, item_embedding).sum(dim=1)
        return torch.sigmoid(y / self.temperature)
