"""MIND (API mirror of torch_rechub/models/matching/mind.py): concat-pooled history -> CapsuleNetwork (bilinear type 0,
one routing launch) -> multi-interest user head -> list-wise scoring against the best interest (csrc/interest.hip)."""
import torch
from torch import nn

from ...basic.layers import CapsuleNetwork, EmbeddingLayer
from ._listwise import MultiInterestUser


class MIND(MultiInterestUser, nn.Module):

    def __init__(self, user_features, history_features, item_features, neg_item_feature, max_length, temperature=1.0,
                 interest_num=4):
        super().__init__()
        self.user_features = user_features
        self.item_features = item_features
        self.history_features = history_features
        self.neg_item_feature = neg_item_feature
        self.temperature = temperature
        self.interest_num = interest_num
        self.max_length = max_length
        self.user_dims = sum([fea.embed_dim for fea in user_features + history_features])
        self.embedding = EmbeddingLayer(user_features + item_features + history_features)
        self.capsule = CapsuleNetwork(self.history_features[0].embed_dim, self.max_length, bilinear_type=0,
                                      interest_num=self.interest_num)
        self.convert_user_weight = nn.Parameter(torch.rand(self.user_dims, self.history_features[0].embed_dim),
                                                requires_grad=True)
        self.mode = None

    def _interests(self, x, hist):
        return self.capsule(hist, self.gen_mask(x))
