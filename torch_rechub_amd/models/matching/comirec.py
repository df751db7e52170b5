"""ComirecSA / ComirecDR (API mirror of torch_rechub/models/matching/comirec.py): concat-pooled history ->
MultiInterestSA (masked softmax + pooling in one launch) or CapsuleNetwork (bilinear type 2: per-position weight staged
in LDS, no (B, L, I*D, D) product) -> multi-interest user head -> list-wise scoring (csrc/interest.hip)."""
import torch
from torch import nn

from ...basic.layers import CapsuleNetwork, EmbeddingLayer, MultiInterestSA
from ._listwise import MultiInterestUser


class ComirecSA(MultiInterestUser, nn.Module):

    def __init__(self, user_features, history_features, item_features, neg_item_feature, temperature=1.0, interest_num=4):
        super().__init__()
        self.user_features = user_features
        self.item_features = item_features
        self.history_features = history_features
        self.neg_item_feature = neg_item_feature
        self.temperature = temperature
        self.interest_num = interest_num
        self.user_dims = sum([fea.embed_dim for fea in user_features + history_features])
        self.embedding = EmbeddingLayer(user_features + item_features + history_features)
        self.multi_interest_sa = MultiInterestSA(embedding_dim=self.history_features[0].embed_dim,
                                                 interest_num=self.interest_num)
        self.convert_user_weight = nn.Parameter(torch.rand(self.user_dims, self.history_features[0].embed_dim),
                                                requires_grad=True)
        self.mode = None

    def _interests(self, x, hist):
        return self.multi_interest_sa(hist, self.gen_mask(x).unsqueeze(-1).float())


class ComirecDR(MultiInterestUser, nn.Module):

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
        self.capsule = CapsuleNetwork(self.history_features[0].embed_dim, self.max_length, bilinear_type=2,
                                      interest_num=self.interest_num)
        self.convert_user_weight = nn.Parameter(torch.rand(self.user_dims, self.history_features[0].embed_dim),
                                                requires_grad=True)
        self.mode = None

    def _interests(self, x, hist):
        return self.capsule(hist, self.gen_mask(x))
