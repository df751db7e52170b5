"""xDeepFM: LR + Compressed Interaction Network + MLP (Lian et al., KDD 2018).

The reference ships the layer (``basic.layers.CIN``, torch_rechub/basic/layers.py:322-368) and reserves a row for the
model in its ranking results, but has no model class; this is DeepFM's shape (torch_rechub/models/ranking/deepfm.py:14-43)
with ``FM`` replaced by ``CIN``: ``sigmoid(LR(flattened fm embeddings) + CIN(fm embeddings as (B, F, D)) + MLP(deep
embeddings))``.  Attributes ``linear``, ``cin``, ``embedding``, ``mlp``, constructed in that order.

When the fm features are plain sparse features of one width on replicated tables, ONE gather launch emits the MLP input
and the LR scalar (ops.fused_embedding), and CIN reads the sparse block of that output in place as a strided (B, F, D)
view -- PaddedEmbedding's padding columns and the dense columns are stepped over by the strides.  Everything else runs on
the layers; row-sharded fm tables are refused, as DeepFFM refuses them.
"""
import torch

from ... import ops
from ...basic.features import SparseFeature
from ...basic.layers import CIN, LR, MLP, EmbeddingLayer


class xDeepFM(torch.nn.Module):

    def __init__(self, deep_features, fm_features, mlp_params, cin_size, split_half=True):
        super().__init__()
        dims = {fea.embed_dim for fea in fm_features}
        if len(dims) != 1:
            raise ValueError(f"xDeepFM: the fm_features must share one embed_dim (CIN interacts them per embedding "
                             f"coordinate), got {sorted(dims)}")
        self.deep_features = deep_features
        self.fm_features = fm_features
        self.embed_dim = next(iter(dims))
        self.deep_dims = sum(fea.embed_dim for fea in deep_features)
        self.fm_dims = sum(fea.embed_dim for fea in fm_features)
        self.linear = LR(self.fm_dims)
        self.cin = CIN(len(fm_features), cin_size, split_half)
        self.embedding = EmbeddingLayer(deep_features + fm_features)
        self.mlp = MLP(self.deep_dims, **mlp_params)

    def _same_sparse_lists(self):
        deep_sparse = [f for f in self.deep_features if isinstance(f, SparseFeature)]
        return len(deep_sparse) == len(self.fm_features) and all(a is b for a, b in zip(deep_sparse, self.fm_features))

    def forward(self, x):
        emb, feas = self.embedding, self.fm_features
        F, D = len(feas), self.embed_dim
        if emb.is_sharded(feas):
            raise RuntimeError("torch_rechub_amd: xDeepFM does not support row-sharded fm tables (tables='shard'); keep "
                               "them replicated")
        dense = [f for f in self.deep_features if not isinstance(f, SparseFeature)]
        w, b = self.linear.fc.weight, self.linear.fc.bias
        if emb.can_fuse(x, feas):
            # replicated tables: the gather kernel emits the MLP input and the LR scalar; CIN reads its sparse block
            shared = self._same_sparse_lists() and emb.can_fuse(x, self.deep_features)
            call = emb.make_call(x, feas, dense if shared else (), want_lr=True)
            out, _, y_linear = ops.fused_embedding(call, emb.pad_lr_weight(w, feas), b)
            input_fm = out[:, :F * call.D].unflatten(1, (F, call.D))[:, :, :D]  # a view: strides (pitch, Dp, 1)
            if shared:
                input_deep = emb.compact(out, feas, len(call.dense))
        else:
            shared = False
            input_fm = emb(x, feas, squeeze_dim=False)
            y_linear = self.linear(input_fm.flatten(start_dim=1))
        if not shared:
            input_deep = emb(x, self.deep_features, squeeze_dim=True)
        return self.mlp.sigmoid_head(input_deep, y_linear, self.cin(input_fm))
