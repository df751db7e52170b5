"""YoutubeSBC: two towers trained with an in-batch softmax and the sampling-bias correction of "Sampling-Bias-Corrected
Neural Modeling for Large Corpus Item Recommendations" (API mirror of torch_rechub/models/matching/youtube_sbc.py:16-98).

``forward`` returns the (B, 1 + n_neg) logits ``(cosine(u_i, v_j) - log(sample_weight_j)) / temperature`` of every user
row with its own item (column 0) and the items of the next ``n_neg`` rows of the batch, for ``MatchTrainer(mode=2)`` with
all-zero targets; ``mode`` "user" / "item" return the RAW tower outputs (no normalisation, as the reference).

The reference forms the cosine of EVERY pair (``torch.cosine_similarity(u.unsqueeze(1), v, dim=2)``: (B, B) out of a
(B, B, D) broadcast) and reads ``scores[index0, index1]`` with ``index1[i, k] = (i + k) mod B``.  On a HIP tensor that band
is computed straight from the tower outputs (``ops.band_logits``, csrc/twotower.hip): no (B, B) tensor, and an item
gradient that is a gather in a fixed order (bit-reproducible).

``index0`` / ``index1`` are the reference's numpy arrays, built and MUTATED exactly as it does (:47-49, :68-73): a batch
shorter than ``batch_size`` rewrites the leading slice of both arrays in place, which stays rewritten for every later full
batch -- those then read a few entries off the band.  The fused path is taken only while the arrays for the current batch
size ARE the band (checked on the host, cached until the arrays change); otherwise the reference's formulation runs on
torch ops on the device.  An index that is out of range for the batch raises IndexError on the host, as indexing does in
the reference, before anything reaches the device.
"""
import numpy as np
import torch
from torch import nn

from ... import ops
from ...basic.layers import MLP, EmbeddingLayer


class YoutubeSBC(nn.Module):

    def __init__(self, user_features, item_features, sample_weight_feature, user_params, item_params, batch_size, n_neg=3,
                 temperature=1.0):
        super().__init__()
        self.user_features = user_features
        self.item_features = item_features
        self.sample_weight_feature = sample_weight_feature
        self.n_neg = n_neg
        self.temperature = temperature
        self.user_dims = sum(fea.embed_dim for fea in user_features)
        self.item_dims = sum(fea.embed_dim for fea in item_features)
        self.batch_size = batch_size
        self.embedding = EmbeddingLayer(user_features + item_features + sample_weight_feature)
        self.user_mlp = MLP(self.user_dims, output_layer=False, **user_params)
        self.item_mlp = MLP(self.item_dims, output_layer=False, **item_params)
        self.mode = None
        # in-batch sampling index (the reference's arrays, :47-49)
        self.index0 = np.repeat(np.arange(batch_size), n_neg + 1)
        self.index1 = np.concatenate([np.arange(i, i + n_neg + 1) for i in range(batch_size)])
        self.index1[np.where(self.index1 >= batch_size)] -= batch_size
        self._band = {}     # batch size -> do the arrays read the band (i + k) mod B?   (host answers, until the arrays change)
        self._index_t = {}  # (batch size, device) -> the two arrays as device tensors, for the torch formulation

    def batch_indices(self, batch):
        """The reference's (index0, index1) for a batch of ``batch`` rows; a short batch rewrites the arrays in place."""
        k1 = self.n_neg + 1
        if batch * k1 == self.index0.shape[0]:
            return self.index0, self.index1
        index0, index1 = self.index0[:batch * k1], self.index1[:batch * k1]  # views: the rewrite below is permanent
        over0, over1 = index0 >= batch, index1 >= batch
        if over0.any() or over1.any():
            index0[over0] -= batch
            index1[over1] -= batch
            self._band.clear()
            self._index_t.clear()
        return index0, index1

    def band_ok(self, batch, indices=None):
        """True when ``scores[index0, index1]`` of a batch of ``batch`` rows is the band j = (i + k) mod batch.  Without
        ``indices`` (the pair ``batch_indices`` returned for this forward) the reference's short-batch rewrite is applied
        first, as one forward of such a batch would."""
        index0, index1 = self.batch_indices(batch) if indices is None else indices
        ok = self._band.get(batch)
        if ok is None:
            k1 = self.n_neg + 1
            rows = np.repeat(np.arange(batch), k1)
            ok = bool(index0.shape[0] == batch * k1 and k1 <= batch and np.array_equal(index0, rows) and
                      np.array_equal(index1, (rows + np.tile(np.arange(k1), batch)) % batch))
            self._band[batch] = ok
        return ok

    def _index_tensors(self, batch, device, indices):
        key = (batch, str(device))
        pair = self._index_t.get(key)
        if pair is None:
            index0, index1 = indices
            if index0.size and max(index0.max(), index1.max()) >= batch:
                raise IndexError(f"YoutubeSBC: in-batch index out of range for a batch of {batch} rows "
                                 f"(batch_size {self.batch_size}, n_neg {self.n_neg})")
            pair = (torch.from_numpy(index0.copy()).to(device), torch.from_numpy(index1.copy()).to(device))
            self._index_t[key] = pair
        return pair

    def forward(self, x):
        user_embedding = self.user_tower(x)
        item_embedding = self.item_tower(x)
        if self.mode == "user":
            return user_embedding
        if self.mode == "item":
            return item_embedding
        sample_weight = self.embedding(x, self.sample_weight_feature, squeeze_dim=True).squeeze(1)
        batch = user_embedding.shape[0]
        indices = self.batch_indices(batch)  # once per forward, as the reference: a short batch rewrites the arrays
        if user_embedding.is_cuda and self.band_ok(batch, indices) and \
                ops.band_logits_ok(user_embedding, item_embedding, sample_weight, self.n_neg):
            return ops.band_logits(user_embedding, item_embedding, sample_weight, self.n_neg, self.temperature)
        # the reference's formulation (:61-80) on torch ops, on the tensors' device
        index0, index1 = self._index_tensors(batch, user_embedding.device, indices)
        pred = torch.cosine_similarity(user_embedding.unsqueeze(1), item_embedding, dim=2)
        scores = (pred - torch.log(sample_weight))[index0, index1] / self.temperature
        return scores.view(-1, self.n_neg + 1)

    def user_tower(self, x):
        if self.mode == "item":
            return None
        return self.user_mlp(self.embedding(x, self.user_features, squeeze_dim=True))

    def item_tower(self, x):
        if self.mode == "user":
            return None
        return self.item_mlp(self.embedding(x, self.item_features, squeeze_dim=True))
