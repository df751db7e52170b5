"""Shared pieces of the list-wise retrieval models (YoutubeDNN, MIND, ComirecDR, ComirecSA): the item side and the
multi-interest user head, on the fused gathers and csrc/interest.hip."""
import torch

from ... import ops


def no_kernel(what):
    return RuntimeError(f"torch_rechub_amd: {what} has no HIP kernel; refusing to fall back to an eager path")


def normalize_rows(h):
    """F.normalize(h, p=2, dim=-1) over the last axis of a (..., D) float32 HIP tensor (csrc/match.hip)."""
    flat = h.reshape(-1, h.shape[-1])
    if not ops.l2_normalize_ok(flat):
        raise no_kernel(f"L2 normalisation of width {h.shape[-1]}")
    return ops.l2_normalize(flat).view(h.shape)


class ListwiseItems(object):
    """Mixin: the item tower and the list-wise logits over the positive and the ``neg_items`` rows."""

    def _check_tables(self):
        feas = self.item_features + self.neg_item_feature + list(getattr(self, "history_features", []))
        if self.embedding.is_sharded(feas):
            raise RuntimeError(f"torch_rechub_amd: {type(self).__name__} on row-sharded item tables is not supported")

    def _item_rows(self, x):
        """(pos (B, D), neg (B, K, D)): the raw rows from the fused gathers (no normalisation, no concatenation)."""
        self._check_tables()
        pos = self.embedding(x, self.item_features, squeeze_dim=True)
        neg = self.embedding(x, self.neg_item_feature, as_list=True)[0]
        if neg.dim() != 3:
            raise ValueError("neg_item_feature must be one concat-pooled SequenceFeature of shape (B, K)")
        return pos, neg

    def item_tower(self, x):
        if self.mode == "user":
            return None
        self._check_tables()
        pos = normalize_rows(self.embedding(x, self.item_features, squeeze_dim=True))
        if self.mode == "item":
            return pos
        neg = normalize_rows(self.embedding(x, self.neg_item_feature, as_list=True)[0])
        return torch.cat((pos.unsqueeze(1), neg), dim=1)

    def _logits(self, x, user, temperature):
        pos, neg = self._item_rows(x)
        logits, _ = ops.listwise_logits(user, pos, neg, temperature)
        return logits


class MultiInterestUser(ListwiseItems):
    """The user head of MIND / ComiRec: normalize(cat(expand(user), interests) @ convert_user_weight) computed as
    user @ W_top (once per sample) + interests @ W_bottom, without the expand and the concatenation."""

    def gen_mask(self, x):
        his_list = x[self.history_features[0].name]
        return (his_list > 0).long()

    def _interests(self, x, hist):
        raise NotImplementedError

    def user_tower(self, x):
        if self.mode == "item":
            return None
        user_in = self.embedding(x, self.user_features, squeeze_dim=True)
        hist = self.embedding(x, self.history_features, as_list=True)[0]
        interests = self._interests(x, hist)
        B, I, D = (int(v) for v in interests.shape)
        nu = int(user_in.shape[1])
        W = self.convert_user_weight
        top = ops.linear(user_in, W[:nu].t())
        bottom = ops.linear(interests.reshape(B * I, D), W[nu:].t()).view(B, I, -1)
        return normalize_rows(bottom + top.unsqueeze(1))

    def forward(self, x):
        user_embedding = self.user_tower(x)
        if self.mode == "user":
            return user_embedding
        if self.mode == "item":
            return self.item_tower(x)
        return self._logits(x, user_embedding, 1.0)  # (temperature is stored but never applied, as in the reference)
