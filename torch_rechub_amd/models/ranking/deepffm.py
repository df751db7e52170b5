"""DeepFFM and FAT-DeepFFM (API mirror of torch_rechub/models/ranking/deepffm.py:15-134).

Reference forward: the linear part as a sum of width-1 lookups; the field-aware part as a lookup of x * F + fields_offset
-- a (B, F, F, D) tensor -- then F(F-1)/2 slice products and a stack (FFM), for FAT-DeepFFM the CEN field attention, then
the MLP.  Here, when the cross features are plain sparse features of one width on replicated tables, ONE kernel reads the
2P rows each sample needs straight from the tables and writes the (B, P*D) MLP input (ops.ffm_fused); the linear part is
the fused gather with its LR epilogue summing the width-1 rows.  Otherwise the reference's path runs on the HIP layers:
(B, K) lookup (EmbeddingLayer) -> FFM.  Parameter and buffer names are the reference's (``b``, ``fields_offset``,
``linear_embedding.*``, ``ffm_embedding.*``, ``cen.*``, ``mlp_out.mlp.*``).
"""
import torch

from ... import ops
from ...basic.features import SparseFeature
from ...basic.layers import CEN, FFM, MLP, EmbeddingLayer


class DeepFFM(torch.nn.Module):

    def __init__(self, linear_features, cross_features, embed_dim, mlp_params):
        super().__init__()
        self._build(linear_features, cross_features, embed_dim, None, mlp_params)

    def _build(self, linear_features, cross_features, embed_dim, reduction_ratio, mlp_params):
        # construction order = the reference's (parameter initialisation draws from the global RNG in this order)
        self.linear_features = linear_features
        self.cross_features = cross_features
        self.num_fields = len(cross_features)
        self.num_field_cross = self.num_fields * (self.num_fields - 1) // 2
        self.embed_dim = embed_dim
        self.ffm = FFM(num_fields=self.num_fields, reduce_sum=False)
        if reduction_ratio is not None:
            self.cen = CEN(embed_dim, self.num_field_cross, reduction_ratio)
        self.mlp_out = MLP(self.num_field_cross * embed_dim, **mlp_params)
        self.linear_embedding = EmbeddingLayer(linear_features)
        self.ffm_embedding = EmbeddingLayer(cross_features)
        self.b = torch.nn.Parameter(torch.zeros(1))
        self.register_buffer("fields_offset", torch.arange(0, self.num_fields, dtype=torch.long))
        self._ones = {}

    def _linear(self, x):
        """(B, 1) sum of the linear features' lookups."""
        emb, feas = self.linear_embedding, self.linear_features
        if all(isinstance(f, SparseFeature) for f in feas) and emb.can_fuse(x, feas):
            call = emb.make_call(x, feas, want_lr=True)
            key = (call.F, call.D, str(call.device))
            ones = self._ones.get(key)
            if ones is None:  # LR weight 1 on the logical columns, 0 on PaddedEmbedding's padding
                ones = torch.zeros((call.F, call.D), dtype=torch.float32, device=call.device)
                for f, fea in enumerate(feas):
                    ones[f, :fea.embed_dim] = 1.0
                ones = self._ones[key] = ones.view(1, -1)
            return ops.fused_embedding(call, ones, None)[2]
        return emb(x, feas, squeeze_dim=True).sum(1, keepdim=True)

    def _interaction(self, x):
        """(B, P*D) field-aware pairwise products (the reference's FFM output, flattened)."""
        emb, feas = self.ffm_embedding, self.cross_features
        if emb.is_sharded(feas):
            raise RuntimeError("torch_rechub_amd: DeepFFM / FatDeepFFM do not support row-sharded field-aware tables "
                               "(tables='shard'); keep them replicated")
        if all(isinstance(f, SparseFeature) for f in feas) and emb.can_fuse(x, feas):
            call = ops.FfmCall([emb.table_of(f).weight for f in feas], [emb.table_of(f).padding_idx for f in feas],
                               [x[f.name] if x[f.name].dtype in (torch.int64, torch.int32) else x[f.name].long()
                                for f in feas], self.embed_dim)
            return ops.ffm_fused(call)
        x_ffm = {f.name: x[f.name].unsqueeze(1) * self.num_fields + self.fields_offset for f in feas}
        return self.ffm(emb(x_ffm, feas, squeeze_dim=False)).flatten(start_dim=1)

    def forward(self, x):
        y_linear = self._linear(x)
        em = self._interaction(x)
        if hasattr(self, "cen"):
            em = self.cen(em)
        return self.mlp_out.sigmoid_head(em, y_linear + self.b)


class FatDeepFFM(DeepFFM):

    def __init__(self, linear_features, cross_features, embed_dim, reduction_ratio, mlp_params):
        torch.nn.Module.__init__(self)
        self._build(linear_features, cross_features, embed_dim, reduction_ratio, mlp_params)
