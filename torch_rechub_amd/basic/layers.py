"""Hot-path building blocks with the reference's constructor signatures, attribute names and
``state_dict`` keys (torch_rechub/basic/layers.py), executing on hand-written gfx950 kernels.

| class            | reference (basic/layers.py) | execution here                                        |
|------------------|-----------------------------|-------------------------------------------------------|
| EmbeddingLayer   | :33-127                     | ONE fused multi-field gather launch (ops.fused_embedding); sequence features: gather+pool kernel |
| InputMask        | :130-161                    | integer compare (API shim; the pooling kernel masks in-register) |
| Sum/Average/ConcatPooling | :192-251           | API shims for direct use; EmbeddingLayer fuses pooling into the gather |
| LR               | :164-189                    | nn.Linear (library GEMV); DeepFM fuses it into the gather kernel |
| MLP              | :254-292                    | nn.Linear / BatchNorm1d / activation / Dropout (hipBLASLt: true dense contraction) |
| FM               | :295-319                    | ops.fm kernel; DeepFM fuses it into the gather kernel |
| CIN              | :322-368                    | ops.cin_layer: one MFMA GEMM launch per layer each way, the (B, F*Hp, D) product formed in registers |
| CrossNetwork     | :390-420                   | ops.cross_network: one wavefront per sample, all layers in registers |
| CrossNetV2       | :423-444                    | library GEMM + ONE fused Hadamard/bias/residual kernel (ops.cross_v2_epilogue) |
| CrossNetMix      | :447-506                    | experts batched into 3 GEMMs per layer (was 150 mm per step) + ONE fused bias/Hadamard/gate-mix/residual kernel |
| FFM              | :736-746                    | ops.ffm: one pass each way over the (B, F, F, D) input (DeepFFM fuses it into the lookup) |
| CEN              | :777-786                    | descriptor and rescale kernels (ops.cen_descriptor / cen_rescale) around the attention MLP |
| MultiInterestSA  | :568-609                    | GEMM path for tanh(E W1) W2, ONE masked-softmax + pooling launch each way (ops.sa_pool) |
| CapsuleNetwork   | :612-712                    | ONE routing launch with the projections in LDS (ops.capsule_routing); type 2 never forms (B, L, I*D, D) |
| HSTULayer / HSTUBlock | :792-972               | LayerNorms / proj1 / proj2 on the library, attention ONE launch each way (ops.hstu_attention) |

Tables stay ``nn.Embedding`` modules inside ``embed_dict`` (checkpoint ABI:
``embedding.embed_dict.<feature>.weight``); kernels read them in place.
"""
import math

import torch
from torch import nn

from .. import _lib, ops, sharding
from .activation import Dice, activation_layer
from .features import DenseFeature, SequenceFeature, SparseFeature


def _fusable_dim(d):
    q = d // 4
    return d % 4 == 0 and 4 <= d <= _lib.H.RH_SEQ_POOL_MAX_D and (q & (q - 1)) == 0


def _as_index(t):
    return t if t.dtype in (torch.int64, torch.int32) else t.long()


class PredictionLayer(nn.Module):
    """sigmoid for classification, identity for regression (reference layers.py:12-30)."""

    def __init__(self, task_type="classification"):
        super().__init__()
        if task_type not in ["classification", "regression"]:
            raise ValueError("task_type must be classification or regression")
        self.task_type = task_type

    def forward(self, x):
        return torch.sigmoid(x) if self.task_type == "classification" else x


class InputMask(nn.Module):
    """Float masks ``x != padding_idx`` (or ``!= -1`` when unset), one (B,1,...) slab per feature."""

    def forward(self, x, features):
        if not isinstance(features, list):
            features = [features]
        masks = []
        for fea in features:
            if not isinstance(fea, (SparseFeature, SequenceFeature)):
                raise ValueError("Only SparseFeature or SequenceFeature support to get mask.")
            sentinel = fea.padding_idx if fea.padding_idx is not None else -1
            masks.append((x[fea.name].long() != sentinel).unsqueeze(1).float())
        return torch.cat(masks, dim=1)


class ConcatPooling(nn.Module):
    """Identity on (B, L, D); the mask is ignored (reference layers.py:192-205)."""

    def forward(self, x, mask=None):
        return x


class SumPooling(nn.Module):
    """Masked sum over L: (B,1,L) x (B,L,D) -> (B,D) (reference layers.py:232-251)."""

    def forward(self, x, mask=None):
        if mask is None:
            return x.sum(dim=1)
        return (mask.transpose(1, 2) * x).sum(dim=1)


class AveragePooling(nn.Module):
    """Masked mean over L, denominator count + 1e-16 (reference layers.py:208-229)."""

    def forward(self, x, mask=None):
        if mask is None:
            return x.mean(dim=1)
        total = (mask.transpose(1, 2) * x).sum(dim=1)
        return total / (mask.sum(dim=-1).float() + 1e-16)


class EmbeddingLayer(nn.Module):
    """Multi-field embedding lookup; same contract as reference layers.py:33-127.

    forward(x, features, squeeze_dim=False):
      * dense only + squeeze_dim        -> (B, n_dense)
      * sparse, squeeze_dim=False       -> (B, n_features, D)   (or (B, n_seq, L, D) for concat pooling)
      * sparse (+dense), squeeze_dim    -> (B, sum(D) [+ n_dense]) with ALL sparse columns first, dense last (Q1)
    """

    def __init__(self, features):
        super().__init__()
        self.features = features
        self.embed_dict = nn.ModuleDict()
        self.n_dense = 0
        self.input_mask = InputMask()
        for fea in features:
            if fea.name in self.embed_dict:
                continue
            if isinstance(fea, (SparseFeature, SequenceFeature)) and fea.shared_with is None:
                self.embed_dict[fea.name] = fea.get_embedding_layer()
            elif isinstance(fea, DenseFeature):
                self.n_dense += 1

    def table_of(self, fea):
        return self.embed_dict[fea.name if fea.shared_with is None else fea.shared_with]

    def phys_dim(self, fea):
        """Row width the kernels see: ``embed_dim``, or the padded width of a PaddedEmbedding (initializers.py)."""
        return int(self.table_of(fea).weight.shape[1])

    _compact_cols = {}

    def compact(self, out, sparse_feas, n_tail=0):
        """(B, sum(phys) + n_tail) kernel output -> (B, sum(embed_dim) + n_tail): drops the zero padding columns of
        PaddedEmbedding tables (one index_select; identity when no table is padded)."""
        dims = tuple((self.phys_dim(f), f.embed_dim) for f in sparse_feas)
        if all(p == d for p, d in dims):
            return out
        key = (dims, n_tail, str(out.device))
        cols = EmbeddingLayer._compact_cols.get(key)
        if cols is None:
            if out.is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("torch_rechub_amd: run the step eagerly once before capturing a hipGraph")
            idx, at = [], 0
            for p, d in dims:
                idx += list(range(at, at + d))
                at += p
            idx += list(range(at, at + n_tail))
            cols = torch.tensor(idx, dtype=torch.long, device=out.device)
            EmbeddingLayer._compact_cols[key] = cols
        return out.index_select(1, cols)

    def pad_lr_weight(self, lr_w, sparse_feas):
        """LR weight (1, sum(embed_dim)) -> (1, sum(phys)) with zeros under the padding columns (differentiable)."""
        if lr_w is None or all(self.phys_dim(f) == f.embed_dim for f in sparse_feas):
            return lr_w
        pieces, at = [], 0
        for f in sparse_feas:
            pieces.append(torch.nn.functional.pad(lr_w[:, at:at + f.embed_dim], (0, self.phys_dim(f) - f.embed_dim)))
            at += f.embed_dim
        return torch.cat(pieces, dim=1).contiguous()

    def fused(self, x, sparse_feas, dense_feas=(), lr_w=None, lr_b=None, want_fm=False):
        """The fused gather (+ FM, + LR, + dense append) on logical widths: (out, fm, lr)."""
        call = self.make_call(x, sparse_feas, dense_feas, want_fm=want_fm, want_lr=lr_w is not None)
        out, fm, lr = ops.fused_embedding(call, self.pad_lr_weight(lr_w, sparse_feas), lr_b)
        return self.compact(out, sparse_feas, len(call.dense)), fm, lr

    # -- helpers ---------------------------------------------------------------------------
    def _dense_columns(self, x, dense_feas):
        cols = []
        for fea in dense_feas:
            v = x[fea.name].float()
            cols.append(v if v.dim() > 1 else v.unsqueeze(1))
        return cols

    def make_call(self, x, sparse_feas, dense_feas=(), **kw):
        """EmbedCall for a list of plain sparse features of one fusable embed_dim (+ 1-D dense values)."""
        weights = [self.table_of(f).weight for f in sparse_feas]
        pads = [self.table_of(f).padding_idx for f in sparse_feas]
        idx = [_as_index(x[f.name]) for f in sparse_feas]
        dense = [x[f.name].float() for f in dense_feas]
        return ops.EmbedCall(weights, pads, idx, dense, **kw)

    def is_sharded(self, features):
        """True when a table behind ``features`` is row-sharded over the ranks (sharding.shard_tables)."""
        return any(sharding.is_sharded(self.table_of(f)) for f in features
                   if isinstance(f, (SparseFeature, SequenceFeature)))

    def can_fuse(self, x, features):
        """True when the whole list is one fused launch: plain sparse, one dim, 1-D dense values, replicated tables
        (a sharded lookup is gather -> reduce-scatter: FM / LR cannot ride in the gather kernel)."""
        dims = set()
        if self.is_sharded(features):
            return False
        for fea in features:
            if isinstance(fea, SparseFeature):
                if x[fea.name].dim() != 1:
                    return False  # (B, K) indices: forward's multi-lookup path
                dims.add(self.phys_dim(fea))
            elif isinstance(fea, SequenceFeature):
                return False
            elif x[fea.name].dim() != 1:
                return False
        return len(dims) == 1 and _fusable_dim(next(iter(dims)))

    def can_fuse_sharded(self, x, features):
        """True when the list is ONE row-sharded lookup: plain sparse features of one width whose tables are all
        sharded, 1-D dense values (appended by ops.fused_rows)."""
        dims = set()
        for fea in features:
            if isinstance(fea, SparseFeature):
                if not sharding.is_sharded(self.table_of(fea)):
                    return False
                dims.add(fea.embed_dim)
            elif isinstance(fea, SequenceFeature):
                return False
            elif x[fea.name].dim() != 1:
                return False
        return len(dims) == 1 and _fusable_dim(next(iter(dims)))

    def sharded_rows(self, x, sparse_feas):
        """(B, F*D) rows of row-sharded tables for the local batch (index all-gather, shard gather, reduce-scatter)."""
        return sharding.lookup([self.table_of(f) for f in sparse_feas], [_as_index(x[f.name]) for f in sparse_feas])

    def _multi_lookup(self, x, table_feas, dense_feas, squeeze_dim):
        """(B, K) index per sparse feature (the field-aware lookup of the reference's DeepFFM, deepffm.py:57-58): (B, n, K, D),
        flattened for squeeze_dim.  ONE fused gather launch over n*K columns, each table repeated K times.  The indices
        are usually computed inside the step (x * F + offset), so the gather is announced as not replayable (EmbedCall)."""
        idx = [_as_index(x[f.name]) if isinstance(f, SparseFeature) else None for f in table_feas]
        if any(t is None or t.dim() != 2 for t in idx) or len({t.shape[1] for t in idx}) != 1:
            raise ValueError("torch_rechub_amd: (B, K) indices need every table feature to be a SparseFeature with the same K")
        if len({f.embed_dim for f in table_feas}) != 1 or len({self.phys_dim(f) for f in table_feas}) != 1:
            raise RuntimeError("torch_rechub_amd: a (B, K) lookup needs one embed_dim across its features")
        if self.is_sharded(table_feas):
            raise RuntimeError("torch_rechub_amd: (B, K) lookups on row-sharded tables are not supported")
        dim = self.phys_dim(table_feas[0])
        if not _fusable_dim(dim):
            raise RuntimeError(f"torch_rechub_amd: embed_dim={dim} has no HIP gather kernel")
        K = int(idx[0].shape[1])
        feas = [f for f in table_feas for _ in range(K)]
        # the indices land in ONE buffer owned by this layer (its address, hence its cached descriptor, stays fixed from the
        # eager steps into a hipGraph capture, where the computed index tensor lives elsewhere): one (B, K) lookup per layer
        # and step -- the backward reads the indices from it
        B = int(idx[0].shape[0])
        key = (B, len(idx), K, idx[0].dtype, str(idx[0].device))
        buf = self.__dict__.setdefault("_bk_index", {}).get(key)
        if buf is None:
            if idx[0].is_cuda and torch.cuda.is_current_stream_capturing():
                raise RuntimeError("torch_rechub_amd: run the step eagerly once before capturing a hipGraph")
            buf = self._bk_index[key] = torch.empty((B, len(idx), K), dtype=idx[0].dtype, device=idx[0].device)
        buf.copy_(torch.stack(idx, 1))
        call = ops.EmbedCall([self.table_of(f).weight for f in feas], [self.table_of(f).padding_idx for f in feas],
                             [buf[:, n, k] for n in range(len(idx)) for k in range(K)], replay=False)
        out, _, _ = ops.fused_embedding(call)
        out = self.compact(out, feas)
        if not squeeze_dim:
            return out.reshape(out.shape[0], len(table_feas), K, table_feas[0].embed_dim)
        if dense_feas:
            return torch.cat([out] + self._dense_columns(x, dense_feas), dim=1)
        return out

    def shared_rows(self, x, features, table=None):
        """(B, sum of L_i, D) rows of features that all read ONE replicated table -- concat-pooled sequence features with
        (B, L_i) ids, plain sparse features with (B,) ids (L_i = 1) -- as ONE gather launch, where ``forward`` takes one
        launch per sequence feature and a concatenation (SASRec: history, positives and negatives of the shared item
        table).  Several features: their ids land side by side in ONE buffer owned by this layer, as in ``_multi_lookup``
        (its address, hence the gather's cached descriptor, stays fixed from the eager steps into a hipGraph capture).
        ``table``: the embedding to read where the features do not name it themselves (SASRec's target item)."""
        if table is None:
            table = self.table_of(features[0])
            if any(self.table_of(f) is not table for f in features):
                raise ValueError("torch_rechub_amd: shared_rows needs features of one table")
        if sharding.is_sharded(table):
            raise RuntimeError("torch_rechub_amd: shared_rows on a row-sharded table is not supported")
        if not _fusable_dim(int(table.weight.shape[1])):
            raise RuntimeError(f"torch_rechub_amd: sequence embed_dim={features[0].embed_dim} has no HIP kernel (> {_lib.H.RH_SEQ_POOL_MAX_D})")
        parts = [_as_index(x[f.name]) for f in features]
        B = int(parts[0].shape[0])
        if len(parts) == 1 and parts[0].dim() == 1:
            # one plain sparse feature: the fused gather, which reads a strided id column (a DeviceDataLoader batch's) in place
            out, _, _ = ops.fused_embedding(ops.EmbedCall([table.weight], [table.padding_idx], parts))
            return out[:, :features[0].embed_dim].unsqueeze(1)
        parts = [t.reshape(B, -1) for t in parts]
        idx = parts[0]
        if len(parts) > 1:
            parts = [t if t.dtype == torch.int64 else t.long() for t in parts]
            key = (B, tuple(int(t.shape[1]) for t in parts), str(parts[0].device))
            idx = self.__dict__.setdefault("_shared_index", {}).get(key)
            if idx is None:
                if parts[0].is_cuda and torch.cuda.is_current_stream_capturing():
                    raise RuntimeError("torch_rechub_amd: run the step eagerly once before capturing a hipGraph")
                idx = self._shared_index[key] = torch.empty((B, sum(key[1])), dtype=torch.int64, device=parts[0].device)
            torch.cat(parts, dim=1, out=idx)
        rows = ops.seq_pool(table.weight, idx, "concat", table.padding_idx)
        return rows[..., :features[0].embed_dim]  # (a PaddedEmbedding's zero padding columns are cut off as a view)

    def pieces(self, x, features):
        """The per-feature tensors of ``forward(x, features)`` as a list -- (B, D) per sparse feature, (B, L, D) per
        concat-pooled sequence feature -- for callers that take the (B, n, ...) result apart again feature by feature
        (DIN: din.py:40-47).  Saves the concatenation and, in the backward, a zero-filled (B, n, L, D) buffer, a copy and
        an add per slice."""
        out = self.forward(x, features, as_list=True)
        return list(out.unbind(1)) if torch.is_tensor(out) else out

    def forward(self, x, features, squeeze_dim=False, as_list=False):
        table_feas = [f for f in features if isinstance(f, (SparseFeature, SequenceFeature))]
        dense_feas = [f for f in features if not isinstance(f, (SparseFeature, SequenceFeature))]
        for fea in table_feas:
            if isinstance(fea, SequenceFeature) and fea.pooling not in ("sum", "mean", "concat"):
                raise ValueError("Sequence pooling method supports only pooling in %s, got %s." %
                                 (["sum", "mean"], fea.pooling))
        if not table_feas:
            if squeeze_dim and dense_feas:
                return torch.cat(self._dense_columns(x, dense_feas), dim=1)
            if squeeze_dim:
                raise ValueError("The input features can note be empty")
            raise ValueError("If keep the original shape:[batch_size, num_features, embed_dim], expected %s in feature "
                             "list, got %s" % ("SparseFeatures", features))

        if any(isinstance(f, SparseFeature) and x[f.name].dim() == 2 for f in table_feas):
            return self._multi_lookup(x, table_feas, dense_feas, squeeze_dim)
        if self.can_fuse(x, features):
            sparse = table_feas
            out, _, _ = self.fused(x, sparse, dense_feas if squeeze_dim else ())
            return out if squeeze_dim else out.reshape(out.shape[0], len(sparse), sparse[0].embed_dim)
        if self.can_fuse_sharded(x, features):
            rows = self.sharded_rows(x, table_feas)
            if squeeze_dim and dense_feas:  # dense values appended by one launch over the received rows (Q1)
                rows, _, _ = ops.fused_rows(rows, len(table_feas), [x[f.name].float() for f in dense_feas])
            return rows if squeeze_dim else rows.view(rows.shape[0], len(table_feas), -1)

        # general path: sequence features, mixed widths, row-sharded tables -> per-group launches, reference order
        pieces = [None] * len(table_feas)
        groups = {}
        for i, fea in enumerate(table_feas):
            if isinstance(fea, SparseFeature):
                groups.setdefault((self.phys_dim(fea), sharding.is_sharded(self.table_of(fea))), []).append(i)
        for (dim, sharded), members in groups.items():
            if not _fusable_dim(dim):
                raise RuntimeError(f"torch_rechub_amd: embed_dim={dim} has no HIP gather kernel "
                                   f"(1 .. {_lib.H.RH_EMBED_MAX_D} supported, widths that are no power-of-two multiple of 4 through padded storage); "
                                   "refusing to fall back to a CPU/eager path")
            feas = [table_feas[i] for i in members]
            if sharded:
                out = sharding.lookup([self.table_of(f) for f in feas], [_as_index(x[f.name]) for f in feas])
            else:
                out, _, _ = ops.fused_embedding(self.make_call(x, feas))
            for k, i in enumerate(members):
                pieces[i] = out[:, k * dim:k * dim + table_feas[i].embed_dim].unsqueeze(1)
        for i, fea in enumerate(table_feas):
            if isinstance(fea, SequenceFeature):
                if not _fusable_dim(self.phys_dim(fea)):
                    raise RuntimeError(f"torch_rechub_amd: sequence embed_dim={fea.embed_dim} has no HIP kernel (> {_lib.H.RH_SEQ_POOL_MAX_D})")
                table = self.table_of(fea)
                idx = _as_index(x[fea.name])
                if not sharding.is_sharded(table):
                    pooled = ops.seq_pool(table.weight, idx, fea.pooling, table.padding_idx)
                elif fea.pooling == "concat":  # (B, L, D): L lookups of one table per sample through the same exchange
                    L = idx.shape[1]
                    pooled = sharding.lookup([table] * L, [idx[:, j] for j in range(L)]).view(-1, L, fea.embed_dim)
                else:
                    pooled = sharding.pooled_lookup(table, idx, fea.pooling)
                if pooled.shape[-1] != fea.embed_dim:  # PaddedEmbedding: cut the zero padding columns off
                    pooled = pooled[..., :fea.embed_dim]
                pieces[i] = pooled.unsqueeze(1)
        if as_list and not squeeze_dim:
            return [p.squeeze(1) for p in pieces]
        sparse_emb = torch.cat(pieces, dim=1)
        if not squeeze_dim:
            return sparse_emb
        flat = sparse_emb.flatten(start_dim=1)
        if dense_feas:
            return torch.cat([flat] + self._dense_columns(x, dense_feas), dim=1)
        return flat


class LR(nn.Module):
    """Linear(input_dim, 1) with optional sigmoid (reference layers.py:164-189)."""

    def __init__(self, input_dim, sigmoid=False):
        super().__init__()
        self.sigmoid = sigmoid
        self.fc = nn.Linear(input_dim, 1, bias=True)

    def forward(self, x):
        y = self.fc(x)
        return torch.sigmoid(y) if self.sigmoid else y


class MLP(nn.Module):
    """[Linear, BatchNorm1d, activation, Dropout] per hidden size, optional Linear(.,1) (reference :254-292)."""

    def __init__(self, input_dim, output_layer=True, dims=None, dropout=0, activation="relu"):
        super().__init__()
        layers = []
        for width in (dims or []):
            layers += [nn.Linear(input_dim, width), nn.BatchNorm1d(width), activation_layer(activation),
                       nn.Dropout(p=dropout)]
            input_dim = width
        if output_layer:
            layers.append(nn.Linear(input_dim, 1))
        self.mlp = nn.Sequential(*layers)

    @staticmethod
    def _bn_ok(bn, x):
        return (isinstance(bn, nn.BatchNorm1d) and bn.affine and bn.track_running_stats and bn.momentum is not None and
                x.is_cuda and x.dim() == 2 and x.dtype == torch.float32 and (x.shape[0] > 1 or not bn.training) and
                not (torch.is_grad_enabled() and not bn.training and x.requires_grad))

    @classmethod
    def _fusable(cls, bn, act, drop, x):
        return cls._bn_ok(bn, x) and isinstance(act, nn.ReLU) and isinstance(drop, nn.Dropout)

    @staticmethod
    def _linear(lin, x):
        return ops.linear(x, lin.weight, lin.bias) if type(lin) is nn.Linear and ops.linear_ok(x, lin.weight) else lin(x)

    @staticmethod
    def head_after(mods, j, width, bn, dice_mod):
        """The output Linear(width, 1) when mods[j:] is nothing but inactive Dropouts and that Linear, else None."""
        while j < len(mods) - 1 and isinstance(mods[j], nn.Dropout) and (mods[j].p == 0 or not mods[j].training):
            j += 1
        if j == len(mods) - 1 and ops.bn_dice_head_ok(width, bn, dice_mod, mods[j]):
            return mods[j]
        return None

    @staticmethod
    def _chain_blocks(mods):
        """[(Linear, BatchNorm1d, p_drop)] when ``mods`` is nothing but [Linear, BatchNorm1d, ReLU, Dropout] groups, else None."""
        if not mods or len(mods) % 4:
            return None
        out = []
        for i in range(0, len(mods), 4):
            lin, bn, act, drop = mods[i:i + 4]
            if not (type(lin) is nn.Linear and type(bn) is nn.BatchNorm1d and type(act) is nn.ReLU and type(drop) is nn.Dropout):
                return None
            out.append((lin, bn, float(drop.p) if drop.training else 0.0))
        return out

    def _run(self, mods, x):
        # [Linear, BatchNorm1d, ReLU, Dropout] blocks: library GEMM + ONE fused epilogue (csrc/mlp.hip); any other
        # activation (dice, prelu, sigmoid ...) runs the modules as they are.  Every Linear's weight / bias gradient
        # is the split-batch MFMA kernel of csrc/linear.hip.
        i = 0
        while i < len(mods):
            if i + 3 < len(mods) + 0 and isinstance(mods[i], nn.Linear) and self._fusable(mods[i + 1], mods[i + 2],
                                                                                            mods[i + 3], x):
                lin, bn = mods[i], mods[i + 1]
                if type(lin) is nn.Linear and bn.training and ops.linear_ok(x, lin.weight):
                    h, stats = ops.linear_stats(x, lin.weight, lin.bias, bn)  # GEMM epilogue emits the BN statistics
                else:
                    h, stats = self._linear(lin, x), None
                x = ops.bn_relu_dropout(h, bn, mods[i + 3].p if mods[i + 3].training else 0.0, stats=stats)
                i += 4
            elif (i + 2 < len(mods) and isinstance(mods[i], nn.Linear) and type(mods[i + 1]) is nn.BatchNorm1d and
                  type(mods[i + 2]) is Dice and self._bn_ok(mods[i + 1], x) and mods[i].out_features <= _lib.H.RH_BN_DICE_MAX_C and
                  not (torch.is_grad_enabled() and not mods[i + 1].training)):
                # Linear -> BatchNorm1d -> Dice (DIN's ActivationUnit): the normalisation is folded into the Dice passes
                head = self.head_after(mods, i + 3, mods[i].out_features, mods[i + 1], mods[i + 2])
                lin, bn = mods[i], mods[i + 1]
                if type(lin) is nn.Linear and bn.training and ops.linear_ok(x, lin.weight):
                    # ((B L)-row inputs: the tile GEMM's epilogue emits the BatchNorm's per-slab statistics, round 6)
                    h, cst, crows = ops.linear_chunk_stats(x, lin.weight, lin.bias)
                else:
                    h, cst, crows = self._linear(lin, x), None, 0
                if head is not None:
                    # ... -> Linear(C, 1) at the end of the stack: the Dice output is never written (ops.bn_dice_head)
                    return ops.bn_dice_head(h, bn, mods[i + 2].alpha, mods[i + 2].epsilon, head, chunk_stats=cst, chunk_rows=crows)
                x = ops.bn_dice(h, bn, mods[i + 2].alpha, mods[i + 2].epsilon, chunk_stats=cst, chunk_rows=crows)
                i += 3
            elif (i + 3 < len(mods) and isinstance(mods[i], nn.Linear) and type(mods[i + 1]) is nn.BatchNorm1d and
                  self._bn_ok(mods[i + 1], x) and isinstance(mods[i + 3], nn.Dropout) and
                  ops.bn_prelu_dropout_ok(x, mods[i + 1], mods[i + 2])):
                # Linear -> BatchNorm1d -> nn.PReLU() -> Dropout (the two-tower MLPs): ONE epilogue each way as for ReLU
                drop = mods[i + 3]
                x = ops.bn_prelu_dropout(self._linear(mods[i], x), mods[i + 1], mods[i + 2], drop.p if drop.training else 0.0)
                i += 4
            elif (i + 1 < len(mods) and isinstance(mods[i], nn.Linear) and type(mods[i + 1]) is nn.BatchNorm1d and
                  self._bn_ok(mods[i + 1], x)):
                # Linear -> BatchNorm1d in front of Dice / PReLU / ...: the normalisation alone through the same kernels
                x = ops.bn_relu_dropout(self._linear(mods[i], x), mods[i + 1], 0.0, relu=False)
                i += 2
            elif isinstance(mods[i], nn.Linear):
                x = self._linear(mods[i], x)
                i += 1
            elif ops.prelu_ok(mods[i], x):
                x = ops.prelu(x, mods[i].weight)  # nn.PReLU() of the two-tower MLPs: one pass each way
                i += 1
            else:
                x = mods[i](x)
                i += 1
        return x

    def forward(self, x):
        return self._run(list(self.mlp), x)

    def sigmoid_head(self, x, *extras):
        """sigmoid((sum(extras) + mlp(x)).squeeze(1)): the output Linear(., 1), the wide / FM terms of DeepFM / WideDeep
        (deepfm.py:39-43, widedeep.py:35-39) and the sigmoid as ONE kernel (ops.head_sigmoid) when the shapes allow."""
        mods = list(self.mlp)
        if mods and type(mods[-1]) is nn.Linear and mods[-1].out_features == 1:
            blocks = self._chain_blocks(mods[:-1])
            if blocks and ops.mlp_chain_ok(x, blocks, mods[-1], extras):
                # every hidden layer is Linear -> BatchNorm1d -> ReLU -> Dropout (training): ONE autograd node, the
                # BatchNorm / ReLU / Dropout of a layer applied where the next GEMM / the head reads it (ops._MlpChainFn)
                return ops.mlp_chain_sigmoid(x, blocks, mods[-1], *extras)
            h = self._run(mods[:-1], x)
            if ops.head_ok(h, mods[-1], extras):
                return ops.head_sigmoid(h, mods[-1].weight, mods[-1].bias, *extras)
            y = self._linear(mods[-1], h)
        else:
            y = self._run(mods, x)
        for e in reversed(extras):
            y = e + y
        return torch.sigmoid(y.squeeze(1))


class FM(nn.Module):
    """0.5 * sum_d[(sum_f x)^2 - sum_f x^2] (reference layers.py:295-319)."""

    def __init__(self, reduce_sum=True):
        super().__init__()
        self.reduce_sum = reduce_sum

    def forward(self, x):
        return ops.fm(x, self.reduce_sum)


class FFM(nn.Module):
    """Field-aware pairwise products of a (B, F, F, D) input: (B, P, D), or (B, P, 1) with reduce_sum (reference
    layers.py:714-746).  One HIP pass each way (ops.ffm); DeepFFM's fused path never builds the input at all."""

    def __init__(self, num_fields, reduce_sum=True):
        super().__init__()
        self.num_fields = num_fields
        self.reduce_sum = reduce_sum

    def forward(self, x):
        return ops.ffm(x, self.reduce_sum)


class CEN(nn.Module):
    """Compose-Excitation Network field attention of FAT-DeepFFM (reference layers.py:749-786): d = relu(sum_d u * em),
    s = mlp_att(d), aem = s * em flattened to (B, P*D).  ``u`` and ``mlp_att.mlp.*`` are the reference's parameters."""

    def __init__(self, embed_dim, num_field_crosses, reduction_ratio):
        super().__init__()
        self.u = torch.nn.Parameter(torch.rand(num_field_crosses, embed_dim), requires_grad=True)
        self.mlp_att = MLP(num_field_crosses, dims=[num_field_crosses // reduction_ratio, num_field_crosses],
                           output_layer=False, activation="relu")

    def forward(self, em):
        d = ops.cen_descriptor(em, self.u)
        s = self.mlp_att(d)
        return ops.cen_rescale(em, s)


class CIN(nn.Module):
    """Compressed Interaction Network of xDeepFM (reference layers.py:322-368): per layer relu(Conv1d(x0 (x) h)) over the
    F * Hp products of the input fields and the previous layer's channels, the first half of the channels kept and the
    second fed on under ``split_half``, then ``fc`` over the sum across the embedding axis.  ``conv_layers.{i}`` and ``fc`` are
    the reference's modules, built in its order.  Each layer is one MFMA GEMM launch each way (ops.cin_layer) that never
    forms the (B, F * Hp, D) product; a non-HIP input or a shape outside the kernel's ranges runs the reference's
    formulation on torch ops."""

    def __init__(self, input_dim, cin_size, split_half=True):
        super().__init__()
        self.num_layers = len(cin_size)
        self.split_half = split_half
        if split_half:
            odd = [int(s) for s in cin_size[:-1] if int(s) % 2]
            if odd:
                raise ValueError(f"CIN: with split_half every cin_size entry but the last must be even, got {list(cin_size)}: "
                                 f"the reference's forward fails on an odd one (torch.split(x, {odd[0]} // 2, dim=1) gives "
                                 "three pieces, unpacked into two names)")
        self.conv_layers = torch.nn.ModuleList()
        prev_dim, fc_input_dim = input_dim, 0
        for i in range(self.num_layers):
            cross_layer_size = cin_size[i]
            self.conv_layers.append(torch.nn.Conv1d(input_dim * prev_dim, cross_layer_size, 1, stride=1, dilation=1, bias=True))
            if self.split_half and i != self.num_layers - 1:
                cross_layer_size //= 2
            prev_dim = cross_layer_size
            fc_input_dim += prev_dim
        self.fc = torch.nn.Linear(fc_input_dim, 1)

    def forward(self, x):
        xs = []
        x0, h = x, x
        for i, conv in enumerate(self.conv_layers):
            if ops.cin_layer_ok(x0, h, conv.weight, conv.bias):
                y = ops.cin_layer(x0, h, conv.weight, conv.bias)
            else:
                z = x0.unsqueeze(2) * h.unsqueeze(1)
                y = torch.relu(conv(z.reshape(z.shape[0], z.shape[1] * z.shape[2], z.shape[3])))
            if self.split_half and i != self.num_layers - 1:
                y, h = torch.split(y, y.shape[1] // 2, dim=1)
            else:
                h = y
            xs.append(y)
        return self.fc(torch.sum(torch.cat(xs, dim=1), 2))


class CrossNetwork(nn.Module):
    """DCN cross layers x <- x0 * (w_l . x) + b_l + x (reference layers.py:390-420)."""

    def __init__(self, input_dim, num_layers):
        super().__init__()
        self.num_layers = num_layers
        self.w = nn.ModuleList([nn.Linear(input_dim, 1, bias=False) for _ in range(num_layers)])
        self.b = nn.ParameterList([nn.Parameter(torch.zeros((input_dim,))) for _ in range(num_layers)])

    def forward(self, x):
        W = torch.cat([lin.weight for lin in self.w], dim=0)
        Bv = torch.stack(list(self.b), dim=0)
        return ops.cross_network(x, W, Bv)


class CrossNetV2(nn.Module):
    """DCN-v2 full-rank cross layers x <- x0 * (W_l x) + b_l + x (reference layers.py:423-444)."""

    def __init__(self, input_dim, num_layers):
        super().__init__()
        self.num_layers = num_layers
        self.w = nn.ModuleList([nn.Linear(input_dim, input_dim, bias=False) for _ in range(num_layers)])
        self.b = nn.ParameterList([nn.Parameter(torch.zeros((input_dim,))) for _ in range(num_layers)])

    def forward(self, x):
        ops.require_hip(x)
        x0 = x
        for i in range(self.num_layers):
            if ops.cross_v2_layer_ok(x, self.w[i]):
                # ONE launch: the (d, d) product on the f32-MFMA tile GEMM with Hadamard + bias + residual as its epilogue
                x = ops.cross_v2_layer(x0, x, self.w[i].weight, self.b[i])
            else:  # (d, d) GEMM on hipBLASLt, then the fused Hadamard + bias + residual pass
                x = ops.cross_v2_epilogue(x0, self.w[i](x), self.b[i], x)
        return x


class CrossNetMix(nn.Module):
    """DCN-v2 mixture of low-rank experts (reference layers.py:447-506), experts batched.

    Per layer l and expert e:  g_e = gating_e(x_l);  v = tanh(V_e^T x_l);  v = tanh(C_e v);
    o_e = x0 * (U_e v + bias_l);  x_{l+1} = sum_e softmax(g)_e o_e + x_l.
    The reference loops layers x experts in Python on (B, d, 1) column vectors (150 mm per train
    step); here every layer is three batched GEMMs.  ``gating`` is shared across layers (Q11).
    """

    def __init__(self, input_dim, num_layers=2, low_rank=32, num_experts=4):
        super().__init__()
        self.num_layers = num_layers
        self.num_experts = num_experts
        mk = lambda *shape: nn.Parameter(nn.init.xavier_normal_(torch.empty(*shape)))
        self.u_list = nn.ParameterList([mk(num_experts, input_dim, low_rank) for _ in range(num_layers)])
        self.v_list = nn.ParameterList([mk(num_experts, input_dim, low_rank) for _ in range(num_layers)])
        self.c_list = nn.ParameterList([mk(num_experts, low_rank, low_rank) for _ in range(num_layers)])
        self.gating = nn.ModuleList([nn.Linear(input_dim, 1, bias=False) for _ in range(num_experts)])
        self.bias = nn.ParameterList([nn.Parameter(torch.zeros(input_dim, 1)) for _ in range(num_layers)])

    def forward(self, x):
        ops.require_hip(x)
        B, d = x.shape
        E = self.num_experts
        if (all(type(g) is nn.Linear and g.bias is None for g in self.gating) and
                ops.cross_moe_ok(x, self.num_layers, E, d, self.u_list[0].shape[2])):
            # two dense products + three fused passes per layer (csrc/moe.hip): the experts are the K dimension
            return ops.cross_moe(x, list(self.u_list), list(self.v_list), list(self.c_list), list(self.bias),
                                 [g.weight for g in self.gating])
        x0 = x
        xl = x
        Wg = torch.cat([g.weight for g in self.gating], dim=0)  # (E, d)
        for i in range(self.num_layers):
            U, V, C = self.u_list[i], self.v_list[i], self.c_list[i]
            r = V.shape[2]
            gate = torch.softmax(xl @ Wg.t(), dim=1)  # (B, E)
            v = torch.tanh(xl @ V.permute(1, 0, 2).reshape(d, E * r))  # (B, E*r)
            v = v.view(B, E, r).transpose(0, 1)  # (E, B, r)
            v = torch.tanh(torch.bmm(v, C.transpose(1, 2)))  # (E, B, r): C_e v
            uv = torch.bmm(v, U.transpose(1, 2))  # (E, B, d): U_e v
            if d <= _lib.H.RH_CROSS_MIX_MAX_D and E <= _lib.H.RH_CROSS_MIX_MAX_E:
                # bias + Hadamard with x0 + gate-weighted expert mix + residual: one pass (csrc/crossmix.hip)
                xl = ops.cross_mix_epilogue(x0, xl, uv, gate, self.bias[i])
            else:
                expert = x0.unsqueeze(0) * (uv + self.bias[i].view(1, 1, d))  # (E, B, d)
                xl = (expert * gate.t().unsqueeze(2)).sum(dim=0) + xl
        return xl


class SENETLayer(nn.Module):
    """SENET field gating: a = relu(W2 relu(W1 mean_d(x))), out = x * a[..., None] (reference layers.py:509-529).

    ``fused`` (off unless the owner sets it: the SENet DSSM does, FiBiNET does not) runs the whole layer as one HIP launch
    each way (csrc/twotower.hip) for a HIP float32 (B, F, D) block with F <= RH_SENET_MAX_F, D <= RH_SENET_MAX_D
    (ops.senet_ok)."""

    def __init__(self, num_fields, reduction_ratio=3):
        super().__init__()
        hidden = max(1, int(num_fields / reduction_ratio))
        self.mlp = nn.Sequential(nn.Linear(num_fields, hidden, bias=False), nn.ReLU(), nn.Linear(hidden, num_fields, bias=False),
                                 nn.ReLU())
        self.fused = False

    def forward(self, x):
        if self.fused and ops.senet_ok(x, self.mlp[0].weight, self.mlp[2].weight):
            return ops.senet(x, self.mlp[0].weight, self.mlp[2].weight)
        return x * self.mlp(x.mean(dim=-1)).unsqueeze(-1)


class BiLinearInteractionLayer(nn.Module):
    """(W v_i) * v_j for every field pair i < j (reference layers.py:532-565); W shared ("field_all"), one per left
    field ("field_each") or one per pair ("field_interaction").  Same parameters as the reference (``bilinear_layer`` is a
    Linear or a ModuleList of Linear(D, D, bias=False)); evaluated as one batched product over the pairs."""

    def __init__(self, input_dim, num_fields, bilinear_type="field_interaction"):
        super().__init__()
        self.bilinear_type = bilinear_type
        pairs = [(i, j) for i in range(num_fields) for j in range(i + 1, num_fields)]
        self.register_buffer("_left", torch.tensor([i for i, _ in pairs], dtype=torch.long), persistent=False)
        self.register_buffer("_right", torch.tensor([j for _, j in pairs], dtype=torch.long), persistent=False)
        if bilinear_type == "field_all":
            self.bilinear_layer = nn.Linear(input_dim, input_dim, bias=False)
        elif bilinear_type == "field_each":
            self.bilinear_layer = nn.ModuleList([nn.Linear(input_dim, input_dim, bias=False) for _ in range(num_fields)])
        elif bilinear_type == "field_interaction":
            self.bilinear_layer = nn.ModuleList([nn.Linear(input_dim, input_dim, bias=False) for _ in pairs])
        else:
            raise NotImplementedError()

    def forward(self, x):
        left, right = x[:, self._left], x[:, self._right]  # (B, P, D)
        if self.bilinear_type == "field_all":
            return self.bilinear_layer(left) * right
        w = torch.stack([lin.weight for lin in self.bilinear_layer])  # (F or P, D_out, D_in)
        if self.bilinear_type == "field_each":
            w = w[self._left]
        return torch.einsum("bpi,poi->bpo", left, w) * right


class InteractingLayer(nn.Module):
    """AutoInt's multi-head self-attention over the fields with a projected residual and a ReLU
    (reference layers.py:973-1044); W_Q / W_K / W_V / W_Res are applied as one product over their concatenation."""

    def __init__(self, embed_dim, num_heads=2, dropout=0.0, residual=True):
        super().__init__()
        if embed_dim % num_heads != 0:
            raise ValueError("embed_dim must be divisible by num_heads")
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.head_dim = embed_dim // num_heads
        self.scale = self.head_dim**-0.5
        self.residual = residual
        self.W_Q = nn.Linear(embed_dim, embed_dim, bias=False)
        self.W_K = nn.Linear(embed_dim, embed_dim, bias=False)
        self.W_V = nn.Linear(embed_dim, embed_dim, bias=False)
        self.W_Res = nn.Linear(embed_dim, embed_dim, bias=False) if residual else None
        self.dropout = nn.Dropout(dropout) if dropout > 0 else None

    def forward(self, x):
        B, Fn, D = x.shape
        H, Dh = self.num_heads, self.head_dim
        ws = [self.W_Q.weight, self.W_K.weight, self.W_V.weight] + ([self.W_Res.weight] if self.W_Res is not None else [])
        proj = (x.reshape(B * Fn, D) @ torch.cat(ws, dim=0).t()).view(B, Fn, len(ws), H, Dh)
        q, k, v = (proj[:, :, i].transpose(1, 2) for i in range(3))  # (B, H, F, Dh)
        w = torch.softmax((q @ k.transpose(-2, -1)) * self.scale, dim=-1)
        if self.dropout is not None:
            w = self.dropout(w)
        out = (w @ v).transpose(1, 2).reshape(B, Fn, D)
        if self.W_Res is not None:
            out = out + proj[:, :, 3].reshape(B, Fn, D)
        return torch.relu(out)


class CrossLayer(nn.Module):
    """One cross step without the residual: (w . x_i) * x_0 + b (reference layers.py:371-387; EDCN adds the residual)."""

    def __init__(self, input_dim):
        super().__init__()
        self.w = nn.Linear(input_dim, 1, bias=False)
        self.b = nn.Parameter(torch.zeros(input_dim))

    def forward(self, x_0, x_i):
        return self.w(x_i) * x_0 + self.b


def _interest_mask(mask, B, L):
    """(B, L) int32, nonzero = kept: the reference's ``mask == 0`` test of a (B, L) mask."""
    return (mask.reshape(B, L) != 0).to(torch.int32).contiguous()


class MultiInterestSA(nn.Module):
    """Self-attentive multi-interest extractor of ComiRec (reference layers.py:568-609), same parameters and init order.

    ``H = tanh(E W1)`` and ``H W2`` run on the GEMM path (ops.linear); the masked softmax over L and the pooling
    ``A^T E`` are one HIP launch each way (ops.sa_pool).  ``W3`` is built and never used, as in the reference."""

    def __init__(self, embedding_dim, interest_num, hidden_dim=None):
        super().__init__()
        self.embedding_dim = embedding_dim
        self.interest_num = interest_num
        if hidden_dim is None:  # (as in the reference, an explicit hidden_dim leaves self.hidden_dim unset)
            self.hidden_dim = self.embedding_dim * 4
        self.W1 = torch.nn.Parameter(torch.rand(self.embedding_dim, self.hidden_dim), requires_grad=True)
        self.W2 = torch.nn.Parameter(torch.rand(self.hidden_dim, self.interest_num), requires_grad=True)
        self.W3 = torch.nn.Parameter(torch.rand(self.embedding_dim, self.embedding_dim), requires_grad=True)

    def forward(self, seq_emb, mask=None):
        ops.require_hip(seq_emb)
        B, L, D = (int(v) for v in seq_emb.shape)
        if not ops.sa_supported(L, self.interest_num, D):
            raise RuntimeError(f"torch_rechub_amd: MultiInterestSA with L={L}, interest_num={self.interest_num}, "
                               f"embed_dim={D} has no HIP kernel (D <= {_lib.H.RH_SA_MAX_D}, "
                               f"L * interest_num <= {_lib.H.RH_SA_MAX_LI})")
        H = torch.tanh(ops.linear(seq_emb.reshape(B * L, D), self.W1.t()))
        A = ops.linear(H, self.W2.t()).view(B, L, self.interest_num)
        return ops.sa_pool(A, seq_emb, None if mask is None else _interest_mask(mask, B, L))


class CapsuleNetwork(nn.Module):
    """Dynamic-routing multi-interest extractor of MIND / ComiRec-DR (reference layers.py:612-712), same constructor,
    parameters, init order and routing semantics (iterations 0 and 1 route the detached projections; the output is the
    last iteration's; masked positions are zeroed after the softmax without renormalising).

    The routing runs in one HIP launch (ops.capsule_routing) with the per-sample projections in LDS; bilinear type 2
    never forms the reference's (B, L, I*D, D) product.  Types 0 / 1 project with ops.linear first.  MIND's (type 0)
    initial logits are ``torch.randn(B, interest_num, seq_len)`` drawn as the reference draws them; ``routing_init``, a
    callable ``(B, interest_num, seq_len, device) -> tensor``, replaces that draw (tests replay recorded draws through it)."""

    def __init__(self, embedding_dim, seq_len, bilinear_type=2, interest_num=4, routing_times=3, relu_layer=False):
        super().__init__()
        self.embedding_dim = embedding_dim
        self.seq_len = seq_len
        self.bilinear_type = bilinear_type
        self.interest_num = interest_num
        self.routing_times = routing_times
        self.relu_layer = relu_layer
        self.stop_grad = True
        self.relu = nn.Sequential(nn.Linear(self.embedding_dim, self.embedding_dim, bias=False), nn.ReLU())
        if self.bilinear_type == 0:
            self.linear = nn.Linear(self.embedding_dim, self.embedding_dim, bias=False)
        elif self.bilinear_type == 1:
            self.linear = nn.Linear(self.embedding_dim, self.embedding_dim * self.interest_num, bias=False)
        else:  # uninitialised storage, as the reference's torch.Tensor(...): no random draws
            self.w = nn.Parameter(torch.empty(1, self.seq_len, self.interest_num * self.embedding_dim, self.embedding_dim))
        self.routing_init = None

    def _init_logits(self, B, device):
        if self.bilinear_type != 0:
            return None
        if self.routing_init is not None:
            t = self.routing_init(B, self.interest_num, self.seq_len, device)
        else:
            t = torch.randn(B, self.interest_num, self.seq_len, device=device, requires_grad=False)
        return t.to(device=device, dtype=torch.float32).contiguous()

    def forward(self, item_eb, mask):
        ops.require_hip(item_eb)
        B, L, D = (int(v) for v in item_eb.shape)
        I = self.interest_num
        if L != self.seq_len or D != self.embedding_dim:
            raise RuntimeError(f"CapsuleNetwork: input of shape {tuple(item_eb.shape)} does not match seq_len={self.seq_len}, "
                               f"embedding_dim={self.embedding_dim}")
        if self.bilinear_type not in (0, 1, 2) or not ops.capsule_supported(L, I, D, self.bilinear_type) or \
                self.routing_times < 1:
            raise RuntimeError(f"torch_rechub_amd: CapsuleNetwork(bilinear_type={self.bilinear_type}, seq_len={L}, "
                               f"interest_num={I}, embedding_dim={D}, routing_times={self.routing_times}) has no HIP kernel")
        m = _interest_mask(mask, B, L)
        init = self._init_logits(B, item_eb.device)
        # with routing_times <= 2 the output comes from the detached projections: no gradient reaches them
        with torch.set_grad_enabled(torch.is_grad_enabled() and self.routing_times > 2):
            if self.bilinear_type == 2:
                cap = ops.capsule_routing(item_eb, self.w, m, init, 2, I, D, self.routing_times)
            else:
                U = ops.linear(item_eb.reshape(B * L, D), self.linear.weight).view(B, L, -1)
                cap = ops.capsule_routing(U, None, m, init, self.bilinear_type, I, D, self.routing_times)
        if self.relu_layer:
            cap = self.relu(cap)
        return cap


class HSTULayer(nn.Module):
    """One HSTU layer (reference basic/layers.py:792-933): U, V, Q, K = split(silu(proj1(LN(x)))), then
    proj2(dropout(LN(A V) * U)) with A = silu(alpha Q K^T + rab) / N under the causal and key-padding masks.  The
    attention is ONE HIP launch each way (ops.hstu_attention) that never forms the (B, H, L, L) scores or bias; the
    LayerNorms and the two projections stay on the library."""

    def __init__(self, d_model=512, n_heads=8, dqk=64, dv=64, dropout=0.1, max_seq_len=200, num_time_buckets=128,
                 time_bucket_fn='sqrt', time_bucket_divisor=1.0, time_bucket_unit='minutes'):
        super().__init__()
        if d_model % n_heads != 0:
            raise ValueError(f"d_model ({d_model}) must be divisible by n_heads ({n_heads}).")
        from ..utils.hstu_utils import RelativeBucketedTimeAndPositionBias
        self.d_model = d_model
        self.n_heads = n_heads
        self.dqk = dqk
        self.dv = dv
        self.max_seq_len = max_seq_len
        self.attn_alpha = 1.0 / math.sqrt(dqk)
        self.norm_in = nn.LayerNorm(d_model)
        self.proj1 = nn.Linear(d_model, 2 * n_heads * dqk + 2 * n_heads * dv)
        self.rab = RelativeBucketedTimeAndPositionBias(n_heads=n_heads, max_seq_len=max_seq_len,
                                                       num_time_buckets=num_time_buckets, time_bucket_fn=time_bucket_fn,
                                                       time_bucket_divisor=time_bucket_divisor,
                                                       time_bucket_unit=time_bucket_unit)
        self.norm_attn = nn.LayerNorm(n_heads * dv)
        self.proj2 = nn.Linear(n_heads * dv, d_model)
        self.dropout = nn.Dropout(dropout)

    def forward(self, x, padding_mask=None, time_diffs=None):
        H, dqk, dv = self.n_heads, self.dqk, self.dv
        proj = torch.nn.functional.silu(self.proj1(self.norm_in(x)))
        u = proj[..., 2 * H * dqk:2 * H * dqk + H * dv]
        rab = self.rab
        attn = ops.hstu_attention(proj, rab.pos_w, rab.ts_w, H, dqk, dv, self.max_seq_len, time_diffs=time_diffs,
                                  padding_mask=padding_mask, num_time_buckets=rab.num_time_buckets,
                                  time_bucket_fn=rab.time_bucket_fn, time_bucket_divisor=rab.time_bucket_divisor,
                                  time_bucket_unit=rab.time_bucket_unit)
        return self.proj2(self.dropout(self.norm_attn(attn) * u))


class HSTUBlock(nn.Module):
    """``n_layers`` HSTULayers with the external residual x = x + layer(x) (reference basic/layers.py:936-972)."""

    def __init__(self, d_model=512, n_heads=8, n_layers=4, dqk=64, dv=64, dropout=0.1, max_seq_len=200,
                 num_time_buckets=128, time_bucket_fn='sqrt', time_bucket_divisor=1.0, time_bucket_unit='minutes'):
        super().__init__()
        self.d_model = d_model
        self.n_heads = n_heads
        self.n_layers = n_layers
        self.layers = nn.ModuleList([
            HSTULayer(d_model=d_model, n_heads=n_heads, dqk=dqk, dv=dv, dropout=dropout, max_seq_len=max_seq_len,
                      num_time_buckets=num_time_buckets, time_bucket_fn=time_bucket_fn,
                      time_bucket_divisor=time_bucket_divisor, time_bucket_unit=time_bucket_unit)
            for _ in range(n_layers)
        ])

    def forward(self, x, padding_mask=None, time_diffs=None):
        for layer in self.layers:
            x = x + layer(x, padding_mask=padding_mask, time_diffs=time_diffs)
        return x
