"""In-batch negative sampling for two-tower training (API mirror of torch_rechub/utils/match.py:104-161).

The reference loops ``for i in range(batch_size)`` in Python, launching a randperm / topk per row (O(B) tiny launches,
SURVEY 3.5).  Here both modes are ONE batched device op over the (B, B) score matrix:
  * hard negatives: top-k of the scores with the diagonal masked to -inf (same indices as the reference: its
    known-answer test [[1,2,3],[4,5,6],[7,8,0]] -> [2,2,1] holds);
  * random negatives, two streams:
    - ``stream="reference"`` (always used for CPU tensors; opt-in on the GPU, ``MatchTrainer(sampler_stream=
      "reference")``): the reference's own draw, ``candidates[randperm(B-1, generator=g)[:k]]`` row after row
      (match.py:141-145) -- the SAME indices as the reference for the same ``torch.Generator`` state on the same
      device type, bit for bit (pinned on CPU by tests/golden/inbatch_random.npz, generated from the unmodified
      reference).  B launches + host control flow: not hipGraph-capturable; for parity runs.
    - ``stream="fast"`` (GPU default): ONE HIP launch (``rh_inbatch_sample``: Floyd's algorithm per row, counter-based
      RNG, hipGraph-replayable).  DOCUMENTED DEVIATION: a different random stream, hence different indices for the
      same seed; what is preserved is the distribution -- every row draws a uniformly random k-subset of the other
      B-1 columns without replacement (chi-square-tested on the device, tests/test_gpu_kernels.py); the in-batch
      losses are symmetric in the negatives, so only the set matters.
"""
import torch


def _reference_stream(n_rows, n_cols, row_offset, neg_ratio, device, generator):
    """The reference's per-row draw (utils/match.py:136-145): row i takes candidates[randperm(C-1)[:k]] with
    candidates = every column but its own.  ``row_offset``: the rows are rows [row_offset, row_offset + n_rows) of a
    C x C global problem -- the generator is advanced through EVERY global row, so N ranks seeded alike draw what
    one process draws for the global batch."""
    out = torch.empty((n_rows, neg_ratio), dtype=torch.long, device=device)
    for i in range(n_cols):
        perm = torch.randperm(n_cols - 1, device=device, generator=generator)
        if row_offset <= i < row_offset + n_rows:
            pick = perm[:neg_ratio]
            out[i - row_offset] = pick + (pick >= i).long()  # candidates = arange(C) without i
    return out

_OWN = {}


def _own_mask(rows, cols, row_offset, device):
    """Cached (rows, cols) boolean mask of each row's own column (row_offset + i): built once, outside any hipGraph
    (an in-graph torch.eye re-creates it from a memset node on every replay)."""
    key = (rows, cols, row_offset, str(device))
    m = _OWN.get(key)
    if m is None:
        if device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("in-batch sampler: run one eager step before capturing a hipGraph")
        m = torch.zeros((rows, cols), dtype=torch.bool, device=device)
        m[torch.arange(rows, device=device), torch.arange(rows, device=device) + row_offset] = True
        _OWN[key] = m
    return m


def inbatch_negative_sampling(scores, neg_ratio=None, hard_negative=False, generator=None, row_offset=0, stream=None):
    """``scores`` (B, B), or (B, C) with ``row_offset``: the rows are rows [row_offset, row_offset + B) of a C x C global
    batch whose item embeddings were gathered from all ranks (cross-rank negatives); row i's positive is column
    row_offset + i and its negatives come from the other C - 1 columns."""
    if scores.dim() != 2:
        raise ValueError(f"inbatch_negative_sampling expects 2D scores, got shape {tuple(scores.shape)}")
    return _sample(scores.size(0), scores.size(1), scores.device, scores, neg_ratio, hard_negative, generator, row_offset,
                   stream)


def random_inbatch_negatives(batch_size, n_cols, device, neg_ratio=None, generator=None, row_offset=0, stream=None):
    """The random branch of ``inbatch_negative_sampling`` for a (batch_size, n_cols) score matrix that is never formed
    (ops.inbatch_logits computes only the 1 + K wanted dot products per row): same streams, same indices."""
    return _sample(batch_size, n_cols, device, None, neg_ratio, False, generator, row_offset, stream)


def _sample(batch_size, n_cols, device, scores, neg_ratio, hard_negative, generator, row_offset, stream):
    if n_cols <= 1:
        raise ValueError("In-batch negative sampling requires batch_size > 1")
    if row_offset < 0 or row_offset + batch_size > n_cols:
        raise ValueError(f"rows [{row_offset}, {row_offset + batch_size}) do not fit the {n_cols} score columns")
    max_neg = n_cols - 1
    if neg_ratio is None or neg_ratio <= 0 or neg_ratio > max_neg:
        neg_ratio = max_neg
    own = _own_mask(batch_size, n_cols, row_offset, device) if (hard_negative or n_cols > 65536 or
                                                                 not str(device).startswith("cuda")) else None
    if hard_negative:
        keys = scores.detach().masked_fill(own, float("-inf"))
        return torch.topk(keys, k=neg_ratio, dim=1).indices
    if stream not in (None, "fast", "reference"):
        raise ValueError("stream must be 'fast' or 'reference'")
    if stream == "reference" or not str(device).startswith("cuda"):
        return _reference_stream(batch_size, n_cols, row_offset, neg_ratio, device, generator)
    if n_cols <= 65536:
        # HIP sampler (Floyd's algorithm per row, counter-based RNG): one launch, replayable from a hipGraph
        from .. import ops
        seed = None if generator is None else generator.initial_seed()
        if n_cols == batch_size:
            return ops.inbatch_sample(batch_size, neg_ratio, device, seed)
        return ops.inbatch_sample(batch_size, neg_ratio, device, seed, cols=n_cols, row0=row_offset)
    keys = torch.rand((batch_size, n_cols), device=device, generator=generator).masked_fill(own, -1.0)
    return torch.topk(keys, k=neg_ratio, dim=1).indices  # > 65536 columns: top-k of i.i.d. uniform keys (same set law)


def gather_inbatch_logits(scores, neg_indices, row_offset=0):
    """(B, 1+K) logits: column 0 = scores[i, row_offset + i] (the positive), then scores[i, neg_indices[i, j]]."""
    positive_logits = torch.diagonal(scores, offset=row_offset).reshape(-1, 1)
    negative_logits = torch.gather(scores, 1, neg_indices)
    return torch.cat([positive_logits, negative_logits], dim=1)


class ExactIndex(object):
    """Exact nearest-neighbour search with the surface of the reference's ``Annoy`` engine (torch_rechub/utils/match.py:
    252-296), on the streaming top-K kernel: ``ExactIndex().fit(item_embedding)`` then ``query(v, n)``, so that the
    examples' ``match_evaluation`` runs with one name changed.  ``metric``: "angular" (Annoy's default), "L2" or "IP".
    ``n_trees`` and ``search_k`` are accepted and ignored: there is no approximation to tune."""

    def __init__(self, metric="angular", n_trees=None, search_k=None, device=None):
        from ..serving.hip import _check_metric
        self._metric = _check_metric({"euclidean": "L2", "l2": "L2", "dot": "IP", "ip": "IP"}.get(metric, metric))
        self._device = device
        self._indexer = None

    def fit(self, X):
        """Index the rows of ``X`` (n, d), a numpy array or a tensor."""
        from ..serving.hip import HipIndexer
        self._indexer = HipIndexer(torch.as_tensor(X), self._metric, self._device)
        return self

    def set_query_arguments(self, search_k=None):
        pass

    def query(self, v, n):
        """1-D ``v``: (ids list, distances list) of the ``n`` nearest rows, as ``Annoy.query``.  2-D ``v`` (a batch
        extension): the two (len(v), n) tensors of ``HipIndexer.query``."""
        if self._indexer is None:
            raise RuntimeError("ExactIndex.query before fit")
        v = torch.as_tensor(v)
        if v.dim() == 2:
            return self._indexer.query(v, n)
        if v.dim() != 1:
            raise ValueError("query takes a 1-D vector or a 2-D batch")
        ids, dist = self._indexer.query(v.reshape(1, -1), n)
        keep = ids[0] >= 0  # Annoy returns fewer than n entries when the index holds fewer
        return ids[0][keep].tolist(), dist[0][keep].tolist()

    def __str__(self):
        return f"ExactIndex(metric={self._metric})"
