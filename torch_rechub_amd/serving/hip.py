"""The exact index: brute force over the whole table on the streaming top-K kernel (``ops.topk_items``, csrc/topk.hip).

Every metric is an inner-product search with a per-item bias, so one kernel serves the three of them:
  "IP"       value = q . x, descending;
  "L2"       value = the squared distance |q|^2 - (2 q . x - |x|^2), ascending (as faiss returns it), clamped at 0; the
             kernel ranks 2 q . x - |x|^2 with -|x|^2 as its bias;
  "angular"  value = sqrt(max(0, 2 - 2 cos)), ascending (Annoy's distance); the table rows are normalised once at build,
             the queries at query time; a zero vector has cos 0 with everything.
A query with fewer than ``top_k`` candidates gets id -1 and value +inf (-inf for "IP") in the tail.

``HipIvfIndexer`` is the inverted-file index over the same three metrics (``HipBuilder(index_type="IVF")``): k-means
centroids trained on the device, every row in the list of its nearest centroid, a query scanning only its ``nprobe``
nearest lists on ``ops.ivf_scan`` (csrc/ivf.hip) -- approximate only in which rows it looks at.
"""
import contextlib

import torch

from .base import BaseBuilder, BaseIndexer

METRICS = ("L2", "IP", "angular")


def _check_metric(metric):
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    return metric


def save_index(file_path, metric, table):
    """Write an index file: the metric name and the float32 table, one ``torch.save``."""
    _check_metric(metric)
    if table.dim() != 2:
        raise ValueError("an index holds a 2D (n, d) table")
    torch.save({"metric": metric, "table": table.detach().to("cpu", torch.float32).contiguous()}, file_path)


def load_index(file_path):
    """(metric, table) of an index file (loaded with ``weights_only=True``)."""
    blob = torch.load(file_path, map_location="cpu", weights_only=True)
    if not isinstance(blob, dict) or set(blob) != {"metric", "table"}:
        raise ValueError(f"{file_path} is not an index file of torch_rechub_amd.serving")
    return _check_metric(blob["metric"]), blob["table"]


def _unit_rows(x):
    n = x.norm(dim=1, keepdim=True)
    return torch.where(n > 0, x / n.clamp_min(torch.finfo(torch.float32).tiny), torch.zeros_like(x))


def _metric_query(metric, dev, embeddings, exclude, bias, search):
    """``query`` of both indexers: ``search(q, bias, exclude) -> (ids, scores)`` is the inner-product search on the device
    ``dev``, given the queries as the metric has them ranked (2 q with the index's ``bias`` = -|x|^2 for "L2", unit rows
    for "angular"); the scores become the metric's values and everything returns to the queries' device."""
    if embeddings.dim() != 2:
        raise ValueError("query takes a 2D (n, d) tensor")
    q = embeddings.detach().to(dev, torch.float32)
    if exclude is not None:
        exclude = exclude.to(dev)
    if metric == "L2":
        qn = (q * q).sum(dim=1, keepdim=True)
        ids, s = search(q * 2.0, bias, exclude)
        val = (qn - s).clamp_min(0.0)
    elif metric == "angular":
        ids, s = search(_unit_rows(q), None, exclude)
        val = (2.0 - 2.0 * s).clamp_min(0.0).sqrt()
    else:
        ids, val = search(q, None, exclude)
    if metric != "IP":
        val = torch.where(ids < 0, torch.full_like(val, float("inf")), val)
    return ids.to(embeddings.device), val.to(embeddings.device)


class HipIndexer(BaseIndexer):
    """``table`` (n, d) on the device, searched exactly."""

    def __init__(self, table, metric="L2", device=None):
        from .. import ops
        self.metric = _check_metric(metric)
        if table.dim() != 2:
            raise ValueError("an index holds a 2D (n, d) table")
        device = torch.device("cuda" if device is None else device)
        self._ops = ops
        self._table = table.detach().to(device, torch.float32).contiguous()
        ops.require_hip(self._table)
        self._bias = None
        self._search = self._table
        if metric == "L2":
            self._bias = -(self._table * self._table).sum(dim=1)
        elif metric == "angular":
            self._search = _unit_rows(self._table)

    def __len__(self):
        return int(self._table.shape[0])

    def query(self, embeddings, top_k, *, exclude=None):
        """(ids (n, top_k) int64, values (n, top_k) float32) on the queries' device, best first.  ``exclude`` (n, S) int64:
        per-query ids that are never returned (entries outside [0, len(index)) are padding)."""
        def search(q, bias, exclude):
            return self._ops.topk_items(q, self._search, top_k, bias=bias, exclude=exclude)

        return _metric_query(self.metric, self._table.device, embeddings, exclude, self._bias, search)

    def save(self, file_path):
        save_index(file_path, self.metric, self._table)


INDEX_TYPES = ("Flat", "IVF")


def _assign(x, centroids, ops):
    """(n,) int64: the nearest centroid of every row under L2, ties to the lower list: argmax of 2 x . c - |c|^2."""
    bias = -(centroids * centroids).sum(dim=1)
    return ops.topk_items(x * 2.0, centroids, 1, bias=bias)[0][:, 0]


def _group(assign, nlists):
    """(order (n,) int64, list_off (nlists + 1,) int32): the rows in list order -- a stable sort, so ids ascend inside a
    list -- and the lists' offsets."""
    key, order = torch.sort(assign, stable=True)
    bounds = torch.arange(nlists + 1, dtype=key.dtype, device=key.device)
    return order, torch.searchsorted(key, bounds, out_int32=True)


def train_centroids(x, centroids, niter, ops):
    """``niter`` rounds of Lloyd's k-means on the device: assign every row to its nearest centroid, then every centroid
    becomes the mean of its rows (``ops.ivf_list_mean``; a centroid that lost all its rows stays where it was)."""
    for _ in range(niter):
        order, list_off = _group(_assign(x, centroids, ops), centroids.shape[0])
        centroids = ops.ivf_list_mean(x[order], list_off, centroids)
    return centroids


class HipIvfIndexer(BaseIndexer):
    """``table`` (n, d) on the device behind an inverted file: every row belongs to the list of its nearest centroid
    (L2; for "angular" between unit vectors), a query scans the ``nprobe`` lists whose centroids are nearest to it (for
    "IP": whose centroids have the largest inner product with it) on ``ops.ivf_scan``.  Among the probed rows the answer
    is exact and means what ``HipIndexer`` returns; with ``nprobe == nlists`` it is ``HipIndexer``'s answer bit for bit."""

    def __init__(self, table, centroids, metric="L2", device=None, nprobe=1):
        from .. import ops
        self.metric = _check_metric(metric)
        if table.dim() != 2 or centroids.dim() != 2 or centroids.shape[1] != table.shape[1]:
            raise ValueError("an IVF index holds a 2D (n, d) table and (nlists, d) centroids")
        device = torch.device("cuda" if device is None else device)
        self._ops = ops
        self._table = table.detach().to(device, torch.float32).contiguous()
        ops.require_hip(self._table)
        self.centroids = centroids.detach().to(device, torch.float32).contiguous()
        self.nlists = int(self.centroids.shape[0])
        if not 1 <= self.nlists <= len(self):
            raise ValueError(f"nlists={self.nlists} must lie in [1, {len(self)}] (the number of rows)")
        self.nprobe = self._clip(nprobe)
        self._cbias = -(self.centroids * self.centroids).sum(dim=1)
        search, bias = self._table, None
        if metric == "L2":
            bias = -(self._table * self._table).sum(dim=1)
        elif metric == "angular":
            search = _unit_rows(self._table)
        order, self._list_off = _group(_assign(search, self.centroids, ops), self.nlists)
        self._row_id = order.to(torch.int32)
        self._search = search[order].contiguous()
        self._bias = None if bias is None else bias[order].contiguous()

    def _clip(self, nprobe):
        nprobe = 1 if nprobe is None else int(nprobe)
        if nprobe < 1:
            raise ValueError(f"nprobe={nprobe} must be at least 1")
        return min(nprobe, self.nlists)

    def __len__(self):
        return int(self._table.shape[0])

    def list_sizes(self):
        """(nlists,) int64: the rows of every list."""
        return (self._list_off[1:] - self._list_off[:-1]).to(torch.int64)

    def lists(self):
        """(row_id (n,) int32 = the original ids in list order, list_off (nlists + 1,) int32)."""
        return self._row_id, self._list_off

    def query(self, embeddings, top_k, *, exclude=None, nprobe=None):
        """As ``HipIndexer.query``, over the ``nprobe`` (default: the index's) nearest lists of every query."""
        nprobe = self.nprobe if nprobe is None else self._clip(nprobe)
        ops = self._ops

        def search(q, bias, exclude):
            # the nearest lists under L2: by 2 q . c - |c|^2 ("L2" hands 2 q in already); under "IP": by q . c
            if self.metric == "IP":
                probe = ops.topk_items(q, self.centroids, nprobe)[0]
            else:
                q2 = q if self.metric == "L2" else q * 2.0
                probe = ops.topk_items(q2, self.centroids, nprobe, bias=self._cbias)[0]
            return ops.ivf_scan(q, self._search, self._row_id, self._list_off, probe.to(torch.int32), top_k, bias=bias,
                                exclude=exclude)

        return _metric_query(self.metric, self._table.device, embeddings, exclude, self._bias, search)

    def save(self, file_path):
        """One ``torch.save`` dict: the metric, the table in its original row order, the centroids and ``nprobe``.
        Loading assigns the rows to the stored centroids again, which gives the same lists."""
        torch.save({"metric": self.metric, "table": self._table.cpu(), "index_type": "IVF",
                    "centroids": self.centroids.cpu(), "nprobe": self.nprobe}, file_path)


_IVF_KEYS = {"metric", "table", "index_type", "centroids", "nprobe"}


class HipBuilder(BaseBuilder):
    """Builder of ``HipIndexer`` (``index_type="Flat"``, exact) and ``HipIvfIndexer`` (``"IVF"``).  ``metric``: "L2" (the
    default, as the reference's FaissBuilder), "IP" or "angular"; ``device``: where the table lives (default: the current
    HIP device).  For "IVF", as the reference's FaissBuilder: ``nlists`` lists, of which a query scans ``nprobe`` (None:
    1, as faiss; clipped to ``nlists``).  The centroids come from ``niter`` rounds of k-means on the device, started from
    ``nlists`` distinct rows drawn by ``torch.Generator(seed)`` or from ``centroids`` (nlists, d); ``niter=0`` with
    ``centroids`` uses them as they are.  k-means minimises L2 for every metric ("angular": between the unit rows).
    An index file carries its own metric and its own type."""

    def __init__(self, metric="L2", device=None, *, index_type="Flat", nlists=100, nprobe=None, niter=10, seed=2022,
                 centroids=None):
        self.metric = _check_metric(metric)
        self.device = device
        if index_type == "HNSW":
            raise NotImplementedError('index_type "HNSW" (graph search) is not built here; use "Flat" or "IVF"')
        if index_type not in INDEX_TYPES:
            raise ValueError(f"index_type must be one of {INDEX_TYPES}, got {index_type!r}")
        self.index_type = index_type
        self.nlists = int(nlists)
        self.nprobe = 1 if nprobe is None else int(nprobe)
        self.niter = int(niter)
        self.seed = int(seed)
        self.centroids = centroids
        if index_type == "IVF":
            if self.nprobe < 1 or self.niter < 0:
                raise ValueError(f"nprobe={nprobe} must be at least 1 and niter={niter} at least 0")
            self.nprobe = min(self.nprobe, max(self.nlists, 1))
            if centroids is not None and (centroids.dim() != 2 or centroids.shape[0] != self.nlists):
                raise ValueError(f"centroids must be a (nlists={self.nlists}, d) tensor")

    def _ivf(self, embeddings):
        from .. import ops
        if embeddings.dim() != 2:
            raise ValueError("an index holds a 2D (n, d) table")
        n = int(embeddings.shape[0])
        if not 1 <= self.nlists <= n:
            raise ValueError(f"nlists={self.nlists} must lie in [1, {n}] (the number of rows)")
        device = torch.device("cuda" if self.device is None else self.device)
        table = embeddings.detach().to(device, torch.float32).contiguous()
        ops.require_hip(table)
        x = _unit_rows(table) if self.metric == "angular" else table
        if self.centroids is not None:
            if self.centroids.shape[1] != table.shape[1]:
                raise ValueError(f"centroids must be a (nlists={self.nlists}, d={int(table.shape[1])}) tensor")
            start = self.centroids.detach().to(device, torch.float32).contiguous()
        else:
            perm = torch.randperm(n, generator=torch.Generator().manual_seed(self.seed))[:self.nlists]
            start = x[perm.to(device)].contiguous()
        return HipIvfIndexer(table, train_centroids(x, start, self.niter, ops), self.metric, device, self.nprobe)

    @contextlib.contextmanager
    def from_embeddings(self, embeddings):
        if self.index_type == "IVF":
            yield self._ivf(embeddings)
        else:
            yield HipIndexer(embeddings, self.metric, self.device)

    @contextlib.contextmanager
    def from_index_file(self, index_file):
        blob = torch.load(index_file, map_location="cpu", weights_only=True)
        if isinstance(blob, dict) and set(blob) == _IVF_KEYS and blob["index_type"] == "IVF":
            yield HipIvfIndexer(blob["table"], blob["centroids"], _check_metric(blob["metric"]), self.device,
                                blob["nprobe"])
        else:
            metric, table = load_index(index_file)
            yield HipIndexer(table, metric, self.device)
