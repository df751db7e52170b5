"""The exact index: brute force over the whole table on the streaming top-K kernel (``ops.topk_items``, csrc/topk.hip).

Every metric is an inner-product search with a per-item bias, so one kernel serves the three of them:
  "IP"       value = q . x, descending;
  "L2"       value = the squared distance |q|^2 - (2 q . x - |x|^2), ascending (as faiss returns it), clamped at 0; the
             kernel ranks 2 q . x - |x|^2 with -|x|^2 as its bias;
  "angular"  value = sqrt(max(0, 2 - 2 cos)), ascending (Annoy's distance); the table rows are normalised once at build,
             the queries at query time; a zero vector has cos 0 with everything.
A query with fewer than ``top_k`` candidates gets id -1 and value +inf (-inf for "IP") in the tail.
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
        if embeddings.dim() != 2:
            raise ValueError("query takes a 2D (n, d) tensor")
        out_dev = embeddings.device
        dev = self._table.device
        q = embeddings.detach().to(dev, torch.float32)
        if exclude is not None:
            exclude = exclude.to(dev)
        if self.metric == "L2":
            qn = (q * q).sum(dim=1, keepdim=True)
            ids, s = self._ops.topk_items(q * 2.0, self._search, top_k, bias=self._bias, exclude=exclude)
            val = (qn - s).clamp_min(0.0)
        elif self.metric == "angular":
            ids, s = self._ops.topk_items(_unit_rows(q), self._search, top_k, exclude=exclude)
            val = (2.0 - 2.0 * s).clamp_min(0.0).sqrt()
        else:
            ids, val = self._ops.topk_items(q, self._search, top_k, exclude=exclude)
        if self.metric != "IP":
            val = torch.where(ids < 0, torch.full_like(val, float("inf")), val)
        return ids.to(out_dev), val.to(out_dev)

    def save(self, file_path):
        save_index(file_path, self.metric, self._table)


class HipBuilder(BaseBuilder):
    """Builder of ``HipIndexer``.  ``metric``: "L2" (the default, as the reference's FaissBuilder), "IP" or "angular";
    ``device``: where the table lives (default: the current HIP device).  An index file carries its own metric."""

    def __init__(self, metric="L2", device=None):
        self.metric = _check_metric(metric)
        self.device = device

    @contextlib.contextmanager
    def from_embeddings(self, embeddings):
        yield HipIndexer(embeddings, self.metric, self.device)

    @contextlib.contextmanager
    def from_index_file(self, index_file):
        metric, table = load_index(index_file)
        yield HipIndexer(table, metric, self.device)
