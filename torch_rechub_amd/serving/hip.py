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

``dtype=torch.float16`` or ``torch.bfloat16`` stores the table in that type T (csrc/topk_half.hip): half the bytes per
item.  The kernel rounds the queries to T and adds exact products in float32, so on data that T holds exactly (small
integers) the answers are the float32 index's.  "IP" searches the rounded table; "L2" takes -|x|^2 from the rounded table
(formed in float64) and rounds the queries to T before doubling them (doubling is exact, so the kernel does not round a
second time) and returns |T(q)|^2 minus the score; "angular" normalises in float32 and then rounds both sides, so its
unit vectors are only approximately unit and its distances approximate (about 2^-11 relative for float16, 2^-8 for
bfloat16).  An index file keeps the stored type.

``quantizer="SQ8"`` stores int8 codes and one float32 scale per row (csrc/topk_q8.hip, ``ops.quantize_rows_int8``): a
quarter of the bytes per item plus 4 bytes per row, and no float copy of the table on the device after the build.  The
queries are quantised by the same rule at query time -- unlike faiss's SQ8, which keeps the query in float -- so both
sides carry up to half a code step of error per coordinate and the answer is approximate: recall@10 against the float32
flat index is 0.978 on unit-Gaussian rows and 0.953 on a Gaussian mixture (profiles/topk_int8_bench.txt, d = 64).
On data the codes hold exactly (integer rows whose largest magnitude is 127) the answers are the float32 index's.  "IP"
searches the codes; "L2" takes -|x^|^2 of the dequantised rows x^ = scale * code (formed in float64), hands the kernel
2 q and returns |q|^2 minus the score, clamped at 0; "angular" normalises in float32 and then quantises, so its rows are
only approximately unit and its distances approximate (by how much has not been measured).  An index file of
a quantised index keeps the codes and the scales (for "angular": of the unit rows) under keys of their own.

``HipIndexer.query`` also takes (n, I, d) queries, one vector per interest of a user (MIND, ComiRec, SINE): every user gets
one list, each item once with its best value over the interests (``ops.topk_items_multi``, csrc/topk_multi.hip) -- the
merged, de-duplicated per-interest lists of the reference's ``match_evaluation``.  Not built for ``quantizer="SQ8"`` nor for
``HipIvfIndexer``: both raise.
"""
import contextlib

import torch

from .base import BaseBuilder, BaseIndexer

METRICS = ("L2", "IP", "angular")


DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def _check_dtype(dtype, table=None):
    """The storage type: ``dtype``, or for None the table's own where that is a half type (an index file keeps its
    type) and float32 otherwise."""
    if dtype is None:
        dtype = table.dtype if table is not None and table.dtype in DTYPES[1:] else torch.float32
    if dtype not in DTYPES:
        raise ValueError(f"dtype must be one of {DTYPES}, got {dtype!r}")
    return dtype


QUANTIZERS = (None, "SQ8")


def _check_quantizer(quantizer, dtype=torch.float32):
    """``quantizer``: None or "SQ8" (int8 codes and a scale per row); it does not combine with a half ``dtype``."""
    if quantizer not in QUANTIZERS:
        raise ValueError(f"quantizer must be one of {QUANTIZERS}, got {quantizer!r}")
    if quantizer is not None and dtype not in (None, torch.float32):
        raise ValueError(f"quantizer={quantizer!r} stores int8 codes and does not combine with dtype={dtype}")
    return quantizer


def _check_codes(codes, scale):
    if codes.dim() != 2 or codes.dtype != torch.int8 or scale.dtype != torch.float32 or tuple(scale.shape) != (codes.shape[0],):
        raise ValueError("a quantised index holds (n, d) int8 codes and (n,) float32 scales")


def _dequantised(codes, scale):
    return codes.float() * scale[:, None]


def _neg_sq_norms_q8(codes, scale, rows=1 << 16):
    """-|x^|^2 of every row x^ = scale * code, formed in float64 (``rows`` rows at a time), float32."""
    out = [-((codes[i:i + rows].double() * scale[i:i + rows].double()[:, None]) ** 2).sum(dim=1).float()
           for i in range(0, codes.shape[0], rows)]
    return torch.cat(out)


def _check_metric(metric):
    if metric not in METRICS:
        raise ValueError(f"metric must be one of {METRICS}, got {metric!r}")
    return metric


def save_index(file_path, metric, table):
    """Write an index file: the metric name and the table (float32, or the half type it is stored in), one
    ``torch.save``."""
    _check_metric(metric)
    if table.dim() != 2:
        raise ValueError("an index holds a 2D (n, d) table")
    torch.save({"metric": metric, "table": table.detach().to("cpu", _check_dtype(None, table)).contiguous()}, file_path)


def load_index(file_path):
    """(metric, table) of an index file (loaded with ``weights_only=True``)."""
    blob = torch.load(file_path, map_location="cpu", weights_only=True)
    if not isinstance(blob, dict) or set(blob) != {"metric", "table"}:
        raise ValueError(f"{file_path} is not an index file of torch_rechub_amd.serving")
    return _check_metric(blob["metric"]), blob["table"]


def _unit_rows(x):
    n = x.norm(dim=1, keepdim=True)
    return torch.where(n > 0, x / n.clamp_min(torch.finfo(torch.float32).tiny), torch.zeros_like(x))


def _neg_sq_norms(table):
    """-|x|^2 of every row, float32; of a half table: formed in float64 from the stored values."""
    if table.dtype == torch.float32:
        return -(table * table).sum(dim=1)
    return -(table.double() ** 2).sum(dim=1).float()


def _metric_query(metric, dev, embeddings, exclude, bias, search, dtype=torch.float32):
    """``query`` of both indexers: ``search(q, bias, exclude) -> (ids, scores)`` is the inner-product search on the device
    ``dev``, given the queries as the metric has them ranked (2 q with the index's ``bias`` = -|x|^2 for "L2", unit rows
    for "angular"); the scores become the metric's values and everything returns to the queries' device.  ``dtype``: the
    table's type; for a half type "L2" rounds the queries to it first, so that 2 q is a value the kernel keeps."""
    if embeddings.dim() != 2:
        raise ValueError("query takes a 2D (n, d) tensor")
    q = embeddings.detach().to(dev, torch.float32)
    if exclude is not None:
        exclude = exclude.to(dev)
    if metric == "L2":
        if dtype != torch.float32:
            q = q.to(dtype).float()
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


def _metric_query_multi(metric, dev, embeddings, exclude, bias, search, dtype=torch.float32):
    """``_metric_query`` for (n, I, d) embeddings, one vector per interest of a user: ``search(q, qbias, bias, exclude) ->
    (ids, scores)`` is ``ops.topk_items_multi``, max_i (q_i . x + qbias_i) + bias per user.  "IP": q as given; "L2": 2 q_i
    with qbias = -|q_i|^2 and the index's bias = -|x|^2, so the value max(-score, 0) is the smallest squared distance over
    the interests; "angular": unit rows per interest.  A row holding a nan is an absent interest: it is zeroed and its
    qbias is -inf.  qbias is always handed over (zeros for "IP" and "angular"), so that no host synchronisation has to ask
    whether an interest is absent; adding 0 changes no value."""
    q = embeddings.detach().to(dev, torch.float32)
    if exclude is not None:
        exclude = exclude.to(dev)
    absent = torch.isnan(q).any(dim=2)
    q = q.masked_fill(absent.unsqueeze(2), 0.0)
    qbias = torch.zeros(q.shape[:2], dtype=torch.float32, device=dev)
    if metric == "L2":
        if dtype != torch.float32:
            q = q.to(dtype).float()
        qbias = -(q * q).sum(dim=2)
        q = q * 2.0
    elif metric == "angular":
        q, bias = _unit_rows(q.reshape(-1, q.shape[2])).reshape(q.shape), None
    else:
        bias = None
    ids, s = search(q, qbias.masked_fill(absent, float("-inf")), bias, exclude)
    if metric == "L2":
        val = (-s).clamp_min(0.0)
    elif metric == "angular":
        val = (2.0 - 2.0 * s).clamp_min(0.0).sqrt()
    else:
        val = s
    if metric != "IP":
        val = torch.where(ids < 0, torch.full_like(val, float("inf")), val)
    return ids.to(embeddings.device), val.to(embeddings.device)


class HipIndexer(BaseIndexer):
    """``table`` (n, d) on the device, searched exactly.  ``dtype``: the type it is stored and searched in (float32,
    float16 or bfloat16; None: a half table keeps its type, anything else becomes float32).  ``quantizer="SQ8"``: int8
    codes and a scale per row instead (``table`` float: quantised here -- for "angular" its unit rows; ``table`` int8 with
    ``scale`` (n,): the codes of an index file, taken as they are); ``_table`` and ``_search`` are then the codes."""

    quantizer = None

    def __init__(self, table, metric="L2", device=None, dtype=None, quantizer=None, scale=None):
        from .. import ops
        self.metric = _check_metric(metric)
        if table.dim() != 2:
            raise ValueError("an index holds a 2D (n, d) table")
        self.quantizer = _check_quantizer(quantizer, dtype)
        device = torch.device("cuda" if device is None else device)
        self._ops = ops
        self._bias = None
        if quantizer is not None:
            self.dtype = torch.float32
            if scale is None:
                x = table.detach().to(device, torch.float32).contiguous()
                ops.require_hip(x)
                table, scale = ops.quantize_rows_int8(_unit_rows(x) if metric == "angular" else x)
                del x
            _check_codes(table, scale)
            self._table = self._search = table.detach().to(device).contiguous()
            self._scale = scale.detach().to(device).contiguous()
            ops.require_hip(self._table)
            if metric == "L2":
                self._bias = _neg_sq_norms_q8(self._table, self._scale)
            return
        self.dtype = _check_dtype(dtype, table)
        self._table = table.detach().to(device, self.dtype).contiguous()
        ops.require_hip(self._table)
        self._search = self._table
        if metric == "L2":
            self._bias = _neg_sq_norms(self._table)
        elif metric == "angular":
            self._search = _unit_rows(self._table.float()).to(self.dtype)

    def __len__(self):
        return int(self._table.shape[0])

    def query(self, embeddings, top_k, *, exclude=None):
        """(ids (n, top_k) int64, values (n, top_k) float32) on the queries' device, best first.  ``exclude`` (n, S) int64:
        per-query ids that are never returned (entries outside [0, len(index)) are padding).  3-D ``embeddings`` (n, I, d),
        one vector per interest of a user (MIND, ComiRec, SINE): one merged list per user, every item once with its best
        value over the interests (``ops.topk_items_multi``); a row of nan is an absent interest."""
        if embeddings.dim() == 3:
            if self.quantizer is not None:
                raise ValueError(f"multi-interest (n, I, d) queries over a quantizer={self.quantizer!r} index are not built; "
                                 "use a float32, float16 or bfloat16 index")

            def search_multi(q, qbias, bias, exclude):
                return self._ops.topk_items_multi(q, self._search, top_k, qbias=qbias, bias=bias, exclude=exclude)

            return _metric_query_multi(self.metric, self._table.device, embeddings, exclude, self._bias, search_multi,
                                       self.dtype)

        def search(q, bias, exclude):
            if self.quantizer is not None:
                return self._ops.topk_items_int8(q, self._search, self._scale, top_k, bias=bias, exclude=exclude)
            return self._ops.topk_items(q, self._search, top_k, bias=bias, exclude=exclude)

        return _metric_query(self.metric, self._table.device, embeddings, exclude, self._bias, search, self.dtype)

    def save(self, file_path):
        if self.quantizer is not None:
            torch.save({"metric": self.metric, "quantizer": self.quantizer, "codes": self._table.cpu(),
                        "scale": self._scale.cpu()}, file_path)
        else:
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
    is exact and means what ``HipIndexer`` returns; with ``nprobe == nlists`` it is ``HipIndexer``'s answer bit for bit.
    ``dtype`` as ``HipIndexer``'s: only the table is stored in it; the rows are assigned to their lists from the stored
    (rounded) values, through a float32 copy that is dropped again, and the centroids and the choice of the probed lists
    stay float32.  ``quantizer`` and ``scale`` as ``HipIndexer``'s: the rows are assigned from the dequantised values
    scale * code (a float32 copy that is dropped again), and only the grouped codes and scales stay (``_table`` is
    ``_search``; ``save`` puts the rows back in their original order)."""

    quantizer = None

    def __init__(self, table, centroids, metric="L2", device=None, nprobe=1, dtype=None, quantizer=None, scale=None):
        from .. import ops
        self.metric = _check_metric(metric)
        if table.dim() != 2 or centroids.dim() != 2 or centroids.shape[1] != table.shape[1]:
            raise ValueError("an IVF index holds a 2D (n, d) table and (nlists, d) centroids")
        self.quantizer = _check_quantizer(quantizer, dtype)
        self.dtype = torch.float32 if quantizer is not None else _check_dtype(dtype, table)
        device = torch.device("cuda" if device is None else device)
        self._ops = ops
        if quantizer is not None:
            if scale is None:
                x = table.detach().to(device, torch.float32).contiguous()
                ops.require_hip(x)
                table, scale = ops.quantize_rows_int8(_unit_rows(x) if metric == "angular" else x)
                del x
            _check_codes(table, scale)
            self._table, scale = table.detach().to(device).contiguous(), scale.detach().to(device).contiguous()
        else:
            self._table = table.detach().to(device, self.dtype).contiguous()
        ops.require_hip(self._table)
        self.centroids = centroids.detach().to(device, torch.float32).contiguous()
        self.nlists = int(self.centroids.shape[0])
        if not 1 <= self.nlists <= len(self):
            raise ValueError(f"nlists={self.nlists} must lie in [1, {len(self)}] (the number of rows)")
        self.nprobe = self._clip(nprobe)
        self._cbias = -(self.centroids * self.centroids).sum(dim=1)
        if quantizer is not None:
            bias = _neg_sq_norms_q8(self._table, scale) if metric == "L2" else None
            order, self._list_off = _group(_assign(_dequantised(self._table, scale), self.centroids, ops), self.nlists)
            self._row_id = order.to(torch.int32)
            self._table = self._search = self._table[order].contiguous()
            self._scale = scale[order].contiguous()
            self._bias = None if bias is None else bias[order].contiguous()
            return
        search, bias = self._table.float(), None
        if metric == "L2":
            bias = _neg_sq_norms(self._table)
        elif metric == "angular":
            search = _unit_rows(search).to(self.dtype).float()
        order, self._list_off = _group(_assign(search, self.centroids, ops), self.nlists)
        self._row_id = order.to(torch.int32)
        self._search = search[order].to(self.dtype).contiguous()
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
        if embeddings.dim() == 3:
            raise ValueError("multi-interest (n, I, d) queries over an IVF index are not built; use index_type=\"Flat\"")
        nprobe = self.nprobe if nprobe is None else self._clip(nprobe)
        ops = self._ops

        def search(q, bias, exclude):
            # the nearest lists under L2: by 2 q . c - |c|^2 ("L2" hands 2 q in already); under "IP": by q . c
            if self.metric == "IP":
                probe = ops.topk_items(q, self.centroids, nprobe)[0]
            else:
                q2 = q if self.metric == "L2" else q * 2.0
                probe = ops.topk_items(q2, self.centroids, nprobe, bias=self._cbias)[0]
            if self.quantizer is not None:
                return ops.ivf_scan_int8(q, self._search, self._scale, self._row_id, self._list_off, probe.to(torch.int32),
                                         top_k, bias=bias, exclude=exclude)
            return ops.ivf_scan(q, self._search, self._row_id, self._list_off, probe.to(torch.int32), top_k, bias=bias,
                                exclude=exclude, dtype=self.dtype)

        return _metric_query(self.metric, self._table.device, embeddings, exclude, self._bias, search, self.dtype)

    def save(self, file_path):
        """One ``torch.save`` dict: the metric, the table in its original row order, the centroids and ``nprobe``.
        Loading assigns the rows to the stored centroids again, which gives the same lists.  A quantised index keeps
        "quantizer", "codes" and "scale" in place of "table"."""
        blob = {"metric": self.metric, "index_type": "IVF", "centroids": self.centroids.cpu(), "nprobe": self.nprobe}
        if self.quantizer is not None:
            back = torch.empty_like(self._row_id, dtype=torch.int64)
            back[self._row_id.long()] = torch.arange(len(self), device=back.device)
            blob.update(quantizer=self.quantizer, codes=self._table[back].cpu(), scale=self._scale[back].cpu())
        else:
            blob["table"] = self._table.cpu()
        torch.save(blob, file_path)


_IVF_KEYS = {"metric", "table", "index_type", "centroids", "nprobe"}
_Q8_KEYS = {"metric", "quantizer", "codes", "scale"}
_IVF_Q8_KEYS = _Q8_KEYS | {"index_type", "centroids", "nprobe"}


class HipBuilder(BaseBuilder):
    """Builder of ``HipIndexer`` (``index_type="Flat"``, exact) and ``HipIvfIndexer`` (``"IVF"``).  ``metric``: "L2" (the
    default, as the reference's FaissBuilder), "IP" or "angular"; ``device``: where the table lives (default: the current
    HIP device).  For "IVF", as the reference's FaissBuilder: ``nlists`` lists, of which a query scans ``nprobe`` (None:
    1, as faiss; clipped to ``nlists``).  The centroids come from ``niter`` rounds of k-means on the device, started from
    ``nlists`` distinct rows drawn by ``torch.Generator(seed)`` or from ``centroids`` (nlists, d); ``niter=0`` with
    ``centroids`` uses them as they are.  k-means minimises L2 for every metric ("angular": between the unit rows).
    ``dtype``: the type the table is stored and searched in, float32, float16 or bfloat16 (see the module's head; k-means
    always trains on the float32 embeddings).  ``quantizer``: None, or "SQ8" for int8 codes with one scale per row (a
    quarter of the bytes; approximate, see the module's head; not together with a half ``dtype``).  An index file carries
    its own metric, its own type, its own dtype and its own quantizer."""

    def __init__(self, metric="L2", device=None, *, index_type="Flat", nlists=100, nprobe=None, niter=10, seed=2022,
                 centroids=None, dtype=torch.float32, quantizer=None):
        self.metric = _check_metric(metric)
        self.dtype = _check_dtype(dtype)
        self.quantizer = _check_quantizer(quantizer, self.dtype)
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
        return HipIvfIndexer(table, train_centroids(x, start, self.niter, ops), self.metric, device, self.nprobe,
                             self.dtype, self.quantizer)

    @contextlib.contextmanager
    def from_embeddings(self, embeddings):
        if self.index_type == "IVF":
            yield self._ivf(embeddings)
        else:
            yield HipIndexer(embeddings, self.metric, self.device, self.dtype, self.quantizer)

    @contextlib.contextmanager
    def from_index_file(self, index_file):
        blob = torch.load(index_file, map_location="cpu", weights_only=True)
        if isinstance(blob, dict) and set(blob) == _IVF_Q8_KEYS and blob["index_type"] == "IVF":
            yield HipIvfIndexer(blob["codes"], blob["centroids"], _check_metric(blob["metric"]), self.device,
                                blob["nprobe"], None, _check_quantizer(blob["quantizer"]), blob["scale"])
        elif isinstance(blob, dict) and set(blob) == _Q8_KEYS:
            yield HipIndexer(blob["codes"], _check_metric(blob["metric"]), self.device, None,
                             _check_quantizer(blob["quantizer"]), blob["scale"])
        elif isinstance(blob, dict) and set(blob) == _IVF_KEYS and blob["index_type"] == "IVF":
            yield HipIvfIndexer(blob["table"], blob["centroids"], _check_metric(blob["metric"]), self.device,
                                blob["nprobe"])
        else:
            metric, table = load_index(index_file)
            yield HipIndexer(table, metric, self.device)
