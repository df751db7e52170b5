"""ops.topk_items_multi (csrc/topk_multi.hip), HipIndexer.query and ExactIndex.query with (n, I, d) queries against a
float64 reference: max_i (q_ui . x_j + qbias_ui) + bias_j per user, ranked by (score descending, id ascending).  All data
are small integers (entries in [-4, 4], integer biases), which fp16 and bf16 hold too: every product and sum is exact in
fp32, so ids AND scores are compared bit for bit, with no tolerance."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
F32, F16, BF16 = torch.float32, torch.float16, torch.bfloat16
NINF = -np.inf


def t(a, dtype=None):
    return None if a is None else torch.as_tensor(a, dtype=dtype).to("cuda:0")


def ref(q, x, k, qbias=None, bias=None, exclude=None, invalid=()):
    s = np.einsum("uid,jd->uij", q.astype(np.float64), x.astype(np.float64))
    s = (s if qbias is None else s + qbias[:, :, None]).max(axis=1)
    s = s if bias is None else s + bias
    ok = np.ones(s.shape, dtype=bool)
    ok[:, [i for i in invalid if 0 <= i < len(x)]] = False
    for u in range(len(q)):
        ok[u, [i for i in ([] if exclude is None else exclude[u]) if 0 <= i < len(x)]] = False
        ok[u] &= qbias is None or not np.isneginf(qbias[u]).all()  # a user without any interest has no candidates
    ids, sc = np.full((len(q), k), -1, dtype=np.int64), np.full((len(q), k), NINF)
    for u in range(len(q)):
        cand = np.nonzero(ok[u])[0]
        order = cand[np.lexsort((cand, -s[u, cand]))][:k]
        ids[u, :len(order)], sc[u, :len(order)] = order, s[u, order]
    return ids, sc


def ints(seed, M, I, D, V):
    rng = np.random.default_rng(seed)
    draw = lambda lim, *shape: rng.integers(-lim, lim + 1, size=shape).astype(np.float32)
    return draw(4, M, I, D), draw(4, V, D), draw(6, M, I), draw(5, V)


def run(q, x, k, T=F32, **kw):
    from torch_rechub_amd import ops
    q = q if torch.is_tensor(q) else t(q)
    kw = {n: (v if n in ("invalid", "nsplit") else t(v, torch.int64 if n == "exclude" else None)) for n, v in kw.items()}
    ids, sc = ops.topk_items_multi(q, t(x).to(T), k, **kw)
    torch.cuda.synchronize()
    assert ids.dtype == torch.int64 and sc.dtype == torch.float32 and ids.shape == sc.shape == (q.shape[0], k)
    return ids.cpu().numpy(), sc.cpu().numpy().astype(np.float64)


def same(got, exp, what=""):
    np.testing.assert_array_equal(got[0], exp[0], err_msg=f"{what} ids")
    np.testing.assert_array_equal(got[1], exp[1], err_msg=f"{what} scores")


# I (every Ip, padded slots, the cross-lane fold at 8, the two-group fold at 16), V (below a tile, ragged tails, V < K),
# D (two k chunks with an odd tail), K (list chunks; above 128 the users per workgroup are capped), table type, nsplit;
# M is one more than the users of a workgroup: a ragged second tile
CASES = [(1, 193, 65, 64, F32, 1), (1, 65, 130, 256, F16, 2), (1, 63, 63, 129, BF16, 1), (2, 193, 63, 129, F32, 3),
         (2, 63, 1, 1, BF16, 1), (2, 65, 130, 64, BF16, 2), (3, 193, 130, 65, F32, 2), (3, 65, 63, 256, F16, 1),
         (4, 193, 65, 256, F32, 3), (4, 1, 1, 64, BF16, 1), (4, 63, 130, 1, F16, 1), (4, 193, 130, 129, F16, 3),
         (5, 193, 63, 64, F32, 2), (5, 65, 65, 129, BF16, 1), (8, 193, 130, 256, F32, 3), (8, 63, 65, 65, F16, 1),
         (8, 1, 63, 1, F32, 1), (16, 193, 65, 129, F32, 2), (16, 65, 130, 64, BF16, 1), (16, 193, 1, 256, F16, 3)]


@pytest.mark.parametrize("I,V,D,K,T,nsplit", CASES)
def test_kernel_matches_float64_bit_for_bit(I, V, D, K, T, nsplit):
    Ip = 1 << (I - 1).bit_length()
    M = min(64 // Ip, 64 if K <= 128 else 32) + 1
    q, x, qbias, bias = ints(I + V + D + K, M, I, D, V)
    same(run(q, x, K, T, qbias=qbias, bias=bias, nsplit=nsplit), ref(q, x, K, qbias, bias))
    same(run(q, x, K, T, nsplit=nsplit), ref(q, x, K), "without biases")


def rule_case(name):
    """M = 9 users of I = 3 interests over V = 193 items (four tiles), K = 70, and what the named rule changes."""
    M, I, D, V, K = 9, 3, 20, 193, 70
    q, x, qbias, bias = ints(7, M, I, D, V)
    kw = dict(qbias=qbias, bias=bias)
    if name == "duplicate rows":  # equal scores on different ids, inside a tile and across tiles
        x = x[np.arange(V) % 7]
    elif name == "one item under two interests":  # equal scores for user 0, unequal for user 1: once, the larger one
        q[0, 1], q[1, 1], kw = q[0, 0], 2 * q[1, 0], {}
    elif name == "absent interests":
        qbias[0, 1] = qbias[1, :2] = qbias[2, :] = qbias[8, :] = NINF
    elif name == "bias with -inf":
        bias[::3] = NINF
    elif name == "exclude and invalid":
        top = ref(q, x, K, qbias, bias)[0]
        exclude = np.random.default_rng(1).integers(-1, V, size=(M, 5))
        exclude[:, 0], exclude[:, 4] = top[:, 0], -1
        kw.update(exclude=exclude, invalid=[int(top[0, 1]), 64, V - 1, V + 5])
    return q, x, K, kw


@pytest.mark.parametrize("T", [F32, F16])
@pytest.mark.parametrize("name", ["duplicate rows", "one item under two interests", "absent interests", "bias with -inf",
                                  "exclude and invalid", "strided q"])
def test_rules(name, T):
    q, x, K, kw = rule_case(name)
    exp = ref(q, x, K, **kw)
    dev_q = t(q)
    if name == "strided q":
        dev_q = torch.zeros((*q.shape[:2], q.shape[2] + 4), device="cuda:0")[:, :, :q.shape[2]].copy_(t(q))
        assert not dev_q.is_contiguous()
    first = run(dev_q, x, K, T, **kw)
    same(first, exp)
    for nsplit in (1, 3, len(x)):  # every split, and a second run, give the same bits
        same(run(dev_q, x, K, T, nsplit=nsplit, **kw), first, f"nsplit {nsplit}")


@pytest.mark.parametrize("I,T", [(1, F32), (3, F32), (4, BF16), (8, F16), (16, F32)])
def test_gaussian_data_equal_the_merge_of_the_flat_scan(I, T):
    from torch_rechub_amd import ops
    M, D, V, K = 11, 72, 4097, 50
    g = torch.Generator().manual_seed(I)
    q, x = torch.randn(M, I, D, generator=g).cuda(), torch.randn(V, D, generator=g).cuda().to(T)
    ids, sc = (a.cpu().numpy() for a in ops.topk_items_multi(q, x, K, nsplit=3))
    fi, fs = (a.cpu().numpy().reshape(M, I * K) for a in ops.topk_items(q.reshape(M * I, D), x, K))
    if I == 1:
        same((ids, sc), (fi, fs), "topk_items itself")
    for u in range(M):
        order = np.lexsort((fi[u], -fs[u]))
        keep = order[np.unique(fi[u][order], return_index=True)[1]]  # the best entry of every id
        keep = keep[np.lexsort((fi[u][keep], -fs[u][keep]))][:K]
        same((ids[u], sc[u]), (fi[u][keep], fs[u][keep]), f"user {u}")


@pytest.mark.parametrize("T", [F32, F16])
@pytest.mark.parametrize("metric", ["IP", "L2"])
def test_serving_with_interest_queries_on_integer_data(metric, T):
    from torch_rechub_amd.utils.match import ExactIndex
    q, x, _, _ = ints(3, 7, 3, 24, 300)
    q[0, 1] = np.nan  # an absent interest is ignored
    index = ExactIndex(metric=metric, device="cuda:0", dtype=T).fit(x)
    ids, val = index.query(torch.as_tensor(q), 20)
    assert ids.device.type == "cpu" and ids.shape == val.shape == (7, 20)
    qz, absent = np.nan_to_num(q), np.where(np.isnan(q).any(axis=2), NINF, 0.0)
    if metric == "IP":
        eid, ev = ref(qz, x, 20, absent)
    else:
        eid, es = ref(2 * qz, x, 20, absent - (qz.astype(np.float64) ** 2).sum(axis=2), -(x.astype(np.float64) ** 2).sum(axis=1))
        ev = np.maximum(-es, 0.0)
    same((ids.numpy(), val.numpy().astype(np.float64)), (eid, ev))
    same([a.numpy() for a in index._indexer.query(torch.as_tensor(q), 20)], (ids.numpy(), val.numpy()), "HipIndexer")


def test_serving_angular_equals_the_per_interest_queries_merged_and_2d_is_unchanged():
    from torch_rechub_amd import ops
    from torch_rechub_amd.serving import HipBuilder, HipIndexer
    n, I, d, V, K = 6, 4, 16, 200, 30
    g = torch.Generator().manual_seed(0)
    q, x = torch.randn(n, I, d, generator=g), torch.randn(V, d, generator=g)
    index = HipIndexer(x, "angular", "cuda:0")
    ids, val = (a.numpy() for a in index.query(q, K))
    best = np.full((n, V), np.inf, dtype=np.float32)  # every item's smallest distance over the interests
    for i in range(I):
        pi, pv = (a.numpy() for a in index.query(q[:, i], V))
        best = np.minimum(best, np.take_along_axis(pv, np.argsort(pi, axis=1), axis=1))
    np.testing.assert_array_equal(val, np.sort(best, axis=1)[:, :K])
    np.testing.assert_array_equal(val, np.take_along_axis(best, ids, axis=1))
    assert all(len(set(r.tolist())) == K for r in ids)
    flat = HipIndexer(x, "IP", "cuda:0")
    got, exp = flat.query(q[:, 0], K), ops.topk_items(q[:, 0].cuda(), x.cuda(), K)
    assert torch.equal(got[0], exp[0].cpu()) and torch.equal(got[1], exp[1].cpu())
    with pytest.raises(ValueError, match="2D"):
        flat.query(q[0, 0], K)
    with pytest.raises(ValueError, match="SQ8.* not built"):
        HipIndexer(x, "IP", "cuda:0", quantizer="SQ8").query(q, K)
    with HipBuilder("IP", "cuda:0", index_type="IVF", nlists=4, niter=1).from_embeddings(x) as ivf:
        with pytest.raises(ValueError, match="IVF index are not built"):
            ivf.query(q, K)


@pytest.mark.parametrize("what,shape,k,kw,error", [
    ("I = 0", (2, 0, 8), 3, {}, RuntimeError), ("I = 17", (2, 17, 8), 3, {}, RuntimeError),
    ("K = 257", (2, 2, 8), 257, {}, RuntimeError), ("D = 1025", (2, 2, 1025), 3, {}, RuntimeError),
    ("q 2-D", (2, 8), 3, {}, ValueError), ("q 4-D", (2, 2, 2, 8), 3, {}, ValueError),
    ("qbias shape", (2, 2, 8), 3, {"qbias": torch.zeros(2, 3)}, ValueError),
    ("qbias dtype", (2, 2, 8), 3, {"qbias": torch.zeros(2, 2, dtype=torch.float64)}, ValueError),
    ("int8 table", (2, 2, 8), 3, {"table": torch.int8}, ValueError)])
def test_refusals_before_any_launch(what, shape, k, kw, error, monkeypatch):
    from torch_rechub_amd import _lib, ops
    call = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: call(name, *a) if "fwd" not in name else pytest.fail(name))
    table = torch.zeros(5, shape[-1], device="cuda:0").to(kw.get("table", F32))
    with pytest.raises(error):
        ops.topk_items_multi(torch.zeros(shape, device="cuda:0"), table, k,
                             **{n: v.cuda() for n, v in kw.items() if n != "table"})
