"""ops.ivf_scan, ops.ivf_list_mean, the k-means build and serving.HipIvfIndexer on the MI355X against the float64 oracle
of tests/ivf_oracle.py.  On integer data (topk_oracle.int_data) every score is exact in fp32, so ids AND scores must
equal the oracle's bit for bit; float data goes through topk_oracle.check_float."""
import numpy as np
import pytest
import torch

import ivf_oracle as IO
import topk_oracle as O
from torch_rechub_amd._lib import H

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 63, 64, 65, 129)  # lists 0 .. 5 of the shared index, V = 322


def t(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def scan(q, x, bias, lists, probe, k, exclude=None, qd=None):
    from torch_rechub_amd import ops
    xs, bs, rid, off = IO.group(x, bias, lists)
    ids, sc = ops.ivf_scan(t(q) if qd is None else qd, t(xs), t(rid), t(off), t(np.asarray(probe, dtype=np.int32)), k,
                           bias=t(bs), exclude=t(exclude))
    assert ids.dtype == torch.int64 and sc.dtype == torch.float32 and ids.shape == sc.shape == (q.shape[0], k)
    return ids.cpu().numpy(), sc.cpu().numpy()


def check_exact(q, x, bias, lists, probe, k, exclude=None, qd=None):
    ids, sc = scan(q, x, bias, lists, probe, k, exclude, qd)
    wi, ws = IO.ivf_rank(q, x, bias, lists, probe, k, exclude)
    np.testing.assert_array_equal(ids, wi)
    np.testing.assert_array_equal(sc.astype(np.float64), ws)
    return ids, sc


@pytest.mark.parametrize("K,M", [(10, 130), (129, 67), (10, 1)])
def test_list_lengths_and_probing_load(K, M):
    """Lists of 0, 1, 63, 64, 65 and 129 rows in one index.  RB = 64 at K = 10, 32 at K = 129: the 129-row list is probed
    by all M queries (three query tiles), the 65-row list by the first RB + 1 (a second tile of one pair), the 64-row
    list by the next RB, the 63-row list by one, the 1-row list by none; slot 2 holds the empty list or nothing."""
    RB = 64 if K <= 128 else 32
    q, x, bias = O.int_data(100 + K, M, 9, sum(LENGTHS), with_bias=True)
    lists = IO.lists_of_lengths(7, LENGTHS)
    probe = np.full((M, 3), -1, dtype=np.int32)
    probe[:, 0] = 5
    probe[:RB + 1, 1] = 4
    probe[RB + 1:2 * RB + 1, 1] = 3
    probe[2 * RB + 1:2 * RB + 2, 1] = 2
    probe[::2, 2] = 0
    check_exact(q, x, bias, lists, probe, K)


@pytest.mark.parametrize("D", [1, 63, 64, 65, 130])
def test_widths_and_a_strided_q(D):
    M, V, K = 5, 300, 10
    q, x, bias = O.int_data(200 + D, M, D, V, with_bias=True)
    wide = torch.zeros((M, D + 3), device="cuda:0")
    wide[:, :D] = t(q)
    lists = IO.random_lists(D, V, 4)
    probe = np.array([[0, 1], [3, 2], [1, -1], [2, 0], [3, 1]])
    check_exact(q, x, bias, lists, probe, K, qd=wide[:, :D])


def test_absent_and_empty_probes():
    """-1 entries; a row whose probes are all -1 and a row whose probes are all empty lists give all -1 / -inf."""
    M, D, V, K = 6, 5, 200, 4
    q, x, _ = O.int_data(3, M, D, V)
    lists = IO.random_lists(3, V, 5, empty=(1, 3))
    probe = np.array([[-1, -1, -1], [1, 3, -1], [3, 1, -1], [-1, 0, 1], [2, -1, 4], [4, 2, 0]])
    ids, sc = check_exact(q, x, None, lists, probe, K)
    assert (ids[:3] == -1).all() and np.isneginf(sc[:3]).all() and (ids[3:] >= 0).all()


@pytest.mark.parametrize("nprobe", [1, 2, 65])
def test_nprobe(nprobe):
    """nprobe = 65: a lane of the merge owns two lists."""
    M, D, V, K, L = 7, 6, 500, 12, 70
    q, x, bias = O.int_data(300 + nprobe, M, D, V, with_bias=True)
    lists = IO.random_lists(nprobe, V, L, empty=(4,))
    rng = np.random.default_rng(nprobe)
    probe = np.stack([rng.permutation(L)[:nprobe] for _ in range(M)])
    check_exact(q, x, bias, lists, probe, K)


def test_ties_go_to_the_lower_original_id():
    """Identical best rows in different lists and on both sides of a tile edge inside one list (positions 63 and 64 of a
    129-row list); the lowest id of all sits in the list probed in the LAST slot."""
    D, K = 4, 6
    q = np.array([[3, -3, 3, 3]], dtype=np.float32)
    _, x, _ = O.int_data(5, 1, D, 300)
    x[np.abs(x).sum(1) == 12] = 0.0  # no accidental copy of the best row
    lists = [np.arange(100, 229), np.arange(0, 100), np.arange(229, 300)]
    twins = [100 + 63, 100 + 64, 40, 250, 2]  # list 0 at the tile edge, list 1, list 2, and id 2 in list 1
    x[twins] = q[0]
    for probe in ([[0, 2, 1]], [[2, 0, 1]], [[1, 0, 2]]):
        ids, sc = check_exact(q, x, None, lists, np.array(probe), K)
        assert ids[0, :5].tolist() == [2, 40, 163, 164, 250] and (sc[0, :5] == 36.0).all() and sc[0, 5] < 36.0
    ids, _ = check_exact(q, x, None, lists, np.array([[0, 2]]), 2)  # K-th place: the equal score does not displace
    assert ids[0].tolist() == [163, 164]


@pytest.mark.parametrize("S", [0, 1, 65])
def test_exclusions(S):
    """Excluded ids in probed lists, in unprobed lists and -1 padding; query 0 probes 63 + 1 rows at K = 64 and loses some
    of them: fewer than K candidates are left."""
    M, D, K = 4, 5, 64
    q, x, bias = O.int_data(400 + S, M, D, sum(LENGTHS), with_bias=True)
    lists = IO.lists_of_lengths(11, LENGTHS)
    probe = np.array([[2, 1], [5, 4], [3, 0], [4, 2]])
    exclude = None
    if S > 0:
        rng = np.random.default_rng(S)
        exclude = np.full((M, S), -1, dtype=np.int64)
        for i in range(M):
            mine = np.concatenate([lists[l] for l in probe[i]])
            other = np.setdiff1d(np.arange(sum(LENGTHS)), mine)
            n_in, n_out = (S + 1) // 2, S // 4
            exclude[i, :n_in] = rng.choice(mine, size=min(n_in, len(mine)), replace=False)
            exclude[i, n_in:n_in + n_out] = rng.choice(other, size=n_out, replace=False)
            rng.shuffle(exclude[i])
    ids, _ = check_exact(q, x, bias, lists, probe, K, exclude)
    if S > 0:
        assert ids[0, -1] == -1
        for i in range(M):
            assert not np.isin(ids[i][ids[i] >= 0], exclude[i]).any()


@pytest.mark.parametrize("K", [1, 128, 129, H.RH_TOPK_MAX_K])
def test_k_range_and_k_above_the_union(K):
    """Query 0 probes 64 + 1 rows (fewer than K from 128 on), query 1 probes 129 + 65 + 63 = 257 rows."""
    q, x, bias = O.int_data(500 + K, 2, 7, sum(LENGTHS), with_bias=True)
    lists = IO.lists_of_lengths(13, LENGTHS)
    ids, _ = check_exact(q, x, bias, lists, np.array([[3, 1, -1], [5, 4, 2]]), K)
    assert (ids[0] >= 0).sum() == min(K, 65) and (ids[1] >= 0).all()


def test_batch_independence_and_reproducibility():
    """A query alone equals the same query inside M = 65, and two calls give the same bits (float data)."""
    M, D, V, K, L = 65, 33, 700, 20, 9
    q, x, bias = O.normal_data(6, M, D, V, with_bias=True)
    lists = IO.random_lists(6, V, L)
    rng = np.random.default_rng(6)
    probe = np.stack([rng.permutation(L)[:3] for _ in range(M)])
    ids, sc = scan(q, x, bias, lists, probe, K)
    ids2, sc2 = scan(q, x, bias, lists, probe, K)
    assert ids.tobytes() == ids2.tobytes() and sc.tobytes() == sc2.tobytes()
    for i in (0, 17, 64):
        one_i, one_s = scan(q[i:i + 1], x, bias, lists, probe[i:i + 1], K)
        assert one_i.tobytes() == ids[i:i + 1].tobytes() and one_s.tobytes() == sc[i:i + 1].tobytes()


@pytest.mark.parametrize("data,shape", [
    pytest.param("int", (70, 65, 3000, 50, 12, 5), id="int"),
    pytest.param("normal", (70, 65, 3000, 50, 12, 5), id="normal"),
    # three k chunks, 32-row tiles with a ragged last one and 65 exclusions per query at once
    pytest.param("int", (67, 130, 400, 129, 12, 65), id="int-three-chunks-rb32-exclude"),
])
def test_every_list_probed_is_the_flat_scan_bit_for_bit(data, shape):
    from torch_rechub_amd import ops
    M, D, V, K, L, S = shape
    q, x, bias = (O.int_data if data == "int" else O.normal_data)(7, M, D, V, with_bias=True)
    rng = np.random.default_rng(7)
    exclude = rng.integers(-1, V, size=(M, S))
    lists = IO.random_lists(7, V, L, empty=(5,))
    probe = np.stack([rng.permutation(L) for _ in range(M)])  # every list, in any order
    ids, sc = scan(q, x, bias, lists, probe, K, exclude)
    fi, fs = ops.topk_items(t(q), t(x), K, bias=t(bias), exclude=t(exclude))
    assert ids.tobytes() == fi.cpu().numpy().tobytes() and sc.tobytes() == fs.cpu().numpy().tobytes()


def test_float_data_with_some_lists_probed():
    """check_float of tests/topk_oracle.py over the probed rows, with eps_i taken over the probed rows of query i."""
    M, D, V, K, L = 9, 70, 2000, 30, 16
    q, x, bias = O.normal_data(8, M, D, V, with_bias=True)
    lists = IO.random_lists(8, V, L)
    rng = np.random.default_rng(8)
    probe = np.stack([rng.permutation(L)[:4] for _ in range(M)])
    exclude = rng.integers(0, V, size=(M, 7))
    ids, sc = scan(q, x, bias, lists, probe, K, exclude)
    ok = IO.valid(M, V, lists, probe, exclude)
    probed = IO.probed_mask(M, V, lists, probe)
    eps = np.array([O.eps_rows(q[i:i + 1], x[probed[i]], bias[probed[i]])[0] for i in range(M)])
    O.check_float(ids, sc, O.scores64(q, x, bias), ok, eps, K, "ivf float")


def test_memory_stays_within_the_plan():
    """M = 130, V = 5000, nprobe = 4 of 16 lists, K = 10: the call's peak above what was allocated before is the planned
    workspace (partials, pair indices, offsets) plus the two outputs, up to the allocator's 512-byte rounding of its six
    blocks -- the temporaries of the pair sort are freed before the partials are allocated and are smaller than they --
    and far below the M V 4 bytes of the logits."""
    from torch_rechub_amd import ops
    M, D, V, K, L, P = 130, 64, 5000, 10, 16, 4
    q, x, _ = O.normal_data(9, M, D, V)
    lists = IO.random_lists(9, V, L)
    rng = np.random.default_rng(9)
    probe = np.stack([rng.permutation(L)[:P] for _ in range(M)])
    xs, _, rid, off = IO.group(x, None, lists)
    args = (t(q), t(xs), t(rid), t(off), t(probe.astype(np.int32)), K)
    rb, grid, nbytes = ops.ivf_plan(M, L, P, K)
    assert rb == 64 and grid == -(-M * P // 64) + L + 1
    assert nbytes == 8 * M * P * K + 4 * M * P + 8 * (L + 2)
    assert ops.ivf_plan(M, L, P, 129)[0] == 32
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    ids, sc = ops.ivf_scan(*args)
    torch.cuda.synchronize()
    rise = torch.cuda.max_memory_allocated() - before
    print(f"peak rise {rise} bytes; workspace {nbytes}, outputs {M * K * 12}; M V 4 = {M * V * 4}")
    assert rise <= nbytes + M * K * 12 + 6 * 512
    assert rise < M * V * 4 // 8
    probed = IO.probed_mask(2, V, lists, probe[:2])
    eps = np.array([O.eps_rows(q[i:i + 1], x[probed[i]])[0] for i in range(2)])
    O.check_float(ids.cpu().numpy()[:2], sc.cpu().numpy()[:2], O.scores64(q[:2], x), probed, eps, K, "memory case")


def test_refusals(monkeypatch):
    """D, K, S and nprobe outside their limits, a wrong dtype, a non-contiguous table and a CPU tensor raise before
    anything is launched."""
    from torch_rechub_amd import _lib, ops
    real, launched = _lib.call, []

    def spy(name, *a):
        if name in ("rh_ivf_scan", "rh_ivf_list_mean"):
            launched.append(name)
        return real(name, *a)

    monkeypatch.setattr(_lib, "call", spy)

    def case(M=2, D=4, V=8, K=3, S=0, nprobe=1):
        i32 = dict(dtype=torch.int32, device="cuda:0")
        return dict(q=torch.zeros(M, D, device="cuda:0"), table_sorted=torch.zeros(V, D, device="cuda:0"),
                    row_ids=torch.arange(V, **i32), list_offsets=torch.tensor([0, V], **i32),
                    probe=torch.zeros(M, nprobe, **i32), k=K,
                    exclude=torch.zeros(M, S, dtype=torch.int64, device="cuda:0") if S else None)

    for bad in (dict(D=1025), dict(K=257), dict(K=0), dict(S=1025), dict(nprobe=257), dict(nprobe=0)):
        with pytest.raises(RuntimeError, match="inverted-file scan.*no HIP kernel"):
            ops.ivf_scan(**case(**bad))
    for name, cast in (("q", torch.float64), ("table_sorted", torch.float16), ("probe", torch.int64),
                       ("row_ids", torch.int64), ("list_offsets", torch.int64)):
        c = case()
        c[name] = c[name].to(cast)
        with pytest.raises(ValueError):
            ops.ivf_scan(**c)
    c = case()
    c["table_sorted"] = torch.zeros(4, 8, device="cuda:0").t()
    with pytest.raises(ValueError, match="contiguous"):
        ops.ivf_scan(**c)
    for name in ("q", "table_sorted", "probe"):
        c = case()
        c[name] = c[name].cpu()
        with pytest.raises(RuntimeError, match="HIP device"):
            ops.ivf_scan(**c)
    x = torch.zeros(8, 4, device="cuda:0")
    off = torch.tensor([0, 8], dtype=torch.int32, device="cuda:0")
    with pytest.raises(ValueError):
        ops.ivf_list_mean(x, off.long(), x[:1])
    with pytest.raises(ValueError):
        ops.ivf_list_mean(x.t(), off, torch.zeros(1, 8, device="cuda:0"))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.ivf_list_mean(x, off, x[:1].cpu())
    assert launched == []
    ids, sc = ops.ivf_scan(**case(M=0))
    assert ids.shape == (0, 3) and sc.shape == (0, 3) and launched == []


# ---- ops.ivf_list_mean ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [7, 70])
def test_list_mean_is_the_correctly_rounded_mean(D):
    """Integer rows, lists of 0, 1, 64, 65 and 1000 rows: the sums are exact in fp32, so the one division gives the
    float64 mean rounded to fp32; the empty list returns ``previous``; two runs give the same bits."""
    from torch_rechub_amd import ops
    lengths = (1000, 0, 1, 64, 65)
    V = sum(lengths)
    rng = np.random.default_rng(D)
    x = rng.integers(-3, 4, size=(V, D)).astype(np.float32)
    prev = rng.standard_normal((len(lengths), D)).astype(np.float32)
    off = np.cumsum((0,) + lengths).astype(np.int32)
    lists = [np.arange(off[l], off[l + 1]) for l in range(len(lengths))]
    want = IO.list_mean(x, lists, prev).astype(np.float32)
    got = ops.ivf_list_mean(t(x), t(off), t(prev)).cpu().numpy()
    again = ops.ivf_list_mean(t(x), t(off), t(prev)).cpu().numpy()
    assert got.tobytes() == want.tobytes()
    assert got[1].tobytes() == prev[1].tobytes() and again.tobytes() == got.tobytes()


# ---- training ------------------------------------------------------------------------------------------------------
def build(x, **config):
    from torch_rechub_amd.serving import builder_factory
    return builder_factory("hip", index_type="IVF", **config).from_embeddings(torch.from_numpy(x))


def partition(index):
    rid, off = (a.cpu().numpy() for a in index.lists())
    a = np.empty(len(index), dtype=np.int64)
    for l in range(index.nlists):
        rows = rid[off[l]:off[l + 1]]
        assert (np.diff(rows) > 0).all()  # ids ascend inside a list
        a[rows] = l
    return a


@pytest.mark.parametrize("seed", IO.LLOYD_SEEDS)
def test_kmeans_reproduces_the_float64_partition(seed):
    """The training case of ivf_oracle.lloyd_data, whose gaps are at least 4 x what fp32 can move them by in every round
    (tests/test_ivf_host.py): six rounds from the given start give the oracle's final partition exactly and centroids
    within centroid_bound of the list's size; niter = 0 is "assign to the given centroids"."""
    x, init = IO.lloyd_data(seed)
    want = IO.lloyd(x, init, 6)
    with build(x, nlists=6, niter=6, centroids=torch.from_numpy(init)) as index:
        np.testing.assert_array_equal(partition(index), want["assign"])
        assert index.list_sizes().cpu().tolist() == want["sizes"].tolist()
        err = np.abs(index.centroids.cpu().numpy().astype(np.float64) - want["centroids"]).max(axis=1)
    bound = np.array([IO.centroid_bound(x, n) for n in want["mean_sizes"]])
    print(f"seed {seed}: centroid error {err.max():.3e} (bound {bound.min():.3e})")
    assert (err <= bound).all()
    with build(x, nlists=6, niter=0, centroids=torch.from_numpy(init)) as index:
        np.testing.assert_array_equal(partition(index), IO.assign(x, init)[0])
        assert index.centroids.cpu().numpy().tobytes() == init.tobytes()


def test_seeded_builds_are_reproducible():
    x, _ = IO.lloyd_data(IO.LLOYD_SEEDS[0])
    out = []
    for seed in (5, 5, 6):
        with build(x, nlists=6, niter=4, seed=seed) as index:
            out.append((index.centroids.cpu().numpy().tobytes(), partition(index).tobytes()))
    assert out[0] == out[1] and out[0][0] != out[2][0]


# ---- serving -------------------------------------------------------------------------------------------------------
def serving_case(seed=21, M=9, D=6, V=900, L=7):
    q, x, _ = O.int_data(seed, M, D, V)
    cent = np.random.default_rng(seed).integers(-3, 4, size=(L, D)).astype(np.float32)
    cent[3] = 40.0  # a centroid far from every row: an empty list
    exclude = np.random.default_rng(seed + 1).integers(-1, V, size=(M, 4))
    return q, x, cent, exclude


@pytest.mark.parametrize("metric", ["L2", "IP", "angular"])
def test_all_lists_probed_is_the_flat_index_bit_for_bit(metric):
    from torch_rechub_amd.serving import HipBuilder, HipIvfIndexer
    q, x, _ = O.normal_data(22, 11, 17, 1500)
    x[5] = 0.0  # a zero row (angular: cos 0 with everything)
    exclude = torch.from_numpy(np.random.default_rng(22).integers(-1, 1500, size=(11, 3)))
    qd = torch.from_numpy(q).to("cuda:0")
    with HipBuilder(metric).from_embeddings(torch.from_numpy(x)) as flat:
        fi, fv = flat.query(qd, 40, exclude=exclude)
    with HipBuilder(metric, index_type="IVF", nlists=13, nprobe=13, niter=3).from_embeddings(torch.from_numpy(x)) as ivf:
        assert isinstance(ivf, HipIvfIndexer) and len(ivf) == 1500 and (ivf.nlists, ivf.nprobe) == (13, 13)
        ii, iv = ivf.query(qd, 40, exclude=exclude)
    assert torch.equal(ii, fi) and iv.cpu().numpy().tobytes() == fv.cpu().numpy().tobytes()


@pytest.mark.parametrize("metric", ["L2", "IP"])
def test_given_centroids_and_fewer_probes_match_the_oracle(metric):
    """Integer table, queries and centroids: assignment and coarse selection are exact in fp32, so the ids equal those of
    the float64 oracle (coarse selection, union of the lists, rank); also the nprobe override and its clipping."""
    q, x, cent, exclude = serving_case()
    M, V, L, K = q.shape[0], x.shape[0], cent.shape[0], 25
    lists = IO.lists_of(IO.assign(x, cent)[0], L)
    assert len(lists[3]) == 0
    score = lambda: O.scores64(q, x) if metric == "IP" else -((q.astype(np.float64)[:, None] - x[None]) ** 2).sum(-1)

    def want(nprobe):
        ok = IO.valid(M, V, lists, IO.coarse(q, cent, nprobe, metric), exclude)
        return O.rank(score(), ok, K)

    qd = torch.from_numpy(q).to("cuda:0")
    with build(x, metric=metric, nlists=L, nprobe=2, niter=0, centroids=torch.from_numpy(cent)) as index:
        assert index.nprobe == 2
        ids, val = index.query(qd, K, exclude=torch.from_numpy(exclude))
        wi, ws = want(2)
        np.testing.assert_array_equal(ids.cpu().numpy(), wi)
        np.testing.assert_array_equal(val.cpu().numpy().astype(np.float64), np.where(wi < 0, np.inf, -ws) if metric == "L2" else ws)
        ids3, _ = index.query(qd, K, exclude=torch.from_numpy(exclude), nprobe=3)
        np.testing.assert_array_equal(ids3.cpu().numpy(), want(3)[0])
        assert (ids3 != ids).any()
        all_i, _ = index.query(qd, K, exclude=torch.from_numpy(exclude), nprobe=L)
        big_i, _ = index.query(qd, K, exclude=torch.from_numpy(exclude), nprobe=L + 50)  # clipped to nlists
        np.testing.assert_array_equal(all_i.cpu().numpy(), want(L)[0])
        assert torch.equal(all_i, big_i)
        on_cpu, _ = index.query(torch.from_numpy(q), K)  # the results land on the queries' device
        assert ids.is_cuda and val.is_cuda and not on_cpu.is_cuda
    with build(x, metric=metric, nlists=L, nprobe=L + 1, niter=0, centroids=torch.from_numpy(cent)) as index:
        assert index.nprobe == L


def test_save_and_load_give_identical_bits(tmp_path):
    from torch_rechub_amd.serving import HipBuilder, HipIndexer, HipIvfIndexer
    q, x, _ = O.normal_data(23, 8, 12, 1000)
    qd = torch.from_numpy(q).to("cuda:0")
    path, flat_path = tmp_path / "ivf.index", tmp_path / "flat.index"
    with build(x, metric="angular", nlists=10, nprobe=3, niter=4, seed=1) as index:
        ids, val = index.query(qd, 15)
        index.save(path)
    with HipBuilder("IP").from_embeddings(torch.from_numpy(x)) as flat:
        fi, fv = flat.query(qd, 15)
        flat.save(flat_path)
    for builder in (HipBuilder(), HipBuilder(index_type="IVF", nlists=4)):  # the file decides its type and its metric
        with builder.from_index_file(path) as index:
            assert isinstance(index, HipIvfIndexer) and (index.metric, index.nlists, index.nprobe) == ("angular", 10, 3)
            ids2, val2 = index.query(qd, 15)
        assert torch.equal(ids, ids2) and val.cpu().numpy().tobytes() == val2.cpu().numpy().tobytes()
        with builder.from_index_file(flat_path) as index:
            assert isinstance(index, HipIndexer) and index.metric == "IP"
            fi2, fv2 = index.query(qd, 15)
        assert torch.equal(fi, fi2) and torch.equal(fv, fv2)
