"""The inverted-file index without a device: the builder's arguments and errors, the two index file formats, the header's
declarations, and the float64 oracle itself (tests/ivf_oracle.py) with the gap condition of its training case."""
import ctypes

import numpy as np
import pytest
import torch

import ivf_oracle as IO

def test_builder_arguments_and_errors():
    from torch_rechub_amd.serving import HipBuilder, HipIvfIndexer, builder_factory
    from torch_rechub_amd.serving.base import BaseIndexer
    assert issubclass(HipIvfIndexer, BaseIndexer) and not HipIvfIndexer.__abstractmethods__
    b = HipBuilder()
    assert (b.metric, b.device, b.index_type) == ("L2", None, "Flat")
    b = HipBuilder("IP", "cuda:0")  # the positional order stays (metric, device)
    assert (b.metric, b.device, b.index_type) == ("IP", "cuda:0", "Flat")
    with pytest.raises(TypeError):
        HipBuilder("IP", None, "IVF")  # the new arguments are keyword-only
    b = builder_factory("hip", index_type="IVF", nlists=1024, nprobe=8)
    assert isinstance(b, HipBuilder) and (b.index_type, b.nlists, b.nprobe, b.niter, b.seed) == ("IVF", 1024, 8, 10, 2022)
    assert HipBuilder(index_type="IVF").nlists == 100 and HipBuilder(index_type="IVF").nprobe == 1  # nprobe=None: 1
    assert HipBuilder(index_type="IVF", nlists=16, nprobe=99).nprobe == 16  # clipped to nlists
    with pytest.raises(NotImplementedError) as e:
        HipBuilder(index_type="HNSW")
    assert '"Flat"' in str(e.value) and '"IVF"' in str(e.value)
    for bad in ("PQ", "flat", "", None):
        with pytest.raises(ValueError, match="index_type"):
            HipBuilder(index_type=bad)
    with pytest.raises(ValueError, match="nprobe"):
        HipBuilder(index_type="IVF", nprobe=0)
    with pytest.raises(ValueError, match="centroids"):
        HipBuilder(index_type="IVF", nlists=4, centroids=torch.zeros(3, 5))


def test_nlists_out_of_range_is_refused_at_from_embeddings():
    """Before anything touches a device."""
    from torch_rechub_amd.serving import HipBuilder
    table = torch.zeros(7, 3)
    for nlists in (8, 0, -1):
        with pytest.raises(ValueError, match="nlists"):
            with HipBuilder(index_type="IVF", nlists=nlists).from_embeddings(table):
                pass


def test_index_files(tmp_path, monkeypatch):
    """An IVF file holds exactly its five keys, the table in original row order; a flat file holds exactly
    {"metric", "table"} as before and still loads; from_index_file lets the file decide the type."""
    from torch_rechub_amd.serving import HipBuilder
    from torch_rechub_amd.serving import hip
    g = torch.Generator().manual_seed(0)
    table, cent = torch.randn(9, 4, generator=g), torch.randn(3, 4, generator=g)
    ivf = hip.HipIvfIndexer.__new__(hip.HipIvfIndexer)  # the fields save() writes, without a device
    ivf.metric, ivf._table, ivf.centroids, ivf.nprobe = "IP", table, cent, 2
    path = tmp_path / "ivf.index"
    ivf.save(path)
    blob = torch.load(path, weights_only=True)
    assert set(blob) == {"metric", "table", "index_type", "centroids", "nprobe"}
    assert blob["index_type"] == "IVF" and blob["metric"] == "IP" and blob["nprobe"] == 2
    assert torch.equal(blob["table"], table) and torch.equal(blob["centroids"], cent)
    with pytest.raises(ValueError, match="not an index file"):
        hip.load_index(path)  # the flat loader is as strict as it was

    flat = tmp_path / "flat.index"
    hip.save_index(flat, "angular", table)
    assert set(torch.load(flat, weights_only=True)) == {"metric", "table"}
    metric, got = hip.load_index(flat)
    assert metric == "angular" and torch.equal(got, table)

    made = []
    monkeypatch.setattr(hip, "HipIndexer", lambda t, m, d: made.append(("Flat", m, t)) or "flat")
    monkeypatch.setattr(hip, "HipIvfIndexer", lambda t, c, m, d, p: made.append(("IVF", m, t, c, p)) or "ivf")
    for builder in (HipBuilder(), HipBuilder(index_type="IVF", nlists=3)):  # the file decides, not the builder
        with builder.from_index_file(flat) as index:
            assert index == "flat"
        with builder.from_index_file(path) as index:
            assert index == "ivf"
    assert [m[:2] for m in made] == [("Flat", "angular"), ("IVF", "IP")] * 2
    assert torch.equal(made[1][2], table) and torch.equal(made[1][3], cent) and made[1][4] == 2
    torch.save({"metric": "IP", "table": table, "index_type": "IVF"}, path)
    with pytest.raises(ValueError, match="not an index file"):
        with HipBuilder().from_index_file(path):
            pass


def test_header_declares_the_entry_points_and_the_signatures_follow():
    from torch_rechub_amd import _header, _lib
    with open(_header.PATH) as f:
        text = f.read()
    for name in ("rh_ivf_supported", "rh_ivf_plan", "rh_ivf_scan", "rh_ivf_list_mean"):
        assert f"int {name}(" in text
        assert name in _lib.SIGNATURES and name not in _lib._VALUE_RETURNING
    i, l, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert _lib.SIGNATURES["rh_ivf_supported"] == [i, i, i, i, p]
    assert _lib.SIGNATURES["rh_ivf_plan"] == [i, i, i, i, p, p, p]
    assert _lib.SIGNATURES["rh_ivf_scan"] == [p, l, p, p, p, p, i, p, p, p, p, i, i, i, i, i, i, p, p, p, p]
    assert _lib.SIGNATURES["rh_ivf_list_mean"] == [p, p, p, i, i, i, p, p]
    assert "torch_rechub/serving/faiss.py" in text and "IVF{nlists},Flat" in text and "`nprobe`" in text


def test_ops_are_present_and_refuse_cpu_tensors():
    from torch_rechub_amd import ops
    x = torch.zeros(4, 3)
    off = torch.tensor([0, 4], dtype=torch.int32)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.ivf_scan(x[:1], x, torch.arange(4, dtype=torch.int32), off, torch.zeros(1, 1, dtype=torch.int32), 2)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.ivf_list_mean(x, off, x[:1])


def test_oracle_on_a_hand_worked_case():
    """Four rows of width 1, x = 1, 3, 2, 3; list 0 = {0, 2}, list 1 = {1, 3}; the query is 1, so the scores are x."""
    x = np.array([[1.0], [3.0], [2.0], [3.0]], dtype=np.float32)
    q = np.ones((1, 1), dtype=np.float32)
    lists = [np.array([0, 2]), np.array([1, 3])]
    ids, s = IO.ivf_rank(q, x, None, lists, np.array([[1]]), 3)
    assert ids.tolist() == [[1, 3, -1]] and s[0, :2].tolist() == [3.0, 3.0] and np.isneginf(s[0, 2])
    ids, s = IO.ivf_rank(q, x, None, lists, np.array([[0, 1]]), 3, exclude=np.array([[3, -1]]))
    assert ids.tolist() == [[1, 2, 0]] and s.tolist() == [[3.0, 2.0, 1.0]]
    ids, s = IO.ivf_rank(q, x, np.array([0, 0, 5, 0], dtype=np.float32), lists, np.array([[-1, 0]]), 2)
    assert ids.tolist() == [[2, 0]] and s.tolist() == [[7.0, 1.0]]
    ids, _ = IO.ivf_rank(q, x, None, lists, np.array([[-1, -1]]), 2)
    assert ids.tolist() == [[-1, -1]]
    xs, bs, rid, off = IO.group(x, np.arange(4, dtype=np.float32), [np.array([2, 0]), np.array([], dtype=np.int64),
                                                                    np.array([1, 3])])
    assert rid.tolist() == [0, 2, 1, 3] and off.tolist() == [0, 2, 2, 4] and rid.dtype == off.dtype == np.int32
    assert xs[:, 0].tolist() == [1.0, 2.0, 3.0, 3.0] and bs.tolist() == [0.0, 2.0, 1.0, 3.0]
    c = np.array([[0.0], [2.0], [4.0]], dtype=np.float32)
    assert IO.coarse(np.array([[1.0]], dtype=np.float32), c, 2, "L2").tolist() == [[0, 1]]  # a tie: the lower list
    assert IO.coarse(np.array([[1.0]], dtype=np.float32), c, 2, "IP").tolist() == [[2, 1]]
    a, _ = IO.assign(x, c)
    assert a.tolist() == [0, 1, 1, 1]  # 1 and 3 are ties: the lower list
    m = IO.list_mean(x, IO.lists_of(a, 3), c)
    assert m[:, 0].tolist() == [1.0, 8.0 / 3.0, 4.0]  # the empty list keeps its centroid


@pytest.mark.parametrize("seed", IO.LLOYD_SEEDS)
def test_lloyd_generator_keeps_its_gap_condition(seed):
    """In every round through the final assign, every row's gap between its best and second-best squared distance is at
    least 4 x what fp32 can move it by (ivf_oracle.gap_bound), so the device build must reproduce the float64 partition;
    and the case is not trivial: the assignment changes in several rounds and every cluster ends up populated."""
    x, init = IO.lloyd_data(seed)
    assert x.shape == (222, 5) and init.shape == (6, 5) and x.dtype == np.float32
    got = IO.lloyd(x, init, 6)
    print(f"seed {seed}: worst gap / bound = {got['ratio']:.1f}, rounds with reassignments = {got['moved']}, "
          f"final sizes = {got['sizes'].tolist()}")
    assert got["ratio"] >= 4.0
    assert got["moved"] >= 2 and (got["sizes"] > 0).all()
