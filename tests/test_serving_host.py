"""The serving package, ExactIndex and the top-K entry points without a device: dispatch, abstract bases, the index file,
the header's declarations and the integration switch."""
import ctypes
import importlib
import sys
import textwrap

import pytest
import torch


def test_builder_factory_dispatch_and_error_types():
    from torch_rechub_amd.serving import BaseBuilder, HipBuilder, builder_factory
    b = builder_factory("hip")
    assert isinstance(b, HipBuilder) and isinstance(b, BaseBuilder) and b.metric == "L2"
    assert builder_factory("hip", metric="angular").metric == "angular"
    for name, lib in (("annoy", "annoy"), ("faiss", "faiss"), ("milvus", "pymilvus")):
        with pytest.raises(ImportError, match=lib) as e:
            builder_factory(name)
        assert '"hip"' in str(e.value)
    with pytest.raises(NotImplementedError):
        builder_factory("hnswlib")


def test_base_classes_are_abstract():
    from torch_rechub_amd.serving import BaseBuilder, BaseIndexer, HipBuilder, HipIndexer
    for cls in (BaseBuilder, BaseIndexer):
        with pytest.raises(TypeError):
            cls()
    assert BaseBuilder.__abstractmethods__ == {"from_embeddings", "from_index_file"}
    assert BaseIndexer.__abstractmethods__ == {"query", "save"}
    assert issubclass(HipBuilder, BaseBuilder) and issubclass(HipIndexer, BaseIndexer)
    assert not HipBuilder.__abstractmethods__ and not HipIndexer.__abstractmethods__


def test_unknown_metric_is_rejected():
    from torch_rechub_amd.serving import HipBuilder
    from torch_rechub_amd.utils.match import ExactIndex
    for good in ("L2", "IP", "angular"):
        assert HipBuilder(metric=good).metric == good
    with pytest.raises(ValueError, match="metric"):
        HipBuilder(metric="cosine")
    with pytest.raises(ValueError, match="metric"):
        ExactIndex(metric="hamming")
    assert str(ExactIndex(n_trees=10)) == "ExactIndex(metric=angular)"


def test_index_file_carries_metric_and_table_bit_for_bit(tmp_path):
    from torch_rechub_amd.serving.hip import load_index, save_index
    table = torch.randn(37, 5, generator=torch.Generator().manual_seed(0))
    table[3] = 0.0
    table[4, 0] = 1e-40  # a subnormal survives too
    path = tmp_path / "items.index"
    save_index(path, "angular", table.t().contiguous().t())  # a non-contiguous view of the same values
    metric, got = load_index(path)
    assert metric == "angular" and got.dtype == torch.float32 and got.is_contiguous()
    assert got.numpy().tobytes() == table.numpy().tobytes()
    blob = torch.load(path, weights_only=True)
    assert set(blob) == {"metric", "table"}
    with pytest.raises(ValueError, match="metric"):
        save_index(path, "cosine", table)
    torch.save({"table": table}, path)
    with pytest.raises(ValueError, match="not an index file"):
        load_index(path)


def test_header_declares_the_entry_points_and_the_signatures_follow():
    from torch_rechub_amd import _header, _lib
    with open(_header.PATH) as f:
        text = f.read()
    for name in ("rh_topk_supported", "rh_topk_plan", "rh_topk_fwd"):
        assert f"int {name}(" in text
        assert name in _lib.SIGNATURES and name not in _lib._VALUE_RETURNING
    i, l, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert _lib.SIGNATURES["rh_topk_supported"] == [i, i, i, p]
    assert _lib.SIGNATURES["rh_topk_plan"] == [i, i, i, p, p]
    assert _lib.SIGNATURES["rh_topk_fwd"] == [p, l, p, p, p, i, p, i, i, i, i, i, i, p, p, p, p]
    assert "replaces: Annoy.fit" in text and "run_hstu_movielens.py:109-114" in text


def _fake_package(tmp_path, monkeypatch, name, serving_source):
    root = tmp_path / name
    (root / "serving").mkdir(parents=True)
    (root / "utils").mkdir()
    (root / "__init__.py").write_text("")
    (root / "utils" / "__init__.py").write_text("")
    (root / "utils" / "match.py").write_text("class Annoy(object):\n    pass\n")
    (root / "serving" / "__init__.py").write_text(textwrap.dedent(serving_source))
    monkeypatch.syspath_prepend(str(tmp_path))
    importlib.invalidate_caches()


def _forget(name):
    for m in [m for m in sys.modules if m == name or m.startswith(name + ".")]:
        del sys.modules[m]


def test_enable_with_an_unimportable_serving_package(tmp_path, monkeypatch):
    """The reference's serving package imports annoy, faiss and pymilvus unconditionally: where one is missing, enable()
    skips the builder, still adds ExactIndex, and disable() leaves nothing behind."""
    from torch_rechub_amd import integration
    from torch_rechub_amd.utils.match import ExactIndex
    name = "rh_fake_ref_a"
    _fake_package(tmp_path, monkeypatch, name, "import a_backend_that_is_not_installed\n")
    try:
        done = integration.enable(layers=False, models=False, trainers=False, data=False, package=name)
        assert done == [f"{name}.utils.match.ExactIndex"]
        match = importlib.import_module(f"{name}.utils.match")
        assert match.ExactIndex is ExactIndex
        assert integration.enable(layers=False, models=False, trainers=False, data=False, package=name) == []
        integration.disable()
        assert not hasattr(match, "ExactIndex") and not integration._undo
        assert integration.enable(layers=False, models=False, trainers=False, data=False, serving=False, package=name) == []
        assert not hasattr(match, "ExactIndex")
    finally:
        integration.disable()
        _forget(name)


def test_enable_teaches_an_importable_builder_factory_hip(tmp_path, monkeypatch):
    from torch_rechub_amd import integration
    from torch_rechub_amd.serving import HipBuilder
    name = "rh_fake_ref_b"
    _fake_package(tmp_path, monkeypatch, name, """
        def builder_factory(model, **builder_config):
            if model == "annoy":
                return ("annoy", builder_config)
            raise NotImplementedError(model)
        """)
    try:
        serving = importlib.import_module(f"{name}.serving")
        original = serving.builder_factory
        done = integration.enable(layers=False, models=False, trainers=False, data=False, package=name)
        assert f"{name}.serving.builder_factory" in done
        assert isinstance(serving.builder_factory("hip", metric="IP"), HipBuilder)
        assert serving.builder_factory("annoy", n_trees=3) == ("annoy", {"n_trees": 3})
        with pytest.raises(NotImplementedError):
            serving.builder_factory("other")
        integration.disable()
        assert serving.builder_factory is original
    finally:
        integration.disable()
        _forget(name)
