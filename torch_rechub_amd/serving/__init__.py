"""Retrieval-stage indexes (API mirror of torch_rechub/serving): ``builder_factory("hip")`` is the exact index on the
streaming top-K kernel (csrc/topk.hip); ``builder_factory("hip", index_type="IVF", nlists=..., nprobe=...)`` is the
inverted-file index on the list-scan kernel (csrc/ivf.hip), which scans ``nprobe`` of ``nlists`` k-means lists per query and
equals the exact index at ``nprobe == nlists``.  ``index_type="HNSW"`` is not built.  The reference's approximate backends are named so that a call written for them
fails with a pointer to ``"hip"`` instead of an import error deep inside a third-party package."""
from .base import BaseBuilder, BaseIndexer
from .hip import HipBuilder, HipIndexer, HipIvfIndexer

_FOREIGN = {"annoy": "annoy", "faiss": "faiss", "milvus": "pymilvus"}


def builder_factory(model, **config):
    """The builder of the retrieval backend ``model``; keyword arguments go to its constructor."""
    if model == "hip":
        return HipBuilder(**config)
    if model in _FOREIGN:
        raise ImportError(f"the {model!r} backend needs the {_FOREIGN[model]} library, which torch_rechub_amd does not "
                          "bundle; use builder_factory(\"hip\"), the exact index on the MI355X")
    raise NotImplementedError(f"no retrieval backend named {model!r}; the one built here is \"hip\"")


__all__ = ["builder_factory", "BaseBuilder", "BaseIndexer", "HipBuilder", "HipIndexer", "HipIvfIndexer"]
