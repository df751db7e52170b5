"""Patch an installed ``torch_rechub`` in place so that its model zoo and trainers run on the MI355X hot path
(INTEGRATION.md section B — the binding a maintainer of the reference would add as ``torch_rechub/_hip.py``).

The reference has no plugin layer: its models bind their layers BY NAME at import time
(``from ...basic.layers import FM, LR, MLP, EmbeddingLayer``, torch_rechub/models/ranking/deepfm.py:10), so swapping
the implementation means rebinding those names in ``torch_rechub.basic.layers`` AND in every already-imported
``torch_rechub.*`` module that holds a reference to the original class.  ``enable()`` does exactly that, at these levels:

  layers    EmbeddingLayer, InputMask, the pooling layers, LR, MLP, FM, CrossNetwork, CrossNetV2, CrossNetMix, Dice and
            the Feature descriptors -> an UNMODIFIED reference model class (e.g. the source of
            torch_rechub/models/ranking/deepfm.py as it stands) then builds and runs on the HIP layers;
  models    DeepFM, WideDeep, DCN, DCNv2, DIN, ... -> the fused forwards (one gather launch emits the MLP input, FM and LR);
  trainers  CTRTrainer / MatchTrainer / MTLTrainer -> TableAdam, device-resident loader, hipGraph step, RCCL data parallel.
  data      EmbDataset of ``utils.data`` (its own flag).
  serving   ``builder_factory`` of ``serving`` learns ``"hip"`` (when that package can be imported at all: it imports annoy,
            faiss and pymilvus unconditionally), and ``utils.match`` gains ``ExactIndex`` (its own flag).

Constructor signatures, attribute names and ``state_dict`` keys are the reference's at every level
(tests/test_integration_patch.py).  ``disable()`` restores the original bindings.
"""
import importlib
import sys

_LAYERS = ("EmbeddingLayer", "InputMask", "SumPooling", "AveragePooling", "ConcatPooling", "LR", "MLP", "FM",
           "CrossNetwork", "CrossNetV2", "CrossNetMix", "SENETLayer", "BiLinearInteractionLayer", "InteractingLayer",
           "CrossLayer", "FFM", "CEN", "CIN", "MultiInterestSA", "CapsuleNetwork", "HSTULayer", "HSTUBlock")
_FEATURES = ("DenseFeature", "SparseFeature", "SequenceFeature")
_ACTIVATIONS = ("Dice", "activation_layer")
_MODELS = {"ranking": ("DeepFM", "WideDeep", "DCN", "DCNv2", "DIN", "DIEN", "BST", "AFM", "AutoInt", "EDCN", "FiBiNet",
                       "DeepFFM", "FatDeepFFM"),
           "matching": ("DSSM", "YoutubeDNN", "MIND", "ComirecSA", "ComirecDR", "GRU4Rec", "NARM", "STAMP", "SINE",
                        "SASRec", "FaceBookDSSM", "YoutubeSBC"),
           "multi_task": ("SharedBottom", "ESMM", "MMOE", "PLE", "AITM"),
           "generative": ("HSTUModel", "HLLMModel", "RQVAEModel")}
# classes a reference module defines beside its model and does not re-export from the sub-package
_MODEL_PARTS = {"matching.sasrec": ("PointWiseFeedForward",),
                "matching.dssm_senet": ("DSSM",),  # its own class of that name; models.matching exports ours as DSSMSENet
                "generative.hllm": ("HLLMTransformerBlock",),
                "generative.rqvae": ("VectorQuantizer", "ResidualVectorQuantizer")}
_TRAINERS = ("CTRTrainer", "MatchTrainer", "MTLTrainer", "SeqTrainer")
# classes the reference keeps in a module of their own, not re-exported from the sub-package: (module, names)
_TRAINER_PARTS = {"trainers.rqvae_trainer": ("Trainer",)}
_DATA = {"utils.data": ("EmbDataset",)}

_undo = []  # (module, attribute, original object or _ABSENT)
_ABSENT = object()  # the attribute did not exist before enable()


def _rebind_everywhere(root, original, replacement):
    """Point every attribute of every imported ``<root>.*`` module that IS ``original`` at ``replacement``."""
    prefix = root + "."
    for modname, mod in list(sys.modules.items()):
        if mod is None or not (modname == root or modname.startswith(prefix)):
            continue
        for attr, val in list(vars(mod).items()):
            if val is original:
                setattr(mod, attr, replacement)
                _undo.append((mod, attr, original))


def _swap(root, ref_modname, amd_module, names):
    try:
        ref_mod = importlib.import_module(ref_modname)
    except ImportError:
        return []
    done = []
    for name in names:
        ours = getattr(amd_module, name, None)
        theirs = getattr(ref_mod, name, None)
        if ours is None or theirs is None or ours is theirs:
            continue
        _rebind_everywhere(root, theirs, ours)
        if getattr(ref_mod, name) is not ours:  # not reached by identity (e.g. re-exported under another object)
            setattr(ref_mod, name, ours)
            _undo.append((ref_mod, name, theirs))
        done.append(f"{ref_modname}.{name}")
    return done


def _enable_serving(package):
    """``"hip"`` for the reference's ``builder_factory`` and ``ExactIndex`` beside its ``Annoy``."""
    from . import serving as amd_serving
    from .utils import match as amd_match
    done = []
    try:
        ref_serving = importlib.import_module(f"{package}.serving")
    except (ImportError, OSError):  # a backend library that is absent or does not load: nothing to teach
        ref_serving = None
    theirs = getattr(ref_serving, "builder_factory", None)
    if theirs is not None and not getattr(theirs, "_rh_hip", False):

        def builder_factory(model, **builder_config):
            if model == "hip":
                return amd_serving.HipBuilder(**builder_config)
            return theirs(model, **builder_config)

        builder_factory._rh_hip = True
        builder_factory.__doc__ = theirs.__doc__
        _rebind_everywhere(package, theirs, builder_factory)
        done.append(f"{package}.serving.builder_factory")
    try:
        ref_match = importlib.import_module(f"{package}.utils.match")
    except ImportError:
        ref_match = None
    if ref_match is not None and getattr(ref_match, "ExactIndex", None) is not amd_match.ExactIndex:
        _undo.append((ref_match, "ExactIndex", getattr(ref_match, "ExactIndex", _ABSENT)))
        ref_match.ExactIndex = amd_match.ExactIndex
        done.append(f"{package}.utils.match.ExactIndex")
    return done


def enable(layers=True, models=True, trainers=True, package="torch_rechub", data=True, serving=True):
    """Rebind the reference package's hot-path classes to the HIP implementations.  Returns the list of patched names.

    Call it after ``import torch_rechub`` (and its ``models`` / ``trainers`` sub-packages, if the level is wanted) and
    before models are built.  ``data`` is a level of its own: the data-set classes of ``utils.data`` that have a mirror here
    (``EmbDataset``).  ``serving`` is another: the retrieval index (``builder_factory("hip")``, ``ExactIndex``); where
    the reference's ``serving`` package cannot be imported, that half is skipped without an error.  Idempotent."""
    from . import basic, trainers as amd_trainers
    from .basic import activation, features, layers as amd_layers
    importlib.import_module(package)
    done = []
    if layers:
        done += _swap(package, f"{package}.basic.features", features, _FEATURES)
        done += _swap(package, f"{package}.basic.activation", activation, _ACTIVATIONS)
        done += _swap(package, f"{package}.basic.layers", amd_layers, _LAYERS)
    if models:
        for sub, names in _MODELS.items():
            amd_sub = importlib.import_module(f"{__package__}.models.{sub}")
            done += _swap(package, f"{package}.models.{sub}", amd_sub, names)
        for sub, names in _MODEL_PARTS.items():
            amd_sub = importlib.import_module(f"{__package__}.models.{sub}")
            done += _swap(package, f"{package}.models.{sub}", amd_sub, names)
    if trainers:
        done += _swap(package, f"{package}.trainers", amd_trainers, _TRAINERS)
        for sub, names in _TRAINER_PARTS.items():
            done += _swap(package, f"{package}.{sub}", importlib.import_module(f"{__package__}.{sub}"), names)
    if data:
        for sub, names in _DATA.items():
            done += _swap(package, f"{package}.{sub}", importlib.import_module(f"{__package__}.{sub}"), names)
    if serving:
        done += _enable_serving(package)
    del basic
    return done


def disable():
    """Undo every rebinding made by ``enable`` (latest first)."""
    while _undo:
        mod, attr, original = _undo.pop()
        if original is _ABSENT:
            delattr(mod, attr)
        else:
            setattr(mod, attr, original)
