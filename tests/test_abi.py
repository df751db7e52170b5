"""The C-ABI shared library loads without a GPU and exports every symbol include/rechub_hip.h declares.
No compute is launched here (argument validation only)."""
import ctypes
import os
import re

import pytest

from conftest import ROOT


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "rechub_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(rh_[a-z0-9_]+)\s*\(", text)))


def test_header_declares_the_hot_path():
    syms = declared_symbols()
    for must in ("rh_embed_fwd", "rh_embed_bwd", "rh_embed_scatter_rows", "rh_cross_fwd", "rh_cross_bwd",
                 "rh_adam_dense", "rh_seq_pool_fwd", "rh_fm_fwd", "rh_batch_gather"):
        assert must in syms


def test_library_exports_every_declared_symbol():
    from torch_rechub_amd import _lib
    lib = _lib.load()
    for name in declared_symbols():
        assert hasattr(lib, name), f"{name} declared in rechub_hip.h but not exported"
        assert name in _lib.SIGNATURES, f"{name} has no ctypes signature in _lib.SIGNATURES"
    assert lib.rh_abi_version() == _lib.ABI_VERSION


def test_argument_errors_are_reported_not_crashed():
    from torch_rechub_amd import _lib
    null = ctypes.c_void_p(0)
    with pytest.raises(RuntimeError, match="null descriptor"):
        _lib.call("rh_embed_fwd", null, null, 1, 4, 2, 16, null, 0, 32, null, 32, null, null, null, null, null, 0, null,
                  null)
    fake = ctypes.c_void_p(4096)  # never dereferenced: validation fails first
    with pytest.raises(RuntimeError, match="embed_dim 6 unsupported"):
        _lib.call("rh_embed_fwd", fake, fake, 1, 4, 2, 6, null, 0, 12, fake, 12, null, null, null, null, null, 0, null,
                  null)
    with pytest.raises(RuntimeError, match="layers per call unsupported"):
        _lib.call("rh_cross_fwd", fake, 8, fake, 8, fake, fake, 4, 8, 9, fake, 8, null)
    assert _lib.call("rh_cross_max_layers", 429) == 4
    assert _lib.call("rh_cross_max_layers", 4096) == 0
    assert _lib.call("rh_embed_bwd_nchunks", 4096, 0) == 16
    assert _lib.call("rh_cross_bwd_nblocks", 4096) == 256


def test_missing_library_fails_loudly(monkeypatch):
    from torch_rechub_amd import _lib
    monkeypatch.setattr(_lib, "_lib", None)
    monkeypatch.setattr(_lib, "LIB_PATH", "/nonexistent/librechub_hip.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _lib.load()


def test_every_declaration_has_a_derived_signature():
    """The ctypes signatures come from the header: the parser may not skip a declaration the regex above finds."""
    from torch_rechub_amd import _lib
    syms = declared_symbols()
    assert not [name for name in syms if name not in _lib.SIGNATURES]
    assert len(_lib.SIGNATURES) == len(syms) == len(_lib._RESTYPES)


def test_loaded_functions_carry_the_derived_types():
    from torch_rechub_amd import _lib
    lib = _lib.load()
    for name in declared_symbols():
        fn = getattr(lib, name)
        assert list(fn.argtypes) == _lib.SIGNATURES[name], name
        assert fn.restype is _lib._RESTYPES[name], name
    assert lib.rh_embed_fwd.argtypes[9:11] == [ctypes.c_void_p, ctypes.c_int64]  # float* out, int64_t out_stride
    assert lib.rh_last_error.restype is ctypes.c_char_p and lib.rh_linear_wgrad_workspace.restype is ctypes.c_int64
    assert lib.rh_cross_max_layers.restype is ctypes.c_int and lib.rh_dice_fwd.argtypes[2] is ctypes.c_float


MINI_HEADER = """
#define RH_ABI_VERSION 1
#define RH_E_BADARG (-1)  /* an argument error */
typedef struct RhPackItem {
  uint64_t src; /* device pointer */
  int64_t numel;
} RhPackItem;
int rh_a(const float* x, int64_t n, float eps, void** out);  // a comment
const char* rh_b(void);
"""


def test_parser_maps_plain_c_and_raises_on_the_rest():
    from torch_rechub_amd import _header
    functions, fields, macros = _header.parse(MINI_HEADER)
    assert functions == {"rh_a": (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int64, ctypes.c_float, ctypes.c_void_p]),
                         "rh_b": (ctypes.c_char_p, [])}
    assert fields == [("src", ctypes.c_uint64), ("numel", ctypes.c_int64)]
    assert macros == {"RH_ABI_VERSION": 1, "RH_E_BADARG": -1}
    for bad, message in (("int rh_c(const float* x, size_t n);", "cannot map `size_t n`"),
                         ("int rh_c(double scale, void* stream);", "cannot map `double scale`"),
                         ("int rh_c(RhPackItem item);", "cannot map `RhPackItem item`"),
                         ("int rh_c(void (*done)(int), void* stream);", "cannot map"),
                         ("double rh_c(int n);", "return type `double`"),
                         ("#define RH_SCALE 0.5", "not an integer constant"),
                         ("int rh_c(int n, void* stream", "cut off before `;`")):
        with pytest.raises(ValueError, match=re.escape(message)):
            _header.parse(MINI_HEADER + bad + "\n")


def test_pack_item_layout_is_the_headers():
    from torch_rechub_amd import _lib
    assert ctypes.sizeof(_lib.PackItem) == 48
    text = open(os.path.join(ROOT, "include", "rechub_hip.h")).read()
    body = re.search(r"typedef struct RhPackItem \{(.*?)\} RhPackItem;", text, flags=re.S).group(1)
    names = re.findall(r"(\w+);", body)
    assert [f for f, _ in _lib.PackItem._fields_] == names == ["src", "add", "nparts", "stride", "numel", "dst_offset"]


def test_header_macros_are_exposed():
    from torch_rechub_amd import _lib
    assert len(vars(_lib.H)) == 92
    assert (_lib.H.RH_E_BADARG, _lib.H.RH_E_UNSUPPORTED) == (-1, -2)
    assert (_lib.H.RH_FLAG_INDEX_OOB, _lib.H.RH_FLAG_TARGET_OOB, _lib.H.RH_ERR_GATE_TIMEOUT, _lib.H.RH_FLAG_SESSION_EMPTY,
            _lib.H.RH_FLAG_SESSION_SHORT) == (1, 2, 64, 128, 256)
    assert (_lib.H.RH_TUNE_DEFERRED_GRID, _lib.H.RH_TUNE_SWEEP_GATE_NS, _lib.H.RH_GATE_WORDS) == (8, 13, 16)


def test_status_and_value_returns_are_told_apart():
    """A function without a pointer parameter returns a value; rh_set_tuning is the exception and returns a status."""
    from torch_rechub_amd import _lib
    assert len(_lib._VALUE_RETURNING) == 32 and "rh_set_tuning" not in _lib._VALUE_RETURNING
    assert "rh_last_error" not in _lib._VALUE_RETURNING and "rh_linear_wgrad_workspace" in _lib._VALUE_RETURNING
    with pytest.raises(RuntimeError, match="rh_set_tuning failed"):
        _lib.call("rh_set_tuning", 3, 0)  # key 3 was removed: the header says it fails
    assert _lib.call("rh_cross_max_layers", 4096) == 0  # a value of 0, not a status


@pytest.mark.parametrize("key", [1, 4, 5, 6, 10, 11, 14, 15, 16])
def test_removed_tuning_keys_are_rejected(key):
    """The keys of the measured-and-rejected experiments went with their variants (the two that were accepted and ignored
    included): rh_set_tuning fails for them as it does for key 3, whatever the value, and the header defines no macro for them."""
    from torch_rechub_amd import _lib
    for value in (0, 1):
        with pytest.raises(RuntimeError, match="rh_set_tuning failed"):
            _lib.call("rh_set_tuning", key, value)
    assert key not in {v for k, v in vars(_lib.H).items() if k.startswith("RH_TUNE_")}


def test_forward_path_key_takes_its_three_values_only():
    from torch_rechub_amd import _lib
    for value in (3, 4, -1):
        with pytest.raises(RuntimeError, match="rh_set_tuning failed"):
            _lib.call("rh_set_tuning", _lib.H.RH_TUNE_FWD_PATH, value)
    for value in (1, 2, 0):
        assert _lib.call("rh_set_tuning", _lib.H.RH_TUNE_FWD_PATH, value) == 0


def test_a_missing_argument_is_a_type_error():
    from torch_rechub_amd import _lib
    with pytest.raises(TypeError):
        _lib.call("rh_cross_max_layers")


# Every kernel shape limit, as the kernels and ops.py held it before the header did.  A limit changes on purpose in two
# places: include/rechub_hip.h and this table.
SHAPE_LIMITS = {
    "RH_EMBED_MAX_D": 128, "RH_EMBED_MAX_LR_FD": 12288, "RH_SEQ_POOL_MAX_D": 128, "RH_DIN_ATT_MAX_D": 128,
    "RH_CROSS_MAX_D": 2048, "RH_CROSS_MIX_MAX_D": 2048, "RH_CROSS_MIX_MAX_E": 16,
    "RH_CROSS_MOE_MAX_L": 8, "RH_CROSS_MOE_MAX_E": 16, "RH_CROSS_MOE_MAX_R": 64, "RH_CROSS_MOE_MAX_ER": 256,
    "RH_DICE_MAX_C": 2048, "RH_BN_DICE_MAX_C": 512, "RH_DIN_ATT_L1_MAX_D": 16, "RH_DIN_ATT_L1_MAX_N": 256,
    "RH_INBATCH_MAX_D": 1024, "RH_L2NORM_MIN_D": 4, "RH_L2NORM_MAX_D": 4096, "RH_CE_MAX_C": 1024,
    "RH_HEAD_MAX_K": 1024, "RH_HEAD_BN_MAX_K": 256, "RH_LINEAR_BNACT_MAX_K": 1024,
    "RH_CROSS_V2_MAX_M": 16384, "RH_CROSS_V2_MAX_D": 1024, "RH_WGRAD_LONG_MIN_B": 32768, "RH_BN_PRE_MAX_CHUNKS": 128,
    "RH_ADAM_MAX_TENSORS": 128, "RH_ADAM_MAX_RING": 1024, "RH_AUGRU_MAX_D": 32, "RH_FFM_MAX_F": 64, "RH_FFM_MAX_D": 128,
    "RH_CAPSULE_MAX_D": 64, "RH_CAPSULE_MAX_ID": 256, "RH_CAPSULE_MAX_IDD": 4096,
    "RH_SA_MAX_D": 64, "RH_SA_MAX_LI": 1024, "RH_SA_MAX_ID": 1024,
    "RH_LISTWISE_MAX_I": 16, "RH_LISTWISE_MAX_D": 64, "RH_LISTWISE_MAX_K": 1023,
    "RH_SINE_MAX_S": 64, "RH_SINE_MAX_E": 128, "RH_SINE_MAX_T": 64, "RH_SINE_MAX_K": 8,
    "RH_RQ_MAX_E": 128, "RH_RQ_MAX_CODES": 1024, "RH_RQ_MAX_L": 8,
    "RH_HSTU_MAX_L": 1024, "RH_HSTU_MAX_DH": 64, "RH_HSTU_MAX_BUCKETS": 1023,
    "RH_ATTN_MAX_L": 1024, "RH_ATTN_MAX_DH": 128, "RH_RMS_NORM_MAX_D": 1024,
    "RH_TOPK_MAX_D": 1024, "RH_TOPK_MAX_K": 256, "RH_TOPK_MAX_S": 1024, "RH_TOPK_MAX_SPLIT": 1024, "RH_IVF_MAX_NPROBE": 256,
    "RH_GRU_MAX_H": 128, "RH_ATTN_POOL_MAX_L": 1024, "RH_ATTN_POOL_MAX_W": 4096, "RH_SASREC_MAX_D": 128,
    "RH_TWOTOWER_MAX_D": 1024, "RH_SENET_MAX_F": 64, "RH_SENET_MAX_D": 256, "RH_BEAM_MAX_K": 64,
    "RH_CIN_MAX_D": 128, "RH_CIN_MAX_F": 64, "RH_CIN_MAX_HP": 256, "RH_CIN_MAX_HO": 512,
    "RH_RANK_MAX_K": 256, "RH_RANK_MAX_CUTOFFS": 8, "RH_ILD_MAX_D": 1024,
}


def test_every_shape_limit_keeps_its_value():
    from torch_rechub_amd import _lib
    have = {k: v for k, v in vars(_lib.H).items() if "_MAX_" in k or "_MIN_" in k}
    assert have == SHAPE_LIMITS
    assert len(SHAPE_LIMITS) == 73


def test_the_functions_that_returned_a_constant_are_gone():
    from torch_rechub_amd import _lib
    lib = _lib.load()
    for name in ("rh_gru_max_hidden", "rh_augru_max_dim"):
        assert name not in _lib.SIGNATURES and not hasattr(lib, name)
    assert lib.rh_abi_version() == 1
