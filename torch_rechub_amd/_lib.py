"""ctypes binding of ``csrc/librechub_hip.so``.  The C ABI is written down once, in ``include/rechub_hip.h``: the argument
and return types, the ``RhPackItem`` layout and the ``RH_*`` constants used here are parsed from it (``_header.py``).

There is deliberately no CPU fallback: if the shared library is missing or a symbol cannot be
resolved the import of any op fails loudly (``RuntimeError``), and every op refuses tensors that
are not on a HIP device.
"""
import ctypes
import os
import types

from . import _header

_HERE = os.path.dirname(os.path.abspath(__file__))
# RECHUB_HIP_LIB: load another build of the same ABI (kernel experiments); default is the in-tree library
LIB_PATH = os.environ.get("RECHUB_HIP_LIB") or os.path.join(_HERE, "csrc", "librechub_hip.so")

# Parsed once, at import (modules read the RH_* integer macros through H when they are imported); nothing on the call path.
if not os.path.exists(_header.PATH):
    raise RuntimeError(f"rechub_hip.h not found at {_header.PATH}: the ctypes signatures are derived from it "
                       "(there is no fallback table).")
with open(_header.PATH) as _f:
    _FUNCTIONS, _PACK_FIELDS, _MACROS = _header.parse(_f.read())
H = types.SimpleNamespace(**_MACROS)
SIGNATURES = {name: argtypes for name, (_, argtypes) in _FUNCTIONS.items()}  # name -> argtypes
_RESTYPES = {name: restype for name, (restype, _) in _FUNCTIONS.items()}
# Functions whose integer return value is a result, not a status: those that take no pointer, hence launch nothing and
# write nothing.  rh_set_tuning is the one exception (a status); rh_last_error returns a string.
_VALUE_RETURNING = {name for name, argtypes in SIGNATURES.items() if ctypes.c_void_p not in argtypes and
                    _RESTYPES[name] is not ctypes.c_char_p and name != "rh_set_tuning"}
ABI_VERSION = H.RH_ABI_VERSION
_lib = None


def ab(name, default=True):
    """Same-box A/B switches of benchmarks, ONE environment variable: RECHUB_AB="chain=0,ahead=0,lookahead=0" turns the named
    round-4 paths off (each has a bit- or tolerance-pinned twin; the tests flip the module attributes instead)."""
    for item in filter(None, os.environ.get("RECHUB_AB", "").split(",")):
        k, _, v = item.partition("=")
        if k.strip() == name:
            return v.strip() not in ("0", "false", "off")
    return default


class PackItem(ctypes.Structure):
    """RhPackItem of include/rechub_hip.h (one parameter's gradient sources for rh_pack_grads)."""
    _fields_ = _PACK_FIELDS


def load():
    """Load the shared library once; raise RuntimeError (never fall back) when it is unusable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(f"librechub_hip.so not found at {LIB_PATH}. Build it with "
                           f"`python -c 'import __graft_entry__ as g; g.build()'` or `{_HERE}/csrc/build.sh` "
                           "(there is no CPU fallback for the HIP hot path).")
    # torch must be imported first so that the HIP runtime already mapped by torch (same SONAME
    # libamdhip64.so.7) is the one this library binds to: one runtime, shared streams.
    import torch  # noqa: F401
    lib = ctypes.CDLL(LIB_PATH)
    for name, argtypes in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RuntimeError(f"librechub_hip.so does not export {name}; rebuild it") from e
        fn.argtypes = argtypes
        fn.restype = _RESTYPES[name]
    got = lib.rh_abi_version()
    if got != ABI_VERSION:
        raise RuntimeError(f"librechub_hip.so ABI {got} != expected {ABI_VERSION}; rebuild it")
    _lib = lib
    # RECHUB_TUNE="key=value,key=value": rh_set_tuning knobs of include/rechub_hip.h (kernel experiments)
    for item in filter(None, os.environ.get("RECHUB_TUNE", "").split(",")):
        k, v = item.split("=")
        if lib.rh_set_tuning(int(k), int(v)) != 0:
            raise RuntimeError(f"RECHUB_TUNE: rh_set_tuning({k}, {v}) rejected")
    return lib


def call(name, *args):
    """Invoke a status-returning entry point; raise RuntimeError with the library's message on failure."""
    lib = load()
    rc = getattr(lib, name)(*args)
    if name in _VALUE_RETURNING:
        return rc
    if rc != 0:
        msg = lib.rh_last_error()
        raise RuntimeError(f"{name} failed (rc={rc}): {msg.decode() if msg else ''}")
    return 0


def query(name, *args, out=(ctypes.c_int,)):
    """The answer of an entry point that writes it to host integers behind its last arguments (the ``*_supported``,
    ``*_plan`` and block-count queries): the value, or a tuple of them when ``out`` names several types."""
    outs = [t(0) for t in out]
    call(name, *args, *[ctypes.c_void_p(ctypes.addressof(o)) for o in outs])
    return outs[0].value if len(outs) == 1 else tuple(o.value for o in outs)
