"""What every kernel family needs to reach the C ABI (``include/rechub_hip.h``): device pointers, the current stream, the
HIP-only check and the device-resident dropout counter, whose per-device state exists once, here.  ops.py and the modules
of ``_families`` import these by name; this module imports neither."""
import ctypes

import torch

from . import _lib

_NULL = ctypes.c_void_p(0)


_empty_stub = {}


def _p(t):
    """Device pointer of a tensor for the C ABI.  An EMPTY tensor has a null data_ptr(); the entry points check their
    pointers before they look at the sizes (and then return at once for B = 0), so empties are passed as a pointer to
    a small per-device stub allocation."""
    if t is None:
        return _NULL
    if t.numel() == 0:
        stub = _empty_stub.get(t.device)
        if stub is None:
            stub = torch.zeros(64, dtype=torch.float32, device=t.device)
            _empty_stub[t.device] = stub
        return ctypes.c_void_p(stub.data_ptr())
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def require_hip(*tensors):
    """Fail loudly for anything that is not a HIP tensor (there is no CPU fallback)."""
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("torch_rechub_amd: this op runs only on a HIP device (MI355X); got a "
                               f"{t.device} tensor. There is no CPU fallback by design.")
    _lib.load()


_rng_state = {}


def _dropout_rng(device):
    """Device-resident (seed, call counter) of the fused dropout; seeded from torch's generator on first use."""
    st = _rng_state.get(device)
    if st is None:
        st = torch.tensor([torch.initial_seed() & 0x7FFFFFFFFFFFFFFF, 0, 0, 0], dtype=torch.int64).to(device)
        _rng_state[device] = st
    return st


def _ptr_array(tensors):
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[t.data_ptr() for t in tensors])


def _int_array(values):
    import ctypes
    return (ctypes.c_int * len(values))(*values)


def _attn_view_ok(t, B, L, W):
    """(B, L, W) with unit column stride and rows B L apart by one stride (a contiguous tensor or a column block of one)."""
    return t.stride(2) == 1 and t.stride(1) >= W and (B <= 1 or t.stride(0) == L * t.stride(1))
