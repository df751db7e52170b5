"""SINE's sparse-interest chain (csrc/sine.hip)."""
import torch

from .. import _lib
from .._opcore import _NULL, _p, _stream, require_hip


class _SineInterestFn(torch.autograd.Function):
    """sine.py:94-118 between the w_1 / w_k1 / w_3 products and h_3: (phi (B, K, E), xhat (B, S, E), idx (B, K) int32)."""

    @staticmethod
    def forward(ctx, X, Y, a1, a2, mask, C):
        X, Y, a1, a2, C = X.contiguous(), Y.contiguous(), a1.contiguous(), a2.contiguous(), C.contiguous()
        B, S, E = (int(v) for v in X.shape)
        K, T = int(a2.shape[2]), int(C.shape[0])
        dev = X.device
        idx = torch.empty((B, K), dtype=torch.int32, device=dev)
        phi = torch.empty((B, K, E), dtype=torch.float32, device=dev)
        xhat = torch.empty((B, S, E), dtype=torch.float32, device=dev)
        P1 = torch.empty((B, S), dtype=torch.float32, device=dev)
        P2 = torch.empty((B, K, S), dtype=torch.float32, device=dev)
        PU = torch.empty((B, K, S), dtype=torch.float32, device=dev)
        _lib.call("rh_sine_interest_fwd", _p(X), _p(Y), _p(a1), _p(a2), _p(mask), _p(C), B, S, E, T, K, _p(idx), _p(phi),
                  _p(xhat), _p(P1), _p(P2), _p(PU), _stream())
        ctx.save_for_backward(X, Y, C, mask, idx, P1, P2, PU)
        ctx.mark_non_differentiable(idx)
        return phi, xhat, idx

    @staticmethod
    def backward(ctx, g_phi, g_xhat, _unused):
        X, Y, C, mask, idx, P1, P2, PU = ctx.saved_tensors
        B, S, E = (int(v) for v in X.shape)
        K, T = int(idx.shape[1]), int(C.shape[0])
        dev = X.device
        g_phi, g_xhat = g_phi.contiguous(), g_xhat.contiguous()  # (autograd materialises an unused output's as zeros)
        g_X = torch.empty((B, S, E), dtype=torch.float32, device=dev)
        g_Y = torch.empty((B, S, E), dtype=torch.float32, device=dev)
        g_a1 = torch.empty((B, S), dtype=torch.float32, device=dev)
        g_a2 = torch.empty((B, S, K), dtype=torch.float32, device=dev)
        g_C = torch.empty((T, E), dtype=torch.float32, device=dev)
        if B == 0:
            g_C.zero_()
        else:
            nch = _lib.query("rh_sine_nchunks", B)
            rows = torch.empty((B, K, E), dtype=torch.float32, device=dev)
            part = torch.empty((nch, T * E), dtype=torch.float32, device=dev)
            _lib.call("rh_sine_interest_bwd", _p(X), _p(Y), _p(C), _p(idx), _p(P1), _p(P2), _p(PU), _p(g_phi), _p(g_xhat), B,
                      S, E, T, K, _p(g_X), _p(g_Y), _p(g_a1), _p(g_a2), _p(rows), _p(part), _stream())
            _lib.call("rh_colsum", _p(part), nch, T * E, _p(g_C), _NULL, 0, _NULL, _stream())
        return g_X, g_Y, g_a1, g_a2, None, g_C


class _SineAggregateFn(torch.autograd.Function):
    """sine.py:122-128 after h_3 w_5: v (B, E).  The backward recomputes the chain from the inputs (in fp64, csrc/sine.hip)."""

    @staticmethod
    def forward(ctx, xhat, a3, mask, phi, inv_t):
        xhat, a3, phi = xhat.contiguous(), a3.contiguous(), phi.contiguous()
        B, S, E = (int(v) for v in xhat.shape)
        K = int(phi.shape[1])
        v = torch.empty((B, E), dtype=torch.float32, device=xhat.device)
        _lib.call("rh_sine_aggregate_fwd", _p(xhat), _p(a3), _p(mask), _p(phi), inv_t, B, S, E, K, _p(v), _stream())
        ctx.inv_t = inv_t
        ctx.save_for_backward(xhat, a3, mask, phi)
        return v

    @staticmethod
    def backward(ctx, g_v):
        xhat, a3, mask, phi = ctx.saved_tensors
        B, S, E = (int(v) for v in xhat.shape)
        K = int(phi.shape[1])
        dev = xhat.device
        g_v = g_v.contiguous()
        g_xhat = torch.empty((B, S, E), dtype=torch.float32, device=dev)
        g_a3 = torch.empty((B, S), dtype=torch.float32, device=dev)
        g_phi = torch.empty((B, K, E), dtype=torch.float32, device=dev)
        _lib.call("rh_sine_aggregate_bwd", _p(xhat), _p(a3), _p(mask), _p(phi), _p(g_v), ctx.inv_t, B, S, E, K, _p(g_xhat),
                  _p(g_a3), _p(g_phi), _stream())
        return g_xhat, g_a3, None, g_phi, None


def sine_supported(S, E, T, K):
    return bool(_lib.query("rh_sine_supported", int(S), int(E), int(T), int(K)))


def _sine_check(what, tensors, mask, S, E, T, K):
    if any(t.dtype != torch.float32 for t in tensors) or mask.dtype != torch.int32 or not mask.is_contiguous():
        raise ValueError(f"torch_rechub_amd: {what} takes float32 tensors and a contiguous int32 mask")
    if not sine_supported(S, E, T, K):
        from ..models.matching._listwise import no_kernel
        raise no_kernel(f"{what} at seq_max_len {S}, embedding_dim {E}, num_concept {T}, num_intention {K} "
                        f"(S <= {_lib.H.RH_SINE_MAX_S}, E <= {_lib.H.RH_SINE_MAX_E}, T <= {_lib.H.RH_SINE_MAX_T}, "
                        f"K <= min(T, {_lib.H.RH_SINE_MAX_K}))")


def sine_interests(X, Y, a1, a2, mask, C):
    """(phi (B, K, E), xhat (B, S, E), idx (B, K) int32) of SINE's sparse-interest extraction (sine.py:94-118) from
    X = x_u and Y = X w_3 (B, S, E), a1 (B, S) = tanh(X w_1) w_2, a2 (B, S, K) = tanh(X w_k1) w_k2, mask (B, S) int32
    (1 = kept) and the concept table C (T, E).  idx are the chosen concepts in descending score order."""
    require_hip(X, Y, a1, a2, mask, C)
    B, S, E = (int(v) for v in X.shape)
    if Y.shape != X.shape or a1.shape != (B, S) or a2.dim() != 3 or a2.shape[:2] != (B, S) or mask.shape != (B, S) or \
            C.dim() != 2 or C.shape[1] != E:
        raise ValueError("sine_interests: X, Y (B, S, E), a1 (B, S), a2 (B, S, K), mask (B, S), C (T, E) expected")
    _sine_check("SINE's interest extraction", (X, Y, a1, a2, C), mask, S, E, int(C.shape[0]), int(a2.shape[2]))
    return _SineInterestFn.apply(X, Y, a1, a2, mask, C)


def sine_aggregate(xhat, a3, mask, phi, temperature):
    """v (B, E) of SINE's interest aggregation (sine.py:122-128) from xhat (B, S, E), a3 (B, S) = tanh(xhat w_4) w_5,
    mask (B, S) int32 and phi (B, K, E)."""
    require_hip(xhat, a3, mask, phi)
    B, S, E = (int(v) for v in xhat.shape)
    if a3.shape != (B, S) or mask.shape != (B, S) or phi.dim() != 3 or phi.shape[0] != B or phi.shape[2] != E:
        raise ValueError("sine_aggregate: xhat (B, S, E), a3 (B, S), mask (B, S), phi (B, K, E) expected")
    K = int(phi.shape[1])
    _sine_check("SINE's interest aggregation", (xhat, a3, phi), mask, S, E, max(K, 1), K)
    return _SineAggregateFn.apply(xhat, a3, mask, phi, 1.0 / float(temperature))
