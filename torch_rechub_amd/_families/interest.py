"""Multi-interest user towers and list-wise scoring (csrc/interest.hip): capsule routing, the self-attentive pooling
and the list-wise logits."""
import torch

from .. import _lib
from .._opcore import _NULL, _p, _stream, require_hip


class _CapsuleFn(torch.autograd.Function):
    """CapsuleNetwork routing (reference basic/layers.py:657-712).  Types 0 / 1: x = the Linear's output U (B, L, Iu*D);
    type 2: x = the history E (B, L, D) and w the (1, L, I*D, D) weight.  Gradient through the last iteration only."""

    @staticmethod
    def forward(ctx, x, w, mask, init, kind, I, D, iters):
        B, L = int(mask.shape[0]), int(mask.shape[1])
        x = x.contiguous()
        w = w.contiguous() if w is not None else None
        dev = x.device
        cap = torch.empty((B, I, D), dtype=torch.float32, device=dev)
        sw = torch.empty((B, I, L), dtype=torch.float32, device=dev)
        s = torch.empty((B, I, D), dtype=torch.float32, device=dev)
        U, E = (None, x) if kind == 2 else (x, None)
        _lib.call("rh_capsule_fwd", _p(U), _p(E), _p(w), _p(mask), _p(init), B, L, I, D, kind, iters, _p(cap), _p(sw), _p(s),
                  _stream())
        ctx.dims = (B, L, I, D, kind)
        ctx.save_for_backward(x, w, sw, s)
        return cap

    @staticmethod
    def backward(ctx, g):
        x, w, sw, s = ctx.saved_tensors
        B, L, I, D, kind = ctx.dims
        g = g.contiguous()
        dev = g.device
        if kind != 2:
            g_u = torch.empty(x.shape, dtype=torch.float32, device=dev)
            _lib.call("rh_capsule_bwd", _p(g), _p(s), _p(sw), _NULL, B, L, I, D, kind, _p(g_u), _NULL, _NULL, _stream())
            return g_u, None, None, None, None, None, None, None
        g_e = torch.empty((B, L, D), dtype=torch.float32, device=dev)
        g_s = torch.empty((B, I, D), dtype=torch.float32, device=dev)
        _lib.call("rh_capsule_bwd", _p(g), _p(s), _p(sw), _p(w), B, L, I, D, 2, _NULL, _p(g_e), _p(g_s), _stream())
        g_w = None
        if ctx.needs_input_grad[1]:
            g_w = torch.empty(w.shape, dtype=torch.float32, device=dev)
            if B == 0:
                g_w.zero_()
            else:
                nch = _lib.call("rh_capsule_wgrad_nchunks", B)
                part = torch.empty((nch, L * I * D * D), dtype=torch.float32, device=dev)
                _lib.call("rh_capsule_wgrad", _p(g_s), _p(sw), _p(x), B, L, I, D, _p(part), _stream())
                _lib.call("rh_colsum", _p(part), nch, L * I * D * D, _p(g_w), _NULL, 0, _NULL, _stream())
        return g_e, g_w, None, None, None, None, None, None


def capsule_supported(L, I, D, kind):
    return bool(_lib.call("rh_capsule_supported", int(L), int(I), int(D), int(kind)))


def capsule_routing(x, w, mask, init, kind, interest_num, embed_dim, routing_times):
    """(B, I, D) interest capsules; ``mask`` (B, L) int32 (nonzero = kept), ``init`` (B, I, L) initial logits or None."""
    require_hip(x, w, mask, init)
    return _CapsuleFn.apply(x, w, mask, init, int(kind), int(interest_num), int(embed_dim), int(routing_times))


class _SaPoolFn(torch.autograd.Function):
    """MultiInterestSA after A = tanh(E W1) W2: softmax over L of A + -1e9 (1 - mask), then A^T E (layers.py:601-608)."""

    @staticmethod
    def forward(ctx, A, E, mask):
        A, E = A.contiguous(), E.contiguous()
        B, L, I = (int(v) for v in A.shape)
        D = int(E.shape[2])
        P = torch.empty((B, L, I), dtype=torch.float32, device=A.device)
        out = torch.empty((B, I, D), dtype=torch.float32, device=A.device)
        _lib.call("rh_sa_pool_fwd", _p(A), _p(E), _p(mask), B, L, I, D, _p(P), _p(out), _stream())
        ctx.save_for_backward(P, E)
        return out

    @staticmethod
    def backward(ctx, g):
        P, E = ctx.saved_tensors
        B, L, I = (int(v) for v in P.shape)
        D = int(E.shape[2])
        g = g.contiguous()
        gA = torch.empty((B, L, I), dtype=torch.float32, device=g.device)
        gE = torch.empty((B, L, D), dtype=torch.float32, device=g.device)
        _lib.call("rh_sa_pool_bwd", _p(P), _p(E), _p(g), B, L, I, D, _p(gA), _p(gE), _stream())
        return gA, gE, None


def sa_supported(L, I, D):
    return bool(_lib.call("rh_sa_supported", int(L), int(I), int(D)))


def sa_pool(A, E, mask=None):
    """(B, I, D) = softmax_L(A + -1e9 (1 - mask))^T E for A (B, L, I), E (B, L, D), mask (B, L) int32 or None."""
    require_hip(A, E, mask)
    return _SaPoolFn.apply(A, E, mask)


class _ListwiseFn(torch.autograd.Function):
    """(B, 1 + K) logits of the list-wise retrieval models: normalised item rows, best interest by the positive."""

    @staticmethod
    def forward(ctx, u, pos, neg, temperature):
        u, neg = u.contiguous(), neg.contiguous()
        if pos.stride(1) != 1:
            pos = pos.contiguous()
        B, I, D = (int(v) for v in u.shape)
        K = int(neg.shape[1])
        dev = u.device
        logits = torch.empty((B, 1 + K), dtype=torch.float32, device=dev)
        best = torch.empty((B,), dtype=torch.int32, device=dev)
        nrm = torch.empty((B, 1 + K), dtype=torch.float32, device=dev)
        _lib.call("rh_listwise_fwd", _p(u), _p(pos), pos.stride(0), _p(neg), B, I, D, K, float(temperature), _p(logits),
                  _p(best), _p(nrm), _stream())
        ctx.temperature = float(temperature)
        ctx.save_for_backward(u, pos, neg, best, nrm)
        ctx.mark_non_differentiable(best)
        return logits, best

    @staticmethod
    def backward(ctx, g, _unused):
        u, pos, neg, best, nrm = ctx.saved_tensors
        B, I, D = (int(v) for v in u.shape)
        K = int(neg.shape[1])
        g = g.contiguous()
        dev = g.device
        g_u = torch.empty((B, I, D), dtype=torch.float32, device=dev)
        g_pos = torch.empty((B, D), dtype=torch.float32, device=dev)
        g_neg = torch.empty((B, K, D), dtype=torch.float32, device=dev)
        _lib.call("rh_listwise_bwd", _p(u), _p(pos), pos.stride(0), _p(neg), _p(best), _p(nrm), _p(g), B, I, D, K,
                  ctx.temperature, _p(g_u), _p(g_pos), _p(g_neg), _stream())
        return g_u, g_pos, g_neg, None


def listwise_ok(u, pos, neg):
    return (u.is_cuda and u.dtype == pos.dtype == neg.dtype == torch.float32 and u.dim() == 3 and pos.dim() == 2 and
            neg.dim() == 3 and 1 <= u.shape[1] <= _lib.H.RH_LISTWISE_MAX_I and 1 <= u.shape[2] <= _lib.H.RH_LISTWISE_MAX_D and
            pos.shape == (u.shape[0], u.shape[2])
            and neg.shape[0] == u.shape[0] and neg.shape[2] == u.shape[2] and neg.shape[1] <= _lib.H.RH_LISTWISE_MAX_K)


def listwise_logits(u, pos, neg, temperature=1.0):
    """(logits (B, 1 + K), best (B,) int32): logits = u_best . normalize([pos, neg]) / temperature, u (B, I, D) the
    normalised user vectors, pos (B, D) / neg (B, K, D) the raw item rows; best = first argmax_i u_i . normalize(pos)."""
    require_hip(u, pos, neg)
    if not listwise_ok(u, pos, neg):
        raise RuntimeError(f"torch_rechub_amd: list-wise scoring of user {tuple(u.shape)}, items {tuple(pos.shape)} / "
                           f"{tuple(neg.shape)} has no HIP kernel (I <= {_lib.H.RH_LISTWISE_MAX_I}, D <= {_lib.H.RH_LISTWISE_MAX_D}, "
                           f"K <= {_lib.H.RH_LISTWISE_MAX_K}, float32)")
    return _ListwiseFn.apply(u, pos, neg, float(temperature))
