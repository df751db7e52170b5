"""RQ-VAE's residual quantizer (csrc/rq.hip)."""
import ctypes

import torch

from .. import _lib
from .._opcore import _p, _stream, require_hip, _ptr_array, _int_array


def rq_supported(E, sizes):
    """Whether csrc/rq.hip takes rows of width E against codebooks of these sizes (E <= RH_RQ_MAX_E, sizes <= RH_RQ_MAX_CODES, <= RH_RQ_MAX_L
    levels)."""
    sizes = [int(v) for v in sizes]
    arr = _int_array(sizes)
    return bool(_lib.query("rh_rq_supported", int(E), len(sizes), ctypes.cast(arr, ctypes.c_void_p)))


def _rq_check(x, codebooks):
    require_hip(x, *codebooks)
    if x.dim() != 2 or not codebooks or any(c.dim() != 2 or c.shape[1] != x.shape[1] for c in codebooks):
        raise ValueError("residual quantizer: rows (N, E) and codebooks (n_e, E) expected")
    if x.dtype != torch.float32 or any(c.dtype != torch.float32 for c in codebooks):
        raise ValueError("torch_rechub_amd: the residual quantizer takes float32 tensors")
    sizes = [int(c.shape[0]) for c in codebooks]
    if not rq_supported(int(x.shape[1]), sizes):
        from ..models.matching._listwise import no_kernel
        raise no_kernel(f"the residual quantizer at e_dim {int(x.shape[1])} with codebook sizes {sizes} "
                        f"(e_dim <= {_lib.H.RH_RQ_MAX_E}, sizes <= {_lib.H.RH_RQ_MAX_CODES}, at most {_lib.H.RH_RQ_MAX_L} levels)")
    return sizes


def rq_forward(r_in, codebooks, l0=0, l1=None, given=0, idx=None, sse=None):
    """The levels [l0, l1) of the residual quantizer on r_in (N, E), the residual entering level l0: (idx (N, L) int32,
    r_out (N, E), x_q = r_in - r_out, sse (L,)).  Level l takes its index from ``idx`` instead of searching it when bit l of
    ``given`` is set.  ``idx`` and ``sse`` of an earlier call are continued in place.  No autograd."""
    codebooks = [c.detach().contiguous() for c in codebooks]
    r_in = r_in.detach().contiguous()
    sizes = _rq_check(r_in, codebooks)
    N, E = (int(v) for v in r_in.shape)
    L = len(sizes)
    l1 = L if l1 is None else int(l1)
    if not 0 <= l0 < l1 <= L:
        raise ValueError(f"residual quantizer: level range [{l0}, {l1}) of {L}")
    dev = r_in.device
    whole = l0 == 0 and l1 == L  # every element of idx and sse is written by this call
    if idx is None:
        if given:
            raise ValueError("residual quantizer: given levels need their indices")
        idx = (torch.empty if whole and N else torch.zeros)((N, L), dtype=torch.int32, device=dev)
    if sse is None:
        sse = (torch.empty if whole and N else torch.zeros)((L,), dtype=torch.float32, device=dev)
    r_out = torch.empty((N, E), dtype=torch.float32, device=dev)
    x_q = torch.empty((N, E), dtype=torch.float32, device=dev)
    if N:
        blocks, _ = _lib.query("rh_rq_nchunks", N, out=(ctypes.c_int, ctypes.c_int))
        part = torch.empty((blocks, l1 - l0), dtype=torch.float32, device=dev)
        _lib.call("rh_rq_fwd", _p(r_in), ctypes.cast(_ptr_array(codebooks), ctypes.c_void_p),
                  ctypes.cast(_int_array(sizes), ctypes.c_void_p), N, E, L, int(l0), l1, int(given), _p(idx), _p(r_out),
                  _p(x_q), _p(part), _p(sse), _stream())
    return idx, r_out, x_q, sse


def _sinkhorn_level(r, C, epsilon, iters):
    """Index of every row at a Sinkhorn level, as torch ops on the device (rqvae.py:248-258)."""
    from ..models.generative.rqvae import VectorQuantizer, sinkhorn_algorithm
    d = torch.sum(r**2, dim=1, keepdim=True) + torch.sum(C**2, dim=1, keepdim=True).t() - 2 * torch.matmul(r, C.t())
    d = VectorQuantizer.center_distance_for_constraint(d).double()
    Q = sinkhorn_algorithm(d, epsilon, iters)
    if torch.isnan(Q).any() or torch.isinf(Q).any():
        print("Sinkhorn Algorithm returns nan/inf values.")
    return torch.argmax(Q, dim=-1).to(torch.int32)


class _ResidualQuantizeFn(torch.autograd.Function):
    """(x_q (N, E), loss (), idx (N, L) int64) of rqvae.py:382-398 on x (N, E); sk = ((level, epsilon, iterations), ...)."""

    @staticmethod
    def forward(ctx, x, beta, sk, *codebooks):
        x = x.contiguous()
        cbs = [c.detach().contiguous() for c in codebooks]
        N, E = (int(v) for v in x.shape)
        L = len(cbs)
        idx, sse, r, l0, given, x_q = None, None, x, 0, 0, None
        for level, eps, iters in sk:  # the cold path: the levels before a Sinkhorn level, then its index as torch ops
            if level > l0:
                idx, r, _, sse = rq_forward(r, cbs, l0, level, given, idx, sse)
            if idx is None:
                idx = torch.zeros((N, L), dtype=torch.int32, device=x.device)
            idx[:, level] = _sinkhorn_level(r, cbs[level], eps, iters)
            l0, given = level, given | (1 << level)
        idx, r, x_q, sse = rq_forward(r, cbs, l0, L, given, idx, sse)
        if l0 > 0:
            x_q = x - r
        loss = sse.sum() * ((1.0 + beta) / (float(N) * E * L)) if N else sse.sum() * float("nan")
        ctx.beta = beta
        ctx.save_for_backward(x, idx, *cbs)
        out_idx = idx.to(torch.int64)
        ctx.mark_non_differentiable(out_idx)
        return x_q, loss, out_idx

    @staticmethod
    def backward(ctx, g_xq, g_loss, _unused):
        x, idx, *cbs = ctx.saved_tensors
        N, E = (int(v) for v in x.shape)
        sizes = [int(c.shape[0]) for c in cbs]
        dev = x.device
        total = sum(sizes) * E
        g_x = torch.empty((N, E), dtype=torch.float32, device=dev)
        g_C = torch.empty((total,), dtype=torch.float32, device=dev)
        if N == 0:
            g_C.zero_()
        else:
            _, nch = _lib.query("rh_rq_nchunks", N, out=(ctypes.c_int, ctypes.c_int))
            part = torch.empty((nch, total), dtype=torch.float32, device=dev)
            g_loss, g_xq = g_loss.to(torch.float32).contiguous(), g_xq.contiguous()
            _lib.call("rh_rq_bwd", _p(x), ctypes.cast(_ptr_array(cbs), ctypes.c_void_p),
                      ctypes.cast(_int_array(sizes), ctypes.c_void_p), _p(idx), _p(g_xq), _p(g_loss),
                      float(ctx.beta), N, E, len(cbs), _p(g_x), _p(part), _p(g_C), _stream())
        grads, off = [], 0
        for n in sizes:
            grads.append(g_C[off:off + n * E].view(n, E))
            off += n * E
        return (g_x, None, None, *grads)


def residual_quantize(x, codebooks, beta, sk_epsilons=None, sk_iters=100, use_sk=True):
    """(x_q, loss, indices) of the RQ-VAE's residual quantizer (rqvae.py:241-274 per level, :382-398 across levels) on x
    (..., E) and the codebooks [(n_e, E), ...]: x_q = x + (sum of the chosen codes - x).detach(), loss = the mean over
    levels of codebook_loss + beta commitment_loss, indices int64 of shape x.shape[:-1] + (L,).  A level with ``use_sk`` and
    ``sk_epsilons[l] > 0`` takes its index from the Sinkhorn assignment (torch ops on the device; ``sk_iters`` an int or one
    per level); every other level, the distances, arg-min, gathers, losses and the backward are csrc/rq.hip."""
    codebooks = list(codebooks)
    if not codebooks:
        raise ValueError("residual_quantize: at least one codebook expected")
    flat = x.reshape(-1, x.shape[-1])
    _rq_check(flat, codebooks)
    L = len(codebooks)
    eps = [0.0] * L if sk_epsilons is None else [float(e) for e in sk_epsilons]
    if len(eps) != L:
        raise ValueError(f"residual_quantize: {len(eps)} sk_epsilons for {L} codebooks")
    iters = [int(sk_iters)] * L if isinstance(sk_iters, int) else [int(v) for v in sk_iters]
    sk = tuple((l, eps[l], iters[l]) for l in range(L) if use_sk and eps[l] > 0)
    x_q, loss, idx = _ResidualQuantizeFn.apply(flat, float(beta), sk, *codebooks)
    return x_q.view(x.shape), loss, idx.view(tuple(x.shape[:-1]) + (L,))
