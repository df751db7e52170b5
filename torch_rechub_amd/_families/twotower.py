"""Two-tower score tails and the SENET field gate (csrc/twotower.hip)."""
import torch

from .. import _lib
from .._opcore import _NULL, _p, _stream, require_hip


def _rows(t):
    """A float32 (B, D) tensor whose rows are contiguous (any row stride), as the row-strided entry points read it."""
    return t if t.stride(1) == 1 and t.stride(0) >= t.shape[1] else t.contiguous()


class _BandLogitsFn(torch.autograd.Function):
    """YoutubeSBC's (B, 1 + n_neg) scores straight from the tower outputs: no (B, B) tensor; the item gradient is a gather."""

    @staticmethod
    def forward(ctx, u, v, w, K1, temperature, eps):
        require_hip(u, v, w)
        u, v, w = _rows(u), _rows(v), w.contiguous()
        B, D = u.shape
        dev = u.device
        logits = torch.empty((B, K1), dtype=torch.float32, device=dev)
        norms = torch.empty((2, B), dtype=torch.float32, device=dev)
        _lib.call("rh_band_logits_fwd", _p(u), u.stride(0), _p(v), v.stride(0), _p(w), B, D, K1, temperature, eps, _p(logits),
                  _p(norms[0]), _p(norms[1]), _stream())
        ctx.save_for_backward(u, v, norms)
        ctx.cfg = (K1, temperature, eps)
        return logits

    @staticmethod
    def backward(ctx, g):
        u, v, norms = ctx.saved_tensors
        K1, temperature, eps = ctx.cfg
        B, D = u.shape
        g = g.contiguous()
        g_u = torch.empty((B, D), dtype=torch.float32, device=u.device)
        g_v = torch.empty((B, D), dtype=torch.float32, device=u.device)
        _lib.call("rh_band_logits_bwd", _p(u), u.stride(0), _p(v), v.stride(0), _p(norms[0]), _p(norms[1]), _p(g), B, D, K1,
                  temperature, eps, _p(g_u), _p(g_v), _stream())
        return g_u, g_v, None, None, None, None


def _f32_rows(*tensors):
    first = tensors[0]
    return all(t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape == first.shape for t in tensors) and \
        first.shape[0] >= 1 and 1 <= first.shape[1] <= _lib.H.RH_TWOTOWER_MAX_D


def band_logits_ok(u, v, w, n_neg):
    return (_f32_rows(u, v) and w.is_cuda and w.dtype == torch.float32 and tuple(w.shape) == (u.shape[0],) and
            0 <= int(n_neg) < u.shape[0])


def band_logits(u, v, w, n_neg, temperature=1.0, eps=1e-8):
    """logits[i, k] = (cosine_similarity(u_i, v_j, eps) - log w_j) / temperature with j = (i + k) mod B, k = 0..n_neg:
    ``((torch.cosine_similarity(u.unsqueeze(1), v, dim=2) - torch.log(w))[index0, index1] / temperature).view(B, -1)`` for
    YoutubeSBC's band ``index1 = (i + k) mod B``.  ``w`` gets no gradient (it is a DenseFeature input)."""
    return _BandLogitsFn.apply(u, v, w, int(n_neg) + 1, float(temperature), float(eps))


class _PairCosineFn(torch.autograd.Function):
    """(sum(n(hu) n(hp)), sum(n(hu) n(hn))), n = F.normalize(., p=2, dim=1, eps): one launch each way."""

    @staticmethod
    def forward(ctx, hu, hp, hn, eps):
        require_hip(hu, hp, hn)
        hu, hp, hn = _rows(hu), _rows(hp), _rows(hn)
        B, D = hu.shape
        dev = hu.device
        score = torch.empty((2, B), dtype=torch.float32, device=dev)
        nrm = torch.empty((3, B), dtype=torch.float32, device=dev)
        _lib.call("rh_pair_cosine_fwd", _p(hu), hu.stride(0), _p(hp), hp.stride(0), _p(hn), hn.stride(0), B, D, eps,
                  _p(score[0]), _p(score[1]), _p(nrm), _stream())
        ctx.save_for_backward(hu, hp, hn, nrm)
        ctx.eps = eps
        return score[0], score[1]

    @staticmethod
    def backward(ctx, g_pos, g_neg):
        hu, hp, hn, nrm = ctx.saved_tensors
        B, D = hu.shape
        g_pos, g_neg = g_pos.contiguous(), g_neg.contiguous()
        grads = torch.empty((3, B, D), dtype=torch.float32, device=hu.device)
        _lib.call("rh_pair_cosine_bwd", _p(hu), hu.stride(0), _p(hp), hp.stride(0), _p(hn), hn.stride(0), _p(nrm), _p(g_pos),
                  _p(g_neg), B, D, ctx.eps, _p(grads[0]), _p(grads[1]), _p(grads[2]), _stream())
        return grads[0], grads[1], grads[2], None


def pair_cosine_scores_ok(hu, hp, hn):
    return _f32_rows(hu, hp, hn)


def pair_cosine_scores(hu, hp, hn, eps=1e-12):
    """(pos, neg) (B,) each: the cosine of every user row with its positive and its negative item row, from the RAW tower
    outputs -- ``(F.normalize(hu) * F.normalize(hp)).sum(1), (F.normalize(hu) * F.normalize(hn)).sum(1)``."""
    return _PairCosineFn.apply(hu, hp, hn, float(eps))


class _SenetFn(torch.autograd.Function):
    """SENETLayer.forward over the (B, F, D) field block; the weight gradients through per-workgroup partials + rh_colsum."""

    @staticmethod
    def forward(ctx, x, w1, w2):
        require_hip(x, w1, w2)
        B, F, D = x.shape
        if x.stride(2) != 1 or x.stride(1) != D or x.stride(0) < F * D:
            x = x.contiguous()
        w1, w2 = w1.contiguous(), w2.contiguous()
        R = w1.shape[0]
        dev = x.device
        y = torch.empty((B, F, D), dtype=torch.float32, device=dev)
        z = torch.empty((B, F), dtype=torch.float32, device=dev)
        h = torch.empty((B, R), dtype=torch.float32, device=dev)
        a = torch.empty((B, F), dtype=torch.float32, device=dev)
        _lib.call("rh_senet_fwd", _p(x), x.stride(0), _p(w1), _p(w2), B, F, R, D, _p(y), _p(z), _p(h), _p(a), _stream())
        ctx.save_for_backward(x, w1, w2, z, h, a)
        return y

    @staticmethod
    def backward(ctx, g):
        x, w1, w2, z, h, a = ctx.saved_tensors
        B, F, D = x.shape
        R = w1.shape[0]
        dev = x.device
        if g.stride(2) != 1 or g.stride(1) != D or g.stride(0) < F * D:
            g = g.contiguous()
        g_x = torch.empty((B, F, D), dtype=torch.float32, device=dev)
        nb = _lib.query("rh_twotower_nblocks", B)
        partial = torch.empty((nb, 2 * R * F), dtype=torch.float32, device=dev)
        _lib.call("rh_senet_bwd", _p(x), x.stride(0), _p(w1), _p(w2), _p(z), _p(h), _p(a), _p(g), g.stride(0), B, F, R, D,
                  _p(g_x), _p(partial), _stream())
        g_w = torch.empty((2, R * F), dtype=torch.float32, device=dev)
        _lib.call("rh_colsum", _p(partial), nb, 2 * R * F, _p(g_w), _NULL, 0, _NULL, _stream())
        return g_x, g_w[0].view(R, F), g_w[1].view(F, R)


def senet_ok(x, w1, w2):
    return (x.is_cuda and x.dtype == torch.float32 and x.dim() == 3 and x.shape[0] >= 1 and
            1 <= x.shape[1] <= _lib.H.RH_SENET_MAX_F and 1 <= x.shape[2] <= _lib.H.RH_SENET_MAX_D and
            w1.is_cuda and w2.is_cuda and w1.dtype == torch.float32 and
            w2.dtype == torch.float32 and w1.dim() == 2 and w1.shape[1] == x.shape[1] and 1 <= w1.shape[0] <= x.shape[1] and
            tuple(w2.shape) == (x.shape[1], w1.shape[0]))


def senet(x, w1, w2):
    """``x * relu(relu(x.mean(-1) @ w1.T) @ w2.T).unsqueeze(-1)`` for x (B, F, D) -- a view of the fused gather's (B, F D)
    output is read in place --, w1 (R, F), w2 (F, R): SENETLayer.forward as one launch each way."""
    return _SenetFn.apply(x, w1, w2)
