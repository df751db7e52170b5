"""Float64 restatement of the three stand-alone kernel pairs of csrc/match.hip that every retrieval model trains through,
forward and backward (numpy only; not a test module).  tests/test_match_host.py pins these functions to torch's float64
autograd of the reference's own formulation (gather_inbatch_logits over the score matrix, F.normalize, CrossEntropyLoss);
tests/test_gpu_match_fm_shapes.py compares the kernels with them.  The stand-alone FM term has its restatement in
oracle/ctr_oracle.py (fm_forward / fm_backward).

F.normalize clamps its norm with clamp_min: where eps wins, the denominator is a constant and the gradient is g / eps.
"""
import numpy as np

F64 = np.float64


# ---- in-batch logits: logits[i, 0] = u_i . v_(row0 + i), logits[i, 1 + k] = u_i . v_neg[i, k] --------------------------------
def inbatch_index(neg, B, row0=0):
    """(B, 1 + K) item rows a user row scores against: its own positive, then its negatives."""
    neg = np.asarray(neg, np.int64).reshape(B, -1)
    return np.concatenate([row0 + np.arange(B, dtype=np.int64)[:, None], neg], 1)


def inbatch_forward(u, v, neg, row0=0):
    u, v = np.asarray(u, F64), np.asarray(v, F64)
    idx = inbatch_index(neg, u.shape[0], row0)
    assert idx.min() >= 0 and idx.max() < v.shape[0]
    return np.einsum("bd,bkd->bk", u, v[idx])


def inbatch_backward(u, v, neg, g, row0=0):
    """(g_u, g_v) for the gradient g (B, 1 + K) of the logits; an item row named more than once collects every term."""
    u, v, g = (np.asarray(t, F64) for t in (u, v, g))
    idx = inbatch_index(neg, u.shape[0], row0)
    g_u = np.einsum("bk,bkd->bd", g, v[idx])
    g_v = np.zeros_like(v)
    np.add.at(g_v, idx.reshape(-1), (g[:, :, None] * u[:, None, :]).reshape(-1, u.shape[1]))
    return g_u, g_v


# ---- L2 normalise: y = x / max(||x||, eps) ---------------------------------------------------------------------------------------
def l2norm_forward(x, eps=1e-12):
    x = np.asarray(x, F64)
    n = np.sqrt((x * x).sum(1, keepdims=True))
    return x / np.maximum(n, eps)


def l2norm_backward(x, g, eps=1e-12):
    """(g - y (g . y)) / ||x|| where ||x|| > eps; g / eps where the norm was clamped."""
    x, g = np.asarray(x, F64), np.asarray(g, F64)
    n = np.sqrt((x * x).sum(1, keepdims=True))
    y = x / np.maximum(n, eps)
    proj = np.where(n > eps, (g * y).sum(1, keepdims=True), 0.0)
    return (g - y * proj) / np.maximum(n, eps)


# ---- mean cross-entropy over (B, C) logits; target None = class 0 everywhere ----------------------------------------------------
def _lse(x):
    m = x.max(1, keepdims=True)
    return m + np.log(np.exp(x - m).sum(1, keepdims=True))


def ce_terms(logits, target=None):
    """(B,) per-row terms logsumexp(row) - row[target]."""
    x = np.asarray(logits, F64)
    t = np.zeros(x.shape[0], np.int64) if target is None else np.asarray(target, np.int64)
    assert t.shape == (x.shape[0],) and t.min() >= 0 and t.max() < x.shape[1]
    return _lse(x)[:, 0] - x[np.arange(x.shape[0]), t]


def ce_forward(logits, target=None):
    return float(ce_terms(logits, target).mean())


def ce_backward(logits, target=None, g_loss=1.0):
    x = np.asarray(logits, F64)
    B = x.shape[0]
    t = np.zeros(B, np.int64) if target is None else np.asarray(target, np.int64)
    p = np.exp(x - _lse(x))
    p[np.arange(B), t] -= 1.0
    return p * (float(g_loss) / B)
