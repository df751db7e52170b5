"""Float64 restatement of the three two-tower stages of csrc/twotower.hip, forward and backward, and of the eval-mode forward
of the three models around them (numpy only; not a test module).  tests/test_twotower_host.py pins these functions to the
reference's recorded numbers (tests/golden/twotower_layers.npz, model_*.npz); tests/test_gpu_twotower.py compares the kernels
with them.

F.normalize clamps its norm with clamp_min: where eps wins the denominator is a constant.  torch.cosine_similarity clamps
its two norms in place outside autograd: the gradient treats the clamped value as the norm itself (d||u||/du = u / ||u||,
0 for a zero row).  Both rules are pinned by the recorded gradients of twotower_layers.npz.
"""
import json

import numpy as np

F64 = np.float64


# ---- YoutubeSBC's score tail: logits[i, k] = (cos(u_i, v_j) - log w_j) / T, j = (i + k) mod B -------------------------------
def band_index(B, n_neg):
    k1 = n_neg + 1
    rows = np.repeat(np.arange(B), k1)
    return rows, (rows + np.tile(np.arange(k1), B)) % B


def band_forward(u, v, w, n_neg, temperature, eps=1e-8):
    u, v, w = (np.asarray(t, F64) for t in (u, v, w))
    B = u.shape[0]
    assert n_neg + 1 <= B
    nu, nv = np.sqrt((u * u).sum(1)), np.sqrt((v * v).sum(1))
    i, j = band_index(B, n_neg)
    cos = (u[i] * v[j]).sum(1) / (np.maximum(nu[i], eps) * np.maximum(nv[j], eps))
    return ((cos - np.log(w[j])) / temperature).reshape(B, n_neg + 1)


def band_backward(u, v, g, n_neg, temperature, eps=1e-8):
    """(g_u, g_v) for the gradient g (B, 1 + n_neg) of the logits; the sample weights get none."""
    u, v, g = (np.asarray(t, F64) for t in (u, v, g))
    B = u.shape[0]
    nu, nv = np.sqrt((u * u).sum(1)), np.sqrt((v * v).sum(1))
    Nu, Nv = np.maximum(nu, eps), np.maximum(nv, eps)
    g_u, g_v = np.zeros_like(u), np.zeros_like(v)
    for i in range(B):
        for k in range(n_neg + 1):
            j = (i + k) % B
            s = g[i, k] / temperature
            cos = u[i] @ v[j] / (Nu[i] * Nv[j])
            g_u[i] += s * (v[j] / (Nu[i] * Nv[j]) - (cos * u[i] / (Nu[i] * nu[i]) if nu[i] > 0 else 0.0))
            g_v[j] += s * (u[i] / (Nu[i] * Nv[j]) - (cos * v[j] / (Nv[j] * nv[j]) if nv[j] > 0 else 0.0))
    return g_u, g_v


# ---- FaceBookDSSM's score tail: pos = n(hu) . n(hp), neg = n(hu) . n(hn), n = x / max(||x||, eps) ---------------------------
def _normalize(x, eps):
    n = np.sqrt((x * x).sum(1, keepdims=True))
    return x / np.maximum(n, eps), n


def pair_forward(hu, hp, hn, eps=1e-12):
    (u, _), (p, _), (n, _) = (_normalize(np.asarray(t, F64), eps) for t in (hu, hp, hn))
    return (u * p).sum(1), (u * n).sum(1)


def _normalize_backward(x, g, eps):
    """Gradient of n(x) against g: (g - y (g . y)) / ||x||, or g / eps where the norm was clamped."""
    y, n = _normalize(x, eps)
    proj = np.where(n > eps, (g * y).sum(1, keepdims=True), 0.0)
    return (g - y * proj) / np.maximum(n, eps)


def pair_backward(hu, hp, hn, g_pos, g_neg, eps=1e-12):
    hu, hp, hn = (np.asarray(t, F64) for t in (hu, hp, hn))
    g_pos, g_neg = np.asarray(g_pos, F64)[:, None], np.asarray(g_neg, F64)[:, None]
    (u, _), (p, _), (n, _) = (_normalize(t, eps) for t in (hu, hp, hn))
    return (_normalize_backward(hu, g_pos * p + g_neg * n, eps), _normalize_backward(hp, g_pos * u, eps),
            _normalize_backward(hn, g_neg * u, eps))


# ---- SENETLayer: z = mean_d x, h = relu(W1 z), a = relu(W2 h), y = x a[..., None] -----------------------------------------
def senet_forward(x, w1, w2):
    x, w1, w2 = (np.asarray(t, F64) for t in (x, w1, w2))
    z = x.mean(2)
    h = np.maximum(z @ w1.T, 0.0)
    a = np.maximum(h @ w2.T, 0.0)
    return x * a[:, :, None]


def senet_backward(x, w1, w2, g):
    """(g_x, g_w1, g_w2); ReLU's derivative at exactly 0 is 0."""
    x, w1, w2, g = (np.asarray(t, F64) for t in (x, w1, w2, g))
    z = x.mean(2)
    h = np.maximum(z @ w1.T, 0.0)
    a = np.maximum(h @ w2.T, 0.0)
    g_a = (g * x).sum(2) * (a > 0)
    g_w2 = g_a.T @ h
    g_h = (g_a @ w2) * (h > 0)
    g_w1 = g_h.T @ z
    g_z = g_h @ w1
    return g * a[:, :, None] + g_z[:, :, None] / x.shape[2], g_w1, g_w2


def hinge_loss(pos, neg, margin=2.0):
    pos, neg = np.asarray(pos, F64).reshape(-1), np.asarray(neg, F64)
    return np.maximum(neg.max(-1) - pos + margin, 0.0).mean()


# ---- eval-mode forward of the three models from a fixture's state ------------------------------------------------------------
def _embed(sd, x, features):
    cols = []
    for f in features:
        table = np.asarray(sd["embedding.embed_dict.%s.weight" % (f["shared_with"] or f["name"])], F64)
        idx = np.asarray(x[f["name"]])
        e = table[idx]
        if f["kind"] == "SequenceFeature":
            assert f["pooling"] == "mean" and f["padding_idx"] is None  # (no masked position: a plain mean over the history)
            e = e.mean(1)
        cols.append(e)
    return np.concatenate(cols, 1)


def _mlp_eval(sd, prefix, h):
    """MLP(output_layer=False) in eval mode: per layer Linear, BatchNorm1d on its running statistics, ReLU or PReLU."""
    layer = 0
    while "%s.mlp.%d.weight" % (prefix, layer) in sd:
        key = lambda k, name: np.asarray(sd["%s.mlp.%d.%s" % (prefix, k, name)], F64)  # noqa: E731
        h = h @ key(layer, "weight").T + key(layer, "bias")
        h = (h - key(layer + 1, "running_mean")) / np.sqrt(key(layer + 1, "running_var") + 1e-5)
        h = h * key(layer + 1, "weight") + key(layer + 1, "bias")
        slope_key = "%s.mlp.%d.weight" % (prefix, layer + 2)
        slope = np.asarray(sd[slope_key], F64) if slope_key in sd else 0.0
        h = np.where(h > 0, h, slope * h)
        layer += 4
    return h


def model_eval(cfg, spec_json, sd, x, n_neg=3, temperature=1.0):
    """The eval-mode outputs of a fixture's model: {"pred": ..., "user": user-mode output, "item": item-mode output}."""
    spec = json.loads(str(spec_json))
    hu = _mlp_eval(sd, "user_mlp", _tower_input(cfg, sd, x, spec["user_features"], "user_senet"))
    items = spec["pos_item_features" if cfg == "facebook_dssm" else "item_features"]
    hi = _mlp_eval(sd, "item_mlp", _tower_input(cfg, sd, x, items, "item_senet"))
    if cfg == "facebook_dssm":
        hn = _mlp_eval(sd, "item_mlp", _embed(sd, x, spec["neg_item_features"]))
        return {"pred": pair_forward(hu, hi, hn), "user": _normalize(hu, 1e-12)[0], "item": hi}
    if cfg == "youtube_sbc":
        return {"pred": band_forward(hu, hi, x["sample_weight"], n_neg, temperature), "user": hu, "item": hi}
    u, v = _normalize(hu, 1e-12)[0], _normalize(hi, 1e-12)[0]
    return {"pred": 1.0 / (1.0 + np.exp(-(u * v).sum(1) / temperature)), "user": u, "item": v}


def _tower_input(cfg, sd, x, features, senet):
    h = _embed(sd, x, features)
    if cfg != "dssm_senet":
        return h
    w1, w2 = sd[senet + ".mlp.0.weight"], sd[senet + ".mlp.2.weight"]
    fields = np.asarray(w1).shape[1]
    return senet_forward(h.reshape(h.shape[0], fields, -1), w1, w2).reshape(h.shape[0], -1)
