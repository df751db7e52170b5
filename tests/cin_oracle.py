"""numpy float64 restatement of the Compressed Interaction Network (reference basic/layers.py:322-368): one layer and the
whole stack, forward and backward.  The 1 x 1 Conv1d over the (B, F * Hp, D) product is the contraction
``pre[b, o, d] = bias[o] + sum_{f, h} W[o, f, h] x0[b, f, d] h[b, h, d]`` with ``W = conv.weight[:, :, 0].reshape(Ho, F, Hp)``.
ReLU's derivative at 0 is 0, as torch's."""
import numpy as np


def layer_pre(x0, h, w, bias):
    """Pre-activation (B, Ho, D) of one layer: x0 (B, F, D), h (B, Hp, D), w (Ho, F * Hp[, 1]), bias (Ho,)."""
    F, Hp = x0.shape[1], h.shape[1]
    W = np.asarray(w, np.float64).reshape(-1, F, Hp)
    return np.einsum("ofh,bfd,bhd->bod", W, x0, h, optimize=True) + np.asarray(bias, np.float64)[None, :, None]


def layer_fwd(x0, h, w, bias):
    return np.maximum(layer_pre(x0, h, w, bias), 0.0)


def layer_bwd(x0, h, w, bias, g_y, pre=None):
    """(g_x0, g_h, g_w (Ho, F * Hp, 1), g_bias) of layer_fwd for the upstream g_y (B, Ho, D); ``pre``: the pre-activation
    whose sign decides the ReLU (default: the float64 one)."""
    F, Hp = x0.shape[1], h.shape[1]
    W = np.asarray(w, np.float64).reshape(-1, F, Hp)
    pre = layer_pre(x0, h, w, bias) if pre is None else pre
    gp = np.where(pre > 0, g_y, 0.0)
    g_x0 = np.einsum("bod,ofh,bhd->bfd", gp, W, h, optimize=True)
    g_h = np.einsum("bod,ofh,bfd->bhd", gp, W, x0, optimize=True)
    g_w = np.einsum("bod,bfd,bhd->ofh", gp, x0, h, optimize=True).reshape(W.shape[0], F * Hp, 1)
    return g_x0, g_h, g_w, gp.sum((0, 2))


def _state(sd):
    return {k: np.asarray(v, np.float64) for k, v in sd.items()}


def cin_fwd(x, sd, split_half, cache=None):
    """(B, 1) output of the stack for the state_dict ``sd`` (conv_layers.{i}.weight / .bias, fc.weight / .bias)."""
    sd = _state(sd)
    n = len([k for k in sd if k.startswith("conv_layers.") and k.endswith(".weight")])
    x = np.asarray(x, np.float64)
    h, outs = x, []
    for i in range(n):
        w, b = sd[f"conv_layers.{i}.weight"], sd[f"conv_layers.{i}.bias"]
        pre = layer_pre(x, h, w, b)
        y = np.maximum(pre, 0.0)
        if cache is not None:
            cache.append((h, pre))
        if split_half and i != n - 1:
            half = y.shape[1] // 2
            outs.append(y[:, :half])
            h = y[:, half:]
        else:
            outs.append(y)
            h = y
    s = np.concatenate(outs, 1).sum(2)
    if cache is not None:
        cache.append(s)
    return s @ sd["fc.weight"].T + sd["fc.bias"]


def cin_bwd(x, sd, split_half, g_out):
    """(g_x, {parameter name: gradient}) of cin_fwd for the upstream g_out (B, 1)."""
    sd = _state(sd)
    x = np.asarray(x, np.float64)
    cache = []
    cin_fwd(x, sd, split_half, cache)
    s = cache.pop()
    n = len(cache)
    g_out = np.asarray(g_out, np.float64)
    grads = {"fc.weight": g_out.T @ s, "fc.bias": g_out.sum(0)}
    g_s = g_out @ sd["fc.weight"]  # (B, sum of kept channels)
    D = x.shape[2]
    kept = [(p.shape[1] // 2 if (split_half and i != n - 1) else p.shape[1]) for i, (_, p) in enumerate(cache)]
    starts = np.concatenate([[0], np.cumsum(kept)])
    g_x = np.zeros_like(x)
    g_next = None  # gradient reaching the part of layer i's output that feeds layer i + 1
    for i in reversed(range(n)):
        h, pre = cache[i]
        g_keep = np.repeat(g_s[:, starts[i]:starts[i + 1], None], D, axis=2)
        if split_half and i != n - 1:
            g_y = np.concatenate([g_keep, g_next], 1)
        else:
            g_y = g_keep if g_next is None else g_keep + g_next
        w, b = sd[f"conv_layers.{i}.weight"], sd[f"conv_layers.{i}.bias"]
        g_x0, g_h, g_w, g_b = layer_bwd(x, h, w, b, g_y, pre)
        grads[f"conv_layers.{i}.weight"], grads[f"conv_layers.{i}.bias"] = g_w, g_b
        g_x += g_x0
        g_next = g_h
    return g_x + g_next, grads
