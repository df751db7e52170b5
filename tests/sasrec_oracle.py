"""numpy float64 restatement of SASRec's four fused stages (csrc/sasrec.hip), forward and backward, plus the causal
attention between them (for chaining a whole block) and the whole model with its BPR loss.  Dropout enters as explicit
boolean keep-masks (a multiplier on the attention weights), so a test can build them from the kernels' counter hash.  Not a
test module; imported by test_sasrec_host.py, test_gpu_sasrec.py and the dropout-oracle modules."""
import numpy as np

F64 = np.float64


def f64(a):
    return np.asarray(a, dtype=F64)


def keep_scale(p):
    """1 / (1 - p) as the kernels form it (in float32)."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))) if p > 0 else 1.0


def emb_scale(D):
    """sqrt(D) as both the reference and the kernels apply it: rounded to float32."""
    return float(np.float32(float(D)**0.5))


def _mult(keep, p, shape):
    return np.ones(shape, F64) if keep is None else f64(keep).reshape(shape) * keep_scale(p)


# ---- LayerNorm -----------------------------------------------------------------------------------------------------
def ln_fwd(x, gamma, beta, eps):
    x = f64(x)
    xc = x - x.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt((xc * xc).mean(-1, keepdims=True) + eps)
    xh = xc * rstd
    return xh * f64(gamma) + f64(beta), (xh, rstd)


def ln_bwd(g, gamma, cache):
    """-> (g_x, g_gamma, g_beta)"""
    xh, rstd = cache
    g = f64(g)
    D = g.shape[-1]
    gg = g * f64(gamma)
    g_x = rstd * (gg - gg.mean(-1, keepdims=True) - xh * (gg * xh).mean(-1, keepdims=True))
    return g_x, (g * xh).reshape(-1, D).sum(0), g.reshape(-1, D).sum(0)


# ---- input stage ---------------------------------------------------------------------------------------------------
def input_fwd(seq, e, P, keep=None, p=0.0):
    """x0 (B, L, D) = m dropout(e sqrt(D) + P[:L]); keep (B, L, D) bool or None."""
    e = f64(e)
    B, L, D = e.shape
    m = (np.asarray(seq) != 0)[..., None]
    return m * (e * emb_scale(D) + f64(P)[:L]) * _mult(keep, p, e.shape)


def input_bwd(seq, g_x0, max_len, keep=None, p=0.0):
    """-> (g_e (B, L, D), g_P (max_len, D))"""
    g = f64(g_x0)
    B, L, D = g.shape
    pre = (np.asarray(seq) != 0)[..., None] * g * _mult(keep, p, g.shape)
    g_P = np.zeros((max_len, D), F64)
    g_P[:L] = pre.sum(0)
    return pre * emb_scale(D), g_P


# ---- LayerNorm + in-projection ---------------------------------------------------------------------------------------
def attn_in_fwd(x, gamma, beta, W, b, eps):
    """-> (Q, qkv (..., 3 D), cache)"""
    x, W, b = f64(x), f64(W), f64(b)
    D = x.shape[-1]
    Q, cache = ln_fwd(x, gamma, beta, eps)
    qkv = np.concatenate([Q @ W[:D].T, x @ W[D:2 * D].T, x @ W[2 * D:].T], -1) + b
    return Q, qkv, (x, Q, cache)


def attn_in_bwd(gamma, W, cache, g_qkv, g_Q):
    """-> dict(x, gamma, beta, W, b)"""
    x, Q, ln = cache
    W, g_qkv = f64(W), f64(g_qkv)
    D = x.shape[-1]
    gq, gk, gv = g_qkv[..., :D], g_qkv[..., D:2 * D], g_qkv[..., 2 * D:]
    g_x, g_gamma, g_beta = ln_bwd(f64(g_Q) + gq @ W[:D], gamma, ln)
    g_x = g_x + gk @ W[D:2 * D] + gv @ W[2 * D:]
    r = lambda a: a.reshape(-1, D)  # noqa: E731
    g_W = np.concatenate([r(gq).T @ r(Q), r(gk).T @ r(x), r(gv).T @ r(x)], 0)
    return dict(x=g_x, gamma=g_gamma, beta=g_beta, W=g_W, b=g_qkv.reshape(-1, 3 * D).sum(0))


# ---- causal multi-head attention (no padding mask) -----------------------------------------------------------------------
def attention_fwd(qkv, H, mult=None):
    """mult: None, or the (B, H, L, L) dropout multiplier on the weights (keep flags times keep_scale(p))."""
    qkv = f64(qkv)
    B, L, D3 = qkv.shape
    D = D3 // 3
    dh = D // H
    q, k, v = (qkv[..., i * D:(i + 1) * D].reshape(B, L, H, dh).transpose(0, 2, 1, 3) for i in range(3))
    s = q @ k.transpose(0, 1, 3, 2) * dh**-0.5
    s = np.where(np.tril(np.ones((L, L), bool)), s, -np.inf)
    w = np.exp(s - s.max(-1, keepdims=True))
    w = w / w.sum(-1, keepdims=True)
    m = None if mult is None else f64(mult).reshape(B, H, L, L)
    out = ((w if m is None else w * m) @ v).transpose(0, 2, 1, 3).reshape(B, L, D)
    return out, (q, k, v, w) if m is None else (q, k, v, w, m)


def attention_bwd(g_out, cache):
    q, k, v, w = cache[:4]
    m = cache[4] if len(cache) > 4 else None
    B, H, L, dh = q.shape
    g = f64(g_out).reshape(B, L, H, dh).transpose(0, 2, 1, 3)
    g_v = (w if m is None else w * m).transpose(0, 1, 3, 2) @ g
    g_w = g @ v.transpose(0, 1, 3, 2)
    if m is not None:
        g_w = g_w * m
    g_s = w * (g_w - (g_w * w).sum(-1, keepdims=True)) * dh**-0.5
    g_q, g_k = g_s @ k, g_s.transpose(0, 1, 3, 2) @ q
    back = lambda a: a.transpose(0, 2, 1, 3).reshape(B, L, H * dh)  # noqa: E731
    return np.concatenate([back(g_q), back(g_k), back(g_v)], -1)


# ---- out-projection + residual + LayerNorm + point-wise FFN + mask ------------------------------------------------------
def ffn_fwd(attn, Q, seq, Wo, bo, gamma, beta, W1, b1, W2, b2, eps, keep1=None, keep2=None, p=0.0):
    """-> (out, dict of intermediates y, z, a and the backward's cache); keep1 / keep2 (M, D) bool or None."""
    attn, Q = f64(attn), f64(Q)
    D = attn.shape[-1]
    Wo, W1, W2 = f64(Wo).reshape(D, D), f64(W1).reshape(D, D), f64(W2).reshape(D, D)
    m = (np.asarray(seq) != 0).reshape(attn.shape[:-1])[..., None]
    y = Q + attn @ Wo.T + f64(bo)
    z, ln = ln_fwd(y, gamma, beta, eps)
    m1, m2 = _mult(keep1, p, z.shape), _mult(keep2, p, z.shape)
    a = np.maximum((z @ W1.T + f64(b1)) * m1, 0.0)
    out = m * (z + (a @ W2.T + f64(b2)) * m2)
    return out, dict(y=y, z=z, a=a, cache=(attn, z, a, ln, m, m1, m2, Wo, W1, W2))


def ffn_bwd(g_out, gamma, inter):
    """-> dict(attn, Q, Wo, bo, gamma, beta, W1, b1, W2, b2)"""
    attn, z, a, ln, m, m1, m2, Wo, W1, W2 = inter["cache"]
    D = z.shape[-1]
    r = lambda t: t.reshape(-1, D)  # noqa: E731
    go = f64(g_out) * m
    g_f = go * m2
    g_h = (g_f @ W2) * (a > 0) * m1
    g_z = go + g_h @ W1
    g_y, g_gamma, g_beta = ln_bwd(g_z, gamma, ln)
    return dict(attn=g_y @ Wo, Q=g_y, Wo=r(g_y).T @ r(attn), bo=r(g_y).sum(0), gamma=g_gamma, beta=g_beta,
                W1=r(g_h).T @ r(z), b1=r(g_h).sum(0), W2=r(g_f).T @ r(a), b2=r(g_f).sum(0))


# ---- final LayerNorm + the two logit sums -------------------------------------------------------------------------------
def head_fwd(x, gamma, beta, pos_e, neg_e, eps):
    """-> (s, pos_logits, neg_logits, cache)"""
    s, ln = ln_fwd(x, gamma, beta, eps)
    pos_e, neg_e = f64(pos_e), f64(neg_e)
    return s, (s * pos_e).sum(-1), (s * neg_e).sum(-1), (s, ln, pos_e, neg_e)


def head_bwd(g_pos, g_neg, gamma, cache, g_s=None):
    """-> dict(x, pos_e, neg_e, gamma, beta)"""
    s, ln, pos_e, neg_e = cache
    gp, gn = f64(g_pos)[..., None], f64(g_neg)[..., None]
    g = gp * pos_e + gn * neg_e + (0.0 if g_s is None else f64(g_s))
    g_x, g_gamma, g_beta = ln_bwd(g, gamma, ln)
    return dict(x=g_x, pos_e=gp * s, neg_e=gn * s, gamma=g_gamma, beta=g_beta)


# ---- the whole model: input stage, blocks, head, BPR loss ------------------------------------------------------------------
def model_fwd_bwd(sd, seq, pos, neg, H, eps, p=0.0, draw=None):
    """SASRec.forward + BPRLoss (-log sigmoid(pos - neg), mean over all B L positions) and its backward from the
    state_dict ``sd`` (numpy arrays under the model's names; the item table's logical columns).

    draw: None, or a callable draw(n) -> n boolean keep flags, called once per dropout COUNTER in the model's program
    order: the input stage (n = B L D, flat over (B, L, D)); per block the attention weights (n = B H L L, flat over
    (B, H, L, L)) and the FFN (n = 2 M D of ONE counter: dropout1 is [0, M D), dropout2 [M D, 2 M D), M = B L).

    -> dict(pos, neg, loss, grads {name: array}, kink): kink = the smallest |conv1 output| over the units dropout1 keeps,
    over all blocks (the ReLU follows dropout1)."""
    sd = {n: f64(a) for n, a in sd.items()}
    seq, pos, neg = np.asarray(seq), np.asarray(pos), np.asarray(neg)
    B, L = seq.shape
    table, P = sd["item_emb.embed_dict.seq.weight"], sd["position_emb.weight"]
    D = table.shape[1]
    n_blocks = sum(1 for n in sd if n.startswith("attention_layernorms.") and n.endswith(".weight"))
    keep0 = None if draw is None else np.asarray(draw(B * L * D)).reshape(B, L, D)
    x = input_fwd(seq, table[seq], P, keep0, p)
    caches, kink = [], float("inf")
    for b in range(n_blocks):
        pa, pm, pf, pw = (f"{s}.{b}." for s in ("attention_layernorms", "attention_layers", "forward_layernorms", "forward_layers"))
        Q, qkv, c_in = attn_in_fwd(x, sd[pa + "weight"], sd[pa + "bias"], sd[pm + "in_proj_weight"], sd[pm + "in_proj_bias"], eps)
        mult = None if draw is None else _mult(np.asarray(draw(B * H * L * L)), p, (B, H, L, L))
        att, c_att = attention_fwd(qkv, H, mult)
        k1 = k2 = None
        if draw is not None:
            both = np.asarray(draw(2 * B * L * D))
            k1, k2 = both[:B * L * D].reshape(B, L, D), both[B * L * D:].reshape(B, L, D)
        x, inter = ffn_fwd(att, Q, seq, sd[pm + "out_proj.weight"], sd[pm + "out_proj.bias"], sd[pf + "weight"], sd[pf + "bias"],
                           sd[pw + "conv1.weight"], sd[pw + "conv1.bias"], sd[pw + "conv2.weight"], sd[pw + "conv2.bias"], eps,
                           k1, k2, p)
        h1 = np.abs(inter["z"] @ sd[pw + "conv1.weight"].reshape(D, D).T + sd[pw + "conv1.bias"])
        kink = min(kink, float((h1 if k1 is None else h1[k1]).min()))
        caches.append((pa, pm, pf, pw, c_in, c_att, inter))
    s, pl, nl, c_head = head_fwd(x, sd["last_layernorm.weight"], sd["last_layernorm.bias"], table[pos], table[neg], eps)
    diff = pl - nl
    loss = float(np.mean(np.logaddexp(0.0, -diff)))
    g_diff = -1.0 / (1.0 + np.exp(diff)) / diff.size
    gh = head_bwd(g_diff, -g_diff, sd["last_layernorm.weight"], c_head)
    grads = {"last_layernorm.weight": gh["gamma"], "last_layernorm.bias": gh["beta"]}
    g_x = gh["x"]
    for pa, pm, pf, pw, c_in, c_att, inter in reversed(caches):
        gf = ffn_bwd(g_x, sd[pf + "weight"], inter)
        gi = attn_in_bwd(sd[pa + "weight"], sd[pm + "in_proj_weight"], c_in, attention_bwd(gf["attn"], c_att), gf["Q"])
        g_x = gi["x"]
        shape = sd[pw + "conv1.weight"].shape
        grads.update({pa + "weight": gi["gamma"], pa + "bias": gi["beta"], pm + "in_proj_weight": gi["W"],
                      pm + "in_proj_bias": gi["b"], pm + "out_proj.weight": gf["Wo"], pm + "out_proj.bias": gf["bo"],
                      pf + "weight": gf["gamma"], pf + "bias": gf["beta"], pw + "conv1.weight": gf["W1"].reshape(shape),
                      pw + "conv1.bias": gf["b1"], pw + "conv2.weight": gf["W2"].reshape(shape), pw + "conv2.bias": gf["b2"]})
    g_e, g_P = input_bwd(seq, g_x, P.shape[0], keep0, p)
    g_table = np.zeros_like(table)
    for ids, g in ((seq, g_e), (pos, gh["pos_e"]), (neg, gh["neg_e"])):
        np.add.at(g_table, ids.reshape(-1), g.reshape(-1, D))
    grads["item_emb.embed_dict.seq.weight"] = g_table
    grads["position_emb.weight"] = g_P
    return dict(pos=pl, neg=nl, loss=loss, grads=grads, kink=kink)
