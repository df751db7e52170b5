"""float64 restatement of csrc/encoder.hip (the post-norm encoder block behind the attention) and of one whole post-norm
encoder layer, in plain torch on the CPU; gradients by autograd on the float64 graph.  The three dropout sites take their
keep flags as arguments (None: no dropout), scaled by 1 / (1 - p) here."""
import math

import torch

F64 = torch.float64


def layer_norm(y, gamma, beta, eps):
    mean = y.mean(-1, keepdim=True)
    var = ((y - mean)**2).mean(-1, keepdim=True)
    return (y - mean) / torch.sqrt(var + eps) * gamma + beta


def drop(t, keep, p):
    return t if keep is None else t * keep.reshape(t.shape).to(F64) / (1.0 - p)


def block(attn, x, P, slope=0.01, p=0.0, keep_o=None, keep_h=None, keep_f=None, eps=1e-5):
    """(out, u) for attn, x (M, D) and P = dict(wo, bo, g1, be1, w1, b1, w2, b2, g2, be2); u (M, F) the pre-activations."""
    y1 = x + drop(attn @ P["wo"].T + P["bo"], keep_o, p)
    x1 = layer_norm(y1, P["g1"], P["be1"], eps)
    u = x1 @ P["w1"].T + P["b1"]
    a = drop(torch.where(u > 0, u, slope * u), keep_h, p)
    y2 = x1 + drop(a @ P["w2"].T + P["b2"], keep_f, p)
    return layer_norm(y2, P["g2"], P["be2"], eps), u


def attention(x, w_in, b_in, H, key_mask):
    """Multi-head self-attention (B, L, D) before out_proj; key_mask (B, L) bool, True = attend."""
    B, L, D = x.shape
    dh = D // H
    q, k, v = ((x @ w_in.T + b_in).view(B, L, 3, H, dh).permute(2, 0, 3, 1, 4))  # each (B, H, L, dh)
    s = (q / math.sqrt(dh)) @ k.transpose(-1, -2)
    if key_mask is not None:
        s = s.masked_fill(~key_mask[:, None, None, :], -math.inf)
    return (torch.softmax(s, -1) @ v).permute(0, 2, 1, 3).reshape(B, L, D)


def layer(x, w_in, b_in, H, key_mask, P, slope=0.01, eps=1e-5):
    """One post-norm encoder layer on x (B, L, D) without dropout: (out (B, L, D), u)."""
    B, L, D = x.shape
    out, u = block(attention(x, w_in, b_in, H, key_mask).reshape(B * L, D), x.reshape(B * L, D), P, slope, eps=eps)
    return out.view(B, L, D), u


def layer_tensors(mod):
    """The block's parameters of an nn.TransformerEncoderLayer under the names ``block`` takes."""
    att = mod.self_attn
    return dict(wo=att.out_proj.weight, bo=att.out_proj.bias, g1=mod.norm1.weight, be1=mod.norm1.bias, w1=mod.linear1.weight,
                b1=mod.linear1.bias, w2=mod.linear2.weight, b2=mod.linear2.bias, g2=mod.norm2.weight, be2=mod.norm2.bias)


def layer_params(mod):
    """(w_in, b_in, P) of an nn.TransformerEncoderLayer as float64 leaves."""
    def leaf(t):
        return t.detach().cpu().to(F64).requires_grad_(True)
    att = mod.self_attn
    return leaf(att.in_proj_weight), leaf(att.in_proj_bias), {k: leaf(v) for k, v in layer_tensors(mod).items()}
