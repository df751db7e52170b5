"""tests/encoder_oracle.py is the reference's layer: at p = 0 it equals nn.TransformerEncoderLayer(activation=LeakyReLU,
batch_first) in float64 on the CPU under a key-padding mask, to 1e-12 of the largest magnitude (both are float64 chains
of the same length; 1e-12 is four decimal orders above their rounding)."""
import pytest
import torch
from torch import nn

import encoder_oracle as EO


@pytest.mark.parametrize("B,L,D,H,F", [(3, 8, 12, 2, 40), (2, 9, 32, 4, 2048)])
def test_oracle_layer_is_the_library_layer(B, L, D, H, F):
    torch.manual_seed(B + L)
    mod = nn.TransformerEncoderLayer(D, H, dim_feedforward=F, dropout=0.0, activation=nn.LeakyReLU(), batch_first=True).double()
    with torch.no_grad():
        for prm in mod.parameters():  # (the biases start at zero and the LayerNorms at one)
            prm.add_(0.1 * torch.randn_like(prm))
    x = torch.randn(B, L, D, dtype=torch.float64, requires_grad=True)
    keep = torch.ones(B, L, dtype=torch.bool)
    keep[0, :L // 2] = False   # padded at the front
    keep[1, L // 2 + 1:-1] = False  # padded inside, the last key kept
    g = torch.randn(B, L, D, dtype=torch.float64)
    want = mod(x, src_key_padding_mask=~keep)
    want.backward(g)
    want_gx, x.grad = x.grad, None
    w_in, b_in, P = EO.layer_params(mod)
    got, _ = EO.layer(x, w_in, b_in, H, keep, P)
    got.backward(g)
    pairs = [(got, want), (x.grad, want_gx), (w_in.grad, mod.self_attn.in_proj_weight.grad), (P["w1"].grad, mod.linear1.weight.grad),
             (P["w2"].grad, mod.linear2.weight.grad), (P["g1"].grad, mod.norm1.weight.grad), (P["be2"].grad, mod.norm2.bias.grad),
             (P["wo"].grad, mod.self_attn.out_proj.weight.grad), (P["b1"].grad, mod.linear1.bias.grad)]
    for a, b in pairs:
        assert float((a - b).detach().abs().max()) <= 1e-12 * float(b.detach().abs().max())
