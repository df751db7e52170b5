"""The two softmax attention families run ONE tile body (csrc/softmax_attn_tile.h) under two compile-time rules, so where
ops.softmax_attention (HLLM's rule, csrc/hllm.hip) and ops.t5_attention (T5's rule, csrc/t5attn.hip) describe the same
attention they give the same bits."""
import pytest
import torch

pytestmark = pytest.mark.gpu

# (B, L, H, dh): the first length on T5's tile path; a ragged second tile with an odd head width; three tiles and two
# column chunks
SHAPES = [(2, 9, 3, 64), (2, 70, 2, 7), (1, 130, 1, 100)]
CASES = [(s, with_table, 0.0) for s in SHAPES for with_table in (False, True)] + [(SHAPES[1], True, 0.3)]


@pytest.mark.parametrize("shape,with_table,p", CASES)
def test_causal_attention_is_bitwise_the_same_in_both_families(shape, with_table, p):
    """Causal, no mask, Lq = Lk, scale 1 and no bias or a bias table of ONE bucket (both bucket rules then give bucket 0
    everywhere): the HLLM rule's -inf above the diagonal and the T5 rule's -FLT_MAX both weigh exactly 0 in a row that
    keeps its own key, s * 1.0f is exact, and the dropout element index is the same, so out, g_q, g_k and g_v are equal
    to the bit (torch.equal does not tell -0 from +0).  Under dropout both calls start from the same device counter.

    g_bias is NOT compared: each family adds a bucket's diagonals in ascending order of its own diagonal index, i - j for
    HLLM and (j - i) + (Lq - 1) for T5, which for causal attention is the opposite order, so the two sums differ in the
    last bits by design."""
    from torch_rechub_amd import ops
    B, L, H, dh = shape
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(1000 * L + dh)
    q, k, v, gout = (torch.randn(B, L, H * dh, generator=g).to(dev) for _ in range(4))
    table = (0.5 * torch.randn(1, H, generator=g)).to(dev) if with_table else None
    rng = ops._dropout_rng(dev)
    rng0 = rng.clone()

    def run(fn):
        rng.copy_(rng0)
        qq, kk, vv = (t.clone().requires_grad_(True) for t in (q, k, v))
        tt = table.clone().requires_grad_(True) if with_table else None
        out = fn(qq, kk, vv, tt)
        out.backward(gout)
        return out.detach(), qq.grad, kk.grad, vv.grad

    hllm = run(lambda qq, kk, vv, tt: ops.softmax_attention(qq, kk, vv, H, max_seq_len=L, scale=1.0, bias_table=tt,
                                                            dropout_p=p))
    t5 = run(lambda qq, kk, vv, tt: ops.t5_attention(qq, kk, vv, H, causal=True, bias_table=tt, bidirectional=False,
                                                     dropout_p=p))
    for name, x, y in zip(("out", "g_q", "g_k", "g_v"), hllm, t5):
        assert torch.isfinite(x).all(), name
        assert torch.equal(x, y), (name, float((x - y).abs().max()))
    if p > 0:
        assert int(rng[1]) == int(rng0[1]) + 1
