"""ops.softmax_attention on float16 / bfloat16 operands (csrc/softmax_attn_half_tile.h under HLLM's rule): against the
float64 numpy restatement on the rounded inputs, under dropout with the float32 kernel's mask, bitwise properties, the
guards, and HLLMTransformerBlock / HLLMModel with ``attn_dtype``."""
import numpy as np
import pytest
import torch

from test_gpu_hllm import attn_inputs, dev, run_attn
from test_gpu_session_hllm_shapes import recover_keep
from test_hllm_host import np_buckets, np_softmax_attention, np_softmax_attention_bwd

pytestmark = pytest.mark.gpu

F16, BF16 = torch.float16, torch.bfloat16
UNIT = {F16: 2.0**-11, BF16: 2.0**-8}  # the rounding of one stored value
NAMES = ("out", "g_q", "g_k", "g_v", "g_table")


def rounded_inputs(B, L, H, dh, nb, seed, dtype):
    """attn_inputs with qkv and g_out rounded to ``dtype`` (kept in it); the table stays float32."""
    qkv, table, gout = attn_inputs(B, L, H, dh, nb, seed)
    return qkv.to(dtype), table, gout.to(dtype)


def twin_attention(q, k, v, H, N, table, keep=None):
    """The plain torch formulation evaluated in the operands' dtype (softmax in float32, cast back), for CPU autograd."""
    B, L, W = q.shape
    dh = W // H
    qh, kh, vh = (t.view(B, L, H, dh).transpose(1, 2) for t in (q, k, v))
    s = torch.matmul(qh, kh.transpose(-2, -1)) * dh**-0.5
    s = s.masked_fill(~torch.tril(torch.ones(L, L, dtype=torch.bool)), float("-inf"))
    if table is not None:
        s = s + table[torch.from_numpy(np_buckets(L, N, table.shape[0]))].permute(2, 0, 1).unsqueeze(0).to(s.dtype)
    p = torch.softmax(s, -1, dtype=torch.float32).to(q.dtype)
    if keep is not None:
        p = p * keep.to(q.dtype)
    return torch.matmul(p, vh).transpose(1, 2).reshape(B, L, W)


def check_half(case, qkv, table, gout, H, N, strided, p=0.0, keep=None):
    """atol = max(2 u max|want|, 4 e_twin), rtol 0: 2 u is the floor any stored T result carries, e_twin the error of the
    CPU evaluation in T against float64 (same per-operation rounding, another summation order: the factor 4 of
    test_attention_kernel_against_float64).  The bound never looks at the kernel's output."""
    dtype, W = qkv.dtype, qkv.shape[2] // 3
    q, k, v = (qkv[..., i * W:(i + 1) * W] for i in range(3))
    f64 = lambda t: t.double().numpy()  # noqa: E731
    ref, cache = np_softmax_attention(f64(q), f64(k), f64(v), H, N, None if table is None else table.numpy(), keep=keep)
    wants = (ref,) + np_softmax_attention_bwd(cache, f64(gout))
    cq, ck, cv = (t.clone().requires_grad_(True) for t in (q, k, v))
    ct = table.clone().requires_grad_(True) if table is not None else None
    co = twin_attention(cq, ck, cv, H, N, ct, None if keep is None else torch.from_numpy(keep))
    co.backward(gout)
    twins = (co.detach(), cq.grad, ck.grad, cv.grad, None if ct is None else ct.grad)
    gots = run_attn(qkv, table, gout, H, N, strided, p=p)
    fails = []
    for name, got, want, twin in zip(NAMES, gots, wants, twins):
        if want is None:
            assert got is None
            continue
        assert got.dtype == (torch.float32 if name == "g_table" else dtype), name
        scale = float(np.abs(want).max())
        e_twin = float(np.abs(twin.double().numpy() - want).max())
        atol = max(2 * UNIT[dtype] * scale, 4 * e_twin)
        err = float(np.abs(got.double().numpy() - want).max())
        print(f"{case} {name}: max|want| {scale:.3e} twin err {e_twin:.3e} kernel err {err:.3e} atol {atol:.3e}")
        assert np.isfinite(got.float().numpy()).all(), name
        if err > atol:
            fails.append((name, err, atol))
    assert not fails, fails


# (B, L, H, dh, max_seq_len, num_buckets (0: no bias), strided, dtype): every head width of {1, 8, 15, 16, 17, 50, 72, 128}
# (the MFMA step of 16 and its padding, single halves against 16-byte loads, odd head offsets with H = 3), every length of
# {1, 63, 64, 65, 130} (ragged, full and several tiles, the diagonal tile), bias tables of 1, 5, 32 buckets and none
HALF_CASES = [(2, 1, 1, 1, 1, 0, False, F16), (2, 63, 3, 8, 70, 5, True, BF16), (1, 64, 3, 15, 64, 1, False, F16),
              (2, 65, 2, 16, 65, 32, True, BF16), (1, 130, 3, 17, 200, 5, False, BF16), (2, 130, 2, 50, 130, 32, True, F16),
              (1, 65, 3, 72, 65, 0, True, BF16), (1, 130, 2, 128, 130, 32, True, F16), (2, 64, 1, 128, 64, 0, False, BF16),
              (1, 63, 3, 16, 63, 0, False, F16), (1, 130, 1, 8, 130, 1, False, BF16), (1, 65, 3, 50, 65, 5, False, BF16)]


@pytest.mark.parametrize("case", HALF_CASES, ids=str)
def test_half_kernel_against_float64(case):
    B, L, H, dh, N, nb, strided, dtype = case
    qkv, table, gout = rounded_inputs(B, L, H, dh, nb, L + H + dh, dtype)
    check_half(case, qkv, table, gout, H, N, strided)


def test_half_kernel_under_dropout_against_float64():
    """p = 0.3, L = 70, dh = 16, bf16 under the mask the float32 kernel draws at the same (seed, counter): the element index
    and key are shared, so it is this kernel's mask too.  The device counter advances by exactly 1."""
    from torch_rechub_amd import ops
    B, L, H, dh, p = 2, 70, 3, 16, 0.3
    rng = ops._dropout_rng(dev())
    state0 = rng.clone()
    keep = recover_keep(B, L, H, p, state0)
    qkv, table, gout = rounded_inputs(B, L, H, dh, 5, 7, BF16)
    check_half("dropout", qkv, table, gout, H, L, True, p=p, keep=keep)
    assert int(rng[1]) == int(state0[1]) + 1 and int(rng[0]) == int(state0[0])


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_half_bitwise_properties(dtype):
    """Two runs, and a call on column blocks of one tensor against a call on three contiguous tensors (another row stride;
    both take 16-byte loads at dh = 72), give equal bits; the types."""
    qkv, table, gout = rounded_inputs(2, 130, 2, 72, 32, 3, dtype)
    a = run_attn(qkv, table, gout, 2, 130, True)
    b = run_attn(qkv, table, gout, 2, 130, True)
    c = run_attn(qkv, table, gout, 2, 130, False)
    for name, x, y, z in zip(NAMES, a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z), name
        assert x.dtype == (torch.float32 if name == "g_table" else dtype), name


@pytest.mark.parametrize("what", ["mixed", "half_table", "float64", "long", "wide"])
def test_half_guards(what):
    """Refused in Python, before any launch: mixed operand types, a half bias table, float64, and the float32 limits."""
    from torch_rechub_amd import _lib, ops
    L, W, H = {"long": (_lib.H.RH_ATTN_MAX_L + 1, 8, 1), "wide": (4, _lib.H.RH_ATTN_MAX_DH + 1, 1)}.get(what, (4, 8, 2))
    q = torch.zeros(1, L, W, device=dev(), dtype=torch.float64 if what == "float64" else BF16)
    k = q.to(F16) if what == "mixed" else q
    table = torch.zeros(4, H, device=dev(), dtype=BF16 if what == "half_table" else torch.float32)
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.softmax_attention(q, k, q, H, 2 * L, bias_table=table)
    ops.check_errors(dev())


@pytest.mark.parametrize("dtype", [F16, BF16])
def test_half_empty_batch(dtype):
    from torch_rechub_amd import ops
    q, k, v = (torch.zeros(0, 5, 12, device=dev(), dtype=dtype, requires_grad=True) for _ in range(3))
    table = torch.zeros(4, 3, device=dev(), requires_grad=True)
    out = ops.softmax_attention(q, k, v, 3, 8, bias_table=table, dropout_p=0.1)
    assert out.shape == (0, 5, 12) and out.dtype == dtype
    out.sum().backward()
    assert q.grad.shape == (0, 5, 12) and q.grad.dtype == dtype and torch.all(table.grad == 0)


def test_block_with_attn_dtype_is_the_written_out_steps():
    from torch_rechub_amd import ops
    from torch_rechub_amd.models.generative.hllm import HLLMTransformerBlock
    from torch_rechub_amd.utils.hstu_utils import RelPosBias
    torch.manual_seed(0)
    m = HLLMTransformerBlock(d_model=32, n_heads=2, dropout=0, attn_dtype=BF16).to(dev())
    assert list(m.state_dict()) == list(HLLMTransformerBlock(d_model=32, n_heads=2, dropout=0).state_dict())
    with pytest.raises(ValueError, match="attn_dtype"):
        HLLMTransformerBlock(d_model=32, n_heads=2, attn_dtype=torch.float64)
    rp = RelPosBias(2, 70, 8).to(dev())
    x = torch.randn(3, 70, 32, device=dev())
    with torch.no_grad():
        h = m.norm1(x)
        attn = ops.softmax_attention(m.W_Q(h).to(BF16), m.W_K(h).to(BF16), m.W_V(h).to(BF16), 2, 70,
                                     bias_table=rp.rel_pos_bias_table, scale=m.scale)
        assert attn.dtype == BF16
        y = x + m.W_O(attn.float())
        y = y + m.ffn[3](torch.relu(m.ffn[0](m.norm2(y))))
        assert torch.equal(m(x, rel_pos_bias=rp), y)


def test_seq_trainer_step_of_a_half_attention_model():
    from torch_rechub_amd.models.generative import HLLMModel
    from torch_rechub_amd.trainers import SeqTrainer
    g = torch.Generator().manual_seed(0)
    V, L = 23, 9
    model = HLLMModel(torch.randn(V, 32, generator=g), V, d_model=32, n_heads=2, n_layers=2, max_seq_len=L,
                      num_time_buckets=16, attn_dtype=F16)
    trainer = SeqTrainer(model, device="cuda:0")
    model.train()
    tok = torch.randint(1, V, (4, L), generator=g).to(dev())
    td = torch.randint(0, 10**6, (4, L), generator=g).to(dev())
    loss = trainer.train_step(tok, td, torch.randint(1, V, (4,), generator=g).to(dev()))
    assert torch.isfinite(loss)
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
