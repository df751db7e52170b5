"""TIGER on the MI355X: the T5 attention kernels of csrc/t5attn.hip (the 64 x 64 MFMA path and the one-wavefront path of
Lq <= 8) and the residual RMS norm against the float64 oracle (tests/tiger_oracle.py), their refusals, bitwise repeatable
backwards, dropout on the weights, the model against the reference's fixtures (logits, losses, gradients, three AdamW
steps, constrained beam search), and the attention's memory bound."""
import json
import os

import numpy as np
import pytest
import torch

import tiger_oracle as O

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def dev():
    return torch.device("cuda:0")


# ---- attention against float64 ----------------------------------------------------------------------------------------------
def key_masks(kind, B, Lk, g):
    """right: ragged right padding; left: ragged left padding; mixed: a full row, a row with ONE valid key, a row with NO
    valid key, then left- and right-padded rows."""
    if kind is None:
        return None
    m = torch.ones(B, Lk, dtype=torch.int64)
    for b in range(B):
        n = int(torch.randint(1, Lk + 1, (1,), generator=g))
        if kind == "right":
            m[b, n:] = 0
        elif kind == "left":
            m[b, :Lk - n] = 0
        else:
            if b % 5 == 1:
                m[b] = 0
                m[b, Lk // 2] = 1
            elif b % 5 == 2:
                m[b] = 0
            elif b % 5 == 3:
                m[b, :Lk - n] = 0
            elif b % 5 == 4:
                m[b, n:] = 0
    return m


def attn_case(B, Lq, Lk, H, dh, mask, causal, nb, seed, md=128):
    g = torch.Generator().manual_seed(seed)
    W = H * dh
    q = torch.randn(B, Lq, W, generator=g)
    k = torch.randn(B, Lk, W, generator=g)
    v = torch.randn(B, Lk, W, generator=g)
    if dh > 16:  # keep the softmax from collapsing onto one key: scores of unit variance
        q = q / dh**0.5
    table = 0.5 * torch.randn(nb, H, generator=g) if nb else None
    gout = torch.randn(B, Lq, W, generator=g)
    return dict(q=q, k=k, v=v, table=table, gout=gout, mask=key_masks(mask, B, Lk, g), causal=causal, H=H, md=md,
                bidirectional=not causal)


def oracle_attn(c, dtype):
    q, k, v = (c[n].clone().to(dtype).requires_grad_(True) for n in "qkv")
    t = c["table"].clone().to(dtype).requires_grad_(True) if c["table"] is not None else None
    out = O.attention(q, k, v, c["H"], c["mask"], c["causal"], t, c["bidirectional"], c["md"])
    out.backward(c["gout"].to(dtype))
    return [x.detach().numpy().astype(np.float64) for x in (out, q.grad, k.grad, v.grad)] + \
        [None if t is None else t.grad.numpy().astype(np.float64)]


def run_attn(c, strided, p=0.0, training=True):
    """-> out, g_q, g_k, g_v, g_table on the CPU.  strided: q, k, v are column blocks of wider tensors (one fused QKV
    product when Lq == Lk, else a padded q and one fused KV product)."""
    from torch_rechub_amd import ops
    q, k, v = c["q"], c["k"], c["v"]
    W = q.shape[2]
    tt = c["table"].to(dev()).requires_grad_(True) if c["table"] is not None else None
    if strided and q.shape[1] == k.shape[1]:
        x = torch.cat((q, k, v), 2).to(dev()).requires_grad_(True)
        qq, kk, vv = x[..., :W], x[..., W:2 * W], x[..., 2 * W:]
        leaves = None
    elif strided:
        xq = torch.cat((torch.zeros_like(q[..., :3]), q), 2).to(dev()).requires_grad_(True)
        xkv = torch.cat((k, v), 2).to(dev()).requires_grad_(True)
        qq, kk, vv = xq[..., 3:], xkv[..., :W], xkv[..., W:]
        leaves = None
    else:
        qq, kk, vv = (t.to(dev()).requires_grad_(True) for t in (q, k, v))
        leaves = (qq, kk, vv)
    mask = None if c["mask"] is None else c["mask"].to(dev())
    out = ops.t5_attention(qq, kk, vv, c["H"], key_mask=mask, causal=c["causal"], bias_table=tt,
                           bidirectional=c["bidirectional"], max_distance=c["md"], dropout_p=p, training=training)
    out.backward(c["gout"].to(dev()))
    if leaves is not None:
        grads = [t.grad.cpu() for t in leaves]
    elif q.shape[1] == k.shape[1]:
        grads = [x.grad[..., i * W:(i + 1) * W].cpu() for i in range(3)]
    else:
        grads = [xq.grad[..., 3:].cpu(), xkv.grad[..., :W].cpu(), xkv.grad[..., W:].cpu()]
    return [out.detach().cpu()] + grads + [None if tt is None else tt.grad.cpu()]


# (B, Lq, Lk, H, dh, mask, causal, num_buckets (0: no bias), strided).  Lq <= 8 runs the one-wavefront path (one 64-key
# chunk, chunk edges at 64 / 128, B H not a multiple of the four wavefronts), longer queries the MFMA tiles (one tile,
# ragged second tile, 16 x 16 tiles).
ATTN_CASES = [
    (2, 1, 1, 1, 1, None, False, 0, False),            # a single score
    (5, 5, 80, 3, 50, "right", False, 0, True),        # cross attention, ragged masks, strided KV
    (5, 33, 33, 3, 64, "mixed", False, 32, True),      # encoder: bidirectional buckets, every kind of mask row
    (3, 7, 7, 3, 50, None, True, 8, False),            # decoder: causal, one-sided buckets (narrow path)
    (1, 3, 200, 1, 128, "left", False, 0, False),      # narrow path over four key chunks
    (1, 1024, 1024, 1, 64, "right", False, 32, False),  # 16 x 16 tiles: the online rescale and every diagonal
    (3, 33, 33, 1, 1, "mixed", False, 1, False),       # one bucket, head width 1
    (2, 70, 70, 1, 128, None, True, 32, True),         # causal on the tiles, two column chunks of the head
    (5, 20, 130, 3, 50, "mixed", False, 0, True),      # rectangular on the tiles, three key tiles
    (5, 8, 130, 3, 4, "mixed", False, 32, False),      # narrow path with a bias across chunk edges (the diagonal carry)
    (2, 9, 64, 1, 64, "right", False, 8, False),       # the first length on the tiles, keys exactly one tile
    (2, 8, 8, 3, 64, None, True, 4, True),             # the last length of the narrow path, causal, strided QKV
    (4, 70, 70, 2, 16, "left", True, 8, False),        # causal WITH a mask on the tiles: left-padded rows have no key left
    (4, 150, 150, 1, 50, "mixed", True, 0, True),      # the same over three key tiles, with fully masked samples
    (4, 7, 7, 2, 16, "left", True, 8, False),          # causal with a mask on the narrow path
]


@pytest.mark.parametrize("case", ATTN_CASES)
def test_attention_kernel_against_float64(case):
    """The tolerance rule of test_gpu_hllm.py::test_attention_kernel_against_float64, unchanged: rtol 1e-4 and a floor of
    max(2e-6 of the tensor's largest magnitude (1e-4 for the bias table's gradient), 4 x the error of the same function
    evaluated in fp32 on the CPU against float64).  The bound never looks at the kernel's output.

    One bucket (nb = 1) makes the table's gradient the sum of ALL dS of a head, which is exactly 0 (every softmax row's dS
    sums to 0), so "the tensor's largest magnitude" is 0 and the rule above has no scale.  There the floor is the fp32
    rounding noise of that sum, taken statistically: n independent roundings of relative size u = 2^-24 on terms x_k add up
    to about u sqrt(sum x_k^2), not u sum |x_k|.  A term is P_ij (dA_ij - delta_i), at most 2 P_ij A_i with
    A_i = max_j |g_out_i . v_j|, and sum_j P_ij^2 <= 1, so sqrt(sum dS^2) <= 2 sqrt(sum_i A_i^2); with the rule's own
    factor 4: 4 * 2^-24 * 2 sqrt(sum_i A_i^2).  Measured at the committed case: kernel error 2.0e-7, this floor 1.5e-5 (the
    fp32 CPU error, 9e-9, is no yardstick here: torch sums the (B, Lq, Lk) tensor pairwise, the kernel per diagonal)."""
    B, Lq, Lk, H, dh, mask, causal, nb, strided = case
    c = attn_case(B, Lq, Lk, H, dh, mask, causal, nb, seed=Lq + Lk + H + dh)
    wants = oracle_attn(c, torch.float64)
    cpu32 = oracle_attn(c, torch.float32)
    gots = run_attn(c, strided)
    fails = []
    for name, got, want, c32 in zip(("out", "g_q", "g_k", "g_v", "g_table"), gots, wants, cpu32):
        if want is None:
            assert got is None
            continue
        scale = max(float(np.abs(want).max()), 1e-30)
        e32 = float(np.abs(c32 - want).max())
        atol = max((1e-4 if name == "g_table" else 2e-6) * scale, 4 * e32)
        if name == "g_table" and nb == 1:
            dA = np.einsum("bihd,bjhd->bhij", c["gout"].numpy().astype(np.float64).reshape(B, Lq, H, dh),
                           c["v"].numpy().astype(np.float64).reshape(B, Lk, H, dh))
            atol = max(atol, 4 * 2.0**-24 * 2 * float(np.sqrt((np.abs(dA).max(-1)**2).sum(axis=(0, 2)).max())))
        err = np.abs(got.numpy() - want)
        worst = float((err - 1e-4 * np.abs(want)).max())
        print(f"{case} {name}: max|want| {scale:.3e} fp32-cpu err {e32:.3e} kernel err {float(err.max()):.3e} atol {atol:.3e}")
        assert np.isfinite(got.numpy()).all(), name
        if worst > atol:
            fails.append((name, worst, atol))
    assert not fails, fails


@pytest.mark.parametrize("Lq", [3, 40])
def test_online_softmax_rescale_with_a_late_spike(Lq):
    """A key far down the row whose score jumps the running maximum by ~60: what came before must be rescaled."""
    c = attn_case(1, Lq, 200, 1, 32, None, False, 0, seed=11)
    c["k"][0, 150] = 60.0 * c["q"][0, Lq - 1] / c["q"][0, Lq - 1].norm()**2
    wants = oracle_attn(c, torch.float64)
    gots = run_attn(c, False)
    for got, want in zip(gots[:4], wants[:4]):
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-4, atol=1e-5 * np.abs(want).max())


def test_fully_masked_and_single_key_rows():
    """No key left: weight 1 / Lk on every key, masked ones included (the reference's additive finfo.min, recorded in
    tiger_layers.npz); one key left: the output is that key's value row, bit for bit."""
    from torch_rechub_amd import ops
    for Lq in (4, 20):
        g = torch.Generator().manual_seed(5)
        q, k, v = (torch.randn(2, n, 6, generator=g).to(dev()) for n in (Lq, 9, 9))
        mask = torch.zeros(2, 9, dtype=torch.int64)
        mask[1, 4] = 1
        out = ops.t5_attention(q, k, v, 2, key_mask=mask.to(dev()))
        np.testing.assert_allclose(out[0].cpu().numpy(), v[0].mean(0, keepdim=True).expand(Lq, 6).cpu().numpy(), rtol=1e-6,
                                   atol=1e-7)
        assert torch.equal(out[1], v[1, 4].expand(Lq, 6))


@pytest.mark.parametrize("kind", ["enc", "dec", "cross"])
def test_attention_against_the_recorded_modules(kind):
    """ops.t5_attention between torch products with the recorded weights, against the reference's recorded output and
    gradients (float64 recording): test_gpu_hllm.py's ``close``."""
    from torch_rechub_amd import ops
    z = np.load(os.path.join(GOLDEN, "tiger_layers.npz"))
    cfg = json.loads(str(z["attn.cfg"]))
    pre = f"attn.{kind}."
    P = {n: torch.tensor(z[pre + f"param.{n}.weight"]).to(dev()).requires_grad_(True) for n in "qkvo"}
    tkey = pre + "param.relative_attention_bias.weight"
    table = torch.tensor(z[tkey]).to(dev()).requires_grad_(True) if tkey in z.files else None
    x = torch.tensor(z[pre + "x"]).to(dev()).requires_grad_(True)
    kv = torch.tensor(z[pre + "kv"]).to(dev()).requires_grad_(True) if kind == "cross" else x
    mask = None if kind == "dec" else torch.tensor(z["attn.key_mask"][:x.shape[0]]).to(dev())
    a = ops.t5_attention(x @ P["q"].T, kv @ P["k"].T, kv @ P["v"].T, cfg["num_heads"], key_mask=mask, causal=kind == "dec",
                         bias_table=table, bidirectional=kind != "dec", max_distance=cfg["max_distance"])
    out = a @ P["o"].T
    out.backward(torch.tensor(z[pre + "gout"]).to(dev()))
    close(out, z[pre + "out"], "out")
    close(x.grad, z[pre + "g_x"], "g_x")
    if kind == "cross":
        close(kv.grad, z[pre + "g_kv"], "g_kv")
    for n in "qkvo":
        close(P[n].grad, z[pre + f"grad.{n}.weight"], n)
    if table is not None:
        close(table.grad, z[pre + "grad.relative_attention_bias.weight"], "table")


def test_rejected_shapes_return_the_error_without_a_launch():
    from torch_rechub_amd import ops
    q = torch.randn(1, 5, 8, device=dev())
    k = torch.randn(1, 7, 8, device=dev())
    out_before = torch.cuda.memory_allocated()
    with pytest.raises(RuntimeError, match=r"rc=-2.*causal"):
        ops.t5_attention(q, k, k, 2, causal=True)
    with pytest.raises(RuntimeError, match=r"rc=-2.*head width 129"):
        x = torch.randn(1, 5, 129, device=dev())
        ops.t5_attention(x, x, x, 1)
    with pytest.raises(RuntimeError, match=r"rc=-2.*Lk=1025"):
        kk = torch.randn(1, 1025, 8, device=dev())
        ops.t5_attention(q, kk, kk, 2)
    with pytest.raises(RuntimeError, match=r"rc=-2.*Lq=1025"):
        qq = torch.randn(1, 1025, 8, device=dev())
        ops.t5_attention(qq, k, k, 2)
    torch.cuda.synchronize()
    ops.check_errors()
    assert torch.cuda.memory_allocated() <= out_before + (1 << 20)
    empty = ops.t5_attention(q[:0], k[:0], k[:0], 2)  # B = 0 returns at once
    assert empty.shape == (0, 5, 8)


@pytest.mark.parametrize("Lq", [6, 200])
def test_backward_twice_bitwise_identical(Lq):
    from torch_rechub_amd import ops
    c = attn_case(8, 200, 200, 5, 40, "mixed", False, 32, seed=3) if Lq > 8 else attn_case(9, Lq, 130, 5, 40, "mixed", False, 32, 3)
    a = run_attn(c, False)
    b = run_attn(c, False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    rng = ops._dropout_rng(dev())
    rng0 = rng.clone()
    a = run_attn(c, True, p=0.2)
    rng.copy_(rng0)
    b = run_attn(c, True, p=0.2)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert not torch.equal(a[0], run_attn(c, True, p=0.2)[0])  # the next counter: another mask


@pytest.mark.parametrize("Lq,p", [(4, 0.1), (4, 0.5), (48, 0.1), (48, 0.5)])
def test_dropout_on_the_weights(Lq, p):
    """v = identity per head (dh = Lk = 64) makes output row i the dropped weights of query i; a masked rectangular case
    on both paths."""
    from torch_rechub_amd import ops
    B, Lk, H = 6, 64, 2
    g = torch.Generator().manual_seed(17)
    q = (0.5 * torch.randn(B, Lq, H * Lk, generator=g)).to(dev())
    k = (0.5 * torch.randn(B, Lk, H * Lk, generator=g)).to(dev())
    v = torch.eye(Lk).repeat(B, 1, H).to(dev()).requires_grad_(True)
    mask = key_masks("right", B, Lk, g)
    mask[:, 0] = 1
    valid = (mask != 0).to(dev())[:, None, None, :].expand(B, Lq, H, Lk)
    mask = mask.to(dev())
    rng = ops._dropout_rng(dev())
    rng0 = rng.clone()
    w0 = ops.t5_attention(q, k, v, H, key_mask=mask).detach().view(B, Lq, H, Lk)
    assert torch.equal(rng, rng0)  # p = 0 draws nothing
    wd = ops.t5_attention(q, k, v, H, key_mask=mask, dropout_p=p)
    assert int(rng[1]) == int(rng0[1]) + 1
    wdv = wd.detach().view(B, Lq, H, Lk)
    assert torch.all(w0[valid] > 0) and torch.all(w0[~valid] == 0) and torch.all(wdv[~valid] == 0)
    kept = (wdv != 0) & valid
    n = int(valid.sum())
    frac = float(kept.sum()) / n
    bound = 5 * (p * (1 - p) / n)**0.5  # five standard deviations of the binomial mean
    assert abs(frac - (1 - p)) <= bound, (frac, bound)
    np.testing.assert_allclose(wdv[kept].cpu().numpy(), (w0[kept] / (1 - p)).cpu().numpy(), rtol=2e-6, atol=0)
    # the backward re-derives the forward's mask: d sum(out) / d v[b, j, h, :] = the column sums of the dropped weights
    wd.sum().backward()
    want = wdv.sum(1)  # (B, H, Lk keys)
    got = v.grad.view(B, Lk, H, Lk).permute(0, 2, 1, 3)  # (B, H, keys, dh): equal over dh
    np.testing.assert_allclose(got.cpu().numpy(), want[..., None].expand_as(got).cpu().numpy(), rtol=1e-5, atol=1e-6)
    rng.copy_(rng0)
    again = ops.t5_attention(q, k, v, H, key_mask=mask, dropout_p=p).detach()
    assert torch.equal(again, wd.detach())
    nxt = ops.t5_attention(q, k, v, H, key_mask=mask, dropout_p=p).detach()
    assert not torch.equal((nxt != 0), (again != 0))
    # eval ignores p
    assert torch.equal(ops.t5_attention(q, k, v, H, key_mask=mask, dropout_p=p, training=False).detach(),
                       w0.view(B, Lq, H * Lk))


def test_attention_memory_stays_below_one_score_tensor():
    """Encoder shape B = 64, L = 512, H = 8, dh = 64: forward plus backward, everything they allocate (output, lse, the
    three gradients, delta, the bias partials) against ONE (B, H, L, L) fp32 score tensor (512 MiB)."""
    from torch_rechub_amd import ops
    B, L, H, dh = 64, 512, 8, 64
    q, k, v = (torch.randn(B, L, H * dh, device=dev(), requires_grad=True) for _ in range(3))
    table = torch.randn(32, H, device=dev(), requires_grad=True)
    mask = torch.ones(B, L, dtype=torch.int64, device=dev())
    mask[:, 400:] = 0
    gout = torch.randn(B, L, H * dh, device=dev())
    ops.t5_relative_buckets(L, L, True, 32, 128, device=dev())
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = ops.t5_attention(q, k, v, H, key_mask=mask, bias_table=table)
    out.backward(gout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    scores = B * H * L * L * 4
    print(f"attention fwd + bwd peak {peak / 2**20:.1f} MiB against a score tensor of {scores / 2**20:.1f} MiB")
    assert peak < scores
    assert all(torch.isfinite(t.grad).all() for t in (q, k, v, table))


# ---- add_rms_norm against float64 -------------------------------------------------------------------------------------------
def rms_run(h, delta, w, gy, gh, dtype=None):
    """dtype None: the kernel; else the oracle in that dtype.  -> h_new, y, g_h, g_delta, g_w"""
    from torch_rechub_amd import ops
    if dtype is None:
        h, w = h.to(dev()).requires_grad_(True), w.to(dev()).requires_grad_(True)
        delta = None if delta is None else delta.to(dev()).requires_grad_(True)
        hn, y = ops.add_rms_norm(h, delta, w, 1e-6)
        (hn * gh.to(dev())).sum().add((y * gy.to(dev())).sum()).backward()
    else:
        h, w = h.clone().to(dtype).requires_grad_(True), w.clone().to(dtype).requires_grad_(True)
        delta = None if delta is None else delta.clone().to(dtype).requires_grad_(True)
        hn = h if delta is None else h + delta
        y = O.rms_norm(hn, w, 1e-6)
        (hn * gh.to(dtype)).sum().add((y * gy.to(dtype)).sum()).backward()
    outs = (hn.detach(), y.detach(), h.grad, None if delta is None else delta.grad, w.grad)
    return [None if t is None else t.cpu().numpy().astype(np.float64) for t in outs]


@pytest.mark.parametrize("M,D,with_delta", [(1, 1, True), (33, 7, True), (33, 64, False), (1, 65, True), (33, 512, True),
                                             (33, 1024, False), (2051, 7, True), (2051, 65, False), (1, 1024, True)])
def test_add_rms_norm_against_float64(M, D, with_delta):
    """The attention test's rule: rtol 1e-4, floor max(2e-6 of the tensor's largest magnitude, 4 x the fp32 CPU error).
    M = 2051 is past one trip of the 512-workgroup grid (four rows each); row 0 is all zero."""
    g = torch.Generator().manual_seed(M + D)
    h = torch.randn(M, D, generator=g)
    delta = torch.randn(M, D, generator=g) if with_delta else None
    h[0] = 0
    if delta is not None:
        delta[0] = 0
    w = 1 + 0.3 * torch.randn(D, generator=g)
    gy, gh = torch.randn(M, D, generator=g), torch.randn(M, D, generator=g)
    wants = rms_run(h, delta, w, gy, gh, torch.float64)
    cpu32 = rms_run(h, delta, w, gy, gh, torch.float32)
    gots = rms_run(h, delta, w, gy, gh)
    assert np.all(gots[1][0] == 0) and np.isfinite(gots[2][0]).all()  # the all-zero row: exactly 0 out, a finite gradient
    for name, got, want, c32 in zip(("h_new", "y", "g_h", "g_delta", "g_w"), gots, wants, cpu32):
        if want is None:
            assert got is None
            continue
        scale = max(float(np.abs(want).max()), 1e-30)
        atol = max(2e-6 * scale, 4 * float(np.abs(c32 - want).max()))
        err = np.abs(got - want)
        print(f"M {M} D {D} {name}: max|want| {scale:.3e} kernel err {float(err.max()):.3e} atol {atol:.3e}")
        assert np.isfinite(got).all() and float((err - 1e-4 * np.abs(want)).max()) <= atol, name
    again = rms_run(h, delta, w, gy, gh)
    assert np.array_equal(again[4], gots[4]) and np.array_equal(again[2], gots[2])  # g_w bitwise over two runs


def test_add_rms_norm_refuses_wide_rows():
    from torch_rechub_amd import ops
    with pytest.raises(RuntimeError, match="1 <= D <= 1024"):
        ops.add_rms_norm(torch.randn(2, 1025, device=dev()), None, torch.ones(1025, device=dev()))


# ---- the model against the reference's fixtures (tools/gen_golden_tiger.py) ------------------------------------------------
def close(got, want, what, rtol=2e-4, atol_rel=2e-5):
    """test_gpu_hllm.py's."""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    scale = max(float(np.abs(want).max()), 1e-12)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol_rel * scale, err_msg=what)


def load_model(tag, **over):
    from torch_rechub_amd.models.generative import TIGERConfig, TIGERModel
    z = np.load(os.path.join(GOLDEN, f"model_tiger_{tag}.npz"))
    cfg = dict(json.loads(str(z["cfg"])), **over)
    arrays = {k[len("param/"):]: z[k] for k in z.files if k.startswith("param/")}
    model = TIGERModel(TIGERConfig.from_dict(cfg))
    keys = json.loads(str(z["keys"]))  # (the recording holds the embedding once; its other names are that array again)
    model.load_state_dict({k: torch.tensor(arrays.get(k, arrays["shared.weight"])) for k in keys}, strict=True)
    batch = tuple(torch.tensor(z[k]).to(dev()) for k in ("input_ids", "attention_mask", "labels"))
    return z, cfg, model.to(dev()), batch


@pytest.mark.parametrize("tag", ["a", "b"])
def test_model_matches_the_fixture(tag):
    z, cfg, model, (ids, mask, labels) = load_model(tag)
    model.train()
    res = model(ids, attention_mask=mask, labels=labels)
    close(res["logits"], z["logits"], "logits")
    close(res.loss, z["loss_t1"], "loss at temperature 1")
    model.set_hyper(float(z["temperature"]))
    res = model(ids, attention_mask=mask, labels=labels)
    close(res.loss, z["loss_t"], "loss at the temperature")
    res.loss.backward()
    names = dict(model.named_parameters())
    recorded = [k[len("grad/"):] for k in z.files if k.startswith("grad/")]
    assert sorted(recorded) == sorted(names)
    for n in recorded:
        close(names[n].grad, z["grad/" + n], n)
    model.zero_grad()
    opt = torch.optim.AdamW(model.parameters(), lr=float(z["lr"]))
    losses = []
    for _ in range(3):
        opt.zero_grad()
        loss = model(ids, attention_mask=mask, labels=labels).loss
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    close(np.array(losses), z["step_losses"], "AdamW step losses")


@pytest.mark.parametrize("tag", ["a", "b"])
def test_generate_matches_the_recorded_beam_search(tag):
    from torch_rechub_amd.utils.data import Trie
    z, cfg, model, (ids, mask, _) = load_model(tag)
    trie = Trie(z["beam.candidates"].tolist())
    fn = trie.def_prefix_allowed_tokens_fn(trie)
    model.train()  # generate runs in eval mode and puts the mode back
    gen = model.generate(ids, mask, max_new_tokens=10, num_beams=3, num_return_sequences=3, prefix_allowed_tokens_fn=fn)
    assert model.training
    np.testing.assert_array_equal(gen["sequences"].cpu().numpy(), z["beam.sequences"])
    close(gen["sequences_scores"], z["beam.scores"], "beam scores")
    top1 = model.generate(ids, mask, max_new_tokens=10, num_beams=3, num_return_sequences=1, prefix_allowed_tokens_fn=fn)
    np.testing.assert_array_equal(top1["sequences"].cpu().numpy(), z["beam.sequences"][::3])
    # unsupported: candidates of different lengths; fewer candidates than beams; more returns than beams; no end in time
    ragged = Trie([[0, 5, 11, 21, 1], [0, 6, 1], [0, 7, 12, 1]])
    with pytest.raises(ValueError, match="differ in length"):
        model.generate(ids, mask, 10, 3, 3, ragged.def_prefix_allowed_tokens_fn(ragged))
    two = Trie([[0, 5, 11, 21, 1], [0, 6, 11, 23, 1]])
    with pytest.raises(ValueError, match="fewer"):
        model.generate(ids, mask, 10, 3, 3, two.def_prefix_allowed_tokens_fn(two))
    with pytest.raises(ValueError, match="num_return_sequences"):
        model.generate(ids, mask, 10, 3, 4, fn)
    with pytest.raises(ValueError, match="max_new_tokens"):
        model.generate(ids, mask, 2, 3, 3, fn)


def test_untied_head_against_the_oracle():
    """transformers >= 5 ties T5's embeddings whatever the config says, so the reference cannot record an untied head; the
    model with its own lm_head and no rescale is held to the float64 oracle instead, by the fixture tests' ``close``."""
    z, cfg, model, (ids, mask, labels) = load_model("b", tie_word_embeddings=False)
    with torch.no_grad():
        model.lm_head.weight.copy_(0.3 * torch.randn(model.lm_head.weight.shape, generator=torch.Generator().manual_seed(1)))
    assert model.lm_head.weight.data_ptr() != model.shared.weight.data_ptr()
    P = O.params({k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}, False, requires_grad=True)
    logits, loss = O.forward(P, cfg, ids.cpu().numpy(), mask.cpu().numpy(), labels.cpu().numpy(), 0.7)
    loss.backward()
    model.set_hyper(0.7)
    res = model(ids, attention_mask=mask, labels=labels)
    res.loss.backward()
    close(res.logits, logits.detach().numpy(), "logits")
    close(res.loss, loss.detach().numpy(), "loss")
    for n, p in model.named_parameters():
        close(p.grad, P[n].grad.numpy(), n)


def test_dropout_in_training_draws_and_replays():
    from torch_rechub_amd import ops
    z, cfg, model, (ids, mask, labels) = load_model("a", dropout_rate=0.1)
    model.train()
    rng = ops._dropout_rng(dev())
    rng0 = rng.clone()
    first = model(ids, attention_mask=mask, labels=labels)
    second = model(ids, attention_mask=mask, labels=labels)
    assert not torch.equal(first.logits, second.logits)
    rng.copy_(rng0)
    again = model(ids, attention_mask=mask, labels=labels)
    assert torch.equal(again.logits, first.logits) and torch.equal(again.loss, first.loss)
    model.eval()
    a, b = (model(ids, attention_mask=mask, labels=labels).logits for _ in range(2))
    assert torch.equal(a, b)
