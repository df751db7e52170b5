"""The FFM / CEN, capsule / self-attentive / list-wise and HSTU kernels against float64 over their supported shape ranges:
tile edges, odd and unit widths, the grid-stride loops, the largest shape each Python-side check accepts (and the
refusal one past it), per-workgroup partial sums that only appear at large batches, and the empty batch."""
import numpy as np
import pytest
import torch

from test_ffm_host import np_cen_desc, np_cen_desc_bwd, np_cen_rescale_bwd, np_ffm, np_ffm_bwd
from test_gpu_ffm import ffm_call, np_em, np_table_grads
from test_hstu_host import np_attention, np_attention_bwd, np_bucket, np_head
from test_interest_host import np_capsule, np_listwise, squash_bwd

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def poison(numel):
    """Hand a NaN block of ``numel`` floats back to the caching allocator, so that a buffer of that size the op takes with
    torch.empty starts as NaN (the autouse fixture poisons only up to 64 MB)."""
    junk = torch.full((int(numel),), float("nan"), device=dev())
    del junk


# ---- HSTU attention -----------------------------------------------------------------------------------------------
def attn_case(B, L, H, dqk, dv, N, nb, mask_kind, tmax, seed):
    g = torch.Generator().manual_seed(seed)
    proj = torch.nn.functional.silu(torch.randn(B, L, 2 * H * (dqk + dv), generator=g))
    pos_w = 0.3 * torch.randn(2 * N - 1, H, generator=g)
    ts_w = 0.3 * torch.randn(nb + 1, H, generator=g)
    td = None if tmax is None else torch.randint(0, tmax, (B, L), generator=g)
    mask = None
    if mask_kind == "pad":
        lens = torch.randint(0, L + 1, (B,), generator=g)
        lens[0] = L
        mask = torch.arange(L)[None, :] < lens[:, None]
        left = torch.arange(B) % 2 == 1
        mask[left] = (torch.arange(L)[None, :] >= (L - lens[:, None]))[left]
    elif mask_kind == "holes":
        mask = torch.rand(B, L, generator=g) < 0.7
        mask[0] = True
        if B > 2:
            mask[1] = False
            mask[2] = False
            mask[2, L - 1] = True  # the only kept key is the last: every earlier query sees nothing
    return proj, pos_w, ts_w, td, mask


ATTN_CASES = {
    # name: (B, L, H, dqk, dv, N, nb, mask, max time diff)
    "L1_d1": (5, 1, 2, 1, 1, 1, 16, "pad", 10**6),
    "L63_qk1_v64": (9, 63, 2, 1, 64, 63, 64, "holes", 10**6),
    "L64_qk64_v1": (9, 64, 2, 64, 1, 80, 0, "pad", 10**6),
    "L65_odd_N1024_nb1023": (7, 65, 3, 33, 17, 1024, 1023, "holes", 2 * 10**6),
    "L65_qk64_v64_nomask": (6, 65, 2, 64, 64, 65, 128, None, 10**6),
    "L1024": (2, 1024, 2, 64, 64, 1024, 1023, "holes", 2 * 10**6),
    "L200_nomask_notime": (3, 200, 1, 33, 17, 256, 8, None, None),
    "partials_2304": (192, 129, 4, 8, 8, 129, 300, "holes", 2 * 10**6),
}


@pytest.mark.parametrize("name", list(ATTN_CASES))
def test_hstu_attention_shapes_against_float64(name):
    from torch_rechub_amd import ops
    B, L, H, dqk, dv, N, nb, mask_kind, tmax = ATTN_CASES[name]
    fn, div, unit = "sqrt", 1.0, "seconds"  # sqrt(|dt| s): deltas up to 2e6 s reach and pass bucket 1023
    proj, pos_w, ts_w, td, mask = attn_case(B, L, H, dqk, dv, N, nb, mask_kind, tmax, seed=L * 7 + dqk)
    gout = torch.randn(B, L, H * dv, generator=torch.Generator().manual_seed(L))
    x = proj.to(dev()).requires_grad_(True)
    pw, tw = pos_w.to(dev()).requires_grad_(True), ts_w.to(dev()).requires_grad_(True)
    out = ops.hstu_attention(x, pw, tw, H, dqk, dv, N, time_diffs=None if td is None else td.to(dev()),
                             padding_mask=None if mask is None else mask.to(dev()), num_time_buckets=nb, time_bucket_fn=fn,
                             time_bucket_divisor=div, time_bucket_unit=unit)
    out.backward(gout.to(dev()))
    ref, cache = np_attention(proj.numpy(), pos_w.numpy(), ts_w.numpy(), None if td is None else td.numpy(),
                              None if mask is None else mask.numpy(), H, dqk, dv, N, nb, fn, div, unit)
    if td is not None and nb >= 256:  # the second tacc pass of the dQ kernel (buckets >= 256) and the top bucket are live
        live = cache["bk"][np.broadcast_to(cache["valid"][:, 0], cache["bk"].shape)]
        assert live.max() == nb and (live >= 256).mean() > 0.1
    got = out.detach().cpu().numpy()
    np.testing.assert_allclose(got, ref, rtol=1e-4, atol=2e-6)
    if mask_kind == "holes" and B > 2:
        assert not got[1].any() and not got[2, :L - 1].any()  # rows without a kept key are exactly zero
    rgp, rgpos, rgts = np_attention_bwd(cache, gout.numpy(), H, dqk, dv, N, 2 * N - 1, nb + 1)
    gp = x.grad.cpu().numpy()
    qkv = np.r_[0:2 * H * dqk, 2 * H * dqk + H * dv:2 * H * (dqk + dv)]
    np.testing.assert_allclose(gp[..., qkv], rgp[..., qkv], rtol=1e-4, atol=2e-6)
    assert not gp[..., 2 * H * dqk:2 * H * dqk + H * dv].any()  # the u columns
    gpos = pw.grad.cpu().numpy()
    np.testing.assert_allclose(gpos, rgpos, rtol=1e-4, atol=1e-4 * np.abs(rgpos).max())
    # rows outside the band |i - j| < L (and every row of a key after its query) are exactly zero
    assert not gpos[:N - L].any() and not gpos[N:].any()
    gts = tw.grad.cpu().numpy()
    if td is None:
        assert not gts.any()
    else:
        np.testing.assert_allclose(gts, rgts, rtol=1e-4, atol=1e-4 * max(np.abs(rgts).max(), 1e-30))


def test_hstu_attention_partial_sums_are_bitwise_repeatable():
    from torch_rechub_amd import ops
    B, L, H, dqk, dv, N, nb, mask_kind, tmax = ATTN_CASES["partials_2304"]
    assert ops._lib.call("rh_hstu_attn_nparts", B, L, H) >= 2000
    proj, pos_w, ts_w, td, mask = attn_case(B, L, H, dqk, dv, N, nb, mask_kind, tmax, seed=3)
    gout = torch.randn(B, L, H * dv, generator=torch.Generator().manual_seed(4)).to(dev())
    grads = []
    for _ in range(2):
        pw, tw = pos_w.to(dev()).requires_grad_(True), ts_w.to(dev()).requires_grad_(True)
        ops.hstu_attention(proj.to(dev()), pw, tw, H, dqk, dv, N, time_diffs=td.to(dev()), padding_mask=mask.to(dev()),
                           num_time_buckets=nb, time_bucket_fn="sqrt", time_bucket_unit="seconds").backward(gout)
        grads.append((pw.grad.cpu(), tw.grad.cpu()))
    assert torch.equal(grads[0][0], grads[1][0]) and torch.equal(grads[0][1], grads[1][1])


def test_hstu_attention_guard_accepts_its_largest_shape_only():
    """L = 1024, dqk = dv = 64, nb = 1023 run (test_hstu_attention_shapes_against_float64[L1024]); one past each limit
    is refused before a launch."""
    from torch_rechub_amd import ops
    pos_w = torch.zeros(2 * 1100 - 1, 1, device=dev())
    ts_w = torch.zeros(1025, 1, device=dev())

    def run(L, dqk, dv, nb, N=1100):
        proj = torch.zeros(1, L, 2 * (dqk + dv), device=dev())
        return ops.hstu_attention(proj, pos_w[:2 * N - 1], ts_w[:nb + 1], 1, dqk, dv, N, num_time_buckets=nb)

    assert run(1024, 64, 64, 1023).shape == (1, 1024, 64)
    for args in ((1025, 8, 8, 16), (64, 65, 8, 16), (64, 8, 65, 16), (64, 8, 8, 1024)):
        with pytest.raises(RuntimeError, match="no HIP kernel"):
            run(*args)
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        run(65, 8, 8, 16, N=64)  # L > max_seq_len


def test_hstu_time_buckets_up_to_1023_match_the_restatement():
    """The kernel's bucket for every delta of a sweep that crosses each edge up to nb = 1023 (q = k = 0, v = 1: the output
    of query 1 is silu(ts_w[bucket]) / N with ts_w[c] = c / 64)."""
    from torch_rechub_amd import ops
    nb = 1023
    edges = np.arange(0, nb + 3, dtype=np.int64) ** 2
    dt = np.unique(np.concatenate([edges + k for k in (-1, 0, 1)]).clip(0))
    B, N = len(dt), 2
    td = torch.stack([torch.from_numpy(dt), torch.zeros(B, dtype=torch.int64)], 1).to(dev())
    proj = torch.zeros(B, 2, 4, device=dev())
    proj[:, 0, 3] = 1.0
    ts_w = (torch.arange(nb + 1, dtype=torch.float32, device=dev()) / 64)[:, None]
    out = ops.hstu_attention(proj, torch.zeros(3, 1, device=dev()), ts_w, 1, 1, 1, N, time_diffs=td, num_time_buckets=nb,
                             time_bucket_fn="sqrt", time_bucket_unit="seconds")[:, 1, 0]
    table = torch.nn.functional.silu(ts_w[:, 0]) / N
    gap = (table[1:] - table[:-1]).min()
    got = torch.searchsorted(table, out - 0.25 * gap).cpu().numpy()
    want = np_bucket(-dt, nb, "sqrt", 1.0, "seconds")
    assert want.max() == nb
    np.testing.assert_array_equal(got, want)


# ---- HSTU next-token head -----------------------------------------------------------------------------------------
HEAD_CASES = [
    # (M, D, V, nce_temperature, bias, dW path at D > 256)
    (1, 1, 2, None, True, None),
    (63, 63, 3, 0.1, False, None),
    (65, 65, 63, None, False, None),
    (65, 1, 64, 0.1, True, None),
    (1, 600, 65, None, True, None),
    (5000, 256, 64, 0.1, True, None),
    (63, 257, 4097, None, True, "direct"),
    (63, 600, 64, 0.1, False, "direct"),
    (65, 600, 4097, 0.1, False, "slab"),
    (5000, 600, 65, None, False, "slab"),
    (5000, 257, 4097, 0.1, True, "slab"),
]


@pytest.mark.parametrize("M,D,V,t2,with_bias,path", HEAD_CASES)
def test_hstu_head_shapes_against_float64(M, D, V, t2, with_bias, path):
    from torch_rechub_amd import _lib, ops
    R = _lib.call("rh_hstu_head_rsplit", M, D, V)
    assert _lib.call("rh_hstu_head_nsplit", M, V) >= 1
    if path is not None:
        assert D > 256 and (R == 1) == (path == "direct"), R
    g = torch.Generator().manual_seed(M + D + V)
    t1 = 0.05
    h = torch.nn.functional.normalize(torch.randn(M, D, generator=g), dim=-1)
    w = torch.nn.functional.normalize(torch.randn(V, D, generator=g), dim=-1)
    b = 0.1 * torch.randn(V, generator=g) if with_bias else None
    labels = torch.randint(0, V, (M,), generator=g)
    labels[0] = V - 1
    if M > 2:
        labels[1] = 1
        labels[2::7] = 0
    hd, wd = h.to(dev()).requires_grad_(True), w.to(dev()).requires_grad_(True)
    bd = b.to(dev()).requires_grad_(True) if with_bias else None
    loss = ops.next_token_loss(hd, wd, bd, labels.to(dev()), temperature=t1, nce_temperature=t2)
    loss.backward()
    ops.check_errors(dev())
    rl, rdh, rdw, rdb = np_head(h.numpy(), w.numpy(), None if b is None else b.numpy(), labels.numpy(), t1, t2)
    assert abs(loss.item() - rl) <= 1e-5 * abs(rl) + 1e-6, (loss.item(), rl)
    pairs = [(hd.grad, rdh), (wd.grad, rdw)] + ([(bd.grad, rdb)] if with_bias else [])
    for got, want in pairs:
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=2e-4, atol=2e-4 * max(np.abs(want).max(), 1e-30))
    assert not wd.grad[0].any()
    if with_bias:
        assert bd.grad[0] == 0


def test_hstu_head_negative_label_sets_the_error_word_and_empty_rows_are_refused():
    from torch_rechub_amd import ops
    h, w = torch.randn(10, 8, device=dev()), torch.randn(30, 8, device=dev())
    labels = torch.arange(10, device=dev())
    labels[6] = -1
    ops.next_token_loss(h, w, None, labels)
    with pytest.raises(IndexError, match="target label"):
        ops.check_errors(dev())
    ops.check_errors(dev())  # the word was cleared
    with pytest.raises(RuntimeError, match="M >= 1"):
        ops.next_token_loss(h[:0], w, None, labels[:0])


# ---- capsule routing ----------------------------------------------------------------------------------------------
def caps_max_len(I, D, kind):
    from torch_rechub_amd import ops
    L = 1
    while ops.capsule_supported(L + 1, I, D, kind):
        L += 1
    return L


def caps_mask(B, L, g):
    mask = (torch.rand(B, L, generator=g) < 0.8).to(torch.int32)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    half = torch.arange(B) % 2 == 0
    mask[half] = (torch.arange(L)[None, :] < lens[:, None]).to(torch.int32)[half]
    if B > 3:
        mask[3] = 0  # nothing kept: a zero capsule
    if B > 1:
        mask[1] = 1
    if B > 2:
        mask[2] = 0
        mask[2, L // 2] = 1  # kept at exactly one position
    return mask


def run_capsule(kind, B, L, I, D, rt, seed):
    from torch_rechub_amd import ops
    g = torch.Generator().manual_seed(seed)
    mask = caps_mask(B, L, g)
    e = 0.5 * torch.randn(B, L, D, generator=g)
    init = torch.randn(B, I, L, generator=g) if kind == 0 else None
    w = wd = None
    if kind == 2:
        w = 0.3 * torch.randn(1, L, I * D, D, generator=g)
        x, wd = e.to(dev()).requires_grad_(True), w.to(dev()).requires_grad_(True)
        uh = np.einsum("ljk,blk->blj", w[0].double().numpy(), e.double().numpy(), optimize=True)
    else:
        Iu = 1 if kind == 0 else I
        x = (0.5 * torch.randn(B, L, Iu * D, generator=g)).to(dev()).requires_grad_(True)
        uh = x.detach().cpu().double().numpy()
        if kind == 0:
            uh = np.tile(uh, (1, 1, I))
    uh = uh.reshape(B, L, I, D).transpose(0, 2, 1, 3)
    cap = ops.capsule_routing(x, wd, mask.to(dev()), None if init is None else init.to(dev()), kind, I, D, rt)
    want, sw, s = np_capsule(uh, mask.numpy(), None if init is None else init.numpy(), rt)
    np.testing.assert_allclose(cap.detach().cpu().numpy(), want, rtol=1e-4, atol=2e-6)
    if B > 3:
        assert not cap[3].any()
    gy = torch.randn(B, I, D, generator=g)
    cap.backward(gy.to(dev()))
    guh = np.einsum("bil,bid->blid", sw, squash_bwd(s, gy.double().numpy()))
    if kind == 2:
        w64 = w[0].double().numpy()
        np.testing.assert_allclose(x.grad.cpu().numpy(), np.einsum("ljk,blj->blk", w64, guh.reshape(B, L, I * D),
                                                                   optimize=True), rtol=1e-4, atol=1e-5)
        gw = np.einsum("blj,blk->ljk", guh.reshape(B, L, I * D), e.double().numpy(), optimize=True)[None]
        np.testing.assert_allclose(wd.grad.cpu().numpy(), gw, rtol=1e-4, atol=1e-4 * max(np.abs(gw).max(), 1e-30))
    else:
        gu = guh.sum(2) if kind == 0 else guh.reshape(B, L, I * D)
        np.testing.assert_allclose(x.grad.cpu().numpy(), gu, rtol=1e-4, atol=1e-5)


CAPS_CASES = [
    # (kind, B, L, I, D, routing_times); L = 0 stands for the largest L capsule_supported accepts
    (0, 301, 20, 16, 16, 3),     # I*D = 256: one sample per workgroup
    (1, 2, 0, 16, 16, 2),
    (2, 1, 30, 16, 1, 1),
    (0, 2001, 50, 4, 1, 5),      # D = 1, four samples per workgroup, B not a multiple of 4
    (2, 5, 0, 4, 1, 3),
    (1, 7, 60, 4, 64, 3),        # D = 64
    (0, 2, 0, 4, 64, 1),
    (0, 3001, 100, 1, 16, 3),    # I = 1, L > 64: 64-lane softmax rows
    (1, 5, 0, 1, 16, 2),
    (2, 31, 50, 4, 32, 3),       # type 2, I*D*D = 4096, B < 32: one sample per wgrad chunk
    (2, 33, 40, 1, 64, 5),       # B = 33: chunks of 2 samples, the last 15 chunks empty
    (2, 2, 0, 1, 64, 3),
    (2, 3001, 20, 4, 32, 2),
    (2, 3, 0, 4, 32, 3),
    (1, 1, 0, 4, 16, 3),
]


@pytest.mark.parametrize("kind,B,L,I,D,rt", CAPS_CASES)
def test_capsule_shapes_against_float64(kind, B, L, I, D, rt):
    if L == 0:
        L = caps_max_len(I, D, kind)
    run_capsule(kind, B, L, I, D, rt, seed=B + L + I + D + kind)


@pytest.mark.parametrize("kind,I,D", [(0, 16, 16), (1, 4, 64), (2, 1, 64), (2, 4, 32), (0, 1, 16)])
def test_capsule_supported_is_the_kernels_limit(kind, I, D):
    """capsule_supported accepts the largest L that runs (test_capsule_shapes_against_float64 runs it) and the op refuses
    the next one without a launch."""
    from torch_rechub_amd import ops
    L = caps_max_len(I, D, kind) + 1
    assert not ops.capsule_supported(L, I, D, kind)
    x = torch.zeros(2, L, D if kind != 1 else I * D, device=dev())
    w = torch.zeros(1, L, I * D, D, device=dev()) if kind == 2 else None
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.capsule_routing(x, w, torch.ones(2, L, dtype=torch.int32, device=dev()), None, kind, I, D, 3)
    assert not ops.capsule_supported(8, 4, 65, 0) and not ops.capsule_supported(8, 17, 16, 1)
    assert not ops.capsule_supported(8, 4, 33, 2) and ops.capsule_supported(8, 4, 32, 2)


# ---- self-attentive pooling -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,L,I,D,masked", [(300, 256, 4, 16, True), (200, 1024, 1, 64, True), (100, 64, 16, 64, False),
                                            (300, 16, 64, 16, True), (500, 50, 4, 1, True), (1000, 1, 4, 16, True),
                                            (70000, 2, 2, 4, False), (66000, 3, 1, 2, True)])
def test_sa_pool_shapes_against_float64(B, L, I, D, masked):
    from torch_rechub_amd import ops
    assert ops.sa_supported(L, I, D)
    g = torch.Generator().manual_seed(B + L + I + D)
    mask = None
    if masked:
        mask = (torch.rand(B, L, generator=g) < 0.7).to(torch.int32)
        mask[0] = 0  # fully padded: uniform weights
        mask[1] = 1
    A = torch.randn(B, L, I, generator=g) * 3
    e = torch.randn(B, L, D, generator=g)
    Ad, ed = A.to(dev()).requires_grad_(True), e.to(dev()).requires_grad_(True)
    out = ops.sa_pool(Ad, ed, None if mask is None else mask.to(dev()))
    Am = A if mask is None else A + np.float32(-1e9) * (1 - mask.float())[..., None]  # formed in float32, as the kernel
    Am = Am.double().numpy()
    ex = np.exp(Am - Am.max(1, keepdims=True))
    P = ex / ex.sum(1, keepdims=True)
    e64 = e.double().numpy()
    np.testing.assert_allclose(out.detach().cpu().numpy(), np.einsum("bli,bld->bid", P, e64), rtol=1e-4, atol=1e-5)
    gy = torch.randn(B, I, D, generator=g)
    out.backward(gy.to(dev()))
    gP = np.einsum("bid,bld->bli", gy.double().numpy(), e64)
    np.testing.assert_allclose(Ad.grad.cpu().numpy(), P * (gP - (P * gP).sum(1, keepdims=True)), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(ed.grad.cpu().numpy(), np.einsum("bli,bid->bld", P, gy.double().numpy()), rtol=1e-4,
                               atol=1e-5)


def test_sa_supported_is_the_kernels_limit():
    from torch_rechub_amd import ops
    for L, I, D in ((1024, 1, 64), (64, 16, 64), (16, 64, 16)):  # run by test_sa_pool_shapes_against_float64
        assert ops.sa_supported(L, I, D)
    for L, I, D in ((1025, 1, 64), (65, 16, 64), (16, 64, 17), (4, 1, 65)):
        assert not ops.sa_supported(L, I, D)
        with pytest.raises(RuntimeError, match="no HIP kernel"):
            ops.sa_pool(torch.zeros(2, L, I, device=dev()), torch.zeros(2, L, D, device=dev()))


# ---- list-wise scoring ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,I,D,K,T", [(300, 1, 1, 0, 0.05), (257, 16, 33, 1, 0.07), (300, 16, 64, 1023, 0.02),
                                       (1000, 4, 1, 5, 1.0), (500, 1, 64, 0, 0.02), (200, 16, 1, 1023, 0.3),
                                       (40000, 2, 8, 1, 0.5), (33000, 16, 64, 0, 0.02)])
def test_listwise_shapes_against_float64(B, I, D, K, T):
    from torch_rechub_amd import ops
    g = torch.Generator().manual_seed(B + I + D + K)
    u = torch.nn.functional.normalize(torch.randn(B, I, D, generator=g), dim=-1)
    wide = 0.1 * torch.randn(B, D + 5, generator=g)
    neg = 0.1 * torch.randn(B, K, D, generator=g)
    wide[3] = 0.0  # a zero positive row
    if K:
        neg[4, K - 1] = 0.0  # a zero negative row
    pos = wide[:, 2:2 + D]
    ud, nd = u.to(dev()).requires_grad_(True), neg.to(dev()).requires_grad_(True)
    wd = wide.to(dev()).requires_grad_(True)
    pd = wd[:, 2:2 + D]
    assert pd.stride(0) == D + 5 and ops.listwise_ok(ud, pd, nd)
    logits, best = ops.listwise_logits(ud, pd, nd, T)
    assert logits.shape == (B, 1 + K)
    gy = torch.randn(B, 1 + K, generator=g)
    want, wbest, g_u, g_pos, g_neg = np_listwise(u.double().numpy(), pos.double().numpy(), neg.double().numpy(), T,
                                                 gy.double().numpy())
    agree = best.cpu().numpy() == wbest
    assert agree.mean() > 0.999 and agree[3]  # (fp32 near-ties may pick the other interest)
    np.testing.assert_allclose(logits.detach().cpu().numpy()[agree], want[agree], rtol=1e-4, atol=1e-4)
    assert not logits[3, 0].item()
    logits.backward(gy.to(dev()))
    np.testing.assert_allclose(ud.grad.cpu().numpy()[agree], g_u[agree], rtol=1e-4, atol=1e-3)
    # The row gradient (gvh - vh (gvh . vh)) / n is formed from terms of size |g / T| |u_best| / n that cancel (exactly, at
    # D = 1: vh = +-1), so float32 leaves a residual of a few ulp of that scale, which 1 / n amplifies for a short row.
    rows = np.concatenate([pos.double().numpy()[:, None], neg.double().numpy()], 1)
    ub = u.double().numpy()[np.arange(B), wbest]
    scale = (np.abs(gy.double().numpy()) / T * np.linalg.norm(ub, axis=-1)[:, None] /
             np.maximum(np.linalg.norm(rows, axis=-1), 1e-12))[..., None]

    def close_rows(got, want, sc):
        bad = np.abs(got - want) > 1e-4 * np.abs(want) + 1e-2 + 1e-5 * sc
        assert not bad.any(), (bad.sum(), np.abs(got - want)[bad].max())

    gw = wd.grad.cpu().numpy()
    close_rows(gw[:, 2:2 + D][agree], g_pos[agree], scale[:, 0][agree])
    assert not gw[:, :2].any() and not gw[:, 2 + D:].any()
    if K:
        close_rows(nd.grad.cpu().numpy()[agree], g_neg[agree], scale[:, 1:][agree])


def test_listwise_ok_is_the_kernels_limit():
    from torch_rechub_amd import ops
    u = torch.zeros(2, 16, 64, device=dev())
    pos, neg = torch.zeros(2, 64, device=dev()), torch.zeros(2, 1023, 64, device=dev())
    assert ops.listwise_ok(u, pos, neg)  # (run by test_listwise_shapes_against_float64)
    for uu, pp, nn in ((u, pos, torch.zeros(2, 1024, 64, device=dev())),
                       (torch.zeros(2, 17, 64, device=dev()), pos, neg[:, :3]),
                       (torch.zeros(2, 4, 65, device=dev()), torch.zeros(2, 65, device=dev()),
                        torch.zeros(2, 3, 65, device=dev()))):
        assert not ops.listwise_ok(uu, pp, nn)
        with pytest.raises(RuntimeError, match="no HIP kernel"):
            ops.listwise_logits(uu, pp, nn)


# ---- FFM and CEN ----------------------------------------------------------------------------------------------------
def ffm_tables(F, D, Dp, vocabs, g):
    ws = []
    for v in vocabs:
        w = torch.zeros(v * F, Dp)
        w[:, :D] = torch.randn(v * F, D, generator=g)
        ws.append(w.to(dev()).requires_grad_(True))
    return ws


@pytest.mark.parametrize("itype", [torch.int64, torch.int32])
@pytest.mark.parametrize("B,F,D,Dp", [(20, 64, 1, 4), (20, 64, 128, 128), (4097, 3, 4, 4), (4100, 5, 10, 16)])
def test_fused_ffm_shapes_bit_equal(B, F, D, Dp, itype):
    """F = 64 (P = 2016, the uint8 pair table at its limit) and B > 4096 (the grid-stride loop over samples): the forward
    and the collision-free table gradients are single float32 products, bit for bit."""
    from torch_rechub_amd import ops
    g = torch.Generator().manual_seed(B + F + D)
    vocabs = [B + 1 + f % 3 for f in range(F)]
    ws = ffm_tables(F, D, Dp, vocabs, g)
    idx = [torch.randperm(v, generator=g)[:B].to(itype).to(dev()) for v in vocabs]
    em = ops.ffm_fused(ffm_call(ws, idx, D))
    P = F * (F - 1) // 2
    assert em.shape == (B, P * D)
    np.testing.assert_array_equal(em.detach().cpu().numpy().reshape(B, P, D), np_em(ws, idx, F, D))
    g_em = torch.randn(B, P * D, generator=g)
    em.backward(g_em.to(dev()))
    torch.cuda.synchronize()
    ops.check_errors()
    G = np_table_grads(ws, idx, F, D, g_em.numpy().reshape(B, P, D), [-1] * F, np.float32)
    for f, w in enumerate(ws):
        got = w.grad.cpu().numpy()
        np.testing.assert_array_equal(got, G[f], err_msg=f"field {f}")
        assert not got[:, D:].any()


@pytest.mark.parametrize("B,F,D", [(1, 64, 128), (1, 26, 10), (1, 2, 128), (4097, 2, 1), (4097, 26, 10), (4097, 64, 1)])
@pytest.mark.parametrize("rs", [0, 1])
def test_dense_ffm_shapes_against_numpy(B, F, D, rs):
    from torch_rechub_amd import ops
    g = torch.Generator().manual_seed(B + F + D + rs)
    x = torch.randn(B, F, F, D, generator=g)
    xd = x.to(dev()).requires_grad_(True)
    out = ops.ffm(xd, bool(rs))
    P = F * (F - 1) // 2
    assert out.shape == (B, P, 1 if rs else D)
    if rs:
        np.testing.assert_allclose(out.detach().cpu().numpy(), np_ffm(x.double().numpy(), 1), rtol=1e-4, atol=1e-5)
    else:  # one product per element
        np.testing.assert_array_equal(out.detach().cpu().numpy(), np_ffm(x.numpy(), 0))
    gy = torch.randn(out.shape, generator=g)
    gyd = gy.to(dev())
    poison(B * F * F * D)
    out.backward(gyd)
    gx = xd.grad.cpu().numpy()
    np.testing.assert_array_equal(gx, np_ffm_bwd(x.numpy(), gy.numpy(), rs))  # one float32 product per element
    assert not gx[:, range(F), range(F)].any()  # the diagonal exactly 0


CEN_CASES = [(1, 2016, 128), (63, 325, 10), (64, 2016, 16), (65, 2016, 128), (4096, 2016, 4), (10000, 325, 10)]


def cen_inputs(B, P, D, seed):
    """em as the first P*D columns of a wider (B, P*D + 3) tensor; a few (b, p) rows zero: d = 0 exactly (a ReLU tie)."""
    g = torch.Generator().manual_seed(seed)
    wide = torch.randn(B, P * D + 3, generator=g)
    em3 = wide[:, :P * D].view(B, P, D)
    em3[0, P // 2] = 0.0
    em3[B // 2, 0] = 0.0
    u = torch.randn(P, D, generator=g)
    return wide, u, g


@pytest.mark.parametrize("B,P,D", CEN_CASES)
def test_cen_descriptor_shapes_against_float64(B, P, D):
    from torch_rechub_amd import ops
    wide, u, g = cen_inputs(B, P, D, seed=B + P + D)
    wd = wide.to(dev()).requires_grad_(True)
    ud = u.to(dev()).requires_grad_(True)
    em = wd[:, :P * D]
    assert em.stride(0) == P * D + 3
    d = ops.cen_descriptor(em, ud)
    em64 = wide[:, :P * D].double().numpy().reshape(B, P, D)
    rd = np_cen_desc(em64, u.double().numpy())
    got = d.detach().cpu().numpy()
    np.testing.assert_allclose(got, rd, rtol=1e-4, atol=1e-5 * np.abs(rd).max())
    assert got[0, P // 2] == 0 and got[B // 2, 0] == 0
    gd = torch.randn(B, P, generator=g)
    d.backward(gd.to(dev()))
    # against the ReLU mask of the kernel's own d: a float32 sum within rounding of 0 may take the other side of the tie
    on = got > 0
    assert (on != (rd > 0)).sum() <= max(1, 1e-4 * on.size)  # ... only there
    rg_em, rg_u = np_cen_desc_bwd(em64, u.double().numpy(), gd.double().numpy(), d=got)
    gw = wd.grad.cpu().numpy()
    g_em = gw[:, :P * D].reshape(B, P, D)
    np.testing.assert_array_equal(g_em, np.where(on, gd.numpy(), 0)[..., None] * u.numpy()[None])  # one product each
    np.testing.assert_allclose(g_em, rg_em, rtol=1e-7, atol=0)
    assert not gw[:, P * D:].any()
    assert not gw[0, (P // 2) * D:(P // 2 + 1) * D].any()  # the tie passes no gradient
    np.testing.assert_allclose(ud.grad.cpu().numpy(), rg_u, rtol=1e-4, atol=1e-4 * np.abs(rg_u).max())


def test_cen_u_gradient_is_bitwise_repeatable_over_many_partials():
    from torch_rechub_amd import ops
    B, P, D = 4096, 325, 10
    assert ops._lib.call("rh_cen_nchunks", B) == 64
    wide, u, g = cen_inputs(B, P, D, seed=1)
    gd = torch.randn(B, P, generator=g).to(dev())
    grads = []
    for _ in range(2):
        ud = u.to(dev()).requires_grad_(True)
        ops.cen_descriptor(wide.to(dev())[:, :P * D], ud).backward(gd)
        grads.append(ud.grad.cpu())
    assert torch.equal(grads[0], grads[1])


@pytest.mark.parametrize("B,P,D", CEN_CASES)
def test_cen_rescale_shapes_against_float64(B, P, D):
    from torch_rechub_amd import ops
    wide, _, g = cen_inputs(B, P, D, seed=B * 3 + P + D)
    s = torch.randn(B, P, generator=g)
    wd, sd = wide.to(dev()).requires_grad_(True), s.to(dev()).requires_grad_(True)
    out = ops.cen_rescale(wd[:, :P * D], sd)
    assert out.shape == (B, P * D)
    em32 = wide[:, :P * D].numpy().reshape(B, P, D)
    np.testing.assert_array_equal(out.detach().cpu().numpy(), (s.numpy()[..., None] * em32).reshape(B, -1))
    gwide = torch.randn(B, P * D + 5, generator=g)
    gs = gwide.to(dev())[:, 1:1 + P * D]  # a strided upstream gradient
    assert gs.stride(0) == P * D + 5
    out.backward(gs)
    g32 = gwide[:, 1:1 + P * D].numpy().reshape(B, P, D)
    rg_em, rg_s = np_cen_rescale_bwd(em32.astype(np.float64), s.double().numpy(), g32.astype(np.float64))
    gw = wd.grad.cpu().numpy()
    np.testing.assert_array_equal(gw[:, :P * D], (s.numpy()[..., None] * g32).reshape(B, -1))  # one product each
    assert not gw[:, P * D:].any()
    np.testing.assert_allclose(sd.grad.cpu().numpy(), rg_s, rtol=1e-4, atol=1e-5 * np.abs(rg_s).max())


# ---- the empty batch ----------------------------------------------------------------------------------------------
def test_empty_batch_through_the_new_ops():
    from torch_rechub_amd import ops
    L, I, D = 8, 4, 16
    mask = torch.zeros(0, L, dtype=torch.int32, device=dev())
    for kind in (0, 1, 2):
        x = torch.zeros(0, L, I * D if kind == 1 else D, device=dev(), requires_grad=True)
        w = torch.randn(1, L, I * D, D, device=dev(), requires_grad=True) if kind == 2 else None
        cap = ops.capsule_routing(x, w, mask, None, kind, I, D, 3)
        assert cap.shape == (0, I, D)
        cap.sum().backward()
        assert x.grad.shape == x.shape
        if kind == 2:
            assert w.grad.shape == w.shape and not w.grad.any()
    A = torch.zeros(0, L, I, device=dev(), requires_grad=True)
    E = torch.zeros(0, L, D, device=dev(), requires_grad=True)
    out = ops.sa_pool(A, E, mask)
    assert out.shape == (0, I, D)
    out.sum().backward()
    assert A.grad.shape == A.shape and E.grad.shape == E.shape
    u = torch.zeros(0, I, D, device=dev(), requires_grad=True)
    pos = torch.zeros(0, D, device=dev(), requires_grad=True)
    neg = torch.zeros(0, 5, D, device=dev(), requires_grad=True)
    logits, best = ops.listwise_logits(u, pos, neg, 0.02)
    assert logits.shape == (0, 6) and best.shape == (0,)
    logits.sum().backward()
    assert u.grad.shape == u.shape and neg.grad.shape == neg.shape
    F, Dp = 4, 8
    ws = ffm_tables(F, 6, Dp, [5] * F, torch.Generator().manual_seed(0))
    em = ops.ffm_fused(ffm_call(ws, [torch.zeros(0, dtype=torch.int64, device=dev()) for _ in range(F)], 6))
    assert em.shape == (0, 6 * 6)
    em.sum().backward()
    assert all(w.grad is None or not w.grad.any() for w in ws)
    x = torch.zeros(0, F, F, 6, device=dev(), requires_grad=True)
    for rs in (False, True):
        y = ops.ffm(x, rs)
        assert y.shape == (0, 6, 1 if rs else 6)
        y.sum().backward()
    assert x.grad.shape == x.shape
    em2 = torch.zeros(0, 6 * 5, device=dev(), requires_grad=True)
    uu = torch.randn(6, 5, device=dev(), requires_grad=True)
    d = ops.cen_descriptor(em2, uu)
    assert d.shape == (0, 6)
    d.sum().backward()
    assert not uu.grad.any() and em2.grad.shape == em2.shape
    s = torch.zeros(0, 6, device=dev(), requires_grad=True)
    y = ops.cen_rescale(em2, s)
    assert y.shape == (0, 30)
    y.sum().backward()
    assert s.grad.shape == (0, 6)
    ops.check_errors()
