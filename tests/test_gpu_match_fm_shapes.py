"""The four stand-alone kernel pairs every retrieval model trains through -- the in-batch logits, the L2 normalisation and
the mean cross-entropy of csrc/match.hip, and the stand-alone FM term of csrc/fm.hip -- against float64 over their supported
shape range: every register width of the in-batch dispatch and both sides of each switch, every lane-group width of FM,
strided operands passed in place, the second trip of every capped launch, the largest shape each guard accepts and the
refusal one past it, duplicate / extreme / out-of-range indices, norms around eps, special softmax rows, bitwise repeats,
the host-side guards of the two ops that read int64 words, and a MatchTrainer in-batch step on the fused path against the
same step on the score-matrix path.

Bounds.  Every comparison is kernel against float64 (tests/match_oracle.py, pinned by tests/test_match_host.py;
oracle/ctr_oracle.py for FM) under the rule of test_gpu_session_hllm_shapes.py::compare: rtol |want| plus the larger of a
floor times the tensor's largest magnitude and 4 x the error of an fp32 torch evaluation of the same case on the CPU against
the same float64 numbers.  Floors and rtol are those of the existing test of the same tensor in test_gpu_kernels.py: 2e-5
(in-batch), 1e-6 / rtol 1e-5 (normalised rows), 2e-6 / rtol 2e-5 (their gradient), 1e-5 of max(1, |loss|) (the loss),
1e-7 / rtol 1e-5 (g_logits), 1e-6 / rtol 1e-5 (FM).  Each comparison prints one table line (pytest -s)."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch

import match_oracle as O
from oracle import ctr_oracle as CTR
from test_gpu_session_hllm_shapes import compare, poison_small_blocks
from test_gpu_twotower import noise_biases, strided

pytestmark = pytest.mark.gpu

F64 = np.float64


def dev():
    return torch.device("cuda:0")


@contextlib.contextmanager
def recorded_calls(*names):
    """The C entry points the ops go through while the block runs, as (name, args); every name when none is given."""
    from torch_rechub_amd import _lib
    seen, real = [], _lib.call

    def spy(name, *args):
        if not names or name in names:
            seen.append((name, args))
        return real(name, *args)

    _lib.call = spy
    try:
        yield seen
    finally:
        _lib.call = real


def raw():
    from torch_rechub_amd import _lib, ops
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    return _lib, ops, p, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.c_void_p(0)


def refused(_lib, rc, name, *args):
    with pytest.raises(RuntimeError, match=r"rc=%d\)" % rc):
        _lib.call(name, *args)


# ---- in-batch logits ----------------------------------------------------------------------------------------------------------
def inbatch_case(B, C, D, K, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(B, D, generator=g), torch.randn(C, D, generator=g), torch.randint(0, C, (B, K), generator=g),
            torch.randn(B, 1 + K, generator=g))


def inbatch_cpu32(u, v, neg, gl, row0):
    """The same 1 + K dot products per row in fp32 torch on the CPU, gathered form (no (B, C) matrix at the large case)."""
    uc, vc = u.clone().requires_grad_(True), v.clone().requires_grad_(True)
    idx = torch.from_numpy(O.inbatch_index(neg.numpy(), u.shape[0], row0))
    logits = (uc[:, None, :] * vc[idx]).sum(-1)
    logits.backward(gl)
    return logits.detach(), uc.grad, vc.grad


def run_inbatch(u, v, neg, gl, row0, stride=False):
    from torch_rechub_amd import ops
    poison_small_blocks()
    ud = (strided(u, 3) if stride else u.to(dev())).requires_grad_(True)
    vd = (strided(v, 5) if stride else v.to(dev())).requires_grad_(True)
    assert ops.inbatch_logits_ok(ud, vd)
    with recorded_calls("rh_inbatch_logits_fwd", "rh_inbatch_logits_bwd") as seen:
        logits = ops.inbatch_logits(ud, vd, neg.to(dev()), row0)
        logits.backward(gl.to(dev()))
    if stride:  # the rows went to both kernels in place
        assert [(a[1], a[3]) for _, a in seen] == [(u.shape[1] + 3, v.shape[1] + 5)] * 2
    ops.check_errors()
    return logits.detach(), ud.grad, vd.grad


def check_inbatch(case, u, v, neg, gl, row0, **kw):
    got = run_inbatch(u, v, neg, gl, row0, **kw)
    want = (O.inbatch_forward(u, v, neg, row0),) + O.inbatch_backward(u, v, neg, gl, row0)
    fails = []
    for name, a, b, c in zip(("logits", "g_u", "g_v"), got, want, inbatch_cpu32(u, v, neg, gl, row0)):
        compare(case, name, a, b, c, 2e-5, fails)
    assert not fails, fails
    return got


@pytest.mark.parametrize("D", [1, 64, 65, 129, 256, 257, 513, 1024])
def test_inbatch_logits_every_register_width_strided(D):
    """PL = 1 (D 1, 64), 2 (65), 4 (129, 256), 8 (257), 16 (513, 1024): one width per instantiation and both sides of each
    switch, user rows of stride D + 3 and item rows of stride D + 5 with NaN in the gaps."""
    check_inbatch(f"inbatch_D{D}", *inbatch_case(7, 9, D, 3, 300 + D), 2, stride=True)


@pytest.mark.parametrize("B,C,K,row0", [(1, 1, 0, 0), (4, 4, 3, 0), (5, 5, 4, 0), (33, 40, 7, 7), (3, 50, 49, 47)])
def test_inbatch_logits_batch_shapes(B, C, K, row0):
    """One row and no negative; a full and a partial workgroup of four rows; a rank's slice of a wider batch; the last rows of
    a batch with K = C - 1."""
    check_inbatch(f"inbatch_B{B}_C{C}_K{K}", *inbatch_case(B, C, 12, K, 400 + B), row0)


def test_inbatch_logits_duplicate_and_extreme_indices():
    """Row 0 names item 10 four times, row 1 names its own positive (item 3) four times, row 2 names items 0 and C - 1; the
    other rows draw from {0, 9, 11}.  Items 1 and 8 are named by nobody: their gradient rows are exact zeros.  Item 3 is hit
    only by row 1, five times: its gradient is the sum of all 1 + K terms."""
    B, C, D, K, row0 = 6, 12, 12, 4, 2
    u, v, neg, gl = inbatch_case(B, C, D, K, 17)
    neg[0] = 10
    neg[1] = row0 + 1
    neg[2] = torch.tensor([0, C - 1, 0, C - 1])
    neg[3:] = torch.tensor([0, 9, 11])[torch.randint(0, 3, (3, K), generator=torch.Generator().manual_seed(1))]
    _, _, g_v = check_inbatch("inbatch_duplicates", u, v, neg, gl, row0)
    assert not g_v[[1, 8]].any()
    fails = []
    compare("inbatch_duplicates", "g_v[3] = sum of 1 + K", g_v[3], gl[1].double().sum().item() * u[1].double().numpy(),
            gl[1].sum() * u[1], 2e-5, fails)
    compare("inbatch_duplicates", "g_v[10] = sum of K", g_v[10], gl[0, 1:].double().sum().item() * u[0].double().numpy(),
            gl[0, 1:].sum() * u[0], 2e-5, fails)
    assert not fails, fails


def test_inbatch_logits_past_the_caps_first_trip():
    """4096 workgroups of four wavefronts cover 16384 rows a trip: one row more takes the row loop round again."""
    B = 4096 * 4 + 1
    check_inbatch("inbatch_past_cap", *inbatch_case(B, B, 4, 1, 5), 0)


def test_inbatch_logits_and_user_gradient_twice_are_bitwise_equal():
    """logits and g_u have a fixed summation order.  g_v is accumulated with float atomics and is not asserted bit-equal."""
    case = inbatch_case(67, 80, 130, 5, 6)
    a, b = run_inbatch(*case, 9, stride=True), run_inbatch(*case, 9, stride=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_inbatch_logits_out_of_range_index_sets_the_error_word_and_spares_the_rest():
    """An index equal to C and an index of -1 take the kernel's clamp branch (item 0 is read instead, the error word is
    set): check_errors raises once, and every other logit is the oracle's.  Forward only."""
    from torch_rechub_amd import ops
    B, C, D, K = 5, 7, 12, 3
    u, v, neg, _ = inbatch_case(B, C, D, K, 23)
    neg[1, 2], neg[3, 0] = C, -1
    ops.check_errors()
    poison_small_blocks()
    with torch.no_grad():
        logits = ops.inbatch_logits(u.to(dev()), v.to(dev()), neg.to(dev()), 0)
    with pytest.raises(IndexError):
        ops.check_errors()
    ops.check_errors()  # the word was cleared
    clean = neg.clone()
    clean[1, 2], clean[3, 0] = 0, 0
    keep = np.ones((B, 1 + K), bool)
    keep[1, 3], keep[3, 1] = False, False
    cpu32 = inbatch_cpu32(u, v, clean, torch.zeros(B, 1 + K), 0)[0]
    fails = []
    compare("inbatch_out_of_range", "other logits", logits.cpu().numpy()[keep], O.inbatch_forward(u, v, clean, 0)[keep],
            cpu32.numpy()[keep], 2e-5, fails)
    assert not fails, fails


def test_inbatch_logits_refusals_touch_nothing():
    _lib, ops, p, st, null = raw()
    x = torch.randn(4, 1025, device=dev())
    neg = torch.zeros(4, 2, dtype=torch.int64, device=dev())
    g = torch.randn(4, 3, device=dev())
    logits = torch.full((4, 3), 7.0, device=dev())
    g_u, g_v = torch.full((4, 1025), 7.0, device=dev()), torch.full((4, 1025), 7.0, device=dev())
    err = ops.err_flag(dev())

    def fwd(u, ldu, v, B, C, D, row0, out):
        return ("rh_inbatch_logits_fwd", u, ldu, v, 1025, p(neg), B, C, D, 2, row0, out, p(err), st)

    def bwd(u, ldu, v, B, C, D, row0, out):
        return ("rh_inbatch_logits_bwd", u, ldu, v, 1025, p(neg), p(g), B, C, D, 2, row0, out, p(g_v), st)

    for call, out in ((fwd, logits), (bwd, g_u)):
        refused(_lib, -2, *call(p(x), 1025, p(x), 4, 4, 1025, 0, p(out)))  # one past the widest width
        refused(_lib, -1, *call(p(x), 1025, null, 4, 4, 8, 0, p(out)))     # a null pointer
        refused(_lib, -1, *call(p(x), 1025, p(x), 4, 4, 8, 0, null))
        refused(_lib, -1, *call(p(x), 7, p(x), 4, 4, 8, 0, p(out)))        # ldu < D
        refused(_lib, -1, *call(p(x), 1025, p(x), 4, 4, 8, 1, p(out)))     # row0 + B > C
    torch.cuda.synchronize()
    assert (logits == 7.0).all() and (g_u == 7.0).all() and (g_v == 7.0).all()
    ops.check_errors()
    assert not ops.inbatch_logits_ok(x, x) and ops.inbatch_logits_ok(x[:, :1024], x[:, :1024])


def test_inbatch_logits_host_guards_raise_before_any_launch():
    """The kernel reads the negatives as int64 words: an int32 tensor would be read past its end.  Each guard raises before
    the first C entry point is called, and the error word stays clear."""
    from torch_rechub_amd import ops
    u, v, neg, _ = (t.to(dev()) for t in inbatch_case(4, 6, 8, 3, 1))
    ops.check_errors()
    with recorded_calls() as seen:
        for bad in (neg.to(torch.int32), neg.reshape(-1), neg[:3], neg.reshape(4, 3, 1)):
            with pytest.raises(ValueError, match="int64"):
                ops.inbatch_logits(u, v, bad, 0)
        with pytest.raises(ValueError, match="one width"):
            ops.inbatch_logits(u, v[:, :7], neg, 0)
    assert seen == []
    ops.check_errors()


# ---- L2 normalise ---------------------------------------------------------------------------------------------------------------
def l2_cpu32(x, gy):
    xc = x.clone().requires_grad_(True)
    y = torch.nn.functional.normalize(xc, p=2, dim=1)
    y.backward(gy)
    return y.detach(), xc.grad


def run_l2(x, gy, stride=True, check_raw=True):
    """-> (y, g_x) through the op; the raw entry points on the same strided buffers must give the same bits."""
    _lib, ops, p, st, _ = raw()
    poison_small_blocks()
    B, d = x.shape
    xs = (strided(x, 4) if stride else x.to(dev())).requires_grad_(True)
    gs = strided(gy, 8) if stride else gy.to(dev())
    assert ops.l2_normalize_ok(xs)
    with recorded_calls("rh_l2norm_fwd", "rh_l2norm_bwd") as seen:
        y = ops.l2_normalize(xs)
        y.backward(gs)
    if stride:  # both strided operands went to the kernels in place
        assert (seen[0][1][1], seen[1][1][3]) == (d + 4, d + 8)
    if check_raw:
        y2, gx2 = torch.full((B, d), 7.0, device=dev()), torch.full((B, d), 7.0, device=dev())
        nrm = torch.full((B,), 7.0, device=dev())
        _lib.call("rh_l2norm_fwd", p(xs), xs.stride(0), B, d, 1e-12, p(y2), p(nrm), st)
        _lib.call("rh_l2norm_bwd", p(y2), p(nrm), p(gs), gs.stride(0), B, d, 1e-12, p(gx2), st)
        assert torch.equal(y2, y) and torch.equal(gx2, xs.grad)
    return y.detach(), xs.grad


def check_l2(case, x, gy, rows=False, **kw):
    y, gx = run_l2(x, gy, **kw)
    want_y, want_g = O.l2norm_forward(x), O.l2norm_backward(x, gy)
    cy, cg = l2_cpu32(x, gy)
    fails = []
    for r in (range(x.shape[0]) if rows else [slice(None)]):
        tag = f"{case} row {r}" if rows else case
        compare(tag, "y", y[r], want_y[r], cy[r], 1e-6, fails, rtol=1e-5)
        compare(tag, "g_x", gx[r], want_g[r], cg[r], 2e-6, fails, rtol=2e-5)
    assert not fails, fails
    return y, gx


def l2_case(B, d, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, d, generator=g), torch.randn(B, d, generator=g)


@pytest.mark.parametrize("d", [4, 60, 64, 68, 128, 1028, 4096])
def test_l2_normalize_widths_and_batches_strided(d):
    """One float4; one short of, exactly and one float4 past a 64-float chunk; two chunks; a ragged 17th; the widest.
    B = 16 fills one workgroup, 17 and 33 leave a partial last one.  x has row stride d + 4, the upstream gradient d + 8."""
    for B in (1, 16, 17, 33):
        check_l2(f"l2_B{B}_d{d}", *l2_case(B, d, 500 + B + d))


@pytest.mark.parametrize("d", [8, 68])
def test_l2_normalize_norm_edges_row_by_row(d):
    """Rows of norm 0, 5e-13 (below eps), 2e-12 (just above), 1e-10, with elements of magnitude 1e15, and an ordinary one.
    The clamped rows' gradients are g / eps, 1e12 times the others: every row is compared on its own."""
    x, gy = l2_case(6, d, 40 + d)
    x[0] = 0.0
    for r, n in ((1, 5e-13), (2, 2e-12), (3, 1e-10)):
        x[r] = (x[r].double() * (n / x[r].double().norm())).float()
    x[4] = torch.sign(x[4]) * 1e15
    _, gx = check_l2(f"l2_edges_d{d}", x, gy, rows=True)
    norms = x.double().norm(dim=1)
    assert norms[1] < 1e-12 < norms[2] < 3e-12
    assert torch.isfinite(gx).all()


def test_l2_normalize_past_the_caps_first_trip():
    """8192 workgroups of 16 rows cover 131072 rows a trip."""
    B = 8192 * 16 + 1
    check_l2("l2_past_cap", *l2_case(B, 4, 8), stride=False, check_raw=False)


def test_l2_normalize_twice_is_bitwise_equal():
    x, gy = l2_case(33, 68, 12)
    a, b = run_l2(x, gy), run_l2(x, gy)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_l2_normalize_refusals_touch_nothing():
    _lib, ops, p, st, null = raw()
    x = torch.randn(4, 4100, device=dev())
    out = torch.full((4, 4100), 7.0, device=dev())
    nrm = torch.full((4,), 7.0, device=dev())
    for d, ld in ((4100, 4100), (6, 8), (8, 10)):  # one past the widest; no multiple of four; a stride that is none
        refused(_lib, -2, "rh_l2norm_fwd", p(x), ld, 4, d, 1e-12, p(out), p(nrm), st)
        refused(_lib, -2, "rh_l2norm_bwd", p(x), p(nrm), p(x), ld, 4, d, 1e-12, p(out), st)
    refused(_lib, -1, "rh_l2norm_fwd", p(x), 4100, 4, 8, 1e-12, null, p(nrm), st)
    refused(_lib, -1, "rh_l2norm_bwd", p(x), p(nrm), null, 4100, 4, 8, 1e-12, p(out), st)
    _lib.call("rh_l2norm_fwd", p(x), 4100, 0, 8, 1e-12, p(out), p(nrm), st)  # B = 0: accepted, nothing written
    _lib.call("rh_l2norm_bwd", p(x), p(nrm), p(x), 4100, 0, 8, 1e-12, p(out), st)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (nrm == 7.0).all()
    assert not ops.l2_normalize_ok(x) and not ops.l2_normalize_ok(x[:, :6]) and not ops.l2_normalize_ok(x[:0, :8])
    assert ops.l2_normalize_ok(x[:, :4096])
    # a row stride that is no multiple of four is the op's to repack, not the kernel's to read
    t, _ = l2_case(5, 8, 3)
    odd = strided(t, 2)
    assert ops.l2_normalize_ok(odd)
    fails = []
    compare("l2_odd_stride", "y", ops.l2_normalize(odd), O.l2norm_forward(t), l2_cpu32(t, t)[0], 1e-6, fails, rtol=1e-5)
    assert not fails, fails


# ---- cross-entropy --------------------------------------------------------------------------------------------------------------
UP = 1.7  # upstream gradient of the loss, as in test_gpu_kernels.py


def ce_case(B, C, seed, with_target=True):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, generator=g) * 20
    if not with_target:
        return x, None
    t = torch.randint(0, C, (B,), generator=g)
    t[0], t[-1] = 0, C - 1
    return x, t


def run_ce(x, target):
    from torch_rechub_amd import ops
    poison_small_blocks()
    xd = x.to(dev()).requires_grad_(True)
    td = None if target is None else target.to(dev())
    assert ops.cross_entropy_ok(torch.nn.CrossEntropyLoss(), xd, td)
    loss = ops.cross_entropy_mean(xd, td)
    (loss * UP).backward()
    ops.check_errors()
    return loss.detach().reshape(1), xd.grad


def check_ce(case, x, target):
    loss, gx = run_ce(x, target)
    tn = None if target is None else target.numpy()
    xc = x.clone().requires_grad_(True)
    closs = torch.nn.CrossEntropyLoss()(xc, target if target is not None else torch.zeros(x.shape[0], dtype=torch.long))
    (closs * UP).backward()
    fails = []
    compare(case, "loss", loss, np.array([O.ce_forward(x, tn)]), closs.detach().reshape(1), 1e-5, fails, scale_min=1.0)
    compare(case, "g_logits", gx, O.ce_backward(x, tn, UP), xc.grad, 1e-7, fails, rtol=1e-5)
    assert not fails, fails
    return loss, gx


@pytest.mark.parametrize("with_target", [True, False])
@pytest.mark.parametrize("B,C", [(1, 1), (255, 2), (256, 63), (257, 64), (513, 65), (1, 1023), (257, 1024), (37, 5), (33, 9),
                                 (300, 21)])
def test_cross_entropy_class_counts_and_batches(B, C, with_target):
    """C from one class to the 1024 the guard admits, both sides of 64; B one short of, exactly and one past a workgroup of
    256 rows, and three workgroups.  Targets include class 0 and class C - 1; None is class 0 everywhere.  The last three
    are the backward's lane groups of 8, 16 and 32 (C = 1, 2 take 4 lanes a row, 63 and wider 64), each with a partly
    filled last workgroup.

    Found with this test: the backward used to read the forward's lse back, exp(x - lse).  lse = fl(m + log s) carries half
    an ulp of a number near the largest logit, which at the target becomes the absolute error of p - 1: g_logits missed this
    bound at (255, 2) by 5.1e-9 against 2.7e-9 and 8.8e-9 against 2.9e-9, at (257, 64) by 1.0e-8 against 4.1e-9, at
    (513, 65) by 4.7e-9 against 2.2e-9 and at (4097, 257) by 6.7e-10 against 4.0e-10.  The backward now takes the row's
    maximum and sum again, exp((x - m) - log s), and stays under 0.8 of the bound everywhere."""
    check_ce(f"ce_B{B}_C{C}_{'t' if with_target else 'none'}", *ce_case(B, C, B * 3 + C, with_target))


def test_cross_entropy_special_rows():
    """All entries equal: the term is log C and the gradient (1/C - onehot)/B.  One logit at +1e4 over -1e4 elsewhere: the
    term is exactly 0 with the target on the large entry, and 2e4 with it elsewhere."""
    from torch_rechub_amd import ops
    C = 7
    x = torch.full((3, C), 3.25)
    x[1:] = -1e4
    x[1, 2] = x[2, 2] = 1e4
    t = torch.tensor([4, 2, 0])
    _, gx = check_ce("ce_special_rows", x, t)
    onehot = np.eye(C)[t.numpy()]
    fails = []
    want = UP * (1.0 / C - onehot[0]) / 3
    compare("ce_special_rows", "equal row's gradient", gx[0], want, want.astype(np.float32), 1e-7, fails, rtol=1e-5)
    terms = []
    for r in range(3):
        poison_small_blocks()
        terms.append(ops.cross_entropy_mean(x[r:r + 1].to(dev()), t[r:r + 1].to(dev())).item())
    ops.check_errors()
    compare("ce_special_rows", "log C", np.array([terms[0]]), np.array([np.log(C)]), torch.log(torch.tensor([float(C)])),
            1e-5, fails, scale_min=1.0)
    assert not fails, fails
    assert terms[1] == 0.0 and terms[2] == 2e4


@pytest.mark.parametrize("B,C", [(4097, 257), (4096 * 4 + 1, 33)])
def test_cross_entropy_past_the_backward_cap(B, C):
    """The backward is capped at 4096 workgroups of 256 / G rows.  4097 x 257 was one trip and 17 workgroups of the
    element-wise backward this kernel had; 16385 rows of 64 lanes are one row past the first trip of the row-wise one."""
    check_ce(f"ce_past_cap_B{B}_C{C}", *ce_case(B, C, 31))


def test_cross_entropy_twice_is_bitwise_equal():
    x, t = ce_case(513, 65, 77)
    a, b = run_ce(x, t), run_ce(x, t)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("bad", ["C", -1, -100])
def test_cross_entropy_out_of_range_target_sets_the_error_word(bad):
    """Both kernels clamp such a target to class 0 and the forward sets the error word: check_errors raises once, and a clean
    call afterwards passes."""
    from torch_rechub_amd import ops
    x, t = ce_case(5, 4, 3)
    dirty = t.clone()
    dirty[2] = 4 if bad == "C" else bad
    ops.check_errors()
    xd = x.to(dev()).requires_grad_(True)
    ops.cross_entropy_mean(xd, dirty.to(dev())).backward()
    with pytest.raises(IndexError):
        ops.check_errors()
    assert torch.isfinite(xd.grad).all()
    check_ce("ce_after_bad_target", x, t)


def test_cross_entropy_refusals_touch_nothing():
    _lib, ops, p, st, null = raw()
    x = torch.randn(4, 1025, device=dev())
    t = torch.zeros(4, dtype=torch.int64, device=dev())
    one = torch.ones(1, device=dev())
    out = torch.full((4, 1025), 7.0, device=dev())
    lse, part = torch.full((4,), 7.0, device=dev()), torch.full((4,), 7.0, device=dev())
    err = ops.err_flag(dev())
    for B, C in ((4, 1025), (0, 8)):  # one class past the guard; an empty batch
        refused(_lib, -2, "rh_ce_fwd", p(x), p(t), B, C, p(lse), p(part), p(err), st)
        refused(_lib, -2, "rh_ce_bwd", p(x), p(t), p(lse), p(one), B, C, p(out), st)
    refused(_lib, -1, "rh_ce_fwd", p(x), p(t), 4, 8, null, p(part), p(err), st)
    refused(_lib, -1, "rh_ce_bwd", p(x), p(t), p(lse), p(one), 4, 8, null, st)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (lse == 7.0).all() and (part == 7.0).all()
    ops.check_errors()
    crit = torch.nn.CrossEntropyLoss()
    assert not ops.cross_entropy_ok(crit, x, t) and ops.cross_entropy_ok(crit, x[:, :1024], t)


def test_cross_entropy_host_guards_raise_before_any_launch():
    """The kernels read the targets as int64 words through a device pointer: an int32, a mis-shaped or a host tensor is
    refused before the first C entry point is called."""
    from torch_rechub_amd import ops
    x, t = ce_case(5, 4, 3)
    xd, td = x.to(dev()), t.to(dev())
    ops.check_errors()
    with recorded_calls() as seen:
        for bad in (td.to(torch.int32), td[:4], td.reshape(5, 1), t):
            with pytest.raises(ValueError, match="int64"):
                ops.cross_entropy_mean(xd, bad)
    assert seen == []
    ops.check_errors()


# ---- FM -------------------------------------------------------------------------------------------------------------------------
def fm_case(B, F, D, rs, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, F, D, generator=g), torch.randn((B, 1) if rs else (B, D), generator=g)


def fm_cpu32(x, gy, rs):
    xc = x.clone().requires_grad_(True)
    ix = xc.sum(1) ** 2 - (xc ** 2).sum(1)
    y = 0.5 * (ix.sum(1, keepdim=True) if rs else ix)
    y.backward(gy)
    return y.detach(), xc.grad


def run_fm(x, gy, rs, stride):
    from torch_rechub_amd import ops
    poison_small_blocks()
    B, F, D = x.shape
    xd = (strided(x.reshape(B, F * D), 7).view(B, F, D) if stride else x.to(dev())).requires_grad_(True)
    with recorded_calls("rh_fm_fwd") as seen:
        y = ops.fm(xd, rs)
    if stride and B > 1:  # the sample stride went to the kernel in place (one sample has none)
        assert seen[0][1][1] == F * D + 7
    y.backward(gy.to(dev()))
    return y.detach(), xd.grad


def check_fm(case, x, gy, rs, stride):
    y, gx = run_fm(x, gy, rs, stride)
    x64 = x.numpy().astype(F64)
    cy, cg = fm_cpu32(x, gy, rs)
    fails = []
    # the two terms being subtracted are each about F max|x|^2: the cancellation error is measured against that
    compare(case, "out", y, CTR.fm_forward(x64, rs), cy, 1e-6, fails, rtol=1e-5, scale_min=x.shape[1] * float(x.abs().max()) ** 2)
    compare(case, "g_x", gx, CTR.fm_backward(x64, gy.numpy().astype(F64), rs), cg, 1e-6, fails, rtol=1e-5)
    assert not fails, fails
    return y, gx


@pytest.mark.parametrize("D", [1, 3, 4, 5, 8, 9, 17, 32, 33, 64, 65, 130])
def test_fm_every_lane_group_width(D):
    """G = 4 (D 1..4), 8 (5, 8), 16 (9), 32 (17, 32), 64 (33 and wider); 65 takes the d loop a second trip, 130 a ragged
    third.  65 samples never fill the last workgroup: its dead lane groups read row B - 1 and take part in the shuffles.
    Once contiguous, once as a (B, F, D) view of a (B, F D + 7) buffer."""
    for F in (1, 2, 39):
        for B in (1, 65):
            for rs in (True, False):
                for stride in (False, True):
                    check_fm(f"fm_B{B}_F{F}_D{D}_{'sum' if rs else 'vec'}{'_strided' if stride else ''}",
                             *fm_case(B, F, D, rs, 1000 * D + 10 * F + B), rs, stride)


@pytest.mark.parametrize("D", [3, 64, 130])
def test_fm_with_one_field_stays_within_the_rounding_error_of_a_square(D):
    """With one field the float64 result is exactly 0.  The kernel's ``s * s - ss`` is contracted to one fma against the
    already rounded ss = fl(x^2), so it returns the rounding error of x^2 (at most 2^-24 x^2 per element), not the
    reference's exact 0.  The kernel is left as it is: the output is held to the bound of every other case, floor 1e-6 of
    F max|x|^2, and the gradient, g (s - x) with s = x, is exactly 0."""
    for rs in (True, False):
        x, gy = fm_case(65, 1, D, rs, 70 + D)
        y, gx = check_fm(f"fm_one_field_D{D}_{'sum' if rs else 'vec'}", x, gy, rs, False)
        assert not gx.any()
        assert float(y.abs().max()) <= 1e-6 * float(x.abs().max()) ** 2


def test_fm_twice_is_bitwise_equal():
    for rs in (True, False):
        x, gy = fm_case(65, 39, 33, rs, 5)
        a, b = run_fm(x, gy, rs, True), run_fm(x, gy, rs, True)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


# ---- the trainer: the fused in-batch step against the score-matrix step ------------------------------------------------------------
def test_match_trainer_fused_in_batch_steps_follow_the_score_matrix_steps():
    """Three Adam steps of the dssm fixture with three random in-batch negatives: the default trainer (ops.inbatch_logits +
    ops.cross_entropy_mean) against deterministic_logits=True (u @ v.T, gather, torch's loss).  Both draw the same negatives
    from the same seed: the sampler's call counter is process-wide per (device, seed), so it is reset before each trainer,
    as test_gpu_models.py does for its twins."""
    from conftest import assert_trajectory_close, build_amd_model, features_from_spec, golden_batch, golden_state, load_golden
    from torch_rechub_amd import ops
    from torch_rechub_amd.trainers import MatchTrainer
    gold = load_golden("model_dssm.npz")
    lr, steps = float(gold["train.lr"]), 3
    batches = [golden_batch(gold, i) for i in range(steps)]
    names = ("inbatch_logits", "inbatch_sample", "cross_entropy_mean")
    orig = {n: getattr(ops, n) for n in names}
    loss_ok = ops.cross_entropy_ok
    runs = []
    for deterministic in (False, True):
        model = build_amd_model("dssm", features_from_spec(gold["spec"]))
        model.load_state_dict(golden_state(gold, "sd0."))
        trainer = MatchTrainer(model.to(dev()), mode=0, in_batch_neg=True, in_batch_neg_ratio=3, sampler_seed=11,
                               optimizer_params={"lr": lr, "weight_decay": float(gold["train.wd"])}, n_epoch=1,
                               device="cuda:0", show_progress=False, use_graph=False, deterministic_logits=deterministic)
        calls = {n: [] for n in names}

        def counted(n, calls=calls):
            def fn(*a, **k):
                out = orig[n](*a, **k)
                calls[n].append(out.detach().clone())
                return out
            return fn

        ops._sample_rng.clear()
        try:
            for n in names:
                setattr(ops, n, counted(n))
            if deterministic:  # torch's loss on that side, not the fused one
                ops.cross_entropy_ok = lambda *a, **k: False
            loss = trainer.train_one_epoch(batches)
        finally:
            ops.cross_entropy_ok = loss_ok
            for n in names:
                setattr(ops, n, orig[n])
        ops.check_errors()
        runs.append((loss, calls, {k: v.detach().cpu().numpy() for k, v in model.state_dict().items()}, model))
    (loss_f, calls_f, state_f, model), (loss_d, calls_d, state_d, _) = runs
    assert len(calls_f["inbatch_logits"]) == steps and len(calls_d["inbatch_logits"]) == 0
    assert len(calls_f["cross_entropy_mean"]) == steps and len(calls_d["cross_entropy_mean"]) == 0
    assert len(calls_f["inbatch_sample"]) == len(calls_d["inbatch_sample"]) == steps
    for a, b in zip(calls_f["inbatch_sample"], calls_d["inbatch_sample"]):
        assert torch.equal(a, b)  # random_inbatch_negatives and inbatch_negative_sampling: one stream
    print(f"| trainer | mean loss | fused {loss_f:.8f} | score matrix {loss_d:.8f} |")
    assert np.isfinite([loss_f, loss_d]).all() and abs(loss_f - loss_d) <= 1e-4 * abs(loss_d)
    noise = noise_biases(model)
    for k, want in state_d.items():
        got = state_f[k]
        if want.dtype.kind != "f":
            assert np.array_equal(got, want), k
        elif k in noise:  # no defined trajectory under Adam: the sign of rounding noise becomes +-lr steps (conftest's rule)
            assert np.abs(got - want).max() <= 2.1 * lr * steps, k
        elif k.endswith("running_mean"):  # carries the drift of the bias above one-for-one
            assert np.abs(got - want).max() <= 0.5 * lr * steps, k
        else:
            assert_trajectory_close(got, want, lr * steps, f"dssm in-batch: {k} fused vs score matrix")
