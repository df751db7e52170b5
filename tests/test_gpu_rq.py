"""The residual quantizer kernels of csrc/rq.hip on the MI355X against the float64 restatement of test_rqvae_host.py.

Inputs: one seeded generator draws x (N, E), then each codebook in level order.  argmin is a discontinuity: a row is
compared only if its float64 gap (d_2 - d_1) / (||r||^2 + max_k ||c_k||^2) is at least 1e-4 at every level -- fp32
rounding of an E-term sum is near 1e-5 relative, a tenfold margin.  Rows are excluded by the oracle's numbers alone, at
most 2 % of them (these draws exclude 0, 0, 0, 2, 3 and 0 rows); their upstream gradient is zeroed on both sides.  The
losses and the codebook gradient sum over all rows: the oracle takes the kernel's own indices at the excluded rows, where
both codes are an argmin to within rounding.  Tolerances are those of test_gpu_sine.py: rtol 1e-4, atol 1e-5 of the
tensor's largest magnitude; g_C: atol 1e-4 of it."""
import numpy as np
import pytest
import torch

from test_rqvae_host import draw_inputs, np_rq_backward, np_rq_forward
from torch_rechub_amd._lib import H

pytestmark = pytest.mark.gpu

BETA, G_LOSS = 0.25, 1.3
MIN_GAP, MAX_EXCLUDED = 1e-4, 0.02
#          N    E    sizes            seed
CASES = [(130, 8, [3], 50),                  # one level
         (64, 20, [5, 7, 4], 51),            # unequal sizes, E not a multiple of 4
         (33, H.RH_RQ_MAX_E, [H.RH_RQ_MAX_CODES] * 2, 52),  # both upper limits
         (512, 32, [256, 256, 256], 53),     # the example's shape
         (257, 64, [16] * H.RH_RQ_MAX_L, 54),  # the most levels
         (70, 1, [4, 4], 55)]                # E = 1


def dev():
    return torch.device("cuda:0")


def _close(got, want, rows, what, atol_frac=1e-5):
    got, want = got.detach().cpu().numpy()[rows], np.asarray(want)[rows]
    assert np.isfinite(got).all(), what
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=atol_frac * float(np.abs(want).max()), err_msg=what)


_ORACLE = {}


def case(N, E, sizes, seed):
    """Inputs, the float64 forward and the kept rows of one case, computed once and shared (read-only) by the tests."""
    key = (N, E, tuple(sizes), seed)
    if key not in _ORACLE:
        x, cbs = draw_inputs(N, E, sizes, seed)
        x_q, loss, idx, c = np_rq_forward(x.numpy(), [t.numpy() for t in cbs], BETA)
        keep = c["gap"] >= MIN_GAP
        assert (~keep).sum() <= MAX_EXCLUDED * N, f"{(~keep).sum()} of {N} rows have a gap below {MIN_GAP}"
        g = torch.Generator().manual_seed(seed + 1000)
        g_xq = torch.randn(N, E, generator=g) * torch.from_numpy(keep)[:, None]
        _ORACLE[key] = dict(x=x, cbs=cbs, x_q=x_q, idx=idx, keep=keep, g_xq=g_xq)
    return _ORACLE[key]


def run(c):
    from torch_rechub_amd import ops
    x = c["x"].to(dev()).requires_grad_(True)
    cbs = [t.to(dev()).requires_grad_(True) for t in c["cbs"]]
    x_q, loss, idx = ops.residual_quantize(x, cbs, BETA)
    torch.autograd.backward([x_q, loss], [c["g_xq"].to(dev()), torch.tensor(G_LOSS, device=dev())])
    return x, cbs, x_q, loss, idx


@pytest.mark.parametrize("N,E,sizes,seed", CASES)
def test_quantizer_kernels_against_float64(N, E, sizes, seed):
    from torch_rechub_amd import ops
    c = case(N, E, sizes, seed)
    keep, L = c["keep"], len(sizes)
    print(f"excluded rows: {int((~keep).sum())} of {N}")
    x, cbs, x_q, loss, idx = run(c)
    assert idx.dtype == torch.int64 and idx.shape == (N, L) and not idx.requires_grad
    got_idx = idx.cpu().numpy()
    np.testing.assert_array_equal(got_idx[keep], c["idx"][keep])
    assert (got_idx >= 0).all() and (got_idx < np.array(sizes)[None, :]).all()
    # the oracle over ALL rows, with the kernel's choice at the excluded ones
    cb64 = [t.numpy() for t in c["cbs"]]
    given = None if keep.all() else {l: got_idx[:, l] for l in range(L)}
    want_xq, want_loss, want_idx, cache = np_rq_forward(c["x"].numpy(), cb64, BETA, given=given)
    assert cache["slack"].max() < MIN_GAP  # where the kernel chose another code, that code is as near to within the margin
    _close(x_q, want_xq, keep, "x_q")
    _, _, _, sse = ops.rq_forward(c["x"].to(dev()), [t.to(dev()) for t in c["cbs"]])
    _close(sse * ((1.0 + BETA) / (N * E)), cache["level_loss"], slice(None), "per-level loss")
    _close(loss.reshape(1), np.array([want_loss]), slice(None), "loss")
    g_x, g_C = np_rq_backward(c["x"].numpy(), cb64, want_idx, c["g_xq"].numpy(), G_LOSS, BETA)
    _close(x.grad, g_x, keep, "g_x")
    for l in range(L):
        _close(cbs[l].grad, g_C[l], slice(None), f"g_C{l}", atol_frac=1e-4)
        unused = np.setdiff1d(np.arange(sizes[l]), got_idx[:, l])
        assert not cbs[l].grad[torch.from_numpy(unused).to(dev())].any(), f"level {l}: a code nobody chose has a gradient"
    x2, cbs2, x_q2, loss2, idx2 = run(c)
    assert torch.equal(idx, idx2) and torch.equal(x_q, x_q2) and torch.equal(loss, loss2) and torch.equal(x.grad, x2.grad)
    for a, b in zip(cbs, cbs2):
        assert torch.equal(a.grad, b.grad)


def test_identical_codes_pick_the_lower_index():
    from torch_rechub_amd import ops
    x, (C,) = draw_inputs(200, 12, [70], 60)
    C[41] = C[5]           # a tie between two lanes ...
    C[69] = C[5]           # ... and between a lane's own two codes
    C[66] = C[64]          # two lanes' second codes
    x[:50] = C[5] + 0.01 * x[:50]
    x[50:100] = C[64] + 0.01 * x[50:100]
    _, _, idx = ops.residual_quantize(x.to(dev()), [C.to(dev())], BETA)
    idx = idx.cpu().numpy()[:, 0]
    assert (idx[:50] == 5).all() and (idx[50:100] == 64).all() and not np.isin(idx, [41, 69, 66]).any()


def test_all_zero_codebook_gives_index_zero():
    from torch_rechub_amd import ops
    x, _ = draw_inputs(100, 16, [1], 61)
    cbs = [torch.zeros(300, 16, device=dev()), torch.zeros(7, 16, device=dev())]
    x_q, loss, idx = ops.residual_quantize(x.to(dev()), cbs, BETA)
    assert not idx.any() and not x_q.any()
    np.testing.assert_allclose(loss.item(), (1 + BETA) * float((x.double()**2).mean()), rtol=1e-5)


def test_level_range_split_with_a_given_index_is_bit_equal():
    from torch_rechub_amd import ops
    c = case(*CASES[1])
    x, cbs = c["x"].to(dev()), [t.to(dev()) for t in c["cbs"]]
    idx, r, x_q, sse = ops.rq_forward(x, cbs)
    idx_a, r_a, x_q_a, sse_a = ops.rq_forward(x, cbs, 0, 2)
    assert torch.equal(idx_a[:, :2], idx[:, :2]) and torch.equal(x_q_a, x - r_a)
    idx_a[:, 2] = idx[:, 2]
    idx_b, r_b, x_q_b, sse_b = ops.rq_forward(r_a, cbs, 2, 3, given=1 << 2, idx=idx_a, sse=sse_a)
    assert torch.equal(idx_b, idx) and torch.equal(r_b, r) and torch.equal(sse_b, sse)
    assert torch.equal(x - r_b, x_q) and torch.equal(x_q_b, r_a - r_b)
    # ... and searched instead of given: the same again
    idx_c, r_c, _, sse_c = ops.rq_forward(r_a, cbs, 2, 3, idx=idx_a.clone().fill_(-1), sse=sse_a.clone())
    assert torch.equal(idx_c[:, 2], idx[:, 2]) and torch.equal(r_c, r) and torch.equal(sse_c, sse)


def test_leading_dimensions_and_single_level_module():
    from torch_rechub_amd import ops
    from torch_rechub_amd.models.generative.rqvae import VectorQuantizer
    x, (C,) = draw_inputs(24, 8, [9], 62)
    flat = ops.residual_quantize(x.to(dev()), [C.to(dev())], BETA)
    x_q, loss, idx = ops.residual_quantize(x.view(2, 3, 4, 8).to(dev()), [C.to(dev())], BETA)
    assert x_q.shape == (2, 3, 4, 8) and idx.shape == (2, 3, 4, 1) and loss.dim() == 0
    assert torch.equal(x_q.reshape(24, 8), flat[0]) and torch.equal(idx.reshape(24, 1), flat[2]) and torch.equal(loss, flat[1])
    vq = VectorQuantizer(9, 8, beta=BETA, sk_epsilon=0.0).to(dev())
    with torch.no_grad():
        vq.embedding.weight.copy_(C)
    v_q, v_loss, v_idx = vq(x.view(6, 4, 8).to(dev()))
    assert v_idx.shape == (6, 4) and torch.equal(v_idx.reshape(24), flat[2][:, 0]) and torch.equal(v_loss, flat[1])
    empty = ops.residual_quantize(torch.zeros(0, 8, device=dev()), [C.to(dev())], BETA)
    assert empty[0].shape == (0, 8) and empty[2].shape == (0, 1)


@pytest.mark.parametrize("E,sizes", [(129, [4]), (8, [1025]), (8, [4] * 9)])
def test_unsupported_shapes_raise(E, sizes):
    from torch_rechub_amd import ops
    assert not ops.rq_supported(E, sizes)
    x = torch.zeros(4, E, device=dev())
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.residual_quantize(x, [torch.zeros(n, E, device=dev()) for n in sizes], BETA)
    assert ops.rq_supported(128, [1024] * 8) and ops.rq_supported(1, [1])
