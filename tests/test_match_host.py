"""Host-side pin of tests/match_oracle.py (no GPU): the float64 numpy restatement of the in-batch logits, the L2
normalisation and the mean cross-entropy equals torch's float64 autograd of the reference's own formulation --
gather_inbatch_logits over the score matrix, F.normalize, nn.CrossEntropyLoss() -- duplicate negatives and clamped rows
included.  Both sides are float64: they agree to a few ulps, so the bound is 1e-12 of the tensor's largest magnitude, row by
row where a clamped row's gradient is 1e12 times the others."""
import numpy as np
import pytest
import torch

import match_oracle as O


def close(got, want, what="", rows=False):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if rows:
        for r in range(want.shape[0]):
            close(got[r], want[r], f"{what} row {r}")
        return
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12 * float(np.abs(want).max()) if want.size else 0.0, err_msg=what)


@pytest.mark.parametrize("B,C,D,K,row0", [(1, 1, 3, 0, 0), (4, 4, 5, 3, 0), (6, 11, 7, 4, 5), (5, 5, 1, 6, 0)])
def test_oracle_inbatch_logits_match_float64_autograd_duplicates_included(B, C, D, K, row0):
    from torch_rechub_amd.utils.match import gather_inbatch_logits
    g = torch.Generator().manual_seed(B * 100 + C)
    u = torch.randn(B, D, generator=g, dtype=torch.float64).requires_grad_()
    v = torch.randn(C, D, generator=g, dtype=torch.float64).requires_grad_()
    neg = torch.randint(0, C, (B, K), generator=g)
    if K >= 3:
        neg[0] = neg[0, 0]         # one row names one item K times
        neg[1] = row0 + 1          # one row names its own positive K times
        neg[2, 0], neg[2, 1] = 0, C - 1
    gl = torch.randn(B, 1 + K, generator=g, dtype=torch.float64)
    ref = gather_inbatch_logits(u @ v.T, neg, row_offset=row0)
    ref.backward(gl)
    close(O.inbatch_forward(u.detach().numpy(), v.detach().numpy(), neg.numpy(), row0), ref.detach().numpy(), "logits")
    g_u, g_v = O.inbatch_backward(u.detach().numpy(), v.detach().numpy(), neg.numpy(), gl.numpy(), row0)
    close(g_u, u.grad.numpy(), "g_u")
    close(g_v, v.grad.numpy(), "g_v")
    hits = O.inbatch_index(neg.numpy(), B, row0)
    assert not g_v[np.setdiff1d(np.arange(C), hits.reshape(-1))].any()  # item rows nobody names: exact zeros


@pytest.mark.parametrize("B,d", [(1, 4), (5, 8), (7, 68), (3, 12)])
def test_oracle_l2_normalize_matches_float64_autograd_clamped_rows_included(B, d):
    g = torch.Generator().manual_seed(B + d)
    x = torch.randn(B, d, generator=g, dtype=torch.float64)
    if B >= 5:
        x[1] = 0.0
        x[2] *= 5e-13 / x[2].norm()   # below eps: clamped
        x[3] *= 2e-12 / x[3].norm()   # just above eps
        x[4] *= 1e15
    x.requires_grad_()
    gy = torch.randn(B, d, generator=g, dtype=torch.float64)
    y = torch.nn.functional.normalize(x, p=2, dim=1)
    y.backward(gy)
    close(O.l2norm_forward(x.detach().numpy()), y.detach().numpy(), "y", rows=True)
    gx = O.l2norm_backward(x.detach().numpy(), gy.numpy())
    close(gx, x.grad.numpy(), "g_x", rows=True)
    if B >= 5:  # the clamped rows' gradient is g / eps
        close(gx[1], gy[1].numpy() / 1e-12, "zero row")
        close(gx[2], gy[2].numpy() / 1e-12, "sub-eps row")
        assert np.abs(gx[3] - gy[3].numpy() / 1e-12).max() > 1e9  # not clamped: the projection is taken out


@pytest.mark.parametrize("B,C,with_target", [(1, 1, False), (5, 2, True), (9, 65, True), (4, 7, False)])
def test_oracle_cross_entropy_matches_float64_autograd(B, C, with_target):
    g = torch.Generator().manual_seed(B * 7 + C)
    x = (20 * torch.randn(B, C, generator=g, dtype=torch.float64)).requires_grad_()
    target = torch.randint(0, C, (B,), generator=g) if with_target else None
    if with_target:
        target[0], target[-1] = 0, C - 1
    loss = torch.nn.CrossEntropyLoss()(x, target if with_target else torch.zeros(B, dtype=torch.long))
    (1.7 * loss).backward()
    t = None if target is None else target.numpy()
    assert abs(O.ce_forward(x.detach().numpy(), t) - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
    close(O.ce_backward(x.detach().numpy(), t, 1.7), x.grad.numpy(), "g_logits")


def test_oracle_cross_entropy_special_rows_are_exact():
    """All entries equal: the term is log C and the gradient (1/C - onehot)/B.  One entry at +1e4 over a floor of -1e4: the
    term is exactly 0 with the target on the large entry and exactly 2e4 elsewhere."""
    C = 6
    x = np.full((3, C), 3.25)
    x[1:] = -1e4
    x[1, 2] = x[2, 2] = 1e4
    t = np.array([4, 2, 0])
    terms = O.ce_terms(x, t)
    assert abs(terms[0] - np.log(C)) <= 1e-15 and terms[1] == 0.0 and terms[2] == 2e4
    g = O.ce_backward(x, t)
    onehot = np.eye(C)[t]
    close(g[0], (1.0 / C - onehot[0]) / 3, "equal row")
    assert np.array_equal(g[1], np.zeros(C)) and np.array_equal(g[2] * 3, np.eye(C)[2] - onehot[2])
