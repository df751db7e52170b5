"""AutoInt's interacting layer on the MI355X: the kernels of csrc/interact.hip against the layer's formula in float64 on the
CPU (test_interact_host.float64_pre, gradients from autograd).

Bounds: the kernel convention of test_gpu_cin.py -- rtol 1e-4, atol 1e-5 of the tensor's largest magnitude, 1e-4 of it for
the weight gradients.  The ReLU edge: the upstream gradient is zeroed where the float64 pre-activation lies within 1e-6 of
the tensor's largest magnitude of zero, and those are at most 0.1 % of the elements."""
import ctypes

import numpy as np
import pytest
import torch

from test_interact_host import float64_pre

pytestmark = pytest.mark.gpu

NAMES = ("y", "g_x", "g_wq", "g_wk", "g_wv", "g_wres")
DEV = "cuda:0"


def make_case(B, F, D, H, residual, seed, score_peak=None):
    """float32 CPU inputs (x, four weights, g_y with the ReLU edge zeroed) and the float64 results by name."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, F, D, generator=g)
    ws = [torch.randn(D, D, generator=g) / D ** 0.5 for _ in range(4)]
    if not residual:
        ws[3] = None
    gy = torch.randn(B, F, D, generator=g)
    if score_peak is not None:  # the scores are quadratic in x
        q, k = ((x.double() @ w.double().t()).view(B, F, H, D // H).transpose(1, 2) for w in ws[:2])
        x = x * float(score_peak / ((q @ k.transpose(-2, -1)).abs().max() * (D // H) ** -0.5)) ** 0.5
    leaves = [t.double().requires_grad_(True) if t is not None else None for t in [x] + ws]
    pre = float64_pre(*leaves, H)
    if pre.numel():
        edge = pre.detach().abs() <= 1e-6 * pre.detach().abs().max()
        assert edge.double().mean() <= 1e-3, f"{float(edge.double().mean()):.2e} of the pre-activations sit on the ReLU edge"
        gy[edge] = 0.0
    torch.relu(pre).backward(gy.double())
    want = {"y": torch.relu(pre).detach()}
    want.update({n: (t.grad if t is not None else None) for n, t in zip(NAMES[1:], leaves)})
    return (x, ws, gy), want


def run_kernel(inputs, H):
    from torch_rechub_amd import ops
    x, ws, gy = inputs
    leaves = [t.to(DEV).requires_grad_(True) if t is not None else None for t in [x] + ws]
    y = ops.interacting_layer(*leaves, H)
    y.backward(gy.to(DEV))
    torch.cuda.synchronize()
    ops.check_errors()
    got = {"y": y.detach()}
    got.update({n: (t.grad if t is not None else None) for n, t in zip(NAMES[1:], leaves)})
    return got


def check(got, want):
    for n in NAMES:
        if want[n] is None:
            assert got[n] is None, n
            continue
        w = want[n].numpy()
        assert torch.isfinite(got[n]).all(), n
        frac = 1e-4 if n.startswith("g_w") else 1e-5
        np.testing.assert_allclose(got[n].cpu().numpy(), w, rtol=1e-4, atol=frac * float(np.abs(w).max()) if w.size else 0,
                                   err_msg=n)


# (F, D, H, residual): G = 64, 32, 3, 2, 2, 1, 1 samples per tile -- a tile exactly full, one row short, single-sample;
# dh = 1, 3 (odd), 8, 1, 16, 64, 3
SHAPES = [(1, 1, 1, True), (2, 6, 2, False), (21, 16, 2, True), (22, 16, 16, False), (32, 64, 4, False), (33, 64, 1, True),
          (64, 6, 2, True)]
CASES = [(B, *s) for s in SHAPES for B in sorted({1, 64 // s[0] - 1, 64 // s[0] + 1, 2 * (64 // s[0])} - {0})]


@pytest.mark.parametrize("B, F, D, H, residual", CASES)
def test_layer_against_float64(B, F, D, H, residual):
    inputs, want = make_case(B, F, D, H, residual, seed=1000 * F + 10 * D + B)
    check(run_kernel(inputs, H), want)


def test_second_and_third_trip_of_the_grid():
    """ntiles = 2 nblocks + 1 at F = 64: workgroup 0 takes three tiles, the others two; every row of `part` sums several."""
    from torch_rechub_amd import _lib
    _, cap = _lib.query("rh_interact_plan", 1 << 20, 64, 4, 2, out=(ctypes.c_int, ctypes.c_int))
    B = 2 * cap + 1
    assert _lib.query("rh_interact_plan", B, 64, 4, 2, out=(ctypes.c_int, ctypes.c_int)) == (B, cap)
    inputs, want = make_case(B, 64, 4, 2, True, seed=5)
    check(run_kernel(inputs, 2), want)


def test_saturated_softmax():
    """Scores up to +-1e3: the softmax rows are one-hot to rounding; everything stays finite and inside the bounds."""
    inputs, want = make_case(5, 21, 16, 2, True, seed=6, score_peak=1e3)
    check(run_kernel(inputs, 2), want)


def test_empty_batch():
    inputs, _ = make_case(0, 21, 16, 2, True, seed=7)
    got = run_kernel(inputs, 2)
    assert got["y"].shape == (0, 21, 16) and got["g_x"].shape == (0, 21, 16)
    assert all(got[n].shape == (16, 16) and not got[n].any() for n in NAMES[2:])


def test_gradients_bit_identical_over_two_runs():
    inputs, _ = make_case(1100, 39, 16, 2, True, seed=8)  # 1100 tiles: a third trip for some workgroups
    a, b = run_kernel(inputs, 2), run_kernel(inputs, 2)
    for n in NAMES:
        assert torch.equal(a[n], b[n]), n


def test_peak_memory_stays_below_one_score_tensor():
    """(4096, 64, 16, 2): y, lse, g_x and the workspace stay below one (B, H, F, F) float32 tensor (128 MiB)."""
    from torch_rechub_amd import ops
    B, F, D, H = 4096, 64, 16, 2
    g = torch.Generator().manual_seed(9)
    leaves = [torch.randn(B, F, D, generator=g).to(DEV).requires_grad_(True)]
    leaves += [(torch.randn(D, D, generator=g) / 4).to(DEV).requires_grad_(True) for _ in range(4)]
    gy = torch.randn(B, F, D, generator=g).to(DEV)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    ops.interacting_layer(*leaves, H).backward(gy)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base < B * H * F * F * 4


def test_layer_takes_the_kernel_unless_dropout_is_active(monkeypatch):
    from torch_rechub_amd import ops
    from torch_rechub_amd.basic.layers import InteractingLayer
    calls = []
    real = ops.interacting_layer
    monkeypatch.setattr(ops, "interacting_layer", lambda *a: calls.append(1) or real(*a))
    torch.manual_seed(10)
    x = torch.randn(9, 7, 16, device=DEV)
    plain = InteractingLayer(16, 2).to(DEV)
    torch.testing.assert_close(plain(x), plain.forward_torch(x), rtol=1e-4, atol=1e-5)
    assert len(calls) == 1
    drop = InteractingLayer(16, 2, dropout=0.2).to(DEV)
    drop(x)
    assert len(calls) == 1
    drop.eval()
    drop(x)
    assert len(calls) == 2
