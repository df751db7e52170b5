"""FiBiNET's bilinear interaction on the MI355X: the kernels of csrc/bilinear.hip against the layer's formula in float64 on
the CPU (test_bilinear_host.float64_bilinear, gradients from autograd).

Bounds: the kernel convention of test_gpu_cin.py -- rtol 1e-4, atol 1e-5 of the tensor's largest magnitude, 1e-4 of it for
the weight gradients."""
import ctypes

import numpy as np
import pytest
import torch

from test_bilinear_host import KINDS, float64_bilinear

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAMES = ("out", "g_x", "g_w", "g_gate")
PLAN = (ctypes.c_int,) * 5 + (ctypes.c_int64,) * 2


def make_case(B, F, D, kind, gated, seed):
    """float32 CPU inputs (x, w, gate, g_out) and the float64 results by name."""
    g = torch.Generator().manual_seed(seed)
    P = F * (F - 1) // 2
    x = torch.randn(B, F, D, generator=g)
    w = torch.randn((1, F, P)[KINDS.index(kind)], D, D, generator=g) / D ** 0.5
    gate = torch.relu(torch.randn(B, F, generator=g)) if gated else None  # exact zeros, as SENET's ReLU gives
    if gated and B > 2:
        gate[2] = 0.0
    gy = torch.randn(B, 2 * P if gated else P, D, generator=g)
    leaves = [t.double().requires_grad_(True) if t is not None else None for t in (x, w, gate)]
    out = float64_bilinear(*leaves[:2], kind, leaves[2])
    out.backward(gy.double())
    want = {"out": out.detach()}
    want.update({n: (t.grad if t is not None else None) for n, t in zip(NAMES[1:], leaves)})
    return (x, w, gate, gy), want


def run_kernel(inputs, kind, needs=(True, True, True), wide=0):
    from torch_rechub_amd import ops
    x, w, gate, gy = inputs
    if wide:  # x as a strided view of a wider buffer
        x = torch.cat([x.flatten(1), torch.full((x.shape[0], wide), float("nan"))], 1).to(DEV)[:, :-wide].view(x.shape)
    leaves = [t.to(DEV).requires_grad_(n) if t is not None else None for t, n in zip((x, w, gate), needs)]
    out = ops.bilinear_interaction(leaves[0], leaves[1], kind, leaves[2])
    if any(n and t is not None for t, n in zip(leaves, needs)):
        out.backward(gy.to(DEV))
    torch.cuda.synchronize()
    ops.check_errors()
    got = {"out": out.detach()}
    got.update({n: (t.grad if t is not None else None) for n, t in zip(NAMES[1:], leaves)})
    return got


def check(got, want, names=NAMES):
    for n in names:
        if want[n] is None:
            assert got[n] is None, n
            continue
        w = want[n].numpy()
        assert got[n].shape == want[n].shape and torch.isfinite(got[n]).all(), n
        frac = 1e-4 if n == "g_w" else 1e-5
        np.testing.assert_allclose(got[n].cpu().numpy(), w, rtol=1e-4, atol=frac * float(np.abs(w).max()) if w.size else 0,
                                   err_msg=n)


# one pair with K = 1; odd K; pair blocks that straddle the 32-column blocks; 13 column blocks over four wavefronts;
# F D = 1024 at each cap; 1020
SHAPES = [(2, 1), (3, 3), (5, 16), (26, 16), (64, 16), (16, 64), (17, 60)]


@pytest.mark.parametrize("gated", [False, True])
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("F, D", SHAPES)
def test_layer_against_float64(F, D, kind, gated):
    """B = 70: three forward tiles and two backward tiles, the last of each ragged."""
    inputs, want = make_case(70, F, D, kind, gated, seed=100 * F + D)
    check(run_kernel(inputs, kind), want)


@pytest.mark.parametrize("B", [1, 31, 33])
@pytest.mark.parametrize("kind", KINDS)
def test_ragged_row_tiles_and_a_strided_x(B, kind):
    inputs, want = make_case(B, 5, 16, kind, True, seed=B)
    check(run_kernel(inputs, kind, wide=B % 7 + 1), want)


@pytest.mark.parametrize("kind", KINDS)
def test_second_trips_come_from_the_plan(kind):
    """B = 32 * the forward grid cap + 33 at (3, 3): the forward's first workgroups take a second unit, and every
    weight-gradient split walks three 64-row tiles, the last tile of the last split ragged."""
    from torch_rechub_amd import _lib
    k = KINDS.index(kind)
    cap = _lib.query("rh_bilinear_plan", 1 << 24, 3, 3, k, out=PLAN)[1]
    B = 32 * cap + 33
    units, grid, slices, splits, tiles, bwd_floats, wgrad_floats = _lib.query("rh_bilinear_plan", B, 3, 3, k, out=PLAN)
    assert (units, grid, slices) == (cap + 2, cap, 1) and bwd_floats == B * 12
    nt = -(-B // 64)
    assert tiles == 3 and splits == -(-nt // 3) and B % 64 == 33 and wgrad_floats == splits * (1, 3, 3)[k] * 9
    inputs, want = make_case(B, 3, 3, kind, True, seed=11)
    check(run_kernel(inputs, kind), want)


@pytest.mark.parametrize("needs", [(True, False, False), (False, True, False), (False, False, True), (False, False, False)])
def test_needs_input_grad_subsets(needs):
    inputs, want = make_case(40, 5, 16, "field_each", True, seed=12)
    got = run_kernel(inputs, "field_each", needs)
    check(got, want, ["out"] + [n for n, need in zip(NAMES[1:], needs) if need])
    assert all(got[n] is None for n, need in zip(NAMES[1:], needs) if not need)


def test_empty_batch():
    inputs, _ = make_case(0, 5, 16, "field_each", True, seed=13)
    got = run_kernel(inputs, "field_each")
    assert got["out"].shape == (0, 20, 16) and got["g_x"].shape == (0, 5, 16) and got["g_gate"].shape == (0, 5)
    assert got["g_w"].shape == (5, 16, 16) and not got["g_w"].any()


@pytest.mark.parametrize("F, D", [(17, 64), (1, 16)])
def test_outside_the_limits_is_refused(F, D):
    from torch_rechub_amd import _lib, ops
    x, w = torch.zeros(4, F, D, device=DEV), torch.zeros(1, D, D, device=DEV)
    assert not ops.bilinear_interaction_ok(x, w, "field_all")
    fake = ctypes.c_void_p(4096)  # never dereferenced: validation fails first
    lib = _lib.load()
    assert lib.rh_bilinear_fwd(fake, F * D, fake, None, 4, F, D, 0, fake, None) == _lib.H.RH_E_UNSUPPORTED
    assert lib.rh_bilinear_bwd(fake, F * D, fake, None, fake, 4, F, D, 0, fake, None, fake, None) == _lib.H.RH_E_UNSUPPORTED
    assert lib.rh_bilinear_wgrad(fake, F * D, None, fake, 4, F, D, 0, fake, None) == _lib.H.RH_E_UNSUPPORTED


def test_gradients_bit_identical_over_two_runs():
    inputs, _ = make_case(300, 26, 16, "field_interaction", True, seed=14)
    a, b = run_kernel(inputs, "field_interaction"), run_kernel(inputs, "field_interaction")
    for n in NAMES:
        assert torch.equal(a[n], b[n]), n


def test_memory_is_the_output_and_the_declared_workspace():
    """(2048, 26, 16) with a gate: the forward allocates the output (+ 1 MiB), where the torch formulation needs about five
    times that; the backward g_x, g_gate, g_w, the plan's two workspaces and a contiguous g_out at most."""
    from torch_rechub_amd import _lib, ops
    B, F, D, P = 2048, 26, 16, 325
    g = torch.Generator().manual_seed(15)
    x, w, gate = (t.to(DEV).requires_grad_(True) for t in (torch.randn(B, F, D, generator=g), torch.randn(P, D, D, generator=g),
                                                            torch.rand(B, F, generator=g)))
    gy = torch.randn(B, 2 * P, D, generator=g).to(DEV)
    plan = _lib.query("rh_bilinear_plan", B, F, D, 2, out=PLAN)
    out_bytes = B * 2 * P * D * 4
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = ops.bilinear_interaction(x, w, "field_interaction", gate)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() - base <= out_bytes + (1 << 20)
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out.backward(gy)
    torch.cuda.synchronize()
    grads = 4 * (x.numel() + gate.numel() + w.numel() + plan[5] + plan[6])
    assert torch.cuda.max_memory_allocated() - base <= grads + (1 << 20)


@pytest.mark.parametrize("kind", KINDS)
def test_fibinet_fused_equals_its_torch_formulation(kind, monkeypatch):
    from torch_rechub_amd import ops
    from torch_rechub_amd.basic.features import SparseFeature
    from torch_rechub_amd.models.ranking import FiBiNet
    torch.manual_seed(16)
    feats = [SparseFeature(f"C{i}", 11 + i, 8) for i in range(5)]
    model = FiBiNet(feats, {"dims": [16], "dropout": 0.0, "activation": "relu"}, bilinear_type=kind).to(DEV)
    npair = {"field_all": 0, "field_each": 5, "field_interaction": 10}[kind]
    keys = ["bilinear_interaction.bilinear_layer" + (f".{k}" if npair else "") + ".weight" for k in range(max(npair, 1))]
    assert [k for k in model.state_dict() if k.startswith("bilinear")] == keys
    assert [k for k in model.state_dict() if k.startswith("senet")] == ["senet_layer.mlp.0.weight", "senet_layer.mlp.2.weight"]
    x = {f.name: torch.randint(0, f.vocab_size, (48,), device=DEV) for f in feats}
    results = []
    for fused in (True, False):
        if not fused:
            monkeypatch.setattr(ops, "bilinear_interaction_ok", lambda *a: False)
        model.zero_grad()
        y = model(x)
        y.sum().backward()
        results.append([y.detach()] + [p.grad.clone() for p in model.parameters()])
    for n, (got, want) in enumerate(zip(*results)):  # y, then the parameters: weight gradients all
        torch.testing.assert_close(got, want, rtol=1e-4, atol=(1e-4 if n else 1e-5) * float(want.abs().max()))
