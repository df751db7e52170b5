"""AutoInt's interacting layer without a GPU: the argument checks of rh_interact_* through the C ABI (pointers never
dereferenced), the tile plan, and the torch formulation the layer keeps for CPU tensors against the float64 formula."""
import ctypes

import pytest
import torch

FAKE = ctypes.c_void_p(4096)  # never dereferenced: validation fails, or B = 0 returns, first


def float64_pre(x, w_q, w_k, w_v, w_res, H):
    """The layer's pre-activation in float64: softmax(Q_h K_h^T / sqrt(dh)) V_h per head, concatenated, plus x W_Res^T."""
    x, w_q, w_k, w_v = (t.double() for t in (x, w_q, w_k, w_v))
    B, F, D = x.shape
    q, k, v = ((x @ w.t()).view(B, F, H, D // H).transpose(1, 2) for w in (w_q, w_k, w_v))
    p = torch.softmax(q @ k.transpose(-2, -1) * (D // H) ** -0.5, dim=-1)
    out = (p @ v).transpose(1, 2).reshape(B, F, D)
    return out if w_res is None else out + x @ w_res.double().t()


def entry_points(B, F, D, H):
    from torch_rechub_amd import _lib
    nt, nb = ctypes.c_int(-1), ctypes.c_int(-1)
    _lib.call("rh_interact_plan", B, F, D, H, ctypes.c_void_p(ctypes.addressof(nt)), ctypes.c_void_p(ctypes.addressof(nb)))
    _lib.call("rh_interact_fwd", FAKE, FAKE, FAKE, FAKE, FAKE, 1.0, B, F, D, H, FAKE, FAKE, None)
    _lib.call("rh_interact_bwd", FAKE, FAKE, FAKE, FAKE, FAKE, 1.0, FAKE, FAKE, FAKE, B, F, D, H, FAKE, FAKE, None)
    return nt.value, nb.value


@pytest.mark.parametrize("F, D, H, rc", [(65, 16, 2, -2), (39, 65, 5, -2), (0, 16, 2, -2), (39, 16, 0, -2), (39, 16, 3, -1)])
def test_one_past_each_limit_is_refused(F, D, H, rc):
    from torch_rechub_amd import _lib
    assert (_lib.H.RH_E_BADARG, _lib.H.RH_E_UNSUPPORTED, _lib.H.RH_CIN_MAX_F, _lib.H.RH_SA_MAX_D) == (-1, -2, 64, 64)
    lib = _lib.load()
    out = ctypes.c_int(0)
    po = ctypes.c_void_p(ctypes.addressof(out))
    assert lib.rh_interact_plan(4, F, D, H, po, po) == rc
    assert lib.rh_interact_fwd(FAKE, FAKE, FAKE, FAKE, FAKE, 1.0, 4, F, D, H, FAKE, FAKE, None) == rc
    assert lib.rh_interact_bwd(FAKE, FAKE, FAKE, FAKE, FAKE, 1.0, FAKE, FAKE, FAKE, 4, F, D, H, FAKE, FAKE, None) == rc


def test_empty_batch_returns_at_once():
    assert entry_points(0, 39, 16, 2) == (0, 0)
    assert entry_points(0, 64, 64, 1) == (0, 0)


@pytest.mark.parametrize("B, F", [(1, 1), (64, 1), (65, 1), (7, 21), (6, 22), (4096, 39), (5, 64), (100, 32)])
def test_plan_counts_the_tiles(B, F):
    from torch_rechub_amd import _lib
    G = 64 // F
    ntiles, nblocks = _lib.query("rh_interact_plan", B, F, 16, 2, out=(ctypes.c_int, ctypes.c_int))
    assert ntiles == -(-B // G) and 1 <= nblocks <= ntiles


@pytest.mark.parametrize("residual", [True, False])
def test_cpu_layer_equals_the_float64_formula(residual):
    from torch_rechub_amd.basic.layers import InteractingLayer
    torch.manual_seed(3)
    layer = InteractingLayer(12, num_heads=3, residual=residual)
    x = torch.randn(5, 7, 12)
    want = torch.relu(float64_pre(x, layer.W_Q.weight, layer.W_K.weight, layer.W_V.weight,
                                  layer.W_Res.weight if residual else None, 3))
    torch.testing.assert_close(layer(x).double(), want.detach(), rtol=1e-5, atol=1e-6)
