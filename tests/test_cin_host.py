"""CIN / xDeepFM without a GPU: the float64 numpy oracle (tests/cin_oracle.py) against the reference's fixtures
(tools/gen_golden_cin.py), the reference's state_dict layout and parameter-initialisation order, the constructor errors,
the torch fallback of the layer, the integration patch and the argument validation of csrc/cin.hip."""
import ctypes
import json

import numpy as np
import pytest
import torch

import cin_oracle as O
from conftest import features_from_spec, load_golden
from oracle.ref_import import available, import_reference

CIN_CASES = ["split", "full"]
XDEEPFM_MODELS = {"xdeepfm": ([8, 6], True), "xdeepfm_criteo": ([6, 6], False)}
MLP = {"dims": [32, 16], "dropout": 0.0, "activation": "relu"}


def cin_case(gold, tag):
    """(x, state_dict, cin_size, split_half) of one configuration of cin_layers.npz (float64 arrays)."""
    sd = {k[len(tag) + 4:]: gold[k] for k in gold.files if k.startswith(tag + ".sd.")}
    return gold[tag + ".x"], sd, [int(c) for c in gold[tag + ".cin_size"]], bool(gold[tag + ".split_half"])


def build_xdeepfm_model(cfg, gold):
    from torch_rechub_amd.models.ranking import xDeepFM
    groups = features_from_spec(gold["spec"])
    cin_size, split_half = XDEEPFM_MODELS[cfg]
    return xDeepFM(groups["deep_features"], groups["fm_features"], dict(MLP), cin_size, split_half)


def test_public_names_import():
    from torch_rechub_amd.basic.layers import CIN  # noqa: F401
    from torch_rechub_amd.models.ranking import xDeepFM  # noqa: F401
    import torch_rechub_amd.models.ranking as R
    from torch_rechub_amd import integration, ops
    assert "xDeepFM" in R.__all__ and "CIN" in integration._LAYERS and callable(ops.cin_layer)


# ---- the oracle against the reference ---------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CIN_CASES)
def test_oracle_reproduces_the_reference_layer_fixture(tag):
    gold = load_golden("cin_layers.npz")
    x, sd, cin_size, split_half = cin_case(gold, tag)
    assert x.dtype == np.float64 and gold[tag + ".out"].dtype == np.float64
    out = O.cin_fwd(x, sd, split_half)
    np.testing.assert_allclose(out, gold[tag + ".out"], rtol=1e-12, atol=1e-13)
    g_x, grads = O.cin_bwd(x, sd, split_half, gold[tag + ".g_out"])
    np.testing.assert_allclose(g_x, gold[tag + ".g_x"], rtol=1e-11, atol=1e-13)
    names = [k[len(tag) + 6:] for k in gold.files if k.startswith(tag + ".grad.")]
    assert sorted(names) == sorted(grads) and len(names) == 2 * len(cin_size) + 2
    for n in names:
        want = gold[f"{tag}.grad.{n}"]
        np.testing.assert_allclose(grads[n].reshape(want.shape), want, rtol=1e-11, atol=1e-12, err_msg=n)


def test_fixture_keeps_its_relu_margin():
    """No pre-activation of the fixtures lies within 1e-6 of its layer's largest magnitude of zero."""
    gold = load_golden("cin_layers.npz")
    for tag in CIN_CASES:
        x, sd, _, split_half = cin_case(gold, tag)
        cache = []
        O.cin_fwd(x, sd, split_half, cache)
        for _, pre in cache[:-1]:
            assert np.abs(pre).min() > 1e-6 * np.abs(pre).max()


def test_oracle_layer_backward_matches_autograd():
    g = torch.Generator().manual_seed(5)
    B, F, Hp, Ho, D = 4, 3, 5, 6, 7
    x0 = torch.randn(B, F, D, generator=g, dtype=torch.float64, requires_grad=True)
    h = torch.randn(B, Hp, D, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(Ho, F * Hp, 1, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(Ho, generator=g, dtype=torch.float64, requires_grad=True)
    z = (x0.unsqueeze(2) * h.unsqueeze(1)).reshape(B, F * Hp, D)
    y = torch.relu(torch.nn.functional.conv1d(z, w, b))
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    np.testing.assert_allclose(O.layer_fwd(x0.detach().numpy(), h.detach().numpy(), w.detach().numpy(), b.detach().numpy()),
                               y.detach().numpy(), rtol=1e-13, atol=1e-14)
    got = O.layer_bwd(x0.detach().numpy(), h.detach().numpy(), w.detach().numpy(), b.detach().numpy(), gy.numpy())
    for a, t in zip(got, (x0, h, w, b)):
        np.testing.assert_allclose(a, t.grad.numpy(), rtol=1e-12, atol=1e-13)


# ---- the layer ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CIN_CASES)
def test_cin_state_dict_checkpoint_and_rng_order_match_reference(tag):
    from torch_rechub_amd.basic.layers import CIN
    gold = load_golden("cin_layers.npz")
    x, sd, cin_size, split_half = cin_case(gold, tag)
    torch.manual_seed(int(gold[tag + ".seed"]))
    cin = CIN(x.shape[1], cin_size, split_half)
    mine = cin.state_dict()
    assert list(mine.keys()) == list(sd.keys())
    assert cin.num_layers == len(cin_size) and cin.split_half is split_half
    for k, v in sd.items():
        assert tuple(mine[k].shape) == v.shape, k
        # the reference initialised in float32 and was then cast to float64: the same draws in the same order
        np.testing.assert_array_equal(mine[k].numpy().astype(np.float64), v, err_msg=k)
    fresh = CIN(x.shape[1], cin_size, split_half)
    fresh.load_state_dict({k: torch.from_numpy(v).float() for k, v in sd.items()}, strict=True)


@pytest.mark.parametrize("tag", CIN_CASES)
def test_cin_torch_fallback_on_cpu_matches_the_fixture(tag):
    """A non-HIP tensor runs the reference's formulation on torch ops, here in float64."""
    from torch_rechub_amd.basic.layers import CIN
    gold = load_golden("cin_layers.npz")
    x, sd, cin_size, split_half = cin_case(gold, tag)
    cin = CIN(x.shape[1], cin_size, split_half).double()
    cin.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    xt = torch.from_numpy(x).requires_grad_(True)
    y = cin(xt)
    np.testing.assert_allclose(y.detach().numpy(), gold[tag + ".out"], rtol=1e-12, atol=1e-13)
    y.backward(torch.from_numpy(gold[tag + ".g_out"]))
    np.testing.assert_allclose(xt.grad.numpy(), gold[tag + ".g_x"], rtol=1e-11, atol=1e-13)
    for n, p in cin.named_parameters():
        np.testing.assert_allclose(p.grad.numpy(), gold[f"{tag}.grad.{n}"], rtol=1e-11, atol=1e-12, err_msg=n)


def test_odd_split_size_is_refused_at_construction():
    from torch_rechub_amd.basic.layers import CIN
    with pytest.raises(ValueError, match="split_half.*even.*reference's forward fails"):
        CIN(5, [6, 5, 4], True)
    CIN(5, [6, 4, 5], True)   # the last layer is not split
    CIN(5, [5, 5], False)


# ---- the model ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", list(XDEEPFM_MODELS))
def test_xdeepfm_state_dict_checkpoint_and_rng_order_match_reference(cfg):
    gold = load_golden(f"model_{cfg}.npz")
    torch.manual_seed(2022)  # the seed of oracle/gen_golden.py::gen_model
    model = build_xdeepfm_model(cfg, gold)
    assert [n for n, _ in model.named_children()] == ["linear", "cin", "embedding", "mlp"]
    want = {k[4:]: gold[k] for k in gold.files if k.startswith("sd0.")}
    sd = model.state_dict()
    assert list(sd.keys()) == list(want.keys())
    for k, v in want.items():
        assert tuple(sd[k].shape) == v.shape, k
        assert sd[k].dtype == torch.from_numpy(v).dtype, k
        # built before the tables: the same draws from the global RNG as the reference's modules made (the fixture
        # re-initialises the tables from a generator of its own; a padded table draws its padding too, so what is built
        # after the tables is compared only where no table is padded)
        if k.startswith(("linear.", "cin.")) or (cfg == "xdeepfm" and k.startswith("mlp.")):
            np.testing.assert_array_equal(sd[k].numpy(), v, err_msg=k)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in want.items()}, strict=True)
    for k, v in want.items():
        np.testing.assert_array_equal(model.state_dict()[k].numpy(), v)
    if cfg == "xdeepfm_criteo":  # width 10 stored padded; the padding stays zero after the load
        w = model.embedding.embed_dict["C1"].weight
        assert w.shape[1] == 16 and torch.count_nonzero(w[:, 10:]) == 0
        spec = json.loads(str(gold["spec"]))
        assert [d["kind"] for d in spec["deep_features"]][:1] == ["DenseFeature"]


def test_xdeepfm_needs_one_embed_dim():
    from torch_rechub_amd.basic.features import SparseFeature
    from torch_rechub_amd.models.ranking import xDeepFM
    feas = [SparseFeature("a", 10, 16), SparseFeature("b", 10, 8)]
    with pytest.raises(ValueError, match="share one embed_dim"):
        xDeepFM(feas, feas, dict(MLP), [4, 4])


def np_xdeepfm(gold, cfg, bi=0):
    """float64 train-mode prediction of the fixture's model on batch ``bi``."""
    from test_ffm_host import np_mlp
    sd = {k[4:]: gold[k].astype(np.float64) for k in gold.files if k.startswith("sd0.")}
    spec = json.loads(str(gold["spec"]))
    emb = lambda d: sd[f"embedding.embed_dict.{d['name']}.weight"][gold[f"x{bi}.{d['name']}"]]  # noqa: E731
    fm = np.stack([emb(d) for d in spec["fm_features"]], 1)
    sparse = [emb(d) for d in spec["deep_features"] if d["kind"] == "SparseFeature"]
    dense = [gold[f"x{bi}.{d['name']}"].astype(np.float64)[:, None] for d in spec["deep_features"] if d["kind"] == "DenseFeature"]
    deep = np.concatenate(sparse + dense, 1)  # all sparse columns first, dense last
    y = fm.reshape(len(fm), -1) @ sd["linear.fc.weight"].T + sd["linear.fc.bias"]
    y = y + O.cin_fwd(fm, {k[4:]: v for k, v in sd.items() if k.startswith("cin.")}, XDEEPFM_MODELS[cfg][1])
    y = y + np_mlp(deep, sd, "mlp.mlp.", 2, True)
    return 1 / (1 + np.exp(-y[:, 0]))


@pytest.mark.parametrize("cfg", list(XDEEPFM_MODELS))
def test_numpy_model_restatement_matches_fixture(cfg):
    gold = load_golden(f"model_{cfg}.npz")
    np.testing.assert_allclose(np_xdeepfm(gold, cfg), gold["pred_train"], rtol=1e-4, atol=1e-6)


# ---- integration, ABI ---------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not available(), reason="needs the unmodified reference torch_rechub package (RECHUB_REFERENCE)")
def test_integration_patches_cin():
    import_reference()
    import torch_rechub.basic.layers as RL
    import torch_rechub.models.ranking  # noqa: F401  (imported BEFORE enable(), as tests/test_integration_patch.py does)
    import torch_rechub.trainers  # noqa: F401
    from torch_rechub_amd import integration
    from torch_rechub_amd.basic import layers as H
    original = RL.CIN
    try:
        names = integration.enable()
        assert "torch_rechub.basic.layers.CIN" in set(names)
        assert RL.CIN is H.CIN
    finally:
        integration.disable()
    assert RL.CIN is original and RL.CIN is not H.CIN


def test_cin_entry_points_reject_unsupported_shapes():
    """Argument validation of csrc/cin.hip: one past each limit is refused and nothing is launched (the pointers are never
    dereferenced)."""
    from torch_rechub_amd import _lib
    fake, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)
    n = ctypes.c_int(-1)
    pn = ctypes.c_void_p(ctypes.addressof(n))
    for (D, F, Hp, Ho), msg in (((129, 4, 4, 4), "embed_dim 129 unsupported"), ((0, 4, 4, 4), "embed_dim 0 unsupported"),
                                ((16, 65, 4, 4), "num_fields 65 unsupported"), ((16, 4, 257, 4), "input channels 257 unsupported"),
                                ((16, 4, 4, 513), "output channels 513 unsupported"), ((16, 4, 4, 0), "output channels 0 unsupported")):
        with pytest.raises(RuntimeError, match=msg):
            _lib.call("rh_cin_fwd", fake, 64, 16, fake, 64, fake, fake, 8, D, F, Hp, Ho, fake, null)
        with pytest.raises(RuntimeError, match=msg):
            _lib.call("rh_cin_bwd", fake, 64, 16, fake, 64, fake, fake, fake, 8, D, F, Hp, Ho, fake, fake, null)
        with pytest.raises(RuntimeError, match=msg):
            _lib.call("rh_cin_wgrad", fake, 64, 16, fake, 64, fake, fake, 8, D, F, Hp, Ho, fake, null)
        with pytest.raises(RuntimeError, match=msg):
            _lib.call("rh_cin_wgrad_chunks", 8, D, F, Hp, Ho, pn)
    assert n.value == -1
    with pytest.raises(RuntimeError, match="null argument"):
        _lib.call("rh_cin_fwd", null, 64, 16, fake, 64, fake, fake, 8, 16, 4, 4, 4, fake, null)
    # the chunk rule: enough workgroups to fill the chip, at most 16 chunks, whole 64-row tiles per chunk
    for (B, D, F, Hp, Ho), want in (((0, 16, 4, 4, 4), 0), ((1, 1, 1, 1, 1), 1), ((300, 1, 1, 1, 1), 5), ((2500, 1, 8, 8, 64), 14),
                                    ((4096, 16, 39, 100, 200), 3), ((4096, 16, 64, 256, 512), 1)):
        _lib.call("rh_cin_wgrad_chunks", B, D, F, Hp, Ho, pn)
        assert n.value == want, (B, D, F, Hp, Ho)
