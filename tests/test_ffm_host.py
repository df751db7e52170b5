"""DeepFFM / FatDeepFFM / FFM / CEN without a GPU: the public names, the reference's state_dict layout (including the
PaddedEmbedding tables of the Criteo widths), the integration patch, and a float64 numpy restatement of the layers and
models checked against the fixtures of tools/gen_golden_ffm.py."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden
from oracle.ref_import import available, import_reference

FFM_MODELS = ["deepffm", "deepffm_criteo", "fatdeepffm"]


def ffm_features(gold):
    """(linear, cross) feature lists of a fixture.  Built here rather than by conftest.features_from_spec, which keys
    features by (kind, name) and would merge the linear and the cross feature of the same name."""
    from torch_rechub_amd.basic.features import SparseFeature
    spec = json.loads(str(gold["spec"]))
    mk = lambda d: SparseFeature(d["name"], d["vocab_size"], d["embed_dim"], padding_idx=d["padding_idx"])  # noqa: E731
    return [mk(d) for d in spec["linear_features"]], [mk(d) for d in spec["cross_features"]]


def build_ffm_model(cfg, gold):
    from torch_rechub_amd.models.ranking import DeepFFM, FatDeepFFM
    linear, cross = ffm_features(gold)
    D = cross[0].embed_dim
    mlp = {"dims": [32, 16], "dropout": 0.0, "activation": "relu"}
    if cfg == "fatdeepffm":
        return FatDeepFFM(linear, cross, D, 3, mlp)
    return DeepFFM(linear, cross, D, mlp)


def test_public_names_import():
    from torch_rechub_amd.basic.layers import CEN, FFM  # noqa: F401
    from torch_rechub_amd.models.ranking import DeepFFM, FatDeepFFM  # noqa: F401
    import torch_rechub_amd.models.ranking as R
    assert {"DeepFFM", "FatDeepFFM"} <= set(R.__all__)


@pytest.mark.parametrize("cfg", FFM_MODELS)
def test_state_dict_layout_and_checkpoint_load_match_reference(cfg):
    gold = load_golden(f"model_{cfg}.npz")
    model = build_ffm_model(cfg, gold)
    want = {k[4:]: gold[k] for k in gold.files if k.startswith("sd0.")}
    sd = model.state_dict()
    assert list(sd.keys()) == [k[4:] for k in gold.files if k.startswith("sd0.")]
    for k, v in want.items():
        assert tuple(sd[k].shape) == v.shape, k
        assert sd[k].dtype == torch.from_numpy(v).dtype, k
    model.load_state_dict({k: torch.from_numpy(v) for k, v in want.items()})
    for k, v in want.items():
        np.testing.assert_array_equal(model.state_dict()[k].numpy(), v)
    if cfg == "deepffm_criteo":  # width 10 / width 1 stored padded; the padding stays zero after the load
        w = model.ffm_embedding.embed_dict["C1"].weight
        assert w.shape[1] == 16 and torch.count_nonzero(w[:, 10:]) == 0
        assert model.linear_embedding.embed_dict["C1"].weight.shape[1] == 4


def test_cen_and_ffm_layer_signatures():
    from torch_rechub_amd.basic.layers import CEN, FFM
    f = FFM(6, reduce_sum=False)
    assert f.num_fields == 6 and f.reduce_sum is False and FFM(3).reduce_sum is True
    gold = load_golden("ffm_layers.npz")
    cen = CEN(10, 15, 3)
    want = {k[len("cen.sd."):]: gold[k] for k in gold.files if k.startswith("cen.sd.")}
    sd = cen.state_dict()
    assert list(sd.keys()) == list(want.keys())
    assert all(tuple(sd[k].shape) == want[k].shape for k in want)


@pytest.mark.skipif(not available(), reason="needs the unmodified reference torch_rechub package (RECHUB_REFERENCE)")
def test_integration_patches_deepffm_fatdeepffm_ffm_and_cen():
    import_reference()
    import torch_rechub.models.ranking as RR
    import torch_rechub.basic.layers as RL
    import torch_rechub.models.ranking.deepffm as ref_deepffm
    from torch_rechub_amd import integration
    from torch_rechub_amd.basic import layers as H
    from torch_rechub_amd.models.ranking import DeepFFM, FatDeepFFM
    try:
        names = integration.enable()
        assert {"torch_rechub.models.ranking.DeepFFM", "torch_rechub.models.ranking.FatDeepFFM",
                "torch_rechub.basic.layers.FFM", "torch_rechub.basic.layers.CEN"} <= set(names)
        assert RR.DeepFFM is DeepFFM and RR.FatDeepFFM is FatDeepFFM
        assert RL.FFM is H.FFM and RL.CEN is H.CEN and ref_deepffm.FFM is H.FFM and ref_deepffm.CEN is H.CEN
    finally:
        integration.disable()
    assert RL.FFM is not H.FFM


# ---- float64 numpy restatement ----------------------------------------------------------------------------------------
def np_ffm(x, reduce_sum):
    F = x.shape[1]
    out = np.stack([x[:, i, j, :] * x[:, j, i, :] for i in range(F - 1) for j in range(i + 1, F)], axis=1)
    return out.sum(-1, keepdims=True) if reduce_sum else out


def np_mlp(h, sd, prefix, n_hidden, output_layer):
    """[Linear, BatchNorm1d (train: batch statistics), ReLU, Dropout(0)] x n_hidden (+ Linear(., 1))."""
    for k in range(n_hidden):
        lin, bn = f"{prefix}{4 * k}.", f"{prefix}{4 * k + 1}."
        h = h @ sd[lin + "weight"].T + sd[lin + "bias"]
        mu, var = h.mean(0), h.var(0)
        h = (h - mu) / np.sqrt(var + 1e-5) * sd[bn + "weight"] + sd[bn + "bias"]
        h = np.maximum(h, 0)
    if output_layer:
        lin = f"{prefix}{4 * n_hidden}."
        h = h @ sd[lin + "weight"].T + sd[lin + "bias"]
    return h


def np_cen(em, sd, prefix):
    d = np.maximum((sd[prefix + "u"] * em).sum(-1), 0)
    s = np_mlp(d, sd, prefix + "mlp_att.mlp.", 2, False)
    return (s[:, :, None] * em).reshape(em.shape[0], -1)


def np_deepffm(gold, cfg, bi=0):
    sd = {k[4:]: gold[k].astype(np.float64) for k in gold.files if k.startswith("sd0.")}
    spec = json.loads(str(gold["spec"]))
    cross = spec["cross_features"]
    F = len(cross)
    x = {d["name"]: gold[f"x{bi}.{d['name']}"] for d in cross}
    y_lin = sum(sd[f"linear_embedding.embed_dict.{d['name']}.weight"][x[d["name"]], 0] for d in spec["linear_features"])
    inp = np.stack([np.stack([sd[f"ffm_embedding.embed_dict.{d['name']}.weight"][x[d["name"]] * F + j]
                              for j in range(F)], 1) for d in cross], 1)  # (B, F, F, D)
    em = np_ffm(inp, False)
    em = np_cen(em, sd, "cen.") if cfg == "fatdeepffm" else em.reshape(em.shape[0], -1)
    y = np_mlp(em, sd, "mlp_out.mlp.", 2, True)[:, 0] + y_lin + sd["b"][0]
    return 1 / (1 + np.exp(-y))


@pytest.mark.parametrize("rs", [0, 1])
def test_numpy_ffm_restatement_matches_fixture(rs):
    gold = load_golden("ffm_layers.npz")
    x = gold[f"ffm_rs{rs}.x"].astype(np.float64)
    np.testing.assert_allclose(np_ffm(x, rs), gold[f"ffm_rs{rs}.out"], rtol=1e-5, atol=1e-6)


def test_numpy_cen_restatement_matches_fixture():
    gold = load_golden("ffm_layers.npz")
    sd = {k[len("cen.sd."):]: gold[k].astype(np.float64) for k in gold.files if k.startswith("cen.sd.")}
    got = np_cen(gold["cen.em"].astype(np.float64), sd, "")
    np.testing.assert_allclose(got, gold["cen.out"], rtol=1e-4, atol=1e-5)


@pytest.mark.parametrize("cfg", FFM_MODELS)
def test_numpy_model_restatement_matches_fixture(cfg):
    gold = load_golden(f"model_{cfg}.npz")
    np.testing.assert_allclose(np_deepffm(gold, cfg), gold["pred_train"], rtol=1e-4, atol=1e-6)


def test_ffm_entry_points_reject_unsupported_shapes():
    """Argument validation of csrc/ffm.hip: nothing is launched (the pointers are never dereferenced)."""
    import ctypes

    from torch_rechub_amd import _lib
    fake, null = ctypes.c_void_p(4096), ctypes.c_void_p(0)
    with pytest.raises(RuntimeError, match="num_fields 65 unsupported"):
        _lib.call("rh_ffm_fwd", fake, fake, 1, null, 0, 4, 65, 4, 4, 0, fake, 8320, null, null)
    with pytest.raises(RuntimeError, match="embed_dim 129 unsupported"):
        _lib.call("rh_ffm_fwd", null, null, 0, fake, 0, 4, 3, 129, 129, 0, fake, 387, null, null)
    with pytest.raises(RuntimeError, match="row width 8 unsupported"):
        _lib.call("rh_ffm_bwd", fake, fake, 1, null, 0, 4, 3, 10, 8, 0, fake, 30, null, 0, 0, null, null, null)
    with pytest.raises(RuntimeError, match="either"):
        _lib.call("rh_ffm_fwd", fake, null, 1, null, 0, 4, 3, 4, 4, 0, fake, 12, null, null)
    assert _lib.call("rh_cen_nchunks", 4096) == 64


def np_ffm_bwd(x, g, reduce_sum):
    """dX (B, F, F, D) of np_ffm for upstream g (B, P, D) or (B, P, 1): dX[:, i, j] = g_p x[:, j, i], the diagonal zero.
    Each element is one product, so in float32 it is what a float32 kernel must produce bit for bit."""
    B, F, _, D = x.shape
    gx = np.zeros_like(x)
    for p, (i, j) in enumerate((i, j) for i in range(F - 1) for j in range(i + 1, F)):
        gp = g[:, p, :] if not reduce_sum else np.broadcast_to(g[:, p, :1], (B, D))
        gx[:, i, j] = gp * x[:, j, i]
        gx[:, j, i] = gp * x[:, i, j]
    return gx


def np_cen_desc(em, u):
    """CEN descriptor d (B, P) = relu(sum_d u * em) for em (B, P, D), u (P, D)."""
    return np.maximum((u[None] * em).sum(-1), 0)


def np_cen_desc_bwd(em, u, g_d, d=None):
    """(g_em (B, P, D), g_u (P, D)) of np_cen_desc; a tie at d = 0 passes no gradient, as torch's ReLU.  ``d``: the
    descriptor whose ReLU mask to use (default: the float64 one)."""
    gg = np.where((np_cen_desc(em, u) if d is None else d) > 0, g_d, 0.0)
    return gg[..., None] * u[None], (gg[..., None] * em).sum(0)


def np_cen_rescale_bwd(em, s, g):
    """(g_em (B, P, D), g_s (B, P)) of aem = s[..., None] * em for upstream g (B, P, D)."""
    return s[..., None] * g, (g * em).sum(-1)


@pytest.mark.parametrize("rs", [0, 1])
def test_numpy_ffm_backward_matches_autograd(rs):
    g = torch.Generator().manual_seed(7 + rs)
    B, F, D = 5, 4, 3
    x = torch.randn(B, F, F, D, generator=g, dtype=torch.float64, requires_grad=True)
    out = torch.stack([x[:, i, j, :] * x[:, j, i, :] for i in range(F - 1) for j in range(i + 1, F)], dim=1)
    if rs:
        out = out.sum(-1, keepdim=True)
    np.testing.assert_allclose(np_ffm(x.detach().numpy(), rs), out.detach().numpy(), rtol=1e-15, atol=0)
    gy = torch.randn(out.shape, generator=g, dtype=torch.float64)
    out.backward(gy)
    want = x.grad.numpy()
    got = np_ffm_bwd(x.detach().numpy(), gy.numpy(), rs)
    np.testing.assert_allclose(got, want, rtol=1e-15, atol=0)
    assert not got[:, range(F), range(F)].any()


def test_numpy_cen_backward_matches_autograd():
    g = torch.Generator().manual_seed(9)
    B, P, D = 7, 6, 5
    em = torch.randn(B, P, D, generator=g, dtype=torch.float64)
    em[0, 1] = 0.0  # d = 0 exactly: a tie of the ReLU
    em[2, 3] = 0.0
    em.requires_grad_(True)
    u = torch.randn(P, D, generator=g, dtype=torch.float64, requires_grad=True)
    d = torch.relu((u * em).sum(-1))
    assert d[0, 1] == 0 and d[2, 3] == 0 and (d == 0).sum() > 2  # ties and negative sums both present
    np.testing.assert_allclose(np_cen_desc(em.detach().numpy(), u.detach().numpy()), d.detach().numpy(), rtol=1e-14)
    gd = torch.randn(B, P, generator=g, dtype=torch.float64)
    d.backward(gd)
    g_em, g_u = np_cen_desc_bwd(em.detach().numpy(), u.detach().numpy(), gd.numpy())
    np.testing.assert_allclose(g_em, em.grad.numpy(), rtol=1e-14, atol=1e-15)
    np.testing.assert_allclose(g_u, u.grad.numpy(), rtol=1e-14, atol=1e-15)
    assert not g_em[0, 1].any() and not g_em[2, 3].any()
    em2 = em.detach().clone().requires_grad_(True)
    s = torch.randn(B, P, generator=g, dtype=torch.float64, requires_grad=True)
    out = (s.unsqueeze(-1) * em2).reshape(B, -1)
    gy = torch.randn(out.shape, generator=g, dtype=torch.float64)
    out.backward(gy)
    g_em, g_s = np_cen_rescale_bwd(em2.detach().numpy(), s.detach().numpy(), gy.numpy().reshape(B, P, D))
    np.testing.assert_allclose(g_em.reshape(B, -1), em2.grad.numpy().reshape(B, -1), rtol=1e-15, atol=0)
    np.testing.assert_allclose(g_s, s.grad.numpy(), rtol=1e-14, atol=1e-15)
