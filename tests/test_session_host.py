"""NARM / STAMP / GRU4Rec without a GPU: the public names, the reference's state_dict layout and seeded initial tensors,
float64 numpy restatements of the GRU recurrence, the additive attention pooling and the full-catalogue cross entropy
(forward and backward, the math csrc/session.hip and csrc/stream_ce.hip implement) checked against torch autograd, and
the shape limits of the C entry points."""
import ctypes
import json

import numpy as np
import pytest
import torch

from conftest import load_golden

SESSION_CFGS = ["narm", "stamp", "gru4rec", "narm_inbatch"]
SEED = 2022


def sig(x):
    return 1.0 / (1.0 + np.exp(-x))


# ---- float64 restatements ---------------------------------------------------------------------------------------------
def np_gru(x, w_ih, w_hh, b_ih=None, b_hh=None):
    """One nn.GRU layer (gates r, z, n) from the zero state: x (B, T, I) -> (h_all (B, T, H), cache)."""
    B, T, _ = x.shape
    H = w_hh.shape[1]
    xw = x @ w_ih.T + (0 if b_ih is None else b_ih)
    h = np.zeros((B, H))
    hs, cache = [], []
    for t in range(T):
        hu = h @ w_hh.T + (0 if b_hh is None else b_hh)
        r = sig(xw[:, t, :H] + hu[:, :H])
        z = sig(xw[:, t, H:2 * H] + hu[:, H:2 * H])
        n = np.tanh(xw[:, t, 2 * H:] + r * hu[:, 2 * H:])
        cache.append((h, r, z, n, hu))
        h = (1 - z) * n + z * h
        hs.append(h)
    return np.stack(hs, 1), cache


def np_gru_bwd(x, w_ih, w_hh, cache, g):
    """Gradients (dx, dW_ih, dW_hh, db_ih, db_hh) of sum(g * h_all)."""
    B, T, _ = x.shape
    H = w_hh.shape[1]
    dh = np.zeros((B, H))
    dxw = np.zeros((B, T, 3 * H))
    dW_hh = np.zeros_like(w_hh)
    db_hh = np.zeros(3 * H)
    for t in range(T - 1, -1, -1):
        hp, r, z, n, hu = cache[t]
        d = dh + g[:, t]
        an = d * (1 - z) * (1 - n * n)
        dpz = d * (hp - n) * z * (1 - z)
        dpr = an * hu[:, 2 * H:] * r * (1 - r)
        ds = np.concatenate([dpr, dpz, an * r], 1)
        dxw[:, t] = np.concatenate([dpr, dpz, an], 1)
        dW_hh += ds.T @ hp
        db_hh += ds.sum(0)
        dh = d * z + ds @ w_hh
    flat = dxw.reshape(B * T, 3 * H)
    return dxw @ w_ih, flat.T @ x.reshape(B * T, -1), dW_hh, flat.sum(0), db_hh


def np_attn_pool(P, r, w0, mask, X, add=None, floor=False):
    """(out (B, Dx), cache): s = sigmoid(P + r) w0, e = exp(s) mask, a = e / den, out = sum_l a_l X_l (+ add)."""
    sg = sig(P + r[:, None, :])
    s = sg @ w0
    e = np.exp(s) * mask
    tot = e.sum(1, keepdims=True)
    den = np.maximum(tot, 1e-12) if floor else tot
    a = e / den
    out = np.einsum("bl,bld->bd", a, X) + (0 if add is None else add)
    return out, (sg, e, tot, den, a)


def np_attn_pool_bwd(P, r, w0, X, cache, g, floor=False):
    """(dP, dr, dw0, dX (pooling term only)) of sum(g * out)."""
    sg, e, tot, den, a = cache
    dX = a[:, :, None] * g[:, None, :]
    da = np.einsum("bd,bld->bl", g, X)
    c = (a * da).sum(1, keepdims=True)
    floored = floor & (tot < 1e-12)
    de = np.where(floored, da / den, (da - c) / den)
    ds = e * de
    dP = ds[:, :, None] * w0[None, None, :] * sg * (1 - sg)
    return dP, dP.sum(1), np.einsum("bl,blh->h", ds, sg), dX


def np_catalogue_ce(u, E, labels):
    """(loss, du, dE) of the mean cross entropy of u E^T against labels, every column a class."""
    z = u @ E.T
    m = z.max(1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(z - m).sum(1))
    B = u.shape[0]
    loss = (lse - z[np.arange(B), labels]).mean()
    p = np.exp(z - lse[:, None])
    p[np.arange(B), labels] -= 1
    p /= B
    return loss, p @ E, p.T @ u


# ---- restatements against torch autograd ------------------------------------------------------------------------------
@pytest.mark.parametrize("bias", [True, False])
@pytest.mark.parametrize("H", [1, 5, 10])
def test_gru_restatement_matches_torch_autograd(bias, H):
    torch.manual_seed(1)
    B, T, I = 4, 6, 7
    gru = torch.nn.GRU(I, H, batch_first=True, bias=bias).double()
    x = torch.randn(B, T, I, dtype=torch.float64, requires_grad=True)
    out, _ = gru(x)
    g = torch.randn_like(out)
    (out * g).sum().backward()
    p = {n: t.detach().numpy() for n, t in gru.named_parameters()}
    h, cache = np_gru(x.detach().numpy(), p["weight_ih_l0"], p["weight_hh_l0"], p.get("bias_ih_l0"), p.get("bias_hh_l0"))
    np.testing.assert_allclose(h, out.detach().numpy(), rtol=1e-10, atol=1e-12)
    dx, dwi, dwh, dbi, dbh = np_gru_bwd(x.detach().numpy(), p["weight_ih_l0"], p["weight_hh_l0"], cache, g.numpy())
    np.testing.assert_allclose(dx, x.grad.numpy(), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(dwi, gru.weight_ih_l0.grad.numpy(), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(dwh, gru.weight_hh_l0.grad.numpy(), rtol=1e-9, atol=1e-12)
    if bias:
        np.testing.assert_allclose(dbi, gru.bias_ih_l0.grad.numpy(), rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(dbh, gru.bias_hh_l0.grad.numpy(), rtol=1e-9, atol=1e-12)


@pytest.mark.parametrize("floor,add", [(False, False), (True, True), (True, False)])
def test_attention_pool_restatement_matches_torch_autograd(floor, add):
    torch.manual_seed(2)
    B, L, H, Dx = 5, 7, 6, 9
    P = torch.randn(B, L, H, dtype=torch.float64, requires_grad=True)
    r = torch.randn(B, H, dtype=torch.float64, requires_grad=True)
    w0 = torch.randn(H, dtype=torch.float64, requires_grad=True)
    X = torch.randn(B, L, Dx, dtype=torch.float64, requires_grad=True)
    A = torch.randn(B, Dx, dtype=torch.float64) if add else None
    mask = (torch.rand(B, L) < 0.7).double()
    mask[:, 0] = 1
    if floor:
        mask[1] = 0  # an empty row: F.normalize's floor keeps it finite (all zero)
    e = torch.exp(torch.sigmoid(P + r[:, None]) @ w0) * mask
    a = torch.nn.functional.normalize(e, p=1, dim=1) if floor else e / e.sum(1, keepdim=True)
    out = (a[:, :, None] * X).sum(1) + (0 if A is None else A)
    g = torch.randn(B, Dx, dtype=torch.float64)
    (out * g).sum().backward()
    got, cache = np_attn_pool(P.detach().numpy(), r.detach().numpy(), w0.detach().numpy(), mask.numpy(),
                              X.detach().numpy(), None if A is None else A.numpy(), floor)
    np.testing.assert_allclose(got, out.detach().numpy(), rtol=1e-12, atol=1e-12)
    dP, dr, dw0, dX = np_attn_pool_bwd(P.detach().numpy(), r.detach().numpy(), w0.detach().numpy(), X.detach().numpy(),
                                       cache, g.numpy(), floor)
    for mine, ref in ((dP, P), (dr, r), (dw0, w0), (dX, X)):
        np.testing.assert_allclose(mine, ref.grad.numpy(), rtol=1e-10, atol=1e-12)


def test_catalogue_ce_restatement_matches_torch_autograd():
    torch.manual_seed(3)
    B, D, V = 6, 5, 11
    u = torch.randn(B, D, dtype=torch.float64, requires_grad=True)
    E = torch.randn(V, D, dtype=torch.float64, requires_grad=True)
    y = torch.tensor([0, 3, 10, 0, 5, 7])
    loss = torch.nn.CrossEntropyLoss()(u @ E.T, y)
    loss.backward()
    ll, du, dE = np_catalogue_ce(u.detach().numpy(), E.detach().numpy(), y.numpy())
    assert abs(ll - loss.item()) < 1e-12
    np.testing.assert_allclose(du, u.grad.numpy(), rtol=1e-10, atol=1e-14)
    np.testing.assert_allclose(dE, E.grad.numpy(), rtol=1e-10, atol=1e-14)


# ---- models -----------------------------------------------------------------------------------------------------------
def session_groups(gold):
    from torch_rechub_amd.basic.features import SequenceFeature, SparseFeature
    spec = json.loads(str(gold["spec"]))
    made = {}

    def mk(d):
        key = (d["kind"], d["name"])
        if key not in made:
            if d["kind"] == "SparseFeature":
                made[key] = SparseFeature(d["name"], d["vocab_size"], d["embed_dim"], shared_with=d["shared_with"],
                                          padding_idx=d["padding_idx"])
            else:
                made[key] = SequenceFeature(d["name"], d["vocab_size"], d["embed_dim"], pooling=d["pooling"],
                                            shared_with=d["shared_with"], padding_idx=d["padding_idx"])
        return made[key]
    return {k: [mk(d) for d in v] for k, v in spec.items()}


def build_session_model(cfg, gold):
    """Same constructor calls as tools/gen_golden_session.py::build, on the torch_rechub_amd classes."""
    from torch_rechub_amd.models.matching import GRU4Rec, NARM, STAMP
    gr = session_groups(gold)
    if cfg in ("narm", "narm_inbatch"):
        item = gr["item_feature"][0] if cfg == "narm_inbatch" else None
        return NARM(gr["item_history_feature"][0], 10, 0.0, 0.0, item_feature=item)
    if cfg == "stamp":
        return STAMP(gr["item_history_feature"][0], 0.05, 0.1)
    D = gr["history_features"][0].embed_dim
    return GRU4Rec(gr["user_features"], gr["history_features"], gr["item_features"], gr["neg_item_feature"],
                   user_params={"dims": [16, D]})


def test_public_names_and_integration_binding():
    from torch_rechub_amd import integration, ops
    from torch_rechub_amd.models import matching
    for n in ("NARM", "STAMP", "GRU4Rec"):
        assert n in matching.__all__ and hasattr(matching, n)
        assert n in integration._MODELS["matching"]
    for n in ("gru_layers", "gru_layers_ok", "additive_attention_pool", "catalogue_cross_entropy"):
        assert callable(getattr(ops, n))


@pytest.mark.parametrize("cfg", SESSION_CFGS)
def test_state_dict_keys_and_seeded_initial_tensors_match_the_reference(cfg):
    gold = load_golden(f"model_session_{cfg}.npz")
    torch.manual_seed(SEED)
    model = build_session_model(cfg, gold)
    sd = model.state_dict()
    want = [k[len("sd0."):] for k in gold.files if k.startswith("sd0.")]
    assert list(sd) == want
    for k in want:
        assert tuple(sd[k].shape) == gold["sd0." + k].shape, k
        # (GRU4Rec's D = 12 tables are stored padded to a kernel width, whose construction draws from the generator
        # too: its seeded stream is compared at a kernel width in test_integration_session.py instead)
        if cfg != "gru4rec":
            np.testing.assert_array_equal(sd[k].numpy(), gold["sd0." + k], err_msg=k)


def test_narm_and_stamp_tables_are_dense_and_stamp_row0_is_drawn():
    gold = load_golden("model_session_stamp.npz")
    torch.manual_seed(SEED)
    model = build_session_model("stamp", gold)
    assert model.item_emb._rh_dense and model.item_emb.weight[0].abs().sum() > 0
    torch.manual_seed(SEED)
    assert build_session_model("narm", load_golden("model_session_narm.npz")).item_emb._rh_dense


def test_gru4rec_num_layers_in_user_params_raises_as_the_reference():
    from torch_rechub_amd.basic.features import SequenceFeature, SparseFeature
    from torch_rechub_amd.models.matching import GRU4Rec
    hist = [SequenceFeature("h", 30, 8, pooling="concat", shared_with="i")]
    item = [SparseFeature("i", 30, 8)]
    neg = [SequenceFeature("n", 30, 8, pooling="concat", shared_with="i")]
    with pytest.raises(TypeError):
        GRU4Rec([SparseFeature("u", 5, 8)], hist, item, neg, user_params={"dims": [8], "num_layers": 1})


def test_entry_points_refuse_the_first_shape_past_each_limit():
    from torch_rechub_amd import _lib
    null = ctypes.c_void_p(0)
    fake = ctypes.c_void_p(4096)  # never dereferenced: validation fails first
    assert _lib.H.RH_GRU_MAX_H == 128
    with pytest.raises(RuntimeError, match="hidden size 129 unsupported"):
        _lib.call("rh_gru_fwd", fake, fake, null, 4, 3, 129, fake, fake, null)
    with pytest.raises(RuntimeError, match="hidden size 129 unsupported"):
        _lib.call("rh_gru_bwd", fake, fake, fake, fake, fake, 4, 3, 129, fake, fake, null)
    with pytest.raises(RuntimeError, match="hidden size 0 unsupported"):
        _lib.call("rh_gru_fwd", fake, fake, null, 4, 3, 0, fake, fake, null)
    for L, H, Dx in ((1025, 8, 8), (8, 4097, 8), (8, 8, 4097)):
        with pytest.raises(RuntimeError, match="unsupported"):
            _lib.call("rh_attn_pool_fwd", fake, fake, fake, fake, fake, null, 4, L, H, Dx, 0, fake, fake, fake, null)
        with pytest.raises(RuntimeError, match="unsupported"):
            _lib.call("rh_attn_pool_bwd", fake, fake, fake, fake, fake, fake, fake, 4, L, H, Dx, 0, fake, fake, fake, fake,
                      fake, null)
    with pytest.raises(RuntimeError, match="unsupported"):
        _lib.call("rh_catalogue_ce_fwd", fake, fake, fake, 4, 8, (1 << 30) + 1, fake, fake, fake, fake, fake, null, null)
    with pytest.raises(RuntimeError, match="unsupported"):
        _lib.call("rh_catalogue_ce_fwd", fake, fake, fake, 4, 8, 1, fake, fake, fake, fake, fake, null, null)
    with pytest.raises(RuntimeError, match="unsupported"):
        _lib.call("rh_catalogue_ce_bwd", fake, fake, fake, fake, fake, fake, 0, 8, 100, fake, fake, fake, fake, null)


def test_ops_refuse_without_a_kernel():
    from torch_rechub_amd import ops
    gru = torch.nn.GRU(4, 129)
    assert not ops.gru_layers_ok(gru, torch.zeros(2, 3, 4))
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.catalogue_cross_entropy(torch.zeros(2, 3), torch.zeros(5, 3), torch.zeros(2, dtype=torch.long))
