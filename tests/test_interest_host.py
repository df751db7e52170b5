"""YoutubeDNN / MIND / ComiRec without a GPU: the public names, the reference's state_dict layout and seeded initial
tensors, and a float64 numpy restatement of capsule routing, self-attentive pooling and list-wise scoring (forward and
backward, the math csrc/interest.hip implements) checked against the fixtures of tools/gen_golden_match.py."""
import json

import numpy as np
import pytest
import torch

from conftest import load_golden

MATCH_MODELS = ["youtubednn", "mind", "comirec_dr", "comirec_sa"]
SEED = 2022


def match_groups(gold):
    from torch_rechub_amd.basic.features import SequenceFeature, SparseFeature
    spec = json.loads(str(gold["spec"]))
    made = {}

    def mk(d):
        key = (d["kind"], d["name"], d.get("pooling"))
        if key not in made:
            if d["kind"] == "SparseFeature":
                made[key] = SparseFeature(d["name"], d["vocab_size"], d["embed_dim"], shared_with=d["shared_with"],
                                          padding_idx=d["padding_idx"])
            else:
                made[key] = SequenceFeature(d["name"], d["vocab_size"], d["embed_dim"], pooling=d["pooling"],
                                            shared_with=d["shared_with"], padding_idx=d["padding_idx"])
        return made[key]
    return {k: [mk(d) for d in v] for k, v in spec.items()}


def build_match_model(cfg, gold):
    """Same constructor calls as tools/gen_golden_match.py::build_match_model, on the torch_rechub_amd classes."""
    from torch_rechub_amd.models.matching import MIND, ComirecDR, ComirecSA, YoutubeDNN
    gr = match_groups(gold)
    if cfg == "youtubednn":
        return YoutubeDNN(gr["user_features"], gr["item_features"], gr["neg_item_feature"], user_params={"dims": [32, 16]},
                          temperature=0.02)
    args = (gr["user_features"], gr["history_features"], gr["item_features"], gr["neg_item_feature"])
    L = gold["x0.hist_item_id"].shape[1]
    if cfg == "mind":
        return MIND(*args, max_length=L, temperature=0.02)
    if cfg == "comirec_dr":
        return ComirecDR(*args, max_length=L, temperature=0.02)
    return ComirecSA(*args, temperature=0.02)


# ---- float64 restatements -------------------------------------------------------------------------------------------
def squash(s):
    n = (s * s).sum(-1, keepdims=True)
    return n / (1 + n) / np.sqrt(n + 1e-9) * s


def squash_bwd(s, g):
    n = (s * s).sum(-1, keepdims=True)
    r = np.sqrt(n + 1e-9)
    f = n / (1 + n) / r
    fp = 1 / ((1 + n) ** 2 * r) - 0.5 * n / ((1 + n) * (n + 1e-9) * r)
    return f * g + 2 * fp * (s * g).sum(-1, keepdims=True) * s


def np_capsule(uhat, mask, init, iters):
    """uhat (B, I, L, D), mask (B, L) -> (cap (B, I, D), last softmax weights (B, I, L), last pre-squash s (B, I, D))."""
    B, I, L, D = uhat.shape
    lg = np.zeros((B, I, L)) if init is None else init.astype(np.float64)
    for it in range(iters):
        e = np.exp(lg - lg.max(-1, keepdims=True))
        sw = e / e.sum(-1, keepdims=True)
        sw = np.where(mask[:, None, :] == 0, 0.0, sw)
        s = np.einsum("bil,bild->bid", sw, uhat)
        cap = squash(s)
        if it < 2:
            lg = lg + np.einsum("bild,bid->bil", uhat, cap)
    return cap, sw, s


def np_capsule_layer(gold, kind, rt):
    """(out, g_e, {param: grad}) of the reference CapsuleNetwork from the fixture's inputs, in float64."""
    k = f"caps{kind}_rt{rt}."
    e = gold[k + "e"].astype(np.float64)
    mask = gold["mask"]
    B, L, D = e.shape
    gy = gold[k + "g_out"].astype(np.float64)
    init = gold[k + "init"] if kind == 0 else None
    if kind == 2:
        w = gold[k + "sd.w"][0].astype(np.float64)  # (L, I*D, D)
        I = w.shape[1] // D
        uh = np.einsum("ljk,blk->blj", w, e).reshape(B, L, I, D).transpose(0, 2, 1, 3)
    else:
        W = gold[k + "sd.linear.weight"].astype(np.float64)
        u = e @ W.T
        I = 4 if kind == 0 else W.shape[0] // D
        uh = (np.tile(u, (1, 1, I)) if kind == 0 else u).reshape(B, L, I, D).transpose(0, 2, 1, 3)
    cap, sw, s = np_capsule(uh, mask, init, rt)
    grads = {}
    if rt <= 2:
        return cap, np.zeros_like(e), grads
    gs = squash_bwd(s, gy)
    guh = np.einsum("bil,bid->blid", sw, gs)  # (B, L, I, D)
    if kind == 2:
        g_e = np.einsum("ljk,blj->blk", w, guh.reshape(B, L, I * D))
        grads["w"] = np.einsum("blj,blk->ljk", guh.reshape(B, L, I * D), e)[None]
    else:
        gu = guh.sum(2) if kind == 0 else guh.reshape(B, L, I * D)
        g_e = gu @ W
        grads["linear.weight"] = np.einsum("blj,blk->jk", gu, e)
    return cap, g_e, grads


def np_sa(e, mask, W1, W2, gy):
    H = np.tanh(e @ W1)
    # the mask term in float32 as the reference forms it: on a fully padded row A + -1e9 rounds to a few values 64 apart
    A = ((H @ W2).astype(np.float32) + np.float32(-1e9) * (1 - mask.astype(np.float32))[..., None]).astype(np.float64)
    ex = np.exp(A - A.max(1, keepdims=True))
    P = ex / ex.sum(1, keepdims=True)  # (B, L, I)
    out = np.einsum("bli,bld->bid", P, e)
    gP = np.einsum("bid,bld->bli", gy, e)
    gA = P * (gP - (P * gP).sum(1, keepdims=True))
    gH = gA @ W2.T
    gZ = gH * (1 - H * H)
    g_e = np.einsum("bli,bid->bld", P, gy) + gZ @ W1.T
    return out, g_e, {"W1": np.einsum("bld,blh->dh", e, gZ), "W2": np.einsum("blh,bli->hi", H, gA)}


def np_listwise(u, pos, neg, temperature, g=None):
    """u (B, I, D) normalised; pos (B, D), neg (B, K, D) raw rows -> logits (B, 1 + K) [and the gradients for g]."""
    rows = np.concatenate([pos[:, None], neg], 1)
    n = np.linalg.norm(rows, axis=-1, keepdims=True)
    vh = rows / np.maximum(n, 1e-12)
    best = np.argmax(np.einsum("bid,bd->bi", u, vh[:, 0]), 1)
    ub = u[np.arange(len(u)), best]
    logits = np.einsum("bd,bkd->bk", ub, vh) / temperature
    if g is None:
        return logits, best
    gk = g / temperature
    g_u = np.zeros_like(u)
    g_u[np.arange(len(u)), best] = np.einsum("bk,bkd->bd", gk, vh)
    gvh = gk[..., None] * ub[:, None]
    g_rows = (gvh - vh * (gvh * vh).sum(-1, keepdims=True)) / np.maximum(n, 1e-12)
    return logits, best, g_u, g_rows[:, 0], g_rows[:, 1:]


# ---- tests ----------------------------------------------------------------------------------------------------------
def test_public_names_import():
    from torch_rechub_amd.basic.layers import CapsuleNetwork, MultiInterestSA  # noqa: F401
    from torch_rechub_amd.models.matching import MIND, ComirecDR, ComirecSA, YoutubeDNN  # noqa: F401
    import torch_rechub_amd.models.matching as M
    assert {"YoutubeDNN", "MIND", "ComirecDR", "ComirecSA"} <= set(M.__all__)
    from torch_rechub_amd import integration
    assert {"CapsuleNetwork", "MultiInterestSA"} <= set(integration._LAYERS)
    assert {"YoutubeDNN", "MIND", "ComirecDR", "ComirecSA"} <= set(integration._MODELS["matching"])


@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("rt", [1, 3, 4])
def test_capsule_restatement_matches_reference(kind, rt):
    gold = load_golden("interest_layers.npz")
    k = f"caps{kind}_rt{rt}."
    out, g_e, grads = np_capsule_layer(gold, kind, rt)
    np.testing.assert_allclose(out, gold[k + "out"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(g_e, gold[k + "g_e"], rtol=1e-5, atol=1e-6)
    for n, gw in grads.items():
        np.testing.assert_allclose(gw, gold[k + "grad." + n], rtol=1e-5, atol=1e-6, err_msg=n)
    if rt <= 2:  # routing on the detached projections only: no gradient anywhere in the reference
        assert not any(n.startswith(k + "grad.") for n in gold.files)
        assert not gold[k + "g_e"].any()
    # the fully padded row routes nothing: zero capsules
    assert not gold[k + "out"][0].any()


def test_sa_restatement_matches_reference():
    gold = load_golden("interest_layers.npz")
    e = gold["sa.e"].astype(np.float64)
    out, g_e, grads = np_sa(e, gold["mask"], gold["sa.sd.W1"].astype(np.float64), gold["sa.sd.W2"].astype(np.float64),
                            gold["sa.g_out"].astype(np.float64))
    np.testing.assert_allclose(out, gold["sa.out"], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(g_e, gold["sa.g_e"], rtol=1e-5, atol=1e-6)
    for n in ("W1", "W2"):
        np.testing.assert_allclose(grads[n], gold["sa.grad." + n], rtol=1e-5, atol=1e-5, err_msg=n)
    assert "sa.grad.W3" not in gold.files  # constructed, never used: its .grad stays None


@pytest.mark.parametrize("cfg", ["youtubednn", "comirec_dr", "comirec_sa"])
def test_listwise_restatement_matches_reference_eval_logits(cfg):
    gold = load_golden(f"model_{cfg}.npz")
    table = gold["sd0.embedding.embed_dict.item_id.weight"].astype(np.float64)
    pos, neg = table[gold["x0.item_id"]], table[gold["x0.neg_items"]]
    u = gold["user_emb"].astype(np.float64)
    if u.ndim == 2:
        u = u[:, None]
    logits, _ = np_listwise(u, pos, neg, 0.02 if cfg == "youtubednn" else 1.0)
    np.testing.assert_allclose(logits, gold["pred_eval"], rtol=1e-5, atol=1e-5 if cfg == "youtubednn" else 1e-6)
    np.testing.assert_allclose(gold["item_emb"], pos / np.linalg.norm(pos, axis=1, keepdims=True), rtol=1e-5, atol=1e-6)


def test_listwise_backward_restatement_against_autograd():
    g = torch.Generator().manual_seed(7)
    B, I, D, K = 9, 4, 16, 5
    u = torch.nn.functional.normalize(torch.randn(B, I, D, generator=g, dtype=torch.float64), dim=-1).requires_grad_(True)
    pos = torch.randn(B, D, generator=g, dtype=torch.float64).requires_grad_(True)
    neg = torch.randn(B, K, D, generator=g, dtype=torch.float64).requires_grad_(True)
    items = torch.nn.functional.normalize(torch.cat([pos[:, None], neg], 1), p=2, dim=-1)
    k = torch.argmax(torch.bmm(u, items[:, 0].unsqueeze(-1)), dim=1).squeeze(-1)
    y = (u[torch.arange(B), k].unsqueeze(1) * items).sum(-1) / 0.5
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    logits, best, g_u, g_pos, g_neg = np_listwise(u.detach().numpy(), pos.detach().numpy(), neg.detach().numpy(), 0.5,
                                                  gy.numpy())
    np.testing.assert_allclose(logits, y.detach().numpy(), rtol=1e-12)
    assert (best == k.numpy()).all()
    for got, want in ((g_u, u.grad), (g_pos, pos.grad), (g_neg, neg.grad)):
        np.testing.assert_allclose(got, want.numpy(), rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("cfg", MATCH_MODELS)
def test_state_dict_layout_and_seeded_init_match_reference(cfg):
    gold = load_golden(f"model_{cfg}.npz")
    torch.manual_seed(SEED)
    model = build_match_model(cfg, gold)
    want = [k[4:] for k in gold.files if k.startswith("sd0.")]
    sd = model.state_dict()
    assert list(sd.keys()) == want
    for k in want:
        ref = gold["sd0." + k]
        assert tuple(sd[k].shape) == ref.shape and sd[k].dtype == torch.from_numpy(ref).dtype, k
        if ".embed_dict." in k or k == "capsule.w":
            continue  # re-drawn by the generator (tables N(0, 0.1), ComirecDR's uninitialised w N(0, 0.3))
        np.testing.assert_array_equal(sd[k].numpy(), ref, err_msg=f"{cfg}: seeded initial {k}")
    model.load_state_dict({k: torch.from_numpy(gold["sd0." + k]) for k in want})


def test_capsule_and_sa_constructors_mirror_reference():
    from torch_rechub_amd.basic.layers import CapsuleNetwork, MultiInterestSA
    gold = load_golden("interest_layers.npz")
    for kind in (0, 1, 2):
        I = 3 if kind == 1 else 4
        c = CapsuleNetwork(16, 8, bilinear_type=kind, interest_num=I, routing_times=3)
        want = [k[len(f"caps{kind}_rt3.sd."):] for k in gold.files if k.startswith(f"caps{kind}_rt3.sd.")]
        assert list(c.state_dict().keys()) == want
        assert all(tuple(c.state_dict()[k].shape) == gold[f"caps{kind}_rt3.sd." + k].shape for k in want)
        assert c.stop_grad and c.relu_layer is False and c.routing_init is None
    sa = MultiInterestSA(16, 4)
    assert sa.hidden_dim == 64 and list(sa.state_dict().keys()) == ["W1", "W2", "W3"]
    with pytest.raises(AttributeError):  # as in the reference: an explicit hidden_dim leaves self.hidden_dim unset
        MultiInterestSA(16, 4, hidden_dim=32)
    torch.manual_seed(0)
    a = CapsuleNetwork(16, 8, bilinear_type=2).state_dict()
    torch.manual_seed(0)
    b = torch.nn.Linear(16, 16, bias=False).weight.detach()
    assert torch.equal(a["relu.0.weight"], b)  # type 2 draws nothing beyond the relu Linear
    assert torch.equal(torch.rand(1), (torch.manual_seed(0), torch.nn.Linear(16, 16, bias=False), torch.rand(1))[2])


def test_models_refuse_cpu_tensors():
    gold = load_golden("model_mind.npz")
    model = build_match_model("mind", gold)
    x = {k[3:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("x0.")}
    with pytest.raises(RuntimeError):
        model(x)


def test_interest_entry_points_reject_unsupported_shapes():
    """Argument validation of csrc/interest.hip at the first shape past each limit: nothing is launched (the pointers are
    never dereferenced), and the support queries agree with the checks."""
    import ctypes

    from torch_rechub_amd import _lib
    f, n = ctypes.c_void_p(4096), ctypes.c_void_p(0)

    def caps_fwd(L, I, D, kind):
        return _lib.call("rh_capsule_fwd", f, f, f, f, n, 4, L, I, D, kind, 3, f, f, f, n)

    def caps_bwd(L, I, D, kind):
        return _lib.call("rh_capsule_bwd", f, f, f, f, 4, L, I, D, kind, f, f, f, n)

    for call in (caps_fwd, caps_bwd):
        with pytest.raises(RuntimeError, match="no HIP kernel|unsupported"):
            call(8, 1, 65, 0)                      # D = 65
        with pytest.raises(RuntimeError, match="no HIP kernel|unsupported"):
            call(8, 257, 1, 1)                     # I*D = 257
        with pytest.raises(RuntimeError, match="no HIP kernel|unsupported"):
            call(8, 5, 29, 2)                      # type 2: I*D*D = 4205 > 4096 (I*D = 145)
        with pytest.raises(RuntimeError, match="no HIP kernel|unsupported"):
            call(8, 17, 16, 2)                     # I*D = 272
        for I, D, kind in ((16, 16, 0), (1, 64, 2), (4, 32, 2), (4, 1, 1)):
            L = 1
            while _lib.call("rh_capsule_supported", 2 * L, I, D, kind):
                L *= 2
            lo, hi = L, 2 * L                      # supported(lo), not supported(hi)
            while hi - lo > 1:
                mid = (lo + hi) // 2
                lo, hi = (mid, hi) if _lib.call("rh_capsule_supported", mid, I, D, kind) else (lo, mid)
            with pytest.raises(RuntimeError, match="no HIP kernel|unsupported"):
                call(hi, I, D, kind)               # one position past the LDS limit
    assert _lib.call("rh_capsule_supported", 8, 1, 64, 2) == 1 and _lib.call("rh_capsule_supported", 8, 4, 32, 2) == 1
    assert _lib.call("rh_capsule_supported", 8, 5, 29, 2) == 0 and _lib.call("rh_capsule_supported", 8, 4, 33, 2) == 0
    with pytest.raises(RuntimeError, match="unsupported"):
        _lib.call("rh_capsule_wgrad", f, f, f, 4, 8, 4, 33, f, n)   # I*D*D = 4356
    with pytest.raises(RuntimeError, match="unsupported"):
        _lib.call("rh_capsule_wgrad", f, f, f, 4, 8, 1, 65, f, n)
    with pytest.raises(RuntimeError, match="unsupported"):
        _lib.call("rh_capsule_wgrad", f, f, f, 0, 8, 4, 16, f, n)   # nothing to sum: the caller zeroes instead
    for L, I, D in ((1025, 1, 1), (257, 4, 16), (1, 1, 65), (4, 1025, 1), (2, 17, 61)):
        assert not _lib.call("rh_sa_supported", L, I, D)
        with pytest.raises(RuntimeError, match="no HIP kernel"):
            _lib.call("rh_sa_pool_fwd", f, f, f, 4, L, I, D, f, f, n)
        with pytest.raises(RuntimeError, match="unsupported"):
            _lib.call("rh_sa_pool_bwd", f, f, f, 4, L, I, D, f, f, n)
    assert _lib.call("rh_sa_supported", 1024, 1, 64) and _lib.call("rh_sa_supported", 64, 16, 64)
    for I, D, K in ((17, 16, 3), (4, 65, 3), (4, 16, 1024)):
        with pytest.raises(RuntimeError, match="no HIP kernel"):
            _lib.call("rh_listwise_fwd", f, f, D, f, 4, I, D, K, 1.0, f, f, f, n)
        with pytest.raises(RuntimeError, match="unsupported"):
            _lib.call("rh_listwise_bwd", f, f, D, f, f, f, f, 4, I, D, K, 1.0, f, f, f, n)
    with pytest.raises(RuntimeError, match="bad arguments"):  # a row stride below D
        _lib.call("rh_listwise_fwd", f, f, 15, f, 4, 4, 16, 3, 1.0, f, f, f, n)
