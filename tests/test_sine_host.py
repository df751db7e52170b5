"""SINE without a GPU: the public name, the reference's constructor / state_dict layout, and a float64 numpy restatement
of the sparse-interest chain (forward and hand-derived backward, the math csrc/sine.hip implements) checked against the
fixtures of tools/gen_golden_sine.py and against torch autograd of the reference's lines in float64.

The masked softmaxes follow the reference's float32 arithmetic, not its formula read in float64: ``a + -1e9 (1 - mask)``
is exactly -1e9 at a dropped position in float32 (|a| is far below half an ulp of 1e9), so a fully padded row comes out
uniform.  The restatement writes -1e9 there; evaluated literally in float64 the formula would keep ``a`` in such a row.

sine.py:122 calls ``F.normalize(m, -1)``: the second positional argument of F.normalize is the ORDER of the norm, so the
adapted intention is divided by its p = -1 "norm" 1 / sum_e 1 / |m_e| (over the last axis, the default one of a (B, E)
tensor), not by its length.  The restatement, the kernels and the fixtures all follow the reference there."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import golden_state, load_golden

EPS = 1e-12
# (a module's own parameters come before its submodules' in a state_dict: the matrices, then the three tables)
MODEL_KEYS = ["w_1", "w_2", "w_3", "w_k1", "w_k2", "w_4", "w_5", "item_embedding.weight", "concept_embedding.weight",
              "position_embedding.weight"]


def build_sine(gold, **kw):
    """Same constructor call as tools/gen_golden_sine.py::build, on the torch_rechub_amd class."""
    from torch_rechub_amd.models.matching import SINE
    c = {k[4:]: int(gold[k]) for k in gold.files if k.startswith("cfg.")}
    kw.setdefault("temperature", float(gold["temperature"]))
    return SINE(["hist_item_id"], ["item_id"], ["neg_items"], c["num_items"], c["embedding_dim"], c["hidden_dim"],
                c["num_concept"], c["num_intention"], c["seq_max_len"], **kw)


# ---- float64 restatement ------------------------------------------------------------------------------------------------
def _softmax(x, axis):
    e = np.exp(x - x.max(axis=axis, keepdims=True))
    return e / e.sum(axis=axis, keepdims=True)


def masked_softmax(a, mask):
    """softmax over axis 1 of a (B, S) or (B, S, K) with dropped positions at -1e9 (see the module docstring)."""
    keep = mask.astype(bool)
    if a.ndim == 3:
        keep = keep[:, :, None]
    return _softmax(np.where(keep, a, -1.e9), 1)


def _softmax_bwd(p, g, axis):
    return p * (g - (p * g).sum(axis=axis, keepdims=True))


def _normalize(v):
    n = np.sqrt((v * v).sum(-1))
    return v / np.maximum(n, EPS)[..., None], n


def _normalize_bwd(vh, n, g):
    dot = (vh * g).sum(-1) * (n > EPS)  # the clamped norm is a constant
    return (g - vh * dot[..., None]) / np.maximum(n, EPS)[..., None]


def top_k_gap(s_u, K):
    """Per row: the smallest gap between adjacent scores among the top K + 1, relative to the row's max |s_u|."""
    top = -np.sort(-s_u, axis=1)[:, :K + 1]
    if top.shape[1] < 2:
        return np.full(s_u.shape[0], np.inf)
    return (top[:, :-1] - top[:, 1:]).min(1) / np.abs(s_u).max(1)


def np_sine_interests(X, Y, a1, a2, mask, C):
    """(phi (B, K, E), xhat (B, S, E), idx (B, K) int32, cache) of sine.py:94-118."""
    K = a2.shape[2]
    P1 = masked_softmax(a1, mask)
    z = np.einsum("bs,bse->be", P1, X)
    s_u = z @ C.T
    idx = np.argsort(-s_u, axis=1, kind="stable")[:, :K]  # descending, ties to the lower index
    gate = 1 / (1 + np.exp(-np.take_along_axis(s_u, idx, 1)))
    Csel = C[idx]
    cu = gate[..., None] * Csel
    yh, ny = _normalize(Y)
    ch, nc = _normalize(cu)
    pu = _softmax(np.einsum("bse,bke->bks", yh, ch), 1)
    P2 = masked_softmax(a2, mask)
    w = pu * P2.transpose(0, 2, 1)
    phi = np.einsum("bks,bse->bke", w, X)
    xhat = np.einsum("bks,bke->bse", pu, cu)
    cache = dict(P1=P1, z_u=z, s_u=s_u, idx=idx, gate=gate, Csel=Csel, c_u=cu, yh=yh, ny=ny, ch=ch, nc=nc, p_u=pu, P2=P2, w=w)
    return phi, xhat, idx.astype(np.int32), cache


def np_sine_interests_bwd(X, C, c, g_phi, g_xhat):
    """(g_X, g_Y, g_a1, g_a2, g_C): the top-k passes gradient to the chosen scores only."""
    pu, P2, P1 = c["p_u"], c["P2"], c["P1"]
    g_w = np.einsum("bke,bse->bks", g_phi, X)
    g_X = np.einsum("bks,bke->bse", c["w"], g_phi)
    g_pu = g_w * P2.transpose(0, 2, 1) + np.einsum("bse,bke->bks", g_xhat, c["c_u"])
    g_a2 = _softmax_bwd(P2, (g_w * pu).transpose(0, 2, 1), 1)
    g_d = _softmax_bwd(pu, g_pu, 1)
    g_Y = _normalize_bwd(c["yh"], c["ny"], np.einsum("bks,bke->bse", g_d, c["ch"]))
    g_cu = np.einsum("bks,bse->bke", pu, g_xhat) + _normalize_bwd(c["ch"], c["nc"], np.einsum("bks,bse->bke", g_d, c["yh"]))
    gate = c["gate"]
    g_st = (g_cu * c["Csel"]).sum(-1) * gate * (1 - gate)
    g_z = np.einsum("bk,bke->be", g_st, c["Csel"])
    g_C = np.zeros_like(C)
    np.add.at(g_C, c["idx"], gate[..., None] * g_cu + g_st[..., None] * c["z_u"][:, None, :])
    g_X = g_X + P1[..., None] * g_z[:, None, :]
    g_a1 = _softmax_bwd(P1, np.einsum("be,bse->bs", g_z, X), 1)
    return g_X, g_Y, g_a1, g_a2, g_C


def np_sine_aggregate(xhat, a3, mask, phi, temperature):
    """(v (B, E), cache) of sine.py:122-128."""
    P3 = masked_softmax(a3, mask)
    m = np.einsum("bs,bse->be", P3, xhat)
    with np.errstate(divide="ignore"):
        n = 1 / (1 / np.abs(m)).sum(-1)  # the p = -1 "norm" of F.normalize(m, -1)
    c_apt = m / np.maximum(n, EPS)[:, None]
    e = _softmax(np.einsum("be,bke->bk", c_apt, phi) / temperature, 1)
    return np.einsum("bk,bke->be", e, phi), dict(P3=P3, m=m, n=n, c_apt=c_apt, e_u=e)


def np_sine_aggregate_bwd(xhat, phi, c, g_v, temperature):
    """(g_xhat, g_a3, g_phi): g_phi arrives through e and directly."""
    e, m, n, c_apt, P3 = c["e_u"], c["m"], c["n"], c["c_apt"], c["P3"]
    # softmax backward over k as e_k sum_j e_j (g_e[k] - g_e[j]): the usual e_k (g_e[k] - sum_j e_j g_e[j]) cancels to
    # rounding noise, float64's included, once the logits of hundreds have saturated e
    g_e = np.einsum("be,bke->bk", g_v, phi)
    g_l = e * (e[:, None, :] * (g_e[:, :, None] - g_e[:, None, :])).sum(-1) / temperature
    g_phi = e[..., None] * g_v[:, None, :] + g_l[..., None] * c_apt[:, None, :]
    g_c = np.einsum("bk,bke->be", g_l, phi)
    dc = (g_c * c_apt).sum(-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        through_norm = np.where((n > EPS)[:, None], dc * n[:, None] / (m * np.abs(m)), 0.0)
    g_m = g_c / np.maximum(n, EPS)[:, None] - through_norm
    g_a3 = _softmax_bwd(P3, np.einsum("be,bse->bs", g_m, xhat), 1)
    return P3[..., None] * g_m[:, None, :], g_a3, g_phi


# ---- torch autograd of the reference's lines ---------------------------------------------------------------------------
def torch_chain(X, Y, a1, a2, mask, C, a3, temperature):
    """sine.py:94-128 on given leaves (float64 tensors); a3 is a leaf too (the w_4 / w_5 product sits between the halves
    and is not part of the fused chain).  Returns (phi, xhat, v, top-k indices)."""
    mf = mask.to(X.dtype)
    a_hist = F.softmax(a1 + -1.e9 * (1 - mf), dim=1)
    z_u = torch.einsum("bse, bs -> be", X, a_hist)
    s_u = torch.einsum("be, te -> bt", z_u, C)
    top = torch.topk(s_u, a2.shape[2])
    c_u = torch.einsum("bk, bke -> bke", torch.sigmoid(top.values), C[top.indices])
    p_u = F.softmax(torch.einsum("bse, bke -> bks", F.normalize(Y, dim=-1), F.normalize(c_u, p=2, dim=-1)), dim=1)
    a_concept_k = F.softmax(a2 + -1.e9 * (1 - mf.unsqueeze(-1)), dim=1)
    phi_u = torch.einsum("bks, bse -> bke", p_u * a_concept_k.permute(0, 2, 1), X)
    x_u_hat = torch.einsum("bks, bke -> bse", p_u, c_u)
    c_u_apt = F.normalize(torch.einsum("bs, bse -> be", F.softmax(a3 + -1.e9 * (1 - mf), dim=1), x_u_hat), -1)
    e_u = F.softmax(torch.einsum("be, bke -> bk", c_u_apt, phi_u) / temperature, dim=1)
    return phi_u, x_u_hat, torch.einsum("bk, bke -> be", e_u, phi_u), top.indices


def draw_inputs(B, S, E, T, K, seed, holes=False):
    """The recipe of the kernel tests: X = 0.5 randn, Y = X w_3 with w_3 = rand / sqrt(E), a1 / a2 / a3 = 3 randn,
    C = randn, left-padded masks of arbitrary length with row 0 fully padded and row 1 full (``holes``: dropped positions
    inside the kept run as well).  float32 tensors."""
    g = torch.Generator().manual_seed(seed)
    X = 0.5 * torch.randn(B, S, E, generator=g)
    Y = X @ (torch.rand(E, E, generator=g) / E ** 0.5)
    a1, a2, a3 = (3 * torch.randn(*shape, generator=g) for shape in ((B, S), (B, S, K), (B, S)))
    C = torch.randn(T, E, generator=g)
    lens = torch.randint(1, S + 1, (B,), generator=g)
    lens[0] = 0
    if B > 1:
        lens[1] = S
    mask = (torch.arange(S)[None, :] >= (S - lens)[:, None]).to(torch.int32)
    if holes:
        mask = mask * (torch.rand(B, S, generator=g) < 0.7).to(torch.int32)
        if B > 1:
            mask[1] = 1
    g_v = torch.randn(B, E, generator=g)
    return dict(X=X, Y=Y, a1=a1, a2=a2, a3=a3, C=C, mask=mask, g_v=g_v)


def oracle(inp, temperature, keep_rows=None):
    """The whole float64 chain of ``draw_inputs``' tensors: values, caches and every gradient for g_v (rows outside
    ``keep_rows`` with a zeroed upstream gradient)."""
    d = {k: v.double().numpy() for k, v in inp.items() if k != "mask"}
    mask = inp["mask"].numpy()
    phi, xhat, idx, c1 = np_sine_interests(d["X"], d["Y"], d["a1"], d["a2"], mask, d["C"])
    v, c2 = np_sine_aggregate(xhat, d["a3"], mask, phi, temperature)
    g_v = d["g_v"] if keep_rows is None else d["g_v"] * keep_rows[:, None]
    g_xhat2, g_a3, g_phi = np_sine_aggregate_bwd(xhat, phi, c2, g_v, temperature)
    g_X, g_Y, g_a1, g_a2, g_C = np_sine_interests_bwd(d["X"], d["C"], c1, g_phi, g_xhat2)
    return dict(phi=phi, xhat=xhat, idx=idx, v=v, s_u=c1["s_u"], g_xhat=g_xhat2, g_a3=g_a3, g_phi=g_phi, g_X=g_X, g_Y=g_Y,
                g_a1=g_a1, g_a2=g_a2, g_C=g_C, cache=(c1, c2))


# ---- the restatement against the reference's fixture -----------------------------------------------------------------------
def _close(got, want, what, rtol=1e-4):
    np.testing.assert_allclose(got, want, rtol=rtol, atol=1e-5 * float(np.abs(want).max()), err_msg=what)


def test_restatement_matches_the_reference_fixture():
    gold = load_golden("sine_layers.npz")
    f = {k: gold[k].astype(np.float64) for k in gold.files if gold[k].dtype == np.float32}
    mask, temperature = gold["mask"], float(gold["temperature"])
    assert not mask[0].any() and mask[1].all() and not mask[2, 3] and mask[2, 2] and mask[2, 4]  # padded, full, a hole
    assert float(top_k_gap(f["s_u"], gold["idx"].shape[1]).min()) >= 1e-3
    phi, xhat, idx, c1 = np_sine_interests(f["X"], f["Y"], f["a1"], f["a2"], mask, f["C"])
    np.testing.assert_array_equal(idx, gold["idx"])
    for name, got in (("P1", c1["P1"]), ("z_u", c1["z_u"]), ("s_u", c1["s_u"]), ("c_u", c1["c_u"]), ("p_u", c1["p_u"]),
                      ("P2", c1["P2"]), ("phi", phi), ("xhat", xhat)):
        _close(got, f[name], name)
    np.testing.assert_allclose(c1["P1"][0], 1 / mask.shape[1], rtol=1e-6)  # the fully padded row: uniform
    # (the second half from the fixture's own xhat / phi, so that its comparison does not inherit the first half's rounding)
    v, c2 = np_sine_aggregate(f["xhat"], f["a3"], mask, f["phi"], temperature)
    for name, got in (("P3", c2["P3"]), ("c_apt", c2["c_apt"]), ("e_u", c2["e_u"]), ("v", v)):
        _close(got, f[name], name)
    g_xhat, g_a3, g_phi = np_sine_aggregate_bwd(f["xhat"], f["phi"], c2, f["g_v"], temperature)
    _close(g_phi, f["g_phi"], "g_phi")
    # g_xhat and g_a3 pass through the p = -1 norm n ~ min_e |m_e| (here 3e-4 .. 7e-4 against |m| ~ 0.1) and logits of
    # 60 .. 410: the reference's own float32 values are 2 % of the largest magnitude from float64 in the one row of this
    # fixture whose softmax over k is not saturated.  They are held to 5 % here; what pins these two gradients exactly is
    # float64 autograd of the reference's lines on the same inputs, to 1e-8.
    for name, got in (("g_xhat", g_xhat), ("g_a3", g_a3)):
        np.testing.assert_allclose(got, f[name], rtol=0, atol=0.05 * float(np.abs(f[name]).max()), err_msg=name)
    t = {k: torch.from_numpy(f[k]).requires_grad_(True) for k in ("xhat", "a3", "phi")}
    mf = torch.from_numpy(mask).double()
    P3 = F.softmax(torch.where(mf > 0, t["a3"], torch.full_like(t["a3"], -1.e9)), dim=1)
    c_apt = F.normalize(torch.einsum("bs, bse -> be", P3, t["xhat"]), -1)
    e_u = F.softmax(torch.einsum("be, bke -> bk", c_apt, t["phi"]) / temperature, dim=1)
    torch.einsum("bk, bke -> be", e_u, t["phi"]).backward(torch.from_numpy(f["g_v"]))
    for name, got in (("xhat", g_xhat), ("a3", g_a3), ("phi", g_phi)):
        want = t[name].grad.numpy()
        np.testing.assert_allclose(got, want, rtol=1e-8, atol=1e-9 * float(np.abs(want).max()), err_msg="g_" + name)
    grads = np_sine_interests_bwd(f["X"], f["C"], c1, f["up_g_phi"], f["up_g_xhat"])  # (upstream drawn for this half)
    for name, got in zip(("g_X", "g_Y", "g_a1", "g_a2", "g_C"), grads):
        _close(got, f[name], name)


@pytest.mark.parametrize("B,S,E,T,K,holes", [(9, 7, 20, 5, 4, False), (5, 1, 8, 3, 1, False), (12, 11, 6, 9, 3, True)])
def test_restatement_matches_torch_autograd_in_float64(B, S, E, T, K, holes):
    inp = draw_inputs(B, S, E, T, K, seed=B + S, holes=holes)
    inp["mask"][inp["mask"].sum(1) == 0, -1] = 1  # (the literal float64 formula is not uniform on a fully padded row)
    temperature = 0.7
    t = {k: v.double().requires_grad_(True) for k, v in inp.items() if k not in ("mask", "g_v")}
    phi, xhat, v, top = torch_chain(t["X"], t["Y"], t["a1"], t["a2"], inp["mask"], t["C"], t["a3"], temperature)
    v.backward(inp["g_v"].double())
    o = oracle(inp, temperature)
    np.testing.assert_array_equal(o["idx"], top.numpy())
    for name, got, want in (("phi", o["phi"], phi), ("xhat", o["xhat"], xhat), ("v", o["v"], v)):
        np.testing.assert_allclose(got, want.detach().numpy(), rtol=1e-9, atol=1e-12, err_msg=name)
    for name in ("X", "Y", "a1", "a2", "a3", "C"):
        want = t[name].grad.numpy()
        np.testing.assert_allclose(o["g_" + name], want, rtol=1e-8, atol=1e-11 * max(1.0, float(np.abs(want).max())),
                                   err_msg="g_" + name)


def test_top_k_takes_the_lower_index_on_ties_like_torch():
    X = np.ones((1, 2, 3))
    C = np.array([[1.0, 0, 0], [2.0, 0, 0], [2.0, 0, 0], [0.5, 0, 0]])
    _, _, idx, _ = np_sine_interests(X, X, np.zeros((1, 2)), np.zeros((1, 2, 3)), np.ones((1, 2), np.int32), C)
    assert idx.tolist() == [[1, 2, 0]]


def test_shape_cases_exclude_at_most_two_percent_of_their_rows():
    """The cases of test_gpu_sine_rq_topk_shapes.py: the rows left out of the comparison (a top-k gap below 1e-4) follow
    from the inputs and the oracle alone, and every value of the oracle is finite at these limits."""
    from retrieval_shape_cases import (MAX_EXCLUDED, MIN_GAP, SINE_AGG_ONLY_CASE, SINE_CASES, SINE_TEMPERATURE,
                                       SINE_WARM_TEMPERATURE)
    assert any(S * E % 4 for _, S, E, _, _, _, _ in SINE_CASES) and any(K == T > 1 for _, _, _, T, K, _, _ in SINE_CASES)
    assert {1, 64, 65} <= {E for _, _, E, _, _, _, _ in SINE_CASES} and SINE_AGG_ONLY_CASE[0] > 16384 * 4
    for B, S, E, T, K, seed, holes in SINE_CASES + [SINE_AGG_ONLY_CASE]:
        inp = draw_inputs(B, S, E, T, K, seed, holes)
        assert not inp["mask"][0].any()
        s_u = oracle(inp, SINE_TEMPERATURE)["s_u"]
        keep = top_k_gap(s_u, K) >= MIN_GAP
        excluded = int((~keep).sum())
        print(f"({B}, {S}, {E}, {T}, {K}, {seed}, {holes}): {excluded} of {B} rows excluded")
        assert excluded <= MAX_EXCLUDED * B, (B, S, E, T, K, seed, excluded)
        for temperature in (SINE_TEMPERATURE, SINE_WARM_TEMPERATURE):
            o = oracle(inp, temperature, keep_rows=keep)
            for name, v in o.items():
                assert name == "cache" or np.isfinite(v).all(), (B, S, E, T, K, seed, temperature, name)


# ---- the model ------------------------------------------------------------------------------------------------------------
def test_sine_is_exported_with_the_reference_layout():
    from torch_rechub_amd.models import matching
    assert "SINE" in matching.__all__
    gold = load_golden("model_sine.npz")
    model = build_sine(gold)
    sd0 = golden_state(gold, "sd0.")
    assert list(model.state_dict()) == list(sd0) == MODEL_KEYS
    for k, v in model.state_dict().items():
        assert tuple(v.shape) == tuple(sd0[k].shape), k
    model.load_state_dict(sd0)
    assert model.mode is None and model.temperature == float(gold["temperature"])
    assert (model.num_concept, model.num_intention, model.seq_max_len) == (10, 3, 8)
    assert model.item_embedding.padding_idx is None  # row 0 is an item row like any other
    assert all(getattr(model, n)._rh_dense for n in ("item_embedding", "concept_embedding", "position_embedding"))


def test_sine_initial_draws_follow_the_reference_recipe():
    gold = load_golden("model_sine.npz")
    torch.manual_seed(3)
    model = build_sine(gold)
    for name in ("item_embedding", "concept_embedding", "position_embedding"):
        w = getattr(model, name).weight
        assert 0.5e-4 < float(w.detach().std()) < 2e-4 and abs(float(w.detach().mean())) < 1e-4  # normal, std 1e-4
    for name in ("w_1", "w_2", "w_3", "w_k1", "w_k2", "w_4", "w_5"):
        w = getattr(model, name)
        assert w.requires_grad and 0 <= float(w.detach().min()) and float(w.detach().max()) < 1  # torch.rand
    torch.manual_seed(3)  # the same sequence of draws: tables first, then the matrices in the reference's order
    item = torch.nn.init.normal_(torch.nn.Embedding(60, 16).weight, 0, 1e-4)  # (nn.Embedding draws once itself)
    assert torch.equal(model.item_embedding.weight.detach(), item.detach())


def test_sine_rejects_more_than_one_head_in_forward():
    gold = load_golden("model_sine.npz")
    model = build_sine(gold, num_heads=2)  # the constructor accepts it and shapes w_2 / w_5 with it
    assert tuple(model.w_2.shape) == (12, 2) and tuple(model.w_5.shape) == (12, 2)
    with pytest.raises(ValueError, match="num_heads"):
        model({"hist_item_id": torch.zeros(2, 8, dtype=torch.long)})


def test_sine_supported_bounds():
    from torch_rechub_amd import ops
    assert ops.sine_supported(50, 128, 10, 2) and ops.sine_supported(64, 128, 64, 8) and ops.sine_supported(1, 1, 1, 1)
    assert ops.sine_supported(7, 20, 5, 4)  # E need not be a multiple of 4, nor S of the wavefront
    for S, E, T, K in ((65, 128, 10, 2), (50, 129, 10, 2), (50, 128, 65, 2), (50, 128, 10, 9), (50, 128, 3, 4),
                       (0, 128, 10, 2), (50, 0, 10, 2), (50, 128, 10, 0)):
        assert not ops.sine_supported(S, E, T, K), (S, E, T, K)


def test_sine_ops_refuse_cpu_tensors():
    from torch_rechub_amd import ops
    inp = draw_inputs(4, 5, 8, 6, 2, seed=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sine_interests(inp["X"], inp["Y"], inp["a1"], inp["a2"], inp["mask"], inp["C"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.sine_aggregate(inp["X"], inp["a3"], inp["mask"], torch.zeros(4, 2, 8), 0.1)
