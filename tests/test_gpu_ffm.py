"""DeepFFM / FatDeepFFM on the MI355X: the field-aware FFM / CEN kernels of csrc/ffm.hip against float32 / float64 numpy,
the models against the reference's fixtures (tools/gen_golden_ffm.py), the layer path a patched reference model takes,
the captured step and lazy Adam bit for bit against their eager / dense twins, and the one-rank data-parallel step."""
import numpy as np
import pytest
import torch

from conftest import assert_state_follows_reference_trajectory, golden_batch, golden_state, load_golden
from test_ffm_host import FFM_MODELS, build_ffm_model

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def to_dev(x):
    return {k: v.to(dev()) for k, v in x.items()}


def pairs(F):
    return [(i, j) for i in range(F - 1) for j in range(i + 1, F)]


def make_tables(F, D, Dp, vocabs, g):
    ws = []
    for v in vocabs:
        w = torch.zeros(v * F, Dp)
        w[:, :D] = torch.randn(v * F, D, generator=g)
        ws.append(w.to(dev()).requires_grad_(True))
    return ws


def np_em(ws, idx, F, D):
    T = [w.detach().cpu().numpy() for w in ws]
    X = [t.cpu().numpy().astype(np.int64) for t in idx]
    return np.stack([T[i][X[i] * F + j, :D] * T[j][X[j] * F + i, :D] for i, j in pairs(F)], 1)  # float32 products


def np_table_grads(ws, idx, F, D, g_em, pads, dtype):
    T = [w.detach().cpu().numpy().astype(dtype) for w in ws]
    X = [t.cpu().numpy().astype(np.int64) for t in idx]
    G = [np.zeros_like(t) for t in T]
    g = g_em.astype(dtype)
    for p, (i, j) in enumerate(pairs(F)):
        ra, rc = X[i] * F + j, X[j] * F + i
        ga, gc = g[:, p] * T[j][rc, :D], g[:, p] * T[i][ra, :D]
        for b in range(len(ra)):
            if ra[b] != pads[i]:
                G[i][ra[b], :D] += ga[b]
            if rc[b] != pads[j]:
                G[j][rc[b], :D] += gc[b]
    return G


def ffm_call(ws, idx, D, pads=None):
    from torch_rechub_amd import ops
    return ops.FfmCall(ws, pads or [None] * len(ws), idx, D)


# ---- kernels ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [2, 6, 26])
@pytest.mark.parametrize("D,Dp", [(4, 4), (10, 16), (16, 16), (128, 128)])
@pytest.mark.parametrize("itype", [torch.int64, torch.int32])
def test_fused_forward_bit_equal_and_collision_free_table_grads_bit_equal(F, D, Dp, itype):
    from torch_rechub_amd import ops
    g = torch.Generator().manual_seed(F * 1000 + D)
    B = 64
    vocabs = [B + 3 + 5 * f for f in range(F)]
    ws = make_tables(F, D, Dp, vocabs, g)
    idx = [torch.randperm(v, generator=g)[:B].to(itype).to(dev()) for v in vocabs]  # collision-free per field
    em = ops.ffm_fused(ffm_call(ws, idx, D))
    P = F * (F - 1) // 2
    assert em.shape == (B, P * D)
    want = np_em(ws, idx, F, D)
    np.testing.assert_array_equal(em.detach().cpu().numpy().reshape(B, P, D), want)
    g_em = torch.randn(B, P * D, generator=g)
    em.backward(g_em.to(dev()))
    torch.cuda.synchronize()
    ops.check_errors()
    G = np_table_grads(ws, idx, F, D, g_em.numpy().reshape(B, P, D), [-1] * F, np.float32)
    for f, w in enumerate(ws):
        got = w.grad.cpu().numpy()
        np.testing.assert_array_equal(got, G[f], err_msg=f"field {f}")  # one contribution per row: exact products
        assert not got[:, D:].any()  # PaddedEmbedding's padding columns stay exactly zero


def test_fused_grads_with_duplicates_and_padding_idx():
    from torch_rechub_amd import ops
    g = torch.Generator().manual_seed(3)
    F, D, Dp, B = 5, 10, 16, 200
    vocabs = [3, 7, 11, 4, 9]
    ws = make_tables(F, D, Dp, vocabs, g)
    pads = [0, None, 2 * F + 1, None, None]  # row 0 of field 0 and row x = 2, j = 1 of field 2 are padding rows
    idx = [torch.randint(0, v, (B,), generator=g).to(dev()) for v in vocabs]
    em = ops.ffm_fused(ffm_call(ws, idx, D, pads))
    np.testing.assert_array_equal(em.detach().cpu().numpy().reshape(B, -1, D), np_em(ws, idx, F, D))
    g_em = torch.randn(em.shape, generator=g)
    em.backward(g_em.to(dev()))
    torch.cuda.synchronize()
    ops.check_errors()
    G = np_table_grads(ws, idx, F, D, g_em.numpy().reshape(B, -1, D), [-1 if p is None else p for p in pads], np.float64)
    for f, w in enumerate(ws):
        got = w.grad.cpu().numpy()
        np.testing.assert_allclose(got, G[f], rtol=1e-5, atol=1e-5, err_msg=f"field {f}")
        assert not got[:, D:].any()
    assert not ws[0].grad[0].any() and not ws[2].grad[2 * F + 1].any()


def test_fused_out_of_range_index_sets_the_error_flag():
    from torch_rechub_amd import ops
    g = torch.Generator().manual_seed(4)
    ws = make_tables(3, 4, 4, [5, 5, 5], g)
    idx = [torch.tensor([0, 1], device=dev()), torch.tensor([5, 1], device=dev()), torch.tensor([2, 3], device=dev())]
    ops.ffm_fused(ffm_call(ws, idx, 4))
    torch.cuda.synchronize()
    with pytest.raises(IndexError):
        ops.check_errors()


def test_unsupported_shapes_are_rejected():
    from torch_rechub_amd import ops
    g = torch.Generator().manual_seed(5)
    ws = make_tables(65, 4, 4, [2] * 65, g)
    idx = [torch.zeros(4, dtype=torch.long, device=dev()) for _ in ws]
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ffm_call(ws, idx, 4)
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ffm_call(make_tables(2, 4, 4, [2, 2], g), idx[:2], 8)
    with pytest.raises(RuntimeError, match="num_fields 1 unsupported"):
        ops.ffm(torch.zeros(4, 1, 1, 4, device=dev()), False)
    with pytest.raises(RuntimeError, match="embed_dim 129 unsupported"):
        ops.ffm(torch.zeros(4, 2, 2, 129, device=dev()), False)


@pytest.mark.parametrize("rs", [0, 1])
def test_layer_ffm_against_fixture(rs):
    from torch_rechub_amd.basic.layers import FFM
    gold = load_golden("ffm_layers.npz")
    x = torch.from_numpy(gold[f"ffm_rs{rs}.x"]).to(dev()).requires_grad_(True)
    y = FFM(x.shape[1], reduce_sum=bool(rs))(x)
    if rs:
        np.testing.assert_allclose(y.detach().cpu().numpy(), gold["ffm_rs1.out"], rtol=1e-5, atol=1e-6)
    else:  # one product per element: bit-equal to the reference's slice products
        np.testing.assert_array_equal(y.detach().cpu().numpy(), gold["ffm_rs0.out"])
    y.backward(torch.from_numpy(gold[f"ffm_rs{rs}.g_out"]).to(dev()))
    np.testing.assert_array_equal(x.grad.cpu().numpy(), gold[f"ffm_rs{rs}.g_x"])


def test_cen_against_fixture_and_u_gradient_bit_identical():
    from torch_rechub_amd.basic.layers import CEN
    gold = load_golden("ffm_layers.npz")
    em0 = torch.from_numpy(gold["cen.em"]).to(dev())
    B, P, D = em0.shape
    sd = {k[len("cen.sd."):]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("cen.sd.")}
    grads = []
    for _ in range(2):
        cen = CEN(D, P, 3).to(dev())
        cen.load_state_dict(sd)
        em = em0.clone().requires_grad_(True)
        y = cen(em)
        np.testing.assert_allclose(y.detach().cpu().numpy(), gold["cen.out"], rtol=1e-5, atol=1e-5)
        y.backward(torch.from_numpy(gold["cen.g_out"]).to(dev()))
        np.testing.assert_allclose(em.grad.cpu().numpy(), gold["cen.g_em"], rtol=1e-4, atol=1e-5)
        for n, p in cen.named_parameters():
            ref = gold["cen.grad." + n]
            if n in ("mlp_att.mlp.0.bias", "mlp_att.mlp.4.bias"):  # a Linear bias in front of BatchNorm: rounding noise
                assert np.abs(p.grad.cpu().numpy()).max() < 1e-4 and np.abs(ref).max() < 1e-4, n
                continue
            np.testing.assert_allclose(p.grad.cpu().numpy(), ref, rtol=1e-4, atol=1e-5 * max(1.0, np.abs(ref).max()), err_msg=n)
        grads.append(cen.u.grad.clone())
    assert torch.equal(grads[0], grads[1])


# ---- models against the reference ------------------------------------------------------------------------------------
def load_model(cfg, cls=None):
    gold = load_golden(f"model_{cfg}.npz")
    model = build_ffm_model(cfg, gold) if cls is None else cls_model(cls, cfg, gold)
    model.load_state_dict(golden_state(gold, "sd0."))
    return gold, model.to(dev())


@pytest.mark.parametrize("cfg", FFM_MODELS)
def test_forward_loss_and_gradients_match_reference(cfg):
    from torch_rechub_amd import ops
    gold, model = load_model(cfg)
    x, y = golden_batch(gold, 0)
    xd, yd = to_dev(x), y.to(dev()).float()
    model.eval()
    with torch.no_grad():
        np.testing.assert_allclose(model(xd).cpu().numpy(), gold["pred_eval"], rtol=1e-5, atol=2e-6)
    model.train()
    pred = model(xd)
    np.testing.assert_allclose(pred.detach().cpu().numpy(), gold["pred_train"], rtol=1e-5, atol=2e-6)
    loss = torch.nn.BCELoss()(pred, yd)
    assert abs(loss.item() - float(gold["loss"])) < 2e-6
    loss.backward()
    ops.check_errors()
    gmax = max(float(np.abs(gold["grad." + n]).max()) for n, _ in model.named_parameters())
    for n, p in model.named_parameters():
        ref = gold["grad." + n]
        got = p.grad.detach().cpu().numpy() if p.grad is not None else np.zeros_like(ref)
        if got.shape != ref.shape:  # PaddedEmbedding: the logical columns (the padding's gradient must be zero)
            assert not got[:, ref.shape[1]:].any(), n
            got = got[:, :ref.shape[1]]
        if n.endswith(".bias") and "mlp" in n and np.abs(ref).max() < 1e-5 * max(gmax, 1e-3):
            continue  # a Linear bias in front of BatchNorm: rounding noise on both sides
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=2e-6 * gmax, err_msg=f"{cfg}: grad of {n}")


@pytest.mark.parametrize("mode", ["dense", "lazy"])
@pytest.mark.parametrize("cfg", FFM_MODELS)
def test_three_step_training_matches_reference_trainer(cfg, mode):
    from torch_rechub_amd.trainers import CTRTrainer
    gold, model = load_model(cfg)
    batches = [golden_batch(gold, i) for i in range(3)]
    params = {"lr": float(gold["train.lr"]), "weight_decay": float(gold["train.wd"])}
    if mode == "lazy":
        params["lazy_small_rows"] = 8
    trainer = CTRTrainer(model, optimizer_params=params, n_epoch=1, device="cuda:0", show_progress=False,
                         table_update=mode, lazy_k=2)
    mean_loss = trainer.train_one_epoch(batches)
    assert abs(mean_loss - float(gold["train.mean_loss"])) < 5e-5
    assert_state_follows_reference_trajectory(gold, model.state_dict(), cfg)


# ---- the layer path of a patched reference model ----------------------------------------------------------------------
def reference_forward(self, x):
    """The reference's DeepFFM / FatDeepFFM forward (deepffm.py:47-65 / :112-134) restated on the HIP layers: (B, K) lookup
    of x * F + fields_offset -> FFM (-> CEN) -> MLP."""
    y_linear = self.linear_embedding(x, self.linear_features, squeeze_dim=True).sum(1, keepdim=True)
    x_ffm = {fea.name: x[fea.name].unsqueeze(1) * self.num_fields + self.fields_offset for fea in self.cross_features}
    input_ffm = self.ffm_embedding(x_ffm, self.cross_features, squeeze_dim=False)
    em = self.ffm(input_ffm)
    aem = self.cen(em) if hasattr(self, "cen") else em.flatten(start_dim=1)
    y = y_linear + self.mlp_out(aem)
    return torch.sigmoid(y.squeeze(1) + self.b)


def cls_model(kind, cfg, gold):
    model = build_ffm_model(cfg, gold)
    if kind == "layer":
        model.forward = reference_forward.__get__(model)
    return model


@pytest.mark.parametrize("cfg", FFM_MODELS)
def test_patched_layer_path_equals_fused_model(cfg):
    gold, fused = load_model(cfg)
    _, layer = load_model(cfg, "layer")
    x, y = golden_batch(gold, 1)
    xd, yd = to_dev(x), y.to(dev()).float()
    pa, pb = fused(xd), layer(xd)
    assert pb.shape == pa.shape
    np.testing.assert_allclose(pb.detach().cpu().numpy(), pa.detach().cpu().numpy(), rtol=1e-5, atol=1e-6)
    torch.nn.BCELoss()(pa, yd).backward()
    torch.nn.BCELoss()(pb, yd).backward()
    da, db = dict(fused.named_parameters()), dict(layer.named_parameters())
    for n in da:
        ga, gb = da[n].grad, db[n].grad
        assert (ga is None) == (gb is None), n
        if ga is None:
            continue
        if n.endswith((".0.bias", ".4.bias")) and "mlp" in n:  # a Linear bias in front of BatchNorm: rounding noise
            assert max(float(ga.abs().max()), float(gb.abs().max())) < 1e-5, n
            continue
        torch.testing.assert_close(gb, ga, rtol=1e-4, atol=1e-6, msg=n)


def test_embedding_layer_bk_lookup_shapes():
    from torch_rechub_amd.basic.features import SparseFeature
    from torch_rechub_amd.basic.layers import EmbeddingLayer
    feas = [SparseFeature("a", 12, 10), SparseFeature("b", 30, 10)]
    emb = EmbeddingLayer(feas).to(dev())
    x = {"a": torch.randint(0, 12, (8, 3), device=dev()), "b": torch.randint(0, 30, (8, 3), device=dev())}
    out = emb(x, feas, squeeze_dim=False)
    assert out.shape == (8, 2, 3, 10)
    want = torch.stack([emb.embed_dict["a"].weight[x["a"]][..., :10], emb.embed_dict["b"].weight[x["b"]][..., :10]], 1)
    assert torch.equal(out, want)
    assert torch.equal(emb(x, feas, squeeze_dim=True), want.flatten(1))


# ---- captured step / lazy Adam, bit for bit ----------------------------------------------------------------------------
def _collision_free(vocabs, nb, B, seed):
    g = torch.Generator().manual_seed(seed)
    cols = []
    for v in vocabs:  # no row twice inside a batch: a random arithmetic progression per batch
        stride = torch.randint(max(1, (v - 1) // B // 2), (v - 1) // B + 1, (nb, 1), generator=g)
        start = (torch.rand(nb, 1, generator=g) * ((v - 1) - stride * (B - 1))).long()
        cols.append((start + stride * torch.arange(B).view(1, B)).view(-1))
    sparse = torch.stack(cols, 1).contiguous()
    label = (torch.rand(nb * B, generator=g) < 0.3).float()
    return sparse, label


VOCABS = [300, 1000, 2000, 5000, 20000, 700]


def _model(kind, fat, seed=11):
    from torch_rechub_amd.basic.features import SparseFeature
    from torch_rechub_amd.models.ranking import DeepFFM, FatDeepFFM
    torch.manual_seed(seed)
    F = len(VOCABS)
    linear = [SparseFeature(f"C{i}", v, 1) for i, v in enumerate(VOCABS)]
    cross = [SparseFeature(f"C{i}", v * F, 10) for i, v in enumerate(VOCABS)]
    mlp = {"dims": [64, 32], "dropout": 0.0, "activation": "relu"}
    m = FatDeepFFM(linear, cross, 10, 3, mlp) if fat else DeepFFM(linear, cross, 10, mlp)
    if kind == "layer":
        m.forward = reference_forward.__get__(m)
    return m, [f.name for f in linear]


def _train_twins(kind, fat, kw_a, kw_b, monkeypatch=None, nb=10, B=256):
    from torch_rechub_amd.trainers import CTRTrainer
    from torch_rechub_amd.utils.data import DeviceDataLoader
    sparse, label = _collision_free(VOCABS, nb, B, seed=21)
    ma, names = _model(kind, fat)
    mb, _ = _model(kind, fat)
    mb.load_state_dict(ma.state_dict())
    base = dict(optimizer_params={"lr": 1e-2, "weight_decay": 1e-4, "lazy_small_rows": 8}, device="cuda:0",
                show_progress=False)
    ta = CTRTrainer(ma, **base, **kw_a)
    tb = CTRTrainer(mb, **base, **kw_b)
    losses = [t.train_one_epoch(DeviceDataLoader(sparse.to(dev()), names, None, [], label.to(dev()), B, shuffle=False))
              for t in (ta, tb)]
    return ma, mb, ta, tb, losses


def _assert_bit_equal(ma, mb):
    sa, sb = ma.state_dict(), mb.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


@pytest.mark.parametrize("fat", [False, True])
def test_graph_step_equals_eager_training_bitwise(fat):
    ma, mb, ta, tb, losses = _train_twins("fused", fat, dict(use_graph=True, table_update="dense"),
                                          dict(use_graph=False, table_update="dense"))
    assert ta._graph is not None
    assert losses[0] == losses[1]
    _assert_bit_equal(ma, mb)


@pytest.mark.parametrize("kind", ["fused", "layer"])
@pytest.mark.parametrize("form", ["inline", "ahead", "relaxed", "strict"])
def test_lazy_equals_dense_adam_bitwise_in_every_step_form(kind, form, monkeypatch):
    """The refresh-ahead hazard: a field-aware gather's indices (x * F + j) exist only inside the step, so its rows must be
    refreshed in front of its own kernel, never replayed from the previous step's record."""
    from torch_rechub_amd import optim
    monkeypatch.setenv("RECHUB_STEP_FORM", "inline" if form == "inline" else "deferred")
    monkeypatch.setattr(optim, "RELAXED_JOIN", form not in ("strict", "inline"))
    monkeypatch.setattr(optim, "STEP_AHEAD", form == "ahead")
    ma, mb, ta, tb, losses = _train_twins(kind, kind == "fused", dict(use_graph=True, table_update="lazy", lazy_k=4),
                                          dict(use_graph=True, table_update="dense"))
    assert ta.optimizer.lazy_k == 4 and ta._form == ("inline" if form == "inline" else "deferred")
    assert losses[0] == losses[1]
    _assert_bit_equal(ma, mb)
    for pa, pb in zip(ta.optimizer._tables, tb.optimizer._tables):
        assert torch.equal(ta.optimizer.state[pa]["exp_avg"], tb.optimizer.state[pb]["exp_avg"])
        assert torch.equal(ta.optimizer.state[pa]["exp_avg_sq"], tb.optimizer.state[pb]["exp_avg_sq"])


def test_row_sharded_field_aware_tables_raise():
    from torch_rechub_amd import sharding
    m, _ = _model("fused", False)
    m = m.to(dev())
    x = {f"C{i}": torch.zeros(4, dtype=torch.long, device=dev()) for i in range(len(VOCABS))}
    tab = m.ffm_embedding.embed_dict["C0"]
    orig = sharding.is_sharded
    try:
        sharding.is_sharded = lambda t: t is tab or orig(t)
        with pytest.raises(RuntimeError, match="row-sharded"):
            m(x)
    finally:
        sharding.is_sharded = orig


# ---- data parallel, replicated tables ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nccl_world1():
    import socket

    import torch.distributed as dist
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda:0"))
    yield
    dist.destroy_process_group()


@pytest.mark.parametrize("use_graph", [False, "single"])
def test_data_parallel_machinery_on_one_rank_equals_plain_training_bitwise(nccl_world1, monkeypatch, use_graph):
    from torch_rechub_amd import ops
    from torch_rechub_amd.trainers import CTRTrainer
    from torch_rechub_amd.utils.data import DeviceDataLoader
    nb, B = 8, 128
    sparse, label = _collision_free(VOCABS, nb, B, seed=31)
    ma, names = _model("fused", True)
    mb, _ = _model("fused", True)
    mb.load_state_dict(ma.state_dict())
    params = {"lr": 1e-2, "weight_decay": 1e-4, "lazy_small_rows": 64}
    mk = lambda: DeviceDataLoader(sparse.to(dev()), names, None, [], label.to(dev()), B, shuffle=False)  # noqa: E731
    monkeypatch.setenv("RECHUB_FORCE_DP", "0")
    ta = CTRTrainer(ma, optimizer_params=dict(params), device="cuda:0", show_progress=False, lazy_k=4)
    assert ta.dp is None
    la = ta.train_one_epoch(mk())
    monkeypatch.setenv("RECHUB_FORCE_DP", "1")
    monkeypatch.setenv("RECHUB_DP_GRAPH", use_graph or "single")
    tb = CTRTrainer(mb, optimizer_params=dict(params), device="cuda:0", show_progress=False, lazy_k=4,
                    use_graph=bool(use_graph), tables="replicate")
    try:
        assert tb.dp is not None and ops._sparse_exchange is not None
        lb = tb.train_one_epoch(mk())
    finally:
        tb.dp.close()
    assert la == lb
    _assert_bit_equal(ma, mb)
