"""NARM / STAMP / GRU4Rec on the MI355X: the kernels of csrc/session.hip and the full-catalogue head (csrc/stream_ce.hip) against float64 at
full size and at their edges, repeatable backwards, the models and three MatchTrainer steps against the reference's
fixtures (tools/gen_golden_session.py), the errors for inputs the reference rejects, batches of different L, the memory
bound of a large-catalogue NARM step and the captured step against eager.  The rest of the kernels' shape range (partly
filled GRU workgroups, second trips of the strided loops, the guards' largest shapes, every split path of the catalogue
head, the empty batch) is in test_gpu_session_hllm_shapes.py."""
import numpy as np
import pytest
import torch

from conftest import assert_state_follows_reference_trajectory, assert_trajectory_close, golden_state, load_golden
from test_session_host import (SESSION_CFGS, build_session_model, np_attn_pool, np_attn_pool_bwd, np_gru, np_gru_bwd)

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _rel_close(got, want, rtol, what):
    scale = max(float(np.abs(want).max()), 1e-30)
    err = float(np.abs(got - want).max()) / scale
    assert err < rtol, f"{what}: max error {err:.3e} of the largest magnitude"


# ---- GRU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,T,I,H,bias", [(4096, 50, 64, 50, True), (4096, 50, 100, 100, False), (4096, 50, 32, 128, True),
                                          (37, 9, 5, 1, True), (37, 9, 5, 127, False), (300, 1, 12, 10, True)])
def test_gru_kernel_against_float64(B, T, I, H, bias):
    from torch_rechub_amd import ops
    torch.manual_seed(H + T)
    gru = torch.nn.GRU(I, H, batch_first=True, bias=bias).to(dev())
    x = (0.5 * torch.randn(B, T, I)).to(dev()).requires_grad_(True)
    out, h_n = ops.gru_layers(gru, x)
    p = {n: t.detach().double().cpu().numpy() for n, t in gru.named_parameters()}
    x64 = x.detach().double().cpu().numpy()
    want, cache = np_gru(x64, p["weight_ih_l0"], p["weight_hh_l0"], p.get("bias_ih_l0"), p.get("bias_hh_l0"))
    _rel_close(out.detach().cpu().numpy(), want, 2e-5, "h_all")
    np.testing.assert_array_equal(h_n[0].detach().cpu().numpy(), out[:, -1].detach().cpu().numpy())
    g = torch.randn(B, T, H)
    out.backward(g.to(dev()))
    dx, dwi, dwh, dbi, dbh = np_gru_bwd(x64, p["weight_ih_l0"], p["weight_hh_l0"], cache, g.double().numpy())
    _rel_close(x.grad.cpu().numpy(), dx, 1e-4, "dx")
    _rel_close(gru.weight_ih_l0.grad.cpu().numpy(), dwi, 1e-4, "dW_ih")
    _rel_close(gru.weight_hh_l0.grad.cpu().numpy(), dwh, 1e-4, "dW_hh")
    if bias:
        _rel_close(gru.bias_ih_l0.grad.cpu().numpy(), dbi, 1e-4, "db_ih")
        _rel_close(gru.bias_hh_l0.grad.cpu().numpy(), dbh, 1e-4, "db_hh")


def test_gru_two_layers_time_major_matches_torch():
    from torch_rechub_amd import ops
    torch.manual_seed(4)
    gru = torch.nn.GRU(16, 16, num_layers=2, bias=False).to(dev())
    x = torch.randn(50, 256, 16, device=dev())
    out, h_n = ops.gru_layers(gru, x)
    ref_out, ref_h = torch.nn.GRU.forward(gru, x)
    np.testing.assert_allclose(out.detach().cpu().numpy(), ref_out.detach().cpu().numpy(), rtol=1e-4, atol=2e-5)
    np.testing.assert_allclose(h_n.detach().cpu().numpy(), ref_h.detach().cpu().numpy(), rtol=1e-4, atol=2e-5)


# ---- attention pooling ----------------------------------------------------------------------------------------------------
POOL_CASES = [(4096, 50, 100, 50, True, True), (4096, 50, 50, 50, False, False), (4096, 50, 128, 100, True, False),
              (64, 1, 7, 9, False, True), (64, 1, 7, 9, True, False), (33, 19, 10, 12, True, True)]


@pytest.mark.parametrize("B,L,H,Dx,floor,add", POOL_CASES)
def test_attention_pool_kernel_against_float64(B, L, H, Dx, floor, add):
    from torch_rechub_amd import ops
    g = torch.Generator().manual_seed(B + L + H)
    P = torch.randn(B, L, H, generator=g)
    r = torch.randn(B, H, generator=g)
    w0 = 0.3 * torch.randn(H, generator=g)
    X = torch.randn(B, L, Dx, generator=g)
    A = torch.randn(B, Dx, generator=g) if add else None
    lens = torch.randint(1, L + 1, (B,), generator=g)
    mask = torch.arange(L)[None] < lens[:, None]
    if floor:
        mask[1:] = False  # every row but one empty: the floor keeps them at zero weight
    ts = [t.to(dev()).requires_grad_(True) for t in (P, r, w0, X)]
    out = ops.additive_attention_pool(ts[0], ts[1], ts[2], mask.to(dev()), ts[3],
                                      None if A is None else A.to(dev()), floor=floor)
    args64 = [t.double().numpy() for t in (P, r, w0)]
    want, cache = np_attn_pool(*args64, mask.double().numpy(), X.double().numpy(), None if A is None else A.double().numpy(),
                               floor)
    _rel_close(out.detach().cpu().numpy(), want, 2e-6, "out")
    gy = torch.randn(B, Dx, generator=g)
    out.backward(gy.to(dev()))
    refs = np_attn_pool_bwd(*args64, X.double().numpy(), cache, gy.double().numpy(), floor)
    for t, ref, name in zip(ts, refs, ("dP", "dr", "dw0", "dX")):
        _rel_close(t.grad.cpu().numpy(), ref, 2e-5, name)


def test_attention_pool_backward_bitwise_repeatable():
    from torch_rechub_amd import ops
    g = torch.Generator().manual_seed(9)
    B, L, H = 4096, 50, 100
    base = [torch.randn(B, L, H, generator=g), torch.randn(B, H, generator=g), torch.randn(H, generator=g),
            torch.randn(B, L, H, generator=g)]
    mask = (torch.rand(B, L, generator=g) < 0.8).to(dev())
    gy = torch.randn(B, H, generator=g).to(dev())
    grads = []
    for _ in range(2):
        ts = [t.to(dev()).requires_grad_(True) for t in base]
        ops.additive_attention_pool(ts[0], ts[1], ts[2], mask, ts[3]).backward(gy)
        grads.append([t.grad.clone() for t in ts])
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def test_gru_backward_bitwise_repeatable():
    from torch_rechub_amd import ops
    torch.manual_seed(11)
    gru = torch.nn.GRU(100, 50, batch_first=True).to(dev())
    x0 = torch.randn(4096, 50, 100, device=dev())
    gy = torch.randn(4096, 50, 50, device=dev())
    grads = []
    for _ in range(2):
        gru.zero_grad(set_to_none=True)
        x = x0.clone().requires_grad_(True)
        ops.gru_layers(gru, x)[0].backward(gy)
        grads.append([x.grad.clone()] + [p.grad.clone() for p in gru.parameters()])
    for a, b in zip(*grads):
        assert torch.equal(a, b)


# ---- full-catalogue cross entropy --------------------------------------------------------------------------------------
def chunked_ce64(u, E, labels, chunk=1 << 16):
    """float64 on the device, V in chunks: (loss, du, dE)."""
    u64, B = u.double(), u.shape[0]
    m = torch.full((B,), -float("inf"), dtype=torch.float64, device=u.device)
    s = torch.zeros(B, dtype=torch.float64, device=u.device)
    for c0 in range(0, E.shape[0], chunk):
        z = u64 @ E[c0:c0 + chunk].double().T
        nm = torch.maximum(m, z.max(1).values)
        s = s * torch.exp(m - nm) + torch.exp(z - nm[:, None]).sum(1)
        m = nm
    lse = m + torch.log(s)
    zl = (u64 * E[labels].double()).sum(1)
    du = torch.zeros_like(u64)
    dE = torch.empty(E.shape, dtype=torch.float64, device=u.device)
    for c0 in range(0, E.shape[0], chunk):
        Ec = E[c0:c0 + chunk].double()
        p = torch.exp(u64 @ Ec.T - lse[:, None])
        sel = (labels >= c0) & (labels < c0 + Ec.shape[0])
        p[sel.nonzero()[:, 0], labels[sel] - c0] -= 1
        p /= B
        du += p @ Ec
        dE[c0:c0 + chunk] = p.T @ u64
    return (lse - zl).mean().item(), du, dE


@pytest.mark.parametrize("B,D,V", [(4096, 100, 1000000), (512, 100, 50000), (6, 12, 40), (70, 7, 2)])
def test_catalogue_ce_against_float64(B, D, V):
    from torch_rechub_amd import ops
    g = torch.Generator(device=dev()).manual_seed(B + V)
    u = torch.randn(B, D, device=dev(), generator=g).requires_grad_(True)
    E = (0.1 * torch.randn(V, D, device=dev(), generator=g)).requires_grad_(True)
    labels = torch.randint(0, V, (B,), device=dev(), generator=g)
    labels[0] = 0
    labels[-1] = V - 1
    loss = ops.catalogue_cross_entropy(u, E, labels)
    loss.backward()
    ops.check_errors()
    want, du, dE = chunked_ce64(u.detach(), E.detach(), labels)
    assert abs(loss.item() - want) < 2e-5 * max(1.0, abs(want))
    _rel_close(u.grad.cpu().numpy(), du.cpu().numpy(), 2e-5, "du")
    _rel_close(E.grad.cpu().numpy(), dE.cpu().numpy(), 2e-5, "dE")
    if V >= 50000:  # bitwise repeatable
        u2, E2 = u.detach().clone().requires_grad_(True), E.detach().clone().requires_grad_(True)
        ops.catalogue_cross_entropy(u2, E2, labels).backward()
        assert torch.equal(u2.grad, u.grad) and torch.equal(E2.grad, E.grad)


def test_catalogue_ce_out_of_range_label_sets_the_error_word():
    from torch_rechub_amd import ops
    u = torch.randn(8, 12, device=dev())
    E = torch.randn(40, 12, device=dev())
    lab = torch.tensor([0, 1, 2, 3, 40, 5, 6, 7], device=dev())
    ops.catalogue_cross_entropy(u, E, lab)
    with pytest.raises(IndexError):
        ops.check_errors()


# ---- models against the reference's fixtures ---------------------------------------------------------------------------
def load_model(cfg):
    gold = load_golden(f"model_session_{cfg}.npz")
    model = build_session_model(cfg, gold)
    model.load_state_dict(golden_state(gold, "sd0."))
    return gold, model.to(dev())


def golden_x(gold, bi):
    return {k[len(f"x{bi}."):]: torch.from_numpy(gold[k]).to(dev()) for k in gold.files if k.startswith(f"x{bi}.")}


def gru4rec_grads64(gold):
    """Parameter gradients of the reference GRU4Rec's training loss on batch 0 (gru4rec.py, basic/layers.py MLP: Linear,
    training-mode BatchNorm1d, ReLU per layer; CrossEntropyLoss against class 0) in float64 on the CPU, from sd0."""
    import torch.nn.functional as F
    sd = {k: v.double().requires_grad_(v.is_floating_point() and "running" not in k) for k, v in golden_state(gold, "sd0.").items()}
    x = {k: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("x0.")}
    E = lambda n: sd[f"embedding.embed_dict.{n}.weight"]  # noqa: E731
    u_in = torch.cat([E("user_id")[x["x0.user_id"]], E("age")[x["x0.age"]]], 1)
    D = E("item_id").shape[1]
    gru = torch.nn.GRU(D, D, num_layers=2, batch_first=True, bias=False).double()
    with torch.no_grad():
        for k in ("weight_ih_l0", "weight_hh_l0", "weight_ih_l1", "weight_hh_l1"):
            getattr(gru, k).copy_(sd["gru." + k])
    _, h_n = gru(E("item_id")[x["x0.hist_item_id"]])
    h = torch.cat([u_in, h_n[-1]], 1)
    i = 0
    while f"user_mlp.mlp.{i}.weight" in sd:
        h = F.linear(h, sd[f"user_mlp.mlp.{i}.weight"], sd[f"user_mlp.mlp.{i}.bias"])
        h = F.batch_norm(h, None, None, sd[f"user_mlp.mlp.{i + 1}.weight"], sd[f"user_mlp.mlp.{i + 1}.bias"], training=True)
        h = torch.relu(h)
        i += 4
    u = F.normalize(h, dim=-1).unsqueeze(1)
    items = F.normalize(torch.cat([E("item_id")[x["x0.item_id"]].unsqueeze(1), E("item_id")[x["x0.neg_items"]]], 1), dim=-1)
    loss = F.cross_entropy((u * items).sum(1), torch.from_numpy(gold["y0"]))
    grads = {}
    loss.backward()
    for k, v in sd.items():
        if v.requires_grad:
            grads[k] = v.grad.numpy() if v.grad is not None else np.zeros(tuple(v.shape))
    # the GRU's weights were copied into a module: their gradients live there
    for k in ("weight_ih_l0", "weight_hh_l0", "weight_ih_l1", "weight_hh_l1"):
        grads["gru." + k] = getattr(gru, k).grad.numpy()
    return grads


@pytest.mark.parametrize("cfg", SESSION_CFGS)
def test_forward_loss_and_gradients_match_reference(cfg):
    from torch_rechub_amd import ops
    gold, model = load_model(cfg)
    x = golden_x(gold, 0)
    y = torch.from_numpy(gold["y0"]).to(dev())
    model.eval()
    with torch.no_grad():
        want = gold["pred_eval"]
        np.testing.assert_allclose(model(x).cpu().numpy(), want, rtol=1e-5, atol=1e-5 * float(np.abs(want).max()))
    if cfg == "narm_inbatch":
        return
    model.train()
    if cfg == "gru4rec":
        pred = model(x)
        loss = torch.nn.CrossEntropyLoss()(pred, y)
    else:
        u, table = model.catalogue_head(x)
        loss = ops.catalogue_cross_entropy(u, table, y)
    assert abs(loss.item() - float(gold["loss"])) < 1e-5 * max(1.0, abs(float(gold["loss"])))
    loss.backward()
    ops.check_errors()
    gmax = max(float(np.abs(gold["grad." + n]).max()) for n, _ in model.named_parameters())
    exact = gru4rec_grads64(gold) if cfg == "gru4rec" else None
    for n, p in model.named_parameters():
        ref = gold["grad." + n]
        got = p.grad.detach().cpu().numpy() if p.grad is not None else np.zeros_like(ref)
        if got.shape != ref.shape:  # a table stored padded to a kernel width: the padding columns get no gradient
            assert not got[:, ref.shape[1]:].any()
            got = got[:, :ref.shape[1]]
        if exact is None:
            np.testing.assert_allclose(got, ref, rtol=1e-5, atol=2e-6 * gmax, err_msg=f"{cfg}: grad of {n}")
            continue
        # GRU4Rec: the user MLP's training-mode BatchNorm over B = 6 rows amplifies float32 rounding, and the reference's
        # own float32 gradient (the fixture) is itself up to ~1e-4 (relative) from the float64 one.  Ours must be as close
        # to float64 as the fixture is (or within the 1e-5 bound), and within 1e-4 of the fixture.
        e64 = exact[n]
        fixture_err = float(np.abs(ref - e64).max())
        mine_err = float(np.abs(got - e64).max())
        assert mine_err <= max(2 * fixture_err, 1e-5 * float(np.abs(e64).max()) + 2e-6 * gmax), \
            f"grad of {n}: {mine_err:.3e} from float64, the reference's float32 {fixture_err:.3e}"
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=2e-5 * gmax, err_msg=f"{cfg}: grad of {n}")
    if cfg in ("narm", "stamp"):  # the scores reach the padding row of the table
        assert float(np.abs(gold["grad.item_emb.weight"][0]).max()) > 0


@pytest.mark.parametrize("cfg", SESSION_CFGS)
def test_three_step_training_matches_reference_trainer(cfg):
    from torch_rechub_amd.trainers import MatchTrainer
    gold, model = load_model(cfg)
    batches = [(golden_x(gold, i), torch.from_numpy(gold[f"y{i}"]).to(dev())) for i in range(3)]
    kw = dict(mode=2)
    if cfg == "narm_inbatch":
        kw = dict(mode=0, in_batch_neg=True, hard_negative=True, in_batch_neg_ratio=3)
    trainer = MatchTrainer(model, optimizer_params={"lr": float(gold["train.lr"]), "weight_decay": float(gold["train.wd"])},
                           n_epoch=1, device="cuda:0", show_progress=False, **kw)
    mean_loss = trainer.train_one_epoch(batches)
    assert abs(mean_loss - float(gold["train.mean_loss"])) < 1e-5 * max(1.0, abs(float(gold["train.mean_loss"])))
    if cfg == "narm_inbatch":  # (no probe gradients in this fixture: the three states directly)
        mine = model.state_dict()
        for k, v in golden_state(gold, "sd3.").items():
            assert_trajectory_close(mine[k].cpu().numpy(), v.numpy(), 3 * float(gold["train.lr"]), k)
        return
    assert_state_follows_reference_trajectory(gold, model.state_dict(), cfg)


# ---- inputs the reference rejects, batches of different L ------------------------------------------------------------------
def test_narm_raises_for_inputs_the_reference_rejects():
    gold, model = load_model("narm")
    x = golden_x(gold, 0)
    empty = x["hist_item_id"].clone()
    empty[3] = 0
    with pytest.raises(RuntimeError, match="greater than 0"):
        model({"hist_item_id": empty})
    short = x["hist_item_id"].clone()
    short[:, -1] = 0
    with pytest.raises(RuntimeError, match="shorter than its padded length"):
        model({"hist_item_id": short})
    gold, stamp = load_model("stamp")
    with pytest.raises(RuntimeError, match="greater than 0"):
        stamp({"hist_item_id": empty})


def test_rejected_sessions_set_the_error_word_under_graph_replay():
    from torch_rechub_amd import ops
    seq = torch.tensor([[3, 4, 0], [0, 0, 0]], device=dev())
    ops.check_errors()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        ops.session_lengths(torch.tensor([[3, 4, 5]], device=dev()), check_full=True)  # (warm-up outside the capture)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        counts = ops.session_lengths(seq, check_full=True)
    graph.replay()
    torch.cuda.synchronize()
    assert counts.tolist() == [2, 0]
    with pytest.raises(RuntimeError, match="greater than 0"):
        ops.check_errors()


def test_batches_of_different_length_train_one_after_another():
    from torch_rechub_amd.trainers import MatchTrainer
    for cfg in ("narm", "stamp"):
        gold, model = load_model(cfg)
        x = golden_x(gold, 0)["hist_item_id"]
        y = torch.from_numpy(gold["y0"]).to(dev())
        short = x[:, :4].clone()
        short[0] = x[0, :4]  # row 0 is full: its first 4 items
        trainer = MatchTrainer(model, mode=2, device="cuda:0", show_progress=False)
        losses = [trainer.train_step({"hist_item_id": b}, y).item() for b in (x, short, x)]
        assert all(np.isfinite(losses))
        model.eval()
        with torch.no_grad():
            assert model({"hist_item_id": short}).shape == (x.shape[0], gold["sd0.item_emb.weight"].shape[0])


# ---- memory bound and the captured step -----------------------------------------------------------------------------------
def _narm(V, D=100, H=50, seed=3):
    from torch_rechub_amd.basic.features import SequenceFeature
    from torch_rechub_amd.models.matching import NARM
    torch.manual_seed(seed)
    m = NARM(SequenceFeature("hist_item_id", V, D, pooling="concat"), H, 0.0, 0.0)
    with torch.no_grad():
        for p in (m.a_1, m.a_2, m.v, m.b):
            p.mul_(0.1)
    return m.to(dev())


def _sessions(N, L, V, seed):
    g = torch.Generator().manual_seed(seed)
    seq = torch.randint(1, V, (N, L), generator=g)
    lens = torch.randint(1, L + 1, (N,), generator=g)
    lens[::7] = L
    seq[torch.arange(L)[None] >= lens[:, None]] = 0
    return seq


def test_narm_large_catalogue_step_never_forms_the_scores():
    from torch_rechub_amd.trainers import MatchTrainer
    B, L, V = 4096, 19, 262144
    assert B * V * 4 >= 4e9
    model = _narm(V)
    trainer = MatchTrainer(model, mode=2, device="cuda:0", show_progress=False)
    seq = _sessions(B, L, V, 1).to(dev())
    y = torch.randint(0, V, (B,)).to(dev())
    trainer.train_step({"hist_item_id": seq}, y)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    loss = trainer.train_step({"hist_item_id": seq}, y)
    torch.cuda.synchronize()
    grew = torch.cuda.max_memory_allocated() - base
    assert np.isfinite(loss.item())
    assert grew < B * V * 4 / 10, f"step allocated {grew / 1e6:.0f} MB"


@pytest.mark.parametrize("cfg,p", [("narm", 0.0), ("stamp", 0.0), ("narm", 0.3)])
def test_graph_step_equals_eager_training_bitwise(cfg, p):
    from torch_rechub_amd.basic.features import SequenceFeature
    from torch_rechub_amd.models.matching import NARM, STAMP
    from torch_rechub_amd.trainers import MatchTrainer
    from torch_rechub_amd.utils.data import DeviceDataLoader
    V, L, Bt, D = 5000, 12, 256, 24
    seq = _sessions(Bt * 10, L, V, 5)  # (every batch holds full rows: NARM's longest prefix reaches L)
    label = torch.randint(0, V, (seq.shape[0],), generator=torch.Generator().manual_seed(6)).float()

    def build():
        torch.manual_seed(8)
        f = SequenceFeature("hist_item_id", V, D, pooling="concat")
        return (NARM(f, 16, p, p) if cfg == "narm" else STAMP(f, 0.05, 0.1)).to(dev())

    from torch_rechub_amd import ops
    rng = ops._dropout_rng(dev())
    rng0 = rng.clone()
    ma, mb = build(), build()
    losses, ts = [], []
    for m, ug in ((ma, True), (mb, False)):
        rng.copy_(rng0)  # the same dropout stream for both runs
        t = MatchTrainer(m, mode=2, use_graph=ug, device="cuda:0", show_progress=False,
                         optimizer_params={"lr": 1e-3, "weight_decay": 1e-5})
        loader = DeviceDataLoader(seq.contiguous().to(dev()), [("hist_item_id", L)], None, [], label.to(dev()), Bt,
                                  shuffle=False)
        losses.append(t.train_one_epoch(loader))
        ts.append(t)
    assert ts[0]._graph is not None
    assert losses[0] == losses[1]
    sa, sb = ma.state_dict(), mb.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


# ---- dropout (NARM's emb_dropout / session_rep_dropout at p > 0) ---------------------------------------------------------
@pytest.mark.parametrize("p", [0.25, 0.5])
def test_dropout_mask_scale_and_stream(p):
    from torch_rechub_amd import ops
    n = 1 << 20
    x = (torch.rand(n, device=dev()) + 0.5).view(1024, 1024).requires_grad_(True)  # no zero: y != 0 marks the kept ones
    y = ops.dropout(x, p)
    keep = y != 0
    scale = torch.tensor(1.0, device=dev()) / (1 - torch.tensor(p, device=dev()))  # 1 / (1 - p) in float32
    assert torch.equal(y[keep], x.detach()[keep] * scale)
    assert abs(keep.float().mean().item() - (1 - p)) < 5e-3
    g = torch.randn(1024, 1024, device=dev())
    y.backward(g)
    assert torch.equal(x.grad, torch.where(keep, g * scale, torch.zeros_like(g)))  # the forward's mask, recomputed
    y2 = ops.dropout(x.detach(), p)
    assert not torch.equal(keep, y2 != 0)  # the counter advanced: another mask
    assert torch.equal(ops.dropout(x, p, training=False), x) and torch.equal(ops.dropout(x, 0.0), x)


def test_narm_trains_with_the_example_dropouts():
    from torch_rechub_amd.basic.features import SequenceFeature
    from torch_rechub_amd.models.matching import NARM
    from torch_rechub_amd.trainers import MatchTrainer
    V, L, B = 3000, 19, 512
    torch.manual_seed(2)
    model = NARM(SequenceFeature("hist_item_id", V, 100, pooling="concat"), 50, 0.25, 0.5).to(dev())
    with torch.no_grad():
        for q in (model.a_1, model.a_2, model.v, model.b):
            q.mul_(0.1)
    trainer = MatchTrainer(model, mode=2, device="cuda:0", show_progress=False)
    seq = _sessions(B, L, V, 3).to(dev())
    y = seq[:, 0].clone()
    losses = [trainer.train_step({"hist_item_id": seq}, y).item() for _ in range(20)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0]
    model.eval()
    with torch.no_grad():
        a = model({"hist_item_id": seq})
        b = model({"hist_item_id": seq})
    assert torch.equal(a, b)  # eval: no dropout


# ---- HSTU's head keeps its bits -----------------------------------------------------------------------------------------
def test_hstu_head_gives_the_recorded_bits_through_its_old_entry_points():
    """tools/gen_golden_hstu_head_bits.py recorded loss, dh, dW and d bias from the library before the full-catalogue mode
    joined the streaming head; the rh_hstu_head_* path must still give exactly those bits."""
    from torch_rechub_amd import ops
    gold = load_golden("hstu_head_bits.npz")
    for ci in range(3):
        t1, t2, nce = (float(v) for v in gold[f"c{ci}.cfg"])
        h = torch.from_numpy(gold[f"c{ci}.h"]).to(dev()).requires_grad_(True)
        w = torch.from_numpy(gold[f"c{ci}.w"]).to(dev()).requires_grad_(True)
        b = torch.from_numpy(gold[f"c{ci}.bias"]).to(dev()).requires_grad_(True) if f"c{ci}.bias" in gold.files else None
        lab = torch.from_numpy(gold[f"c{ci}.labels"]).to(dev())
        loss = ops.next_token_loss(h, w, b, lab, temperature=t1, nce_temperature=t2 if nce else None)
        loss.backward()
        assert np.array_equal(loss.detach().cpu().numpy(), gold[f"c{ci}.loss"]), ci
        assert np.array_equal(h.grad.cpu().numpy(), gold[f"c{ci}.g_h"]), ci
        assert np.array_equal(w.grad.cpu().numpy(), gold[f"c{ci}.g_w"]), ci
        if b is not None:
            assert np.array_equal(b.grad.cpu().numpy(), gold[f"c{ci}.g_bias"]), ci
