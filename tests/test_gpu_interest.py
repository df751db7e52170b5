"""YoutubeDNN / MIND / ComiRec on the MI355X: the kernels of csrc/interest.hip against float64 numpy at full size, the
layers and models against the reference's fixtures (tools/gen_golden_match.py, MIND's routing draws replayed through
CapsuleNetwork.routing_init), the 3-step MatchTrainer(mode=2) trajectory, the captured step against eager, repeatable
weight gradients, the memory bound of the ComirecDR step, and the one-rank data-parallel step."""
import numpy as np
import pytest
import torch

from conftest import assert_state_follows_reference_trajectory, golden_state, load_golden
from test_interest_host import MATCH_MODELS, build_match_model, np_capsule, np_listwise, squash_bwd

from torch_rechub_amd._lib import H

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def rand_mask(B, L, g):
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0], lens[1] = 0, L
    return (torch.arange(L)[None, :] < lens[:, None]).to(torch.int32)


# ---- kernels at full size against float64 numpy -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_capsule_kernel_full_size_against_float64(kind):
    capsule_case(kind, 4096, 50, 4, 16, 3)


@pytest.mark.parametrize("kind,I,D", [(0, 1, H.RH_CAPSULE_MAX_D), (1, H.RH_CAPSULE_MAX_ID // H.RH_CAPSULE_MAX_D, H.RH_CAPSULE_MAX_D),
                                      (1, H.RH_CAPSULE_MAX_ID, 1), (2, H.RH_CAPSULE_MAX_IDD // H.RH_CAPSULE_MAX_D ** 2, H.RH_CAPSULE_MAX_D)])
def test_capsule_kernel_at_each_limit(kind, I, D):
    """D, I D and (type 2) I D D at the limits of include/rechub_hip.h, two samples of two positions."""
    capsule_case(kind, 2, 2, I, D, 3)


def capsule_case(kind, B, L, I, D, rt):
    from torch_rechub_amd import ops
    g = torch.Generator().manual_seed(10 + kind)
    mask = rand_mask(B, L, g)
    e = 0.5 * torch.randn(B, L, D, generator=g)
    init = torch.randn(B, I, L, generator=g) if kind == 0 else None
    if kind == 2:
        w = 0.3 * torch.randn(1, L, I * D, D, generator=g)
        x, wd = e.to(dev()).requires_grad_(True), w.to(dev()).requires_grad_(True)
        uh = np.einsum("ljk,blk->blj", w[0].double().numpy(), e.double().numpy())
    else:
        Iu = 1 if kind == 0 else I
        x = (0.5 * torch.randn(B, L, Iu * D, generator=g)).to(dev()).requires_grad_(True)
        wd = None
        uh = x.detach().cpu().double().numpy()
        if kind == 0:
            uh = np.tile(uh, (1, 1, I))
    uh = uh.reshape(B, L, I, D).transpose(0, 2, 1, 3)
    cap = ops.capsule_routing(x, wd, mask.to(dev()), None if init is None else init.to(dev()), kind, I, D, rt)
    want, sw, s = np_capsule(uh, mask.numpy(), None if init is None else init.numpy(), rt)
    np.testing.assert_allclose(cap.detach().cpu().numpy(), want, rtol=1e-4, atol=2e-6)
    assert not cap[0].any()
    gy = torch.randn(B, I, D, generator=g)
    cap.backward(gy.to(dev()))
    gs = squash_bwd(s, gy.double().numpy())
    guh = np.einsum("bil,bid->blid", sw, gs)
    if kind == 2:
        w64 = w[0].double().numpy()
        np.testing.assert_allclose(x.grad.cpu().numpy(), np.einsum("ljk,blj->blk", w64, guh.reshape(B, L, I * D)),
                                   rtol=1e-4, atol=1e-5)
        gw = np.einsum("blj,blk->ljk", guh.reshape(B, L, I * D), e.double().numpy())[None]
        np.testing.assert_allclose(wd.grad.cpu().numpy(), gw, rtol=1e-4, atol=1e-4 * np.abs(gw).max())
    else:
        gu = guh.sum(2) if kind == 0 else guh.reshape(B, L, I * D)
        np.testing.assert_allclose(x.grad.cpu().numpy(), gu, rtol=1e-4, atol=1e-5)


def test_sa_pool_kernel_full_size_against_float64():
    from torch_rechub_amd import ops
    g = torch.Generator().manual_seed(20)
    B, L, I, D = 4096, 50, 4, 16
    mask = rand_mask(B, L, g)
    A = torch.randn(B, L, I, generator=g) * 3
    e = torch.randn(B, L, D, generator=g)
    Ad, ed = A.to(dev()).requires_grad_(True), e.to(dev()).requires_grad_(True)
    out = ops.sa_pool(Ad, ed, mask.to(dev()))
    Am = (A + np.float32(-1e9) * (1 - mask.float())[..., None]).double().numpy()
    ex = np.exp(Am - Am.max(1, keepdims=True))
    P = ex / ex.sum(1, keepdims=True)
    np.testing.assert_allclose(out.detach().cpu().numpy(), np.einsum("bli,bld->bid", P, e.double().numpy()), rtol=1e-4,
                               atol=1e-5)
    gy = torch.randn(B, I, D, generator=g)
    out.backward(gy.to(dev()))
    gP = np.einsum("bid,bld->bli", gy.double().numpy(), e.double().numpy())
    np.testing.assert_allclose(Ad.grad.cpu().numpy(), P * (gP - (P * gP).sum(1, keepdims=True)), rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(ed.grad.cpu().numpy(), np.einsum("bli,bid->bld", P, gy.double().numpy()), rtol=1e-4,
                               atol=1e-5)


@pytest.mark.parametrize("K", [3, 64])
@pytest.mark.parametrize("I", [1, 4])
def test_listwise_kernel_full_size_against_float64(K, I):
    from torch_rechub_amd import ops
    g = torch.Generator().manual_seed(30 + K + I)
    B, D = 4096, 16
    u = torch.nn.functional.normalize(torch.randn(B, I, D, generator=g), dim=-1)
    pos, neg = 0.1 * torch.randn(B, D, generator=g), 0.1 * torch.randn(B, K, D, generator=g)
    neg[5, 1] = 0.0  # a zero row: F.normalize's clamped denominator
    ud, pd, nd = (t.to(dev()).requires_grad_(True) for t in (u, pos, neg))
    logits, best = ops.listwise_logits(ud, pd, nd, 0.02)
    gy = torch.randn(B, 1 + K, generator=g)
    want, wbest, g_u, g_pos, g_neg = np_listwise(u.double().numpy(), pos.double().numpy(), neg.double().numpy(), 0.02,
                                                 gy.double().numpy())
    got_best = best.cpu().numpy()
    agree = got_best == wbest
    assert agree.mean() > 0.999  # (fp32 near-ties may pick the other interest)
    np.testing.assert_allclose(logits.detach().cpu().numpy()[agree], want[agree], rtol=1e-4, atol=1e-4)
    logits.backward(gy.to(dev()))
    np.testing.assert_allclose(ud.grad.cpu().numpy()[agree], g_u[agree], rtol=1e-4, atol=1e-3)
    np.testing.assert_allclose(pd.grad.cpu().numpy()[agree], g_pos[agree], rtol=1e-4, atol=1e-2)
    np.testing.assert_allclose(nd.grad.cpu().numpy()[agree], g_neg[agree], rtol=1e-4, atol=1e-2)


def test_listwise_ties_pick_the_first_interest():
    from torch_rechub_amd import ops
    u = torch.tensor([[[1.0, 0, 0, 0], [1.0, 0, 0, 0], [0, 1.0, 0, 0]]], device=dev())
    pos = torch.tensor([[2.0, 0, 0, 0]], device=dev())
    neg = torch.tensor([[[0, 3.0, 0, 0]]], device=dev())
    logits, best = ops.listwise_logits(u, pos, neg, 1.0)
    assert int(best[0]) == 0 and logits.cpu().tolist() == [[1.0, 0.0]]


# ---- layers against the fixtures ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2])
@pytest.mark.parametrize("rt", [1, 3, 4])
def test_capsule_layer_against_fixture(kind, rt):
    from torch_rechub_amd.basic.layers import CapsuleNetwork
    gold = load_golden("interest_layers.npz")
    k = f"caps{kind}_rt{rt}."
    I = 3 if kind == 1 else 4
    caps = CapsuleNetwork(16, 8, bilinear_type=kind, interest_num=I, routing_times=rt)
    caps.load_state_dict(golden_state(gold, k + "sd."))
    caps = caps.to(dev())
    if kind == 0:
        caps.routing_init = lambda B, I_, L, device: torch.from_numpy(gold[k + "init"]).to(device)
    e = torch.from_numpy(gold[k + "e"]).to(dev()).requires_grad_(True)
    y = caps(e, torch.from_numpy(gold["mask"]).to(dev()))
    np.testing.assert_allclose(y.detach().cpu().numpy(), gold[k + "out"], rtol=1e-5, atol=1e-6)
    assert y.requires_grad == (rt > 2)
    if rt > 2:
        y.backward(torch.from_numpy(gold[k + "g_out"]).to(dev()))
        np.testing.assert_allclose(e.grad.cpu().numpy(), gold[k + "g_e"], rtol=1e-5, atol=1e-6)
        for n, p in caps.named_parameters():
            if n.startswith("relu."):
                assert p.grad is None
                continue
            np.testing.assert_allclose(p.grad.cpu().numpy(), gold[k + "grad." + n], rtol=1e-5, atol=1e-6, err_msg=n)
    with pytest.raises(RuntimeError):
        caps(e[:, :7], torch.from_numpy(gold["mask"][:, :7]).to(dev()))


def test_sa_layer_against_fixture_and_w3_has_no_grad():
    from torch_rechub_amd.basic.layers import MultiInterestSA
    gold = load_golden("interest_layers.npz")
    sa = MultiInterestSA(16, 4)
    sa.load_state_dict(golden_state(gold, "sa.sd."))
    sa = sa.to(dev())
    e = torch.from_numpy(gold["sa.e"]).to(dev()).requires_grad_(True)
    mask = torch.from_numpy(gold["mask"]).to(dev()).unsqueeze(-1).float()
    y = sa(e, mask)
    # (H W2 with torch.rand weights sums 64 positive terms: |A| ~ 30, so the GEMMs' fp32 summation order moves the softmax
    # weights by ~1e-5 relative)
    np.testing.assert_allclose(y.detach().cpu().numpy(), gold["sa.out"], rtol=3e-5, atol=1e-6)
    y.backward(torch.from_numpy(gold["sa.g_out"]).to(dev()))
    np.testing.assert_allclose(e.grad.cpu().numpy(), gold["sa.g_e"], rtol=3e-5, atol=1e-6)
    for n in ("W1", "W2"):
        ref = gold["sa.grad." + n]
        np.testing.assert_allclose(getattr(sa, n).grad.cpu().numpy(), ref, rtol=3e-5, atol=1e-6 * max(1, np.abs(ref).max()))
    assert sa.W3.grad is None


# ---- models against the reference ------------------------------------------------------------------------------------
class Replay(object):
    """CapsuleNetwork.routing_init that hands out MIND's recorded torch.randn draws in call order."""

    def __init__(self, draws, start):
        self.draws, self.i = draws, start

    def __call__(self, B, I, L, device):
        t = torch.from_numpy(self.draws[self.i]).to(device)
        self.i += 1
        assert t.shape == (B, I, L)
        return t


def load_model(cfg, draw=0):
    gold = load_golden(f"model_{cfg}.npz")
    model = build_match_model(cfg, gold)
    model.load_state_dict(golden_state(gold, "sd0."))
    model = model.to(dev())
    if cfg == "mind":
        model.capsule.routing_init = Replay(gold["routing_draws"], draw)
    return gold, model


def golden_x(gold, bi):
    return {k[len(f"x{bi}."):]: torch.from_numpy(gold[k]).to(dev()) for k in gold.files if k.startswith(f"x{bi}.")}


@pytest.mark.parametrize("cfg", MATCH_MODELS)
def test_forward_loss_and_gradients_match_reference(cfg):
    from torch_rechub_amd import ops
    gold, model = load_model(cfg)  # draws: eval 0, user mode 1, probe 2
    x = golden_x(gold, 0)
    tol = dict(rtol=1e-5, atol=1e-4 if cfg == "youtubednn" else 2e-6)  # (YoutubeDNN: logits / 0.02)
    model.eval()
    with torch.no_grad():
        np.testing.assert_allclose(model(x).cpu().numpy(), gold["pred_eval"], **tol)
        model.mode = "user"
        np.testing.assert_allclose(model(x).cpu().numpy(), gold["user_emb"], rtol=1e-5, atol=1e-6)
        model.mode = "item"
        np.testing.assert_allclose(model(x).cpu().numpy(), gold["item_emb"], rtol=1e-5, atol=1e-6)
        model.mode = None
    model.train()
    pred = model(x)
    np.testing.assert_allclose(pred.detach().cpu().numpy(), gold["pred_train"], **tol)
    loss = ops.cross_entropy_mean(pred, torch.zeros(pred.shape[0], dtype=torch.long, device=dev()))
    assert abs(loss.item() - float(gold["loss"])) < 1e-5 * max(1.0, abs(float(gold["loss"])))
    loss.backward()
    ops.check_errors()
    gmax = max(float(np.abs(gold["grad." + n]).max()) for n, _ in model.named_parameters())
    for n, p in model.named_parameters():
        ref = gold["grad." + n]
        got = p.grad.detach().cpu().numpy() if p.grad is not None else np.zeros_like(ref)
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=2e-6 * gmax, err_msg=f"{cfg}: grad of {n}")


@pytest.mark.parametrize("cfg", MATCH_MODELS)
def test_three_step_training_matches_reference_trainer(cfg):
    from torch_rechub_amd.trainers import MatchTrainer
    gold, model = load_model(cfg, draw=3)  # the three training steps' draws
    batches = [(golden_x(gold, i), torch.from_numpy(gold[f"y{i}"]).to(dev())) for i in range(3)]
    trainer = MatchTrainer(model, mode=2, optimizer_params={"lr": float(gold["train.lr"]), "weight_decay":
                                                            float(gold["train.wd"])},
                           n_epoch=1, device="cuda:0", show_progress=False)
    mean_loss = trainer.train_one_epoch(batches)
    assert abs(mean_loss - float(gold["train.mean_loss"])) < 5e-5 * max(1.0, abs(float(gold["train.mean_loss"])))
    assert_state_follows_reference_trajectory(gold, model.state_dict(), cfg)


def reference_forward(self, x):
    """The reference MIND / ComiRec forward (mind.py / comirec.py) restated on the HIP layers, as a patched reference
    model runs it: expand + cat + matmul + F.normalize, torch.cat of the item rows, bmm / argmax / gather."""
    F = torch.nn.functional
    input_user = self.embedding(x, self.user_features, squeeze_dim=True).unsqueeze(1)
    input_user = input_user.expand([input_user.shape[0], self.interest_num, input_user.shape[-1]])
    history_emb = self.embedding(x, self.history_features).squeeze(1)
    mask = self.gen_mask(x)
    if hasattr(self, "capsule"):
        interests = self.capsule(history_emb, mask)
    else:
        interests = self.multi_interest_sa(history_emb, mask.unsqueeze(-1).float())
    user = F.normalize(torch.matmul(torch.cat([input_user, interests], dim=-1), self.convert_user_weight), p=2, dim=-1)
    pos = F.normalize(self.embedding(x, self.item_features, squeeze_dim=False), p=2, dim=-1)
    neg = F.normalize(self.embedding(x, self.neg_item_feature, squeeze_dim=False).squeeze(1), p=2, dim=-1)
    items = torch.cat((pos, neg), dim=1)
    k = torch.argmax(torch.bmm(user, items[:, 0, :].unsqueeze(-1)), dim=1).squeeze(-1)
    best = user[torch.arange(user.shape[0], device=user.device), k, :].unsqueeze(1)
    return torch.mul(best, items).sum(dim=-1)


@pytest.mark.parametrize("cfg", ["mind", "comirec_dr", "comirec_sa"])
def test_reference_layer_path_matches_fixture(cfg):
    gold, model = load_model(cfg, draw=2)
    model.forward = reference_forward.__get__(model)
    model.train()
    pred = model(golden_x(gold, 0))
    np.testing.assert_allclose(pred.detach().cpu().numpy(), gold["pred_train"], rtol=1e-5, atol=2e-6)


# ---- captured step, repeatability, memory ----------------------------------------------------------------------------
B_T, L_T, K_T, N_ITEM, N_USER = 64, 8, 3, 100000, 20000


def _unique_batches(nb, seed):
    """Every table row at most once per step (no float-atomic order in the embedding backward): user ids and the
    item rows of history + positive + negatives are drawn without replacement; full-length histories."""
    g = torch.Generator().manual_seed(seed)
    cols = []
    for _ in range(nb):
        items = torch.randperm(N_ITEM - 1, generator=g)[:B_T * (L_T + 1 + K_T)].view(B_T, -1) + 1
        users = torch.randperm(N_USER, generator=g)[:B_T].view(B_T, 1)
        cols.append(torch.cat([users, items[:, :1], items[:, 1:1 + L_T], items[:, 1 + L_T:]], 1))
    return torch.cat(cols).contiguous()


def _train_model(cfg, seed=5):
    from torch_rechub_amd.basic.features import SequenceFeature, SparseFeature
    from torch_rechub_amd.models.matching import MIND, ComirecDR, ComirecSA, YoutubeDNN
    torch.manual_seed(seed)
    user = [SparseFeature("user_id", N_USER, 16)]
    hist = [SequenceFeature("hist_item_id", N_ITEM, 16, pooling="concat", shared_with="item_id")]
    item = [SparseFeature("item_id", N_ITEM, 16)]
    neg = [SequenceFeature("neg_items", N_ITEM, 16, pooling="concat", shared_with="item_id")]
    if cfg == "youtubednn":
        m = YoutubeDNN(user, item, neg, user_params={"dims": [32, 16]}, temperature=0.05)
    elif cfg == "mind":
        m = MIND(user, hist, item, neg, max_length=L_T)
    elif cfg == "comirec_dr":
        m = ComirecDR(user, hist, item, neg, max_length=L_T)
        with torch.no_grad():
            m.capsule.w.normal_(0, 0.3)
    else:
        m = ComirecSA(user, hist, item, neg)
    with torch.no_grad():
        for e in m.embedding.embed_dict.values():
            e.weight.normal_(0, 0.1)
    return m


def _loader(cfg, sparse):
    from torch_rechub_amd.utils.data import DeviceDataLoader
    names = ["user_id", "item_id", ("hist_item_id", L_T), ("neg_items", K_T)]
    label = torch.zeros(sparse.shape[0], device=dev())
    return DeviceDataLoader(sparse.to(dev()), names, None, [], label, B_T, shuffle=False)


@pytest.mark.parametrize("cfg", MATCH_MODELS)
def test_graph_step_equals_eager_training_bitwise(cfg):
    from torch_rechub_amd.trainers import MatchTrainer
    sparse = _unique_batches(10, seed=41)
    ma, mb = _train_model(cfg), _train_model(cfg)
    mb.load_state_dict(ma.state_dict())
    base = dict(mode=2, optimizer_params={"lr": 1e-2, "weight_decay": 1e-4}, device="cuda:0", show_progress=False,
                table_update="dense")
    losses = []
    ts = []
    for m, ug in ((ma, True), (mb, False)):
        torch.cuda.manual_seed(7)  # MIND's per-step torch.randn: the same stream eager and captured
        t = MatchTrainer(m, use_graph=ug, **base)
        losses.append(t.train_one_epoch(_loader(cfg, sparse)))
        ts.append(t)
    assert ts[0]._graph is not None
    assert losses[0] == losses[1]
    sa, sb = ma.state_dict(), mb.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


def test_weight_gradients_bit_identical_across_runs():
    from torch_rechub_amd.basic.layers import CapsuleNetwork, MultiInterestSA
    g = torch.Generator().manual_seed(50)
    B, L, D = 4096, 50, 16
    e = (0.5 * torch.randn(B, L, D, generator=g)).to(dev())
    mask = rand_mask(B, L, g).to(dev())
    torch.manual_seed(1)
    caps = CapsuleNetwork(D, L, bilinear_type=2).to(dev())
    with torch.no_grad():
        caps.w.normal_(0, 0.3)
    sa = MultiInterestSA(D, 4).to(dev())
    gy = torch.randn(B, 4, D, generator=g).to(dev())
    runs = []
    for _ in range(2):
        caps.zero_grad(set_to_none=True)
        sa.zero_grad(set_to_none=True)
        caps(e, mask).backward(gy)
        sa(e, mask.unsqueeze(-1).float()).backward(gy)
        runs.append([caps.w.grad.clone(), sa.W1.grad.clone(), sa.W2.grad.clone()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_comirec_dr_step_never_allocates_the_bilinear_product():
    """The reference's type-2 routing forms a (B, L, I*D, D) product (839 MB here); the whole step stays far below it."""
    from torch_rechub_amd.trainers import MatchTrainer
    B, L, I, D = 4096, 50, 4, 16
    from torch_rechub_amd.basic.features import SequenceFeature, SparseFeature
    from torch_rechub_amd.models.matching import ComirecDR
    torch.manual_seed(3)
    user = [SparseFeature("user_id", 1000, D)]
    hist = [SequenceFeature("hist_item_id", 5000, D, pooling="concat", shared_with="item_id")]
    item = [SparseFeature("item_id", 5000, D)]
    neg = [SequenceFeature("neg_items", 5000, D, pooling="concat", shared_with="item_id")]
    m = ComirecDR(user, hist, item, neg, max_length=L)
    with torch.no_grad():
        m.capsule.w.normal_(0, 0.3)
    g = torch.Generator().manual_seed(3)
    x = {"user_id": torch.randint(0, 1000, (B,), generator=g), "item_id": torch.randint(1, 5000, (B,), generator=g),
         "hist_item_id": torch.randint(0, 5000, (B, L), generator=g), "neg_items": torch.randint(1, 5000, (B, 3), generator=g)}
    batch = [({k: v.to(dev()) for k, v in x.items()}, torch.zeros(B, dtype=torch.long, device=dev()))]
    t = MatchTrainer(m, mode=2, device="cuda:0", show_progress=False)
    t.train_one_epoch(batch)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t.train_one_epoch(batch)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    product = B * L * I * D * D * 4
    assert peak < product // 4, f"step peak {peak / 2**20:.1f} MiB vs the {product / 2**20:.0f} MiB product"


# ---- data parallel, one rank -------------------------------------------------------------------------------------------
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


@pytest.mark.parametrize("cfg", ["comirec_sa", "comirec_dr"])
def test_data_parallel_one_rank_equals_plain_training_bitwise(nccl_world1, monkeypatch, cfg):
    """ComirecSA's W3 never receives a gradient (as in the reference): the gradient exchange must tolerate it."""
    from torch_rechub_amd.trainers import MatchTrainer
    sparse = _unique_batches(6, seed=61)
    ma, mb = _train_model(cfg), _train_model(cfg)
    mb.load_state_dict(ma.state_dict())
    base = dict(mode=2, optimizer_params={"lr": 1e-2, "weight_decay": 1e-4}, device="cuda:0", show_progress=False)
    monkeypatch.setenv("RECHUB_FORCE_DP", "0")
    ta = MatchTrainer(ma, **base)
    assert ta.dp is None
    la = ta.train_one_epoch(_loader(cfg, sparse))
    monkeypatch.setenv("RECHUB_FORCE_DP", "1")
    tb = MatchTrainer(mb, tables="replicate", **base)
    try:
        assert tb.dp is not None
        lb = tb.train_one_epoch(_loader(cfg, sparse))
    finally:
        tb.dp.close()
    assert la == lb
    sa, sb = ma.state_dict(), mb.state_dict()
    # parameters that never receive a gradient (ComirecSA's W3, the unused relu Linear of CapsuleNetwork): plain training
    # leaves them untouched (torch Adam skips a None gradient, as the reference's trainer does); the data-parallel bucket
    # hands a missing gradient over as zeros (distributed.GradBucket.finish), so weight decay moves them there
    unused = {n for n, p in ma.named_parameters() if p.grad is None}
    assert unused == ({"multi_interest_sa.W3"} if cfg == "comirec_sa" else {"capsule.relu.0.weight"})
    sd0 = _train_model(cfg).state_dict()
    for k in sa:
        if k in unused:
            assert torch.equal(sa[k], sd0[k].to(dev())), k
            continue
        assert torch.equal(sa[k], sb[k]), k
