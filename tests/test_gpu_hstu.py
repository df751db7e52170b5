"""HSTU on the MI355X: the attention kernels of csrc/hstu.hip and the next-token head of csrc/stream_ce.hip against
float64 numpy at full size, the kernel's time buckets against torch CPU, bitwise repeatable backwards, the model step
against a float64 restatement, and the memory bound of the fused step."""
import numpy as np
import pytest
import torch

from test_hstu_host import BUCKET_CFGS, adversarial_deltas, np_attention, np_attention_bwd, np_head
from torch_rechub_amd.utils.hstu_utils import bucketize_time

from torch_rechub_amd._lib import H

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def attn_inputs(B, L, H, dqk, dv, N, nb, seed):
    g = torch.Generator().manual_seed(seed)
    proj = torch.nn.functional.silu(torch.randn(B, L, 2 * H * (dqk + dv), generator=g))
    pos_w = 0.3 * torch.randn(2 * N - 1, H, generator=g)
    ts_w = 0.3 * torch.randn(nb + 1, H, generator=g)
    td = torch.randint(0, 10**7, (B, L), generator=g)
    lens = torch.randint(0, L + 1, (B,), generator=g)
    lens[0], lens[1] = 0, L
    ar = torch.arange(L)[None, :]
    mask = ar < lens[:, None]             # right padding
    left = torch.arange(B) % 2 == 1
    mask[left] = (ar >= (L - lens[:, None]))[left]  # left padding on odd rows
    return proj, pos_w, ts_w, td, mask


def run_attn(proj, pos_w, ts_w, td, mask, H, dqk, dv, N, nb, fn, div, unit, gout):
    from torch_rechub_amd import ops
    x = proj.to(dev()).requires_grad_(True)
    pw = pos_w.to(dev()).requires_grad_(True)
    tw = ts_w.to(dev()).requires_grad_(True)
    out = ops.hstu_attention(x, pw, tw, H, dqk, dv, N, time_diffs=None if td is None else td.to(dev()),
                             padding_mask=mask.to(dev()), num_time_buckets=nb, time_bucket_fn=fn, time_bucket_divisor=div,
                             time_bucket_unit=unit)
    out.backward(gout.to(dev()))
    return out.detach().cpu(), x.grad.cpu(), pw.grad.cpu(), tw.grad.cpu()


@pytest.mark.parametrize("shape", [(128, 200, 1, 50, 50, 200, 128, "log", 0.301, "seconds", True),
                                   (16, 256, 8, H.RH_HSTU_MAX_DH, H.RH_HSTU_MAX_DH, 256, 128, "sqrt", 1.0, "minutes", True),
                                   (2, H.RH_HSTU_MAX_L, 1, 4, 4, H.RH_HSTU_MAX_L, 8, "sqrt", 1.0, "minutes", True),
                                   (2, 8, 1, 4, 4, 8, H.RH_HSTU_MAX_BUCKETS, "log", 0.301, "seconds", True),
                                   (16, 130, 2, 12, 10, 150, 64, "sqrt", 1.0, "minutes", False)])
def test_attention_kernel_full_size_against_float64(shape):
    B, L, H, dqk, dv, N, nb, fn, div, unit, with_time = shape
    proj, pos_w, ts_w, td, mask = attn_inputs(B, L, H, dqk, dv, N, nb, seed=L + H)
    td = td if with_time else None
    gout = torch.randn(B, L, H * dv, generator=torch.Generator().manual_seed(5))
    out, gp, gpos, gts = run_attn(proj, pos_w, ts_w, td, mask, H, dqk, dv, N, nb, fn, div, unit, gout)
    ref, cache = np_attention(proj.numpy(), pos_w.numpy(), ts_w.numpy(), None if td is None else td.numpy(), mask.numpy(),
                              H, dqk, dv, N, nb, fn, div, unit)
    np.testing.assert_allclose(out.numpy(), ref, rtol=1e-4, atol=2e-6)
    # rows whose keys are all masked (sample 0: every position padded) give an exact zero
    assert torch.all(out[0] == 0)
    rgp, rgpos, rgts = np_attention_bwd(cache, gout.numpy(), H, dqk, dv, N, 2 * N - 1, nb + 1)
    qkv = np.r_[0:2 * H * dqk, 2 * H * dqk + H * dv:2 * H * (dqk + dv)]
    np.testing.assert_allclose(gp.numpy()[..., qkv], rgp[..., qkv], rtol=1e-4, atol=2e-6)
    assert torch.all(gp[..., 2 * H * dqk:2 * H * dqk + H * dv] == 0)
    np.testing.assert_allclose(gpos.numpy(), rgpos, rtol=1e-4, atol=1e-4 * np.abs(rgpos).max())
    np.testing.assert_allclose(gts.numpy(), rgts, rtol=1e-4, atol=1e-4 * max(np.abs(rgts).max(), 1e-30))


@pytest.mark.parametrize("cfg", BUCKET_CFGS)
def test_kernel_time_buckets_match_torch_cpu(cfg):
    """Sample b has L = 2 and time diffs (dt_b, 0): query 1 sees key 0 at delta -dt_b.  With q = k = 0, pos_w = 0,
    ts_w[c] = c and v = (1, 0), the output of query 1 is silu(bucket) / N, which reveals the bucket exactly."""
    from torch_rechub_amd import ops
    nb, fn, div, unit = cfg
    dt = torch.from_numpy(adversarial_deltas(div, fn, unit))
    B, N = dt.numel(), 2
    td = torch.stack([dt, torch.zeros_like(dt)], 1).to(dev())
    proj = torch.zeros(B, 2, 4, device=dev())  # H = 1, dqk = dv = 1: [q | k | u | v]
    proj[:, 0, 3] = 1.0
    pos_w = torch.zeros(2 * N - 1, 1, device=dev())
    ts_w = torch.arange(nb + 1, dtype=torch.float32, device=dev())[:, None]
    out = ops.hstu_attention(proj, pos_w, ts_w, 1, 1, 1, N, time_diffs=td, num_time_buckets=nb, time_bucket_fn=fn,
                             time_bucket_divisor=div, time_bucket_unit=unit)[:, 1, 0]
    table = torch.nn.functional.silu(ts_w[:, 0]) / N
    got = torch.searchsorted(table, out - 1e-7 * table[-1]).cpu()
    want = bucketize_time(-dt, nb, fn, div, unit)
    assert torch.equal(got, want), int((got != want).sum())


@pytest.mark.parametrize("V", [3707, 100003])
@pytest.mark.parametrize("t2", [None, 0.1])
def test_head_kernel_against_float64(V, t2):
    from torch_rechub_amd import ops
    g = torch.Generator().manual_seed(V)
    M, D, t1 = 700, 50, 0.05
    h = torch.nn.functional.normalize(torch.randn(M, D, generator=g), dim=-1)
    w = torch.nn.functional.normalize(torch.randn(V, D, generator=g), dim=-1)
    b = 0.1 * torch.randn(V, generator=g)
    labels = torch.randint(1, V, (M,), generator=g)
    labels[::7] = 0
    hd, wd, bd = (t.to(dev()).requires_grad_(True) for t in (h, w, b))
    loss = ops.next_token_loss(hd, wd, bd, labels.to(dev()), temperature=t1, nce_temperature=t2)
    loss.backward()
    rl, rdh, rdw, rdb = np_head(h.numpy(), w.numpy(), b.numpy(), labels.numpy(), t1, t2)
    assert abs(loss.item() - rl) <= 1e-5 * abs(rl)
    for got, want in ((hd.grad, rdh), (wd.grad, rdw), (bd.grad, rdb)):
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=2e-4, atol=2e-4 * np.abs(want).max())
    assert torch.all(wd.grad[0] == 0) and bd.grad[0] == 0


@pytest.mark.parametrize("t2", [None, 0.1])
def test_head_all_rows_ignored(t2):
    from torch_rechub_amd import ops
    g = torch.Generator().manual_seed(3)
    M, D, V = 70, 20, 130
    h, w = torch.randn(M, D, generator=g), torch.randn(V, D, generator=g)
    labels = torch.zeros(M, dtype=torch.long)
    hd, wd = h.to(dev()).requires_grad_(True), w.to(dev()).requires_grad_(True)
    loss = ops.next_token_loss(hd, wd, None, labels.to(dev()), temperature=1.0, nce_temperature=t2)
    rl, rdh, rdw, _ = np_head(h.numpy(), w.numpy(), None, labels.numpy(), 1.0, t2)
    if t2 is None:  # nn.CrossEntropyLoss: NaN loss, zero gradients (nothing is selected)
        assert torch.isnan(loss)
        loss.backward()
        assert torch.all(hd.grad == 0) and torch.all(wd.grad == 0)
        return
    assert abs(loss.item() - rl) <= 1e-6 * abs(rl)
    loss.backward()
    np.testing.assert_allclose(hd.grad.cpu().numpy(), rdh, rtol=2e-4, atol=2e-4 * np.abs(rdh).max())
    np.testing.assert_allclose(wd.grad.cpu().numpy(), rdw, rtol=2e-4, atol=2e-4 * np.abs(rdw).max())


def test_backwards_are_bitwise_repeatable():
    from torch_rechub_amd import ops
    B, L, H, dqk, dv, N, nb = 8, 200, 2, 50, 50, 200, 128
    proj, pos_w, ts_w, td, mask = attn_inputs(B, L, H, dqk, dv, N, nb, seed=9)
    gout = torch.randn(B, L, H * dv, generator=torch.Generator().manual_seed(2))
    a = run_attn(proj, pos_w, ts_w, td, mask, H, dqk, dv, N, nb, "log", 0.301, "seconds", gout)
    b = run_attn(proj, pos_w, ts_w, td, mask, H, dqk, dv, N, nb, "log", 0.301, "seconds", gout)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    g = torch.Generator().manual_seed(4)
    h, w, bias = torch.randn(3000, 50, generator=g), torch.randn(3707, 50, generator=g), torch.randn(3707, generator=g)
    labels = torch.randint(0, 3707, (3000,), generator=g).to(dev())
    grads = []
    for _ in range(2):
        ts = [t.to(dev()).requires_grad_(True) for t in (h, w, bias)]
        ops.next_token_loss(*ts, labels, temperature=0.05).backward()
        grads.append([t.grad.cpu() for t in ts])
    for x, y in zip(*grads):
        assert torch.equal(x, y)


def np_model_loss(model, tokens, td, targets, loss_type, nce_t):
    """float64 restatement of HSTUModel + SeqTrainer._compute_next_token_loss from the model's parameters."""
    from test_hstu_host import np_attention as npa
    P = {k: v.detach().cpu().double().numpy() for k, v in model.state_dict().items()}
    tok, tdn = tokens.numpy(), td.numpy()
    B, L = tok.shape
    keep = tok != 0
    x = P["token_embedding.weight"][tok] + P["position_embedding.weight"][:L][None]
    if model.use_time_embedding:
        x = x + P["time_embedding.weight"][model._time_diff_to_bucket(td).numpy()]
    x = x * keep[..., None]

    def ln(v, wgt, bias):
        mu = v.mean(-1, keepdims=True)
        var = ((v - mu)**2).mean(-1, keepdims=True)
        return (v - mu) / np.sqrt(var + 1e-5) * wgt + bias

    for li, layer in enumerate(model.hstu_block.layers):
        p = f"hstu_block.layers.{li}."
        z = ln(x, P[p + "norm_in.weight"], P[p + "norm_in.bias"]) @ P[p + "proj1.weight"].T + P[p + "proj1.bias"]
        proj = z / (1 + np.exp(-z))
        H, dqk, dv = layer.n_heads, layer.dqk, layer.dv
        att, _ = npa(proj, P[p + "rab.pos_w"], P[p + "rab.ts_w"], tdn, keep, H, dqk, dv, layer.max_seq_len,
                     layer.rab.num_time_buckets, layer.rab.time_bucket_fn, layer.rab.time_bucket_divisor,
                     layer.rab.time_bucket_unit)
        u = proj[..., 2 * H * dqk:2 * H * dqk + H * dv]
        gated = ln(att, P[p + "norm_attn.weight"], P[p + "norm_attn.bias"]) * u
        x = x + gated @ P[p + "proj2.weight"].T + P[p + "proj2.bias"]
    x = x * keep[..., None]
    if model.tie_embeddings:
        w, b = P["token_embedding.weight"], P.get("output_bias")
    else:
        w, b = P["output_projection.weight"], P.get("output_projection.bias")
    if model.score_norm == "l2":
        x = x / np.maximum(np.linalg.norm(x, axis=-1, keepdims=True), model.l2_norm_eps)
        w = w / np.maximum(np.linalg.norm(w, axis=-1, keepdims=True), model.l2_norm_eps)
    nxt = np.concatenate([tok[:, 1:], targets.numpy()[:, None]], 1) * keep
    return np_head(x.reshape(B * L, -1), w, b, nxt.ravel(), model.temperature, nce_t if loss_type == "nce" else None)[0]


@pytest.mark.parametrize("cfg", [dict(tie_embeddings=True, score_norm="l2", temperature=0.05, loss_type="cross_entropy"),
                                 dict(tie_embeddings=False, score_norm="none", temperature=1.0, use_output_bias=False,
                                      loss_type="nce", time_bucket_fn="log", time_bucket_divisor=0.301,
                                      time_bucket_unit="seconds")])
def test_model_step_against_float64_and_graph_free_trainer(cfg):
    from torch_rechub_amd.models.generative import HSTUModel
    from torch_rechub_amd.trainers import SeqTrainer
    cfg = dict(cfg)
    loss_type = cfg.pop("loss_type")
    torch.manual_seed(0)
    V, B, L = 300, 6, 20
    model = HSTUModel(V, d_model=24, n_heads=2, n_layers=2, dqk=12, dv=10, max_seq_len=24, dropout=0.0,
                      num_time_buckets=16, **cfg)
    with torch.no_grad():
        for n, p in model.named_parameters():
            if "bias" in n or "rab" in n:
                p.add_(0.05 * torch.randn_like(p))
        model.token_embedding.weight[0].zero_()
    g = torch.Generator().manual_seed(1)
    tokens = torch.randint(1, V, (B, L), generator=g)
    tokens[0, :7] = 0
    tokens[1, 15:] = 0
    td = torch.sort(torch.randint(0, 10**6, (B, L), generator=g), 1, descending=True).values
    targets = torch.randint(1, V, (B,), generator=g)
    want = np_model_loss(model, tokens, td, targets, loss_type, 0.1)
    trainer = SeqTrainer(model, device="cuda:0", loss_type=loss_type, optimizer_params={"lr": 1e-3})
    got = trainer._loss(tokens.to(dev()), td.to(dev()), targets.to(dev()))
    assert abs(got.item() - want) <= 1e-4 * abs(want), (got.item(), want)
    # the fused loss equals the reference formula on the materialised logits
    ref = trainer._compute_next_token_loss(model(tokens.to(dev()), td.to(dev())), tokens.to(dev()), targets.to(dev()))
    assert abs(got.item() - ref.item()) <= 1e-4 * abs(ref.item())
    before = {k: v.clone() for k, v in model.state_dict().items()}
    loader = torch.utils.data.DataLoader(torch.utils.data.TensorDataset(tokens, torch.zeros_like(tokens), td, targets),
                                         batch_size=3)
    loss = trainer.train_one_epoch(loader)
    assert np.isfinite(loss)
    assert not torch.equal(before["hstu_block.layers.0.rab.pos_w"], model.state_dict()["hstu_block.layers.0.rab.pos_w"])
    vl, acc = trainer.evaluate(loader)
    assert np.isfinite(vl) and 0.0 <= acc <= 1.0


def test_fused_step_memory_below_logits():
    from torch_rechub_amd.models.generative import HSTUModel
    from torch_rechub_amd.trainers import SeqTrainer
    torch.manual_seed(0)
    B, L, V = 128, 200, 100003
    model = HSTUModel(V, d_model=50, n_heads=1, n_layers=2, dqk=50, dv=50, max_seq_len=L, dropout=0.0, score_norm="l2",
                      temperature=0.05)
    trainer = SeqTrainer(model, device="cuda:0")
    g = torch.Generator().manual_seed(0)
    tokens = torch.randint(1, V, (B, L), generator=g).to(dev())
    td = torch.randint(0, 10**6, (B, L), generator=g).to(dev())
    tg = torch.randint(1, V, (B,), generator=g).to(dev())
    trainer.train_step(tokens, td, tg)  # optimizer state exists from here on
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    trainer.train_step(tokens, td, tg)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    assert extra < 0.25 * B * L * V * 4, extra


# ---- layers and models against the reference's fixtures (tools/gen_golden_hstu.py) ------------------------------------
LAYER_CFGS = {"none": None, "sqrt_min": ("sqrt", 1.0, "minutes"), "log_sec": ("log", 0.301, "seconds")}
MODEL_CFGS = ["tied_l2_ce", "untied_none_nce", "tied_none_t2_nobias_ce", "untied_l2_bias_nce"]


def close(got, want, what, rtol=2e-4, atol_rel=2e-5):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    scale = max(float(np.abs(want).max()), 1e-12)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol_rel * scale, err_msg=what)


@pytest.mark.parametrize("kind", ["layer", "block"])
@pytest.mark.parametrize("cfg", list(LAYER_CFGS))
def test_layers_against_reference_fixture(kind, cfg):
    from conftest import golden_state, load_golden
    from torch_rechub_amd.basic.layers import HSTUBlock, HSTULayer
    gold = load_golden("hstu_layers.npz")
    fn, div, unit = LAYER_CFGS[cfg] or ("sqrt", 1.0, "minutes")
    kw = dict(num_time_buckets=16, time_bucket_fn=fn, time_bucket_divisor=div, time_bucket_unit=unit)
    m = HSTULayer(24, 2, 12, 10, 0.0, 12, **kw) if kind == "layer" else HSTUBlock(24, 2, 2, 12, 10, 0.0, 12, **kw)
    k = f"{kind}.{cfg}."
    m.load_state_dict(golden_state(gold, k + "sd."))
    m.to(dev())
    x = torch.from_numpy(gold[k + "x"]).to(dev()).requires_grad_(True)
    mask = torch.from_numpy(gold["mask"]).to(dev())
    td = torch.from_numpy(gold["time_diffs"]).to(dev()) if LAYER_CFGS[cfg] else None
    y = m(x, padding_mask=mask, time_diffs=td)
    close(y, gold[k + "out"], k + "out")
    y.backward(torch.from_numpy(gold[k + "g_out"]).to(dev()))
    close(x.grad, gold[k + "g_x"], k + "g_x")
    for n, p in m.named_parameters():
        close(p.grad, gold[k + "grad." + n], k + "grad." + n, rtol=5e-4, atol_rel=5e-5)


def fixture_model(gold, **extra):
    import json
    from conftest import golden_state
    from torch_rechub_amd.models.generative import HSTUModel
    kw = json.loads(str(gold["cfg"]))
    loss_type = kw.pop("loss_type")
    model = HSTUModel(40, d_model=24, n_heads=2, n_layers=2, dqk=12, dv=10, max_seq_len=12, dropout=0.0,
                      num_time_buckets=16, **kw)
    model.load_state_dict(golden_state(gold, "sd0."))
    assert list(model.state_dict()) == [str(s) for s in gold["sd_keys"]]
    return model, loss_type


def fixture_batches(gold):
    return [tuple(torch.from_numpy(gold[f"b{i}.{n}"]) for n in ("tokens", "positions", "time_diffs", "targets"))
            for i in range(3)]


@pytest.mark.parametrize("cfg", MODEL_CFGS)
def test_model_and_seq_trainer_against_reference_fixture(cfg):
    from conftest import assert_state_follows_reference_trajectory, load_golden
    from torch_rechub_amd.trainers import SeqTrainer
    gold = load_golden(f"model_hstu_{cfg}.npz")
    model, loss_type = fixture_model(gold)
    lr, wd = float(gold["train.lr"]), float(gold["train.wd"])
    trainer = SeqTrainer(model, device="cuda:0", loss_type=loss_type, optimizer_params={"lr": lr, "weight_decay": wd})
    batches = fixture_batches(gold)
    tok, _, td, tg = (t.to(dev()) for t in batches[0])
    model.eval()
    with torch.no_grad():
        close(model(tok, td), gold["logits"], "logits")
    model.train()
    loss = trainer._loss(tok, td, tg)  # the fused next-token loss
    assert abs(loss.item() - float(gold["loss"])) <= 2e-5 * abs(float(gold["loss"])), (loss.item(), float(gold["loss"]))
    model.zero_grad()
    loss.backward()
    for n, p in model.named_parameters():
        close(p.grad, gold["grad." + n], cfg + " grad." + n, rtol=1e-3, atol_rel=1e-4)
    model.zero_grad(set_to_none=True)
    mean_loss = trainer.train_one_epoch(batches)
    assert abs(mean_loss - float(gold["train.mean_loss"])) <= 1e-4 * abs(float(gold["train.mean_loss"]))
    assert_state_follows_reference_trajectory(gold, model.state_dict(), cfg)
    ev_loss, ev_acc = trainer.evaluate(batches)
    assert abs(ev_loss - float(gold["eval.loss"])) <= 1e-3 * abs(float(gold["eval.loss"]))
    assert abs(ev_acc - float(gold["eval.accuracy"])) <= 1.0 / 18 + 1e-12


def test_graph_step_equals_eager_step_bitwise():
    """SeqTrainer(use_graph=True): two eager warm-up steps, then the captured step replayed for every later batch of the
    same shape; the state after each step is bitwise the eager twin's (same capturable Adam)."""
    from conftest import load_golden
    from torch_rechub_amd.trainers import SeqTrainer
    gold = load_golden("model_hstu_tied_l2_ce.npz")
    batches = fixture_batches(gold) * 2
    twins = []
    for use_graph in (False, True):
        model, loss_type = fixture_model(gold)
        twins.append(SeqTrainer(model, device="cuda:0", loss_type=loss_type, use_graph=use_graph,
                                optimizer_params={"lr": 1e-2, "weight_decay": 1e-5, "capturable": True}))
    eager, graph = twins
    for i, b in enumerate(batches):
        args = tuple(t.to(dev()) for t in (b[0], b[2], b[3]))
        le = eager.train_step(*args)
        lg = graph.train_step(*args)
        assert torch.equal(le, lg), i
        for (k, v), w in zip(eager.model.state_dict().items(), graph.model.state_dict().values()):
            assert torch.equal(v, w), (i, k)
    assert len(graph._graphs) == 1


def test_attention_step_memory_below_one_score_tensor():
    """L = 512, H = 8: one fused step's peak above the model and optimizer state stays below one (B, H, L, L) fp32."""
    from torch_rechub_amd.models.generative import HSTUModel
    from torch_rechub_amd.trainers import SeqTrainer
    torch.manual_seed(0)
    B, L, V = 64, 512, 2000
    model = HSTUModel(V, d_model=128, n_heads=8, n_layers=2, dqk=16, dv=16, max_seq_len=L, dropout=0.0)
    trainer = SeqTrainer(model, device="cuda:0")
    g = torch.Generator().manual_seed(0)
    tok = torch.randint(1, V, (B, L), generator=g).to(dev())
    td = torch.sort(torch.randint(0, 10**7, (B, L), generator=g), 1, descending=True).values.to(dev())
    tg = torch.randint(1, V, (B,), generator=g).to(dev())
    trainer.train_step(tok, td, tg)
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    trainer.train_step(tok, td, tg)
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    assert extra < B * 8 * L * L * 4, extra


def test_out_of_range_label_raises():
    from torch_rechub_amd import ops
    h, w = torch.randn(10, 8, device=dev()), torch.randn(30, 8, device=dev())
    labels = torch.arange(10, device=dev())
    labels[4] = 30
    ops.next_token_loss(h, w, None, labels)
    with pytest.raises(IndexError, match="target label"):
        ops.check_errors(dev())


def test_empty_batch_attention():
    from torch_rechub_amd import ops
    proj = torch.zeros(0, 5, 2 * 2 * (4 + 3), device=dev(), requires_grad=True)
    pos_w = torch.zeros(2 * 8 - 1, 2, device=dev(), requires_grad=True)
    ts_w = torch.zeros(17, 2, device=dev(), requires_grad=True)
    out = ops.hstu_attention(proj, pos_w, ts_w, 2, 4, 3, 8, time_diffs=torch.zeros(0, 5, dtype=torch.long, device=dev()),
                             num_time_buckets=16)
    assert out.shape == (0, 5, 6)
    out.sum().backward()
    assert torch.all(pos_w.grad == 0) and torch.all(ts_w.grad == 0)
