"""The two-tower tails on the MI355X: the three kernel pairs of csrc/twotower.hip against the float64 restatement
(tests/twotower_oracle.py, pinned to the reference by tests/test_twotower_host.py) at the smallest shapes where each thing can
go wrong, repeatable backwards, refused shapes, and FaceBookDSSM, YoutubeSBC and the SENet DSSM against the reference's
fixtures (tools/gen_golden_twotower.py): eval outputs, tower modes, probe loss and gradients, three Adam steps, a captured
train step, YoutubeSBC through its short batch, the in-batch mode and top-k retrieval.

Tolerances are the project's kernel convention (test_gpu_sine.py, test_gpu_interest.py): rtol 1e-4, atol 1e-5 of the tensor's
largest magnitude.  Gradients of rows whose norm eps clamped are ~1e8 times the others: those tensors are compared row by row
under the same rule, which is the stricter reading.
"""
import ctypes

import numpy as np
import pytest
import torch

import twotower_oracle as O
from conftest import assert_state_follows_reference_trajectory, golden_batch, golden_state, load_golden
from test_twotower_host import MODELS, build

pytestmark = pytest.mark.gpu

WIDTHS = [1, 63, 64, 65, 128, 1024]


def dev():
    return torch.device("cuda:0")


def close(got, want, what, rows=False):
    got = got.detach().cpu().numpy().astype(np.float64) if torch.is_tensor(got) else np.asarray(got, np.float64)
    want = np.asarray(want, np.float64)
    assert got.shape == want.shape, f"{what}: {got.shape} != {want.shape}"
    assert np.isfinite(got).all(), what
    if rows:
        for r in range(want.shape[0]):
            np.testing.assert_allclose(got[r], want[r], rtol=1e-4, atol=1e-5 * float(np.abs(want[r]).max()) + 1e-30,
                                       err_msg=f"{what} row {r}")
    else:
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-5 * float(np.abs(want).max()) + 1e-30, err_msg=what)


def rows_per_trip():
    """Rows one trip of the capped launches covers (the cap's workgroups x four wavefronts)."""
    from torch_rechub_amd import _lib
    return 4 * _lib.query("rh_twotower_nblocks", 1 << 30)


def strided(t, pad=3):
    """The same values as rows of a wider buffer (row stride D + pad), on the device."""
    wide = torch.full((t.shape[0], t.shape[1] + pad), float("nan"))
    wide[:, :t.shape[1]] = t
    return wide.to(dev())[:, :t.shape[1]]


# ---- band logits ---------------------------------------------------------------------------------------------------------
def band_case(B, D, n_neg, seed, w=None):
    g = torch.Generator().manual_seed(seed)
    u, v = torch.randn(B, D, generator=g), torch.randn(B, D, generator=g)
    w = 0.05 + 0.95 * torch.rand(B, generator=g) if w is None else torch.full((B,), float(w))
    return u, v, w, torch.randn(B, n_neg + 1, generator=g)


def run_band(u, v, w, gl, n_neg, temp, stride=False):
    from torch_rechub_amd import ops
    ud = (strided(u) if stride else u.to(dev())).requires_grad_(True)
    vd = (strided(v, 5) if stride else v.to(dev())).requires_grad_(True)
    logits = ops.band_logits(ud, vd, w.to(dev()), n_neg, temp)
    logits.backward(gl.to(dev()))
    return logits, ud.grad, vd.grad


def check_band(u, v, w, gl, n_neg, temp, rows=False, **kw):
    logits, g_u, g_v = run_band(u, v, w, gl, n_neg, temp, **kw)
    close(logits, O.band_forward(u, v, w, n_neg, temp), "logits")
    want_u, want_v = O.band_backward(u, v, gl, n_neg, temp)
    close(g_u, want_u, "g_u", rows)
    close(g_v, want_v, "g_v", rows)
    return g_u, g_v


@pytest.mark.parametrize("B,n_neg", [(1, 0), (4, 3), (5, 3), (7, 2), (48, 3)])
def test_band_logits_against_float64_over_batch_shapes(B, n_neg):
    """(4, 3): every row wraps; (5, 3) / (7, 2): a partial last workgroup; every item row is hit by all 1 + n_neg user rows."""
    check_band(*band_case(B, 12, n_neg, 100 + B), n_neg, 0.2)


@pytest.mark.parametrize("D", WIDTHS)
def test_band_logits_against_float64_over_widths_strided(D):
    check_band(*band_case(7, D, 2, 200 + D), 2, 0.5, stride=True)


def test_band_logits_past_the_grid_caps_first_trip():
    B = rows_per_trip() + 1
    check_band(*band_case(B, 4, 3, 7), 3, 0.2)


@pytest.mark.parametrize("w", [1.0, 1e-30])
def test_band_logits_unit_and_tiny_sample_weights(w):
    u, v, wt, gl = band_case(9, 16, 3, 11, w=w)
    logits, _, _ = run_band(u, v, wt, gl, 3, 0.02)
    close(logits, O.band_forward(u, v, wt, 3, 0.02), "logits")


def test_band_logits_zero_and_sub_eps_rows_follow_the_recorded_rule():
    """The reference's own recorded case (zero rows and rows of norm 1e-9 in u and v), then a random one at width 65."""
    gold = load_golden("twotower_layers.npz")
    c = {k[6:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("band1.")}
    logits, g_u, g_v = run_band(c["u"], c["v"], c["w"], c["g"], int(c["n_neg"]), float(c["temperature"]))
    close(logits, gold["band1.logits"], "logits vs reference")
    close(g_u, gold["band1.g_u"], "g_u vs reference", rows=True)
    close(g_v, gold["band1.g_v"], "g_v vs reference", rows=True)
    u, v, w, gl = band_case(6, 65, 2, 5)
    u[1], v[4] = 0, 0
    u[3] *= 1e-9 / u[3].norm()
    g_u, g_v = check_band(u, v, w, gl, 2, 0.5, rows=True)
    assert torch.isfinite(g_u).all() and torch.isfinite(g_v).all()


def test_band_logits_backward_twice_is_bitwise_equal():
    u, v, w, gl = band_case(rows_per_trip() // 8 + 3, 65, 3, 3)
    a, b = run_band(u, v, w, gl, 3, 0.2), run_band(u, v, w, gl, 3, 0.2)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def _raw():
    from torch_rechub_amd import _lib
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    return _lib, p, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream), ctypes.c_void_p(0)


def test_band_logits_refusals_touch_nothing():
    _lib, p, st, null = _raw()
    x = torch.randn(4, 1025, device=dev())
    w = torch.ones(4, device=dev())
    out = torch.full((4, 1025), 7.0, device=dev())
    out2 = torch.full((4, 1025), 7.0, device=dev())
    n = torch.full((2, 4), 7.0, device=dev())
    bad = [(4, 1025, 2), (4, 8, 5)]  # D = 1025; K1 > B
    for B, D, K1 in bad:
        with pytest.raises(RuntimeError, match="rc=-2"):
            _lib.call("rh_band_logits_fwd", p(x), 1025, p(x), 1025, p(w), B, D, K1, 1.0, 1e-8, p(out), p(n[0]), p(n[1]), st)
        with pytest.raises(RuntimeError, match="rc=-2"):
            _lib.call("rh_band_logits_bwd", p(x), 1025, p(x), 1025, p(w), p(w), p(x), B, D, K1, 1.0, 1e-8, p(out), p(out2), st)
    with pytest.raises(RuntimeError, match="rc=-1"):
        _lib.call("rh_band_logits_fwd", p(x), 1025, null, 1025, p(w), 4, 8, 2, 1.0, 1e-8, p(out), p(n[0]), p(n[1]), st)
    with pytest.raises(RuntimeError, match="rc=-1"):
        _lib.call("rh_band_logits_bwd", p(x), 1025, p(x), 1025, p(w), p(w), p(x), 4, 8, 2, 1.0, 1e-8, null, p(out2), st)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (out2 == 7.0).all() and (n == 7.0).all()
    from torch_rechub_amd import ops
    assert not ops.band_logits_ok(x, x, w, 1) and not ops.band_logits_ok(x[:, :8], x[:, :8], w, 4)
    assert ops.band_logits_ok(x[:, :8], x[:, :8], w, 3)


# ---- pair cosine ---------------------------------------------------------------------------------------------------------
def run_pair(hu, hp, hn, gp, gn, stride=False):
    from torch_rechub_amd import ops
    ts = [(strided(t, 1 + i) if stride else t.to(dev())).requires_grad_(True) for i, t in enumerate((hu, hp, hn))]
    pos, neg = ops.pair_cosine_scores(*ts)
    torch.autograd.backward([pos, neg], [gp.to(dev()), gn.to(dev())])
    return pos, neg, [t.grad for t in ts]


def pair_case(B, D, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(B, D, generator=g) for _ in range(3)] + [torch.randn(B, generator=g) for _ in range(2)]


def check_pair(hu, hp, hn, gp, gn, rows=False, **kw):
    pos, neg, grads = run_pair(hu, hp, hn, gp, gn, **kw)
    want_pos, want_neg = O.pair_forward(hu, hp, hn)
    close(pos, want_pos, "pos")
    close(neg, want_neg, "neg")
    for got, want, name in zip(grads, O.pair_backward(hu, hp, hn, gp, gn), ("g_hu", "g_hp", "g_hn")):
        close(got, want, name, rows)
    return pos, neg, grads


@pytest.mark.parametrize("B", [1, 7, 48])
@pytest.mark.parametrize("D", WIDTHS)
def test_pair_cosine_against_float64(D, B):
    check_pair(*pair_case(B, D, 300 + D + B), stride=B == 7)


def test_pair_cosine_zero_rows_and_identical_items():
    gold = load_golden("twotower_layers.npz")
    c = {k[6:]: torch.from_numpy(gold[k]) for k in gold.files if k.startswith("pair1.")}
    pos, neg, grads = run_pair(c["hu"], c["hp"], c["hn"], c["g_pos"], c["g_neg"])
    close(pos, gold["pair1.pos"], "pos vs reference")
    close(neg, gold["pair1.neg"], "neg vs reference")
    for got, name in zip(grads, ("g_hu", "g_hp", "g_hn")):
        close(got, gold["pair1." + name], name + " vs reference", rows=True)
    hu, hp, hn, gp, gn = pair_case(7, 65, 9)
    hu[0], hp[1], hn[2] = 0, 0, 0
    check_pair(hu, hp, hn, gp, gn, rows=True)
    pos, neg, grads = run_pair(hu, hp, hp.clone(), gp, gp)
    assert torch.equal(pos, neg) and torch.equal(grads[1], grads[2])
    a, b = run_pair(hu, hp, hn, gp, gn), run_pair(hu, hp, hn, gp, gn)
    assert all(torch.equal(x, y) for x, y in zip(a[2], b[2]))


def test_pair_cosine_refusals_touch_nothing():
    _lib, p, st, null = _raw()
    x = torch.randn(3, 1025, device=dev())
    out = torch.full((3, 3, 1025), 7.0, device=dev())
    with pytest.raises(RuntimeError, match="rc=-2"):
        _lib.call("rh_pair_cosine_fwd", p(x), 1025, p(x), 1025, p(x), 1025, 3, 1025, 1e-12, p(out[0]), p(out[1]), p(out[2]), st)
    with pytest.raises(RuntimeError, match="rc=-2"):
        _lib.call("rh_pair_cosine_bwd", p(x), 1025, p(x), 1025, p(x), 1025, p(x), p(x), p(x), 3, 1025, 1e-12, p(out[0]), p(out[1]),
                  p(out[2]), st)
    with pytest.raises(RuntimeError, match="rc=-1"):
        _lib.call("rh_pair_cosine_fwd", p(x), 1025, p(x), 1025, null, 1025, 3, 8, 1e-12, p(out[0]), p(out[1]), p(out[2]), st)
    torch.cuda.synchronize()
    assert (out == 7.0).all()


# ---- SENET gate ------------------------------------------------------------------------------------------------------------
SENET_SHAPES = [(1, 1, 1), (3, 1, 16), (7, 2, 16), (64, 21, 4), (5, 1, 256)]


def senet_case(B, F, R, D, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, F, D, generator=g)
    w1, w2 = torch.randn(R, F, generator=g) * 0.6 + 0.2, torch.randn(F, R, generator=g) * 0.6 + 0.2
    return x, w1, w2, torch.randn(B, F, D, generator=g)


def run_senet(x, w1, w2, gy, stride=False):
    from torch_rechub_amd import ops
    B, F, D = x.shape
    w1d, w2d = w1.to(dev()).requires_grad_(True), w2.to(dev()).requires_grad_(True)
    if stride:  # the (B, F D) block inside a wider buffer, as the fused gather's output with dense columns behind it
        xd = strided(x.reshape(B, F * D), 5).requires_grad_(True)
        y = ops.senet(xd.as_strided((B, F, D), (xd.stride(0), D, 1)), w1d, w2d)
    else:
        xd = x.to(dev()).requires_grad_(True)
        y = ops.senet(xd, w1d, w2d)
    y.backward(gy.to(dev()))
    return y, xd.grad.reshape(B, F, D), w1d.grad, w2d.grad


def check_senet(x, w1, w2, gy, **kw):
    y, g_x, g_w1, g_w2 = run_senet(x, w1, w2, gy, **kw)
    close(y, O.senet_forward(x, w1, w2), "y")
    want_x, want_w1, want_w2 = O.senet_backward(x, w1, w2, gy)
    close(g_x, want_x, "g_x")
    close(g_w1, want_w1, "g_w1")
    close(g_w2, want_w2, "g_w2")


@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("FRD", SENET_SHAPES, ids=lambda v: "F%dR%dD%d" % v)
def test_senet_against_float64(FRD, B):
    check_senet(*senet_case(B, *FRD, seed=400 + B + sum(FRD)), stride=B == 9)


def test_senet_past_the_grid_caps_first_trip_and_twice_bitwise():
    c = senet_case(rows_per_trip() + 1, 7, 2, 16, 17)
    check_senet(*c)
    a, b = run_senet(*c), run_senet(*c)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_senet_closed_gate_gives_exact_zeros():
    """Positive first-layer weights and an all-negative sample: every hidden unit is <= 0, the gate is exactly 0 and that
    sample contributes exact zeros to g_x and to both weight gradients (alone in a batch: the gradients ARE zero)."""
    x, w1, w2, gy = senet_case(6, 7, 2, 16, 23)
    w1 = w1.abs()
    x[1] = -x[1].abs()
    x[4] = 0
    y, g_x, g_w1, g_w2 = run_senet(x, w1, w2, gy)
    assert not y[1].any() and not g_x[1].any() and not y[4].any() and not g_x[4].any()
    check_senet(x, w1, w2, gy)
    y, g_x, g_w1, g_w2 = run_senet(x[1:2], w1, w2, gy[1:2])
    assert not y.any() and not g_x.any() and not g_w1.any() and not g_w2.any()


def test_senet_refusals_touch_nothing():
    from torch_rechub_amd import ops
    _lib, p, st, null = _raw()
    x = torch.randn(2, 65 * 257, device=dev())
    w = torch.randn(65, 65, device=dev())
    out = torch.full((2, 65 * 257), 7.0, device=dev())
    small = torch.full((3, 2, 65), 7.0, device=dev())
    part = torch.full((1, 2 * 65 * 65), 7.0, device=dev())
    ld = x.stride(0)
    for F, R, D in [(65, 2, 4), (4, 2, 257), (4, 5, 4)]:
        with pytest.raises(RuntimeError, match="rc=-2"):
            _lib.call("rh_senet_fwd", p(x), ld, p(w), p(w), 2, F, R, D, p(out), p(small[0]), p(small[1]), p(small[2]), st)
        with pytest.raises(RuntimeError, match="rc=-2"):
            _lib.call("rh_senet_bwd", p(x), ld, p(w), p(w), p(x), p(x), p(x), p(x), ld, 2, F, R, D, p(out), p(part), st)
    with pytest.raises(RuntimeError, match="rc=-1"):
        _lib.call("rh_senet_fwd", p(x), ld, null, p(w), 2, 4, 2, 4, p(out), p(small[0]), p(small[1]), p(small[2]), st)
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (small == 7.0).all() and (part == 7.0).all()
    x3 = x[:, :65 * 4].view(2, 65, 4)
    assert not ops.senet_ok(x3, w[:2], w[:, :2]) and ops.senet_ok(x3[:, :64], w[:2, :64], w[:64, :2])


# ---- the models against the reference's fixtures ------------------------------------------------------------------------------
def load_model(cfg):
    gold = load_golden(f"model_{cfg}.npz")
    model = build(cfg, gold)
    model.load_state_dict(golden_state(gold, "sd0."))
    return gold, model.to(dev())


def to_dev(x):
    return {k: v.to(dev()) for k, v in x.items()}


def probe_loss(cfg, model, x, y):
    from torch_rechub_amd.basic.loss_func import BPRLoss
    pred = model(x)
    if cfg == "facebook_dssm":
        return BPRLoss()(pred[0], pred[1]), pred
    if cfg == "youtube_sbc":
        return torch.nn.functional.cross_entropy(pred, y.long()), pred
    return torch.nn.functional.binary_cross_entropy(pred, y.float()), pred


def put(gold, key, pred):
    return [(pred[0], gold[key + "_pos"]), (pred[1], gold[key + "_neg"])] if isinstance(pred, tuple) else [(pred, gold[key])]


@pytest.mark.parametrize("cfg", MODELS)
def test_eval_outputs_and_tower_modes_match_the_reference(cfg):
    gold, model = load_model(cfg)
    model.eval()
    x = to_dev(golden_batch(gold, 0)[0])
    with torch.no_grad():
        for got, want in put(gold, "pred_eval", model(x)):
            close(got, want, "eval output")
        model.mode = "user"
        close(model(x), gold["user_emb"], "mode=user")
        model.mode = "item"
        close(model(x), gold["item_emb"], "mode=item")


def noise_biases(model):
    """Biases of a Linear feeding a BatchNorm1d: their gradient is exactly zero mathematically and rounding noise on either
    side (the rule of test_gpu_models.py)."""
    noise = set()
    for mn, m in model.named_modules():
        if isinstance(m, torch.nn.Sequential):
            mods = list(m)
            noise |= {f"{mn}.{i}.bias" for i in range(len(mods) - 1)
                      if isinstance(mods[i], torch.nn.Linear) and isinstance(mods[i + 1], torch.nn.BatchNorm1d)}
    return noise


@pytest.mark.parametrize("cfg", MODELS)
def test_probe_loss_and_gradients_match_the_reference(cfg):
    gold, model = load_model(cfg)
    model.train()
    x, y = golden_batch(gold, 0)
    loss, pred = probe_loss(cfg, model, to_dev(x), y.to(dev()))
    loss.backward()
    for got, want in put(gold, "pred_train", pred):
        close(got, want, "train output")
    assert abs(loss.item() - float(gold["loss"])) <= 1e-5 * abs(float(gold["loss"]))
    gmax = max(float(np.abs(gold[k]).max()) for k in gold.files if k.startswith("grad."))
    noise = noise_biases(model)
    for n, p in model.named_parameters():
        want = gold["grad." + n]
        got = np.zeros_like(want) if p.grad is None else p.grad.detach().cpu().numpy()
        assert np.isfinite(got).all(), n
        if n in noise:
            bound = 1e-5 * max(gmax, 1e-3) + 1e-6
            assert np.abs(got).max() <= bound and np.abs(want).max() <= bound, n
            continue
        # fp32 against the reference's recorded fp32: the kernel convention's rtol and 1e-4 of the tensor's largest magnitude,
        # what test_gpu_sasrec.py allows a weight gradient summed over the batch.  (The reference's own distance from a
        # float64 evaluation of the same three models is at most 5.5e-6 of a tensor's largest magnitude.)
        np.testing.assert_allclose(got, want, rtol=1e-4, atol=1e-4 * float(np.abs(want).max()), err_msg=n)


def make_trainer(cfg, model, gold, **kw):
    from torch_rechub_amd.trainers import MatchTrainer
    mode = {"facebook_dssm": 1, "youtube_sbc": 2, "dssm_senet": 0}[cfg]
    params = {"lr": float(gold["train.lr"]), "weight_decay": float(gold["train.wd"])}
    return MatchTrainer(model, mode=mode, optimizer_params=params, n_epoch=1, device="cuda:0", show_progress=False, **kw)


@pytest.mark.parametrize("cfg", MODELS)
def test_three_adam_steps_follow_the_reference_trajectory(cfg):
    gold, model = load_model(cfg)
    trainer = make_trainer(cfg, model, gold)
    mean_loss = trainer.train_one_epoch([golden_batch(gold, i) for i in range(3)])
    assert abs(mean_loss - float(gold["train.mean_loss"])) < 5e-5 * max(1.0, abs(float(gold["train.mean_loss"])))
    assert_state_follows_reference_trajectory(gold, model.state_dict(), cfg)


def test_youtube_sbc_short_batch_then_full_batch_match_the_recorded_losses():
    """Steps 4 and 5 of the reference's run: the 10-row batch (the band of a batch of 10: fused) rewrites the index arrays,
    the full batch after it reads them off the band (the torch formulation on the device)."""
    from torch_rechub_amd import ops
    gold, model = load_model("youtube_sbc")
    trainer = make_trainer("youtube_sbc", model, gold)
    trainer.train_one_epoch([golden_batch(gold, i) for i in range(3)])
    calls = []
    orig = ops.band_logits
    ops.band_logits = lambda *a, **k: (calls.append(a[0].shape[0]), orig(*a, **k))[1]
    try:
        loss3 = trainer.train_one_epoch([golden_batch(gold, 3)])
        assert np.array_equal(model.index1, gold["index1_after"]) and np.array_equal(model.index0, gold["index0_after"])
        loss4 = trainer.train_one_epoch([golden_batch(gold, 4)])
    finally:
        ops.band_logits = orig
    assert calls == [10]
    assert abs(loss3 - float(gold["loss_step3"])) <= 1e-4 * abs(float(gold["loss_step3"]))
    assert abs(loss4 - float(gold["loss_step4"])) <= 1e-4 * abs(float(gold["loss_step4"]))
    model.eval()
    with torch.no_grad():
        pred = model(to_dev(golden_batch(gold, 4)[0]))
    np.testing.assert_allclose(pred.cpu().numpy(), gold["pred_eval_after"], rtol=1e-3, atol=1e-3 * np.abs(gold["pred_eval_after"]).max())


def device_loader(gold, order, batch_size):
    """The fixture's full batches ``order`` as one HBM-resident data set."""
    from torch_rechub_amd.utils.data import DeviceDataLoader
    xs = [golden_batch(gold, i) for i in order]
    names, cols, dnames, dcols = [], [], [], []
    for k, v in xs[0][0].items():
        full = torch.cat([x[k] for x, _ in xs], 0)
        if full.dtype == torch.int64:
            names.append(k if full.dim() == 1 else (k, full.shape[1]))
            cols.append(full.reshape(full.shape[0], -1))
        else:
            dnames.append(k)
            dcols.append(full.float().reshape(-1, 1))
    label = torch.cat([y for _, y in xs], 0).float()
    return DeviceDataLoader(torch.cat(cols, 1).contiguous().to(dev()), names,
                            torch.cat(dcols, 1).contiguous().to(dev()) if dcols else None, dnames, label.to(dev()), batch_size,
                            shuffle=False)


@pytest.mark.parametrize("cfg", MODELS)
def test_captured_train_steps_equal_the_eager_ones(cfg):
    """Five steps from one HBM-resident data set: eagerly, and in the trainer's captured form (eager warm-up steps, the
    capture, replays).  The tails are deterministic; the table gradients' float atomics are not, so states are compared as
    trajectories."""
    from conftest import assert_trajectory_close
    order = [0, 1, 2, 0, 1]
    states, losses = [], []
    for use_graph in (False, True):
        gold, model = load_model(cfg)
        trainer = make_trainer(cfg, model, gold, use_graph=use_graph)
        losses.append(trainer.train_one_epoch(device_loader(gold, order, 48)))
        assert (trainer._graph is not None) == use_graph
        states.append({k: v.detach().cpu().numpy() for k, v in model.state_dict().items()})
    assert np.isfinite(losses).all() and abs(losses[0] - losses[1]) <= 1e-4 * abs(losses[0])
    lr, steps = float(gold["train.lr"]), len(order)
    noise = noise_biases(model)
    for k, want in states[0].items():
        got = states[1][k]
        if want.dtype.kind != "f":
            assert np.array_equal(got, want), k
        elif k in noise:  # no defined trajectory under Adam: the sign of rounding noise becomes +-lr steps (conftest's rule)
            assert np.abs(got - want).max() <= 2.1 * lr * steps, k
        elif k.endswith("running_mean"):  # carries the drift of the bias above one-for-one
            assert np.abs(got - want).max() <= 0.5 * lr * steps, k
        else:
            assert_trajectory_close(got, want, lr * steps, f"{cfg}: {k} captured vs eager")


def test_senet_dssm_trains_with_in_batch_negatives():
    from torch_rechub_amd.trainers import MatchTrainer
    gold, model = load_model("dssm_senet")
    trainer = MatchTrainer(model, mode=0, in_batch_neg=True, in_batch_neg_ratio=3, sampler_seed=3,
                           optimizer_params={"lr": 1e-2}, n_epoch=1, device="cuda:0", show_progress=False)
    batches = [golden_batch(gold, 0)] * 4
    first = trainer.train_one_epoch(batches)
    for _ in range(3):
        last = trainer.train_one_epoch(batches)
    assert np.isfinite(first) and np.isfinite(last) and last < first


@pytest.mark.parametrize("cfg", MODELS)
def test_each_fused_tail_runs_once_per_forward_on_the_hip_path(cfg):
    from torch_rechub_amd import ops
    gold, model = load_model(cfg)
    model.train()
    names = ("band_logits", "pair_cosine_scores", "senet")
    calls = {n: 0 for n in names}
    orig = {n: getattr(ops, n) for n in names}

    def counted(n):
        def fn(*a, **k):
            calls[n] += 1
            return orig[n](*a, **k)
        return fn

    x, y = golden_batch(gold, 0)
    try:
        for n in names:
            setattr(ops, n, counted(n))
        probe_loss(cfg, model, to_dev(x), y.to(dev()))[0].backward()
    finally:
        for n in names:
            setattr(ops, n, orig[n])
    want = {"facebook_dssm": {"pair_cosine_scores": 1}, "youtube_sbc": {"band_logits": 1}, "dssm_senet": {"senet": 2}}[cfg]
    assert calls == {n: want.get(n, 0) for n in names}  # (the SENet DSSM has one gate per tower)
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n


@pytest.mark.parametrize("cfg", MODELS)
def test_user_embeddings_through_topk_items_match_dense_topk(cfg):
    from torch_rechub_amd import ops
    gold, model = load_model(cfg)
    model.eval()
    x = to_dev(golden_batch(gold, 0)[0])
    with torch.no_grad():
        model.mode = "user"
        user = model(x).contiguous()
        model.mode = "item"
        items = model(to_dev(golden_batch(gold, 1)[0])).contiguous()  # a 48-item catalogue from the next batch
        ids, scores = ops.topk_items(user, items, 5)
        want = torch.topk(user @ items.t(), 5, dim=1)
    torch.testing.assert_close(scores, want.values, rtol=1e-5, atol=1e-6)
    dense = (user @ items.t()).gather(1, ids)
    torch.testing.assert_close(dense, want.values, rtol=1e-5, atol=1e-6)  # (duplicate items tie: the scores decide)
