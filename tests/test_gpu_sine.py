"""SINE on the MI355X: the kernels of csrc/sine.hip against the float64 restatement of test_sine_host.py at the smallest
shapes where each thing can go wrong, repeatable backwards, the model and three MatchTrainer steps against the
reference's fixture (tools/gen_golden_sine.py) and the captured step against eager.

torch.topk is a discontinuity: a row is compared only if the float64 gap between adjacent scores among its top K + 1,
relative to the row's max |s_u|, is at least 1e-4 -- fp32 rounding of an (S + E)-term score is near 1e-5 relative, a
tenfold margin.  Rows are excluded by the oracle's numbers alone, at most 2 % of them; their upstream gradient is zeroed
on both sides so that the concept table's gradient is compared as a whole.  (Seeds 40-43 exclude none.)

Each kernel's backward gets an upstream gradient of its own, so a comparison checks one kernel.  Tolerances are those of
test_gpu_interest.py for the capsule and pooling kernels: rtol 1e-4, atol 1e-5 of the tensor's largest magnitude;
g_C: atol 1e-4 of it, as the capsule weight gradient there.  The aggregation runs at the example's temperature 0.1."""
import numpy as np
import pytest
import torch

from conftest import assert_state_follows_reference_trajectory, golden_state, load_golden
from test_sine_host import (build_sine, draw_inputs, np_sine_aggregate, np_sine_aggregate_bwd, np_sine_interests,
                            np_sine_interests_bwd, top_k_gap)

pytestmark = pytest.mark.gpu

TEMPERATURE = 0.1
MIN_GAP, MAX_EXCLUDED = 1e-4, 0.02
#          B    S   E    T   K  seed holes
CASES = [(130, 1, 8, 3, 1, 40, False),      # one position, one intention; B not a multiple of any chunk
         (64, 7, 20, 5, 4, 41, False),      # E not a multiple of 4, odd S, K = T - 1
         (33, 64, 128, 64, 8, 42, False),   # every upper limit at once
         (256, 50, 128, 10, 2, 43, False),  # the example's shape
         (64, 7, 20, 5, 4, 41, True)]       # a mask with holes


def dev():
    return torch.device("cuda:0")


def _close(got, want, rows, what, atol_frac=1e-5):
    got, want = got.detach().cpu().numpy()[rows], want[rows]
    assert np.isfinite(got).all(), what
    np.testing.assert_allclose(got, want, rtol=1e-4, atol=atol_frac * float(np.abs(want).max()), err_msg=what)


_ORACLE = {}


def case(B, S, E, T, K, seed, holes):
    """Inputs and the float64 forward of one case, computed once and shared (read-only) by the tests."""
    key = (B, S, E, T, K, seed, holes)
    if key not in _ORACLE:
        inp = draw_inputs(B, S, E, T, K, seed, holes)
        d = {k: v.double().numpy() for k, v in inp.items() if k != "mask"}
        phi, xhat, idx, c1 = np_sine_interests(d["X"], d["Y"], d["a1"], d["a2"], inp["mask"].numpy(), d["C"])
        keep = top_k_gap(c1["s_u"], K) >= MIN_GAP
        assert (~keep).sum() <= MAX_EXCLUDED * B, f"{(~keep).sum()} of {B} rows have a top-k gap below {MIN_GAP}"
        g = torch.Generator().manual_seed(seed + 1000)
        up = dict(g_phi=torch.randn(B, K, E, generator=g) * keep[:, None, None],
                  g_xhat=torch.randn(B, S, E, generator=g) * keep[:, None, None])
        _ORACLE[key] = dict(inp=inp, d=d, phi=phi, xhat=xhat, idx=idx, c1=c1, keep=keep, up=up)
    return _ORACLE[key]


def run_interests(c, grad=True):
    from torch_rechub_amd import ops
    t = {k: c["inp"][k].to(dev()).requires_grad_(grad) for k in ("X", "Y", "a1", "a2", "C")}
    phi, xhat, idx = ops.sine_interests(t["X"], t["Y"], t["a1"], t["a2"], c["inp"]["mask"].to(dev()), t["C"])
    return t, phi, xhat, idx


@pytest.mark.parametrize("B,S,E,T,K,seed,holes", CASES)
def test_interest_kernels_against_float64(B, S, E, T, K, seed, holes):
    c = case(B, S, E, T, K, seed, holes)
    keep, mask = c["keep"], c["inp"]["mask"].numpy()
    assert not mask[0].any() and mask[1].all()
    t, phi, xhat, idx = run_interests(c)
    assert idx.dtype == torch.int32 and not idx.requires_grad
    np.testing.assert_array_equal(idx.cpu().numpy()[keep], c["idx"][keep])
    _close(phi, c["phi"], keep, "phi")
    _close(xhat, c["xhat"], keep, "xhat")
    # the fully padded row: the uniform softmax over S, as float32 makes of a + -1e9
    assert keep[0] and np.allclose(c["c1"]["P1"][0], 1.0 / S) and torch.isfinite(phi[0]).all() and torch.isfinite(xhat[0]).all()
    up = c["up"]
    torch.autograd.backward([phi, xhat], [up["g_phi"].to(dev()), up["g_xhat"].to(dev())])
    want = np_sine_interests_bwd(c["d"]["X"], c["d"]["C"], c["c1"], up["g_phi"].double().numpy(), up["g_xhat"].double().numpy())
    for name, ref in zip(("X", "Y", "a1", "a2"), want[:4]):
        _close(t[name].grad, ref, keep, "g_" + name)
    _close(t["C"].grad, want[4], slice(None), "g_C", atol_frac=1e-4)
    first = {k: v.grad.clone() for k, v in t.items()}
    t2, phi2, xhat2, _ = run_interests(c)
    torch.autograd.backward([phi2, xhat2], [up["g_phi"].to(dev()), up["g_xhat"].to(dev())])
    for k in first:
        assert torch.equal(first[k], t2[k].grad), k


# With the p = -1 normalisation the logits c_apt . phi / 0.1 are in the hundreds and the softmax over K is saturated in all
# but a few rows, where g_xhat and g_a3 vanish.  At temperature 50 the logits are of order one, so the two E = 128 shapes also
# run the gradient through the softmax over K and through the norm (the lane + 64 columns included) in every row.
AGG_CASES = [c + (TEMPERATURE,) for c in CASES] + [CASES[2] + (50.0,), CASES[3] + (50.0,)]


@pytest.mark.parametrize("B,S,E,T,K,seed,holes,TEMPERATURE", AGG_CASES)
def test_aggregate_kernels_against_float64(B, S, E, T, K, seed, holes, TEMPERATURE):
    from torch_rechub_amd import ops
    c = case(B, S, E, T, K, seed, holes)
    inp = c["inp"]
    xhat32, phi32 = torch.from_numpy(c["xhat"]).float(), torch.from_numpy(c["phi"]).float()  # (the kernel's inputs, rounded once)
    xhat64, phi64, mask = xhat32.double().numpy(), phi32.double().numpy(), inp["mask"].numpy()
    want, c2 = np_sine_aggregate(xhat64, c["d"]["a3"], mask, phi64, TEMPERATURE)
    g_v = c["d"]["g_v"]
    refs = np_sine_aggregate_bwd(xhat64, phi64, c2, g_v, TEMPERATURE)
    grads = []
    for _ in range(2):
        t = [x.to(dev()).requires_grad_(True) for x in (xhat32, inp["a3"], phi32)]
        v = ops.sine_aggregate(t[0], t[1], inp["mask"].to(dev()), t[2], TEMPERATURE)
        v.backward(inp["g_v"].to(dev()))
        grads.append([x.grad.clone() for x in t])
    rows = slice(None)
    _close(v, want, rows, "v")
    assert np.allclose(c2["P3"][0], 1.0 / S) and torch.isfinite(v[0]).all()
    for got, ref, name in zip(grads[0], refs, ("g_xhat", "g_a3", "g_phi")):
        _close(got, ref, rows, name)
    for a, b in zip(*grads):
        assert torch.equal(a, b)


def test_zero_position_row_forward():
    """An all-zero X row (hence zero Y row): the clamped normalisation gives a zero direction, every intention the same
    score, p_u uniform at that position.  Forward only: through the clamp the gradient is ~1e12 g in the reference too."""
    B, S, E, T, K, seed, holes = CASES[1]
    from torch_rechub_amd import ops
    inp = {k: v.clone() for k, v in draw_inputs(B, S, E, T, K, seed, holes).items()}
    inp["X"][3, S - 1] = 0
    inp["Y"][3, S - 1] = 0
    d = {k: v.double().numpy() for k, v in inp.items() if k != "mask"}
    phi, xhat, idx, c1 = np_sine_interests(d["X"], d["Y"], d["a1"], d["a2"], inp["mask"].numpy(), d["C"])
    assert top_k_gap(c1["s_u"], K)[3] >= MIN_GAP and np.allclose(c1["p_u"][3, :, S - 1], 1.0 / K)
    got_phi, got_xhat, got_idx = ops.sine_interests(*(inp[k].to(dev()) for k in ("X", "Y", "a1", "a2", "mask", "C")))
    np.testing.assert_array_equal(got_idx[3].cpu().numpy(), idx[3])
    _close(got_phi, phi, [3], "phi")
    _close(got_xhat, xhat, [3], "xhat")


def test_unsupported_shape_raises_and_does_not_launch():
    from torch_rechub_amd import ops
    B, S, E, T, K = 4, 5, 129, 6, 2
    X = torch.zeros(B, S, E, device=dev())
    mask = torch.ones(B, S, dtype=torch.int32, device=dev())
    assert not ops.sine_supported(S, E, T, K)
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.sine_interests(X, X, torch.zeros(B, S, device=dev()), torch.zeros(B, S, K, device=dev()), mask,
                           torch.zeros(T, E, device=dev()))
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.sine_aggregate(X, torch.zeros(B, S, device=dev()), mask, torch.zeros(B, K, E, device=dev()), 0.1)
    torch.cuda.synchronize()
    ops.check_errors()


# ---- the model against the reference's fixture -----------------------------------------------------------------------
def load_model():
    gold = load_golden("model_sine.npz")
    model = build_sine(gold)
    model.load_state_dict(golden_state(gold, "sd0."))
    return gold, model.to(dev())


def golden_x(gold, bi):
    return {k[len(f"x{bi}."):]: torch.from_numpy(gold[k]).to(dev()) for k in gold.files if k.startswith(f"x{bi}.")}


def test_forward_outputs_match_reference():
    gold, model = load_model()
    x = golden_x(gold, 0)
    assert not gold["x0.hist_item_id"][0].any() and gold["x0.hist_item_id"][1].all()
    model.eval()
    with torch.no_grad():
        for mode, key in ((None, "pred_eval"), ("user", "user_emb"), ("item", "item_emb")):
            model.mode = mode
            want = gold[key]
            np.testing.assert_allclose(model(x).cpu().numpy(), want, rtol=1e-5, atol=1e-5 * float(np.abs(want).max()),
                                       err_msg=key)
    model.mode = None


def test_loss_and_gradients_match_reference_and_reach_row_zero():
    from torch_rechub_amd import ops
    gold, model = load_model()
    x = golden_x(gold, 0)
    y = torch.from_numpy(gold["y0"]).to(dev())
    model.train()
    pred = model(x)
    want = gold["pred_train"]
    np.testing.assert_allclose(pred.detach().cpu().numpy(), want, rtol=1e-5, atol=1e-5 * float(np.abs(want).max()))
    loss = ops.cross_entropy_mean(pred, y)
    assert abs(loss.item() - float(gold["loss"])) < 1e-5 * max(1.0, abs(float(gold["loss"])))
    loss.backward()
    ops.check_errors()
    # no padding row: the padded positions of the histories look row 0 up, and its gradient is not dropped
    assert float(model.item_embedding.weight.grad[0].abs().max()) > 0
    assert float(np.abs(gold["grad.item_embedding.weight"][0]).max()) > 0


def test_three_step_training_matches_reference_trainer():
    from torch_rechub_amd.trainers import MatchTrainer
    gold, model = load_model()
    batches = [(golden_x(gold, i), torch.from_numpy(gold[f"y{i}"]).to(dev())) for i in range(3)]
    trainer = MatchTrainer(model, mode=2, optimizer_params={"lr": float(gold["train.lr"]), "weight_decay": float(gold["train.wd"])},
                           n_epoch=1, device="cuda:0", show_progress=False)
    mean_loss = trainer.train_one_epoch(batches)
    assert abs(mean_loss - float(gold["train.mean_loss"])) < 1e-5 * max(1.0, abs(float(gold["train.mean_loss"])))
    assert_state_follows_reference_trajectory(gold, model.state_dict(), "sine")


def test_graph_step_equals_eager_training_bitwise():
    """The example's optimizer settings (weight_decay 1e-6) on the captured hipGraph step and on the eager one."""
    from torch_rechub_amd.models.matching import SINE
    from torch_rechub_amd.trainers import MatchTrainer
    from torch_rechub_amd.utils.data import DeviceDataLoader
    V, S, E, H, T, K, NEG, Bt = 3000, 12, 24, 32, 10, 2, 3, 256
    g = torch.Generator().manual_seed(5)
    hist = torch.randint(1, V, (Bt * 10, S), generator=g)
    lens = torch.randint(1, S + 1, (hist.shape[0],), generator=g)
    hist[torch.arange(S)[None, :] < (S - lens)[:, None]] = 0
    cols = torch.cat([hist, torch.randint(1, V, (hist.shape[0], 1 + NEG), generator=g)], 1).contiguous()
    label = torch.zeros(hist.shape[0])

    def build():
        torch.manual_seed(8)
        m = SINE(["hist_item_id"], ["item_id"], ["neg_items"], V, E, H, T, K, S, temperature=0.1)
        with torch.no_grad():
            for table in (m.item_embedding, m.concept_embedding, m.position_embedding):
                table.weight.normal_(0, 0.1)
        return m.to(dev())

    ma, mb = build(), build()
    losses, ts = [], []
    for m, ug in ((ma, True), (mb, False)):
        t = MatchTrainer(m, mode=2, use_graph=ug, device="cuda:0", show_progress=False,
                         optimizer_params={"lr": 1e-3, "weight_decay": 1e-6})
        loader = DeviceDataLoader(cols.to(dev()), [("hist_item_id", S), "item_id", ("neg_items", NEG)], None, [],
                                  label.to(dev()), Bt, shuffle=False)
        losses.append(t.train_one_epoch(loader))
        ts.append(t)
    assert ts[0]._graph is not None
    assert np.isfinite(losses[0]) and losses[0] == losses[1]
    sa, sb = ma.state_dict(), mb.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    assert not torch.equal(sa["concept_embedding.weight"], build().state_dict()["concept_embedding.weight"])  # it trained
