"""CIN / xDeepFM on the MI355X: the compressed-interaction kernels of csrc/cin.hip against the float64 oracle
(tests/cin_oracle.py) over their shape range, the layer and the models against the reference's fixtures
(tools/gen_golden_cin.py), the fused-gather path against the layer path, and the captured step bit for bit against its eager
twin.

Bounds.  Kernel against float64 with the project's kernel convention (test_gpu_sasrec.py): rtol 1e-4, atol 1e-5 of the
tensor's largest magnitude, 1e-4 of it for g_W; where fp32 itself cannot meet that at the larger K, the rule of
test_gpu_session_hllm_shapes.py::compare: the larger of that bound and 4 x the error of an fp32 torch evaluation of the same
case on the CPU against the same float64 numbers.  It never looks at the kernel's output.  Each comparison prints the table
line of ``compare`` (pytest -s).

The ReLU edge.  A float32 kernel may decide a pre-activation that is zero to rounding the other way than float64 does, so
every test zeroes the upstream gradient at the (b, o, d) whose float64 pre-activation lies within 1e-6 of the tensor's
largest magnitude of zero, and asserts that those are at most 0.1 % of the elements."""
import numpy as np
import pytest
import torch

import cin_oracle as O
from conftest import assert_state_follows_reference_trajectory, golden_batch, golden_state, load_golden
from test_cin_host import CIN_CASES, XDEEPFM_MODELS, build_xdeepfm_model, cin_case
from test_gpu_session_hllm_shapes import compare, poison_small_blocks
from torch_rechub_amd._lib import H

pytestmark = pytest.mark.gpu

EDGE = 1e-6


def dev():
    return torch.device("cuda:0")


def to_dev(x):
    return {k: v.to(dev()) for k, v in x.items()}


def torch_layer(x0, h, w, b):
    """The reference's formulation of one layer on torch ops (layers.py:359-362)."""
    z = x0.unsqueeze(2) * h.unsqueeze(1)
    return torch.relu(torch.nn.functional.conv1d(z.reshape(z.shape[0], z.shape[1] * z.shape[2], z.shape[3]), w, b))


def make_case(B, D, F, Hp, Ho, seed, dead=None, zero_x0=False):
    """float32 CPU inputs of one layer, the upstream gradient with the ReLU edge zeroed, the float64 results and the fp32
    CPU results.  ``dead``: a channel whose bias is -1e6 (the edge is judged on the other channels)."""
    g = torch.Generator().manual_seed(seed)
    K = F * Hp
    x0 = torch.zeros(B, F, D) if zero_x0 else torch.randn(B, F, D, generator=g)
    h = torch.randn(B, Hp, D, generator=g)
    w = torch.randn(Ho, K, 1, generator=g) / K ** 0.5
    b = 0.5 * torch.randn(Ho, generator=g)
    if dead is not None:
        b[dead] = -1e6
    gy = torch.randn(B, Ho, D, generator=g)
    a64 = [t.numpy().astype(np.float64) for t in (x0, h, w, b)]
    pre = O.layer_pre(*a64)
    live = np.ones(Ho, bool)
    if dead is not None:
        live[dead] = False
    if pre.size:
        edge = np.abs(pre) <= EDGE * np.abs(pre[:, live]).max()
        edge[:, ~live] = False
        assert edge.mean() <= 1e-3, f"{edge.mean():.2e} of the pre-activations sit on the ReLU edge"
        gy[torch.from_numpy(edge)] = 0.0
    want = dict(zip(("g_x0", "g_h", "g_w", "g_b"), O.layer_bwd(*a64, gy.numpy().astype(np.float64), pre)))
    want["y"] = np.maximum(pre, 0.0)
    leaves = [t.clone().requires_grad_(True) for t in (x0, h, w, b)]
    y32 = torch_layer(*leaves)
    y32.backward(gy)
    cpu32 = {"y": y32.detach(), "g_x0": leaves[0].grad, "g_h": leaves[1].grad, "g_w": leaves[2].grad, "g_b": leaves[3].grad}
    return (x0, h, w, b, gy), want, cpu32


def strided_x0(x0, pad_d=6, tail=7):
    """x0 as the sparse block of a wider row: field stride D + pad_d, sample stride F (D + pad_d) + tail, the gaps NaN."""
    B, F, D = x0.shape
    buf = torch.full((B, F * (D + pad_d) + tail), float("nan"), device=dev())
    view = buf[:, :F * (D + pad_d)].unflatten(1, (F, D + pad_d))[:, :, :D]
    view.copy_(x0)
    return view


def second_half(h):
    """h as the second half of a tensor twice as wide (what split_half hands to the next layer), the first half NaN."""
    B, Hp, D = h.shape
    buf = torch.full((B, 2 * Hp, D), float("nan"), device=dev())
    buf[:, Hp:].copy_(h)
    return buf[:, Hp:]


def run_kernel(inputs, views=False):
    from torch_rechub_amd import ops
    x0, h, w, b, gy = inputs
    xd = strided_x0(x0.to(dev())) if views else x0.to(dev())
    hd = second_half(h.to(dev())) if views else h.to(dev())
    leaves = [xd.requires_grad_(True), hd.requires_grad_(True), w.to(dev()).requires_grad_(True), b.to(dev()).requires_grad_(True)]
    gyd = gy.to(dev())
    poison_small_blocks()
    y = ops.cin_layer(*leaves)
    assert y.shape == gy.shape and y.is_contiguous()
    y.backward(gyd)
    torch.cuda.synchronize()
    ops.check_errors()
    return {"y": y.detach(), "g_x0": leaves[0].grad, "g_h": leaves[1].grad, "g_w": leaves[2].grad, "g_b": leaves[3].grad}


def check(case, got, want, cpu32):
    fails = []
    for name in ("y", "g_x0", "g_h", "g_w", "g_b"):
        compare(case, name, got[name], want[name], cpu32[name], 1e-4 if name == "g_w" else 1e-5, fails, rtol=1e-4)
    assert not fails, f"{case}: (tensor, error beyond rtol, bound) {fails}"


# name: (B, D, F, Hp, Ho).  M = B D in {1, 63, 64, 65, 130}; F in {1, 2, 5, 39}; Hp in {1, 3, 64, 65}; K = F Hp odd (15, 39,
# 65, 2535) and one past a K chunk (65); Ho in {1, 2, 63, 64, 65, 130}: one short of, exactly and one past a tile, two tiles
# and a ragged third.
OP_CASES = {
    "M1": (1, 1, 1, 1, 1),
    "M63_K6": (9, 7, 2, 3, 2),
    "M64_K15": (4, 16, 5, 3, 63),
    "M65_K39": (65, 1, 39, 1, 64),
    "M130_K65": (13, 10, 5, 13, 65),
    "Hp64_Ho130": (4, 16, 2, 64, 130),
    "Hp65_K2535": (9, 7, 39, 65, 65),
    "F1_Hp65_Ho1": (13, 10, 1, 65, 1),
}


@pytest.mark.parametrize("case", list(OP_CASES))
def test_layer_op_against_float64(case):
    B, D, F, Hp, Ho = OP_CASES[case]
    inputs, want, cpu32 = make_case(B, D, F, Hp, Ho, seed=sum(map(ord, case)))
    check(case, run_kernel(inputs), want, cpu32)


def test_strided_x0_and_second_half_h_are_read_in_place():
    inputs, want, cpu32 = make_case(13, 10, 5, 3, 6, seed=1)
    got = run_kernel(inputs, views=True)
    check("strided", got, want, cpu32)
    plain = run_kernel(inputs)
    for k in got:  # the same arithmetic in the same order, wherever the operands lie
        assert torch.equal(got[k], plain[k]), k


def test_empty_batch():
    inputs, want, cpu32 = make_case(0, 16, 5, 3, 6, seed=2)
    got = run_kernel(inputs)
    assert got["y"].shape == (0, 6, 16) and got["g_x0"].shape == (0, 5, 16) and got["g_h"].shape == (0, 3, 16)
    assert not got["g_w"].any() and not got["g_b"].any() and got["g_w"].shape == (6, 15, 1)


def test_second_trip_of_the_row_grid():
    """Forward and input-gradient launches are capped at 1024 row tiles: M = 600 x 128 = 76800 rows are 1200 tiles, so 176
    workgroups take a second tile; the same rows are 16 wgrad chunks of 75 tiles."""
    inputs, want, cpu32 = make_case(600, 128, 2, 3, 2, seed=3)
    check("second_trip", run_kernel(inputs), want, cpu32)


def test_wgrad_chunks_with_a_ragged_last_one():
    """M = 2500 rows, one 64 x 64 output tile: 16 chunks asked for, 3 tiles (192 rows) each, so 14 chunks and the last holds
    4 rows."""
    from torch_rechub_amd import _lib
    assert _lib.query("rh_cin_wgrad_chunks", 2500, 1, 8, 8, 64) == 14
    inputs, want, cpu32 = make_case(2500, 1, 8, 8, 64, seed=4)
    check("ragged_chunks", run_kernel(inputs), want, cpu32)


def test_dead_channel_is_exactly_zero_everywhere():
    """A channel whose bias is -1e6: output exactly 0, an exactly-zero g_W row and g_bias entry, and input gradients that
    are bit for bit those of the layer without the channel."""
    B, D, F, Hp, Ho = 13, 10, 5, 3, 6
    inputs, want, cpu32 = make_case(B, D, F, Hp, Ho, seed=5, dead=Ho - 1)
    got = run_kernel(inputs)
    check("dead_channel", got, want, cpu32)
    assert not got["y"][:, Ho - 1].any() and not got["g_w"][Ho - 1].any() and got["g_b"][Ho - 1] == 0
    x0, h, w, b, gy = inputs
    without = run_kernel((x0, h, w[:Ho - 1].contiguous(), b[:Ho - 1].contiguous(), gy[:, :Ho - 1].contiguous()))
    assert torch.equal(got["g_x0"], without["g_x0"]) and torch.equal(got["g_h"], without["g_h"])
    assert torch.equal(got["g_w"][:Ho - 1], without["g_w"]) and torch.equal(got["y"][:, :Ho - 1], without["y"])


def test_all_zero_x0():
    inputs, want, cpu32 = make_case(13, 10, 5, 3, 6, seed=6, zero_x0=True)
    got = run_kernel(inputs)
    check("zero_x0", got, want, cpu32)
    assert torch.equal(got["y"], torch.relu(inputs[3].to(dev())).view(1, -1, 1).expand_as(got["y"]))
    assert not got["g_h"].any() and not got["g_w"].any()


def test_gradients_bit_identical_over_two_runs():
    inputs, _, _ = make_case(130, 16, 5, 13, 70, seed=7)  # 33 row tiles, two K chunks, two Ho tiles, 11 wgrad chunks
    a, b = run_kernel(inputs), run_kernel(inputs)
    for k in ("y", "g_w", "g_b", "g_x0", "g_h"):
        assert torch.equal(a[k], b[k]), k


def test_one_past_each_limit_is_refused():
    from torch_rechub_amd import ops
    from torch_rechub_amd.basic.layers import CIN

    def call(B, D, F, Hp, Ho):
        z = lambda *s: torch.zeros(*s, device=dev())  # noqa: E731
        assert not ops.cin_layer_ok(z(B, F, D), z(B, Hp, D), z(Ho, F * Hp, 1), z(Ho))
        return ops.cin_layer(z(B, F, D), z(B, Hp, D), z(Ho, F * Hp, 1), z(Ho))

    with pytest.raises(RuntimeError, match=f"embed_dim {H.RH_CIN_MAX_D + 1} unsupported"):
        call(2, H.RH_CIN_MAX_D + 1, 2, 2, 2)
    with pytest.raises(RuntimeError, match=f"num_fields {H.RH_CIN_MAX_F + 1} unsupported"):
        call(2, 4, H.RH_CIN_MAX_F + 1, 2, 2)
    with pytest.raises(RuntimeError, match=f"input channels {H.RH_CIN_MAX_HP + 1} unsupported"):
        call(2, 4, 2, H.RH_CIN_MAX_HP + 1, 2)
    with pytest.raises(RuntimeError, match=f"output channels {H.RH_CIN_MAX_HO + 1} unsupported"):
        call(2, 4, 2, 2, H.RH_CIN_MAX_HO + 1)
    torch.cuda.synchronize()
    # the largest shape on every axis but the batch runs, and the layer falls back to torch ops one past a limit
    inputs, want, cpu32 = make_case(1, H.RH_CIN_MAX_D, H.RH_CIN_MAX_F, H.RH_CIN_MAX_HP, H.RH_CIN_MAX_HO, seed=8)
    check("limits", run_kernel(inputs), want, cpu32)
    torch.manual_seed(0)
    cin = CIN(H.RH_CIN_MAX_F + 1, [4], split_half=False).to(dev())
    x = torch.randn(3, H.RH_CIN_MAX_F + 1, 4, device=dev())
    want = cin.fc(torch_layer(x, x, cin.conv_layers[0].weight, cin.conv_layers[0].bias).sum(2))
    torch.testing.assert_close(cin(x), want, rtol=1e-5, atol=1e-6)


def test_peak_memory_stays_below_one_product_tensor():
    """B = 512, F = 8, Hp = 32, Ho = 32, D = 16: the (B, F Hp, D) product the reference materialises (and keeps for backward)
    is 512 x 256 x 16 x 4 B = 8 MiB.  The op legitimately allocates y (1 MiB), g_x0 (0.25 MiB), g_h (1 MiB), the wgrad
    workspace (16 chunks x (32 x 256 + 32) floats = 0.5 MiB) and [g_W | g_bias] (32 KiB): under 3 MiB above the inputs.
    The torch formulation of the same layer exceeds the bound -- the check of this test itself."""
    from torch_rechub_amd import ops
    B, F, Hp, Ho, D = 512, 8, 32, 32, 16
    product_bytes = B * F * Hp * D * 4
    g = torch.Generator().manual_seed(9)
    mk = lambda *s: torch.randn(*s, generator=g).to(dev())  # noqa: E731
    tensors = [mk(B, F, D), mk(B, Hp, D), mk(Ho, F * Hp, 1) / (F * Hp) ** 0.5, mk(Ho)]
    gy = mk(B, Ho, D)
    peaks, grads = {}, {}
    for name, fn in (("kernel", ops.cin_layer), ("torch", torch_layer)):
        leaves = [t.clone().requires_grad_(True) for t in tensors]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        y = fn(*leaves)
        y.backward(gy)
        torch.cuda.synchronize()
        peaks[name] = torch.cuda.max_memory_allocated() - base
        grads[name] = [y.detach()] + [t.grad for t in leaves]
        del y, leaves
    print(f"peak above the inputs: kernel {peaks['kernel'] / 2**20:.2f} MiB, torch {peaks['torch'] / 2**20:.2f} MiB, "
          f"one product tensor {product_bytes / 2**20:.2f} MiB")
    assert peaks["kernel"] < product_bytes
    assert peaks["torch"] > product_bytes
    for a, b in zip(grads["kernel"], grads["torch"]):
        torch.testing.assert_close(a, b, rtol=1e-4, atol=1e-4 * float(b.abs().max()))


# ---- the layer against the reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", CIN_CASES)
def test_cin_layer_against_fixture(tag):
    from torch_rechub_amd.basic.layers import CIN
    gold = load_golden("cin_layers.npz")
    x, sd, cin_size, split_half = cin_case(gold, tag)
    cin = CIN(x.shape[1], cin_size, split_half)
    cin.load_state_dict({k: torch.from_numpy(v).float() for k, v in sd.items()})
    cin = cin.to(dev())
    xt = torch.from_numpy(x).float().to(dev()).requires_grad_(True)
    y = cin(xt)
    y.backward(torch.from_numpy(gold[tag + ".g_out"]).float().to(dev()))

    def close(got, want, frac, what):
        np.testing.assert_allclose(got.detach().cpu().numpy(), want, rtol=1e-4, atol=frac * float(np.abs(want).max()),
                                   err_msg=f"{tag}: {what}")

    close(y, gold[tag + ".out"], 1e-5, "out")
    close(xt.grad, gold[tag + ".g_x"], 1e-5, "g_x")
    for n, p in cin.named_parameters():
        close(p.grad, gold[f"{tag}.grad.{n}"], 1e-4 if n.endswith("weight") else 1e-5, n)


# ---- the models against the reference ---------------------------------------------------------------------------------
def reference_forward(self, x):
    """DeepFM's reference forward (deepfm.py:33-43) with FM replaced by CIN, restated on the HIP layers: two lookups, LR
    on the flattened fm embeddings, CIN, MLP, sigmoid."""
    input_deep = self.embedding(x, self.deep_features, squeeze_dim=True)
    input_fm = self.embedding(x, self.fm_features, squeeze_dim=False)
    y = self.linear(input_fm.flatten(start_dim=1)) + self.cin(input_fm) + self.mlp(input_deep)
    return torch.sigmoid(y.squeeze(1))


def load_model(cfg, kind="fused"):
    gold = load_golden(f"model_{cfg}.npz")
    model = build_xdeepfm_model(cfg, gold)
    if kind == "layer":
        model.forward = reference_forward.__get__(model)
    model.load_state_dict(golden_state(gold, "sd0."))
    return gold, model.to(dev())


@pytest.mark.parametrize("cfg", list(XDEEPFM_MODELS))
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
@pytest.mark.parametrize("cfg", list(XDEEPFM_MODELS))
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


@pytest.mark.parametrize("cfg", list(XDEEPFM_MODELS))
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


# ---- the captured step, bit for bit -----------------------------------------------------------------------------------
def _twin_model(seed=11):
    from test_gpu_ffm import VOCABS
    from torch_rechub_amd.basic.features import SparseFeature
    from torch_rechub_amd.models.ranking import xDeepFM
    torch.manual_seed(seed)
    sparse = [SparseFeature(f"C{i}", v, 10) for i, v in enumerate(VOCABS)]  # width 10: padded tables, a strided CIN input
    m = xDeepFM(sparse, sparse, {"dims": [64, 32], "dropout": 0.0, "activation": "relu"}, [8, 6])
    return m, [f.name for f in sparse]


def test_graph_step_equals_eager_training_bitwise():
    """What the deterministic backward is for: ten captured steps end in the state of ten eager steps, bit for bit."""
    from test_gpu_ffm import VOCABS, _assert_bit_equal, _collision_free
    from torch_rechub_amd.trainers import CTRTrainer
    from torch_rechub_amd.utils.data import DeviceDataLoader
    nb, B = 10, 256
    sparse, label = _collision_free(VOCABS, nb, B, seed=21)
    ma, names = _twin_model()
    mb, _ = _twin_model()
    mb.load_state_dict(ma.state_dict())
    base = dict(optimizer_params={"lr": 1e-2, "weight_decay": 1e-4, "lazy_small_rows": 8}, device="cuda:0",
                show_progress=False, table_update="dense")
    ta = CTRTrainer(ma, use_graph=True, **base)
    tb = CTRTrainer(mb, use_graph=False, **base)
    losses = [t.train_one_epoch(DeviceDataLoader(sparse.to(dev()), names, None, [], label.to(dev()), B, shuffle=False))
              for t in (ta, tb)]
    assert ta._graph is not None
    assert losses[0] == losses[1]
    _assert_bit_equal(ma, mb)
