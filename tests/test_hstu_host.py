"""HSTU host side: a float64 restatement of the attention (forward and backward) and of the next-token head, checked
against autograd; the time-bucket arithmetic (numpy float32 restatement, the one csrc/hstu.hip repeats) against torch
CPU over adversarial deltas; constructor, state_dict and error-case parity of the layers, the model and the trainer."""
import numpy as np
import pytest
import torch

from torch_rechub_amd.utils.hstu_utils import RelativeBucketedTimeAndPositionBias, RelPosBias, VocabMask, bucketize_time

BUCKET_CFGS = [(128, "sqrt", 1.0, "minutes"), (128, "log", 0.301, "seconds"), (64, "sqrt", 3.7, "seconds"),
               (128, "log", 1.0, "minutes")]


def np_bucket(dt, nb, fn, div, unit):
    """The kernel's bucket arithmetic in numpy float32: (float)dt -> abs -> [/ 60] -> max 1e-6 -> sqrt | log (correctly
    rounded through float64) -> / divisor -> clamp [0, nb] -> truncate."""
    x = np.abs(np.asarray(dt, dtype=np.int64).astype(np.float32))
    if unit == "minutes":
        x = (x / np.float32(60.0)).astype(np.float32)
    x = np.maximum(x, np.float32(1e-6))
    v = np.sqrt(x) if fn == "sqrt" else np.log(x.astype(np.float64)).astype(np.float32)
    v = (v / np.float32(div)).astype(np.float32)
    return np.clip(v, np.float32(0), np.float32(nb)).astype(np.int64)


def adversarial_deltas(div, fn, unit):
    """Every integer in [0, 1e6], the neighbourhoods of the bucket edges, negative and large int64 deltas."""
    parts = [np.arange(0, 1_000_001, dtype=np.int64)]
    k = np.arange(0, 400, dtype=np.float64)
    scale = 60.0 if unit == "minutes" else 1.0
    edges = scale * (k * div)**2 if fn == "sqrt" else scale * np.exp(np.minimum(k * div, 40.0))
    edges = edges[edges < 4e18]
    near = (np.round(edges)[:, None] + np.arange(-3, 4)[None, :]).astype(np.int64).ravel()
    parts += [near, -near, np.array([2**62, -2**62, 2**63 - 1, -2**63 + 1, 10**12, -10**12, 10**15 + 7], dtype=np.int64)]
    return np.concatenate(parts)


@pytest.mark.parametrize("cfg", BUCKET_CFGS)
def test_bucket_restatement_matches_torch_cpu(cfg):
    nb, fn, div, unit = cfg
    dt = adversarial_deltas(div, fn, unit)
    want = bucketize_time(torch.from_numpy(dt), nb, fn, div, unit).numpy()
    np.testing.assert_array_equal(np_bucket(dt, nb, fn, div, unit), want)


def np_attention(proj, pos_w, ts_w, td, mask, H, dqk, dv, N, nb=128, fn="sqrt", div=1.0, unit="minutes"):
    """float64 forward of the attention; returns (out (B, L, H dv), cache for np_attention_bwd)."""
    proj = np.asarray(proj, np.float64)
    B, L, _ = proj.shape
    q = proj[..., :H * dqk].reshape(B, L, H, dqk).transpose(0, 2, 1, 3)
    k = proj[..., H * dqk:2 * H * dqk].reshape(B, L, H, dqk).transpose(0, 2, 1, 3)
    v = proj[..., 2 * H * dqk + H * dv:].reshape(B, L, H, dv).transpose(0, 2, 1, 3)
    i = np.arange(L)
    rel = i[None, :] - i[:, None] + N - 1
    bias = np.asarray(pos_w, np.float64)[rel].transpose(2, 0, 1)[None]  # (1, H, L, L)
    bk = None
    if td is not None:
        td = np.asarray(td, np.int64)
        bk = np_bucket(td[:, :, None] - td[:, None, :], nb, fn, div, unit)  # (B, L, L)
        bias = bias + np.asarray(ts_w, np.float64)[bk].transpose(0, 3, 1, 2)
    valid = np.tril(np.ones((L, L), bool))[None, None]
    if mask is not None:
        valid = valid & np.asarray(mask, bool)[:, None, None, :]
    alpha = 1.0 / np.sqrt(dqk)
    s = np.einsum("bhik,bhjk->bhij", q, k) * alpha + bias
    sig = 1.0 / (1.0 + np.exp(-s))
    a = np.where(valid, s * sig / N, 0.0)
    out = np.einsum("bhij,bhjd->bhid", a, v).transpose(0, 2, 1, 3).reshape(B, L, H * dv)
    return out, dict(q=q, k=k, v=v, s=s, sig=sig, a=a, valid=valid, bk=bk, rel=rel, alpha=alpha)


def np_attention_bwd(c, g, H, dqk, dv, N, npos, nts):
    """float64 gradients (g_proj over the q / k / v columns, g_pos_w, g_ts_w) of np_attention for upstream g."""
    B, L, _ = g.shape
    go = np.asarray(g, np.float64).reshape(B, L, H, dv).transpose(0, 2, 1, 3)
    da = np.einsum("bhid,bhjd->bhij", go, c["v"])
    dv_ = np.einsum("bhij,bhid->bhjd", c["a"], go)
    sig, s = c["sig"], c["s"]
    ds = np.where(c["valid"], da * sig * (1 + s * (1 - sig)) / N, 0.0)
    dq = np.einsum("bhij,bhjk->bhik", ds, c["k"]) * c["alpha"]
    dk = np.einsum("bhij,bhik->bhjk", ds, c["q"]) * c["alpha"]
    gp = np.zeros((B, L, 2 * H * (dqk + dv)))
    gp[..., :H * dqk] = dq.transpose(0, 2, 1, 3).reshape(B, L, -1)
    gp[..., H * dqk:2 * H * dqk] = dk.transpose(0, 2, 1, 3).reshape(B, L, -1)
    gp[..., 2 * H * dqk + H * dv:] = dv_.transpose(0, 2, 1, 3).reshape(B, L, -1)
    gpos = np.zeros((npos, H))
    np.add.at(gpos, c["rel"].ravel(), ds.sum(0).reshape(H, -1).T)
    gts = np.zeros((nts, H))
    if c["bk"] is not None:
        np.add.at(gts, c["bk"].ravel(), ds.transpose(0, 2, 3, 1).reshape(-1, H))
    return gp, gpos, gts


def np_head(h, w, b, labels, t1, t2=None):
    """float64 next-token loss and gradients (loss, dh, dW, db) of the reference's logits.clone / [..., 0] = -1e9 /
    CrossEntropyLoss (t2 None) or NCELoss (t2) chain."""
    h, w = np.asarray(h, np.float64), np.asarray(w, np.float64)
    z = h @ w.T + (0.0 if b is None else np.asarray(b, np.float64))
    z = z / t1
    z[:, 0] = -1e9
    tt = 1.0 if t2 is None else t2
    z = z / tt
    m = z.max(1, keepdims=True)
    lse = (m + np.log(np.exp(z - m).sum(1, keepdims=True)))[:, 0]
    p = np.exp(z - lse[:, None])
    labels = np.asarray(labels)
    keep = labels != 0
    M = len(labels)
    if keep.any():
        wr = keep / keep.sum()
    elif t2 is not None:
        wr = np.full(M, 1.0 / M)
    else:
        return np.nan, np.zeros_like(h), np.zeros_like(w), np.zeros(w.shape[0])
    loss = float((wr * (lse - z[np.arange(M), labels])).sum())
    dz = p.copy()
    dz[np.arange(M), labels] -= 1.0
    dz *= wr[:, None]
    dz[:, 0] = 0.0
    dz = dz / tt / t1
    return loss, dz @ w, dz.T @ h, dz.sum(0)


def test_np_attention_matches_autograd():
    """The float64 restatement (forward and all gradients) against torch autograd of the dense reference formula."""
    g = torch.Generator().manual_seed(0)
    B, L, H, dqk, dv, N, nb = 3, 9, 2, 5, 3, 12, 16
    proj = torch.randn(B, L, 2 * H * (dqk + dv), generator=g, dtype=torch.float64)
    rab = RelativeBucketedTimeAndPositionBias(H, N, nb, "log", 0.301, "seconds").double()
    td = torch.randint(0, 100000, (B, L), generator=g)
    mask = torch.ones(B, L, dtype=torch.bool)
    mask[0, :3] = False
    mask[1, 5:] = False
    mask[2] = False
    out, c = np_attention(proj.numpy(), rab.pos_w.detach().numpy(), rab.ts_w.detach().numpy(), td.numpy(), mask.numpy(),
                          H, dqk, dv, N, nb, "log", 0.301, "seconds")
    gout = torch.randn(B, L, H * dv, generator=g, dtype=torch.float64)
    gp, gpos, gts = np_attention_bwd(c, gout.numpy(), H, dqk, dv, N, 2 * N - 1, nb + 1)
    x = proj.clone().requires_grad_(True)
    q = x[..., :H * dqk].reshape(B, L, H, dqk).transpose(1, 2)
    k = x[..., H * dqk:2 * H * dqk].reshape(B, L, H, dqk).transpose(1, 2)
    v = x[..., 2 * H * dqk + H * dv:].reshape(B, L, H, dv).transpose(1, 2)
    s = q @ k.transpose(-2, -1) / np.sqrt(dqk) + rab(time_diffs=td)
    valid = torch.tril(torch.ones(L, L, dtype=torch.bool))[None, None] & mask[:, None, None, :]
    a = torch.nn.functional.silu(s.masked_fill(~valid, -1e4)) / N
    ref = (a @ v).transpose(1, 2).reshape(B, L, H * dv)
    np.testing.assert_allclose(out, ref.detach().numpy(), rtol=1e-12, atol=1e-12)
    ref.backward(gout)
    np.testing.assert_allclose(gp, x.grad.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(gpos, rab.pos_w.grad.numpy(), rtol=1e-10, atol=1e-12)
    np.testing.assert_allclose(gts, rab.ts_w.grad.numpy(), rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("t2", [None, 0.1])
@pytest.mark.parametrize("all_ignored", [False, True])
def test_np_head_matches_autograd(t2, all_ignored):
    from torch_rechub_amd.basic.loss_func import NCELoss
    g = torch.Generator().manual_seed(1)
    M, D, V, t1 = 13, 6, 29, 0.05
    h = torch.randn(M, D, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.randn(V, D, generator=g, dtype=torch.float64, requires_grad=True)
    b = torch.randn(V, generator=g, dtype=torch.float64, requires_grad=True)
    labels = torch.randint(0, V, (M,), generator=g)
    labels[:3] = 0
    if all_ignored:
        labels[:] = 0
    loss, dh, dw, db = np_head(h.detach().numpy(), w.detach().numpy(), b.detach().numpy(), labels.numpy(), t1, t2)
    logits = (h @ w.T + b) / t1
    logits = logits.clone()
    logits[..., 0] = -1e9
    fn = torch.nn.CrossEntropyLoss(ignore_index=0) if t2 is None else NCELoss(temperature=t2, ignore_index=0)
    ref = fn(logits, labels)
    if all_ignored and t2 is None:  # NaN loss; autograd's gradients are zero, as np_head's
        assert np.isnan(loss) and torch.isnan(ref)
        ref.backward()
        assert not h.grad.any() and not w.grad.any() and not dh.any() and not dw.any()
        return
    assert abs(loss - ref.item()) <= 1e-9 * max(1.0, abs(loss))
    ref.backward()
    np.testing.assert_allclose(dh, h.grad.numpy(), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(dw, w.grad.numpy(), rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(db, b.grad.numpy(), rtol=1e-9, atol=1e-12)


def test_constructors_state_dict_and_errors():
    from torch_rechub_amd.basic.layers import HSTUBlock, HSTULayer
    from torch_rechub_amd.models.generative import HSTUModel
    with pytest.raises(ValueError, match="must be divisible"):
        HSTULayer(d_model=30, n_heads=4, dqk=8, dv=8, max_seq_len=16)
    with pytest.raises(ValueError, match="score_norm must be"):
        HSTUModel(50, score_norm="cos")
    with pytest.raises(ValueError, match="temperature must be positive"):
        HSTUModel(50, temperature=0)
    with pytest.raises(ValueError, match="Unsupported time_bucket_fn"):
        RelativeBucketedTimeAndPositionBias(2, 8, time_bucket_fn="exp")
    with pytest.raises(ValueError, match="exceeds max_seq_len"):
        HSTUModel(50, d_model=24, n_heads=2, n_layers=1, dqk=12, dv=10, max_seq_len=8)(torch.ones(2, 9, dtype=torch.long))
    m = HSTUModel(50, d_model=24, n_heads=2, n_layers=2, dqk=12, dv=10, max_seq_len=16, num_time_buckets=8)
    assert torch.all(m.token_embedding.weight[0] == 0)
    sd = m.state_dict()
    assert sd["hstu_block.layers.1.proj1.weight"].shape == (2 * 2 * 12 + 2 * 2 * 10, 24)
    assert sd["hstu_block.layers.0.rab.pos_w"].shape == (31, 2)
    assert sd["hstu_block.layers.0.rab.ts_w"].shape == (9, 2)
    assert sd["output_bias"].shape == (50,)
    untied = HSTUModel(50, d_model=24, n_heads=2, n_layers=1, dqk=12, dv=10, max_seq_len=16, tie_embeddings=False,
                       use_output_bias=False)
    assert untied.output_projection.bias is None and untied.output_bias is None
    blk = HSTUBlock(d_model=24, n_heads=2, n_layers=3, dqk=12, dv=10, max_seq_len=16)
    assert len(blk.layers) == 3
    assert RelPosBias(4, 16, 8)(32).shape == (1, 4, 32, 32)
    masked = VocabMask(10, [0]).apply_mask(torch.zeros(2, 10), invalid_ids=torch.tensor([[1, 3], [2, 5]]))
    assert masked[0, 1] <= -1e8 and masked[1, 5] <= -1e8 and masked[0, 2] == 0


def test_seq_trainer_contract_on_host():
    from torch_rechub_amd.trainers import SeqTrainer
    with pytest.raises(RuntimeError, match="HIP device"):
        SeqTrainer(torch.nn.Linear(1, 1), device="cpu")
    with pytest.raises(NotImplementedError):
        SeqTrainer(torch.nn.Linear(1, 1), device="cuda:0", gpus=[0, 1])


def test_seq_dataset_yields_reference_tuple():
    from torch_rechub_amd.utils.data import SeqDataset
    ds = SeqDataset(np.ones((3, 4), np.int64), np.tile(np.arange(4), (3, 1)), np.array([5, 6, 7]), np.zeros((3, 4), np.int64))
    assert len(ds) == 3
    tok, pos, td, tgt = ds[1]
    assert tok.dtype == torch.long and pos.tolist() == [0, 1, 2, 3] and td.shape == (4,) and int(tgt) == 6


def test_rab_dense_bias_and_state_dict_against_reference_fixtures():
    """The mirror's dense rab forward equals the reference's on the fixture's parameters; each model fixture's state_dict
    keys and shapes are the mirror's."""
    import json

    from conftest import load_golden
    from torch_rechub_amd.models.generative import HSTUModel
    gold = load_golden("hstu_layers.npz")
    rab = RelativeBucketedTimeAndPositionBias(2, 12, 16, "log", 0.301, "seconds")
    rab.load_state_dict({"pos_w": torch.from_numpy(gold["rab.pos_w"]), "ts_w": torch.from_numpy(gold["rab.ts_w"])})
    with torch.no_grad():
        assert torch.equal(rab(time_diffs=torch.from_numpy(gold["time_diffs"])), torch.from_numpy(gold["rab.bias_time"]))
        assert torch.equal(rab(seq_len=10), torch.from_numpy(gold["rab.bias_pos"]))
    for cfg in ("tied_l2_ce", "untied_none_nce", "tied_none_t2_nobias_ce", "untied_l2_bias_nce"):
        mg = load_golden(f"model_hstu_{cfg}.npz")
        kw = json.loads(str(mg["cfg"]))
        kw.pop("loss_type")
        sd = HSTUModel(40, d_model=24, n_heads=2, n_layers=2, dqk=12, dv=10, max_seq_len=12, dropout=0.0,
                       num_time_buckets=16, **kw).state_dict()
        assert list(sd) == [str(s) for s in mg["sd_keys"]]
        for k, v in sd.items():
            assert tuple(v.shape) == mg["sd0." + k].shape, (cfg, k)


def test_seq_trainer_rejects_unsupported_loss_params_at_construction():
    from torch_rechub_amd.models.generative import HSTUModel
    from torch_rechub_amd.trainers import SeqTrainer
    m = HSTUModel(20, d_model=8, n_heads=2, n_layers=1, dqk=4, dv=4, max_seq_len=8)
    for lp in ({"ignore_index": 0, "reduction": "sum"}, {"ignore_index": 0, "label_smoothing": 0.1}, {"ignore_index": -100}):
        with pytest.raises(NotImplementedError, match="fused next-token loss"):
            SeqTrainer(m, device="cuda:0", loss_params=lp)
    with pytest.raises(ValueError, match="loss_type"):
        SeqTrainer(m, device="cuda:0", loss_type="bpr")


def test_hstu_entry_points_reject_unsupported_shapes():
    """Argument validation of csrc/hstu.hip and csrc/stream_ce.hip at the first shape past each limit: nothing is
    launched (the pointers are never dereferenced)."""
    import ctypes

    from torch_rechub_amd import _lib
    f, n = ctypes.c_void_p(4096), ctypes.c_void_p(0)

    def attn(L, H, dqk, dv, N, nb, td=f):
        ld = 2 * H * (dqk + dv)
        fwd = ("rh_hstu_attn_fwd", f, ld, 2, L, H, dqk, dv, td, f, f, f, N, nb, 0, 1, 1.0, 0.5, f, n)
        bwd = ("rh_hstu_attn_bwd", f, ld, 2, L, H, dqk, dv, td, f, f, f, N, nb, 0, 1, 1.0, 0.5, f, f, f, f, f, f, n)
        return fwd, bwd

    for args, what in ((attn(1025, 1, 8, 8, 1025, 16), "L=1025"), (attn(65, 1, 8, 8, 64, 16), "L=65"),
                       (attn(8, 1, 65, 8, 8, 16), "dqk=65"), (attn(8, 1, 8, 65, 8, 16), "dv=65"),
                       (attn(8, 1, 0, 8, 8, 16), "dqk=0"), (attn(8, 1, 8, 8, 8, 1024), "num_time_buckets=1024")):
        for call in args:
            with pytest.raises(RuntimeError, match=what):
                _lib.call(*call)
    assert _lib.call("rh_hstu_attn_nparts", 3, 65, 2) == 3 * 2 * 2
    for M, D, V, t1 in ((0, 8, 10, 1.0), (4, 0, 10, 1.0), (4, 8, 1, 1.0), (4, 8, 10, 0.0)):
        with pytest.raises(RuntimeError, match="unsupported"):
            _lib.call("rh_hstu_head_fwd", f, f, n, f, M, D, V, t1, 1.0, 0, f, f, f, f, f, n, n)
        with pytest.raises(RuntimeError, match="unsupported"):
            _lib.call("rh_hstu_head_bwd", f, f, n, f, f, f, f, M, D, V, t1, 1.0, f, f, f, n, n)
