"""HLLM on the MI355X: the causal softmax attention kernels of csrc/hllm.hip against the float64 numpy restatement over
the supported head widths and lengths, bitwise repeatable backwards, the block and the model against the reference's
fixtures (outputs, loss, gradients, the three-step SeqTrainer trajectory), dropout on the weights, the captured step, and
the memory bounds of the attention and of the frozen head.  Tile and chunk edges, many-partial bias-table sums, the guard
and the backward under dropout against float64 are in test_gpu_session_hllm_shapes.py."""
import json

import numpy as np
import pytest
import torch

from test_hllm_host import np_softmax_attention, np_softmax_attention_bwd, torch_attention

pytestmark = pytest.mark.gpu

MODEL_CFGS = ["bias_time_ce", "nobias_notime_nce", "odd_bias_time_nce"]


def dev():
    return torch.device("cuda:0")


def attn_inputs(B, L, H, dh, nb, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(B, L, 3 * H * dh, generator=g)
    table = 0.5 * torch.randn(nb, H, generator=g) if nb else None
    gout = torch.randn(B, L, H * dh, generator=g)
    return qkv, table, gout


def run_attn(qkv, table, gout, H, N, strided, p=0.0, training=True):
    """-> out, g_q, g_k, g_v, g_table on the CPU.  strided: q, k, v are column blocks of ONE (B, L, 3 W) tensor."""
    from torch_rechub_amd import ops
    W = qkv.shape[2] // 3
    tt = table.to(dev()).requires_grad_(True) if table is not None else None
    if strided:
        x = qkv.to(dev()).requires_grad_(True)
        q, k, v = x[..., :W], x[..., W:2 * W], x[..., 2 * W:]
    else:
        q, k, v = (qkv[..., i * W:(i + 1) * W].contiguous().to(dev()).requires_grad_(True) for i in range(3))
    out = ops.softmax_attention(q, k, v, H, N, bias_table=tt, dropout_p=p, training=training)
    out.backward(gout.to(dev()))
    if strided:
        gq, gk, gv = (x.grad[..., i * W:(i + 1) * W].cpu() for i in range(3))
    else:
        gq, gk, gv = q.grad.cpu(), k.grad.cpu(), v.grad.cpu()
    return out.detach().cpu(), gq, gk, gv, None if tt is None else tt.grad.cpu()


# (B, L, H, dh, max_seq_len, num_buckets (0: no bias), strided): every head width of {1, 4, 32, 50, 64, 96, 128}, every
# length of {1, 7, 33, 200, 256, 1024} and every head count of {1, 3, 16} at least once, with and without the bias
ATTN_CASES = [(2, 1, 1, 1, 1, 0, False), (3, 7, 3, 4, 9, 16, False), (2, 33, 3, 50, 40, 32, True),
              (4, 200, 16, 32, 200, 32, False), (2, 256, 3, 64, 256, 32, True), (1, 1024, 1, 96, 1024, 32, False),
              (2, 200, 16, 128, 256, 32, True), (1, 1024, 3, 128, 1024, 5, False), (2, 256, 1, 128, 300, 0, True),
              (3, 33, 16, 4, 33, 1, False), (2, 7, 1, 50, 7, 0, False)]


@pytest.mark.parametrize("case", ATTN_CASES)
def test_attention_kernel_against_float64(case):
    """Tolerance: rtol 1e-4 and an absolute floor of 2e-6 of the tensor's largest magnitude (test_gpu_hstu.py's, scaled;
    1e-4 for the bias table's gradient as there).  Softmax adds an exponential and a division per element and the
    gradients are sums over up to 1024 keys, so the floor is raised to 4 x the error of an fp32 torch CPU evaluation of
    the same case against the float64 one where that is larger: the kernel's k-ordered fp32 chains and torch's blocked
    fp32 sums round alike per operation and differ in summation order only, which is worth a small factor.  The bound
    never looks at the kernel's output."""
    B, L, H, dh, N, nb, strided = case
    qkv, table, gout = attn_inputs(B, L, H, dh, nb, seed=L + H + dh)
    W = H * dh
    q, k, v = (qkv[..., i * W:(i + 1) * W] for i in range(3))
    ref, cache = np_softmax_attention(q.numpy(), k.numpy(), v.numpy(), H, N, None if table is None else table.numpy())
    wants = (ref,) + np_softmax_attention_bwd(cache, gout.numpy())
    # fp32 on the CPU against float64
    cq, ck, cv = (t.clone().requires_grad_(True) for t in (q, k, v))
    ct = table.clone().requires_grad_(True) if table is not None else None
    co = torch_attention(cq, ck, cv, H, N, ct)
    co.backward(gout)
    cpu32 = (co.detach(), cq.grad, ck.grad, cv.grad, None if ct is None else ct.grad)
    gots = run_attn(qkv, table, gout, H, N, strided)
    names = ("out", "g_q", "g_k", "g_v", "g_table")
    fails = []
    for name, got, want, c32 in zip(names, gots, wants, cpu32):
        if want is None:
            assert got is None
            continue
        scale = max(float(np.abs(want).max()), 1e-30)
        e32 = float(np.abs(c32.numpy() - want).max())
        atol = max((1e-4 if name == "g_table" else 2e-6) * scale, 4 * e32)
        err = np.abs(got.numpy() - want)
        worst = float((err - 1e-4 * np.abs(want)).max())
        print(f"{case} {name}: max|want| {scale:.3e} fp32-cpu err {e32:.3e} kernel err {float(err.max()):.3e} atol {atol:.3e}")
        assert np.isfinite(got.numpy()).all(), name
        if worst > atol:
            fails.append((name, worst, atol))
    assert not fails, fails


def test_online_softmax_rescale_with_a_late_spike():
    """A key far down the row whose score jumps the running maximum by ~60: the tiles before it must be rescaled."""
    B, L, H, dh = 1, 200, 1, 32
    qkv, table, gout = attn_inputs(B, L, H, dh, 8, seed=11)
    qkv[0, 150, dh:2 * dh] = 12.0 * qkv[0, 199, :dh] / qkv[0, 199, :dh].norm() * 5  # k_150 aligned with q_199
    qkv[0, 199, :dh] *= 3
    q, k, v = (qkv[..., i * dh:(i + 1) * dh] for i in range(3))
    ref, cache = np_softmax_attention(q.numpy(), k.numpy(), v.numpy(), H, 200, table.numpy())
    wants = (ref,) + np_softmax_attention_bwd(cache, gout.numpy())
    gots = run_attn(qkv, table, gout, H, 200, False)
    for got, want in zip(gots, wants):
        np.testing.assert_allclose(got.numpy(), want, rtol=1e-4, atol=1e-5 * np.abs(want).max())


def test_backward_twice_bitwise_identical():
    qkv, table, gout = attn_inputs(8, 200, 16, 128, 32, seed=3)
    a = run_attn(qkv, table, gout, 16, 200, False)
    b = run_attn(qkv, table, gout, 16, 200, False)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    from torch_rechub_amd import ops
    rng = ops._dropout_rng(dev())
    rng0 = rng.clone()
    a = run_attn(qkv, table, gout, 16, 200, True, p=0.2)
    rng.copy_(rng0)
    b = run_attn(qkv, table, gout, 16, 200, True, p=0.2)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


# ---- dropout on the attention weights -------------------------------------------------------------------------------------
@pytest.mark.parametrize("p", [0.1, 0.5])
def test_dropout_on_the_weights(p):
    """v = identity per head (dh = L = 64) makes the output row i the dropped weights of query i."""
    from torch_rechub_amd import ops
    B, L, H = 4, 64, 2
    g = torch.Generator().manual_seed(17)
    q, k = (0.5 * torch.randn(B, L, H * L, generator=g).to(dev()) for _ in range(2))
    v = torch.eye(L).repeat(B, 1, H).to(dev()).requires_grad_(True)
    table = (0.3 * torch.randn(8, H, generator=g)).to(dev())
    rng = ops._dropout_rng(dev())
    rng0 = rng.clone()
    w0 = ops.softmax_attention(q, k, v, H, L, bias_table=table).detach().view(B, L, H, L)
    assert torch.equal(rng, rng0)  # p = 0 draws nothing
    wd = ops.softmax_attention(q, k, v, H, L, bias_table=table, dropout_p=p)
    assert int(rng[1]) == int(rng0[1]) + 1
    wdv = wd.detach().view(B, L, H, L)
    causal = torch.tril(torch.ones(L, L, dtype=torch.bool, device=dev()))[None, :, None, :].expand(B, L, H, L)
    assert torch.all(w0[causal] > 0) and torch.all(w0[~causal] == 0) and torch.all(wdv[~causal] == 0)
    kept = (wdv != 0) & causal
    n = int(causal.sum())
    frac = float(kept.sum()) / n
    bound = 5 * (p * (1 - p) / n)**0.5  # five standard deviations of the binomial mean
    assert abs(frac - (1 - p)) <= bound, (frac, bound)
    np.testing.assert_allclose(wdv[kept].cpu().numpy(), (w0[kept] / (1 - p)).cpu().numpy(), rtol=2e-6, atol=0)
    # the backward re-derives the forward's mask: d sum(out) / d v[b, j, h, :] = the column sums of the dropped weights
    wd.sum().backward()
    want = wdv.sum(1)  # (B, H, L keys)
    got = v.grad.view(B, L, H, L).permute(0, 2, 1, 3)  # (B, H, keys, dh): equal over dh
    np.testing.assert_allclose(got.cpu().numpy(), want[..., None].expand_as(got).cpu().numpy(), rtol=1e-5, atol=1e-6)
    # the same (seed, counter) gives the same bits, the next call another mask
    rng.copy_(rng0)
    again = ops.softmax_attention(q, k, v, H, L, bias_table=table, dropout_p=p).detach()
    assert torch.equal(again, wd.detach())
    nxt = ops.softmax_attention(q, k, v, H, L, bias_table=table, dropout_p=p).detach()
    assert not torch.equal((nxt != 0), (again != 0))
    # eval ignores p
    assert torch.equal(ops.softmax_attention(q, k, v, H, L, bias_table=table, dropout_p=p, training=False).detach(),
                       w0.view(B, L, H * L))


# ---- the block and the model against the reference's fixtures (tools/gen_golden_hllm.py) ---------------------------------
def close(got, want, what, rtol=2e-4, atol_rel=2e-5):
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    scale = max(float(np.abs(want).max()), 1e-12)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol_rel * scale, err_msg=what)


@pytest.mark.parametrize("name", ["d12h3_bias", "d12h3_nobias", "d15h3_bias", "d14h2_bias"])
def test_block_against_reference_fixture(name):
    from conftest import golden_state, load_golden
    from torch_rechub_amd.models.generative.hllm import HLLMTransformerBlock
    from torch_rechub_amd.utils.hstu_utils import RelPosBias
    gold = load_golden("hllm_layers.npz")
    dm, H, with_bias = json.loads(str(gold["block.cfgs"]))[name]
    k = f"block.{name}."
    m = HLLMTransformerBlock(dm, H, 0.0)
    m.load_state_dict(golden_state(gold, k + "sd."))
    m.to(dev())
    rp = None
    if with_bias:
        rp = RelPosBias(H, 9, 8)
        with torch.no_grad():
            rp.rel_pos_bias_table.copy_(torch.from_numpy(gold[k + "table"]))
        rp.to(dev())
    x = torch.from_numpy(gold[k + "x"]).to(dev()).requires_grad_(True)
    y = m(x, rel_pos_bias=rp)
    close(y, gold[k + "out"], k + "out")
    y.backward(torch.from_numpy(gold[k + "g_out"]).to(dev()))
    close(x.grad, gold[k + "g_x"], k + "g_x")
    gmax = max(float(np.abs(gold[k + "grad." + n]).max()) for n, _ in m.named_parameters())
    for n, p in m.named_parameters():
        if n == "W_K.bias":  # shifts every score of a row alike: the gradient is zero, rounding noise on both sides
            assert float(p.grad.abs().max()) <= 1e-5 * gmax and float(np.abs(gold[k + "grad." + n]).max()) <= 1e-5 * gmax
            continue
        close(p.grad, gold[k + "grad." + n], k + "grad." + n, rtol=5e-4, atol_rel=5e-5)
    if with_bias:
        close(rp.rel_pos_bias_table.grad, gold[k + "g_table"], k + "g_table", rtol=5e-4, atol_rel=5e-5)


def fixture_model(gold, dropout=0.0):
    from conftest import golden_state
    from torch_rechub_amd.models.generative import HLLMModel
    kw = json.loads(str(gold["cfg"]))
    loss_type = kw.pop("loss_type")
    model = HLLMModel(torch.from_numpy(gold["item_embeddings_raw"]), 23, n_layers=2, max_seq_len=9, dropout=dropout,
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
    gold = load_golden(f"model_hllm_{cfg}.npz")
    model, loss_type = fixture_model(gold)
    lr, wd = float(gold["train.lr"]), float(gold["train.wd"])
    trainer = SeqTrainer(model, device="cuda:0", loss_type=loss_type, optimizer_params={"lr": lr, "weight_decay": wd})
    assert trainer.fused
    batches = fixture_batches(gold)
    tok, _, td, tg = (t.to(dev()) for t in batches[0])
    model.eval()
    with torch.no_grad():
        close(model(tok, td), gold["logits"], "logits")
    model.train()
    close(model(tok, td), gold["train_logits"], "training logits")
    loss = trainer._loss(tok, td, tg)  # the fused next-token loss on the frozen item table
    assert abs(loss.item() - float(gold["loss"])) <= 2e-5 * abs(float(gold["loss"])), (loss.item(), float(gold["loss"]))
    model.zero_grad()
    loss.backward()
    gmax = max(float(np.abs(gold["grad." + n]).max()) for n, _ in model.named_parameters())
    for n, p in model.named_parameters():
        want = gold["grad." + n]
        if n.endswith("W_K.bias"):  # zero by the softmax's shift invariance: rounding noise on both sides
            assert float(np.abs(want).max()) <= 1e-5 * gmax and float(p.grad.abs().max()) <= 1e-5 * gmax, n
            continue
        close(p.grad, want, cfg + " grad." + n, rtol=1e-3, atol_rel=1e-4)
    if model.use_time_embedding:  # the padding row holds Xavier values and takes no gradient
        assert torch.all(model.time_embedding.weight.grad[0] == 0) and float(model.time_embedding.weight[0].detach().abs().max()) > 0
    model.zero_grad(set_to_none=True)
    mean_loss = trainer.train_one_epoch(batches)
    assert abs(mean_loss - float(gold["train.mean_loss"])) <= 1e-4 * abs(float(gold["train.mean_loss"]))
    assert_state_follows_reference_trajectory(gold, model.state_dict(), cfg)
    assert torch.equal(model.item_embeddings.cpu(), torch.from_numpy(gold["sd0.item_embeddings"]))


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_graph_step_equals_eager_step_bitwise(p):
    """SeqTrainer(use_graph=True): two eager warm-up steps, then the captured step replayed for every later batch; with
    p > 0 each replay reads and advances the device-resident dropout counter, so it draws the mask the eager run draws
    at that step.  Losses and states equal bit for bit."""
    from conftest import load_golden
    from torch_rechub_amd import ops
    from torch_rechub_amd.trainers import SeqTrainer
    gold = load_golden("model_hllm_bias_time_ce.npz")
    batches = fixture_batches(gold) * 2
    rng = ops._dropout_rng(dev())
    rng0 = rng.clone()
    runs = []
    for use_graph in (False, True):
        rng.copy_(rng0)  # the same dropout stream for both runs
        model, loss_type = fixture_model(gold, dropout=p)
        t = SeqTrainer(model, device="cuda:0", loss_type=loss_type, use_graph=use_graph,
                       optimizer_params={"lr": 1e-2, "weight_decay": 1e-3, "capturable": True})
        model.train()
        losses, states = [], []
        for b in batches:
            losses.append(t.train_step(*(x.to(dev()) for x in (b[0], b[2], b[3]))).clone())
            states.append({k: v.clone() for k, v in model.state_dict().items()})
        runs.append((t, losses, states, rng.clone()))
    (_, le, se, re), (tg, lg, sg, rg) = runs
    assert len(tg._graphs) == 1
    assert torch.equal(re, rg)
    for i in range(len(batches)):
        assert torch.equal(le[i], lg[i]), i
        for k in se[i]:
            assert torch.equal(se[i][k], sg[i][k]), (i, k)
    if p > 0:  # every step, replayed ones included, drew its nine masks (input, and four per block) from the counter
        assert int(rg[1]) - int(rng0[1]) == 9 * len(batches)


# ---- memory ---------------------------------------------------------------------------------------------------------------
def test_attention_memory_below_one_score_tensor():
    """B 64, L 256, H 16, dh 128: the peak of one attention forward + backward above its inputs stays below the output,
    the output gradient, the three input gradients and the row statistics plus ONE (B, H, L, L) fp32 tensor (the eager
    formulation keeps five of those)."""
    from torch_rechub_amd import ops
    B, L, H, dh = 64, 256, 16, 128
    g = torch.Generator().manual_seed(0)
    q, k, v = (torch.randn(B, L, H * dh, generator=g).to(dev()).requires_grad_(True) for _ in range(3))
    table = torch.zeros(32, H, device=dev(), requires_grad=True)
    gout = torch.randn(B, L, H * dh, generator=g).to(dev())

    def step():
        out = ops.softmax_attention(q, k, v, H, L, bias_table=table, dropout_p=0.1)
        out.backward(gout)
        q.grad = k.grad = v.grad = table.grad = None

    step()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    tensors = 5 * B * L * H * dh * 4 + 2 * B * H * L * 4  # out, g_out's contiguous form, g_q, g_k, g_v; lse, delta
    assert extra < tensors + B * H * L * L * 4, (extra, tensors)


def test_frozen_head_allocates_no_table_gradient():
    """V 100 000, D 512: the step's peak above the resident state stays below what must exist -- h and its gradient, the
    normalised h and its autograd copies (six (M, D) tensors), the per-row statistics and the forward's per-split
    partials -- plus HALF a (V, D) buffer; the (V, D) gradient (and the (rsplit, V, D + 1) partials) would break it."""
    from torch_rechub_amd import _lib, ops
    M, D, V = 512, 512, 100000
    g = torch.Generator().manual_seed(0)
    w = torch.nn.functional.normalize(torch.randn(V, D, generator=g)).to(dev())
    h = torch.randn(M, D, generator=g).to(dev()).requires_grad_(True)
    labels = torch.randint(1, V, (M,), generator=g).to(dev())

    def step():
        loss = ops.next_token_loss(torch.nn.functional.normalize(h, dim=-1, eps=1e-8), w, None, labels, temperature=0.07)
        loss.backward()
        out = (loss.item(), h.grad.clone())
        h.grad = None
        return out

    l0, g0 = step()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    step()
    torch.cuda.synchronize()
    extra = torch.cuda.max_memory_allocated() - base
    nsplit = _lib.call("rh_hstu_head_nsplit", M, V)
    must = 6 * M * D * 4 + 4 * M * 4 + M * nsplit * 2 * 4
    assert extra < must + V * D * 4 // 2, (extra, must)
    # and the gradient is the one the full backward computes
    w2 = w.clone().requires_grad_(True)
    loss = ops.next_token_loss(torch.nn.functional.normalize(h, dim=-1, eps=1e-8), w2, None, labels, temperature=0.07)
    loss.backward()
    assert loss.item() == l0 and torch.equal(h.grad, g0) and w2.grad is not None and w2.grad.shape == (V, D)


# ---- errors and edges -----------------------------------------------------------------------------------------------------
def test_out_of_range_label_raises():
    from conftest import load_golden
    from torch_rechub_amd import ops
    from torch_rechub_amd.trainers import SeqTrainer
    gold = load_golden("model_hllm_bias_time_ce.npz")
    model, loss_type = fixture_model(gold)
    trainer = SeqTrainer(model, device="cuda:0", loss_type=loss_type)
    tok, _, td, tg = (t.to(dev()) for t in fixture_batches(gold)[0])
    tg = tg.clone()
    tg[0] = 23
    trainer.train_step(tok, td, tg)
    with pytest.raises(IndexError, match="target label"):
        ops.check_errors(dev())


def test_empty_batch():
    from torch_rechub_amd import ops
    q, k, v = (torch.zeros(0, 5, 12, device=dev(), requires_grad=True) for _ in range(3))
    table = torch.zeros(4, 3, device=dev(), requires_grad=True)
    out = ops.softmax_attention(q, k, v, 3, 8, bias_table=table, dropout_p=0.1)
    assert out.shape == (0, 5, 12)
    out.sum().backward()
    assert q.grad.shape == (0, 5, 12) and torch.all(table.grad == 0)


def test_sequence_longer_than_max_seq_len_raises():
    from conftest import load_golden
    from torch_rechub_amd import ops
    gold = load_golden("model_hllm_bias_time_ce.npz")
    model, _ = fixture_model(gold)
    model.to(dev())
    with pytest.raises(IndexError, match="index out of range in self"):
        model(torch.ones(2, 10, dtype=torch.long, device=dev()))
    q = torch.zeros(1, 10, 12, device=dev())
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.softmax_attention(q, q, q, 3, 9)
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.softmax_attention(torch.zeros(1, 4, 129, device=dev()), torch.zeros(1, 4, 129, device=dev()),
                              torch.zeros(1, 4, 129, device=dev()), 1, 9)
