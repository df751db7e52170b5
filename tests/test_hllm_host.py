"""HLLM without a GPU: public names, constructor checks, state_dict keys / shapes / seeded initial tensors against the
reference's fixtures, a float64 numpy restatement of the causal softmax attention (forward, backward, bias-table gradient)
and of the transformer block checked against torch autograd on the CPU and against hllm_layers.npz, the bucket rule
against torch's integers, and the shape limits of the C entry points."""
import json

import numpy as np
import pytest
import torch

from conftest import golden_state, load_golden
from torch_rechub_amd.models.generative import HLLMModel
from torch_rechub_amd.models.generative.hllm import HLLMTransformerBlock
from torch_rechub_amd.utils.hstu_utils import RelPosBias

MODEL_CFGS = ["bias_time_ce", "nobias_notime_nce", "odd_bias_time_nce"]


# ---- float64 numpy restatement ------------------------------------------------------------------------------------------
def np_buckets(L, N, nb):
    """(L, L) bucket(i, j) = min(|i - j|, N) * (nb - 1) // N."""
    i = np.arange(L)
    d = np.minimum(np.abs(i[None, :] - i[:, None]), N)
    return d * (nb - 1) // N


def np_softmax_attention(q, k, v, H, N, table=None, scale=None, keep=None):
    """q, k, v (B, L, H dh); table (nb, H) or None; keep (B, H, L, L) dropout multipliers (0 or 1 / (1 - p)) or None.
    Returns (out (B, L, H dh), cache for the backward)."""
    q, k, v = (np.asarray(t, np.float64) for t in (q, k, v))
    B, L, W = q.shape
    dh = W // H
    scale = dh**-0.5 if scale is None else scale
    qh, kh, vh = (t.reshape(B, L, H, dh).transpose(0, 2, 1, 3) for t in (q, k, v))
    s = np.einsum("bhid,bhjd->bhij", qh, kh) * scale
    bk = None
    if table is not None:
        bk = np_buckets(L, N, table.shape[0])
        s = s + np.asarray(table, np.float64)[bk].transpose(2, 0, 1)[None]
    causal = np.tril(np.ones((L, L), bool))
    s = np.where(causal, s, -np.inf)
    p = np.exp(s - s.max(-1, keepdims=True))
    p = p / p.sum(-1, keepdims=True)
    pd = p if keep is None else p * keep
    out = np.einsum("bhij,bhjd->bhid", pd, vh).transpose(0, 2, 1, 3).reshape(B, L, W)
    return out, (qh, kh, vh, p, pd, keep, bk, scale, None if table is None else table.shape[0])


def np_softmax_attention_bwd(cache, g_out):
    """-> g_q, g_k, g_v (B, L, H dh), g_table (nb, H) or None."""
    qh, kh, vh, p, pd, keep, bk, scale, nb = cache
    B, H, L, dh = qh.shape
    go = np.asarray(g_out, np.float64).reshape(B, L, H, dh).transpose(0, 2, 1, 3)
    g_v = np.einsum("bhij,bhid->bhjd", pd, go)
    g_pd = np.einsum("bhid,bhjd->bhij", go, vh)
    g_p = g_pd if keep is None else g_pd * keep
    g_s = p * (g_p - (p * g_p).sum(-1, keepdims=True))
    g_q = np.einsum("bhij,bhjd->bhid", g_s, kh) * scale
    g_k = np.einsum("bhij,bhid->bhjd", g_s, qh) * scale
    g_table = None
    if bk is not None:
        g_table = np.zeros((nb, H))
        per = g_s.sum(0)  # (H, L, L); entries above the diagonal are exactly zero
        for c in range(nb):
            g_table[c] = per[:, bk == c].sum(-1)
    back = lambda t: t.transpose(0, 2, 1, 3).reshape(B, L, H * dh)
    return back(g_q), back(g_k), back(g_v), g_table


def np_layer_norm(x, w, b, eps=1e-5):
    mu = x.mean(-1, keepdims=True)
    var = ((x - mu)**2).mean(-1, keepdims=True)
    return (x - mu) / np.sqrt(var + eps) * w + b


def np_block(x, sd, H, N, table):
    """HLLMTransformerBlock.forward (dropout 0) in float64 from a state_dict of numpy arrays."""
    sd = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    lin = lambda t, n: t @ sd[n + ".weight"].T + sd[n + ".bias"]
    x = np.asarray(x, np.float64)
    h = np_layer_norm(x, sd["norm1.weight"], sd["norm1.bias"])
    a, _ = np_softmax_attention(lin(h, "W_Q"), lin(h, "W_K"), lin(h, "W_V"), H, N, table)
    x = x + lin(a, "W_O")
    h = np_layer_norm(x, sd["norm2.weight"], sd["norm2.bias"])
    return x + lin(np.maximum(lin(h, "ffn.0"), 0), "ffn.3")


def torch_attention(q, k, v, H, N, table, keep=None):
    """The reference's dense formulation in torch (any dtype), for autograd on the CPU."""
    B, L, W = q.shape
    dh = W // H
    qh, kh, vh = (t.view(B, L, H, dh).transpose(1, 2) for t in (q, k, v))
    s = torch.matmul(qh, kh.transpose(-2, -1)) * dh**-0.5
    s = s.masked_fill(~torch.tril(torch.ones(L, L, dtype=torch.bool)), float("-inf"))
    if table is not None:
        bk = torch.from_numpy(np_buckets(L, N, table.shape[0]))
        s = s + table[bk].permute(2, 0, 1).unsqueeze(0)
    p = torch.softmax(s, -1)
    if keep is not None:
        p = p * keep
    return torch.matmul(p, vh).transpose(1, 2).reshape(B, L, W)


def attention_case(B, L, H, dh, N, nb, seed, p_drop=0.0):
    g = torch.Generator().manual_seed(seed)
    q, k, v = (torch.randn(B, L, H * dh, generator=g) for _ in range(3))
    table = 0.5 * torch.randn(nb, H, generator=g) if nb else None
    gout = torch.randn(B, L, H * dh, generator=g)
    keep = None
    if p_drop:
        keep = (torch.rand(B, H, L, L, generator=g) >= p_drop).double() / (1 - p_drop)
    return q, k, v, table, gout, keep


# ---- tests --------------------------------------------------------------------------------------------------------------
def test_public_names():
    import torch_rechub_amd.models.generative as G
    from torch_rechub_amd import integration, ops
    assert G.HLLMModel is HLLMModel and G.HLLMTransformerBlock is HLLMTransformerBlock
    assert "HLLMModel" in integration._MODELS["generative"] and "HSTUModel" in integration._MODELS["generative"]
    assert callable(ops.softmax_attention)
    assert hasattr(HLLMModel, "hidden_and_head")


def test_constructor_errors():
    emb = torch.randn(10, 8)
    with pytest.raises(ValueError, match=r"item_embeddings.shape\[0\]=10 != vocab_size=11"):
        HLLMModel(emb, 11, d_model=8, n_heads=2)
    with pytest.raises(ValueError, match=r"item_embeddings.shape\[1\]=8 != d_model=12"):
        HLLMModel(emb, 10, d_model=12, n_heads=2)
    with pytest.raises(AssertionError, match="d_model must be divisible by n_heads"):
        HLLMModel(emb, 10, d_model=8, n_heads=3)
    with pytest.raises(AssertionError, match="d_model must be divisible by n_heads"):
        HLLMTransformerBlock(10, 4)
    m = HLLMModel(emb, 10, d_model=8, n_heads=2, n_layers=1, max_seq_len=4, num_time_buckets=5, time_bucket_fn="cube")
    with pytest.raises(ValueError, match="Unsupported time_bucket_fn: cube"):
        m._time_diff_to_bucket(torch.zeros(1, 2))
    with pytest.raises(IndexError, match="index out of range"):
        m.hidden_and_head(torch.ones(2, 5, dtype=torch.long))
    assert m.temperature == 0.07 and not m.item_embeddings.requires_grad


def test_item_embeddings_from_a_path_and_normalised(tmp_path):
    emb = torch.randn(6, 4)
    emb[0] = 0
    path = str(tmp_path / "emb.pt")
    torch.save(emb, path)
    m = HLLMModel(path, 6, d_model=4, n_heads=2, n_layers=1, max_seq_len=4, use_time_embedding=False)
    want = torch.nn.functional.normalize(emb, dim=-1, eps=1e-8)
    assert torch.equal(m.item_embeddings, want) and torch.all(m.item_embeddings[0] == 0)
    assert "item_embeddings" in m.state_dict() and "item_embeddings" not in dict(m.named_parameters())


@pytest.mark.parametrize("cfg", MODEL_CFGS)
def test_state_dict_keys_shapes_and_seeded_init_against_fixture(cfg):
    gold = load_golden(f"model_hllm_{cfg}.npz")
    kw = json.loads(str(gold["cfg"]))
    kw.pop("loss_type")
    torch.manual_seed(2022)
    m = HLLMModel(torch.from_numpy(gold["item_embeddings_raw"]), 23, n_layers=2, max_seq_len=9, dropout=0.0,
                  num_time_buckets=16, **kw)
    sd = m.state_dict()
    assert list(sd) == [str(s) for s in gold["sd_keys"]]
    for k, v in sd.items():  # the reference's creation order: a seeded construction gives its initial tensors
        assert tuple(v.shape) == gold["sd0." + k].shape, k
        assert np.array_equal(v.numpy(), gold["sd0." + k]), k
    if kw["use_time_embedding"]:  # _init_weights overwrites the padding row
        assert np.abs(gold["sd0.time_embedding.weight"][0]).max() > 0
        assert m.time_embedding.weight.shape[0] == 17 and m.time_embedding.padding_idx == 0
    m.load_state_dict(golden_state(gold, "sd3."))


def test_time_buckets_are_minutes_clamped_below_the_table():
    m = HLLMModel(torch.randn(5, 4), 5, d_model=4, n_heads=2, n_layers=1, max_seq_len=4, num_time_buckets=7)
    t = torch.tensor([[0, 59, 60, 239, 240, 60 * 36, 60 * 49, 10**9, -5]])
    assert m._time_diff_to_bucket(t).tolist() == [[0, 0, 1, 1, 2, 6, 6, 6, 0]]
    m.time_bucket_fn = "log"
    assert m._time_diff_to_bucket(torch.tensor([[0, 60, 163, 164, 10**9]])).tolist() == [[0, 0, 0, 1, 6]]


@pytest.mark.parametrize("N,nb", [(9, 32), (9, 4), (5, 1), (40, 7), (256, 32), (200, 33), (7, 2)])
def test_bucket_rule_against_torch_integers(N, nb):
    m = RelPosBias(2, N, nb)
    for L in sorted({1, 2, N // 2 + 1, N}):
        pos = torch.arange(L)
        want = m._relative_position_bucket(pos[None, :] - pos[:, None]).numpy()
        got = np_buckets(L, N, nb)
        assert np.array_equal(got, want) and got.max() <= nb - 1 and got.min() >= 0
        # the kernel's int arithmetic: by diagonal, d < N always (L <= N)
        for d in range(L):
            assert (min(d, N) * (nb - 1)) // N == got[d, 0]


def test_relposbias_against_fixture():
    gold = load_golden("hllm_layers.npz")
    assert RelPosBias(3, 9).rel_pos_bias_table.shape == (32, 3)
    t = RelPosBias(3, 9, 16).rel_pos_bias_table
    assert float(t.detach().abs().max()) <= 0.25
    for N, nb, L in gold["relpos.cfgs"]:
        k = f"relpos.{N}_{nb}_{L}."
        m = RelPosBias(2, int(N), int(nb))
        with torch.no_grad():
            m.rel_pos_bias_table.copy_(torch.from_numpy(gold[k + "table"]))
        assert np.array_equal(m(int(L)).detach().numpy(), gold[k + "bias"])
        want = gold[k + "table"][np_buckets(int(L), int(N), int(nb))].transpose(2, 0, 1)[None]
        assert np.array_equal(want, gold[k + "bias"])


@pytest.mark.parametrize("case", [(2, 7, 3, 4, 9, 8, 0.0), (3, 33, 2, 5, 40, 7, 0.0), (2, 70, 1, 3, 70, 32, 0.0),
                                  (2, 9, 2, 6, 9, 0, 0.0), (2, 12, 2, 4, 16, 5, 0.3)])
def test_numpy_attention_against_torch_autograd(case):
    B, L, H, dh, N, nb, p = case
    q, k, v, table, gout, keep = attention_case(B, L, H, dh, N, nb, seed=L, p_drop=p)
    tq, tk, tv = (t.double().requires_grad_(True) for t in (q, k, v))
    tt = table.double().requires_grad_(True) if table is not None else None
    out = torch_attention(tq, tk, tv, H, N, tt, keep)
    out.backward(gout.double())
    ref, cache = np_softmax_attention(q.numpy(), k.numpy(), v.numpy(), H, N, None if table is None else table.numpy(),
                                      keep=None if keep is None else keep.numpy())
    np.testing.assert_allclose(ref, out.detach().numpy(), rtol=1e-11, atol=1e-12)
    gq, gk, gv, gt = np_softmax_attention_bwd(cache, gout.numpy())
    for got, want in ((gq, tq.grad), (gk, tk.grad), (gv, tv.grad)):
        np.testing.assert_allclose(got, want.numpy(), rtol=1e-10, atol=1e-11)
    if table is not None:
        np.testing.assert_allclose(gt, tt.grad.numpy(), rtol=1e-10, atol=1e-11)


def block_cfgs():
    return json.loads(str(load_golden("hllm_layers.npz")["block.cfgs"]))


@pytest.mark.parametrize("name", ["d12h3_bias", "d12h3_nobias", "d15h3_bias", "d14h2_bias"])
def test_numpy_block_and_torch_gradients_against_fixture(name):
    gold = load_golden("hllm_layers.npz")
    dm, H, with_bias = block_cfgs()[name]
    k = f"block.{name}."
    sd = {n[len(k + "sd."):]: gold[n] for n in gold.files if n.startswith(k + "sd.")}
    table = gold[k + "table"] if with_bias else None
    out = np_block(gold[k + "x"], sd, H, 9, table)
    np.testing.assert_allclose(out, gold[k + "out"], rtol=2e-5, atol=2e-5)
    # gradients: the same block in torch float64 with the restated attention
    tsd = {n: torch.from_numpy(v).double().requires_grad_(True) for n, v in sd.items()}
    x = torch.from_numpy(gold[k + "x"]).double().requires_grad_(True)
    tt = torch.from_numpy(table).double().requires_grad_(True) if with_bias else None
    F = torch.nn.functional
    lin = lambda t, n: F.linear(t, tsd[n + ".weight"], tsd[n + ".bias"])
    h = F.layer_norm(x, (dm,), tsd["norm1.weight"], tsd["norm1.bias"])
    y = x + lin(torch_attention(lin(h, "W_Q"), lin(h, "W_K"), lin(h, "W_V"), H, 9, tt), "W_O")
    h = F.layer_norm(y, (dm,), tsd["norm2.weight"], tsd["norm2.bias"])
    y = y + lin(F.relu(lin(h, "ffn.0")), "ffn.3")
    np.testing.assert_allclose(y.detach().numpy(), out, rtol=1e-10, atol=1e-11)
    y.backward(torch.from_numpy(gold[k + "g_out"]).double())

    def close(got, want, what):
        np.testing.assert_allclose(got.numpy(), want, rtol=2e-4, atol=2e-5 * max(np.abs(want).max(), 1e-3), err_msg=what)
    close(x.grad, gold[k + "g_x"], "g_x")
    for n, t in tsd.items():
        if n == "W_K.bias":  # shifts every score of a row alike: zero gradient, rounding noise in the fixture
            assert np.abs(gold[k + "grad." + n]).max() < 1e-5 and t.grad.abs().max() < 1e-12
            continue
        close(t.grad, gold[k + "grad." + n], n)
    if with_bias:
        close(tt.grad, gold[k + "g_table"], "g_table")


def test_softmax_attn_entry_points_reject_unsupported_shapes():
    """Argument validation of csrc/hllm.hip at the first shape past each limit: nothing is launched (the pointers are
    never dereferenced)."""
    import ctypes

    from torch_rechub_amd import _lib
    f, n = ctypes.c_void_p(4096), ctypes.c_void_p(0)

    def attn(L, H, dh, N, nb, bias=f, p=0.0, rng=n, ld=None):
        ld = H * dh if ld is None else ld
        fwd = ("rh_softmax_attn_fwd", f, f, f, ld, 2, L, H, dh, bias, N, nb, 0.5, p, rng, rng, f, f, n)
        bwd = ("rh_softmax_attn_bwd", f, f, f, ld, 2, L, H, dh, bias, N, nb, 0.5, p, rng, rng, f, f, f, f, f, f, f, H * dh,
               f, f, n)
        return fwd, bwd

    for args, what in ((attn(1025, 1, 8, 1025, 16), "L=1025"), (attn(65, 1, 8, 64, 16), "L=65"), (attn(0, 1, 8, 8, 16), "L=0"),
                       (attn(8, 1, 129, 8, 16), "head width 129"), (attn(8, 1, 0, 8, 16), "head width 0"),
                       (attn(8, 0, 8, 8, 16), "H=0"), (attn(8, 1, 8, 8, 0), "num_buckets=0"),
                       (attn(8, 2, 8, 8, 4, ld=15), "row stride 15"), (attn(8, 1, 8, 8, 4, p=1.0), "dropout p=1"),
                       (attn(8, 1, 8, 8, 4, p=0.5), "dropout without")):
        for call in args:
            with pytest.raises(RuntimeError, match=what):
                _lib.call(*call)
    with pytest.raises(RuntimeError, match="null"):
        _lib.call("rh_softmax_attn_fwd", n, f, f, 8, 2, 8, 1, 8, n, 8, 0, 0.5, 0.0, n, n, f, f, n)
    # an empty batch returns before any launch, with or without a bias
    assert _lib.call(*attn(8, 1, 8, 8, 0, bias=n)[0][:5], 0, *attn(8, 1, 8, 8, 0, bias=n)[0][6:]) == 0
    assert _lib.call("rh_softmax_attn_nparts", 3, 65, 2) == 3 * 2 * 2 + 2
    # the head's backward without a weight gradient must not be handed a bias gradient
    with pytest.raises(RuntimeError, match="null"):
        _lib.call("rh_hstu_head_bwd", f, f, f, f, f, f, f, 4, 8, 10, 1.0, 1.0, n, f, n, f, n)
