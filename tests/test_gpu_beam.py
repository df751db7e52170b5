"""The device beam search on the MI355X: ops.beam_step (csrc/beam.hip) against the numpy step oracle (tests/beam_oracle.py)
over its shape range, its edge cases (-inf and huge logits, the step-one form, ties on the K-th place, dead beams, short
queries), its independence of batch and stride, and TIGERModel.generate(constraint=DeviceTrie) against the recorded beam
search and against the callback path.

Inputs: ``check`` asserts on the CPU, before the GPU is touched, that every neighbouring pair of the first K + 1
candidates of every query is either more than 1e-3 apart in float64 (the margin tools/gen_golden_tiger.py demands of its
recording) or equal by construction -- at float64 distance 0 (bitwise-equal rows and running scores), or both at running
-1e9 with |logp| < 16, where float32 absorbs the log-probability -- so that the tie rule decides.
Comparison: parent, token, node and short exactly; scores within the larger of 2e-6 of the largest magnitude and 4 times
the error of torch's float32 CPU log_softmax + add against float64 on the same inputs (DESIGN 3.f's rule).  Scores of
magnitude 1e8 and above (the -1e9 form) are held to equality, and do not count as the largest magnitude."""
import json
import os

import numpy as np
import pytest
import torch

import beam_oracle as BO
import tiger_oracle as O
from torch_rechub_amd._lib import H

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MARGIN = 1e-3


def dev():
    return torch.device("cuda:0")


def host(trie):
    return [a.cpu().numpy() for a in (trie.child_off, trie.child_tok, trie.child_node)]


def two_level(fans, V, rng):
    """A trie of two-token sequences [i, t]: first-level node 1 + i has fans[i] >= 1 children (random distinct tokens
    below V); the leaves behind them have none.  -> (DeviceTrie on the GPU, the first-level nodes, one leaf)."""
    from torch_rechub_amd.utils.data import DeviceTrie
    seqs = [[i, int(t)] for i, f in enumerate(fans) for t in rng.choice(V, size=f, replace=False)]
    trie = DeviceTrie(seqs, dev())
    return trie, [trie.find([i]) for i in range(len(fans))], trie.find(seqs[0])


def check(res, running, ties):
    for head in res["head"]:
        for x, y in zip(head, head[1:]):
            d = abs(x[1] - y[1])
            absorbed = abs(x[0]) == 1e9 and abs(y[0]) == 1e9 and abs(x[5]) < 16 and abs(y[5]) < 16
            assert d > MARGIN or (ties and (d == 0 or absorbed)), f"candidates {x} and {y} are {d} apart"


def cpu_float32_error(logits, running, res):
    """max |float32 CPU log_softmax + add - float64| over the oracle's selected candidates."""
    B, K = running.shape
    lp32 = torch.log_softmax(torch.from_numpy(np.ascontiguousarray(logits)), -1).numpy()
    lp64 = BO.log_softmax64(logits)
    err = 0.0
    for b in range(B):
        for j in range(K):
            k, t = int(res["parent"][b, j]), int(res["token"][b, j])
            if k >= 0 and abs(float(running[b, k])) < 1e8:
                got = np.float32(running[b, k]) + lp32[b * K + k, t]
                err = max(err, abs(float(got) - (float(running[b, k]) + lp64[b * K + k, t])))
    return err


def run(logits, running, node, trie, ties=False, pad=None):
    """Checks the inputs, runs the step on the GPU, compares with the oracle; -> the GPU outputs as numpy arrays.  pad: the
    rows are the last position of a (B K, pad, V) tensor (row stride pad V)."""
    from torch_rechub_amd import ops
    off, tok, child = host(trie)
    res = BO.step(logits, running, node, off, tok, child)
    check(res, running, ties)
    lg = torch.from_numpy(logits).to(dev())
    if pad:
        wide = torch.full((lg.shape[0], pad, lg.shape[1]), float("nan"), device=dev())
        wide[:, -1, :] = lg
        lg = wide[:, -1, :]
        assert lg.stride(0) == pad * logits.shape[1]
    out = ops.beam_step(lg, torch.from_numpy(running).to(dev()), torch.from_numpy(node).to(dev()), trie)
    got = [t.cpu().numpy() for t in out]
    assert [g.dtype for g in got] == [np.float32, np.int32, np.int32, np.int32, np.int32]
    np.testing.assert_array_equal(got[1], res["parent"])
    np.testing.assert_array_equal(got[2], res["token"])
    np.testing.assert_array_equal(got[3], res["node"])
    np.testing.assert_array_equal(got[4], res["short"])
    want = res["running"]
    exact = ~np.isfinite(want) | (np.abs(want) >= 1e8)
    np.testing.assert_array_equal(got[0][exact], want[exact])
    if (~exact).any():
        tol = max(2e-6 * float(np.abs(want[~exact]).max()), 4 * cpu_float32_error(logits, running, res))
        print(f"scores: max error {float(np.abs(got[0][~exact] - want[~exact]).max()):.3g}, bound {tol:.3g}")
        np.testing.assert_allclose(got[0][~exact], want[~exact], rtol=0, atol=tol)
    return got


def random_case(V, K, B, fans, pattern, scale=3.0, tries=40):
    """The first seed whose inputs pass ``check`` without ties (decided on the CPU).  pattern(rng, level, leaf) -> (B, K)
    nodes."""
    for seed in range(tries):
        rng = np.random.default_rng(1000 * V + 10 * K + B + 7919 * seed)
        trie, level, leaf = two_level(fans, V, rng)
        node = np.asarray(pattern(rng, level, leaf), dtype=np.int32).reshape(B, K)
        logits = (scale * rng.standard_normal((B * K, V))).astype(np.float32)
        running = (-5 * rng.random((B, K))).astype(np.float32)
        res = BO.step(logits, running, node, *host(trie))
        if res["gap"] > MARGIN and all(abs(x[1] - y[1]) > 0 for h in res["head"] for x, y in zip(h, h[1:])):
            return logits, running, node, trie
    raise AssertionError("no seed with a gap above the margin")


def mixed(B, K):
    """Beams on random first-level nodes, about one in five dead, one in five on a leaf (no children)."""
    def pattern(rng, level, leaf):
        node = rng.choice(level, size=(B, K))
        u = rng.random((B, K))
        node[u < 0.2] = -1
        node[(u >= 0.2) & (u < 0.4)] = leaf
        return node
    return pattern


# ---- the shape table --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,K,B,fans,pad", [
    (1, 1, 1, [1], None), (1, 3, 3, [1], 3), (63, 3, 3, [1, 63, 5], None), (64, 4, 1, [64, 1, 7], 3), (65, 5, 3, [65, 64, 1], None),
    (65, 1, 3, [65, 64, 1], 3), (257, 64, 3, [3, 2, 1, 2], None), (257, 5, 1, [65, 64, 1, 30], 3),
    (1000, 5, 3, [65, 64, 1, 200], 3), (1000, 64, 1, [65, 64, 1, 200], None), (1000, 4, 3, [1000, 3], None)])
def test_step_against_the_oracle_over_the_shape_table(V, K, B, fans, pad):
    if V == 1:  # one token: every live beam has the one candidate at logp 0; distinct running scores keep them apart
        rng = np.random.default_rng(K)
        trie, level, leaf = two_level(fans, V, rng)
        node = np.full((B, K), level[0], dtype=np.int32)
        node[0, K - 1] = leaf if K > 1 else level[0]
        logits = rng.standard_normal((B * K, 1)).astype(np.float32)
        running = -(np.arange(B * K, dtype=np.float32).reshape(B, K))
    else:
        logits, running, node, trie = random_case(V, K, B, fans, mixed(B, K))
    run(logits, running, node, trie, pad=pad)


@pytest.mark.parametrize("where", ["first", "last", "throughout", "none_live"])
def test_dead_beams(where):
    K, B, V = 5, 3, 65

    def pattern(rng, level, leaf):
        node = rng.choice(level, size=(B, K))
        if where == "first":
            node[:, 0] = -1
        elif where == "last":
            node[:, K - 1] = -1
        elif where == "throughout":
            node[:, ::2] = -1
        else:
            node[:] = -1
            node[1, 2] = leaf  # a live beam without children adds nothing either
        return node

    logits, running, node, trie = random_case(V, K, B, [65, 64, 1], pattern)
    got = run(logits, running, node, trie)
    if where == "none_live":
        assert got[4].tolist() == [1, 1, 1] and np.isinf(got[0]).all() and (got[1] == -1).all() and (got[3] == -1).all()


@pytest.mark.parametrize("extra", [-1, 0, 1])
def test_k_minus_one_k_and_k_plus_one_candidates(extra):
    """K = 4 beams on nodes with one child each, one of them dead / all live / one with two children."""
    K, B, V = 4, 3, 63
    pattern = {-1: lambda rng, level, leaf: [[level[0], level[1], -1, level[2]]] * B,
               0: lambda rng, level, leaf: [[level[0], level[1], level[1], level[2]]] * B,
               1: lambda rng, level, leaf: [[level[0], level[3], level[1], level[2]]] * B}[extra]
    logits, running, node, trie = random_case(V, K, B, [1, 1, 1, 2], pattern)
    got = run(logits, running, node, trie)
    assert got[4].tolist() == [int(extra < 0)] * B
    if extra < 0:
        assert np.all(got[0][:, 3] == -np.inf) and np.all(got[1][:, 3] == -1) and np.all(got[2][:, 3] == -1)
        assert np.all(got[3][:, 3] == -1) and np.isfinite(got[0][:, :3]).all()


# ---- edge cases -------------------------------------------------------------------------------------------------------------
def test_an_allowed_token_at_minus_inf_is_no_candidate():
    """One live beam on a node with three children, one of them at a -inf logit: with K = 2 it loses to the two finite
    ones; with K = 3 its slot stays unused and the query is short, as the dense formulation (which cannot tell it from a
    masked token) has it."""
    from torch_rechub_amd.utils.data import DeviceTrie
    trie = DeviceTrie([[0, 3], [0, 9], [0, 20]], dev())
    rng = np.random.default_rng(3)
    for K, short in ((2, 0), (3, 1)):
        logits = rng.standard_normal((K, 33)).astype(np.float32)
        logits[:, 9] = -np.inf
        logits[0, [3, 20]] = [4.0, 2.0]
        running = np.zeros((1, K), dtype=np.float32)
        node = np.full((1, K), -1, dtype=np.int32)
        node[0, 0] = trie.find([0])
        got = run(logits, running, node, trie)
        assert got[4].tolist() == [short] and got[2].tolist()[0][:2] == [3, 20] and 9 not in got[2].tolist()[0]
        if K == 3:
            assert (got[0][0, 2], got[1][0, 2], got[2][0, 2], got[3][0, 2]) == (-np.inf, -1, -1, -1)


def test_logits_of_magnitude_1e4_need_the_max_subtraction():
    logits, running, node, trie = random_case(257, 5, 3, [65, 64, 1, 30], mixed(3, 5), scale=1e4)
    assert float(np.abs(logits).max()) > 2e4
    got = run(logits, running, node, trie, pad=3)
    assert np.isfinite(got[0][got[1] >= 0]).all()


@pytest.mark.parametrize("K,c", [(3, 1), (5, 2), (H.RH_BEAM_MAX_K, 3), (4, 4)])
def test_the_step_one_form(K, c):
    """All beams of a query on one node with c children, equal rows, running = [0, -1e9, ...]: the c children of beam 0,
    then beam 1 upwards at exactly -1e9 in (beam, token) order."""
    from torch_rechub_amd.utils.data import DeviceTrie
    B, V = 3, 65
    rng = np.random.default_rng(K * 10 + c)
    toks = sorted(int(t) for t in rng.choice(V, size=c, replace=False))
    trie = DeviceTrie([[0, t] for t in toks], dev())
    rows = np.repeat((2 * rng.standard_normal((B, V))).astype(np.float32), K, axis=0)
    assert float(np.abs(BO.log_softmax64(rows)).max()) < 16
    # (the first c scores: apart by more than the margin)
    running = np.zeros((B, K), dtype=np.float32)
    running[:, 1:] = -1e9
    node = np.full((B, K), trie.find([0]), dtype=np.int32)
    got = run(rows, running, node, trie, ties=True)
    tail = [(k, t) for k in range(1, K) for t in toks][:K - c]
    for b in range(B):
        assert sorted(got[2][b, :c].tolist()) == toks and got[1][b, :c].tolist() == [0] * c
        assert list(zip(got[1][b, c:].tolist(), got[2][b, c:].tolist())) == tail
        assert np.all(got[0][b, c:] == np.float32(-1e9))
    assert got[4].tolist() == [0] * B


@pytest.mark.parametrize("K", [1, 3, 4, 5])
def test_ties_on_the_kth_place(K):
    """Two beams with bitwise-equal rows and running scores on one node {2, 4, 6}; token 2 leads, tokens 4 and 6 are
    equal.  The order is (0, 2), (1, 2), (0, 4), (0, 6), (1, 4), (1, 6): K = 1 cuts between the two beams' equal best, K = 3
    between two equal tokens of beam 0, K = 4 between beam 0 and beam 1, K = 5 between the tokens of beam 1.  (Beams beyond
    the first two are dead.)"""
    from torch_rechub_amd.utils.data import DeviceTrie
    trie = DeviceTrie([[0, 2], [0, 4], [0, 6]], dev())
    rng = np.random.default_rng(K)
    row = rng.standard_normal(63).astype(np.float32)
    row[[2, 4, 6]] = [5.0, 3.0, 3.0]
    logits = np.tile(row, (K, 1))
    running = np.full((1, K), -1.5, dtype=np.float32)
    node = np.full((1, K), -1, dtype=np.int32)
    node[0, :2] = trie.find([0])
    got = run(logits, running, node, trie, ties=True)
    order = [(0, 2), (1, 2), (0, 4), (0, 6), (1, 4), (1, 6)] if K > 1 else [(0, 2)]
    assert list(zip(got[1][0].tolist(), got[2][0].tolist())) == order[:K]


def test_a_query_alone_another_stride_and_a_second_run_give_the_same_bytes():
    from torch_rechub_amd import ops
    B, K, V = 3, 5, 1000
    logits, running, node, trie = random_case(V, K, B, [65, 64, 1, 200], mixed(B, K))
    lg, rn, nd = (torch.from_numpy(a).to(dev()) for a in (logits, running, node))
    base = ops.beam_step(lg, rn, nd, trie)
    again = ops.beam_step(lg, rn, nd, trie)
    wide = torch.zeros((B * K, 2, V + 3), device=dev())
    wide[:, -1, :V] = lg
    strided = ops.beam_step(wide[:, -1, :V], rn, nd, trie)
    assert wide[:, -1, :V].stride(0) == 2 * (V + 3)
    for x, y, z in zip(base, again, strided):
        assert torch.equal(x, y) and torch.equal(x, z)
    for b in range(B):
        alone = ops.beam_step(lg[b * K:(b + 1) * K], rn[b:b + 1], nd[b:b + 1], trie)
        for x, y in zip(base, alone):
            assert torch.equal(x[b:b + 1], y)
    # lse as a function of the row alone: the same row as another beam of another query gives the same score
    swapped = ops.beam_step(lg.flip(0), rn.flip(0, 1), nd.flip(0, 1), trie)
    one = ops.beam_step(lg[:K], rn[:1], nd[:1], trie)[0]
    assert torch.equal(swapped[0][B - 1:], one)


def test_op_refusals():
    from torch_rechub_amd import ops
    from torch_rechub_amd.utils.data import DeviceTrie
    trie = DeviceTrie([[0, 3], [0, 9]], dev())
    lg, rn, nd = torch.zeros(4, 16, device=dev()), torch.zeros(2, 2, device=dev()), torch.zeros(2, 2, dtype=torch.int32, device=dev())
    with pytest.raises(ValueError, match="outside the vocabulary"):
        ops.beam_step(lg[:, :9], rn, nd, trie)
    with pytest.raises(ValueError, match="int32"):
        ops.beam_step(lg, rn, nd.long(), trie)
    with pytest.raises(ValueError, match="logits rows"):
        ops.beam_step(lg[:3], rn, nd, trie)
    with pytest.raises(RuntimeError, match="HIP"):
        ops.beam_step(lg.cpu(), rn, nd, trie)
    empty = ops.beam_step(lg[:0], rn[:0], nd[:0], trie)
    assert [tuple(t.shape) for t in empty] == [(0, 2)] * 4 + [(0,)]


# ---- the model --------------------------------------------------------------------------------------------------------------
def close(got, want, what, rtol=2e-4, atol_rel=2e-5):
    """test_gpu_tiger.py's."""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    scale = max(float(np.abs(want).max()), 1e-12)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol_rel * scale, err_msg=what)


def load_model(tag):
    from torch_rechub_amd.models.generative import TIGERConfig, TIGERModel
    z = np.load(os.path.join(GOLDEN, f"model_tiger_{tag}.npz"))
    cfg = json.loads(str(z["cfg"]))
    arrays = {k[len("param/"):]: z[k] for k in z.files if k.startswith("param/")}
    model = TIGERModel(TIGERConfig.from_dict(cfg))
    keys = json.loads(str(z["keys"]))
    model.load_state_dict({k: torch.tensor(arrays.get(k, arrays["shared.weight"])) for k in keys}, strict=True)
    return z, model.to(dev()), torch.tensor(z["input_ids"]).to(dev()), torch.tensor(z["attention_mask"]).to(dev())


@pytest.mark.parametrize("tag", ["a", "b"])
def test_generate_on_the_trie_matches_the_recorded_beam_search(tag):
    from torch_rechub_amd.utils.data import DeviceTrie
    z, model, ids, mask = load_model(tag)
    cands = z["beam.candidates"].tolist()
    trie = DeviceTrie(cands, dev())
    model.train()  # generate runs in eval mode and puts the mode back
    gen = model.generate(ids, mask, max_new_tokens=10, num_beams=3, num_return_sequences=3, constraint=trie)
    assert model.training
    assert sorted(gen) == ["item_index", "sequences", "sequences_scores"]
    np.testing.assert_array_equal(gen["sequences"].cpu().numpy(), z["beam.sequences"])
    close(gen["sequences_scores"], z["beam.scores"], "beam scores")
    items = gen["item_index"]
    assert items.dtype == torch.int64 and tuple(items.shape) == (ids.shape[0], 3)
    assert [cands[i] for i in items.reshape(-1).tolist()] == z["beam.sequences"].tolist()
    top1 = model.generate(ids, mask, max_new_tokens=4, num_beams=3, num_return_sequences=1, constraint=trie)
    np.testing.assert_array_equal(top1["sequences"].cpu().numpy(), z["beam.sequences"][::3])
    np.testing.assert_array_equal(top1["item_index"].cpu().numpy(), items[:, :1].cpu().numpy())
    close(top1["sequences_scores"], z["beam.scores"][::3], "best scores")


def larger_case(seed):
    """Vocabulary 300, three levels of 40 codes, 200 candidates, 6 queries of 12 tokens; the model's weights from ``seed``."""
    from torch_rechub_amd.models.generative import TIGERConfig, TIGERModel
    rng = np.random.default_rng(seed)
    codes = {tuple(int(2 + 40 * l + c) for l, c in enumerate(rng.integers(0, 40, size=3))) for _ in range(260)}
    cands = [[0, *c, 1] for c in sorted(codes)][:200]
    rng.shuffle(cands)
    torch.manual_seed(seed)
    cfg = TIGERConfig(vocab_size=300, d_model=32, d_kv=8, d_ff=48, num_layers=2, num_heads=4, dropout_rate=0.0,
                      relative_attention_num_buckets=8, relative_attention_max_distance=16)
    model = TIGERModel(cfg)
    ids = rng.integers(2, 300, size=(6, 12))
    mask = np.ones((6, 12), dtype=np.int64)
    mask[1, 9:] = 0
    mask[4, 5:] = 0
    return cfg, model, cands, ids, mask


def oracle_search(cfg, model, cands, ids, mask, K):
    """tiger_oracle's float64 model under the iterated step oracle: -> (sequences, the smallest gap of any step, the error
    of torch's float32 CPU log_softmax + add against float64 on the returned mean scores, along the same selections)."""
    from torch_rechub_amd.utils.data import DeviceTrie
    c = cfg.to_dict()
    P = {k: v.detach().double() for k, v in model.state_dict().items()}
    trie = DeviceTrie(cands)
    off, tok, child = host(trie)
    B = len(ids)
    gap = np.inf
    with torch.no_grad():
        enc = O.stack(P, c, "encoder", ids, mask).repeat_interleave(K, 0)
        m = np.repeat(mask, K, 0)
        seqs = np.zeros((B * K, 1), dtype=np.int64)
        node = np.full((B, K), trie.find([0]), dtype=np.int32)
        running = np.zeros((B, K), dtype=np.float32)
        running[:, 1:] = -1e9
        run32, run64 = running.copy(), running.astype(np.float64)
        for _ in range(trie.depth - 1):
            logits = O.decode(P, c, seqs, enc, m)[:, -1, :].float().numpy()
            res = BO.step(logits, running, node, off, tok, child)
            picked = (np.arange(B)[:, None] * K + res["parent"], res["token"])
            lp32 = torch.log_softmax(torch.from_numpy(logits), -1).numpy()
            run32 = np.take_along_axis(run32, res["parent"].astype(np.int64), 1) + lp32[picked]
            run64 = np.take_along_axis(run64, res["parent"].astype(np.int64), 1) + BO.log_softmax64(logits)[picked]
            for head in res["head"]:  # the -1e9 copies of step one are equal by construction, not by chance
                gap = min([gap] + [abs(x[1] - y[1]) for x, y in zip(head, head[1:]) if abs(x[0]) < 1e8 or abs(y[0]) < 1e8])
            rows = (np.arange(B)[:, None] * K + res["parent"]).reshape(-1)
            seqs = np.concatenate([seqs[rows], res["token"].reshape(-1, 1)], 1)
            running, node = res["running"], res["node"]
    steps = trie.depth - 1
    return seqs, gap, float(np.abs(run32.astype(np.float64) / np.float32(steps) - run64 / steps).max())


def test_generate_on_the_trie_equals_the_callback_path_on_a_larger_model():
    from torch_rechub_amd.utils.data import DeviceTrie, Trie
    K = 5
    for seed in range(8):  # the first seed whose float64 search is decided by more than the margin at every step
        cfg, model, cands, ids, mask = larger_case(seed)
        want, gap, err32 = oracle_search(cfg, model, cands, ids, mask, K)
        if gap > MARGIN:
            break
    else:
        raise AssertionError("no seed with beam gaps above the margin")
    model = model.to(dev())
    ids_d, mask_d = torch.from_numpy(ids).to(dev()), torch.from_numpy(mask).to(dev())
    host_trie = Trie(cands)
    cb = model.generate(ids_d, mask_d, max_new_tokens=6, num_beams=K, num_return_sequences=K,
                        prefix_allowed_tokens_fn=host_trie.def_prefix_allowed_tokens_fn(host_trie))
    on = model.generate(ids_d, mask_d, max_new_tokens=6, num_beams=K, num_return_sequences=K, constraint=DeviceTrie(cands, dev()))
    assert "item_index" not in cb
    np.testing.assert_array_equal(on["sequences"].cpu().numpy(), want)
    np.testing.assert_array_equal(cb["sequences"].cpu().numpy(), want)
    assert [cands[i] for i in on["item_index"].reshape(-1).tolist()] == want.tolist()
    # the rule of ``run``: the larger of 2e-6 of the largest magnitude and 4 times the float32 CPU error on these scores
    a, b = on["sequences_scores"].cpu().numpy(), cb["sequences_scores"].cpu().numpy()
    tol = max(2e-6 * float(np.abs(b).max()), 4 * err32)
    print(f"scores: max |device - callback| {float(np.abs(a - b).max()):.3g}, bound {tol:.3g} (float32 CPU error {err32:.3g})")
    np.testing.assert_allclose(a, b, rtol=0, atol=tol)


def test_generate_refusals_on_the_trie():
    from torch_rechub_amd.utils.data import DeviceTrie, Trie
    z, model, ids, mask = load_model("a")
    cands = z["beam.candidates"].tolist()
    trie = DeviceTrie(cands, dev())
    host_trie = Trie(cands)
    with pytest.raises(ValueError, match="give one"):
        model.generate(ids, mask, 10, 3, 3, host_trie.def_prefix_allowed_tokens_fn(host_trie), constraint=trie)
    with pytest.raises(ValueError, match="max_new_tokens"):
        model.generate(ids, mask, 3, 3, 3, constraint=trie)
    with pytest.raises(ValueError, match="eos_token_id"):
        model.generate(ids, mask, 10, 3, 3, constraint=DeviceTrie([c[:-1] + [2] for c in cands], dev()))
    with pytest.raises(ValueError, match="eos_token_id"):
        model.generate(ids, mask, 10, 3, 3, constraint=DeviceTrie([c[:-1] + [1 + i % 2] for i, c in enumerate(cands)], dev()))
    with pytest.raises(ValueError, match="fewer than num_beams=3"):
        model.generate(ids, mask, 10, 3, 3, constraint=DeviceTrie(cands[:2], dev()))
    with pytest.raises(ValueError, match="fewer than num_beams=3"):  # two first codes, then one continuation each
        model.generate(ids, mask, 10, 3, 3, constraint=DeviceTrie([cands[0], cands[2]], dev()))
    with pytest.raises(ValueError, match="vocab_size"):
        model.generate(ids, mask, 10, 3, 3, constraint=DeviceTrie([c[:2] + [40 + i] + c[3:] for i, c in enumerate(cands)], dev()))
    with pytest.raises(ValueError, match="decoder_start_token_id"):
        model.generate(ids, mask, 10, 3, 3, constraint=DeviceTrie([[3] + c[1:] for c in cands], dev()))
    with pytest.raises(ValueError, match="num_return_sequences"):
        model.generate(ids, mask, 10, 3, 4, constraint=trie)
    assert model.training  # every refusal left the mode as it was
