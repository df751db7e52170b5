"""torch_rechub_amd.serving.HipIndexer, utils.match.ExactIndex and the two evaluation protocols (DSSM's item index, HSTU's
masked top-K) on the MI355X, against float64 brute force (tests/topk_oracle.py)."""
import numpy as np
import pytest
import torch

import topk_oracle as O
from conftest import golden_batch, golden_state, load_golden, build_amd_model, features_from_spec

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def builder(metric):
    from torch_rechub_amd.serving import builder_factory
    return builder_factory("hip", metric=metric)


def test_ip_is_topk_items():
    from torch_rechub_amd import ops
    q, x, _ = O.normal_data(1, 5, 20, 300)
    with builder("IP").from_embeddings(torch.from_numpy(x)) as index:
        ids, val = index.query(torch.from_numpy(q).to(dev()), 7)
    wi, ws = ops.topk_items(torch.from_numpy(q).to(dev()), torch.from_numpy(x).to(dev()), 7)
    assert ids.is_cuda and torch.equal(ids, wi) and torch.equal(val, ws)


def test_l2_on_integer_data_is_exact():
    """ids and squared distances equal the float64 ones; ascending, ties to the lower id; a query that is a table row finds
    that row first at distance exactly 0."""
    M, D, V, K = 5, 7, 4097, 200
    q, x, _ = O.int_data(2, M, D, V)
    q[0] = x[1234]
    x[77] = x[1234]  # a duplicate row with a lower id comes first
    d64 = ((q.astype(np.float64)[:, None, :] - x.astype(np.float64)[None, :, :]) ** 2).sum(-1)
    wi, wneg = O.rank(-d64, O.valid_mask(M, V), K)
    with builder("L2").from_embeddings(torch.from_numpy(x).to(dev())) as index:
        assert len(index) == V
        ids, val = index.query(torch.from_numpy(q).to(dev()), K)
    ids, val = ids.cpu().numpy(), val.cpu().numpy()
    np.testing.assert_array_equal(ids, wi)
    np.testing.assert_array_equal(val.astype(np.float64), -wneg)
    assert ids[0, 0] == 77 and ids[0, 1] == 1234 and val[0, 0] == 0.0 and val[0, 1] == 0.0
    assert (np.diff(val, axis=1) >= 0).all()


def test_l2_tail_when_the_index_is_smaller_than_top_k():
    q, x, _ = O.int_data(3, 2, 7, 5)
    with builder("L2").from_embeddings(torch.from_numpy(x)) as index:
        ids, val = index.query(torch.from_numpy(q).to(dev()), 8)
    assert (ids[:, 5:] == -1).all() and torch.isposinf(val[:, 5:]).all() and (ids[:, :5] >= 0).all()


def test_angular_against_float64():
    """cos under the float criterion of test_gpu_topk.py on the normalised vectors, and the distance compared after the
    same transformation: v^2 against max(0, 2 - 2 cos64).  fp32 forms t = 2 - 2 cos with one rounding (|t| <= 4: at most
    4 * 2^-24) and its root with another (relative 2^-24, so 2 * 2^-24 * t <= 8 * 2^-24 on the square); cos itself carries
    eps_i / 2.  A zero query has cos 0 with everything: distance sqrt(2), no NaN."""
    from torch_rechub_amd import ops
    from torch_rechub_amd.serving.hip import _unit_rows
    M, D, V, K = 6, 64, 4097, 50
    q, x, _ = O.normal_data(4, M, D, V)
    q[2] = 0.0
    x[10] = 0.0
    qn = q.astype(np.float64) / np.maximum(np.linalg.norm(q.astype(np.float64), axis=1, keepdims=True), 1e-300)
    xn = x.astype(np.float64) / np.maximum(np.linalg.norm(x.astype(np.float64), axis=1, keepdims=True), 1e-300)
    cos64 = qn @ xn.T
    eps = 2.0 * (D + 2) * O.U * (np.abs(qn) @ np.abs(xn).T).max(axis=1)
    with builder("angular").from_embeddings(torch.from_numpy(x)) as index:
        ids, val = index.query(torch.from_numpy(q).to(dev()), K)
        # the kernel's own cos on the vectors the index normalised: same ids, in the strict order (ties to the lower id)
        # (each fp32 unit vector carries up to 3 * 2^-24 relative error -- norm, root, division -- so D + 8 for D + 2)
        own_ids, own_cos = ops.topk_items(_unit_rows(torch.from_numpy(q).to(dev())), index._search, K)
    assert torch.equal(ids, own_ids)
    O.check_float(own_ids.cpu().numpy(), own_cos.cpu().numpy(), cos64, O.valid_mask(M, V), eps * (D + 8) / (D + 2), K,
                  "angular cos")
    ids, val = ids.cpu().numpy(), val.cpu().numpy().astype(np.float64)
    assert np.isfinite(val).all()
    np.testing.assert_allclose(val[2], np.sqrt(2.0), rtol=0, atol=1e-6)
    np.testing.assert_array_equal(ids[2], np.arange(K))  # all tied: ascending ids
    cos_got = 1.0 - val ** 2 / 2.0
    live = [i for i in range(M) if i != 2]
    O.check_float(ids[live], cos_got[live], cos64[live], O.valid_mask(len(live), V), eps[live] + 12 * O.U, K, "angular",
                  tie_order=False)
    for i in live:
        want = np.maximum(0.0, 2.0 - 2.0 * cos64[i, ids[i]])
        assert np.abs(val[i] ** 2 - want).max() <= eps[i] + 12 * O.U
    assert (np.diff(val, axis=1) >= 0).all()


@pytest.mark.parametrize("metric", ["L2", "IP", "angular"])
def test_save_and_load_round_trip(tmp_path, metric):
    q, x, _ = O.normal_data(5, 4, 16, 500)
    qd = torch.from_numpy(q).to(dev())
    path = tmp_path / "items.index"
    with builder(metric).from_embeddings(torch.from_numpy(x)) as index:
        a = index.query(qd, 20)
        index.save(path)
    with builder("IP" if metric != "IP" else "L2").from_index_file(path) as index:  # the file carries its metric
        assert index.metric == metric
        b = index.query(qd, 20)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_cpu_queries_get_cpu_answers_and_exclusions_are_forwarded():
    q, x, _ = O.int_data(6, 3, 7, 300)
    with builder("IP").from_embeddings(torch.from_numpy(x)) as index:
        ids, val = index.query(torch.from_numpy(q), 5)
        assert not ids.is_cuda and not val.is_cuda and ids.dtype == torch.int64 and val.dtype == torch.float32
        ex = torch.cat([ids[:, :2], torch.full((3, 1), -1)], dim=1)
        ids2, _ = index.query(torch.from_numpy(q), 5, exclude=ex)
    want = O.rank(O.scores64(q, x), O.valid_mask(3, 300, ex.numpy()), 5)[0]
    np.testing.assert_array_equal(ids2.numpy(), want)
    np.testing.assert_array_equal(ids.numpy(), O.rank(O.scores64(q, x), O.valid_mask(3, 300), 5)[0])


def test_exact_index_has_annoys_surface():
    from torch_rechub_amd.utils.match import ExactIndex
    q, x, _ = O.normal_data(7, 3, 16, 200)
    index = ExactIndex(n_trees=10)
    index.fit(x)  # numpy, as the examples pass it
    ids, dist = index.query(v=q[0], n=10)
    assert isinstance(ids, list) and isinstance(dist, list) and len(ids) == len(dist) == 10
    assert all(isinstance(i, int) for i in ids) and dist == sorted(dist)
    bi, bd = index.query(torch.from_numpy(q), 10)
    assert bi.shape == bd.shape == (3, 10) and bi[0].tolist() == ids and bd[0].tolist() == dist
    small = ExactIndex(metric="IP").fit(torch.from_numpy(x[:4]))
    ids, dist = small.query(q[1], 10)  # fewer rows than n: as many as there are
    assert len(ids) == len(dist) == 4 and sorted(ids) == [0, 1, 2, 3]


def test_dssm_item_index_ranks_as_float64():
    """The DSSM fixture's towers on the device: every user's top-K items from the index equal the float64 ranking of
    user @ item.T on the same vectors, under the float criterion."""
    gold = load_golden("model_dssm.npz")
    model = build_amd_model("dssm", features_from_spec(gold["spec"]))
    model.load_state_dict(golden_state(gold, "sd0."))
    model = model.to(dev()).eval()
    x, _ = golden_batch(gold, 0)
    xd = {k: v.to(dev()) for k, v in x.items()}
    with torch.no_grad():
        u, it = model.user_tower(xd), model.item_tower(xd)
    K = min(10, int(it.shape[0]))
    with builder("IP").from_embeddings(it) as index:
        ids, val = index.query(u, K)
    un, itn = u.cpu().numpy(), it.cpu().numpy()
    O.check_float(ids.cpu().numpy(), val.cpu().numpy(), O.scores64(un, itn), O.valid_mask(len(un), len(itn)),
                  O.eps_rows(un, itn), K, "dssm")


def test_hstu_evaluation_protocol_matches_the_masked_topk_of_the_logits():
    """examples/generative/run_hstu_movielens.py's ranking: last position's logits, PAD and the history masked, torch.topk.
    Here: hidden_and_head + ops.topk_items(..., exclude=seq_tokens, invalid=[0]).  The model is re-seeded until every
    float64 gap between neighbours among each row's best K + 1 valid scores exceeds eps_i, so that both sides must agree."""
    from torch_rechub_amd import ops
    from torch_rechub_amd.models.generative import HSTUModel
    V, B, L, K = 300, 6, 20, 10
    found = None
    for seed in range(8):
        torch.manual_seed(seed)
        model = HSTUModel(V, d_model=24, n_heads=2, n_layers=2, dqk=12, dv=10, max_seq_len=24, dropout=0.0,
                          num_time_buckets=16, use_output_bias=True)
        with torch.no_grad():
            for n, p in model.named_parameters():
                if "bias" in n:
                    p.add_(0.05 * torch.randn_like(p))
        model = model.to(dev()).eval()
        tokens = torch.randint(1, V, (B, L))
        tokens[0, :7] = 0  # left padding
        tokens[3, :19] = 0
        tokens = tokens.to(dev())
        with torch.no_grad():
            h, W, bias = model.hidden_and_head(tokens)
            logits = model(tokens)[:, -1]
        hl = h[:, -1]
        hn, Wn, bn = hl.cpu().numpy(), W.detach().cpu().numpy(), bias.detach().cpu().numpy()
        s64 = O.scores64(hn, Wn, bn)
        ok = O.valid_mask(B, V, tokens.cpu().numpy(), [0])
        eps = O.eps_rows(hn, Wn, bn)
        gaps = -np.diff(O.rank(s64, ok, K + 1)[1], axis=1)
        if (gaps.min(axis=1) > eps).all():
            found = seed
            break
    assert found is not None, "no seed with float64 gaps above eps among the best K + 1"
    ids, sc = ops.topk_items(hl, W, K, bias=bias, exclude=tokens, invalid=[0])
    masked = logits.clone()
    masked[:, 0] = float("-inf")
    masked.scatter_(1, tokens, float("-inf"))
    want = torch.topk(masked, K, dim=1).indices
    assert torch.equal(ids, want)
    np.testing.assert_array_equal(ids.cpu().numpy(), O.rank(s64, ok, K)[0])
    O.check_float(ids.cpu().numpy(), sc.cpu().numpy(), s64, ok, eps, K, "hstu")
