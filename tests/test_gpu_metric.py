"""csrc/metric.hip through ops and basic.metric, against tests/metric_oracle.py: the rank statistic (P, N, U2) exactly, gauc
and log_loss at rtol 1e-12, the list metrics bit for bit per user.  Shapes are the smallest at which each kernel can still
go wrong: around one chunk / stage / workgroup, and one trip past each grid cap.

Why 1e-12 for the double sums: every term is exact or within an ulp of double, only the order of summation differs (a fixed
tree here, one by one in the oracle), and log2(n) 2^-53 lies three orders of magnitude below it."""
import math

import numpy as np
import pytest
import torch

import metric_oracle as O
from conftest import load_golden
from torch_rechub_amd._lib import H

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LIST_NAMES = ("NDCG", "MRR", "Recall", "Hit", "Precision")


@pytest.fixture(scope="module")
def ops():
    from torch_rechub_amd import ops
    return ops


@pytest.fixture(scope="module")
def metric():
    import torch_rechub_amd.basic.metric as metric
    return metric


@pytest.fixture(scope="module")
def cases():
    return load_golden("metric_cases.npz")


@pytest.fixture(scope="module")
def plan(ops):
    chunk, max_grid, _ = ops.auc_plan(1)
    return chunk, max_grid


def dev(a):
    return torch.as_tensor(a).to(DEV)


def stat(ops, pred, label, group=None):
    out = ops.auc_groups(dev(pred), dev(label), None if group is None else dev(group))
    return tuple(t.tolist() for t in out)


def check_stat(ops, pred, label, group=None):
    got = stat(ops, pred, label, group)
    want = O.rank_stat(pred, label, group)
    assert got == want
    return got


def tied_scores(rng, n, levels):
    return (rng.integers(0, levels, n) / levels).astype(np.float32)


# ---- rank statistic ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("which", ["1", "2", "c-1", "c", "c+1", "3c+5"])
def test_rank_statistic_around_the_chunk_size(ops, plan, which, grouped):
    c = plan[0]
    n = {"1": 1, "2": 2, "c-1": c - 1, "c": c, "c+1": c + 1, "3c+5": 3 * c + 5}[which]
    rng = np.random.default_rng(n + grouped)
    pred, label = tied_scores(rng, n, 97), (rng.random(n) < 0.4).astype(np.float32)
    group = rng.integers(0, 7, n).astype(np.int64) if grouped else None
    check_stat(ops, pred, label, group)


def test_one_tie_run_over_four_chunks(ops, plan):
    n = 3 * plan[0] + 5
    label = (np.random.default_rng(1).random(n) < 0.3).astype(np.float32)
    P, N, U2 = check_stat(ops, np.full(n, 0.25, np.float32), label)
    assert U2[0] == P[0] * N[0] and P[0] + N[0] == n


def test_tie_and_group_borders_exactly_on_chunk_borders(ops, plan):
    c = plan[0]
    rng = np.random.default_rng(2)
    # sorted: c distinct values, then a run that fills chunk 1 exactly, then a run of c + 5
    pred = np.concatenate([np.arange(c) / (2 * c), np.full(c, 0.6), np.full(c + 5, 0.7)]).astype(np.float32)
    label = (rng.random(3 * c + 5) < 0.5).astype(np.float32)
    perm = rng.permutation(len(pred))
    check_stat(ops, pred[perm], label[perm])
    # groups of c, c and c + 5 samples: the group borders are the chunk borders
    group = np.concatenate([np.zeros(c), np.ones(c), np.full(c + 5, 2)]).astype(np.int64)
    pred = tied_scores(rng, 3 * c + 5, 13)
    check_stat(ops, pred[perm], label[perm], group[perm])


def test_one_group_over_three_chunks_among_many_small_ones(ops, plan):
    c = plan[0]
    rng = np.random.default_rng(3)
    sizes = rng.integers(1, 4, 6 * c + 1).tolist()
    big = len(sizes) // 2 + 1
    sizes.insert(big, 3 * c)  # somewhere behind many small groups: it starts inside a chunk
    group = np.repeat(np.arange(len(sizes)), sizes).astype(np.int64)
    n = len(group)
    assert len(sizes) > n // 3
    perm = rng.permutation(n)
    pred, label = tied_scores(rng, n, 5), (rng.random(n) < 0.5).astype(np.float32)
    P, N, U2 = check_stat(ops, pred, label, group[perm])
    assert P[big] + N[big] == 3 * c


def test_second_trip_past_the_grid_cap(ops, plan):
    c, max_grid = plan
    n = max_grid * c + 7
    rng = np.random.default_rng(4)
    pred, label = tied_scores(rng, n, 4001), (rng.random(n) < 0.2).astype(np.uint8)
    check_stat(ops, pred, label)
    group = rng.integers(0, 1000, n).astype(np.int64)
    group[:1000] = np.arange(1000)
    check_stat(ops, pred, label, group)


def test_signed_zeros_tie_and_denormals_do_not(ops):
    assert stat(ops, np.array([-0.0, 0.0], np.float32), np.array([1, 0], np.float32)) == ([1], [1], [1])
    assert stat(ops, np.array([0.0, -0.0], np.float32), np.array([1, 0], np.float32)) == ([1], [1], [1])
    rng = np.random.default_rng(5)
    pred = np.where(rng.random(300) < 0.5, -0.0, 0.0).astype(np.float32)
    pred[::7] = 1e-3
    pred[3::11] = -1e-3
    check_stat(ops, pred, (rng.random(300) < 0.5).astype(np.float32))
    tiny = np.array([0.0, 1e-45, 3e-45, 4e-45], np.float32)
    assert len(set(tiny.tolist())) == 4
    assert stat(ops, tiny, np.array([0, 1, 0, 1], np.float32)) == ([2], [2], [6])
    assert stat(ops, tiny[::-1].copy(), np.array([1, 0, 1, 0], np.float32)) == ([2], [2], [6])
    tiny = np.concatenate([tiny, -tiny]).astype(np.float32)
    check_stat(ops, np.tile(tiny, 40), (rng.random(320) < 0.5).astype(np.float32))


@pytest.mark.parametrize("dtype", [np.float32, np.float64, np.int64, np.uint8, np.bool_])
def test_every_label_dtype(ops, dtype):
    rng = np.random.default_rng(6)
    pred, label = tied_scores(rng, 777, 31), (rng.random(777) < 0.5).astype(dtype)
    check_stat(ops, pred, label, rng.integers(0, 5, 777).astype(np.int64))


def test_counted_errors_raise(ops):
    rng = np.random.default_rng(7)
    pred, label = rng.random(2000).astype(np.float32), (rng.random(2000) < 0.5).astype(np.float32)
    for bad in (float("nan"), float("inf"), float("-inf")):
        p = pred.copy()
        p[1234] = bad
        with pytest.raises(ValueError, match="1 predictions are NaN or infinite"):
            ops.auc_groups(dev(p), dev(label))
    for dtype, value in ((np.float32, 2), (np.float32, 0.5), (np.int64, 2), (np.int64, -1), (np.uint8, 2)):
        y = label.astype(dtype)
        y[[5, 1999]] = value
        with pytest.raises(ValueError, match="2 labels are neither 0 nor 1"):
            ops.auc(dev(pred), dev(y))
    assert ops.auc(dev(pred), dev(label)) == O.auc(pred, label)  # nothing lingers


def test_single_class_input(ops):
    pred = np.random.default_rng(8).random(1500).astype(np.float32)
    assert stat(ops, pred, np.ones(1500, np.float32)) == ([1500], [0], [0])
    assert stat(ops, pred, np.zeros(1500, np.float32)) == ([0], [1500], [0])
    with pytest.raises(ValueError, match="Only one class"):
        ops.auc(dev(pred), dev(np.ones(1500, np.float32)))


def test_strided_predictions_and_two_runs(ops, plan):
    c = plan[0]
    n = 2 * c + 9
    rng = np.random.default_rng(9)
    wide = dev(tied_scores(rng, 3 * n, 50))
    label, group = (rng.random(n) < 0.5).astype(np.float32), rng.integers(0, n // 2, n).astype(np.int64)
    group[0] = n // 2 - 1
    view = wide[::3]
    assert not view.is_contiguous()
    first = ops.auc_groups(view, dev(label), dev(group))
    second = ops.auc_groups(view, dev(label), dev(group))
    want = O.rank_stat(view.cpu().numpy(), label, group)
    for a, b, w in zip(first, second, want):
        assert torch.equal(a, b) and a.tolist() == w
    column = dev(tied_scores(rng, n, 50)).reshape(n, 1)
    assert tuple(t.tolist() for t in ops.auc_groups(column, dev(label))) == O.rank_stat(column.cpu().numpy()[:, 0], label)


def test_auc_is_the_correctly_rounded_rational(ops, metric, cases):
    from sklearn.metrics import roc_auc_score
    rng = np.random.default_rng(10)
    pred, label = tied_scores(rng, 5000, 211), (rng.random(5000) < 0.3).astype(np.float32)
    got = ops.auc(dev(pred), dev(label))
    P, N, U2 = O.rank_stat(pred, label)
    assert got == U2[0] / (2 * P[0] * N[0])
    assert got == pytest.approx(roc_auc_score(label, pred), rel=0, abs=1e-12)
    got = metric.auc_score(dev(cases["auc_label"]), dev(cases["auc_pred"]))
    assert isinstance(got, float) and got == pytest.approx(float(cases["auc_out"]), rel=0, abs=1e-12)


def test_pointwise_guards_come_before_any_launch(ops):
    p, y = torch.rand(8, device=DEV), torch.ones(8, device=DEV)
    with pytest.raises(ValueError, match="float32 predictions"):
        ops.auc_groups(p.double(), y)
    with pytest.raises(ValueError, match="float32 predictions"):
        ops.log_loss(p.double(), y)
    with pytest.raises(ValueError, match="labels"):
        ops.auc_groups(p, y.to(torch.int32))
    with pytest.raises(ValueError, match="do not agree"):
        ops.auc_groups(p, y[:7])
    with pytest.raises(ValueError, match="do not agree"):
        ops.gauc(p, y, torch.zeros(9, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="empty"):
        ops.auc_groups(p[:0], y[:0])
    with pytest.raises(ValueError, match="empty"):
        ops.log_loss(p[:0], y[:0])
    with pytest.raises(ValueError, match="int64 group ids"):
        ops.auc_groups(p, y, torch.zeros(8, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="dense group ids"):
        ops.auc_groups(p, y, torch.full((8,), -1, dtype=torch.int64, device=DEV))
    with pytest.raises(ValueError, match="int64 user ids"):
        ops.gauc(p, y, torch.zeros(8, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.auc_groups(p.cpu(), y)


# ---- gauc and log_loss ---------------------------------------------------------------------------------------------
def two_class_users(rng, n_users, id_space):
    """Shuffled samples of n_users users with scattered ids, every user holding both classes."""
    ids = rng.choice(id_space, size=n_users, replace=False)
    counts = rng.integers(2, 20, n_users)
    users = np.repeat(ids, counts)
    label = (rng.random(len(users)) < 0.4).astype(np.float32)
    starts = np.cumsum(counts) - counts
    label[starts], label[starts + 1] = 0.0, 1.0
    perm = rng.permutation(len(users))
    return users[perm].astype(np.int64), label[perm]


def test_gauc_against_the_oracle(ops, metric, cases):
    rng = np.random.default_rng(11)
    users, label = two_class_users(rng, 700, 5000)
    pred = tied_scores(rng, len(users), 53)
    got = ops.gauc(dev(pred), dev(label), dev(users))
    assert got == pytest.approx(O.gauc(pred, label, users), rel=1e-12, abs=0)
    assert got == ops.gauc(dev(pred), dev(label), dev(users))  # two runs: the same bits
    weights = np.round(rng.random(5000) + 0.25, 3)
    for w in (dev(weights), dev(weights.astype(np.float32))):
        got = ops.gauc(dev(pred), dev(label), dev(users), w)
        assert got == pytest.approx(O.gauc(pred, label, users, w.cpu().numpy()), rel=1e-12, abs=0)
        assert got == metric.gauc_score(dev(label), dev(pred), dev(users), w)
    c = cases
    got = metric.gauc_score(dev(c["gauc_label"]), dev(c["gauc_pred"]), dev(c["gauc_users"]))
    assert got == pytest.approx(float(c["gauc_out"]), rel=1e-12, abs=0)
    got = metric.gauc_score(dev(c["gauc_label"]), dev(c["gauc_pred"]), dev(c["gauc_users"]), dev(c["gauc_weights"]))
    assert got == pytest.approx(float(c["gauc_weighted_out"]), rel=1e-12, abs=0)
    with pytest.raises(ValueError, match="outside the weight tensor"):
        ops.gauc(dev(pred), dev(label), dev(users), dev(weights[:10]))


def test_gauc_with_a_single_class_user_is_nan(ops, metric, cases):
    c = cases
    assert math.isnan(metric.gauc_score(dev(c["gaucnan_label"]), dev(c["gaucnan_pred"]), dev(c["gaucnan_users"])))
    rng = np.random.default_rng(12)
    users, label = two_class_users(rng, 300, 1000)
    label[users == users[0]] = 1.0
    assert math.isnan(ops.gauc(dev(tied_scores(rng, len(users), 9)), dev(label), dev(users)))
    assert math.isnan(ops.gauc(dev(np.float32([.5])), dev(np.float32([1])), dev(np.int64([42]))))


def test_gauc_past_the_reduction_grid(ops):
    """More users than one trip of the reduction takes (1024 workgroups of 256): pairs of one negative and one positive,
    so every user's AUC is 0, 1/2 or 1 and the weighted mean is exact in double."""
    G = 1024 * 256 + 77
    rng = np.random.default_rng(13)
    neg, pos = rng.integers(0, 4, G), rng.integers(0, 4, G)
    pred = np.stack([neg, pos], 1).reshape(-1).astype(np.float32)
    label = np.tile(np.float32([0, 1]), G)
    users = np.repeat(rng.permutation(G).astype(np.int64) * 3, 2)
    want = float(((pos > neg) + 0.5 * (pos == neg)).sum() * 2.0) / (2.0 * G)
    assert ops.gauc(dev(pred), dev(label), dev(users)) == want


@pytest.mark.parametrize("n", [1, 255, 257, 1024 * 256 + 3])
def test_log_loss_against_the_oracle(ops, n):
    rng = np.random.default_rng(n)
    pred = (0.001 + 0.998 * rng.random(n)).astype(np.float32)
    label = (rng.random(n) < 0.3)
    want = O.log_loss(pred, label)
    for dtype in (np.float32, np.float64, np.int64, np.uint8, np.bool_):
        got = ops.log_loss(dev(pred), dev(label.astype(dtype)))
        assert got == pytest.approx(want, rel=1e-12, abs=0)
    assert ops.log_loss(dev(pred), dev(label)) == ops.log_loss(dev(pred), dev(label))
    wide = dev(np.repeat(pred, 2))
    assert ops.log_loss(wide[::2], dev(label)) == ops.log_loss(dev(pred), dev(label))


def test_log_loss_soft_labels_fixture_and_non_finite_terms(ops, metric, cases):
    rng = np.random.default_rng(14)
    pred, soft = (0.01 + 0.98 * rng.random(999)).astype(np.float32), rng.random(999)
    assert ops.log_loss(dev(pred), dev(soft)) == pytest.approx(O.log_loss(pred, soft), rel=1e-12, abs=0)
    c = cases
    got = metric.log_loss(dev(c["logloss_label"]), dev(c["logloss_pred"]))
    assert isinstance(got, float) and got == pytest.approx(float(c["logloss_out64"]), rel=1e-12, abs=0)
    pred[17] = 0.0
    hard = np.zeros(999, np.float32)
    assert math.isnan(ops.log_loss(dev(pred), dev(hard))) and math.isnan(O.log_loss(pred, hard))  # 0 * log 0
    pred[17] = 1.0
    assert ops.log_loss(dev(pred), dev(hard)) == math.inf == O.log_loss(pred, hard)


# ---- list metrics --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rank_plan(ops):
    return ops.rank_metrics_plan(1)[:3]  # stage, users per workgroup, grid cap


def check_lists(ops, pred, truth, cutoffs, device_pred=None, pair=False):
    ids = dev(pred) if device_pred is None else device_pred
    t = ops.pack_truth(truth, DEV) if pair else truth
    got = ops.rank_metrics(ids, t, cutoffs, per_user=True)
    want = O.list_metrics(pred, truth, cutoffs)
    per_user = got["per_user"].cpu().numpy()
    assert per_user.shape == want["per_user"].shape
    assert np.array_equal(per_user.view(np.int64), want["per_user"].view(np.int64))  # bit for bit
    assert got["hits"].tolist() == want["hits"] and int(got["gts"]) == want["gts"]
    np.testing.assert_allclose(got["sums"].cpu().numpy(), want["sums"], rtol=1e-12, atol=0)
    again = ops.rank_metrics(ids, t, cutoffs)
    assert again["per_user"] is None and torch.equal(again["sums"], got["sums"]) and torch.equal(again["hits"], got["hits"])
    return got


def truth_of_lengths(rng, lengths, K):
    return [rng.integers(0, max(3 * K, 2 * n), n).tolist() for n in lengths]


@pytest.mark.parametrize("K", [1, 2, 63, 64, 65, 128, 255, H.RH_RANK_MAX_K])
def test_list_metrics_over_the_width_range(ops, rank_plan, K):
    s = rank_plan[0]
    rng = np.random.default_rng(K)
    lengths = [0, 1, s - 1, s, s + 1, 2 * s + 3, 3, 7, 2]
    truth = truth_of_lengths(rng, lengths, K)
    pred = rng.integers(0, 2 * K, (len(lengths), K))   # duplicates inside a row
    truth[7] = [int(pred[7, 0])] * 3 + truth[7]        # and inside a truth list
    truth[8] = [int(pred[8, 0]), 5 * K]
    pred[8, (K + 1) // 2:] = -1                        # a padding tail never matches
    check_lists(ops, pred, truth, [K])
    eight = [1, K] + rng.integers(1, K + 1, 6).tolist()
    check_lists(ops, pred, truth, eight, pair=True)
    wide = dev(np.concatenate([pred, rng.integers(0, 2 * K, (len(lengths), 7))], 1))
    view = wide[:, :K]
    assert view.stride(0) == K + 7
    check_lists(ops, pred, truth, [1, K], device_pred=view)


@pytest.mark.parametrize("which", ["1", "upw-1", "upw+1", "past the cap", "34 partials"])
def test_list_metrics_over_the_user_range(ops, rank_plan, which):
    """The "34 partials" case: 133 users are 34 workgroups, the last with one user -- more partials than the final sum has parts
    (32) and no multiple of them, at one cut-off and at eight; the other cases end in 1, 2 or 1024 partials."""
    _, upw, cap = rank_plan
    M = {"1": 1, "upw-1": upw - 1, "upw+1": upw + 1, "past the cap": cap * upw + 3, "34 partials": 133}[which]
    rng = np.random.default_rng(M)
    K, cuts = (65, ([65], [1, 2, 3, 5, 8, 13, 21, 65])) if which == "34 partials" else (8, ([3, 8],))
    truth = truth_of_lengths(rng, rng.integers(0, 6, M).tolist(), K)
    truth[-1] = [3]
    pred = rng.integers(0, 3 * K, (M, K))
    for cut in cuts:
        check_lists(ops, pred, truth, cut)


def test_all_truth_lists_empty(ops, metric):
    pred = np.arange(12).reshape(3, 4)
    got = check_lists(ops, pred, [[], [], []], [2, 4])
    assert int(got["gts"]) == 0 and not got["sums"].any() and not got["per_user"].any()
    with pytest.raises(ZeroDivisionError):
        metric.topk_metrics([[], [], []], dev(pred), topKs=[2])


@pytest.mark.parametrize("case", ["self", "topk"])
def test_device_topk_metrics_give_the_fixture_strings(metric, cases, case):
    c = cases
    cut = [int(k) for k in c[f"{case}_cutoffs"]]
    pred, off, ids = c[f"{case}_pred"], c[f"{case}_off"], c[f"{case}_ids"]
    truth = [ids[off[u]:off[u + 1]].tolist() for u in range(len(pred))]
    for y_true in ((dev(off), dev(ids)), truth):
        res = metric.topk_metrics(y_true, dev(pred), topKs=cut)
        for name in LIST_NAMES:
            assert res[name] == c[f"{case}_{name}"].tolist(), name
        assert sorted(res) == sorted(LIST_NAMES) and res["missing"] == []
    assert metric.ndcg_score(truth, dev(pred), topKs=tuple(cut)) == c[f"{case}_NDCG"].tolist()
    assert metric.hit_score(truth, dev(pred), topKs=cut) == c[f"{case}_Hit"].tolist()
    assert metric.mrr_score(truth, dev(pred), topKs=cut) == c[f"{case}_MRR"].tolist()
    assert metric.recall_score(truth, dev(pred), topKs=cut) == c[f"{case}_Recall"].tolist()
    assert metric.precision_score(truth, dev(pred), topKs=cut) == c[f"{case}_Precision"].tolist()


def test_list_metric_guards_come_before_any_launch(ops, metric):
    pred = torch.zeros((3, 6), dtype=torch.int64, device=DEV)
    truth = [[1], [2], [3]]
    for cut in ([0], [7], [1] * 9, []):
        with pytest.raises(ValueError, match="cut-offs"):
            ops.rank_metrics(pred, truth, cut)
    with pytest.raises(ValueError, match="int64 id tensor"):
        ops.rank_metrics(pred.int(), truth, [1])
    with pytest.raises(ValueError, match="2 truth lists for 3 users"):
        ops.rank_metrics(pred, truth[:2], [1])
    with pytest.raises(ValueError, match="3 truth offsets"):
        ops.rank_metrics(pred, (torch.zeros(3, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int64, device=DEV)), [1])
    with pytest.raises(ValueError, match="empty"):
        ops.rank_metrics(pred[:0], [], [1])
    with pytest.raises(RuntimeError, match="no HIP kernel"):
        ops.rank_metrics(torch.zeros((1, 257), dtype=torch.int64, device=DEV), [[1]], [1])
    with pytest.raises(ValueError, match="topKs wrong"):
        metric.topk_metrics(truth, pred, topKs=5)


def test_topk_items_feeds_topk_metrics_on_the_device(ops, metric):
    g = torch.Generator().manual_seed(15)
    q, table = torch.randn((70, 16), generator=g), torch.randn((900, 16), generator=g)
    ids, _ = ops.topk_items(q.to(DEV), table.to(DEV), 50)
    rng = np.random.default_rng(15)
    truth = [rng.integers(0, 900, int(rng.integers(0, 40))).tolist() for _ in range(70)]
    host_ids = ids.cpu().tolist()
    for k_view, cut in ((ids, [1, 10, 50]), (ids[:, :20], [5, 20])):
        on_device = metric.topk_metrics(truth, k_view, topKs=cut)
        on_host = metric.topk_metrics({u: truth[u] for u in range(70)}, {u: host_ids[u] for u in range(70)}, topKs=cut)
        assert dict(on_device) == dict(on_host)


# ---- trainers ------------------------------------------------------------------------------------------------------
def golden_loader(gold):
    from conftest import golden_batch
    return [golden_batch(gold, b) for b in range(3)]


def test_ctr_trainer_evaluates_on_the_device():
    from conftest import build_amd_model, features_from_spec, golden_state
    from torch_rechub_amd.trainers import CTRTrainer
    gold = load_golden("model_deepfm_tutorial.npz")
    model = build_amd_model("deepfm_tutorial", features_from_spec(gold["spec"]))
    model.load_state_dict(golden_state(gold, "sd0."))
    trainer = CTRTrainer(model.to(DEV), device=DEV, show_progress=False)
    loader = golden_loader(gold)
    on_host = trainer.evaluate(trainer.model, loader)
    on_device = trainer.evaluate(trainer.model, loader, on_device=True)
    assert isinstance(on_device, float) and on_device == pytest.approx(on_host, rel=0, abs=1e-12)
    trainer.evaluate_fn = lambda y, p: 0.0
    with pytest.raises(ValueError, match="on_device=True"):
        trainer.evaluate(trainer.model, loader, on_device=True)
    assert trainer.evaluate(trainer.model, loader) == 0.0


def test_mtl_trainer_evaluates_on_the_device():
    import json

    from conftest import build_mtl_model, features_from_spec, golden_state
    from torch_rechub_amd.trainers import MTLTrainer
    gold = load_golden("model_mmoe.npz")
    types = json.loads(str(gold["task_types"]))
    model = build_mtl_model("mmoe", features_from_spec(gold["spec"]), types)
    trainer = MTLTrainer(model, task_types=types, n_epoch=1, device=DEV, show_progress=False)
    model.load_state_dict(golden_state(gold, "sd0."))
    loader = golden_loader(gold)
    on_host = trainer.evaluate(trainer.model, loader)
    on_device = trainer.evaluate(trainer.model, loader, on_device=True)
    assert len(on_device) == len(on_host) == 2
    for a, b in zip(on_device, on_host):
        assert isinstance(a, float) and a == pytest.approx(b, rel=0, abs=1e-12)
    trainer.evaluate_fns[1] = lambda y, p: 0.0
    with pytest.raises(ValueError, match="on_device=True"):
        trainer.evaluate(trainer.model, loader, on_device=True)


def test_mtl_regression_task_is_scored_with_the_mean_squared_error():
    """sklearn squares and averages the float32 arrays in float32, the device form widens to float64 first: the two agree to
    float32 rounding of 144 squares and their mean, a few 2^-24 relative -- 1e-5 leaves an order of magnitude."""
    import json

    from conftest import build_mtl_model, features_from_spec, golden_state
    from torch_rechub_amd.trainers import MTLTrainer
    gold = load_golden("model_shared_bottom.npz")
    types = json.loads(str(gold["task_types"]))
    assert types == ["classification", "regression"]
    model = build_mtl_model("shared_bottom", features_from_spec(gold["spec"]), types)
    trainer = MTLTrainer(model, task_types=types, n_epoch=1, device=DEV, show_progress=False)
    model.load_state_dict(golden_state(gold, "sd0."))
    loader = golden_loader(gold)
    on_host = trainer.evaluate(trainer.model, loader)
    on_device = trainer.evaluate(trainer.model, loader, on_device=True)
    assert on_device[0] == pytest.approx(on_host[0], rel=0, abs=1e-12)
    assert isinstance(on_device[1], float) and on_device[1] == pytest.approx(float(on_host[1]), rel=1e-5, abs=0)


def test_match_trainer_evaluates_on_the_device():
    from conftest import build_amd_model, features_from_spec, golden_state
    from torch_rechub_amd.trainers import MatchTrainer
    gold = load_golden("model_dssm.npz")
    model = build_amd_model("dssm", features_from_spec(gold["spec"]))
    model.load_state_dict(golden_state(gold, "sd0."))
    trainer = MatchTrainer(model.to(DEV), mode=0, device=DEV, show_progress=False)
    loader = golden_loader(gold)
    on_host = trainer.evaluate(trainer.model, loader)
    assert trainer.evaluate(trainer.model, loader, on_device=True) == pytest.approx(on_host, rel=0, abs=1e-12)
