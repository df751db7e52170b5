"""basic.metric on host inputs against tests/golden/metric_cases.npz (the unmodified reference's results, written by
tools/gen_golden_metric.py), tests/metric_oracle.py against the same fixture and against roc_auc_score, and the guards.
No GPU: the device forms are tests/test_gpu_metric.py's."""
import ctypes
import math
import warnings

import numpy as np
import pytest
import torch

import metric_oracle as O
from conftest import load_golden

LIST_NAMES = ("NDCG", "MRR", "Recall", "Hit", "Precision")


@pytest.fixture(scope="module")
def cases():
    return load_golden("metric_cases.npz")


@pytest.fixture(scope="module")
def metric():
    import torch_rechub_amd.basic.metric as metric
    return metric


def truth_lists(off, ids):
    return [ids[off[u]:off[u + 1]].tolist() for u in range(len(off) - 1)]


def as_dicts(pred, off, ids, key=int):
    truth = truth_lists(off, ids)
    return ({key(u): truth[u] for u in range(len(truth))}, {key(u): pred[u].tolist() for u in range(len(truth))})


def test_the_module_has_the_reference_surface(metric):
    for name in ("auc_score", "get_user_pred", "gauc_score", "topk_metrics", "ndcg_score", "hit_score", "mrr_score",
                 "recall_score", "precision_score", "log_loss", "diversity_score", "coverage_score", "novelty_score"):
        assert callable(getattr(metric, name)), name
    import torch_rechub_amd.basic
    assert torch_rechub_amd.basic.metric is metric


def test_pointwise_host_forms_equal_the_reference(cases, metric):
    c = cases
    assert metric.auc_score(c["auc_label"], c["auc_pred"]) == pytest.approx(float(c["auc_out"]), rel=0, abs=1e-12)
    users = c["gauc_users"]
    assert metric.gauc_score(c["gauc_label"], c["gauc_pred"], users) == pytest.approx(float(c["gauc_out"]), rel=0, abs=1e-12)
    weights = {int(u): c["gauc_weights"][u] for u in np.unique(users)}
    got = metric.gauc_score(c["gauc_label"], c["gauc_pred"], users, weights)
    assert got == pytest.approx(float(c["gauc_weighted_out"]), rel=0, abs=1e-12)
    y, p = c["logloss_label"], c["logloss_pred"]
    assert metric.log_loss(y, p) == pytest.approx(float(c["logloss_out32"]), rel=0, abs=1e-12)
    got = metric.log_loss(y.astype(np.float64), p.astype(np.float64))
    assert got == pytest.approx(float(c["logloss_out64"]), rel=0, abs=1e-12)


def test_a_single_class_user_makes_gauc_nan(cases, metric):
    c = cases
    assert math.isnan(float(c["gaucnan_out"]))
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        assert math.isnan(metric.gauc_score(c["gaucnan_label"], c["gaucnan_pred"], c["gaucnan_users"]))
    assert math.isnan(O.gauc(c["gaucnan_pred"], c["gaucnan_label"], c["gaucnan_users"]))


def test_get_user_pred_groups_in_order_of_first_appearance(metric):
    got = metric.get_user_pred([1, 0, 1, 0], [.1, .2, .3, .4], [7, 3, 7, 3])
    assert got == {7: {"y_true": [1, 1], "y_pred": [.1, .3]}, 3: {"y_true": [0, 0], "y_pred": [.2, .4]}}
    assert list(got) == [7, 3]


@pytest.mark.parametrize("case", ["self", "topk"])
def test_list_metric_strings_equal_the_reference(cases, metric, case):
    c = cases
    cut = tuple(int(k) for k in c[f"{case}_cutoffs"])
    y_true, y_pred = as_dicts(c[f"{case}_pred"], c[f"{case}_off"], c[f"{case}_ids"], key=str)
    res = metric.topk_metrics(y_true, y_pred, topKs=cut)
    assert sorted(res) == sorted(LIST_NAMES)
    for name in LIST_NAMES:
        assert res[name] == c[f"{case}_{name}"].tolist(), name
    wrappers = {"NDCG": metric.ndcg_score, "MRR": metric.mrr_score, "Recall": metric.recall_score, "Hit": metric.hit_score,
                "Precision": metric.precision_score}
    for name, fn in wrappers.items():
        assert fn(y_true, y_pred, topKs=list(cut)) == c[f"{case}_{name}"].tolist()
    assert res["missing"] == []  # a defaultdict of lists, like the reference's


def test_the_self_check_strings_are_the_hand_calculated_ones(cases):
    c = cases
    assert c["self_NDCG"][1] == "NDCG@2: 0.7956" and c["self_MRR"][1] == "MRR@2: 0.8333"
    assert c["self_Recall"][1] == "Recall@2: 0.7222" and c["self_Hit"][1] == "Hit@2: 0.7143"
    assert c["self_Precision"][1] == "Precision@2: 0.8333"
    assert c["self_Coverage"].tolist() == ["Coverage@1: 0.3333", "Coverage@2: 0.6667"]
    assert c["self_Diversity"].tolist() == ["Diversity@2: 0.3374", "Diversity@1: 0.0"]
    assert c["self_Novelty"].tolist() == ["Novelty@1: 2.1073", "Novelty@2: 2.74"]


def test_default_cutoff_is_five_and_bad_cutoffs_raise(metric):
    y_true, y_pred = {"a": [1, 2]}, {"a": [2, 9, 8, 7, 1, 3]}
    assert metric.topk_metrics(y_true, y_pred)["Hit"] == ["Hit@5: 1.0"]
    assert metric.recall_score(y_true, y_pred) == ["Recall@5: 1.0"]
    with pytest.raises(ValueError, match="topKs wrong"):
        metric.topk_metrics(y_true, y_pred, topKs=5)
    with pytest.raises(AssertionError):
        metric.topk_metrics(y_true, {"a": [1], "b": [2]}, topKs=[1])
    with pytest.raises(ZeroDivisionError):
        metric.topk_metrics({"a": []}, {"a": [1]}, topKs=[1])
    with pytest.raises(IndexError):
        metric.topk_metrics(y_true, {"a": [1]}, topKs=[2])


def test_beyond_accuracy_host_forms_equal_the_reference(cases, metric):
    c = cases
    y_pred = {"0": [0, 1], "1": [0, 1], "2": [2, 3]}
    embs = {i: c["self_embs"][i].tolist() for i in range(4)}
    pop = {i: float(c["self_pop"][i]) for i in range(4)}
    assert metric.coverage_score(y_pred, {0, 1, 2, 3, 4, 5}, topKs=[1, 2])["Coverage"] == c["self_Coverage"].tolist()
    got = metric.diversity_score(y_pred, embs, topKs=[2])["Diversity"] + metric.diversity_score(y_pred, embs, [1])["Diversity"]
    assert got == c["self_Diversity"].tolist()
    assert metric.novelty_score(y_pred, pop, topKs=[1, 2])["Novelty"] == c["self_Novelty"].tolist()

    cut = [int(k) for k in c["beyond_cutoffs"]]
    rec = {u: row.tolist() for u, row in enumerate(c["beyond_pred"])}
    V = len(c["beyond_pop"])
    assert metric.diversity_score(rec, c["beyond_embs"], topKs=cut)["Diversity"] == c["beyond_Diversity"].tolist()
    catalogue = set(range(int(c["beyond_catalogue"])))
    assert metric.coverage_score(rec, catalogue, topKs=cut)["Coverage"] == c["beyond_Coverage"].tolist()
    popularity = {i: c["beyond_pop"][i] for i in range(V)}
    assert metric.novelty_score(rec, popularity, topKs=cut)["Novelty"] == c["beyond_Novelty"].tolist()
    # tensors are copied to the host: rows become users 0 .. M - 1
    ids, table = torch.from_numpy(c["beyond_pred"]), torch.from_numpy(c["beyond_embs"])
    assert metric.diversity_score(ids, table, topKs=cut)["Diversity"] == c["beyond_Diversity"].tolist()
    assert metric.coverage_score(ids, catalogue, topKs=cut)["Coverage"] == c["beyond_Coverage"].tolist()
    assert metric.novelty_score(ids, popularity, topKs=cut)["Novelty"] == c["beyond_Novelty"].tolist()
    assert metric.diversity_score({}, embs)["Diversity"] == ["Diversity@5: 0.0"]
    assert metric.novelty_score({"a": []}, pop)["Novelty"] == ["Novelty@5: 0.0"]


def test_the_exact_auc_agrees_with_roc_auc_score(cases):
    """U2 / (2 P N) is the exact rational; roc_auc_score integrates the ROC curve in float64: only summation order differs."""
    from sklearn.metrics import roc_auc_score
    c = cases
    for label, pred in ((c["auc_label"], c["auc_pred"]), (c["gauc_label"], c["gauc_pred"])):
        assert O.auc(pred, label) == pytest.approx(roc_auc_score(label, pred), rel=0, abs=1e-12)
    rng = np.random.default_rng(5)
    pred = np.concatenate([rng.standard_normal(500).astype(np.float32), np.zeros(40, np.float32), -np.zeros(40, np.float32)])
    label = rng.random(580) < 0.5
    assert O.auc(pred, label) == pytest.approx(roc_auc_score(label, pred), rel=0, abs=1e-12)


def test_the_oracle_equals_the_fixture(cases):
    c = cases
    assert O.auc(c["auc_pred"], c["auc_label"]) == pytest.approx(float(c["auc_out"]), rel=0, abs=1e-12)
    users = c["gauc_users"]
    assert O.gauc(c["gauc_pred"], c["gauc_label"], users) == pytest.approx(float(c["gauc_out"]), rel=0, abs=1e-12)
    got = O.gauc(c["gauc_pred"], c["gauc_label"], users, c["gauc_weights"])
    assert got == pytest.approx(float(c["gauc_weighted_out"]), rel=0, abs=1e-12)
    assert O.log_loss(c["logloss_pred"], c["logloss_label"]) == pytest.approx(float(c["logloss_out64"]), rel=0, abs=1e-12)
    for case in ("self", "topk"):
        cut = [int(k) for k in c[f"{case}_cutoffs"]]
        pred = c[f"{case}_pred"]
        res = O.list_metrics(pred, truth_lists(c[f"{case}_off"], c[f"{case}_ids"]), cut)
        strings = O.list_strings(res, cut, len(pred))
        for name in LIST_NAMES:
            assert strings[name] == c[f"{case}_{name}"].tolist(), (case, name)
        assert min(O.rounding_margin(v) for v in O.unrounded(res, cut, len(pred))) > 1e-7


def test_rank_stat_counts_ties_once_and_keeps_denormals_apart():
    P, N, U2 = O.rank_stat([0.5, 0.5, 0.5, 0.5], [1, 0, 1, 0])
    assert (P, N, U2) == ([2], [2], [4])  # every pair tied: U2 = P N
    P, N, U2 = O.rank_stat(np.array([-0.0, 0.0], np.float32), [1, 0])
    assert U2 == [1]
    tiny = np.array([0.0, 1e-45, 3e-45, 4e-45], np.float32)  # zero and three distinct denormals
    assert len(set(tiny.tolist())) == 4
    assert O.rank_stat(tiny, [0, 1, 0, 1])[2] == [2 * 1 + 2 * 2]
    P, N, U2 = O.rank_stat([.1, .9, .2, .8], [0, 1, 1, 0], [0, 0, 2, 2])
    assert (P, N, U2) == ([1, 0, 1], [1, 0, 1], [2, 0, 0])


def test_the_device_ops_refuse_host_tensors_and_the_header_declares_them():
    from torch_rechub_amd import _lib, ops
    p, y = torch.rand(8), (torch.rand(8) < 0.5).float()
    for call in (lambda: ops.auc_groups(p, y), lambda: ops.auc(p, y), lambda: ops.log_loss(p, y),
                 lambda: ops.gauc(p, y, torch.arange(8)),
                 lambda: ops.rank_metrics(torch.zeros((2, 3), dtype=torch.int64), [[1], [2]], [1])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    i, l, v = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert _lib.SIGNATURES["rh_auc_plan"] == [l, v, v, v]
    assert _lib.SIGNATURES["rh_auc_keys"] == [v, l, v, l, v, v]
    assert _lib.SIGNATURES["rh_auc_groups"] == [v, l, v, i, v, v, l, l, v, v, v, v]
    assert _lib.SIGNATURES["rh_gauc_reduce"] == [v, v, l, v, v, v, v]
    assert _lib.SIGNATURES["rh_log_loss"] == [v, l, v, i, l, v, v, v]
    assert _lib.SIGNATURES["rh_rank_metrics_plan"] == [i, v, v, v, v]
    assert _lib.SIGNATURES["rh_rank_metrics"] == [v, l, i, i, v, v, l, v, i, v, v, v, v, v, v, v, v]
    for name in ("rh_auc_plan", "rh_rank_metrics_plan", "rh_auc_groups", "rh_rank_metrics"):
        assert name not in _lib._VALUE_RETURNING


def test_the_plans_and_argument_errors_need_no_device():
    from torch_rechub_amd import _lib, ops
    chunk, max_grid, nbytes = ops.auc_plan(3 * 1024 + 5)
    assert chunk >= 64 and chunk % 64 == 0 and max_grid >= 1 and nbytes >= 4 * 52
    assert ops.auc_plan(0)[2] >= 0
    stage, users, grid, partial = ops.rank_metrics_plan(10)
    assert stage >= 1 and users >= 1 and grid >= 1 and partial >= 32
    with pytest.raises(RuntimeError, match="outside"):
        ops.auc_plan(2 ** 31)
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(4096)  # never dereferenced: validation fails first
    with pytest.raises(RuntimeError, match="K=257 unsupported"):
        _lib.call("rh_rank_metrics", fake, 257, 1, 257, fake, fake, 0, fake, 1, fake, fake, fake, fake, fake, fake, null, null)
    with pytest.raises(RuntimeError, match="9 cut-offs"):
        _lib.call("rh_rank_metrics", fake, 4, 1, 4, fake, fake, 0, fake, 9, fake, fake, fake, fake, fake, fake, null, null)
    cuts = (ctypes.c_int * 2)(1, 5)
    with pytest.raises(RuntimeError, match="cut-off 5 outside"):
        _lib.call("rh_rank_metrics", fake, 4, 1, 4, fake, fake, 0, ctypes.c_void_p(ctypes.addressof(cuts)), 2, fake, fake,
                  fake, fake, fake, fake, null, null)
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib.call("rh_auc_groups", fake, 1, null, 0, null, fake, 4, 1, fake, fake, fake, null)
    with pytest.raises(RuntimeError, match="label_dtype=7"):
        _lib.call("rh_log_loss", fake, 1, fake, 7, 4, fake, fake, null)


def test_gain_tables_and_truth_packing():
    from torch_rechub_amd import ops
    gain, ideal = ops.rank_gain_tables(7)
    assert gain.tolist() == [1. / np.log2(j + 2) for j in range(7)] and ideal[0] == 0.0
    run = 0.0
    for j in range(7):
        run += gain[j]
        assert ideal[j + 1] == run
    off, ids = ops.pack_truth([[3, 3], [], [9]], "cpu")
    assert off.tolist() == [0, 2, 2, 3] and ids.tolist() == [3, 3, 9] and off.dtype == ids.dtype == torch.int64
