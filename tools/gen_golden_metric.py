"""Generate tests/golden/metric_cases.npz from the UNMODIFIED reference's torch_rechub/basic/metric.py (CPU).

Run where the reference checkout exists:  ``python tools/gen_golden_metric.py``

The archive holds inputs and what the reference returned for them:

  auc_*         labels, float32 predictions with many ties            -> auc_score
  gauc_*        the same over 25 users with scattered ids             -> gauc_score under sample counts and under weights
  gaucnan_*     five users, one of them with a single class           -> nan (the one single-class group of the fixture)
  logloss_*     float32 and float64 predictions                       -> log_loss of each
  self_*        the data of the reference's own ``__main__`` check    -> topk_metrics, coverage, diversity, novelty strings
  topk_*        40 users, K = 20, cut-offs (1, 5, 10, 20), truth lists of 0 to 8 ids with duplicates on both sides
  beyond_*      30 users, 12 recommendations over a catalogue of 50   -> diversity, coverage, novelty at (1, 5, 12)

A result string rounds to the fourth decimal.  The unrounded values (recomputed by tests/metric_oracle.py for the list
metrics, in float64 below for the rest) must keep 1e-7 from every rounding boundary -- asserted here, so that the tests can
demand every string exactly -- and no group is single-class outside ``gaucnan``.  The seed is stepped until both hold.  The
archive is written with a fixed member timestamp, so it regenerates byte-identically.
"""
import importlib
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import metric_oracle as O  # noqa: E402
from oracle.ref_import import import_reference  # noqa: E402
from tools.gen_golden_ffm import _save_fixed  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "metric_cases.npz")
MARGIN = 1e-7
LIST_NAMES = ("NDCG", "MRR", "Recall", "Hit", "Precision")


def strings(result, names):
    return {name: np.array(result[name]) for name in names}


def check_margin(values, what):
    for v in values:
        assert O.rounding_margin(float(v)) > MARGIN, f"{what}: {v!r} lies within {MARGIN} of a rounding boundary"


def pointwise(R, rng, out):
    n = 300
    label = (rng.random(n) < 0.4).astype(np.float32)
    pred = np.round(rng.random(n), 2).astype(np.float32)
    out.update(auc_label=label.copy(), auc_pred=pred, auc_out=np.float64(R.auc_score(label, pred)))
    ids = rng.choice(60, size=25, replace=False)
    users = ids[rng.integers(0, 25, size=n)]
    for u in ids:  # both classes for every user
        where = np.flatnonzero(users == u)
        assert len(where) >= 2
        label[where[0]], label[where[1]] = 0.0, 1.0
    weights = np.round(rng.random(61) + 0.5, 3)
    P, N, _ = O.rank_stat(pred, label, users)
    assert all(p > 0 and q > 0 for p, q in zip(P, N) if p + q > 0)
    out.update(gauc_label=label, gauc_pred=pred, gauc_users=users.astype(np.int64), gauc_weights=weights,
               gauc_out=np.float64(R.gauc_score(label, pred, users)),
               gauc_weighted_out=np.float64(R.gauc_score(label, pred, users, {int(u): weights[u] for u in ids})))
    label5 = np.array([0, 1, 1, 0, 1, 1, 0, 1, 0, 1], dtype=np.float32)
    users5 = np.array([3, 3, 7, 7, 9, 9, 11, 11, 20, 20], dtype=np.int64)  # user 9 holds positives only
    pred5 = np.round(rng.random(10), 2).astype(np.float32)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        nan = R.gauc_score(label5, pred5, users5)
    assert np.isnan(nan), f"the reference gave {nan!r} for a single-class user"
    out.update(gaucnan_label=label5, gaucnan_pred=pred5, gaucnan_users=users5, gaucnan_out=np.float64(nan))
    p32 = (0.01 + 0.98 * rng.random(200)).astype(np.float32)
    y32 = (rng.random(200) < 0.3).astype(np.float32)
    out.update(logloss_label=y32, logloss_pred=p32, logloss_out32=np.float64(R.log_loss(y32, p32)),
               logloss_out64=np.float64(R.log_loss(y32.astype(np.float64), p32.astype(np.float64))))


def pack(lists):
    off = np.zeros(len(lists) + 1, dtype=np.int64)
    off[1:] = np.cumsum([len(t) for t in lists])
    return off, np.array([i for t in lists for i in t], dtype=np.int64)


def lists(R, rng, out):
    # the reference's own self-check
    y_pred = {'0': [0, 1], '1': [0, 1], '2': [2, 3]}
    y_true = {'0': [1, 2], '1': [0, 1, 2], '2': [2, 3]}
    embs = {0: [1.0, 0.0, 0.0], 1: [0.9, 0.1, 0.0], 2: [0.0, 1.0, 0.0], 3: [0.0, 0.0, 1.0]}
    pop = {0: 0.5, 1: 0.3, 2: 0.05, 3: 0.01}
    res = R.topk_metrics(y_true, y_pred, topKs=(1, 2))
    assert res['NDCG'][1] == 'NDCG@2: 0.7956' and res['Hit'][1] == 'Hit@2: 0.7143'
    off, ids = pack(list(y_true.values()))
    out.update(self_pred=np.array(list(y_pred.values()), dtype=np.int64), self_off=off, self_ids=ids,
               self_cutoffs=np.array([1, 2]), self_embs=np.array([embs[i] for i in range(4)]),
               self_pop=np.array([pop[i] for i in range(4)]))
    out.update({f"self_{k}": v for k, v in strings(res, LIST_NAMES).items()})
    out["self_Coverage"] = np.array(R.coverage_score(y_pred, {0, 1, 2, 3, 4, 5}, topKs=[1, 2])["Coverage"])
    out["self_Diversity"] = np.array(R.diversity_score(y_pred, embs, topKs=[2])["Diversity"] +
                                     R.diversity_score(y_pred, embs, topKs=[1])["Diversity"])
    out["self_Novelty"] = np.array(R.novelty_score(y_pred, pop, topKs=[1, 2])["Novelty"])

    M, K, cut = 40, 20, (1, 5, 10, 20)
    pred = rng.integers(0, 30, size=(M, K))  # 30 ids for 20 places: duplicates inside a row
    truth = [rng.integers(0, 30, size=int(rng.integers(0, 9))).tolist() for _ in range(M)]
    truth[0], truth[1] = [], [int(pred[1, 0])] * 3  # an empty list; one id three times
    res = R.topk_metrics({u: truth[u] for u in range(M)}, {u: pred[u].tolist() for u in range(M)}, topKs=cut)
    mine = O.list_metrics(pred, truth, cut)
    check_margin(O.unrounded(mine, cut, M), "topk")
    assert O.list_strings(mine, cut, M) == {k: list(v) for k, v in res.items()}
    off, ids = pack(truth)
    out.update(topk_pred=pred.astype(np.int64), topk_off=off, topk_ids=ids, topk_cutoffs=np.array(cut))
    out.update({f"topk_{k}": v for k, v in strings(res, LIST_NAMES).items()})

    M, K, V, cut = 30, 12, 50, (1, 5, 12)
    rec = {u: rng.choice(V + 5, size=K, replace=False).tolist() for u in range(M)}  # ids >= V: no embedding, no popularity
    table = rng.standard_normal((V, 6))
    popularity = rng.random(V) * 0.2 + 1e-4
    out.update(beyond_pred=np.array([rec[u] for u in range(M)], dtype=np.int64), beyond_embs=table,
               beyond_pop=popularity, beyond_cutoffs=np.array(cut), beyond_catalogue=np.int64(V + 5))
    out["beyond_Diversity"] = np.array(R.diversity_score(rec, table, topKs=list(cut))["Diversity"])
    out["beyond_Coverage"] = np.array(R.coverage_score(rec, set(range(V + 5)), topKs=list(cut))["Coverage"])
    out["beyond_Novelty"] = np.array(R.novelty_score(rec, {i: popularity[i] for i in range(V)},
                                                     topKs=list(cut))["Novelty"])
    # unrounded, in float64, for the margin
    for k in cut:
        seen = set()
        for items in rec.values():
            seen.update(items[:k])
        check_margin([len(seen) / (V + 5)], "coverage")
        nov = [np.mean([-np.log2(max(popularity[i] if i < V else 1e-10, 1e-10)) for i in items[:k]])
               for items in rec.values()]
        check_margin([np.mean(nov)], "novelty")
        div = []
        for items in rec.values():
            v = np.stack([table[i] for i in items[:k] if i < V] or [np.zeros(6)])
            if len(v) < 2:
                continue
            unit = v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-10)
            div.append((1 - unit @ unit.T)[np.triu_indices(len(v), k=1)].sum() / (len(v) * (len(v) - 1) / 2))
        check_margin([np.mean(div)] if div else [], "diversity")


def main():
    import_reference()
    R = importlib.import_module("torch_rechub.basic.metric")
    for seed in range(2022, 2122):
        out = {}
        rng = np.random.default_rng(seed)
        try:
            pointwise(R, rng, out)
            lists(R, rng, out)
        except AssertionError as e:
            print(f"seed {seed}: {e}")
            continue
        out["seed"] = np.int64(seed)
        _save_fixed(OUT, out)
        print(f"metric_cases.npz (seed {seed}, {os.path.getsize(OUT)} bytes)")
        return
    raise SystemExit("no seed in range met the margins")


if __name__ == "__main__":
    main()
