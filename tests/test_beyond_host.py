"""tests/beyond_oracle.py against the reference's recorded results (the ``beyond_*`` entries of
tests/golden/metric_cases.npz), the rounding margins that make string equality a fair demand in tests/test_gpu_beyond.py,
and the parts of rh_ild / rh_coverage / rh_novelty that need no device: the header entries, the plans, the refusals."""
import ctypes

import numpy as np
import pytest
import torch

import beyond_cases as C
import beyond_oracle as O
from conftest import load_golden


@pytest.fixture(scope="module")
def cases():
    return load_golden("metric_cases.npz")


def test_the_oracle_reproduces_the_reference_strings(cases):
    c = cases
    f = C.fixture_case(c)
    cut = f["cutoffs"]
    assert (f["pred"] >= 0).all()  # the fixture has no padding: the oracle is the reference itself here
    for table in (c["beyond_embs"], f["table"]):  # as recorded (float64), and rounded to float32 for the device
        got = O.strings("Diversity", O.means(O.diversity(f["pred"], table, cut)), cut)
        assert got == c["beyond_Diversity"].tolist()
    assert O.coverage_strings(O.coverage(f["pred"], cut), f["catalogue"], cut) == c["beyond_Coverage"].tolist()
    assert O.strings("Novelty", O.means(O.novelty(f["pred"], f["pop"], cut)), cut) == c["beyond_Novelty"].tolist()


def test_the_oracle_equals_the_host_functions_on_padded_rows():
    """With the negative entries removed from the rows, the package's host loops (the reference's) give the oracle's
    strings: the padding rule is the only thing the oracle adds."""
    import torch_rechub_amd.basic.metric as metric
    f = C.string_case("small")
    cut = f["cutoffs"]
    rec = {u: [int(i) for i in row if i >= 0] for u, row in enumerate(f["pred"])}
    want = O.strings("Diversity", O.means(O.diversity(f["pred"], f["table"], cut)), cut)
    assert metric.diversity_score(rec, f["table"], topKs=cut)["Diversity"] == want
    popularity = {i: float(p) for i, p in enumerate(f["pop"])}
    want = O.strings("Novelty", O.means(O.novelty(f["pred"], f["pop"], cut)), cut)
    assert metric.novelty_score(rec, popularity, topKs=cut)["Novelty"] == want
    want = O.coverage_strings(O.coverage(f["pred"], cut), f["catalogue"], cut)
    assert metric.coverage_score(rec, range(f["catalogue"]), topKs=cut)["Coverage"] == want


def test_the_oracle_on_hand_made_lists():
    table = np.array([[1, 0], [0, 1], [-1, 0], [0, 0]], np.float32)
    pred = np.array([[0, 1, 2, -1], [0, 9, -1, -1], [3, 0, 0, 5], [-1, -1, -1, -1]])
    got = O.diversity(pred, table, [1, 2, 4])
    assert np.isnan(got[:, 0]).all() and np.isnan(got[1]).all() and np.isnan(got[3]).all()
    assert got[0, 1] == 1.0 and got[0, 2] == pytest.approx((1 + 2 + 1) / 3, abs=1e-15)
    assert got[2, 1] == 1.0 and got[2, 2] == pytest.approx(2 / 3, abs=1e-15)  # the zero row is at 1 from both copies
    assert O.coverage(pred, [1, 2, 4]) == [2, 4, 6]
    nov = O.novelty(pred, np.array([0.5, 0.25, 1.0, 0.0]), [1, 4])
    assert nov[0].tolist() == [1.0, 1.0] and np.isnan(nov[3]).all()
    assert nov[1, 1] == pytest.approx((1 - np.log2(1e-10)) / 2, abs=1e-13)
    assert O.means(nov)[0] == pytest.approx((1 + 1 - np.log2(1e-10)) / 3, abs=1e-13)
    assert O.means(got)[0] == 0.0 and O.strings("Diversity", [0.0], [1]) == ["Diversity@1: 0.0"]


def test_every_compared_string_is_far_from_a_rounding_boundary(cases):
    todo = [C.fixture_case(cases)] + [C.string_case(name) for name in C.STRING_CASES]
    for f in todo:
        cut = f["cutoffs"]
        values = O.means(O.diversity(f["pred"], f["table"], cut)) + O.means(O.novelty(f["pred"], f["pop"], cut))
        values += [c / f["catalogue"] for c in O.coverage(f["pred"], cut)]
        assert min(O.rounding_margin(v) for v in values) >= 1e-8


def test_the_header_declares_the_new_entries():
    from torch_rechub_amd import _lib
    i, l, v = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    assert _lib.SIGNATURES["rh_ild_plan"] == [i, v, v, v]
    assert _lib.SIGNATURES["rh_ild"] == [v, l, i, i, v, l, l, i, v, i, v, v, v, v, v]
    assert _lib.SIGNATURES["rh_coverage_plan"] == [l, v, v, v]
    assert _lib.SIGNATURES["rh_coverage"] == [v, l, i, i, l, v, i, v, v, v]
    assert _lib.SIGNATURES["rh_novelty_plan"] == [i, v, v, v]
    assert _lib.SIGNATURES["rh_novelty"] == [v, l, i, i, v, i, l, v, i, v, v, v, v, v]
    for name in ("rh_ild_plan", "rh_ild", "rh_coverage_plan", "rh_coverage", "rh_novelty_plan", "rh_novelty"):
        assert name not in _lib._VALUE_RETURNING


def test_the_ops_refuse_host_tensors():
    from torch_rechub_amd import ops
    ids = torch.zeros((2, 3), dtype=torch.int64)
    for call in (lambda: ops.ild(ids, torch.zeros(4, 2), [2]), lambda: ops.coverage(ids, 4, [2]),
                 lambda: ops.novelty(ids, torch.ones(4), [2])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_the_plans_and_argument_errors_need_no_device():
    from torch_rechub_amd import _lib, ops
    for plan in (ops.ild_plan, ops.novelty_plan):
        users, grid, partial = plan(10)
        assert users >= 1 and grid >= 1 and partial >= 8 * 3  # three workgroups of four users at the least
        assert plan(users * grid + 1)[2] == plan(users * grid)[2]  # the grid is capped: further trips
    rows, grid, nbytes = ops.coverage_plan(7)
    assert rows >= 1 and grid >= 1 and nbytes == 28
    with pytest.raises(RuntimeError, match="outside"):
        ops.coverage_plan(2 ** 31)
    null, fake = ctypes.c_void_p(0), ctypes.c_void_p(4096)  # never dereferenced: validation fails first
    cuts = (ctypes.c_int * 2)(1, 5)
    cp = ctypes.c_void_p(ctypes.addressof(cuts))
    with pytest.raises(RuntimeError, match="K=257 unsupported"):
        _lib.call("rh_ild", fake, 257, 1, 257, fake, 4, 9, 4, cp, 1, fake, fake, fake, null, null)
    with pytest.raises(RuntimeError, match="D=1025 unsupported"):
        _lib.call("rh_ild", fake, 4, 1, 4, fake, 1025, 9, 1025, cp, 1, fake, fake, fake, null, null)
    with pytest.raises(RuntimeError, match="9 cut-offs"):
        _lib.call("rh_ild", fake, 4, 1, 4, fake, 4, 9, 4, cp, 9, fake, fake, fake, null, null)
    with pytest.raises(RuntimeError, match="cut-off 5 outside"):
        _lib.call("rh_novelty", fake, 4, 1, 4, fake, 0, 9, cp, 2, fake, fake, fake, null, null)
    with pytest.raises(RuntimeError, match="pop_dtype=2"):
        _lib.call("rh_novelty", fake, 4, 1, 4, fake, 2, 9, cp, 1, fake, fake, fake, null, null)
    with pytest.raises(RuntimeError, match="n_slots=0"):
        _lib.call("rh_coverage", fake, 4, 1, 4, 0, cp, 1, fake, fake, null)
    with pytest.raises(RuntimeError, match="K=257 unsupported"):
        _lib.call("rh_coverage", fake, 257, 1, 257, 8, cp, 1, fake, fake, null)
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib.call("rh_ild", fake, 4, 1, 4, null, 4, 9, 4, cp, 1, fake, fake, fake, null, null)
    with pytest.raises(RuntimeError, match="table_stride=3"):
        _lib.call("rh_ild", fake, 4, 1, 4, fake, 3, 9, 4, cp, 1, fake, fake, fake, null, null)
