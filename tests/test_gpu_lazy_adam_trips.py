"""Blocked-lazy exact Adam (csrc/optim.hip) at every row width and past the caps of its sweep grids, against float64.

What runs: the touched-rows pass, the pre-gather refresh, the window sweep in its narrow, merged and two-float4-per-lane
("wide") forms and the flush, at embed_dim 4 .. 128 (1 .. 32 lanes per row), each sweep on a grid capped so low
(RH_TUNE_SWEEP_GRID, RH_TUNE_DEFERRED_GRID) that a workgroup's ping-pong loop walks a second and a third work unit, crosses a
table boundary inside a trip and ends on a ragged last trip.  Every case first asks the library for the plan of the launches it
is about -- rh_adam_lazy_sweep_plan is the function launch_sweep / launch_sweep_wide take their grid from -- and asserts,
before it steps anything: the grid is at its cap, work units > 2 x grid (the third unit of workgroup 0 is live), work units no
multiple of the grid (ragged tail), and which kernel is taken.

Three optimizers on identical inputs, no trainer and no hipGraph: a lazy TableAdam (lazy_k = 4, explicit lazy_small_rows), a
dense TableAdam twin (rh_adam_dense) and the float64 oracle oracle.ctr_oracle.adam_step stepping every row every step
(reference: torch.optim.Adam, trainers/ctr_trainer.py:59-61,99).  Per step and record: 97 lookups per field (two 64-sample
chunks, the second ragged), float32 gradient rows, the dense gradient formed ONCE on the CPU by index_add_ and copied into both
twins' gradient buffers (the oracle gets the same float32 values as float64).  Deferred form: ops._pre_gather first (refresh
kernel, then the previous step's sweep forked to the side stream); in-line form: no refresh, so the touched pass replays its
rows itself.  2 K + 3 = 11 steps (every window swept at least twice), then flush(); one variant flushes every 3 steps.

Tables, in units of R = 1024 / D rows (one narrow work unit; a wide unit is 2 R rows), lazy_small_rows = 5 R + 3:
  t_dense 5 R + 3    dense                    6 units, the last with 3 rows
  t_a     24 R + 18  lazy, window 6 R + 5     7 narrow / 4 wide; the last window ends 2 rows short of its width
  t_tiny  7          dense                    1 unit; a zero-width entry between two lazy tables in RH_SWEEP_LAZY_TABLES
  t_b     16 R       lazy, window 4 R         4 narrow / 2 wide, no tail
  t_c     6 R + 4    lazy, window 1.5 R + 1   2 narrow / 1 wide
RH_SWEEP_LAZY_TABLES 13 narrow or 7 wide units, RH_SWEEP_DENSE_TABLES 7, RH_SWEEP_WINDOW 20, RH_SWEEP_FLUSH 55 .. 57.
Six fields: one per table and a second one on t_a whose first half repeats the first field's rows (two fields race for one
claim word, the gradient row holds their sum); the field of t_b carries padding_idx = 0 with a non-zero padding row and about a
seventh of its lookups are that index.  Index columns are columns of one (B, 6) matrix (stride 6).

Asserted in every case: after the flush the lazy and dense twins are bit-equal in parameter, exp_avg and exp_avg_sq, table by
table; every gradient buffer is zero; every last-step word and the step counter equal the step count; the error word is clean;
before the last flush no lazy row lags K steps or more (K + 1 in the deferred form, whose last sweep is still to be forked);
both twins meet the float64 oracle within the bounds test_gpu_kernels.py::test_adam_dense_vs_oracle uses (rtol 1e-5, atol
1e-6 / 1e-7 / 1e-9 x max(1, max|want|) for parameter / exp_avg / exp_avg_sq).  Not widened: stock float32 torch.optim.Adam on
the CPU stays under 0.45 of each bound against the same oracle through 21 steps on inputs of this kind.  Each case prints its
worst error / bound (``LAZYTRIPS`` lines).

Worst error / bound on the MI355X, every case measured (always exp_avg; the lazy and dense twins are bit-equal, so one figure):
  deferred           D = 4 .. 128: 0.152, 0.325, 0.335, 0.465, 0.358, 0.563
  in line            D = 4 .. 128: 0.162, 0.264, 0.343, 0.296, 0.359, 0.590;  int32 D = 8: 0.264, D = 64: 0.359
  flush every 3      D = 64 deferred 0.358;  D = 16 in line 0.343
  interleaved        D = 16: x 4, cap 30, period 3: 0.349;  x 10, cap 84, period 7: 0.209;  D = 64: 0.414, 0.476
  two groups         in line 0.333, deferred 0.366;   two records: in line 0.415, deferred 0.461
Found by this module: no defect -- every kernel passed as it was.  That the cases bite was tried on scratch builds with one line
of csrc/optim.hip changed each, value-only and in bounds, this module and the suite's earlier lazy-Adam tests run against each:
  lazy_sweep_wide_body without its ``fetch(vb + 2 * nblk, ua)``: the deferred cases at D = 8 .. 128 fail (every case whose sweep is
      the wide kernel, 8 of them) and the D = 128 step-ahead case; earlier tests: only the Criteo-size ones (D = 16) fail
  the touched pass's claim broadcast ``__shfl(old, lane - q)`` right only up to 8 lanes per row (``lane - (q & 7)``): every case
      at D = 64 and 128 fails (10 here, the two new step-ahead cases); every earlier test passes
  ``u.with_g = true`` dropped from the merged sweep's claim: the in-line cases at D = 32, 64, 128 and the four interleaved cases
      fail (at D = 4 .. 16 under period 1 the touched-rows workgroups come first and win every claim); earlier tests: four fail
  ``kPerWave`` fixed at 4 in the refresh's rotation: nothing fails, here or elsewhere, and nothing can -- the ranks of a pass are
      a permutation of 0 .. LPP - 1 and adding any constant modulo LPP keeps them one; which lane group replays a row changes no
      bit of it.  The rotation decides only which SIMD gets the longest replay.
"""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ctr_oracle as O
from test_gpu_kernels import dev

pytestmark = pytest.mark.gpu
F64 = np.float64
K = 4
STEPS = 2 * K + 3
NB = 97       # lookups per field: two 64-sample chunks, the second ragged
NF = 6        # fields per record
TOUCH_BLOCKS = 2 * NF  # touched-rows workgroups of a merged launch: 64-sample chunks x fields
LR, WD = 1e-2, 1e-3
WINDOW, FLUSH, LAZY_TABLES, DENSE_TABLES = 0, 1, 2, 3  # RH_SWEEP_* (asserted against the header below)
FIELD_TABLE = [0, 1, 2, 3, 4, 1]   # field -> table of its set: t_dense, t_a, t_tiny, t_b, t_c, t_a again
FIELD_PAD = [None, None, None, 0, None, None]
TOL = {"param": 1e-6, "exp_avg": 1e-7, "exp_avg_sq": 1e-9}  # atol_scale; rtol 1e-5 (test_adam_dense_vs_oracle)


def table_rows(D, mult=1):
    R = 1024 // D
    return [mult * n for n in (5 * R + 3, 24 * R + 18, 7, 16 * R, 6 * R + 4)]


def ceil_div(a, b):
    return -(-a // b)


# ---- the library's own plan -------------------------------------------------------------------------------------------------
@pytest.fixture
def caps():
    """set(sweep, deferred): RH_TUNE_SWEEP_GRID / RH_TUNE_DEFERRED_GRID; both back at their defaults afterwards."""
    from torch_rechub_amd import _lib
    H = _lib.H
    assert (H.RH_SWEEP_WINDOW, H.RH_SWEEP_FLUSH, H.RH_SWEEP_LAZY_TABLES, H.RH_SWEEP_DENSE_TABLES) == (0, 1, 2, 3)
    assert (H.RH_TUNE_SWEEP_GRID, H.RH_TUNE_DEFERRED_GRID) == (2, 8)

    def set_caps(sweep=None, deferred=None):
        if sweep is not None:
            _lib.call("rh_set_tuning", H.RH_TUNE_SWEEP_GRID, int(sweep))
        if deferred is not None:
            _lib.call("rh_set_tuning", H.RH_TUNE_DEFERRED_GRID, int(deferred))

    try:
        yield set_caps
    finally:
        _lib.call("rh_set_tuning", H.RH_TUNE_SWEEP_GRID, 0)
        _lib.call("rh_set_tuning", H.RH_TUNE_DEFERRED_GRID, 512)


def plan(grp, mode, t_value=-1, touch_blocks=0):
    """(work units, sweep workgroups, touch_period, wide) of one launch over a table group of the lazy optimizer, under the
    caps set at this moment -- from the host arrays the optimizer itself hands to the launch."""
    from torch_rechub_amd import _lib
    return _lib.query("rh_adam_lazy_sweep_plan", len(grp["members"]), ctypes.cast(grp["h_rows"], ctypes.c_void_p),
                      ctypes.cast(grp["h_win"], ctypes.c_void_p), grp["D"], mode, t_value, touch_blocks,
                      out=(ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int))


def assert_past_cap(pl, cap, what):
    """The fixed condition of every launch here: at its cap, a third unit for workgroup 0, a ragged last trip."""
    units, grid = pl[0], pl[1]
    assert grid == cap, f"{what}: grid {grid} is not the cap {cap}"
    assert units > 2 * grid, f"{what}: {units} work units give workgroup 0 of {grid} no third one"
    assert units % grid != 0, f"{what}: {units} work units are a multiple of the grid {grid}: no ragged tail"


def ragged_cap(unit_counts, candidates):
    """The first candidate cap under which every one of the launches is past it with a ragged tail."""
    for cap in candidates:
        if all(u > 2 * cap and u % cap != 0 for u in unit_counts):
            return cap
    raise AssertionError(f"no cap in {list(candidates)} leaves {unit_counts} past it and ragged")


def group_of(D, mult, small_rows):
    """The host arrays of one set's table group as TableAdam._lazy_setup builds them, without building the tables."""
    rows = table_rows(D, mult)
    win = [ceil_div(r, 1 if r <= small_rows else K) for r in rows]
    return dict(D=D, members=list(range(len(rows))), h_rows=(ctypes.c_int64 * len(rows))(*rows),
                h_win=(ctypes.c_int64 * len(rows))(*win))


# ---- the driver -------------------------------------------------------------------------------------------------------------
class Run(object):
    """sets: [(D, size multiplier, [(lookups per field, index dtype), ...] records)]; one lazy optimizer, one dense twin and the
    oracle's arrays over the tables of all sets, set by set in the order listed above."""

    def __init__(self, sets, overlap, small_rows, seed):
        from torch_rechub_amd import ops
        from torch_rechub_amd.optim import TableAdam
        self.ops = ops
        self.g = torch.Generator().manual_seed(seed)
        self.sets = []
        init = []
        for D, mult, records in sets:
            rows = table_rows(D, mult)
            first = len(init)
            for n in rows:
                init.append(torch.randn(n, D, generator=self.g) * 0.1)  # (the padding row of t_b is NOT zero)
            recs = []
            for B, dtype in records:
                buf = torch.zeros(B, NF, dtype=dtype, device=dev())  # static index buffer: its columns have stride NF
                recs.append(dict(B=B, dtype=dtype, buf=buf, cols=[buf[:, f] for f in range(NF)], i64=int(dtype == torch.int64)))
            self.sets.append(dict(D=D, rows=rows, first=first, recs=recs))
        self.A = [torch.nn.Parameter(t.clone().to(dev())) for t in init]   # dense twin
        self.L = [torch.nn.Parameter(t.clone().to(dev())) for t in init]   # lazy
        self.dense = TableAdam(self.A, table_params=self.A, lr=LR, weight_decay=WD)
        self.lazy = TableAdam(self.L, table_params=self.L, lr=LR, weight_decay=WD, lazy_k=K, lazy_small_rows=small_rows)
        self.lazy.overlap_sweep = bool(overlap)
        self.ref = [t.numpy().astype(F64) for t in init]
        self.ms = [np.zeros_like(r) for r in self.ref]
        self.vs = [np.zeros_like(r) for r in self.ref]
        for s in self.sets:
            for rec in s["recs"]:
                rec["weights"] = [self.L[s["first"] + FIELD_TABLE[f]] for f in range(NF)]
                esz = 8 if rec["i64"] else 4
                key = tuple([rec["buf"].data_ptr() + esz * f for f in range(NF)] + [NF] * NF + list(range(NF)))
                rec["idesc"] = ops.EmbedCall._icache.get(key, dev())
        self.t = 0

    def groups(self):
        """The lazy optimizer's table groups (one per embed_dim), in the order of the sets."""
        grps = self.lazy._lazy_setup()
        assert [g["D"] for g in grps] == [s["D"] for s in self.sets]
        return grps

    def kinds(self):
        return [self.lazy.table_k(p) for p in self.L]

    def step(self):
        ops = self.ops
        self.t += 1
        grads = [torch.zeros(r.shape, dtype=torch.float32) for r in self.ref]
        for s in self.sets:
            D, rows = s["D"], s["rows"]
            for rec in s["recs"]:
                B = rec["B"]
                idx = torch.stack([torch.randint(0, rows[FIELD_TABLE[f]], (B,), generator=self.g) for f in range(NF)], 1)
                idx[: B // 2, 5] = idx[: B // 2, 1]  # the two fields of t_a race for the same claim words
                idx[torch.rand(B, generator=self.g) < 1 / 7, 3] = 0  # padding lookups of t_b's field
                rows_g = torch.randn(B, NF, D, generator=self.g)
                for f in range(NF):
                    live = idx[:, f] != FIELD_PAD[f] if FIELD_PAD[f] is not None else torch.ones(B, dtype=torch.bool)
                    grads[s["first"] + FIELD_TABLE[f]].index_add_(0, idx[live, f], rows_g[live, f])
                rec["buf"].copy_(idx.to(rec["dtype"]))
        if self.lazy.overlap_sweep:  # what a gather's forward does: refresh the rows (and fork the last step's sweep)
            for s in self.sets:
                for rec in s["recs"]:
                    ops._pre_gather(rec["weights"], FIELD_PAD, rec["idesc"], rec["i64"], rec["B"], NF, s["D"], training=True,
                                    keep=rec["cols"])
        for i, gr in enumerate(grads):
            gd = gr.to(dev())
            for P in (self.A[i], self.L[i]):
                ops.grad_buffer(P).copy_(gd)
                P._rh_dirty = True
            self.ref[i], self.ms[i], self.vs[i] = O.adam_step(self.ref[i], gr.numpy().astype(F64), self.ms[i], self.vs[i],
                                                              self.t, lr=LR, weight_decay=WD)
        for s in self.sets:
            for rec in s["recs"]:
                ops._log_touch(rec["weights"], FIELD_PAD, rec["idesc"], rec["i64"], rec["B"], NF, s["D"], rec["cols"])
        self.lazy.step()
        self.dense.step()

    def assert_lag_bound(self):
        """Before the last flush: no lazy row is K steps or more behind -- K + 1 in the deferred form, where the window sweep of
        the step just taken has not been forked yet (the next refresh forks it)."""
        torch.cuda.synchronize()
        t = int(self.lazy._t_step.item())
        bound = K + 1 if self.lazy.overlap_sweep else K
        for p, last in zip(self.L, self.lazy._t_last):
            if self.lazy.table_k(p) != 1:
                lag = t - last
                assert int(lag.min()) >= 0 and int(lag.max()) < bound, (tuple(p.shape), int(lag.min()), int(lag.max()))

    def check(self, case):
        ops = self.ops
        torch.cuda.synchronize()
        ops.check_errors()
        steps = self.t
        assert int(self.lazy._t_step.item()) == steps and int(self.dense._t_step.item()) == steps
        worst = ("", 0.0)
        for i, (a, b) in enumerate(zip(self.A, self.L)):
            what = f"{case} table {i} {tuple(a.shape)}"
            assert torch.equal(a.detach(), b.detach()), f"{what}: lazy and dense parameters differ"
            assert torch.equal(self.dense.state[a]["exp_avg"], self.lazy.state[b]["exp_avg"]), f"{what}: exp_avg differs"
            assert torch.equal(self.dense.state[a]["exp_avg_sq"], self.lazy.state[b]["exp_avg_sq"]), f"{what}: exp_avg_sq differs"
            assert not bool(ops.grad_buffer(a).any()) and not bool(ops.grad_buffer(b).any()), f"{what}: gradient rows left"
            assert bool(torch.all(self.lazy._t_last[i] == steps)), f"{what}: rows behind step {steps} after the flush"
            for opt, p in ((self.dense, a), (self.lazy, b)):
                for name, got, want in (("param", p, self.ref[i]), ("exp_avg", opt.state[p]["exp_avg"], self.ms[i]),
                                        ("exp_avg_sq", opt.state[p]["exp_avg_sq"], self.vs[i])):
                    r = ratio(got, want, TOL[name], f"{what} {name}")
                    if r > worst[1]:
                        worst = (f"{name} of table {i}", r)
        print(f"LAZYTRIPS {case}: {steps} steps, worst error / bound {worst[1]:.3f} [{worst[0]}]")
        assert worst[1] <= 1.0, f"{case}: error / bound {worst[1]:.3f} at {worst[0]}"
        return worst


def ratio(got, want, atol_scale, what, rtol=1e-5):
    """max |got - want| / (atol + rtol |want|), atol = atol_scale max(1, max|want|): test_gpu_kernels.close as a figure."""
    got = got.detach().cpu().numpy().astype(F64)
    assert got.shape == want.shape and np.isfinite(got).all(), what
    atol = atol_scale * max(1.0, float(np.abs(want).max()))
    return float((np.abs(got - want) / (atol + rtol * np.abs(want))).max())


class Spy(object):
    """Counts the library calls by name (the optimizer reaches the library through _lib.call)."""

    def __init__(self, monkeypatch):
        from torch_rechub_amd import _lib
        self.n = {}
        real = _lib.call

        def call(name, *args):
            self.n[name] = self.n.get(name, 0) + 1
            return real(name, *args)

        monkeypatch.setattr(_lib, "call", call)

    def __getitem__(self, name):
        return self.n.get(name, 0)


def flush_with_cap(run, caps, sweep_cap, flush_cap):
    caps(sweep=flush_cap)
    run.lazy.flush()
    caps(sweep=sweep_cap)


def flush_cap_of(grps, caps):
    """3 or 4, whichever leaves every group's flush ragged (the flush takes the in-line cap)."""
    for cap in (3, 4):
        caps(sweep=cap)
        pls = [plan(g, FLUSH) for g in grps]
        if all(pl[1] == cap and pl[0] > 2 * cap and pl[0] % cap != 0 for pl in pls):
            return cap
    raise AssertionError(f"flush: neither 3 nor 4 workgroups leave a ragged tail: {pls}")


def drive(run, caps, sweep_cap, flush_cap, flush_every=None, before_flush=None):
    for _ in range(STEPS):
        run.step()
        if flush_every and run.t % flush_every == 0:
            flush_with_cap(run, caps, sweep_cap, flush_cap)
    if before_flush is not None:
        before_flush()
    flush_with_cap(run, caps, sweep_cap, flush_cap)


def one_width(D, overlap, dtype, caps, monkeypatch, flush_every=None):
    R = 1024 // D
    run = Run([(D, 1, [(NB, dtype)])], overlap, small_rows=5 * R + 3, seed=1000 + D + int(overlap))
    assert run.kinds() == [1, K, 1, K, K]
    (grp,) = run.groups()
    assert list(grp["h_win"]) == [5 * R + 3, 6 * R + 5, 7, 4 * R, 3 * R // 2 + 1]
    assert 3 * (6 * R + 5) + (6 * R + 5) - 2 == run.sets[0]["rows"][1]  # t_a's last window is 2 rows short
    tb = TOUCH_BLOCKS
    flush_cap = flush_cap_of([grp], caps)
    caps(sweep=3, deferred=3)
    if overlap:
        lazy_pl = plan(grp, LAZY_TABLES, t_value=1)  # the deferred sweep of the lazy tables, by value
        assert lazy_pl == ((7, 3, 1, 1) if D >= 8 else (13, 3, 1, 0)), lazy_pl
        assert_past_cap(lazy_pl, 3, "deferred sweep")
        merged = plan(grp, DENSE_TABLES, touch_blocks=tb)  # the end of the step: touched rows + the dense tables
        assert merged == (7, 3, 1, 0), merged
    else:
        merged = plan(grp, WINDOW, touch_blocks=tb)  # touched rows + the window of every table, claims inside the sweep
        assert merged == (20, 3, 1, 0), merged
    assert_past_cap(merged, 3, "merged end-of-step launch")
    spy = Spy(monkeypatch)
    drive(run, caps, 3, flush_cap, flush_every=flush_every, before_flush=run.assert_lag_bound)
    assert spy["rh_adam_lazy_step_mode_idx"] == STEPS and spy["rh_adam_lazy_touched_group"] == 0
    assert spy["rh_adam_lazy_touched"] == (STEPS if overlap else 0)  # the refresh in front of every step
    n_flush = (STEPS // flush_every if flush_every else 0) + 1
    # deferred: every step's sweep is forked by the next refresh, but for the steps a flush took over
    assert spy["rh_adam_lazy_sweep"] == n_flush + ((STEPS - n_flush) if overlap else 0)
    return run


# ---- every width --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [4, 8, 16, 32, 64, 128])
def test_every_width_deferred_sweep_past_its_cap(D, caps, monkeypatch):
    """overlap_sweep: refresh -> fork the wide (D >= 8) or narrow (D = 4) sweep of the lazy tables, 7 / 13 units on 3
    workgroups; the end of the step is the merged touched-rows + dense-tables launch, 7 units on 3."""
    one_width(D, True, torch.int64, caps, monkeypatch).check(f"deferred D={D}")


@pytest.mark.parametrize("D,dtype", [(4, torch.int64), (8, torch.int64), (16, torch.int64), (32, torch.int64), (64, torch.int64),
                                     (128, torch.int64), (8, torch.int32), (64, torch.int32)],
                         ids=lambda v: str(v).replace("torch.", ""))
def test_every_width_inline_merged_sweep_past_its_cap(D, dtype, caps, monkeypatch):
    """In line: ONE merged launch per step (rh_adam_lazy_step_mode_idx, RH_SWEEP_WINDOW), 20 units on 3 sweep workgroups beside
    12 touched-rows workgroups, the claims made inside the sweep; int32 index columns at D = 8 and 64.  Before the last flush no
    lazy row lags K steps or more."""
    one_width(D, False, dtype, caps, monkeypatch).check(f"inline D={D} {str(dtype)[6:]}")


@pytest.mark.parametrize("D,overlap", [(64, True), (16, False)])
def test_flush_every_three_steps(D, overlap, caps, monkeypatch):
    """The flush (past its cap, ragged) in the middle of the run: a deferred sweep joined and subsumed, windows re-swept."""
    one_width(D, overlap, torch.int64, caps, monkeypatch, flush_every=3).check(f"flush every 3, D={D} overlap={overlap}")


# ---- the interleaved merged launch ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D", [16, 64])
@pytest.mark.parametrize("rule", ["plain", "minus-one"])
def test_interleaved_merged_launch_past_its_cap(D, rule, caps, monkeypatch):
    """Tables large enough (all sizes x one integer) for a touch_period above 1 while the window is past the cap: every
    touch_period-th workgroup of the merged launch is a touched-rows one, the sweep's workgroups number the rest.  "plain": a
    period that is no multiple of 8; "minus-one": (grid + 12) / 12 = 8, which the keep-every-XCD rule turns into 7.  Cap and
    multiplier come from the plan query."""
    tb = TOUCH_BLOCKS
    R = 1024 // D
    # minus-one: the least cap with (cap + tb) / tb = 8; plain: from 2.5 tb on, the first one the query accepts
    cap_range = [7 * tb] if rule == "minus-one" else range(5 * tb // 2, 7 * tb)
    found = None
    for mult in range(1, 17):
        trial = group_of(D, mult, mult * (5 * R + 3))
        for cap in cap_range:
            caps(sweep=cap)
            pl = plan(trial, WINDOW, touch_blocks=tb)
            period_ok = pl[2] == 7 if rule == "minus-one" else (pl[2] > 1 and pl[2] % 8 != 0)
            if pl[1] == cap and pl[0] > 2 * cap and pl[0] % cap != 0 and period_ok:
                found = (mult, cap)
                break
        if found:
            break
    assert found, "no multiplier up to 16 puts the window past a cap with such a period"
    mult, cap = found
    run = Run([(D, mult, [(NB, torch.int64)])], False, small_rows=mult * (5 * R + 3), seed=2000 + D)
    assert run.kinds() == [1, K, 1, K, K]
    (grp,) = run.groups()
    assert list(grp["h_rows"]) == list(trial["h_rows"]) and list(grp["h_win"]) == list(trial["h_win"])
    pl = plan(grp, WINDOW, touch_blocks=tb)
    assert_past_cap(pl, cap, "interleaved merged launch")
    assert pl[3] == 0
    if rule == "minus-one":
        assert (cap + tb) // tb == 8 and pl[2] == 7
    else:
        assert pl[2] == (cap + tb) // tb and pl[2] > 1 and pl[2] % 8 != 0
    assert (tb - 1) * pl[2] < cap + tb  # every touched-rows workgroup exists
    flush_cap = ragged_cap([plan(grp, FLUSH)[0]], (cap, cap + 1, cap + 2))
    caps(sweep=cap)
    spy = Spy(monkeypatch)
    drive(run, caps, cap, flush_cap, before_flush=run.assert_lag_bound)
    assert spy["rh_adam_lazy_step_mode_idx"] == STEPS
    run.check(f"interleaved D={D} x{mult} cap {cap} period {pl[2]}")


# ---- unmerged launches --------------------------------------------------------------------------------------------------------
def _caps_for(grps, overlap, caps, candidates=range(3, 9)):
    """One in-line cap, one deferred cap and one flush cap under which EVERY group's launches are past the cap and ragged."""
    caps(sweep=1, deferred=1)  # (unit counts do not depend on the caps)
    inline_units = [plan(g, DENSE_TABLES if overlap else WINDOW)[0] for g in grps]
    sweep_cap = ragged_cap(inline_units, candidates)
    deferred_cap = ragged_cap([plan(g, LAZY_TABLES, t_value=1)[0] for g in grps], candidates) if overlap else 512
    flush_cap = ragged_cap([plan(g, FLUSH)[0] for g in grps], candidates)
    caps(sweep=sweep_cap, deferred=deferred_cap)
    for g in grps:
        assert_past_cap(plan(g, DENSE_TABLES if overlap else WINDOW), sweep_cap, f"D={g['D']} in-line sweep")
        if overlap:
            pl = plan(g, LAZY_TABLES, t_value=1)
            assert_past_cap(pl, deferred_cap, f"D={g['D']} deferred sweep")
            assert pl[3] == 1  # the wide kernel
    caps(sweep=flush_cap)
    for g in grps:
        assert_past_cap(plan(g, FLUSH), flush_cap, f"D={g['D']} flush")
    caps(sweep=sweep_cap)
    return sweep_cap, flush_cap


@pytest.mark.parametrize("overlap", [False, True], ids=["inline", "deferred"])
def test_two_table_groups_take_the_unmerged_launches(overlap, caps, monkeypatch):
    """One optimizer over the D = 8 and the D = 32 table sets: two groups, so the touched-rows passes (_touch_many: one
    rh_adam_lazy_touched per record) and rh_adam_lazy_sweep run per group, unmerged -- the plain narrow sweep kernel with the
    gradient of the dense tables, the RH_SWEEP_WINDOW sweep without claims.  The D = 32 set has its sizes x 4 (the rows of the
    D = 8 set's units), so that ONE lazy_small_rows keeps both sets' tables in their kinds."""
    small = 4 * (5 * 32 + 3)
    run = Run([(8, 1, [(NB, torch.int64)]), (32, 4, [(NB, torch.int64)])], overlap, small_rows=small, seed=3000 + int(overlap))
    assert run.kinds() == [1, K, 1, K, K] * 2
    grps = run.groups()
    sweep_cap, flush_cap = _caps_for(grps, overlap, caps)
    spy = Spy(monkeypatch)
    drive(run, caps, sweep_cap, flush_cap, before_flush=run.assert_lag_bound)
    assert spy["rh_adam_lazy_step_mode_idx"] == 0 and spy["rh_adam_lazy_touched_group"] == 0
    assert spy["rh_adam_lazy_touched"] == 2 * STEPS * (2 if overlap else 1)  # per record: the step's pass (+ its refresh)
    # per group: the in-line sweep of every step, the flush, and (deferred) the forked sweep of every step but the last
    assert spy["rh_adam_lazy_sweep"] == 2 * (STEPS + 1 + ((STEPS - 1) if overlap else 0))
    run.check(f"two groups D=8+32 overlap={overlap}")


@pytest.mark.parametrize("overlap", [False, True], ids=["inline", "deferred"])
def test_two_gather_records_take_the_grouped_touched_launch(overlap, caps, monkeypatch):
    """One D = 64 group, two gather records per step of different batch sizes (97 lookups per field, int32; 33, int64): the
    touched-rows passes of the step are ONE rh_adam_lazy_touched_group launch with n = 2, the sweep a launch of its own."""
    R = 1024 // 64
    run = Run([(64, 1, [(NB, torch.int32), (33, torch.int64)])], overlap, small_rows=5 * R + 3, seed=4000 + int(overlap))
    assert run.kinds() == [1, K, 1, K, K]
    grps = run.groups()
    sweep_cap, flush_cap = _caps_for(grps, overlap, caps)
    spy = Spy(monkeypatch)
    drive(run, caps, sweep_cap, flush_cap, before_flush=run.assert_lag_bound)
    assert spy["rh_adam_lazy_touched_group"] == STEPS and spy["rh_adam_lazy_step_mode_idx"] == 0
    assert spy["rh_adam_lazy_touched"] == (2 * STEPS if overlap else 0)  # the two refreshes in front of every step
    assert spy["rh_adam_lazy_sweep"] == STEPS + 1 + ((STEPS - 1) if overlap else 0)
    run.check(f"two records D=64 overlap={overlap}")
