"""The end-of-step launch of the step-ahead form (rh_adam_lazy_step_ahead_wgrad: refresh of the next batch's rows, touched-rows
step, lookahead, batch assembly, dense tables, weight-gradient rider) across the shapes at which its parts take different paths:
batches of less than one workgroup pass / a partial last chunk / several chunks, embed_dim 4 .. 128 (1 .. 32 lanes per row),
tables from a thousand to 150 000 rows, duplicated samples, a padding row, and lookahead workgroups that collect their hits over
several rounds of samples (carried over / flushed early / two workgroups per field).  Small twins of
test_gpu_models.py::test_full_size_graph_step_with_long_sweeps_equals_dense_adam_bitwise: a blocked-lazy trainer (lazy_k = 8,
every table lazy) against a table_update="dense" twin from the same state dict, 3 eager steps + 27 hipGraph replays (every
window swept three times over; rows lag 0 .. lazy_k steps), bit for bit after the flush.  Reference semantics:
torch.optim.Adam steps every row every step (trainers/ctr_trainer.py:59-61,99).  The launch whose touched-rows part walks
another index matrix (rh_adam_lazy_step_ahead_touched, data parallel with replicated tables) has no case here: it runs the same
parts, and the one-rank data-parallel training of tests/test_gpu_models.py goes through it and asserts that it ran
(test_replicated_step_with_a_second_ranks_rows_is_the_same_in_every_form_of_its_head_and_tail[merged])."""
import pytest
import torch

from test_gpu_models import _assert_no_row_behind, _duplicate_samples, dev

pytestmark = pytest.mark.gpu

VOCABS = [1000, 3000, 20000, 150000]
BIG_VOCABS = [20000, 150000]  # for the batches of more than 500 samples (a progression needs more than 2 B rows)
LOOK_ROUND = 1024  # samples whose index loads a lookahead workgroup keeps in flight together (csrc/optim.hip, kAheadLookRounds)
LOOK_FLUSH = 256   # it flushes its list of hits early once it holds more rows than this


def _nb(lazy_k):
    return 3 + 3 * lazy_k + 3  # batches = steps of the one epoch


def _progressions(v, n, nb, g, first_row=1, n_rows=None, spread=False):
    """(nb, n) rows of a table of v rows, every batch an arithmetic progression inside rows first_row .. : no row twice in a
    batch, so the table gradient has no order-dependent float sums and two trainings are comparable bit for bit.
    spread: the progression spans the whole table and the batch's samples come in random order, so ANY run of samples of a
    batch holds about the same share of its rows in every window of the table."""
    n_rows = (v - first_row) if n_rows is None else n_rows
    assert n_rows > 2 * n
    stride = torch.randint(n_rows // n if spread else max(1, n_rows // n // 2), n_rows // n + 1, (nb, 1), generator=g)
    start = (torch.rand(nb, 1, generator=g) * (n_rows - stride * (n - 1))).long()
    rows = start + stride * torch.arange(n).view(1, n)
    if spread:
        rows = torch.stack([r[torch.randperm(n, generator=g)] for r in rows])
    return rows


def _data(B, layout, seed, VOCABS=VOCABS, NB=_nb(8)):
    g = torch.Generator().manual_seed(seed)
    if layout != "dup":
        # "flush": every lookup in the lower half of its table, so the windows there hold twice their share of the samples
        cols = [(_progressions(v, B, NB, g, spread=layout in ("carry", "flush"),
                               n_rows=(v - 1) // 2 if layout == "flush" else None) + 1).view(-1) for v in VOCABS]
        sparse = torch.stack(cols, 1).contiguous()
        dense = torch.rand(NB * B, 3, generator=g)
        label = (torch.rand(NB * B, generator=g) < 0.3).float()
        if layout == "pad":  # field 1 carries padding_idx = 0, and a seventh of its lookups ARE the padding index
            sparse[::7, 1] = 0
        for i in range(len(VOCABS)):  # the condition for bitwise twins, on the CPU tensors
            for b in range(NB):
                col = sparse[b * B:(b + 1) * B, i]
                live = col[col != 0] if (layout == "pad" and i == 1) else col
                assert live.unique().numel() == live.numel() and (layout == "pad" and i == 1 or live.numel() == B)
        return sparse, dense, label
    # every sample twice in its batch (identical addends: 0 + g, g + g in either order) and every row again in the next batch:
    # batch b looks up the rows U_b and U_(b-1), B/4 fresh rows each from the rows whose parity is that of the batch
    q = B // 4
    cols = []
    for v in VOCABS:
        n_class = (v - 2) // 2
        fresh = 1 + (torch.arange(NB + 1).view(-1, 1) % 2) + 2 * _progressions(v, q, NB + 1, g, n_rows=n_class)
        cols.append(torch.cat([fresh[1:], fresh[:-1]], 1).reshape(-1))  # (NB, B/2): U_b | U_(b-1)
    sparse = _duplicate_samples(torch.stack(cols, 1).contiguous(), B)
    dense = _duplicate_samples(torch.rand(NB * B // 2, 3, generator=g), B)
    label = _duplicate_samples((torch.rand(NB * B // 2, generator=g) < 0.3).float(), B)
    first, second = sparse[:B], sparse[B:2 * B]
    assert torch.equal(first[:B // 2], first[B // 2:]) and first[:, 0].unique().numel() == B // 2
    assert set(first[:B // 4, 0].tolist()) <= set(second[:, 0].tolist())  # U_1: fresh in batch 0, looked up again by batch 1
    return sparse, dense, label


def _first_round_hits(sparse, B, vocabs, lazy_k):
    """Per step, field and window of the table: how many of the first LOOK_ROUND samples the lookahead walks (the two batches
    after the next one) lie in that window of ceil(rows / lazy_k) rows -- (min, max) over all of them."""
    lo, hi = None, 0
    for i, v in enumerate(vocabs):
        w = -(-v // lazy_k)
        for b in range(sparse.shape[0] // B - 3):
            first = sparse[(b + 2) * B:(b + 2) * B + LOOK_ROUND, i]
            cnt = torch.bincount(first // w, minlength=lazy_k)
            lo, hi = (int(cnt.min()) if lo is None else min(lo, int(cnt.min()))), max(hi, int(cnt.max()))
    return lo, hi


CASES = [  # (B, embed_dim, layout)
    (64, 16, "plain"),    # less than one pass of the refresh part
    (200, 16, "plain"),   # a partial last chunk
    (384, 16, "plain"),   # several whole chunks
    (200, 4, "plain"),    # one lane per row
    (200, 8, "plain"),
    (200, 32, "plain"),   # eight lanes per row
    (200, 64, "plain"),   # sixteen lanes per row: four rows per wavefront, 16 rows per pass of the refresh's re-deal
    (200, 128, "plain"),  # thirty-two lanes per row: two rows per wavefront, 8 rows per pass
    (200, 16, "dup"),     # two lookups race for one claim; a row wanted by the touched-rows step AND the refresh of one launch
    (200, 16, "pad"),     # the padding-row pass
    (600, 16, "carry"),   # lookahead: 1200 samples = two rounds, the first round's hits carried into the second
    (1536, 16, "flush"),  # lookahead, lazy_k = 4 (the least the step-ahead form takes), all lookups in the lower half of the
                          # tables: in the steps that sweep a window there, the first round's ~ 512 hits overflow the flush
                          # threshold with a round to go; two lookahead workgroups per field
]


@pytest.mark.parametrize("B,D,layout", CASES, ids=[f"B{b}-D{d}-{l}" for b, d, l in CASES])
def test_step_ahead_launch_equals_dense_adam_bitwise_across_shapes(B, D, layout, monkeypatch):
    from torch_rechub_amd import _lib, optim
    from torch_rechub_amd.basic.features import DenseFeature, SparseFeature
    from torch_rechub_amd.models.ranking import DeepFM
    from torch_rechub_amd.trainers import CTRTrainer
    from torch_rechub_amd.utils.data import DeviceDataLoader
    monkeypatch.setenv("RECHUB_STEP_FORM", "deferred")
    LAZY_K = 4 if layout == "flush" else 8
    NB = _nb(LAZY_K)
    VOCABS = BIG_VOCABS if B > 500 else globals()["VOCABS"]
    sparse, dense, label = _data(B, layout, seed=100 + B + D, VOCABS=VOCABS, NB=NB)
    assert all(int(sparse[:, i].max()) < v and int(sparse[:, i].min()) >= 0 for i, v in enumerate(VOCABS))
    if layout == "carry":  # whichever window a step sweeps: the first round leaves a list that is not flushed, a second follows
        lo, hi = _first_round_hits(sparse, B, VOCABS, LAZY_K)
        assert 2 * B > LOOK_ROUND and 1 <= lo and hi <= LOOK_FLUSH, (lo, hi)
    if layout == "flush":  # ... the first round's hits exceed the threshold while samples are left (every other pair of steps)
        lo, hi = _first_round_hits(sparse, B, VOCABS, LAZY_K)
        assert 2 * B > 2 * LOOK_ROUND and hi > LOOK_FLUSH + 128, (lo, hi)

    def build():
        torch.manual_seed(7)
        dfe = [DenseFeature(f"I{i}") for i in range(3)]
        sfe = [SparseFeature(f"C{i}", v, D, padding_idx=0 if (layout == "pad" and i == 1) else None)
               for i, v in enumerate(VOCABS)]
        m = DeepFM(dfe + sfe, sfe, {"dims": [32, 16], "dropout": 0.0, "activation": "relu"})
        with torch.no_grad():
            for i, e in enumerate(m.embedding.embed_dict.values()):
                e.weight.normal_(0, 0.05)
                if layout == "pad" and i == 1:
                    e.weight[0].zero_()
        return m, [f.name for f in sfe], [f.name for f in dfe]

    launches = {"rh_adam_lazy_step_ahead_wgrad": 0, "rh_adam_lazy_step_ahead": 0}
    real_call = _lib.call

    def spy(name, *args):
        if name in launches:
            launches[name] += 1
        return real_call(name, *args)

    monkeypatch.setattr(_lib, "call", spy)
    kw = dict(optimizer_params={"lr": 1e-2, "weight_decay": 1e-3}, device="cuda:0", show_progress=False, use_graph=True)
    ma, names, dnames = build()
    mb, _, _ = build()
    mb.load_state_dict(ma.state_dict())
    ta = CTRTrainer(ma, table_update="lazy", lazy_k=LAZY_K, lazy_small_rows=8, **kw)
    tb = CTRTrainer(mb, table_update="dense", **kw)
    assert ta.optimizer.lazy_k == LAZY_K and all(ta.optimizer.table_k(p) == LAZY_K for p in ta.optimizer._tables)
    losses = []
    for t in (ta, tb):
        dl = DeviceDataLoader(sparse.to(dev()), names, dense.to(dev()), dnames, label.to(dev()), B, shuffle=False)
        losses.append(t.train_one_epoch(dl))
        assert t._graph is not None
    assert ta._form == "deferred"
    assert len(ta.optimizer._sweep_events or ()) == optim.LOOK_DEPTH + 1  # the step-ahead form did run ...
    assert launches["rh_adam_lazy_step_ahead_wgrad"] >= 1 and launches["rh_adam_lazy_step_ahead"] == 0  # ... with the MLP's rider
    assert losses[0] == losses[1]
    assert _assert_no_row_behind(ta) == NB
    sa, sb = ma.state_dict(), mb.state_dict()
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k
    for pa, pb in zip(ta.optimizer._tables, tb.optimizer._tables):
        assert torch.equal(ta.optimizer.state[pa]["exp_avg"], tb.optimizer.state[pb]["exp_avg"])
        assert torch.equal(ta.optimizer.state[pa]["exp_avg_sq"], tb.optimizer.state[pb]["exp_avg_sq"])
