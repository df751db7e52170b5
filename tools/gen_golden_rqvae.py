"""Generate the RQ-VAE fixtures of tests/golden/ from the UNMODIFIED reference (CPU).

Run where the reference checkout exists:  ``python tools/gen_golden_rqvae.py``

  model_rqvae.npz    RQVAEModel(in_dim=24, num_emb_list=[8, 6, 5], e_dim=8, layers=[16, 12], dropout_prob=0.0, beta=0.25,
                     quant_loss_weight=1.0, loss_type="mse", kmeans_init=False, sk_epsilons=[0, 0, 0]).  The codebooks are
                     redrawn N(0, 0.5) before sd0 is saved (the reference's uniform(+-1 / n_e) leaves every code within a hair of
                     the others), and the BatchNorm running statistics are set to those of a 4000-row draw (at their initial 0 / 1 the
                     eval-mode encoder sends every row to the same few codes).  Eval and train forward (out, rq_loss, indices), compute_loss, the parameter gradients of one
                     probe step, three steps of the reference's Trainer loop (B = 48, Adam, lr 1e-2, weight decay 1e-3); get_indices
                     on a second data set of 40 rows without collisions and the dict generate_semantic_ids returns for it (as a
                     (40, 3) array of strings); the same for a third, the second plus eight near-duplicate rows (near_duplicates).
  rqvae_layers.npz   one forward / backward of ResidualVectorQuantizer on its own inputs (N = 12, E = 8, sizes [8, 6, 5]): per
                     level the residual, the (N, K) distances, the indices, the level's output and loss; x_q, the mean loss and
                     the gradients for a drawn g_xq and g_loss.  A second forward with sk_epsilons = [0, 0, 0.003], sk_iters = 50:
                     the last level's centred distances, Q and indices.

argmin and argmax are discontinuities: where the two nearest codes of a row are closer than fp32 rounding, the reference's own
fp32 and another correct implementation may pick different codes, and the fixture would pin noise.  So for every row recorded,
at every level and at the model state that batch meets, the float64 gap (d_2 - d_1) / (||r||^2 + max_k ||c_k||^2) must be at
least 1e-3, and for the Sinkhorn level the top-2 gap of Q relative to its row maximum as well; the generator re-seeds until
that holds.  The second data set is the first 40 rows of a longer draw whose IDs are new and whose gaps pass.  The archives are
written with a fixed member timestamp: the files regenerate byte-identically.
"""
import copy
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_golden_ffm import _save_fixed  # noqa: E402
from oracle import gen_golden as G  # noqa: E402
from oracle.ref_import import import_reference  # noqa: E402

IN_DIM, SIZES, E, LAYERS, BETA = 24, [8, 6, 5], 8, [16, 12], 0.25
LR, WD = 1e-2, 1e-3
MIN_GAP = 1e-3
SK_EPS, SK_ITERS = 0.003, 50


class GapTooSmall(Exception):
    pass


def build(sk_epsilons=(0, 0, 0)):
    from torch_rechub.models.generative.rqvae import RQVAEModel
    return RQVAEModel(in_dim=IN_DIM, num_emb_list=list(SIZES), e_dim=E, layers=list(LAYERS), dropout_prob=0.0, beta=BETA,
                      quant_loss_weight=1.0, loss_type="mse", kmeans_init=False, sk_epsilons=list(sk_epsilons))


def row_gaps(x, codebooks):
    """Per row, the smallest over the levels of (d_2 - d_1) / (||r||^2 + max_k ||c_k||^2), hard assignment, in float64."""
    r = x.double()
    worst = torch.full((r.shape[0],), float("inf"), dtype=torch.float64)
    for C in codebooks:
        C = C.double()
        d = ((r[:, None, :] - C[None, :, :])**2).sum(-1)
        srt = torch.sort(d, dim=1).values
        if C.shape[0] > 1:
            worst = torch.minimum(worst, (srt[:, 1] - srt[:, 0]) / ((r**2).sum(1) + (C**2).sum(1).max()))
        r = r - C[d.argmin(1)]
    return worst


def model_gaps(model, x):
    """row_gaps of the encoder's output at the model's state and mode, on a float64 copy (the copy's BatchNorm statistics move)."""
    m = copy.deepcopy(model).double()
    with torch.no_grad():
        z = m.encoder(x.double())
    return row_gaps(z, [vq.embedding.weight.detach() for vq in m.rq.vq_layers])


def check_gap(model, x, what):
    gap = float(model_gaps(model, x).min())
    if gap < MIN_GAP:
        raise GapTooSmall(f"{what}: relative gap {gap:.2e} < {MIN_GAP}")
    return gap


class CheckedBatches(list):
    """The batches of the training epoch; each is checked against the state the model has when the trainer takes it."""

    def __init__(self, batches, model):
        super().__init__(batches)
        self.model, self.gaps = model, []

    def __iter__(self):
        for i, x in enumerate(list.__iter__(self)):
            self.gaps.append(check_gap(self.model, x, f"training batch {i}"))
            yield x


def redraw_codebooks(module, g):
    for m in module.modules():
        if isinstance(m, torch.nn.Embedding):
            torch.nn.init.normal_(m.weight, 0, 0.5, generator=g)


def prime_batchnorm(model, x):
    """Running statistics := the statistics of one training-mode pass over x (momentum 1 for that pass)."""
    bns = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm1d)]
    for bn in bns:
        bn.momentum = 1.0
    model.train()
    with torch.no_grad():
        model(x)
    for bn in bns:
        bn.momentum = 0.1
        bn.num_batches_tracked.zero_()


def near_duplicates(model, data2, ids2, seed):
    """The third data set: data2 plus eight near-duplicate rows (base row + 1e-2 N(0, 1)), one each of the first eight items
    whose first two codes no other item shares -- so a reassigned last code cannot land on a third item's ID and the
    reference's loop separates every pair in its first round.  The noise is re-drawn until each duplicate collides with its
    item, its arg-min gaps pass and, in every Sinkhorn call of the loop, the top-2 gap of Q relative to its row maximum is
    at least MIN_GAP.  Recorded: the rows, the hard indices, the dict generate_semantic_ids returns, the number of rounds."""
    from torch_rechub.models.generative.rqvae import VectorQuantizer, sinkhorn_algorithm
    prefixes = [tuple(r[:2]) for r in ids2.tolist()]
    bases = [i for i, p in enumerate(prefixes) if prefixes.count(p) == 1][:8]
    if len(bases) < 8:
        raise GapTooSmall(f"only {len(bases)} items with a first-two-codes prefix of their own")
    for attempt in range(64):
        g = torch.Generator().manual_seed(seed + 3 + 1000 * attempt)
        data3 = torch.cat([data2, data2[bases] + 1e-2 * torch.randn(8, IN_DIM, generator=g)])
        if float(model_gaps(model, data3).min()) < MIN_GAP:
            continue
        hard = model.get_indices(data3)
        if not torch.equal(hard[40:], hard[bases]):
            continue
        m = copy.deepcopy(model)
        checks, q_gaps, inner = [], [], m.get_indices

        def watched(xs, use_sk=False):
            if use_sk:  # the last level's Q of this call, restated
                r = m.encoder(xs)
                for vq in m.rq.vq_layers[:-1]:
                    r = r - vq(r, use_sk=False)[0]
                C = m.rq.vq_layers[-1].embedding.weight
                d = torch.sum(r**2, dim=1, keepdim=True) + torch.sum(C**2, dim=1, keepdim=True).t() - 2 * torch.matmul(r, C.t())
                Q = sinkhorn_algorithm(VectorQuantizer.center_distance_for_constraint(d).double(), m.rq.vq_layers[-1].sk_epsilon,
                                       m.rq.vq_layers[-1].sk_iters)
                top = torch.sort(Q, dim=1, descending=True).values
                q_gaps.append(float(((top[:, 0] - top[:, 1]) / top[:, 0]).min()))
                assert torch.equal(inner(xs, use_sk=True)[:, -1], Q.argmax(-1))
            return inner(xs, use_sk=use_sk)

        check = m._check_collision
        m._check_collision = lambda s: checks.append(check(s)) or checks[-1]
        m.get_indices = watched
        with torch.no_grad():
            sids = m.generate_semantic_ids(data3, torch.utils.data.DataLoader(data3, batch_size=16), device="cpu")
        if not checks[-1] or len(checks) > 20 or min(q_gaps) < MIN_GAP:
            continue
        assert len({tuple(v) for v in sids.values()}) == 48
        return {"data3": G.npy(data3), "dup_of": np.array(bases), "indices3": G.npy(hard), "sids3": np.array([sids[i] for i in range(48)]),
                "rounds3": np.array(len(checks) - 1), "sk_min_gap3": np.array(min(q_gaps))}
    raise GapTooSmall("no draw of near-duplicates that the loop separates with a Sinkhorn gap")


def gen_model(seed):
    from torch_rechub.trainers.rqvae_trainer import Trainer
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed + 1)
    model = build()
    redraw_codebooks(model, g)
    prime_batchnorm(model, torch.randn(4000, IN_DIM, generator=g))
    B = 48
    batches = [torch.randn(B, IN_DIM, generator=g) for _ in range(3)]
    out = {"cfg": np.array("rqvae"), "seed": np.array(seed), "cfg.in_dim": np.array(IN_DIM), "cfg.num_emb_list": np.array(SIZES),
           "cfg.e_dim": np.array(E), "cfg.layers": np.array(LAYERS), "cfg.beta": np.array(BETA)}
    for n, t in model.state_dict().items():
        out["sd0." + n] = G.npy(t)
    for bi, bx in enumerate(batches):
        out[f"x{bi}"] = G.npy(bx)
    x = batches[0]
    model.eval()
    gaps = [check_gap(model, x, "batch 0 at sd0, eval")]
    with torch.no_grad():
        o, ql, ind = model(x)
    out["out_eval"], out["rq_loss_eval"], out["indices_eval"] = G.npy(o), np.array(ql.item(), np.float32), G.npy(ind)

    # the second data set: the first 40 rows of a longer draw with a new ID each and a passing gap
    cand = torch.randn(4000, IN_DIM, generator=g)
    cand_gap = model_gaps(model, cand)
    cand_ids = model.get_indices(cand).tolist()
    rows, seen = [], set()
    for i, code in enumerate(cand_ids):
        if tuple(code) not in seen and float(cand_gap[i]) >= MIN_GAP:
            seen.add(tuple(code))
            rows.append(i)
        if len(rows) == 40:
            break
    if len(rows) < 40:
        raise GapTooSmall(f"only {len(rows)} distinct IDs among the candidates")
    data2 = cand[rows].clone()
    gaps.append(check_gap(model, data2, "second data set"))
    ids2 = model.get_indices(data2)
    assert len({tuple(r) for r in ids2.tolist()}) == 40
    sid_model = copy.deepcopy(model)
    sids = sid_model.generate_semantic_ids(data2, torch.utils.data.DataLoader(data2, batch_size=16), device="cpu")
    out["data2"], out["indices2"] = G.npy(data2), G.npy(ids2)
    out["sids2"] = np.array([sids[i] for i in range(40)])
    out["sk_epsilon_after"] = np.array([vq.sk_epsilon for vq in sid_model.rq.vq_layers], np.float64)

    out.update(near_duplicates(model, data2, ids2, seed))

    model.train()
    sd_backup = copy.deepcopy(model.state_dict())
    gaps.append(check_gap(model, x, "batch 0 at sd0, train"))
    o, ql, ind = model(x)
    loss, loss_recon = model.compute_loss(o, ql, xs=x)
    model.zero_grad()
    loss.backward()
    out["out_train"], out["rq_loss_train"], out["indices_train"] = G.npy(o), np.array(ql.item(), np.float32), G.npy(ind)
    out["loss"], out["loss_recon"] = np.array(loss.item(), np.float32), np.array(loss_recon.item(), np.float32)
    for n, p in model.named_parameters():
        out["grad." + n] = G.npy(p.grad) if p.grad is not None else np.zeros(tuple(p.shape), np.float32)
    model.load_state_dict(sd_backup)
    model.zero_grad()
    trainer = Trainer(model, optimizer_params={"lr": LR, "weight_decay": WD}, n_epoch=1, device="cpu")
    checked = CheckedBatches(batches, model)
    total_loss, total_recon = trainer.train_one_epoch(checked)
    gaps += checked.gaps
    assert len(checked.gaps) == 3
    out["train.lr"], out["train.wd"] = np.array(LR), np.array(WD)
    out["train.total_loss"], out["train.total_recon_loss"] = np.array(total_loss), np.array(total_recon)
    out["min_gap"] = np.array(min(gaps))
    for n, t in model.state_dict().items():
        out["sd3." + n] = G.npy(t)
    return out


def gen_layers(seed):
    from torch_rechub.models.generative.rqvae import ResidualVectorQuantizer, VectorQuantizer, sinkhorn_algorithm
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed + 2)
    N = 12
    rvq = ResidualVectorQuantizer(list(SIZES), E, sk_epsilons=[0, 0, 0], beta=BETA)
    redraw_codebooks(rvq, g)
    x = torch.randn(N, E, generator=g).requires_grad_(True)
    g_xq, g_loss = torch.randn(N, E, generator=g), 1.7
    cbs = [vq.embedding.weight for vq in rvq.vq_layers]
    gap = float(row_gaps(x.detach(), [c.detach() for c in cbs]).min())
    if gap < MIN_GAP:
        raise GapTooSmall(f"layers: relative gap {gap:.2e} < {MIN_GAP}")
    seen = []
    hooks = [vq.register_forward_hook(lambda mod, inp, res, seen=seen: seen.append((inp[0], res))) for vq in rvq.vq_layers]
    x_q, loss, idx = rvq(x)
    for h in hooks:
        h.remove()
    ((x_q * g_xq).sum() + g_loss * loss).backward()
    out = {"x": G.npy(x), "beta": np.array(BETA), "g_xq": G.npy(g_xq), "g_loss": np.array(g_loss), "seed": np.array(seed),
           "x_q": G.npy(x_q), "loss": np.array(loss.item(), np.float32), "idx": G.npy(idx), "g_x": G.npy(x.grad),
           "min_gap": np.array(gap)}
    for l, (r, (x_res, lvl_loss, lvl_idx)) in enumerate(seen):
        C = cbs[l].detach()
        out[f"C{l}"], out[f"g_C{l}"] = G.npy(C), G.npy(cbs[l].grad)
        out[f"r{l}"] = G.npy(r)
        rd = r.detach()
        out[f"d{l}"] = G.npy(torch.sum(rd**2, dim=1, keepdim=True) + torch.sum(C**2, dim=1, keepdim=True).t() - 2 * torch.matmul(rd, C.t()))
        out[f"x_res{l}"], out[f"loss{l}"], out[f"idx{l}"] = G.npy(x_res), np.array(lvl_loss.item(), np.float32), G.npy(lvl_idx)

    # the same rows with the Sinkhorn assignment at the last level
    sk = ResidualVectorQuantizer(list(SIZES), E, sk_epsilons=[0, 0, SK_EPS], beta=BETA, sk_iters=SK_ITERS)
    sk.load_state_dict(rvq.state_dict())
    with torch.no_grad():
        sk_xq, sk_loss, sk_idx = sk(x.detach())
        r2, C2 = seen[2][0].detach(), cbs[2].detach()
        d = torch.sum(r2**2, dim=1, keepdim=True) + torch.sum(C2**2, dim=1, keepdim=True).t() - 2 * torch.matmul(r2, C2.t())
        dc = VectorQuantizer.center_distance_for_constraint(d).double()
        Q = sinkhorn_algorithm(dc, SK_EPS, SK_ITERS)
    assert torch.equal(sk_idx[:, :2], idx[:, :2]) and torch.equal(sk_idx[:, 2], Q.argmax(-1))
    top = torch.sort(Q, dim=1, descending=True).values
    q_gap = float(((top[:, 0] - top[:, 1]) / top[:, 0]).min())
    if q_gap < MIN_GAP:
        raise GapTooSmall(f"layers: Sinkhorn top-2 gap {q_gap:.2e} < {MIN_GAP}")
    out.update({"sk_epsilon": np.array(SK_EPS), "sk_iters": np.array(SK_ITERS), "sk_dc": G.npy(dc), "sk_Q": G.npy(Q),
                "sk_idx": G.npy(sk_idx), "sk_x_q": G.npy(sk_xq), "sk_loss": np.array(sk_loss.item(), np.float32),
                "sk_min_gap": np.array(q_gap)})
    return out


def reseeding(fn, what):
    for attempt in range(1024):
        try:
            return fn(G.SEED + 100 * attempt)
        except GapTooSmall as e:
            print(f"{what}: seed {G.SEED + 100 * attempt} rejected ({e})")
    raise RuntimeError(f"{what}: no seed with a gap of {MIN_GAP}")


def main():
    import_reference()
    out = reseeding(gen_model, "model_rqvae")
    _save_fixed(os.path.join(G.OUT, "model_rqvae.npz"), out)
    print("model_rqvae.npz", len(out), "arrays, seed", int(out["seed"]), "loss", float(out["loss"]), "min gap", float(out["min_gap"]))
    layers = reseeding(gen_layers, "rqvae_layers")
    _save_fixed(os.path.join(G.OUT, "rqvae_layers.npz"), layers)
    print("rqvae_layers.npz", len(layers), "arrays, seed", int(layers["seed"]), "min gap", float(layers["min_gap"]),
          "Sinkhorn gap", float(layers["sk_min_gap"]))


if __name__ == "__main__":
    main()
