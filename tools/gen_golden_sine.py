"""Generate the SINE fixtures of tests/golden/ from the UNMODIFIED reference (CPU).

Run where the reference checkout exists:  ``python tools/gen_golden_sine.py``
Uses oracle/gen_golden.py's recipe (seed 2022, B = 48, three batches through the reference ``MatchTrainer(mode=2)``,
list-wise softmax with the positive in column 0) by importing its constants and helpers.

  model_sine.npz    SINE, 60 items, S = 8 positions, E = 16, hidden_dim 12, T = 10 concepts, K = 3 intentions, temperature
                    0.1, three negatives.  The three tables are redrawn N(0, 0.1) before sd0 is saved (the reference's
                    std 1e-4 leaves every concept score within rounding of the others).  History left-padded as the
                    example's, row 0 fully padded, row 1 full.  Eval forward, user-mode and item-mode outputs, probe loss
                    and parameter gradients, three trainer steps (Adam, lr 1e-2, weight decay 1e-3).
  sine_layers.npz   one forward / backward of sine.py:93-128 on its own inputs (B = 6, S = 8, E = 16, T = 10, K = 3): x_u,
                    the weights, every intermediate of the chain, the second half's gradients for a drawn g_v and the
                    first half's for drawn up_g_phi / up_g_xhat; the chain's output is checked against the reference model's user_tower before anything is saved.

torch.topk over the concept scores is a discontinuity: where two scores among a row's top K + 1 are closer than fp32
rounding, the reference's own fp32 and another correct implementation may pick different concepts, and the fixture
would pin noise.  So for every row of every batch recorded (at the model state that batch meets), the float64 gap between
adjacent scores among the top K + 1, divided by the row's max |s_u|, must be at least 1e-3; the generator re-seeds until
that holds.  The archives are written with a fixed member timestamp: the files regenerate byte-identically.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_golden_ffm import _save_fixed  # noqa: E402
from oracle import gen_golden as G  # noqa: E402
from oracle.ref_import import import_reference  # noqa: E402

N_ITEMS, S, E, H, T, K, NEG, TEMP = 60, 8, 16, 12, 10, 3, 3, 0.1
LR, WD = 1e-2, 1e-3
MIN_GAP = 1e-3


class GapTooSmall(Exception):
    pass


def build():
    from torch_rechub.models.matching import SINE
    return SINE(["hist_item_id"], ["item_id"], ["neg_items"], N_ITEMS, E, H, T, K, S, temperature=TEMP)


def left_padded(B, g):
    hist = torch.randint(1, N_ITEMS, (B, S), generator=g)
    lens = torch.randint(1, S + 1, (B,), generator=g)
    lens[0], lens[1] = 0, S
    hist[torch.arange(S)[None, :] < (S - lens)[:, None]] = 0
    return hist


def make_batch(B, g):
    x = {"hist_item_id": left_padded(B, g), "item_id": torch.randint(1, N_ITEMS, (B,), generator=g),
         "neg_items": torch.randint(1, N_ITEMS, (B, NEG), generator=g)}
    return x, torch.zeros(B, dtype=torch.long)


def score_gap(s_u, k):
    """min over rows of the smallest gap between adjacent scores among the top k + 1, relative to the row's max |s_u|."""
    top = torch.sort(s_u.double(), dim=1, descending=True).values[:, :k + 1]
    if top.shape[1] < 2:
        return float("inf")
    gap = (top[:, :-1] - top[:, 1:]).min(dim=1).values / s_u.double().abs().max(dim=1).values
    return float(gap.min())


def concept_scores64(model, hist):
    """s_u (sine.py:86-100) of the model's current state in float64."""
    sd = {k: v.detach().double() for k, v in model.state_dict().items()}
    x_u = sd["item_embedding.weight"][hist] + sd["position_embedding.weight"].unsqueeze(0)
    # -1e9 AT the dropped positions, which is what float32 makes of a + -1e9 (1 - mask): a fully padded row is uniform
    a = torch.where((hist > 0).unsqueeze(-1), torch.tanh(x_u @ sd["w_1"]) @ sd["w_2"], torch.full((), -1.e9, dtype=torch.float64))
    z_u = (x_u * F.softmax(a, dim=1)).sum(1)
    return z_u @ sd["concept_embedding.weight"].T


def check_gap(model, hist, what):
    gap = score_gap(concept_scores64(model, hist), K)
    if gap < MIN_GAP:
        raise GapTooSmall(f"{what}: relative top-{K + 1} gap {gap:.2e} < {MIN_GAP}")
    return gap


class CheckedBatches(list):
    """The batches of the training epoch; each is checked against the state the model has when the trainer takes it."""

    def __init__(self, batches, model):
        super().__init__(batches)
        self.model, self.gaps = model, []

    def __iter__(self):
        for i, (x, y) in enumerate(list.__iter__(self)):
            self.gaps.append(check_gap(self.model, x["hist_item_id"], f"training batch {i}"))
            yield x, y


def gen_model(seed):
    from torch_rechub.trainers import MatchTrainer
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed + 1)
    model = build()
    for m in model.modules():
        if isinstance(m, torch.nn.Embedding):
            torch.nn.init.normal_(m.weight, 0, 0.1, generator=g)
    B = 48
    batches = [make_batch(B, g) for _ in range(3)]
    cfg = {"num_items": N_ITEMS, "seq_max_len": S, "embedding_dim": E, "hidden_dim": H, "num_concept": T, "num_intention": K}
    out = {"cfg": np.array("sine"), "temperature": np.array(TEMP), "seed": np.array(seed)}
    out.update({"cfg." + k: np.array(v) for k, v in cfg.items()})
    for n, t in model.state_dict().items():
        out["sd0." + n] = G.npy(t)
    for bi, (bx, by) in enumerate(batches):
        for k, v in bx.items():
            out[f"x{bi}.{k}"] = G.npy(v)
        out[f"y{bi}"] = G.npy(by)
    x, y = batches[0]
    gaps = [check_gap(model, x["hist_item_id"], "batch 0 at sd0")]
    model.eval()
    with torch.no_grad():
        out["pred_eval"] = G.npy(model(x))
        model.mode = "user"
        out["user_emb"] = G.npy(model(x))
        model.mode = "item"
        out["item_emb"] = G.npy(model(x))
        model.mode = None
    model.train()
    sd_backup = {k: v.clone() for k, v in model.state_dict().items()}
    pred = model(x)
    loss = torch.nn.CrossEntropyLoss()(pred, y)
    model.zero_grad()
    loss.backward()
    out["pred_train"], out["loss"] = G.npy(pred), np.array(loss.item())
    for n, p in model.named_parameters():
        out["grad." + n] = G.npy(p.grad) if p.grad is not None else np.zeros(tuple(p.shape), np.float32)
    model.load_state_dict(sd_backup)
    model.zero_grad()
    trainer = MatchTrainer(model, mode=2, optimizer_params={"lr": LR, "weight_decay": WD}, n_epoch=1, device="cpu")
    checked = CheckedBatches(batches, model)
    mean_loss = trainer.train_one_epoch(checked)
    gaps += checked.gaps
    assert len(checked.gaps) == 3
    out["train.lr"], out["train.wd"], out["train.mean_loss"] = np.array(LR), np.array(WD), np.array(mean_loss)
    out["min_gap"] = np.array(min(gaps))
    for n, t in model.state_dict().items():
        out["sd3." + n] = G.npy(t)
    return out, float(loss.item()), mean_loss


def chain(x_u, mask, w, C, g_v=None, up=None):
    """sine.py:93-128 on leaves of its own (float32 as the reference runs it), every intermediate kept; with g_v, the
    gradient of each as well.  The two halves are cut at (phi, xhat), where the fused path is cut by the w_4 GEMM, so that
    g_X / g_Y / g_a1 / g_a2 are the gradients with respect to the first half's own inputs.  The first half's backward is
    fed ``up`` = (up_g_phi, up_g_xhat), drawn for it: the g_phi / g_xhat that come out of the second half carry the
    1 / m_e^2 outliers of its p = -1 norm, under which the first half's float32 gradients are rounding noise."""
    keep = {}
    leaf = lambda t: t.detach().clone().requires_grad_(True)  # noqa: E731
    mf = mask.float()
    X = leaf(x_u)
    Y = leaf(x_u @ w["w_3"])
    a1 = leaf((torch.tanh(x_u @ w["w_1"]) @ w["w_2"]).squeeze(-1))
    a2 = leaf(torch.tanh(x_u @ w["w_k1"]) @ w["w_k2"])
    Cl = leaf(C)
    P1 = F.softmax(a1 + -1.e9 * (1 - mf), dim=1)
    z_u = torch.einsum("bse, bs -> be", X, P1)
    s_u = torch.einsum("be, te -> bt", z_u, Cl)
    top = torch.topk(s_u, a2.shape[2])
    c_u = torch.sigmoid(top.values).unsqueeze(-1) * Cl[top.indices]
    p_u = F.softmax(torch.einsum("bse, bke -> bks", F.normalize(Y, dim=-1), F.normalize(c_u, p=2, dim=-1)), dim=1)
    P2 = F.softmax(a2 + -1.e9 * (1 - mf.unsqueeze(-1)), dim=1)
    phi = torch.einsum("bks, bse -> bke", p_u * P2.permute(0, 2, 1), X)
    xhat = torch.einsum("bks, bke -> bse", p_u, c_u)
    xh, ph = leaf(xhat), leaf(phi)
    a3 = leaf((torch.tanh(xhat @ w["w_4"]) @ w["w_5"]).squeeze(-1))
    P3 = F.softmax(a3 + -1.e9 * (1 - mf), dim=1)
    c_apt = F.normalize(torch.einsum("bs, bse -> be", P3, xh), -1)  # (p = -1 over the last axis, as sine.py:122 has it)
    e_u = F.softmax(torch.einsum("be, bke -> bk", c_apt, ph) / TEMP, dim=1)
    v = torch.einsum("bk, bke -> be", e_u, ph)
    for name, t in (("X", X), ("Y", Y), ("a1", a1), ("a2", a2), ("C", Cl), ("P1", P1), ("z_u", z_u), ("s_u", s_u),
                    ("s_top", top.values), ("c_u", c_u), ("p_u", p_u), ("P2", P2), ("phi", phi), ("xhat", xhat), ("a3", a3),
                    ("P3", P3), ("c_apt", c_apt), ("e_u", e_u), ("v", v)):
        keep[name] = G.npy(t)
    keep["idx"] = top.indices.numpy().astype(np.int32)
    if g_v is not None:
        v.backward(g_v)
        torch.autograd.backward([phi, xhat], list(up))
        keep.update({"g_v": G.npy(g_v), "g_phi": G.npy(ph.grad), "g_xhat": G.npy(xh.grad), "g_a3": G.npy(a3.grad),
                     "up_g_phi": G.npy(up[0]), "up_g_xhat": G.npy(up[1]),
                     "g_X": G.npy(X.grad), "g_Y": G.npy(Y.grad), "g_a1": G.npy(a1.grad), "g_a2": G.npy(a2.grad),
                     "g_C": G.npy(Cl.grad)})
    return keep, s_u.detach()


def gen_layers(seed):
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed + 2)
    model = build()
    for m in model.modules():
        if isinstance(m, torch.nn.Embedding):
            torch.nn.init.normal_(m.weight, 0, 0.1, generator=g)
    B = 6
    hist = left_padded(B, g)
    hist[2, 3] = 0  # a hole inside the kept run
    mask = (hist > 0).long()
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    x_u = sd["item_embedding.weight"][hist] + sd["position_embedding.weight"].unsqueeze(0)
    g_v = torch.randn(B, E, generator=g)
    up = (torch.randn(B, K, E, generator=g), torch.randn(B, S, E, generator=g))
    keep, s_u = chain(x_u, mask, sd, sd["concept_embedding.weight"], g_v, up)
    gap = score_gap(s_u, K)
    if gap < MIN_GAP:
        raise GapTooSmall(f"layers: relative top-{K + 1} gap {gap:.2e} < {MIN_GAP}")
    model.mode = "user"
    with torch.no_grad():
        want = model({"hist_item_id": hist})
    np.testing.assert_allclose(keep["v"], want.numpy(), rtol=1e-5, atol=1e-7)  # the chain IS the reference's user tower
    out = {"hist": G.npy(hist), "mask": mask.numpy().astype(np.int32), "x_u": G.npy(x_u), "temperature": np.array(TEMP),
           "min_gap": np.array(gap), "seed": np.array(seed)}
    for k in ("w_1", "w_2", "w_3", "w_k1", "w_k2", "w_4", "w_5"):
        out[k] = G.npy(sd[k])
    out.update(keep)
    return out


def reseeding(fn, what):
    for attempt in range(64):
        try:
            return fn(G.SEED + 100 * attempt)
        except GapTooSmall as e:
            print(f"{what}: seed {G.SEED + 100 * attempt} rejected ({e})")
    raise RuntimeError(f"{what}: no seed with a top-k gap of {MIN_GAP}")


def main():
    import_reference()
    out, loss, mean_loss = reseeding(gen_model, "model_sine")
    _save_fixed(os.path.join(G.OUT, "model_sine.npz"), out)
    print("model_sine.npz", len(out), "arrays, seed", int(out["seed"]), "loss", loss, "mean train loss", mean_loss, "min gap",
          float(out["min_gap"]))
    layers = reseeding(gen_layers, "sine_layers")
    _save_fixed(os.path.join(G.OUT, "sine_layers.npz"), layers)
    print("sine_layers.npz", len(layers), "arrays, seed", int(layers["seed"]), "min gap", float(layers["min_gap"]))


if __name__ == "__main__":
    main()
