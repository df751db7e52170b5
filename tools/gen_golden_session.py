"""Generate the session-based retrieval fixtures of tests/golden/ from the UNMODIFIED reference (CPU).

Run where the reference checkout exists:  ``python tools/gen_golden_session.py``

  model_session_<cfg>.npz  the seeded initial state_dict, three batches (B 6, L 7), the eval output of batch 0, the
                           training-mode output, loss and every parameter gradient on batch 0, then three
                           MatchTrainer.train_one_epoch steps (dropout 0, Adam, lr 1e-2, weight decay 1e-3) and the
                           state_dict after them.
  cfgs: narm (hidden 10) and stamp (mode 2, CrossEntropyLoss over the (B, V) scores, labels in [0, V) with a 0 among them),
        gru4rec (list-wise, K = 3 negatives, two bias-free GRU layers, user MLP [16, 12]), narm_inbatch (item_feature
        given, MatchTrainer(mode=0, in_batch_neg=True, hard_negative=True, in_batch_neg_ratio=3)).
Widths are odd on purpose (V 40, D 12, H 10, L 7).  Rows: full, short, with a zero inside the prefix, single item.
The archives are written with a fixed member timestamp: the files regenerate byte-identically.
"""
import json
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

CFGS = ["narm", "stamp", "gru4rec", "narm_inbatch"]
V, D, H, L, B, K = 40, 12, 10, 7, 6, 3
LR, WD = 1e-2, 1e-3


def build(cfg):
    from torch_rechub.basic.features import SequenceFeature, SparseFeature
    hist = SequenceFeature("hist_item_id", vocab_size=V, embed_dim=D, pooling="concat", shared_with="item_id")
    item = SparseFeature("item_id", vocab_size=V, embed_dim=D)
    if cfg == "narm":
        from torch_rechub.models.matching import NARM
        return NARM(hist, H, 0.0, 0.0), {"item_history_feature": [hist]}
    if cfg == "narm_inbatch":
        from torch_rechub.models.matching import NARM
        return NARM(hist, H, 0.0, 0.0, item_feature=item), {"item_history_feature": [hist], "item_feature": [item]}
    if cfg == "stamp":
        from torch_rechub.models.matching import STAMP
        return STAMP(hist, 0.05, 0.1), {"item_history_feature": [hist]}
    from torch_rechub.models.matching import GRU4Rec
    user = [SparseFeature("user_id", vocab_size=20, embed_dim=D), SparseFeature("age", vocab_size=7, embed_dim=D)]
    neg = [SequenceFeature("neg_items", vocab_size=V, embed_dim=D, pooling="concat", shared_with="item_id")]
    groups = {"user_features": user, "history_features": [hist], "item_features": [item], "neg_item_feature": neg}
    return GRU4Rec(user, [hist], [item], neg, user_params={"dims": [16, D]}), groups


def sessions(g):
    """(B, L) ids: row 0 full, row 1 short (3 items), row 2 a zero inside its prefix, row 3 one item, the rest random
    lengths; every batch holds a full row (NARM needs its longest prefix to reach L)."""
    seq = torch.randint(1, V, (B, L), generator=g)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0], lens[1], lens[2], lens[3] = L, 3, 5, 1
    seq[torch.arange(L)[None, :] >= lens[:, None]] = 0
    seq[2, 1] = 0
    return seq


def make_batch(cfg, g):
    x = {"hist_item_id": sessions(g)}
    if cfg == "gru4rec":
        x["user_id"] = torch.randint(0, 20, (B,), generator=g)
        x["age"] = torch.randint(0, 7, (B,), generator=g)
        x["item_id"] = torch.randint(1, V, (B,), generator=g)
        x["neg_items"] = torch.randint(1, V, (B, K), generator=g)
        return x, torch.zeros(B, dtype=torch.long)
    if cfg == "narm_inbatch":
        x["item_id"] = torch.randint(1, V, (B,), generator=g)
        return x, torch.ones(B, dtype=torch.long)
    y = torch.randint(0, V, (B,), generator=g)
    y[1] = 0  # label 0 is a class like any other
    return x, y


def gen(cfg):
    from torch_rechub.trainers import MatchTrainer
    torch.manual_seed(G.SEED)
    g = torch.Generator().manual_seed(G.SEED + 7)
    model, groups = build(cfg)
    batches = [make_batch(cfg, g) for _ in range(3)]
    out = {"cfg": np.array(cfg), "spec": np.array(json.dumps({k: [G.spec_of(f) for f in v] for k, v in groups.items()}))}
    for n, t in model.state_dict().items():
        out["sd0." + n] = G.npy(t)
    for bi, (bx, by) in enumerate(batches):
        for k, v in bx.items():
            out[f"x{bi}.{k}"] = G.npy(v)
        out[f"y{bi}"] = G.npy(by)
    x, y = batches[0]
    model.eval()
    with torch.no_grad():
        out["pred_eval"] = G.npy(model(x))
    model.train()
    sd_backup = {k: v.clone() for k, v in model.state_dict().items()}
    if cfg != "narm_inbatch":
        pred = model(x)
        loss = torch.nn.CrossEntropyLoss()(pred, y)
        model.zero_grad()
        loss.backward()
        out["pred_train"], out["loss"] = G.npy(pred), np.array(loss.item())
        for n, p in model.named_parameters():
            out["grad." + n] = G.npy(p.grad) if p.grad is not None else np.zeros(tuple(p.shape), np.float32)
    model.load_state_dict(sd_backup)
    model.zero_grad()
    if cfg == "narm_inbatch":
        trainer = MatchTrainer(model, mode=0, in_batch_neg=True, hard_negative=True, in_batch_neg_ratio=3,
                               optimizer_params={"lr": LR, "weight_decay": WD}, n_epoch=1, device="cpu")
    else:
        trainer = MatchTrainer(model, mode=2, optimizer_params={"lr": LR, "weight_decay": WD}, n_epoch=1, device="cpu")
    mean_loss = trainer.train_one_epoch(batches)
    out["train.lr"], out["train.wd"], out["train.mean_loss"] = np.array(LR), np.array(WD), np.array(mean_loss)
    for n, t in model.state_dict().items():
        out["sd3." + n] = G.npy(t)
    _save_fixed(os.path.join(G.OUT, f"model_session_{cfg}.npz"), out)
    print(f"model_session_{cfg}.npz", len(out), "arrays, mean train loss", mean_loss)


def main():
    import_reference()
    for cfg in CFGS:
        gen(cfg)


if __name__ == "__main__":
    main()
