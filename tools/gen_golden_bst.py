"""Generate tests/golden/model_bst_l2.npz from the UNMODIFIED reference (CPU): BST with TWO encoder layers, so that the
all-rows path of ops.encoder_layer is pinned as well as the target-only one (model_bst.npz has one layer).

Run where the reference checkout exists:  ``python tools/gen_golden_bst.py``

The model is oracle/gen_golden.py's "bst" config with num_layers=2 and nhead=4 (item_dim 32, T = 7, max_seq_len 8, dropout
0), three batches of 48 whose odd samples are padded at the front and even ones at the back.  Same members as the other
model fixtures (spec, batches, sd0.*, predictions, loss, grad.*, train.*, sd3.*) with one difference that keeps the file
small: the reference fixes the feed-forward width at 2048, so the four (2048, 32) / (32, 2048) matrices would be 3 MiB.
Their INITIAL values are not stored: both sides draw them from torch.Generator().manual_seed(wide_seed + i) * wide_std in
the order of ``wide`` (a json list of state_dict names).  Their gradients and final values are stored for every 16th
hidden unit only (``[::16]`` along the 2048 axis).

The archive is written with a fixed member timestamp: the file regenerates byte-identically.
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

WIDE_SEED, WIDE_STD, EVERY = 7000, 0.05, 16


def wide_names(state):
    return [k for k, v in state.items() if v.dim() == 2 and 2048 in v.shape]


def draw_wide(state, names):
    """The seeded initial values of the 2048-wide matrices, in place."""
    for i, k in enumerate(names):
        g = torch.Generator().manual_seed(WIDE_SEED + i)
        state[k].copy_(WIDE_STD * torch.randn(state[k].shape, generator=g))


def thin(k, arr, names):
    """Every 16th hidden unit of a 2048-wide matrix; anything else whole."""
    if k not in names:
        return arr
    return arr[::EVERY] if arr.shape[0] == 2048 else arr[:, ::EVERY]


def main():
    import_reference()
    from torch_rechub.models.ranking import BST
    from torch_rechub.trainers import CTRTrainer
    torch.manual_seed(G.SEED)
    g = torch.Generator().manual_seed(G.SEED + 1)
    _, groups = G.build_model(None, "bst")
    model = BST(groups["features"], groups["history_features"], groups["target_features"],
                mlp_params={"dims": [32, 16], "dropout": 0.0, "activation": "relu"}, nhead=4, dropout=0.0, num_layers=2,
                max_seq_len=8)
    for m in model.modules():
        if isinstance(m, torch.nn.Embedding):
            torch.nn.init.normal_(m.weight, 0, 0.1, generator=g)
            if m.padding_idx is not None:
                with torch.no_grad():
                    m.weight[m.padding_idx].zero_()
    names = wide_names(model.state_dict())
    with torch.no_grad():
        draw_wide(model.state_dict(), names)
    batches = []
    for _ in range(3):
        x, y = G.make_batch(groups, 48, g)
        for f in groups["history_features"]:  # odd samples: the padding moves to the front
            x[f.name][1::2] = x[f.name][1::2].flip(1)
        batches.append((x, y))
    out = {"spec": np.array(json.dumps({k: [G.spec_of(f) for f in v] for k, v in groups.items()})), "cfg": np.array("bst_l2"),
           "wide": np.array(json.dumps(names)), "wide_seed": np.array(WIDE_SEED), "wide_std": np.array(WIDE_STD),
           "wide_every": np.array(EVERY)}
    for n, t in model.state_dict().items():
        if n not in names:
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
    backup = {k: v.clone() for k, v in model.state_dict().items()}
    pred = model(x)
    loss = torch.nn.BCELoss()(pred, y.float())
    model.zero_grad()
    loss.backward()
    out["pred_train"], out["loss"] = G.npy(pred), np.array(loss.item())
    for n, p in model.named_parameters():
        out["grad." + n] = thin(n, G.npy(p.grad), names)
    model.load_state_dict(backup)  # undo the BatchNorm running-stat update of the probe forward
    model.zero_grad()
    trainer = CTRTrainer(model, optimizer_params={"lr": 1e-2, "weight_decay": 1e-3}, n_epoch=1, device="cpu")
    mean_loss = trainer.train_one_epoch(batches)
    out["train.lr"], out["train.wd"], out["train.mean_loss"] = np.array(1e-2), np.array(1e-3), np.array(mean_loss)
    for n, t in model.state_dict().items():
        out["sd3." + n] = thin(n, G.npy(t), names)
    path = os.path.join(G.OUT, "model_bst_l2.npz")
    _save_fixed(path, out)
    print("model_bst_l2.npz", len(out), "arrays,", os.path.getsize(path), "bytes, loss", loss.item(), "mean train loss", mean_loss)


if __name__ == "__main__":
    main()
