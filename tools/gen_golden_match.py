"""Generate the list-wise retrieval fixtures of tests/golden/ from the UNMODIFIED reference (CPU).

Run where the reference checkout exists:  ``python tools/gen_golden_match.py``
Uses oracle/gen_golden.py's recipe (seed 2022, tables drawn N(0, 0.1), B = 48, three batches through the reference
``MatchTrainer(mode=2)``, list-wise softmax with the positive in column 0) by importing its constants and helpers.

  model_youtubednn.npz   YoutubeDNN, user tower MLP [32, 16], temperature 0.02
  model_mind.npz         MIND (capsule bilinear type 0), interest_num 4
  model_comirec_dr.npz   ComirecDR (capsule bilinear type 2; w drawn N(0, 0.3) before sd0 is saved)
  model_comirec_sa.npz   ComirecSA (self-attentive)
  interest_layers.npz    CapsuleNetwork (types 0 / 1 / 2, routing_times 1 / 3 / 4) and MultiInterestSA: inputs,
                         parameters, outputs, gradients; rows fully and partly padded

Features as in the reference's retrieval examples: user SparseFeatures, a concat-pooled history SequenceFeature of length
L = 8 shared with the item table (mask = his > 0, post padding), the item SparseFeature and a concat-pooled ``neg_items``
SequenceFeature (K = 3) shared with the item table.  MIND draws its initial routing logits with torch.randn inside every
forward; those draws are recorded in call order (``routing_draws``: eval forward, user-mode forward, probe forward, three training steps) so
a test can replay them.  The archives are written with a fixed member timestamp: the files regenerate byte-identically.
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

MODELS = ["youtubednn", "mind", "comirec_dr", "comirec_sa"]
L, K, D, N_ITEMS = 8, 3, 16, 60


def build_match_model(cfg):
    from torch_rechub.basic.features import SequenceFeature, SparseFeature
    user = [SparseFeature("user_id", vocab_size=40, embed_dim=D), SparseFeature("gender", vocab_size=3, embed_dim=D),
            SparseFeature("age", vocab_size=7, embed_dim=D)]
    hist = [SequenceFeature("hist_item_id", vocab_size=N_ITEMS, embed_dim=D, pooling="concat", shared_with="item_id")]
    item = [SparseFeature("item_id", vocab_size=N_ITEMS, embed_dim=D)]
    neg = [SequenceFeature("neg_items", vocab_size=N_ITEMS, embed_dim=D, pooling="concat", shared_with="item_id")]
    if cfg == "youtubednn":
        from torch_rechub.models.matching import YoutubeDNN
        user_yt = user + [SequenceFeature("hist_item_id", vocab_size=N_ITEMS, embed_dim=D, pooling="mean",
                                          shared_with="item_id")]
        model = YoutubeDNN(user_yt, item, neg, user_params={"dims": [32, 16]}, temperature=0.02)
        return model, {"user_features": user_yt, "item_features": item, "neg_item_feature": neg}
    groups = {"user_features": user, "history_features": hist, "item_features": item, "neg_item_feature": neg}
    if cfg == "mind":
        from torch_rechub.models.matching import MIND
        return MIND(user, hist, item, neg, max_length=L, temperature=0.02), groups
    if cfg == "comirec_dr":
        from torch_rechub.models.matching import ComirecDR
        return ComirecDR(user, hist, item, neg, max_length=L, temperature=0.02), groups
    from torch_rechub.models.matching import ComirecSA
    return ComirecSA(user, hist, item, neg, temperature=0.02), groups


def make_batch(B, g):
    """User ids, a post-padded history (row 0 fully padded, row 1 full, the rest of random length), the positive and K
    negatives (never the padding id 0)."""
    x = {"user_id": torch.randint(0, 40, (B,), generator=g), "gender": torch.randint(0, 3, (B,), generator=g),
         "age": torch.randint(0, 7, (B,), generator=g)}
    hist = torch.randint(1, N_ITEMS, (B, L), generator=g)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0], lens[1] = 0, L
    hist[torch.arange(L)[None, :] >= lens[:, None]] = 0
    x["hist_item_id"] = hist
    x["item_id"] = torch.randint(1, N_ITEMS, (B,), generator=g)
    x["neg_items"] = torch.randint(1, N_ITEMS, (B, K), generator=g)
    return x, torch.zeros(B, dtype=torch.long)


class RecordRandn(object):
    """Records every torch.randn draw (MIND's initial routing logits) without changing the random stream."""

    def __init__(self):
        self.draws = []
        self.orig = torch.randn

    def __enter__(self):
        def randn(*a, **kw):
            t = self.orig(*a, **kw)
            self.draws.append(G.npy(t))
            return t
        torch.randn = randn
        return self

    def __exit__(self, *exc):
        torch.randn = self.orig


def gen_model(cfg):
    from torch_rechub.trainers import MatchTrainer
    torch.manual_seed(G.SEED)
    g = torch.Generator().manual_seed(G.SEED + 1)
    model, groups = build_match_model(cfg)
    for m in model.modules():
        if isinstance(m, torch.nn.Embedding):
            torch.nn.init.normal_(m.weight, 0, 0.1, generator=g)
    if cfg == "comirec_dr":  # the reference leaves w uninitialised (torch.Tensor(...)); a seeded draw makes it defined
        with torch.no_grad():
            model.capsule.w.normal_(0, 0.3, generator=g)
    B = 48
    batches = [make_batch(B, g) for _ in range(3)]
    out = {"spec": np.array(json.dumps({k: [G.spec_of(f) for f in v] for k, v in groups.items()})), "cfg": np.array(cfg)}
    for n, t in model.state_dict().items():
        out["sd0." + n] = G.npy(t)
    for bi, (bx, by) in enumerate(batches):
        for k, v in bx.items():
            out[f"x{bi}.{k}"] = G.npy(v)
        out[f"y{bi}"] = G.npy(by)
    x, y = batches[0]
    with RecordRandn() as rec:
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
        model.load_state_dict(sd_backup)  # undo the BatchNorm running-stat update of the probe forward
        model.zero_grad()
        wd = 1e-3
        trainer = MatchTrainer(model, mode=2, optimizer_params={"lr": 1e-2, "weight_decay": wd}, n_epoch=1, device="cpu")
        mean_loss = trainer.train_one_epoch(batches)
    if rec.draws:  # eval forward, user-mode forward, probe forward, three training steps
        out["routing_draws"] = np.stack(rec.draws)
    out["train.lr"], out["train.wd"], out["train.mean_loss"] = np.array(1e-2), np.array(wd), np.array(mean_loss)
    for n, t in model.state_dict().items():
        out["sd3." + n] = G.npy(t)
    _save_fixed(os.path.join(G.OUT, f"model_{cfg}.npz"), out)
    print(f"model_{cfg}.npz", len(out), "arrays, loss", loss.item(), "mean train loss", mean_loss)


def gen_interest_layers():
    from torch_rechub.basic.layers import CapsuleNetwork, MultiInterestSA
    torch.manual_seed(G.SEED)
    g = torch.Generator().manual_seed(G.SEED)
    out = {}
    B, Lc = 6, 8
    lens = torch.tensor([0, Lc, 3, 1, 5, Lc])  # fully padded, full, partly padded rows
    mask = (torch.arange(Lc)[None, :] < lens[:, None]).long()
    out["mask"] = G.npy(mask)
    for kind in (0, 1, 2):
        for rt in (1, 3, 4):
            I = 3 if kind == 1 else 4
            caps = CapsuleNetwork(D, Lc, bilinear_type=kind, interest_num=I, routing_times=rt)
            if kind == 2:
                with torch.no_grad():
                    caps.w.normal_(0, 0.3, generator=g)
            e = (0.5 * torch.randn(B, Lc, D, generator=g)).requires_grad_(True)
            with RecordRandn() as rec:
                y = caps(e, mask)
            k = f"caps{kind}_rt{rt}."
            gy = torch.randn(y.shape, generator=g)
            if y.requires_grad:
                y.backward(gy)
            out[k + "e"], out[k + "out"], out[k + "g_out"] = G.npy(e), G.npy(y), G.npy(gy)
            out[k + "g_e"] = G.npy(e.grad) if e.grad is not None else np.zeros(tuple(e.shape), np.float32)
            if rec.draws:
                out[k + "init"] = rec.draws[0]
            for n, t in caps.state_dict().items():
                out[k + "sd." + n] = G.npy(t)
            for n, p in caps.named_parameters():
                if p.grad is not None:
                    out[k + "grad." + n] = G.npy(p.grad)
    sa = MultiInterestSA(D, 4)
    e = (0.5 * torch.randn(B, Lc, D, generator=g)).requires_grad_(True)
    y = sa(e, mask.unsqueeze(-1).float())
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    out["sa.e"], out["sa.out"], out["sa.g_out"], out["sa.g_e"] = G.npy(e), G.npy(y), G.npy(gy), G.npy(e.grad)
    for n, t in sa.state_dict().items():
        out["sa.sd." + n] = G.npy(t)
    for n, p in sa.named_parameters():
        if p.grad is not None:
            out["sa.grad." + n] = G.npy(p.grad)
    return out


def main():
    import_reference()
    for cfg in MODELS:
        gen_model(cfg)
    _save_fixed(os.path.join(G.OUT, "interest_layers.npz"), gen_interest_layers())
    print("interest_layers.npz")


if __name__ == "__main__":
    main()
