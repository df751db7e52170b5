"""Generate the two-tower fixtures of tests/golden/ from the UNMODIFIED reference (CPU).

Run where the reference checkout exists:  ``python tools/gen_golden_twotower.py``
Uses oracle/gen_golden.py's recipe (seed 2022, tables drawn N(0, 0.1), B = 48, three Adam steps through the reference's
``MatchTrainer``) by importing its constants and helpers.

  model_facebook_dssm.npz  FaceBookDSSM, towers [32, 16], MatchTrainer(mode=1) (BPRLoss on (pos_score, neg_score))
  model_youtube_sbc.npz    YoutubeSBC, batch_size 48, n_neg 3, temperature 0.2, sample_weight in [0.05, 1],
                           MatchTrainer(mode=2); after the three steps a SHORT batch of 10 rows and one more full batch
                           (``x3.*``, ``x4.*``): their losses (``loss_step3``, ``loss_step4``), the model's index arrays
                           after the short batch (``index0_after``, ``index1_after``) and the state after five steps (``sd5.*``)
  model_dssm_senet.npz     the SENet DSSM (models/matching/dssm_senet.py), 6 user fields (one a mean-pooled sequence that
                           owns its table) and 2 item fields, temperature 0.25, MatchTrainer(mode=0) (BCELoss)
  twotower_layers.npz      SENETLayer, YoutubeSBC's score tail and FaceBookDSSM's score tail in isolation (inputs,
                           parameters, outputs, gradients; zero rows and rows whose norm is below eps) and HingeLoss values

Each model file: feature spec, initial state (``sd0.*``), batches (``x{i}.*``, ``y{i}``), eval outputs, both tower modes, a
probe loss with gradients, the state after three steps (``sd3.*``).  The archives are written with a fixed member timestamp:
the files regenerate byte-identically.
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

MODELS = ["facebook_dssm", "youtube_sbc", "dssm_senet"]
D, N_ITEMS, N_CATE, L = 16, 60, 9, 6
B, B_SHORT, N_NEG = 48, 10, 3
TRAIN_MODE = {"facebook_dssm": 1, "youtube_sbc": 2, "dssm_senet": 0}


def build_model(cfg):
    from torch_rechub.basic.features import DenseFeature, SequenceFeature, SparseFeature
    user = [SparseFeature("user_id", vocab_size=40, embed_dim=D), SparseFeature("gender", vocab_size=3, embed_dim=D),
            SparseFeature("age", vocab_size=7, embed_dim=D)]
    item = [SparseFeature("item_id", vocab_size=N_ITEMS, embed_dim=D), SparseFeature("cate_id", vocab_size=N_CATE, embed_dim=D)]
    tower = {"dims": [32, 16]}
    if cfg == "facebook_dssm":
        from torch_rechub.models.matching import FaceBookDSSM
        neg = [SparseFeature("neg_item_id", vocab_size=N_ITEMS, embed_dim=D, shared_with="item_id"),
               SparseFeature("neg_cate_id", vocab_size=N_CATE, embed_dim=D, shared_with="cate_id")]
        model = FaceBookDSSM(user, item, neg, user_params=dict(tower), item_params=dict(tower), temperature=0.02)
        return model, {"user_features": user, "pos_item_features": item, "neg_item_features": neg}
    if cfg == "youtube_sbc":
        from torch_rechub.models.matching import YoutubeSBC
        weight = [DenseFeature("sample_weight")]
        model = YoutubeSBC(user, item, weight, user_params=dict(tower), item_params=dict(tower), batch_size=B, n_neg=N_NEG,
                           temperature=0.2)
        return model, {"user_features": user, "item_features": item, "sample_weight_feature": weight}
    from torch_rechub.models.matching.dssm_senet import DSSM
    user6 = user + [SparseFeature("occupation", vocab_size=21, embed_dim=D), SparseFeature("zip", vocab_size=50, embed_dim=D),
                    SequenceFeature("hist_cate_id", vocab_size=N_CATE, embed_dim=D, pooling="mean")]
    tower = {"dims": [32, 16], "activation": "prelu"}
    model = DSSM(user6, item, user_params=dict(tower), item_params=dict(tower), temperature=0.25)
    return model, {"user_features": user6, "item_features": item}


def make_batch(cfg, n, g):
    x = {"user_id": torch.randint(0, 40, (n,), generator=g), "gender": torch.randint(0, 3, (n,), generator=g),
         "age": torch.randint(0, 7, (n,), generator=g), "item_id": torch.randint(0, N_ITEMS, (n,), generator=g),
         "cate_id": torch.randint(0, N_CATE, (n,), generator=g)}
    y = torch.zeros(n, dtype=torch.long)
    if cfg == "facebook_dssm":
        x["neg_item_id"] = torch.randint(0, N_ITEMS, (n,), generator=g)
        x["neg_cate_id"] = torch.randint(0, N_CATE, (n,), generator=g)
    elif cfg == "youtube_sbc":
        x["sample_weight"] = 0.05 + 0.95 * torch.rand(n, generator=g)
    else:
        x["occupation"] = torch.randint(0, 21, (n,), generator=g)
        x["zip"] = torch.randint(0, 50, (n,), generator=g)
        x["hist_cate_id"] = torch.randint(0, N_CATE, (n, L), generator=g)
        y = (torch.rand(n, generator=g) < 0.4).long()
    return x, y


def probe_loss(cfg, pred, y):
    if cfg == "facebook_dssm":
        from torch_rechub.basic.loss_func import BPRLoss
        return BPRLoss()(pred[0], pred[1])
    if cfg == "youtube_sbc":
        return torch.nn.CrossEntropyLoss()(pred, y)
    return torch.nn.BCELoss()(pred, y.float())


def put_pred(out, key, pred):
    if isinstance(pred, tuple):
        out[key + "_pos"], out[key + "_neg"] = G.npy(pred[0]), G.npy(pred[1])
    else:
        out[key] = G.npy(pred)


def gen_model(cfg):
    from torch_rechub.trainers import MatchTrainer
    torch.manual_seed(G.SEED)
    g = torch.Generator().manual_seed(G.SEED + 1)
    model, groups = build_model(cfg)
    for m in model.modules():
        if isinstance(m, torch.nn.Embedding):
            torch.nn.init.normal_(m.weight, 0, 0.1, generator=g)
    if cfg == "dssm_senet":
        # nn.Linear's default draw leaves the gates near 0.005 on N(0, 0.1) tables: the towers' first BatchNorm then divides
        # by a batch deviation of ~1e-3 and fp32 noise decides the recorded gradients.  A seeded wider draw opens the gates
        # to O(1) (about half of them, and a quarter of the hidden units, stay closed: both ReLU branches are taken).
        with torch.no_grad():
            for senet in (model.user_senet, model.item_senet):
                senet.mlp[0].weight.normal_(0, 4.0, generator=g)
                senet.mlp[2].weight.normal_(0, 4.0, generator=g)
    sizes = [B, B, B] + ([B_SHORT, B] if cfg == "youtube_sbc" else [])
    batches = [make_batch(cfg, n, g) for n in sizes]
    out = {"spec": np.array(json.dumps({k: [G.spec_of(f) for f in v] for k, v in groups.items()})), "cfg": np.array(cfg)}
    for n, t in model.state_dict().items():
        out["sd0." + n] = G.npy(t)
    for bi, (bx, by) in enumerate(batches):
        for k, v in bx.items():
            out[f"x{bi}.{k}"] = G.npy(v)
        out[f"y{bi}"] = G.npy(by)
    x, y = batches[0]
    model.eval()
    with torch.no_grad():
        put_pred(out, "pred_eval", model(x))
        model.mode = "user"
        out["user_emb"] = G.npy(model(x))
        model.mode = "item"
        out["item_emb"] = G.npy(model(x))
        model.mode = None
    model.train()
    sd_backup = {k: v.clone() for k, v in model.state_dict().items()}
    pred = model(x)
    loss = probe_loss(cfg, pred, y)
    model.zero_grad()
    loss.backward()
    put_pred(out, "pred_train", pred)
    out["loss"] = np.array(loss.item())
    for n, p in model.named_parameters():
        out["grad." + n] = G.npy(p.grad) if p.grad is not None else np.zeros(tuple(p.shape), np.float32)
    model.load_state_dict(sd_backup)  # undo the BatchNorm running-stat update of the probe forward
    model.zero_grad()
    wd = 1e-3
    trainer = MatchTrainer(model, mode=TRAIN_MODE[cfg], optimizer_params={"lr": 1e-2, "weight_decay": wd}, n_epoch=1,
                           device="cpu")
    mean_loss = trainer.train_one_epoch(batches[:3])
    out["train.lr"], out["train.wd"], out["train.mean_loss"] = np.array(1e-2), np.array(wd), np.array(mean_loss)
    for n, t in model.state_dict().items():
        out["sd3." + n] = G.npy(t)
    if cfg == "youtube_sbc":
        out["index0_before"], out["index1_before"] = model.index0.copy(), model.index1.copy()
        out["loss_step3"] = np.array(trainer.train_one_epoch(batches[3:4]))  # the short batch: rewrites the index arrays
        out["index0_after"], out["index1_after"] = model.index0.copy(), model.index1.copy()
        out["loss_step4"] = np.array(trainer.train_one_epoch(batches[4:5]))  # a full batch on the rewritten arrays
        with torch.no_grad():
            model.eval()
            out["pred_eval_after"] = G.npy(model(batches[4][0]))
        for n, t in model.state_dict().items():
            out["sd5." + n] = G.npy(t)
    _save_fixed(os.path.join(G.OUT, f"model_{cfg}.npz"), out)
    print(f"model_{cfg}.npz", len(out), "arrays, loss", loss.item(), "mean train loss", mean_loss)


def _clamp_rows(t, g):
    """Row 0 exactly zero, row 2 of norm 1e-9 (below cosine_similarity's eps = 1e-8; above F.normalize's 1e-12)."""
    with torch.no_grad():
        t[0] = 0
        t[2] *= 1e-9 / t[2].norm()
    return t


def gen_layers():
    from torch_rechub.basic.layers import SENETLayer
    from torch_rechub.basic.loss_func import HingeLoss
    torch.manual_seed(G.SEED)
    g = torch.Generator().manual_seed(G.SEED)
    out = {}
    for ci, (F_, ratio, Dd) in enumerate([(3, 3, 16), (7, 3, 16), (6, 2, 4), (1, 3, 1)]):
        layer = SENETLayer(F_, reduction_ratio=ratio)
        with torch.no_grad():  # both signs at the hidden units and the gates, so both ReLU branches are taken
            for lin in (layer.mlp[0], layer.mlp[2]):
                lin.weight.normal_(0.2, 0.6, generator=g)
        x = torch.randn(5, F_, Dd, generator=g)
        x[0] = 0  # z = 0: hidden units and gates exactly 0 (ReLU's derivative at 0)
        x.requires_grad_(True)
        y = layer(x)
        gy = torch.randn(y.shape, generator=g)
        y.backward(gy)
        k = f"senet{ci}."
        out[k + "x"], out[k + "out"], out[k + "g_out"], out[k + "g_x"] = G.npy(x), G.npy(y), G.npy(gy), G.npy(x.grad)
        out[k + "w1"], out[k + "w2"] = G.npy(layer.mlp[0].weight), G.npy(layer.mlp[2].weight)
        out[k + "g_w1"], out[k + "g_w2"] = G.npy(layer.mlp[0].weight.grad), G.npy(layer.mlp[2].weight.grad)
    # YoutubeSBC's tail (youtube_sbc.py:61-80) on given tower outputs
    for name, n, d, n_neg, temp, clamp in (("band0", 7, 5, 2, 0.5, False), ("band1", 6, 5, 3, 0.2, True), ("band2", 1, 3, 0, 1.0, False)):
        u, v = torch.randn(n, d, generator=g), torch.randn(n, d, generator=g)
        if clamp:
            u = _clamp_rows(u, g)
            v = _clamp_rows(v.flip(0), g).flip(0).contiguous()  # v: row n-1 zero, row n-3 tiny
        w = 0.05 + 0.95 * torch.rand(n, generator=g)
        u.requires_grad_(True), v.requires_grad_(True)
        index0 = np.repeat(np.arange(n), n_neg + 1)
        index1 = np.concatenate([np.arange(i, i + n_neg + 1) for i in range(n)]) % n
        pred = torch.cosine_similarity(u.unsqueeze(1), v, dim=2)
        scores = ((pred - torch.log(w))[index0, index1] / temp).view(-1, n_neg + 1)
        gs = torch.randn(scores.shape, generator=g)
        scores.backward(gs)
        k = name + "."
        out[k + "u"], out[k + "v"], out[k + "w"], out[k + "logits"] = G.npy(u), G.npy(v), G.npy(w), G.npy(scores)
        out[k + "g"], out[k + "g_u"], out[k + "g_v"] = G.npy(gs), G.npy(u.grad), G.npy(v.grad)
        out[k + "n_neg"], out[k + "temperature"] = np.array(n_neg), np.array(temp)
    # FaceBookDSSM's tail (dssm_facebook.py:52-53,64,75-76) on given tower outputs
    import torch.nn.functional as F
    for name, clamp in (("pair0", False), ("pair1", True)):
        hs = [torch.randn(6, 5, generator=g) for _ in range(3)]
        if clamp:
            with torch.no_grad():
                hs[0][0] = 0
                hs[1][1] = 0
                hs[2][2] = 0
                hs[0][3] *= 1e-13 / hs[0][3].norm()  # below F.normalize's eps = 1e-12
        for h in hs:
            h.requires_grad_(True)
        nu, np_, nn_ = (F.normalize(h, p=2, dim=1) for h in hs)
        pos, neg = torch.mul(nu, np_).sum(dim=1), torch.mul(nu, nn_).sum(dim=1)
        gp, gn = torch.randn(6, generator=g), torch.randn(6, generator=g)
        torch.autograd.backward([pos, neg], [gp, gn])
        k = name + "."
        for nm, h in zip(("hu", "hp", "hn"), hs):
            out[k + nm], out[k + "g_" + nm] = G.npy(h), G.npy(h.grad)
        out[k + "pos"], out[k + "neg"], out[k + "g_pos"], out[k + "g_neg"] = G.npy(pos), G.npy(neg), G.npy(gp), G.npy(gn)
    pos, neg2, neg1 = torch.randn(8, generator=g), torch.randn(8, 3, generator=g), torch.randn(8, generator=g)
    out["hinge.pos"], out["hinge.neg2d"], out["hinge.neg1d"] = G.npy(pos), G.npy(neg2), G.npy(neg1)
    out["hinge.loss2d"] = G.npy(HingeLoss()(pos, neg2))
    out["hinge.loss1d"] = G.npy(HingeLoss()(pos, neg1))
    out["hinge.loss2d_margin"] = G.npy(HingeLoss(margin=0.5)(pos, neg2))
    return out


def main():
    import_reference()
    for cfg in MODELS:
        gen_model(cfg)
    _save_fixed(os.path.join(G.OUT, "twotower_layers.npz"), gen_layers())
    print("twotower_layers.npz")


if __name__ == "__main__":
    main()
