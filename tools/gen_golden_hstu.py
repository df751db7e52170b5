"""Generate the HSTU fixtures of tests/golden/ from the UNMODIFIED reference (CPU).

Run where the reference checkout exists:  ``python tools/gen_golden_hstu.py``

  hstu_layers.npz     RelativeBucketedTimeAndPositionBias (dense bias), HSTULayer and HSTUBlock: inputs, parameters,
                      outputs and every gradient.  d_model 24, H 2, dqk 12, dv 10 (dqk != dv, neither a multiple of 16),
                      max_seq_len 12, L 10, 16 time buckets; without time_diffs, sqrt / minutes / 1.0 and log / seconds /
                      0.301; rows left-padded, right-padded, empty and full.
  model_hstu_<cfg>.npz HSTUModel (2 layers, V 40): the eval logits of batch 0, the next-token loss of batch 0 and every
                      parameter gradient, three SeqTrainer.train_one_epoch steps (dropout 0, Adam) and the evaluate
                      result after them.  cfgs: tied / untied head, score_norm none / l2, temperature != 1, with and
                      without the output bias, loss_type cross_entropy and nce.

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

DM, H, DQK, DV, N, L, NB = 24, 2, 12, 10, 12, 10, 16
LAYER_CFGS = {"none": None, "sqrt_min": ("sqrt", 1.0, "minutes"), "log_sec": ("log", 0.301, "seconds")}
MODEL_CFGS = {
    "tied_l2_ce": dict(tie_embeddings=True, score_norm="l2", temperature=0.05, use_output_bias=True,
                       time_bucket_fn="log", time_bucket_divisor=0.301, time_bucket_unit="seconds", loss_type="cross_entropy"),
    "untied_none_nce": dict(tie_embeddings=False, score_norm="none", temperature=1.0, use_output_bias=False,
                            time_bucket_fn="sqrt", time_bucket_divisor=1.0, time_bucket_unit="minutes", loss_type="nce"),
    "tied_none_t2_nobias_ce": dict(tie_embeddings=True, score_norm="none", temperature=2.0, use_output_bias=False,
                                   time_bucket_fn="sqrt", time_bucket_divisor=1.0, time_bucket_unit="minutes",
                                   loss_type="cross_entropy"),
    "untied_l2_bias_nce": dict(tie_embeddings=False, score_norm="l2", temperature=0.5, use_output_bias=True,
                               time_bucket_fn="log", time_bucket_divisor=0.301, time_bucket_unit="seconds", loss_type="nce"),
}
V, B, LR, WD = 40, 6, 1e-2, 1e-5


def padding_rows(Bn, g):
    """(Bn, L) bool: row 0 empty, row 1 full, row 2 left-padded, row 3 right-padded, the rest random lengths either way."""
    mask = torch.ones(Bn, L, dtype=torch.bool)
    mask[0] = False
    mask[2, :4] = False
    mask[3, 6:] = False
    for b in range(4, Bn):
        n = int(torch.randint(1, L + 1, (1,), generator=g))
        mask[b] = torch.arange(L) >= L - n if b % 2 else torch.arange(L) < n
    return mask


def anchored_times(Bn, g):
    """Per-position seconds from a single anchor (non-increasing along the sequence, as the examples' preprocessing)."""
    return torch.sort(torch.randint(0, 3 * 10**6, (Bn, L), generator=g), 1, descending=True).values


def gen_layers():
    from torch_rechub.basic.layers import HSTUBlock, HSTULayer
    from torch_rechub.utils.hstu_utils import RelativeBucketedTimeAndPositionBias
    torch.manual_seed(G.SEED)
    g = torch.Generator().manual_seed(G.SEED)
    out = {}
    Bn = 7
    mask = padding_rows(Bn, g)
    td = anchored_times(Bn, g)
    out["mask"], out["time_diffs"] = G.npy(mask), G.npy(td)
    for name, tb in LAYER_CFGS.items():
        fn, div, unit = tb or ("sqrt", 1.0, "minutes")
        kw = dict(num_time_buckets=NB, time_bucket_fn=fn, time_bucket_divisor=div, time_bucket_unit=unit)
        for kind in ("layer", "block"):
            m = (HSTULayer(DM, H, DQK, DV, 0.0, N, **kw) if kind == "layer" else
                 HSTUBlock(DM, H, 2, DQK, DV, 0.0, N, **kw))
            with torch.no_grad():  # biases and LayerNorm affine away from their zero / one init
                for n, p in m.named_parameters():
                    if p.dim() == 1:
                        p.add_(0.1 * torch.randn(p.shape, generator=g))
            x = torch.randn(Bn, L, DM, generator=g).requires_grad_(True)
            y = m(x, padding_mask=mask, time_diffs=td if tb else None)
            gy = torch.randn(y.shape, generator=g)
            y.backward(gy)
            k = f"{kind}.{name}."
            out[k + "x"], out[k + "out"], out[k + "g_out"], out[k + "g_x"] = G.npy(x), G.npy(y), G.npy(gy), G.npy(x.grad)
            for n, t in m.state_dict().items():
                out[k + "sd." + n] = G.npy(t)
            for n, p in m.named_parameters():
                out[k + "grad." + n] = G.npy(p.grad) if p.grad is not None else np.zeros(tuple(p.shape), np.float32)
    rab = RelativeBucketedTimeAndPositionBias(H, N, NB, "log", 0.301, "seconds")
    out["rab.pos_w"], out["rab.ts_w"] = G.npy(rab.pos_w), G.npy(rab.ts_w)
    out["rab.bias_time"] = G.npy(rab(time_diffs=td))
    out["rab.bias_pos"] = G.npy(rab(seq_len=L))
    return out


def make_batch(g):
    mask = padding_rows(B, g)
    tok = torch.randint(1, V, (B, L), generator=g) * mask
    pos = torch.arange(L).repeat(B, 1)
    return tok, pos, anchored_times(B, g) * mask, torch.randint(1, V, (B,), generator=g)


def gen_model(cfg):
    from torch_rechub.models.generative.hstu import HSTUModel
    from torch_rechub.trainers.seq_trainer import SeqTrainer
    kw = dict(MODEL_CFGS[cfg])
    loss_type = kw.pop("loss_type")
    torch.manual_seed(G.SEED)
    g = torch.Generator().manual_seed(G.SEED + 1)
    model = HSTUModel(V, d_model=DM, n_heads=H, n_layers=2, dqk=DQK, dv=DV, max_seq_len=N, dropout=0.0,
                      num_time_buckets=NB, **kw)
    batches = [make_batch(g) for _ in range(3)]
    out = {"cfg": np.array(json.dumps(dict(MODEL_CFGS[cfg]))), "sd_keys": np.array(list(model.state_dict()))}
    for n, t in model.state_dict().items():
        out["sd0." + n] = G.npy(t)
    for bi, (tok, pos, td, tg) in enumerate(batches):
        out[f"b{bi}.tokens"], out[f"b{bi}.positions"], out[f"b{bi}.time_diffs"], out[f"b{bi}.targets"] = (
            G.npy(tok), G.npy(pos), G.npy(td), G.npy(tg))
    trainer = SeqTrainer(model, optimizer_params={"lr": LR, "weight_decay": WD}, device="cpu", loss_type=loss_type)
    tok, _, td, tg = batches[0]
    model.eval()
    with torch.no_grad():
        out["logits"] = G.npy(model(tok, td))
    model.train()
    loss = trainer._compute_next_token_loss(model(tok, td), tok, tg)
    model.zero_grad()
    loss.backward()
    out["loss"] = np.array(loss.item())
    for n, p in model.named_parameters():
        out["grad." + n] = G.npy(p.grad) if p.grad is not None else np.zeros(tuple(p.shape), np.float32)
    model.zero_grad()
    mean_loss = trainer.train_one_epoch(batches)
    out["train.lr"], out["train.wd"], out["train.mean_loss"] = np.array(LR), np.array(WD), np.array(mean_loss)
    for n, t in model.state_dict().items():
        out["sd3." + n] = G.npy(t)
    ev_loss, ev_acc = trainer.evaluate(batches)
    out["eval.loss"], out["eval.accuracy"] = np.array(ev_loss), np.array(ev_acc)
    _save_fixed(os.path.join(G.OUT, f"model_hstu_{cfg}.npz"), out)
    print(f"model_hstu_{cfg}.npz", len(out), "arrays, loss", loss.item(), "mean train loss", mean_loss, "eval", ev_loss, ev_acc)


def main():
    import_reference()
    _save_fixed(os.path.join(G.OUT, "hstu_layers.npz"), gen_layers())
    print("hstu_layers.npz")
    for cfg in MODEL_CFGS:
        gen_model(cfg)


if __name__ == "__main__":
    main()
