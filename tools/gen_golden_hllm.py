"""Generate the HLLM fixtures of tests/golden/ from the UNMODIFIED reference (CPU).

Run where the reference checkout exists:  ``python tools/gen_golden_hllm.py``

  hllm_layers.npz      RelPosBias.forward (several (max_seq_len, num_buckets, L)), and HLLMTransformerBlock with and
                       without the bias at head widths 4, 5 and 7: input, parameters, output and every gradient (input,
                       parameters, bias table), dropout 0.
  model_hllm_<cfg>.npz HLLMModel (2 layers, V 23, L 7, max_seq_len 9, 16 time buckets): the seeded state_dict, three
                       batches, the eval logits, training logits, next-token loss and every gradient of batch 0, three
                       SeqTrainer.train_one_epoch steps (dropout 0, Adam lr 1e-2, weight decay 1e-3) and the state after
                       them.  cfgs: bias_time_ce (D 12, H 3), nobias_notime_nce (D 12, H 3), odd_bias_time_nce (D 15, H 3:
                       head width 5, log time buckets).  Rows with PAD at the front, PAD at the back, and full rows.

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

V, B, L, N, NB, LR, WD = 23, 6, 7, 9, 16, 1e-2, 1e-3
BLOCK_CFGS = {"d12h3_bias": (12, 3, True), "d12h3_nobias": (12, 3, False), "d15h3_bias": (15, 3, True),
              "d14h2_bias": (14, 2, True)}
RELPOS_CFGS = ((9, 32, 7), (9, 4, 9), (5, 1, 5), (40, 7, 33))  # (max_seq_len, num_buckets, L)
MODEL_CFGS = {
    "bias_time_ce": dict(d_model=12, n_heads=3, use_rel_pos_bias=True, use_time_embedding=True, time_bucket_fn="sqrt",
                         temperature=0.5, loss_type="cross_entropy"),
    "nobias_notime_nce": dict(d_model=12, n_heads=3, use_rel_pos_bias=False, use_time_embedding=False,
                              time_bucket_fn="sqrt", temperature=1.0, loss_type="nce"),
    "odd_bias_time_nce": dict(d_model=15, n_heads=3, use_rel_pos_bias=True, use_time_embedding=True, time_bucket_fn="log",
                              temperature=0.3, loss_type="nce"),
}


def gen_layers():
    from torch_rechub.models.generative.hllm import HLLMTransformerBlock
    from torch_rechub.utils.hstu_utils import RelPosBias
    torch.manual_seed(G.SEED)
    g = torch.Generator().manual_seed(G.SEED)
    out = {"relpos.cfgs": np.array(RELPOS_CFGS), "block.cfgs": np.array(json.dumps(BLOCK_CFGS))}
    for n, nb, length in RELPOS_CFGS:
        m = RelPosBias(2, n, nb)
        out[f"relpos.{n}_{nb}_{length}.table"] = G.npy(m.rel_pos_bias_table)
        out[f"relpos.{n}_{nb}_{length}.bias"] = G.npy(m(length))
    for name, (dm, h, with_bias) in BLOCK_CFGS.items():
        m = HLLMTransformerBlock(dm, h, 0.0)
        rp = RelPosBias(h, N, 8) if with_bias else None
        with torch.no_grad():  # biases and LayerNorm affine away from their zero / one init
            for _, p in m.named_parameters():
                if p.dim() == 1:
                    p.add_(0.1 * torch.randn(p.shape, generator=g))
        x = torch.randn(5, L, dm, generator=g).requires_grad_(True)
        y = m(x, rel_pos_bias=rp(L) if with_bias else None)
        gy = torch.randn(y.shape, generator=g)
        y.backward(gy)
        k = f"block.{name}."
        out[k + "x"], out[k + "out"], out[k + "g_out"], out[k + "g_x"] = G.npy(x), G.npy(y), G.npy(gy), G.npy(x.grad)
        for n, t in m.state_dict().items():
            out[k + "sd." + n] = G.npy(t)
        for n, p in m.named_parameters():
            out[k + "grad." + n] = G.npy(p.grad)
        if with_bias:
            out[k + "table"], out[k + "g_table"] = G.npy(rp.rel_pos_bias_table), G.npy(rp.rel_pos_bias_table.grad)
    return out


def make_batch(g):
    """Row 0 full, row 1 PAD at the front, row 2 PAD at the back, the rest random lengths either way."""
    mask = torch.ones(B, L, dtype=torch.bool)
    mask[1, :3] = False
    mask[2, 4:] = False
    for b in range(3, B):
        n = int(torch.randint(1, L + 1, (1,), generator=g))
        mask[b] = torch.arange(L) >= L - n if b % 2 else torch.arange(L) < n
    tok = torch.randint(1, V, (B, L), generator=g) * mask
    td = torch.sort(torch.randint(0, 3 * 10**5, (B, L), generator=g), 1, descending=True).values * mask
    return tok, torch.arange(L).repeat(B, 1), td, torch.randint(1, V, (B,), generator=g)


def gen_model(cfg):
    from torch_rechub.models.generative.hllm import HLLMModel
    from torch_rechub.trainers.seq_trainer import SeqTrainer
    kw = dict(MODEL_CFGS[cfg])
    loss_type = kw.pop("loss_type")
    torch.manual_seed(G.SEED)
    g = torch.Generator().manual_seed(G.SEED + 1)
    emb = torch.randn(V, kw["d_model"], generator=g)
    model = HLLMModel(emb, V, n_layers=2, max_seq_len=N, dropout=0.0, num_time_buckets=NB, **kw)
    batches = [make_batch(g) for _ in range(3)]
    out = {"cfg": np.array(json.dumps(dict(MODEL_CFGS[cfg]))), "sd_keys": np.array(list(model.state_dict())),
           "item_embeddings_raw": G.npy(emb)}
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
    logits = model(tok, td)
    out["train_logits"] = G.npy(logits)
    loss = trainer._compute_next_token_loss(logits, tok, tg)
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
    _save_fixed(os.path.join(G.OUT, f"model_hllm_{cfg}.npz"), out)
    print(f"model_hllm_{cfg}.npz", len(out), "arrays, loss", loss.item(), "mean train loss", mean_loss)


def main():
    import_reference()
    _save_fixed(os.path.join(G.OUT, "hllm_layers.npz"), gen_layers())
    print("hllm_layers.npz")
    for cfg in MODEL_CFGS:
        gen_model(cfg)


if __name__ == "__main__":
    main()
