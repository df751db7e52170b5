"""Generate the SASRec fixtures of tests/golden/ from the UNMODIFIED reference (CPU).

Run where the reference checkout exists:  ``python tools/gen_golden_sasrec.py``

  sasrec_layers.npz       one block + the input stage + the head of the reference's SASRec at (B 5, L 7, D 12, H 3) and
                          (B 4, L 5, D 10, H 1), dropout 0: ids, parameters (1-D ones shifted off their 0 / 1 init), every
                          intermediate captured with forward hooks (x0, Q, the MHA output, y, z, the block output, the final
                          LayerNorm, both logits) and every gradient (parameters and intermediates) for a drawn gradient of
                          the two logit matrices.
  model_sasrec_<cfg>.npz  SASRec (V 23, L 7, max_len 9; d12h3b2: D 12, 3 heads, 2 blocks; d10h1b1: D 10, 1 head, 1 block):
                          the seeded state_dict with both tables redrawn N(0, 0.1) (the reference's 1e-4 item table leaves
                          every other gradient at rounding noise), three batches (row 0 full, row 1 PAD at the front, row 2
                          PAD at the back, row 3 all PAD, row 4 random), the eval logits and user_tower in both modes, the
                          probe loss BPRLoss()(pos.reshape(-1), neg.reshape(-1)) and its gradients on batch 0, three
                          torch.optim.Adam steps (lr 1e-2, weight decay 1e-3) on it and the state after them.

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

V, L, N, LR, WD = 23, 7, 9, 1e-2, 1e-3
LAYER_CFGS = {"b5l7d12h3": (5, 7, 12, 3), "b4l5d10h1": (4, 5, 10, 1)}  # (B, L, D, H)
MODEL_CFGS = {"d12h3b2": dict(D=12, H=3, blocks=2), "d10h1b1": dict(D=10, H=1, blocks=1)}


def features(D):
    from torch_rechub.basic.features import SequenceFeature
    return [SequenceFeature("seq", vocab_size=V, embed_dim=D, pooling="concat"),
            SequenceFeature("pos", vocab_size=V, embed_dim=D, pooling="concat", shared_with="seq"),
            SequenceFeature("neg", vocab_size=V, embed_dim=D, pooling="concat", shared_with="seq")]


def make_batch(g, B, length):
    """Row 0 full, row 1 PAD at the front, row 2 PAD at the back, row 3 all PAD, the rest random lengths either way."""
    mask = torch.ones(B, length, dtype=torch.bool)
    mask[1, :length // 2] = False
    mask[2, length // 2 + 1:] = False
    mask[3] = False
    for b in range(4, B):
        n = int(torch.randint(1, length + 1, (1,), generator=g))
        mask[b] = torch.arange(length) >= length - n if b % 2 else torch.arange(length) < n
    return {k: torch.randint(1, V, (B, length), generator=g) * mask for k in ("seq", "pos", "neg")}


def redraw(model, g, std):
    with torch.no_grad():
        model.item_emb.embed_dict["seq"].weight.copy_(std * torch.randn(model.item_emb.embed_dict["seq"].weight.shape,
                                                                        generator=g))
        model.position_emb.weight.copy_(std * torch.randn(model.position_emb.weight.shape, generator=g))


def gen_layers():
    from torch_rechub.models.matching.sasrec import SASRec
    torch.manual_seed(G.SEED)
    g = torch.Generator().manual_seed(G.SEED)
    out = {"cfgs": np.array(json.dumps(LAYER_CFGS))}
    for name, (B, length, D, H) in LAYER_CFGS.items():
        model = SASRec(features(D), max_len=length + 2, dropout_rate=0.0, num_blocks=1, num_heads=H).train()
        redraw(model, g, 0.5)
        with torch.no_grad():  # biases and LayerNorm affine away from their zero / one init
            for _, p in model.named_parameters():
                if p.dim() == 1:
                    p.add_(0.1 * torch.randn(p.shape, generator=g))
        x = make_batch(g, B, length)
        k = f"{name}."
        seen = {}

        def keep(tag, t, time_major=False):
            seen[tag] = t.detach().clone().transpose(0, 1) if time_major else t.detach().clone()
            if t.requires_grad:
                t.register_hook(lambda gr, tag=tag, tm=time_major: seen.__setitem__(
                    "g_" + tag, gr.detach().clone().transpose(0, 1) if tm else gr.detach().clone()))

        def hook(*captures):  # (tag, "in" | "out", time_major) ...; returns None, so the module's output stands
            def fn(m, i, o):
                for tag, side, tm in captures:
                    keep(tag, i[0] if side == "in" else (o[0] if isinstance(o, tuple) else o), tm)
            return fn

        hooks = [
            model.attention_layernorms[0].register_forward_hook(hook(("x0", "in", True), ("Q", "out", True))),
            model.attention_layers[0].register_forward_hook(hook(("mha", "out", True))),
            model.forward_layernorms[0].register_forward_hook(hook(("y", "in", False), ("z", "out", False))),
            model.last_layernorm.register_forward_hook(hook(("block", "in", False), ("s", "out", False))),
        ]
        pos, neg = model(x)
        for h in hooks:
            h.remove()
        g_pos, g_neg = torch.randn(pos.shape, generator=g), torch.randn(neg.shape, generator=g)
        ((pos * g_pos).sum() + (neg * g_neg).sum()).backward()
        for n, t in x.items():
            out[k + n] = G.npy(t)
        out[k + "pos_logits"], out[k + "neg_logits"] = G.npy(pos), G.npy(neg)
        out[k + "g_pos_logits"], out[k + "g_neg_logits"] = G.npy(g_pos), G.npy(g_neg)
        for tag, t in seen.items():
            out[k + tag] = G.npy(t.contiguous())
        for n, t in model.state_dict().items():
            out[k + "sd." + n] = G.npy(t)
        for n, p in model.named_parameters():
            out[k + "grad." + n] = G.npy(p.grad)
    return out


def gen_model(cfg):
    from torch_rechub.basic.loss_func import BPRLoss
    from torch_rechub.models.matching.sasrec import SASRec
    c = MODEL_CFGS[cfg]
    torch.manual_seed(G.SEED)
    g = torch.Generator().manual_seed(G.SEED + 1)
    model = SASRec(features(c["D"]), max_len=N, dropout_rate=0.0, num_blocks=c["blocks"], num_heads=c["H"])
    out = {"cfg": np.array(json.dumps(c)), "sd_keys": np.array(list(model.state_dict()))}
    for n, t in model.state_dict().items():  # the reference's own initialisation, for its statistics
        out["init." + n] = G.npy(t)
    redraw(model, g, 0.1)
    for n, t in model.state_dict().items():
        out["sd0." + n] = G.npy(t)
    batches = [make_batch(g, 5, L) for _ in range(3)]
    for bi, x in enumerate(batches):
        for n, t in x.items():
            out[f"b{bi}.{n}"] = G.npy(t)
    x = batches[0]
    probe = BPRLoss()
    model.eval()
    with torch.no_grad():
        pos, neg = model(x)
        out["pos_logits"], out["neg_logits"] = G.npy(pos), G.npy(neg)
        out["user_tower"] = G.npy(model.user_tower(x))
        model.mode = "user"
        out["user_mode"] = G.npy(model(x))
        model.mode = None
    model.train()
    pos, neg = model(x)
    loss = probe(pos.reshape(-1), neg.reshape(-1))
    model.zero_grad()
    loss.backward()
    out["loss"] = np.array(loss.item())
    for n, p in model.named_parameters():
        out["grad." + n] = G.npy(p.grad) if p.grad is not None else np.zeros(tuple(p.shape), np.float32)
    model.zero_grad()
    opt = torch.optim.Adam(model.parameters(), lr=LR, weight_decay=WD)
    losses = []
    for x in batches:
        pos, neg = model(x)
        loss = probe(pos.reshape(-1), neg.reshape(-1))
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    out["train.lr"], out["train.wd"], out["train.losses"] = np.array(LR), np.array(WD), np.array(losses)
    for n, t in model.state_dict().items():
        out["sd3." + n] = G.npy(t)
    _save_fixed(os.path.join(G.OUT, f"model_sasrec_{cfg}.npz"), out)
    print(f"model_sasrec_{cfg}.npz", len(out), "arrays, losses", losses)


def main():
    import_reference()
    _save_fixed(os.path.join(G.OUT, "sasrec_layers.npz"), gen_layers())
    print("sasrec_layers.npz")
    for cfg in MODEL_CFGS:
        gen_model(cfg)


if __name__ == "__main__":
    main()
