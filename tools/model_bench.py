#!/usr/bin/env python
"""Train-step throughput of the secondary BASELINE.json configs on ONE GPU (eager + hipGraph):
  dcn / dcnv2 : configs[2] shape (Criteo tables, 13 dense + 26 sparse, 3 cross layers)          [C3 runs it data-parallel]
  din         : configs[3] shape (2 history fields x L=100 + 2 targets + user_id, D=16, attention MLP [256,128] Dice)
  dien / bst  : the same tables and histories through DIEN (GRU + AUGRU recurrences, auxiliary loss) / BST (1 encoder layer)
  dssm        : configs[4] shape (100 M-item + 10 M-user tables, history L=50 mean-pooled, towers [256,128,64] prelu,
                in-batch negatives)
  deepffm / fatdeepffm : the Criteo example's DeepFFM / FAT-DeepFFM (examples/ranking/run_criteo.py:77-80: 26 sparse fields,
                field-aware tables of v * 26 rows x 10, width-1 linear tables, MLP [1600, 1600] dropout 0.5); --scale 0.04
                gives field-aware tables of about as many rows as the DeepFM headline's.  Also times a plain-PyTorch eager
                restatement of the same model on the same GPU (nn.Embedding lookups, indexed pair products, torch.optim.Adam).
  youtubednn / mind / comirec_dr / comirec_sa : the retrieval examples' list-wise models (MatchTrainer(mode=2)) at B = 4096,
                history L = 50, D = 16, I = 4 interests, K = 3 negatives, a 10 M-row item table (--scale scales it), five
                user fields.  Also times a plain-PyTorch eager restatement (the reference's op chain, torch.optim.Adam).
  hstu / hstu_large : HSTUModel + SeqTrainer on synthetic sequences: the MovieLens-1M example shape (B 128, L 200, d 50,
                H 1, dqk = dv = 50, 2 layers, V 3707, l2 scoring, temperature 0.05, log buckets / 0.301 / seconds) and the
                reference defaults (d 512, H 8, dqk = dv = 64, 4 layers, L 256) at B 64, V 100 k.  Times the HIP step
                (fused attention and next-token loss), a plain-PyTorch eager restatement of the reference's op chain
                (dense (B, H, L, L) attention, (B, L, V) logits, clone, CrossEntropyLoss) and the kernels' device times.
  hllm / hllm_large : HLLMModel + SeqTrainer(loss_type='nce', temperature 1.0) on synthetic sequences: the MovieLens
                example's shape with a small embedding (B 64, L 200, d 512, H 8, 2 layers, V 3707, dropout 0.1) and
                d 2048, H 16, V 100 k.  Times the HIP step (fused causal softmax attention, frozen-table next-token
                loss), a plain-PyTorch eager restatement of the reference's op chain (dense (B, H, L, L) softmax
                attention with nn.Dropout, (B, L, V) logits, clone, NCELoss) and the kernels' device times.
  narm / stamp : the session-based example's shape (examples/matching/run_sbr.py: B 512, L <= 19, D 100, NARM hidden 50,
                NARM's dropouts 0.25 / 0.5) with
                a synthetic 50 000-item catalogue; narm_large / stamp_large: B 4096 against 10^6 items.  MatchTrainer(mode=2)
                through the fused catalogue loss, against a plain-PyTorch eager restatement of the reference's step
                (pack_padded_sequence + nn.GRU, the (B, V) scores, CrossEntropyLoss, torch.optim.Adam).
  gru4rec     : run_ml_gru4rec.py's shape (D 16, L 50, K 3 negatives, two bias-free GRU layers) at B 4096.
    python tools/model_bench.py --models dcn,dcnv2,din,dssm --steps 30
"""
import argparse
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import CRITEO_VOCABS  # noqa: E402


def build(name, dev, B, scale):
    from torch_rechub_amd.basic.features import DenseFeature, SequenceFeature, SparseFeature
    from torch_rechub_amd.models.matching import DSSM
    from torch_rechub_amd.models.ranking import DCN, DIN, DCNv2
    from torch_rechub_amd.trainers import CTRTrainer, MatchTrainer
    g = torch.Generator(device=dev).manual_seed(0)
    mlp = {"dims": [256, 128], "dropout": 0.2, "activation": "relu"}
    if name in ("dcn", "dcnv2"):
        vocabs = [max(3, int(v * scale)) for v in CRITEO_VOCABS]
        dense = [DenseFeature(f"I{i}") for i in range(13)]
        sparse = [SparseFeature(f"C{i}", v, 16) for i, v in enumerate(vocabs)]
        with torch.device(dev):
            model = DCN(dense + sparse, 3, {"dims": [256, 128]}) if name == "dcn" else DCNv2(dense + sparse, 3, mlp)
        x = {f.name: torch.randint(0, v, (B,), device=dev, generator=g) for f, v in zip(sparse, vocabs)}
        x.update({f.name: torch.rand(B, device=dev, generator=g) for f in dense})
        trainer = CTRTrainer(model, device=str(dev), show_progress=False)
    elif name in ("din", "dien", "bst"):
        nu, ni, nc, L = int(200000 * scale) + 10, int(63001 * scale) + 10, 801, 100
        feats = [SparseFeature("user_id", nu, 16)]
        hist = [SequenceFeature("hist_item", ni, 16, pooling="concat", shared_with="target_item", padding_idx=0),
                SequenceFeature("hist_cate", nc, 16, pooling="concat", shared_with="target_cate", padding_idx=0)]
        tgt = [SparseFeature("target_item", ni, 16, padding_idx=0), SparseFeature("target_cate", nc, 16, padding_idx=0)]
        with torch.device(dev):
            if name == "din":
                model = DIN(feats, hist, tgt, mlp_params={"dims": [256, 128], "dropout": 0.2},
                            attention_mlp_params={"dims": [256, 128]})
            elif name == "dien":  # same tables and history shape; negative histories for the auxiliary loss
                from torch_rechub_amd.models.ranking import DIEN
                neg = [SequenceFeature("neg_hist_item", ni, 16, pooling="concat", shared_with="target_item", padding_idx=0),
                       SequenceFeature("neg_hist_cate", nc, 16, pooling="concat", shared_with="target_cate", padding_idx=0)]
                model = DIEN(feats, hist, neg, tgt, mlp_params={"dims": [256, 128], "dropout": 0.2})
            else:
                from torch_rechub_amd.models.ranking import BST
                model = BST(feats, hist, tgt, mlp_params=mlp, nhead=4, dropout=0.2, num_layers=1, max_seq_len=L + 1)
        lens = torch.randint(1, L + 1, (B,), device=dev, generator=g)
        pad = torch.arange(L, device=dev)[None, :] >= lens[:, None]
        x = {"user_id": torch.randint(0, nu, (B,), device=dev, generator=g),
             "target_item": torch.randint(1, ni, (B,), device=dev, generator=g),
             "target_cate": torch.randint(1, nc, (B,), device=dev, generator=g),
             "hist_item": torch.randint(1, ni, (B, L), device=dev, generator=g).masked_fill(pad, 0),
             "hist_cate": torch.randint(1, nc, (B, L), device=dev, generator=g).masked_fill(pad, 0)}
        if name == "dien":
            x["neg_hist_item"] = torch.randint(1, ni, (B, L), device=dev, generator=g).masked_fill(pad, 0)
            x["neg_hist_cate"] = torch.randint(1, nc, (B, L), device=dev, generator=g).masked_fill(pad, 0)
        trainer = CTRTrainer(model, device=str(dev), show_progress=False, loss_mode=name != "dien")
    elif name == "dssm":
        nu, ni, L = int(10_000_000 * scale) + 10, int(100_000_000 * scale) + 10, 50
        user = [SparseFeature("user_id", nu, 16),
                SequenceFeature("hist_item", ni, 16, pooling="mean", shared_with="item_id", padding_idx=0)]
        item = [SparseFeature("item_id", ni, 16, padding_idx=0), SparseFeature("cate_id", 1000, 16)]
        tower = {"dims": [256, 128, 64], "activation": "prelu"}
        with torch.device(dev):
            model = DSSM(user, item, user_params=dict(tower), item_params=dict(tower), temperature=0.02)
        lens = torch.randint(1, L + 1, (B,), device=dev, generator=g)
        pad = torch.arange(L, device=dev)[None, :] >= lens[:, None]
        x = {"user_id": torch.randint(0, nu, (B,), device=dev, generator=g),
             "item_id": torch.randint(1, ni, (B,), device=dev, generator=g),
             "cate_id": torch.randint(0, 1000, (B,), device=dev, generator=g),
             "hist_item": torch.randint(1, ni, (B, L), device=dev, generator=g).masked_fill(pad, 0)}
        trainer = MatchTrainer(model, mode=0, in_batch_neg=True, in_batch_neg_ratio=20, device=str(dev),
                               show_progress=False)
    elif name in ("deepffm", "fatdeepffm"):
        from torch_rechub_amd.models.ranking import DeepFFM, FatDeepFFM
        vocabs = [max(3, int(v * scale)) for v in CRITEO_VOCABS]
        F = len(vocabs)
        linear = [SparseFeature(f"C{i}", v, 1) for i, v in enumerate(vocabs)]
        cross = [SparseFeature(f"C{i}", v * F, 10) for i, v in enumerate(vocabs)]
        ffm_mlp = {"dims": [1600, 1600], "dropout": 0.5, "activation": "relu"}
        with torch.device(dev):
            model = DeepFFM(linear, cross, 10, ffm_mlp) if name == "deepffm" else FatDeepFFM(linear, cross, 10, 3, ffm_mlp)
        x = {f.name: torch.randint(0, v, (B,), device=dev, generator=g) for f, v in zip(linear, vocabs)}
        trainer = CTRTrainer(model, device=str(dev), show_progress=False)
    elif name in RETRIEVAL:
        model, x = build_retrieval(name, dev, B, scale, g)
        return MatchTrainer(model, mode=2, device=str(dev), show_progress=False), x, torch.zeros(B, dtype=torch.long,
                                                                                                  device=dev)
    else:
        raise ValueError(name)
    y = (torch.rand(B, device=dev, generator=g) < 0.25).float()
    return trainer, x, y


RETRIEVAL = ("youtubednn", "mind", "comirec_dr", "comirec_sa")
R_L, R_D, R_I, R_K, R_ITEMS, R_USERS = 50, 16, 4, 3, 10_000_000, [1_000_000, 3, 8, 22, 4000]


def retrieval_batch(dev, B, n_item, g):
    lens = torch.randint(1, R_L + 1, (B,), device=dev, generator=g)
    pad = torch.arange(R_L, device=dev)[None, :] >= lens[:, None]
    x = {f"u{i}": torch.randint(0, v, (B,), device=dev, generator=g) for i, v in enumerate(R_USERS)}
    x["hist_movie_id"] = torch.randint(1, n_item, (B, R_L), device=dev, generator=g).masked_fill(pad, 0)
    x["movie_id"] = torch.randint(1, n_item, (B,), device=dev, generator=g)
    x["neg_items"] = torch.randint(1, n_item, (B, R_K), device=dev, generator=g)
    return x


def build_retrieval(name, dev, B, scale, g):
    from torch_rechub_amd.basic.features import SequenceFeature, SparseFeature
    from torch_rechub_amd.models.matching import MIND, ComirecDR, ComirecSA, YoutubeDNN
    n_item = max(1000, int(R_ITEMS * scale))
    user = [SparseFeature(f"u{i}", v, R_D) for i, v in enumerate(R_USERS)]
    hist = [SequenceFeature("hist_movie_id", n_item, R_D, pooling="concat", shared_with="movie_id")]
    item = [SparseFeature("movie_id", n_item, R_D)]
    neg = [SequenceFeature("neg_items", n_item, R_D, pooling="concat", shared_with="movie_id")]
    with torch.device(dev):
        if name == "youtubednn":
            mean_hist = [SequenceFeature("hist_movie_id", n_item, R_D, pooling="mean", shared_with="movie_id")]
            model = YoutubeDNN(user + mean_hist, item, neg, user_params={"dims": [128, 64, 16]}, temperature=0.02)
        elif name == "mind":
            model = MIND(user, hist, item, neg, max_length=R_L, temperature=0.02)
        elif name == "comirec_dr":
            model = ComirecDR(user, hist, item, neg, max_length=R_L, temperature=0.02)
            torch.nn.init.normal_(model.capsule.w, 0, 0.3)
        else:
            model = ComirecSA(user, hist, item, neg, temperature=0.02)
    return model, retrieval_batch(dev, B, n_item, g)


def torch_retrieval_ms(name, dev, B, scale, steps):
    """ms/step of a plain-PyTorch eager restatement of the reference's list-wise step at the same shape."""
    from torch import nn
    F_ = nn.functional
    n_item = max(1000, int(R_ITEMS * scale))
    g = torch.Generator(device=dev).manual_seed(0)
    x = retrieval_batch(dev, B, n_item, g)
    users = nn.ModuleList([nn.Embedding(v, R_D) for v in R_USERS]).to(dev)
    items = nn.Embedding(n_item, R_D).to(dev)
    nu = len(R_USERS) * R_D
    params = list(users.parameters()) + list(items.parameters())
    if name == "youtubednn":
        dims = [nu + R_D, 128, 64, 16]
        mlp = []
        for a, w in zip(dims, dims[1:]):
            mlp += [nn.Linear(a, w), nn.BatchNorm1d(w), nn.ReLU()]
        mlp = nn.Sequential(*mlp).to(dev)
        params += list(mlp.parameters())
    else:
        conv = nn.Parameter(torch.rand(nu + R_D, R_D, device=dev))
        params.append(conv)
        if name == "comirec_sa":
            W1 = nn.Parameter(torch.rand(R_D, 4 * R_D, device=dev))
            W2 = nn.Parameter(torch.rand(4 * R_D, R_I, device=dev))
            params += [W1, W2]
        elif name == "mind":
            lin = nn.Linear(R_D, R_D, bias=False).to(dev)
            params += list(lin.parameters())
        else:
            w = nn.Parameter(0.3 * torch.randn(1, R_L, R_I * R_D, R_D, device=dev))
            params.append(w)
    opt = torch.optim.Adam(params, lr=1e-3)
    y = torch.zeros(B, dtype=torch.long, device=dev)

    def capsule(e, mask, kind):
        uh = lin(e).repeat(1, 1, R_I) if kind == 0 else torch.sum(w[:, :R_L] * e.unsqueeze(2), dim=3)
        uh = uh.reshape(-1, R_L, R_I, R_D).transpose(1, 2).contiguous()
        uh_it = uh.detach()
        cw = torch.randn(B, R_I, R_L, device=dev) if kind == 0 else torch.zeros(B, R_I, R_L, device=dev)
        am = mask.unsqueeze(1).repeat(1, R_I, 1)
        for i in range(3):
            sw = torch.where(am == 0, torch.zeros_like(cw), F_.softmax(cw, dim=-1)).unsqueeze(2)
            cap = torch.matmul(sw, uh_it if i < 2 else uh)
            n = torch.sum(torch.square(cap), -1, True)
            cap = n / (1 + n) / torch.sqrt(n + 1e-9) * cap
            if i < 2:
                cw = cw + torch.matmul(uh_it, cap.transpose(2, 3)).reshape(-1, R_I, R_L)
        return cap.reshape(-1, R_I, R_D)

    def step():
        u_in = torch.cat([t(x[f"u{i}"]) for i, t in enumerate(users)], 1)
        his = x["hist_movie_id"]
        e = items(his)
        if name == "youtubednn":
            hmask = (his > 0).float().unsqueeze(-1)
            u = F_.normalize(mlp(torch.cat([u_in, (e * hmask).sum(1) / (hmask.sum(1) + 1e-16)], 1)), dim=-1).unsqueeze(1)
        else:
            mask = (his > 0).long()
            if name == "comirec_sa":
                A = torch.einsum("bsd,dk->bsk", torch.einsum("bse,ed->bsd", e, W1).tanh(), W2)
                A = F_.softmax(A + -1.e9 * (1 - mask.unsqueeze(-1).float()), dim=1)
                interests = torch.matmul(A.permute(0, 2, 1), e)
            else:
                interests = capsule(e, mask, 0 if name == "mind" else 2)
            u = torch.cat([u_in.unsqueeze(1).expand(B, R_I, nu), interests], -1)
            u = F_.normalize(torch.matmul(u, conv), p=2, dim=-1)
        it = F_.normalize(torch.cat([items(x["movie_id"]).unsqueeze(1), items(x["neg_items"])], 1), p=2, dim=-1)
        if name == "youtubednn":
            logits = (u * it).sum(2) / 0.02
        else:
            k = torch.argmax(torch.bmm(u, it[:, 0].unsqueeze(-1)), dim=1).squeeze(-1)
            logits = (u[torch.arange(B, device=dev), k].unsqueeze(1) * it).sum(-1)
        loss = F_.cross_entropy(logits, y)
        opt.zero_grad()
        loss.backward()
        opt.step()

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


def torch_ffm_ms(name, dev, B, scale, steps):
    """ms/step of a plain-PyTorch eager DeepFFM / FAT-DeepFFM train step at the same shape (the comparison line)."""
    from torch import nn
    vocabs = [max(3, int(v * scale)) for v in CRITEO_VOCABS]
    F, D = len(vocabs), 10
    I, J = torch.triu_indices(F, F, 1, device=dev)
    P = I.numel()
    lin = nn.ModuleList([nn.Embedding(v, 1) for v in vocabs]).to(dev)
    ffm = nn.ModuleList([nn.Embedding(v * F, D) for v in vocabs]).to(dev)

    def blocks(d_in, dims, p_drop):
        out = []
        for a, w in zip([d_in] + dims, dims):
            out += [nn.Linear(a, w), nn.BatchNorm1d(w), nn.ReLU(), nn.Dropout(p_drop)]
        return out

    mlp = nn.Sequential(*blocks(P * D, [1600, 1600], 0.5), nn.Linear(1600, 1)).to(dev)
    fat = name == "fatdeepffm"
    u = nn.Parameter(torch.rand(P, D, device=dev))
    att = nn.Sequential(*blocks(P, [P // 3, P], 0.0)).to(dev)
    params = list(lin.parameters()) + list(ffm.parameters()) + list(mlp.parameters()) + ([u] + list(att.parameters()) if fat else [])
    opt = torch.optim.Adam(params, lr=1e-3)
    g = torch.Generator(device=dev).manual_seed(0)
    x = torch.stack([torch.randint(0, v, (B,), device=dev, generator=g) for v in vocabs], 1)
    y = (torch.rand(B, device=dev, generator=g) < 0.25).float()
    off = torch.arange(F, device=dev)

    def step():
        y_lin = sum(t(x[:, f]) for f, t in enumerate(lin))
        e = torch.stack([t(x[:, f:f + 1] * F + off) for f, t in enumerate(ffm)], 1)  # (B, F, F, D)
        em = e[:, I, J] * e[:, J, I]
        if fat:
            em = att(torch.relu((u * em).sum(-1))).unsqueeze(-1) * em
        p = torch.sigmoid((mlp(em.flatten(1)) + y_lin).squeeze(1))
        loss = nn.functional.binary_cross_entropy(p, y)
        opt.zero_grad()
        loss.backward()
        opt.step()

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / steps * 1e3


HSTU = {"hstu": dict(B=128, L=200, V=3707, d_model=50, n_heads=1, n_layers=2, dqk=50, dv=50, score_norm="l2",
                     temperature=0.05, time_bucket_fn="log", time_bucket_divisor=0.301, time_bucket_unit="seconds"),
        "hstu_large": dict(B=64, L=256, V=100000, d_model=512, n_heads=8, n_layers=4, dqk=64, dv=64)}


def hstu_bench(name, dev, steps):
    """ms/step of the HIP SeqTrainer step and of a plain-PyTorch eager restatement of the reference's step."""
    import torch.nn.functional as F

    from torch_rechub_amd.models.generative import HSTUModel
    from torch_rechub_amd.trainers import SeqTrainer
    cfg = dict(HSTU[name])
    B, L, V = cfg.pop("B"), cfg.pop("L"), cfg.pop("V")
    torch.manual_seed(0)
    model = HSTUModel(V, max_seq_len=L, dropout=0.0, **cfg)
    trainer = SeqTrainer(model, device=str(dev))
    g = torch.Generator().manual_seed(0)
    lens = torch.randint(L // 4, L + 1, (B,), generator=g)
    tok = torch.randint(1, V, (B, L), generator=g) * (torch.arange(L)[None, :] >= L - lens[:, None])  # left padded
    td = torch.sort(torch.randint(0, 10**8, (B, L), generator=g), 1, descending=True).values
    tok, td, tg = tok.to(dev), td.to(dev), torch.randint(1, V, (B,), generator=g).to(dev)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    hip = timed(lambda: trainer.train_step(tok, td, tg))
    kernels = {}
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            trainer.train_step(tok, td, tg)
            torch.cuda.synchronize()
        import re
        for ev in prof.key_averages():
            m = re.search(r"\b(hstu_\w+_kernel|head_\w+_kernel)", ev.key)
            if m:
                us, n = kernels.get(m.group(1), (0.0, 0))
                kernels[m.group(1)] = (us + ev.device_time_total, n + ev.count)
    except Exception as e:  # noqa: BLE001
        print(f"  [{name}] profiler unavailable: {type(e).__name__}: {e}")
    mem_hip = torch.cuda.max_memory_allocated() / 2**30
    torch.cuda.reset_peak_memory_stats()

    def eager_loss():
        padding = tok.ne(0)
        x = model.token_embedding(tok) + model.position_embedding(torch.arange(L, device=dev))[None]
        x = x + model.time_embedding(model._time_diff_to_bucket(td))
        x = x * padding[..., None]
        causal = torch.tril(torch.ones(L, L, device=dev, dtype=torch.bool))[None, None] & padding[:, None, None, :]
        for layer in model.hstu_block.layers:
            H, dqk, dv = layer.n_heads, layer.dqk, layer.dv
            p = F.silu(layer.proj1(layer.norm_in(x)))
            q = p[..., :H * dqk].reshape(B, L, H, dqk).transpose(1, 2)
            k = p[..., H * dqk:2 * H * dqk].reshape(B, L, H, dqk).transpose(1, 2)
            u = p[..., 2 * H * dqk:2 * H * dqk + H * dv]
            v = p[..., 2 * H * dqk + H * dv:].reshape(B, L, H, dv).transpose(1, 2)
            s = torch.matmul(q, k.transpose(-2, -1)) * layer.attn_alpha + layer.rab(time_diffs=td, seq_len=L)
            a = F.silu(s.masked_fill(~causal, -1e4)) / layer.max_seq_len
            o = torch.matmul(a, v).transpose(1, 2).reshape(B, L, H * dv)
            x = x + layer.proj2(layer.norm_attn(o) * u)
        x = x * padding[..., None]
        w, b = model.token_embedding.weight, model.output_bias
        if model.score_norm == "l2":
            x, w = F.normalize(x, dim=-1, eps=model.l2_norm_eps), F.normalize(w, dim=-1, eps=model.l2_norm_eps)
        logits = F.linear(x, w, b)
        if model.temperature != 1.0:
            logits = logits / model.temperature
        return trainer._compute_next_token_loss(logits, tok, tg)

    def eager_step():
        loss = eager_loss()
        model.zero_grad()
        loss.backward()
        trainer.optimizer.step()

    eager_top = []
    try:
        eager = timed(eager_step)
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            eager_step()
            torch.cuda.synchronize()
        evs = [ev for ev in prof.key_averages() if ev.device_time_total > 0]
        total = sum(ev.device_time_total for ev in evs)
        eager_top = [(ev.key[:70], ev.device_time_total, ev.count) for ev in
                     sorted(evs, key=lambda ev: -ev.device_time_total)[:8]] + [("(all device work)", total, 0)]
    except torch.cuda.OutOfMemoryError:
        eager = float("nan")
        print(f"  [{name}] eager restatement does not fit")
    mem_eager = torch.cuda.max_memory_allocated() / 2**30
    print(f"{name:10s} B={B} L={L} V={V}  HIP {hip:8.3f} ms/step (peak {mem_hip:.1f} GiB)   plain PyTorch eager "
          f"{eager:8.3f} ms/step (peak {mem_eager:.1f} GiB)   speedup {eager / hip:.2f}x", flush=True)
    for k, (us, n) in sorted(kernels.items(), key=lambda kv: -kv[1][0]):
        print(f"    {k:32s} {us:10.1f} us per step ({n} launches)", flush=True)
    for k, us, n in eager_top:
        print(f"    eager: {k:70s} {us:12.1f} us per step ({n} launches)", flush=True)
    from torch_rechub_amd import ops
    ops.check_errors()


SESSION = {"narm": dict(B=512, L=19, V=50000), "stamp": dict(B=512, L=19, V=50000),
           "narm_large": dict(B=4096, L=19, V=1000000), "stamp_large": dict(B=4096, L=19, V=1000000),
           "gru4rec": dict(B=4096, L=50, V=100000)}


def session_bench(name, dev, steps):
    """ms/step of MatchTrainer on NARM / STAMP / GRU4Rec and of a plain-PyTorch eager restatement of the reference's step."""
    import re

    import torch.nn.functional as F
    import torch.nn.utils.rnn as rnn_utils

    from torch_rechub_amd.basic.features import SequenceFeature, SparseFeature
    from torch_rechub_amd.models.matching import NARM, STAMP, GRU4Rec
    from torch_rechub_amd.trainers import MatchTrainer
    c = SESSION[name]
    B, L, V = c["B"], c["L"], c["V"]
    kind = name.split("_")[0]
    g = torch.Generator().manual_seed(0)
    seq = torch.randint(1, V, (B, L), generator=g)
    lens = torch.randint(1, L + 1, (B,), generator=g)
    lens[0] = L
    if kind != "gru4rec":
        seq[torch.arange(L)[None] >= lens[:, None]] = 0
    torch.manual_seed(0)
    if kind == "gru4rec":
        D = 16
        hist = SequenceFeature("hist_item_id", V, D, pooling="concat", shared_with="item_id")
        user = [SparseFeature("user_id", 6040, D), SparseFeature("gender", 3, D), SparseFeature("age", 8, D)]
        item = [SparseFeature("item_id", V, D)]
        neg = [SequenceFeature("neg_items", V, D, pooling="concat", shared_with="item_id")]
        model = GRU4Rec(user, [hist], item, neg, user_params={"dims": [64, D]}).to(dev)
        x = {"user_id": torch.randint(0, 6040, (B,), generator=g), "gender": torch.randint(0, 3, (B,), generator=g),
             "age": torch.randint(0, 8, (B,), generator=g), "hist_item_id": seq,
             "item_id": torch.randint(1, V, (B,), generator=g), "neg_items": torch.randint(1, V, (B, 3), generator=g)}
        y = torch.zeros(B, dtype=torch.long)
    else:
        D = 100
        f = SequenceFeature("hist_item_id", V, D, pooling="concat")
        model = (NARM(f, 50, 0.25, 0.5) if kind == "narm" else STAMP(f, 0.05, 0.002)).to(dev)  # (run_sbr.py defaults)
        x = {"hist_item_id": seq}
        y = torch.randint(0, V, (B,), generator=g)
    x, y = {k: v.to(dev) for k, v in x.items()}, y.to(dev)
    trainer = MatchTrainer(model, mode=2, device=str(dev), show_progress=False)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    torch.cuda.reset_peak_memory_stats()
    hip = timed(lambda: trainer.train_step(x, y))
    mem_hip = torch.cuda.max_memory_allocated() / 2**30
    kernels = {}
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            trainer.train_step(x, y)
            torch.cuda.synchronize()
        for ev in prof.key_averages():
            if ev.device_time_total > 0:
                m = re.search(r"\b(\w+_kernel)\b", ev.key)
                key = m.group(1) if m else ev.key[:40]
                us, n = kernels.get(key, (0.0, 0))
                kernels[key] = (us + ev.device_time_total, n + ev.count)
    except Exception as e:  # noqa: BLE001
        print(f"  [{name}] profiler unavailable: {type(e).__name__}: {e}")

    # plain PyTorch: the reference's op chain on the same parameters, torch.optim.Adam
    params = [p for p in model.parameters()]
    opt = torch.optim.Adam(params, lr=1e-3, weight_decay=1e-5)
    if kind == "narm":
        def eager_loss():
            mask = seq_d != 0
            counts = mask.sum(1).cpu()
            embs = rnn_utils.pack_padded_sequence(F.dropout(F.embedding(seq_d, model.item_emb.weight, 0), 0.25), counts, batch_first=True,
                                                  enforce_sorted=False)
            h, h_t = torch.nn.GRU.forward(model.gru, embs)
            h_t = h_t.permute(1, 0, 2)
            h, _ = rnn_utils.pad_packed_sequence(h, batch_first=True)
            q = torch.sigmoid(h_t @ model.a_1.T + h @ model.a_2.T) @ model.v
            alpha = torch.exp(q) * mask.unsqueeze(-1)
            alpha = alpha / alpha.sum(dim=1, keepdim=True)
            cvec = F.dropout(torch.hstack((h_t.squeeze(1), (alpha * h).sum(1))), 0.5)
            return F.cross_entropy(cvec @ model.b.T @ model.item_emb.weight.T, y)
    elif kind == "stamp":
        def eager_loss():
            m = model
            vm = (seq_d != 0).unsqueeze(-1)
            vc = vm.sum(dim=1, keepdim=True).squeeze(-1)
            e = F.embedding(seq_d, m.item_emb.weight, 0) * vm
            x_t = F.embedding(torch.gather(seq_d, 1, vc - 1), m.item_emb.weight, 0)
            m_s = (e.sum(1) / vc).unsqueeze(1)
            a = F.normalize(torch.exp(torch.sigmoid(e @ m.w_1_t + x_t @ m.w_2_t + m_s @ m.w_3_t + m.b_a) @ m.w_0) * vm,
                            p=1, dim=1)
            m_a = (a * e).sum(1) + m_s.squeeze(1)
            u = m.f_s(m_a) * m.f_t(x_t).squeeze(1)
            return F.cross_entropy(u @ m.item_emb.weight.T, y)
    else:
        tabs = model.embedding.embed_dict

        def emb(k, ids):
            t = tabs["item_id" if k in ("hist_item_id", "neg_items") else k]
            return F.embedding(ids, t.weight)[..., :D]

        def eager_loss():
            u_in = torch.cat([emb(k, x[k]) for k in ("user_id", "gender", "age")], 1)
            _, h = torch.nn.GRU.forward(model.gru, emb("hist_item_id", x["hist_item_id"]))
            u = F.normalize(model.user_mlp.mlp(torch.cat([u_in, h[-1]], 1)), dim=-1).unsqueeze(1)
            items = F.normalize(torch.cat([emb("item_id", x["item_id"]).unsqueeze(1), emb("neg_items", x["neg_items"])], 1),
                                dim=-1)
            return F.cross_entropy((u * items).sum(1), y)
    seq_d = x["hist_item_id"]

    def eager_step():
        loss = eager_loss()
        opt.zero_grad()
        loss.backward()
        opt.step()

    torch.cuda.reset_peak_memory_stats()
    try:
        eager = timed(eager_step)
    except torch.cuda.OutOfMemoryError:
        eager = float("nan")
        print(f"  [{name}] eager restatement does not fit")
    mem_eager = torch.cuda.max_memory_allocated() / 2**30
    print(f"{name:12s} B={B} L={L} V={V}  HIP {hip:8.3f} ms/step (peak {mem_hip:.1f} GiB)   plain PyTorch eager "
          f"{eager:8.3f} ms/step (peak {mem_eager:.1f} GiB)   speedup {eager / hip:.2f}x", flush=True)
    for k, (us, n) in sorted(kernels.items(), key=lambda kv: -kv[1][0])[:12]:
        print(f"    {k:40s} {us:10.1f} us per step ({n} launches)", flush=True)
    from torch_rechub_amd import ops
    ops.check_errors()


HLLM = {"hllm": dict(B=64, L=200, V=3707, d_model=512, n_heads=8, n_layers=2),
        "hllm_large": dict(B=64, L=200, V=100000, d_model=2048, n_heads=16, n_layers=2)}


def hllm_bench(name, dev, steps):
    """ms/step of the HIP SeqTrainer step of HLLMModel and of a plain-PyTorch eager restatement of the reference's step."""
    import re

    import torch.nn.functional as F
    from torch.profiler import ProfilerActivity, profile

    from torch_rechub_amd.models.generative import HLLMModel
    from torch_rechub_amd.trainers import SeqTrainer
    cfg = dict(HLLM[name])
    B, L, V = cfg.pop("B"), cfg.pop("L"), cfg.pop("V")
    torch.manual_seed(0)
    g = torch.Generator().manual_seed(0)
    model = HLLMModel(torch.randn(V, cfg["d_model"], generator=g), V, max_seq_len=L, dropout=0.1, **cfg)
    trainer = SeqTrainer(model, device=str(dev), loss_type="nce", loss_params={"temperature": 1.0, "ignore_index": 0})
    model.train()
    lens = torch.randint(L // 4, L + 1, (B,), generator=g)
    tok = torch.randint(1, V, (B, L), generator=g) * (torch.arange(L)[None, :] >= L - lens[:, None])  # left padded
    td = torch.sort(torch.randint(0, 10**8, (B, L), generator=g), 1, descending=True).values
    tok, td, tg = tok.to(dev), td.to(dev), torch.randint(1, V, (B,), generator=g).to(dev)

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / steps * 1e3

    torch.cuda.reset_peak_memory_stats()
    hip = timed(lambda: trainer.train_step(tok, td, tg))
    mem_hip = torch.cuda.max_memory_allocated() / 2**30
    kernels = {}
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        trainer.train_step(tok, td, tg)
        torch.cuda.synchronize()
    evs = [ev for ev in prof.key_averages() if ev.device_time_total > 0]
    hip_total = sum(ev.device_time_total for ev in evs)
    for ev in evs:
        m = re.search(r"\b(softmax_attn_\w+_kernel|head_\w+_kernel|dropout\w*_kernel|drop_advance_kernel)", ev.key)
        if m:
            us, n = kernels.get(m.group(1), (0.0, 0))
            kernels[m.group(1)] = (us + ev.device_time_total, n + ev.count)
    torch.cuda.reset_peak_memory_stats()

    def eager_loss():
        x = model.item_embeddings[tok] + model.position_embedding(torch.arange(L, device=dev))[None]
        x = x + model.time_embedding(model._time_diff_to_bucket(td))
        x = F.dropout(x, 0.1)
        bias = model.rel_pos_bias(L)
        causal = torch.tril(torch.ones(L, L, device=dev, dtype=torch.bool))[None, None]
        for blk in model.transformer_blocks:
            H, dh = blk.n_heads, blk.head_dim
            h = blk.norm1(x)
            q, k, v = (w(h).view(B, L, H, dh).transpose(1, 2) for w in (blk.W_Q, blk.W_K, blk.W_V))
            s = (torch.matmul(q, k.transpose(-2, -1)) * blk.scale).masked_fill(~causal, float("-inf")) + bias
            a = F.dropout(F.softmax(s, dim=-1), 0.1)
            o = torch.matmul(a, v).transpose(1, 2).contiguous().view(B, L, H * dh)
            x = x + F.dropout(blk.W_O(o), 0.1)
            h = F.dropout(F.relu(blk.ffn[0](blk.norm2(x))), 0.1)
            x = x + F.dropout(blk.ffn[3](h), 0.1)
        logits = torch.matmul(F.normalize(x, dim=-1, eps=1e-8), model.item_embeddings.t()) / model.temperature
        return trainer._compute_next_token_loss(logits, tok, tg)

    def eager_step():
        loss = eager_loss()
        model.zero_grad()
        loss.backward()
        trainer.optimizer.step()

    eager_top = []
    try:
        eager = timed(eager_step)
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            eager_step()
            torch.cuda.synchronize()
        evs = [ev for ev in prof.key_averages() if ev.device_time_total > 0]
        total = sum(ev.device_time_total for ev in evs)
        eager_top = [(ev.key[:70], ev.device_time_total, ev.count) for ev in
                     sorted(evs, key=lambda ev: -ev.device_time_total)[:8]] + [("(all device work)", total, 0)]
    except torch.cuda.OutOfMemoryError:
        eager = float("nan")
        print(f"  [{name}] eager restatement does not fit")
    mem_eager = torch.cuda.max_memory_allocated() / 2**30
    print(f"{name:10s} B={B} L={L} V={V}  HIP {hip:8.3f} ms/step (peak {mem_hip:.2f} GiB)   plain PyTorch eager "
          f"{eager:8.3f} ms/step (peak {mem_eager:.2f} GiB)   speedup {eager / hip:.2f}x", flush=True)
    for k, (us, n) in sorted(kernels.items(), key=lambda kv: -kv[1][0]):
        print(f"    {k:32s} {us:10.1f} us per step ({n} launches)", flush=True)
    print(f"    {'(all device work of the HIP step)':32s} {hip_total:10.1f} us per step", flush=True)
    for k, us, n in eager_top:
        print(f"    eager: {k:70s} {us:12.1f} us per step ({n} launches)", flush=True)
    from torch_rechub_amd import ops
    ops.check_errors()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--models", default="dcn,dcnv2,din,dssm")
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--scale", type=float, default=1.0, help="vocabulary scale")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in a.models.split(","):
        torch.cuda.empty_cache()
        if name in SESSION:
            session_bench(name, dev, a.steps)
            torch.cuda.reset_peak_memory_stats()
            continue
        if name in HSTU:
            hstu_bench(name, dev, a.steps)
            torch.cuda.reset_peak_memory_stats()
            continue
        if name in HLLM:
            hllm_bench(name, dev, a.steps)
            torch.cuda.reset_peak_memory_stats()
            continue
        trainer, x, y = build(name, dev, a.batch, a.scale)
        trainer.model.train()
        trainer.optimizer.sync_hyper()
        print(f"  [{name}] built", flush=True)
        for i in range(5):
            trainer.train_step(x, y)
            if os.environ.get("MB_SYNC"):
                torch.cuda.synchronize()
                print(f"  [{name}] warm step {i} ok", flush=True)
        torch.cuda.synchronize()
        print(f"  [{name}] warm-up done", flush=True)
        t0 = time.perf_counter()
        for _ in range(a.steps):
            trainer.train_step(x, y)
        trainer.flush()
        torch.cuda.synchronize()
        eager = (time.perf_counter() - t0) / a.steps
        print(f"  [{name}] eager done {eager * 1e3:.3f} ms/step", flush=True)
        # hipGraph replay of the same step on the same static batch
        graph_ms = float("nan")
        try:
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                for _ in range(2):
                    trainer.train_step(x, y)
            torch.cuda.current_stream().wait_stream(s)
            from torch_rechub_amd.graphs import SegmentedGraph
            gph = SegmentedGraph()  # lets the optimizer cut the step where it launches its side-stream sweep
            gph.capture(lambda: trainer.train_step(x, y))
            print(f"  [{name}] captured ({len(gph.segments)} segments)", flush=True)
            for _ in range(3):
                gph.replay()
            torch.cuda.synchronize()
            print(f"  [{name}] replays ok", flush=True)
            t0 = time.perf_counter()
            for _ in range(a.steps):
                gph.replay()
            trainer.flush()
            torch.cuda.synchronize()
            graph_ms = (time.perf_counter() - t0) / a.steps * 1e3
        except Exception as e:  # noqa: BLE001
            print(f"  [{name}] graph capture failed: {type(e).__name__}: {e}")
            torch.cuda.synchronize()
        mem = torch.cuda.max_memory_allocated() / 2**30
        print(f"{name:6s} B={a.batch} eager {eager * 1e3:8.3f} ms/step ({a.batch / eager / 1e3:9.1f} k samples/s)   "
              f"hipGraph {graph_ms:8.3f} ms/step ({a.batch / graph_ms:9.1f} k samples/s)   peak mem {mem:.1f} GiB",
              flush=True)
        from torch_rechub_amd import ops
        ops.check_errors()
        del trainer, x, y
        if name in ("deepffm", "fatdeepffm") + RETRIEVAL:
            torch.cuda.empty_cache()
            ms = (torch_ffm_ms if name in ("deepffm", "fatdeepffm") else torch_retrieval_ms)(name, dev, a.batch, a.scale,
                                                                                            a.steps)
            print(f"{name:6s} B={a.batch} plain PyTorch eager {ms:8.3f} ms/step ({a.batch / ms:9.1f} k samples/s)", flush=True)
        torch.cuda.reset_peak_memory_stats()


if __name__ == "__main__":
    main()
