"""TIGER and SASRec as whole models in training mode, dropout on, against float64 oracles (tests/tiger_oracle.py with its
``drop`` callable, tests/sasrec_oracle.py model_fwd_bwd with its ``draw`` callable) whose masks come from the host: ``host_keep``
of tests/test_gpu_mlp_dropout_oracle.py, never from a kernel under test.

Counter protocol.  Every dropout site with p > 0 in training reads (seed, counter) from the device state, saves the counter for
its own backward and advances it by one (csrc/common.h drop_key; ops._DropoutFn, ops._T5AttnFn, ops._SoftmaxAttnFn,
ops._SasrecInputFn, ops._SasrecFfnFn).  With the state set to (RNG_SEED, C0, 0, 0), site s of pass t uses counter
C0 + t SITES + s, and rng[1] == C0 + 2 SITES after the two passes.  Sites in program order and their element index:
  TIGER (models/generative/tiger.py T5Stack.forward; the encoder, then the decoder): the token dropout (flat over (B, L, D));
        per block the self-attention weights (((b H + h) Lq + i) Lk + j), the attention delta (flat), in the decoder the
        cross-attention weights and their delta, relu(wi) (flat over (B, L, d_ff)) and wo (flat); the final dropout (flat).
        SITES = (2 + 4 num_layers) + (2 + 6 num_decoder_layers): 24 for fixture a, 20 for fixture b.
  SASRec (models/matching/sasrec.py seq_forward): ops.sasrec_input (flat over (B, L, D)); per block ops.softmax_attention
        (((b H + h) L + i) L + j) and ops.sasrec_ffn, which draws ONE counter: dropout1 is elements [0, M D) and dropout2
        [M D, 2 M D) of it, M = B L.  SITES = 1 + 2 blocks = 5.
Two forward and backward passes on the fixture batch, gradients accumulated; compared after pass 2: logits (pos, neg), loss and
every parameter's gradient.  TIGER: test_gpu_tiger.py's ``close`` (rtol 2e-4, atol 2e-5 max|want|).  SASRec: the ``close``
calls of test_gpu_sasrec.py::test_probe_loss_and_gradients_match_the_reference (rtol 1e-4, atol 1e-4 max|want| for the wide
weights and 1e-5 otherwise, the loss to 1e-5 relative, the item table's logical columns).  The p = 0 controls go through the
same helpers.  No floor was raised.

ReLU kink (TIGER's wi, SASRec's conv1 after dropout1): a condition on the inputs, asserted from the float64 oracle alone before
any comparison: the smallest |pre-activation| over the kept units, every ReLU, both passes, is >= 1e-5.  C0 was chosen by scanning
C0 = 1..12 with the oracle only (``python tests/test_gpu_seq_models_dropout_oracle.py`` repeats the scan on the CPU).  Margins at
the chosen C0: TIGER a p 0.3 C0 12: 1.3e-03 (1.3e-05 to 1.3e-03 over the scan, all twelve qualify); TIGER b p 0.1 C0 9: 1.1e-03
(1.0e-04 to 1.1e-03); SASRec d12h3b2 p 0.5 C0 11: 7.0e-03 (2.4e-04 to 7.0e-03); the p = 0 controls 7.8e-04 and 1.1e-03.
Negative control, one per model: the oracle with the counters of two sites swapped (the first self-attention's weights against
the site that follows it: TIGER's attention delta, SASRec's FFN) must be missed by more than 100 x the tolerance.  Host side
(wrong oracle against right oracle, worst quantity, in units of the tolerance): TIGER a 44550 x (b: 44749 x), SASRec 54493 x.
Worst error / tolerance per compared quantity on the MI355X (the ``ORACLE`` lines): TIGER a p 0.3: logits 0.009, loss 0.000, gradients at
most 0.027 (decoder.block.0.layer.1.EncDecAttention.q.weight); TIGER b p 0.1: logits 0.006, loss 0.001, gradients 0.024; TIGER a
p 0 control: logits 0.008, gradients 0.027; SASRec p 0.5: pos 0.005, neg 0.009, loss 0.007, gradients 0.019
(forward_layers.0.conv1.bias); SASRec p 0 control: pos 0.006, neg 0.003, loss 0.012, gradients 0.015.  The swapped-counter
oracles are missed by 67454 x (TIGER a) and 35083 x (SASRec).  No bug was found.  With a scratch build (not committed) whose
attention kernels swap Lq and Lk in the dropout index, or whose backwards read rng[1] instead of the saved counter, every
p > 0 test of this module fails and the p = 0 controls pass.
"""
import functools
import json

import numpy as np
import pytest
import torch

import sasrec_oracle as SO
import tiger_oracle as TO
from test_gpu_mlp_dropout_oracle import RNG_SEED, host_keep
from test_tiger_host import model_fixture

pytestmark = pytest.mark.gpu
PASSES = 2
KINK = 1e-5
TIGER_C0 = {("a", 0.3): 12, ("b", 0.1): 9, ("a", 0.0): 12}
SASREC_C0 = {0.5: 11, 0.0: 11}
SASREC_CFG = "d12h3b2"
SWAP = {1: 2, 2: 1}  # the first self-attention's weights <-> the site after it


def dev():
    return torch.device("cuda:0")


def set_rng(c0):
    from torch_rechub_amd import ops
    rng = ops._dropout_rng(dev())
    rng.copy_(torch.tensor([RNG_SEED, c0, 0, 0], dtype=torch.int64))
    return rng


class Counters(object):
    """Hands out the host's keep flags counter by counter: site s of pass t takes C0 + t sites + s (s through ``perm`` for a
    deliberately wrong oracle)."""

    def __init__(self, c0, p, sites, perm=None):
        self.c0, self.p, self.sites, self.perm, self.calls = c0, p, sites, perm or {}, 0

    def keep(self, n):
        t, s = divmod(self.calls, self.sites)
        self.calls += 1
        return host_keep(RNG_SEED, self.c0 + t * self.sites + self.perm.get(s, s), n, self.p)

    def drop(self, shape):  # tiger_oracle's ``drop``
        keep = self.keep(int(np.prod(shape))).reshape(tuple(shape))
        return torch.from_numpy(keep.astype(np.float64) * SO.keep_scale(self.p))


def ratio(got, want, rtol, atol_rel):
    """largest |got - want| / (atol_rel max|want| + rtol |want|): what the ``close`` helpers bound by 1."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float((np.abs(got - want) / (atol_rel * max(float(np.abs(want).max()), 1e-12) + rtol * np.abs(want) + 1e-300)).max())


def report(what, r):
    k = max(r, key=lambda q: r[q])
    print(f"ORACLE {what}: worst error / tolerance {r[k]:.3f} ({k}); logits-like and loss: " +
          ", ".join(f"{q} {v:.3f}" for q, v in r.items() if not q.startswith("grad ")))
    return r[k]


# ---- TIGER --------------------------------------------------------------------------------------------------------------------
def tiger_sites(cfg):
    return (2 + 4 * cfg["num_layers"]) + (2 + 6 * cfg["num_decoder_layers"])


@functools.lru_cache(maxsize=None)
def tiger_oracle(tag, p, c0, swapped=False):
    """-> dict(logits, loss, grads {name: array}, kink) after PASSES passes, float64."""
    z, cfg, arrays = model_fixture(tag)
    P = TO.params(arrays, cfg["tie_word_embeddings"], requires_grad=True)
    ctr = Counters(c0, p, tiger_sites(cfg), SWAP if swapped else None)
    kink = []
    for _ in range(PASSES):
        logits, loss = TO.forward(P, cfg, z["input_ids"], z["attention_mask"], z["labels"], float(z["temperature"]),
                                  drop=ctr.drop if p > 0 else None, kink=kink)
        loss.backward()
    assert p == 0 or ctr.calls == PASSES * ctr.sites
    assert len(kink) == PASSES * (cfg["num_layers"] + cfg["num_decoder_layers"])
    return dict(logits=logits.detach().numpy(), loss=loss.detach().numpy(), grads={n: t.grad.numpy() for n, t in P.items()},
                kink=min(kink))


@functools.lru_cache(maxsize=None)
def tiger_kernel(tag, p, c0):
    from torch_rechub_amd import ops
    from test_gpu_tiger import load_model
    z, cfg, model, (ids, mask, labels) = load_model(tag, dropout_rate=p)
    model.train()
    model.set_hyper(float(z["temperature"]))
    rng = set_rng(c0)
    for _ in range(PASSES):
        res = model(ids, attention_mask=mask, labels=labels)
        res.loss.backward()
    torch.cuda.synchronize()
    ops.check_errors()
    assert int(rng[1]) == c0 + (PASSES * tiger_sites(cfg) if p > 0 else 0), "dropout call counter"
    return dict(logits=res.logits.detach().cpu().numpy(), loss=res.loss.detach().cpu().numpy(),
                grads={n: q.grad.detach().cpu().numpy() for n, q in model.named_parameters()})


def tiger_ratios(got, want):
    r = {k: ratio(got[k], want[k], 2e-4, 2e-5) for k in ("logits", "loss")}
    assert got["grads"].keys() <= want["grads"].keys()
    r.update({"grad " + n: ratio(g, want["grads"][n], 2e-4, 2e-5) for n, g in got["grads"].items()})
    return r


@pytest.mark.parametrize("tag,p", [("a", 0.3), ("b", 0.1), ("a", 0.0)], ids=["a-p0.3", "b-p0.1", "a-p0-control"])
def test_tiger_two_training_passes_against_float64(tag, p):
    from test_gpu_tiger import close
    c0 = TIGER_C0[(tag, p)]
    want = tiger_oracle(tag, p, c0)
    assert want["kink"] >= KINK, f"C0 {c0}: a kept wi pre-activation sits {want['kink']:.2e} from the ReLU kink"
    got = tiger_kernel(tag, p, c0)
    report(f"TIGER {tag} p {p}", tiger_ratios(got, want))
    close(got["logits"], want["logits"], "logits")
    close(got["loss"], want["loss"], "loss")
    for n, g in got["grads"].items():
        close(g, want["grads"][n], n)


def test_tiger_misses_an_oracle_with_two_counters_swapped():
    tag, p = "a", 0.3
    c0 = TIGER_C0[(tag, p)]
    got = tiger_kernel(tag, p, c0)
    assert report(f"TIGER {tag} p {p}", tiger_ratios(got, tiger_oracle(tag, p, c0))) <= 1.0
    v = report(f"TIGER {tag} p {p} swapped counters", tiger_ratios(got, tiger_oracle(tag, p, c0, True)))
    assert v > 100.0, f"an oracle with two counters swapped is only {v:.1f} x the tolerance away"


# ---- SASRec -------------------------------------------------------------------------------------------------------------------
def sasrec_fixture():
    from conftest import load_golden
    gold = load_golden(f"model_sasrec_{SASREC_CFG}.npz")
    c = json.loads(str(gold["cfg"]))
    sd = {n[4:]: gold[n] for n in gold.files if n.startswith("sd0.")}
    sd["item_emb.embed_dict.seq.weight"] = sd["item_emb.embed_dict.seq.weight"][:, :c["D"]]
    return gold, c, sd


@functools.lru_cache(maxsize=None)
def sasrec_oracle(p, c0, swapped=False):
    gold, c, sd = sasrec_fixture()
    ctr = Counters(c0, p, 1 + 2 * c["blocks"], SWAP if swapped else None)
    grads, kink = None, float("inf")
    for _ in range(PASSES):
        res = SO.model_fwd_bwd(sd, gold["b0.seq"], gold["b0.pos"], gold["b0.neg"], c["H"], 1e-8, p, ctr.keep if p > 0 else None)
        grads = res["grads"] if grads is None else {n: g + res["grads"][n] for n, g in grads.items()}
        kink = min(kink, res["kink"])
    assert p == 0 or ctr.calls == PASSES * ctr.sites
    return dict(pos=res["pos"], neg=res["neg"], loss=np.float64(res["loss"]), grads=grads, kink=kink)


@functools.lru_cache(maxsize=None)
def sasrec_kernel(p, c0):
    from torch_rechub_amd import ops
    from test_gpu_sasrec import batch, load_model
    from torch_rechub_amd.basic.loss_func import BPRLoss
    gold, model = load_model(SASREC_CFG, dropout=p)
    model.train()
    x = batch(gold, 0)
    sites = 1 + 2 * len(model.attention_layers)
    rng = set_rng(c0)
    for _ in range(PASSES):
        pos, neg = model(x)
        loss = BPRLoss()(pos.reshape(-1), neg.reshape(-1))  # test_gpu_sasrec.probe_loss, keeping the logits
        loss.backward()
    torch.cuda.synchronize()
    ops.check_errors()
    assert int(rng[1]) == c0 + (PASSES * sites if p > 0 else 0), "dropout call counter"
    return dict(pos=pos.detach().cpu().numpy(), neg=neg.detach().cpu().numpy(), loss=loss.detach().cpu().numpy(),
                grads={n: q.grad.detach().cpu().numpy() for n, q in model.named_parameters()})


def _sasrec_grad(n, g, want):
    """(gradient's logical columns, atol fraction): test_probe_loss_and_gradients_match_the_reference's."""
    g = g[:, :want.shape[1]] if n.startswith("item_emb") else g
    return g, (1e-4 if want.ndim >= 2 and "emb" not in n else 1e-5)


def sasrec_ratios(got, want):
    r = {k: ratio(got[k], want[k], 1e-4, 1e-5) for k in ("pos", "neg")}
    r["loss"] = abs(float(got["loss"]) - float(want["loss"])) / (1e-5 * abs(float(want["loss"])))
    assert got["grads"].keys() == want["grads"].keys()
    for n, g in got["grads"].items():
        g, frac = _sasrec_grad(n, g, want["grads"][n])
        r["grad " + n] = ratio(g, want["grads"][n], 1e-4, frac)
    return r


@pytest.mark.parametrize("p", [0.5, 0.0], ids=["p0.5", "p0-control"])
def test_sasrec_two_training_passes_against_float64(p):
    from test_gpu_sasrec import close
    c0 = SASREC_C0[p]
    want = sasrec_oracle(p, c0)
    assert want["kink"] >= KINK, f"C0 {c0}: a kept conv1 output sits {want['kink']:.2e} from the ReLU kink"
    got = sasrec_kernel(p, c0)
    report(f"SASRec {SASREC_CFG} p {p}", sasrec_ratios(got, want))
    close(torch.from_numpy(got["pos"]), want["pos"], "pos_logits")
    close(torch.from_numpy(got["neg"]), want["neg"], "neg_logits")
    assert abs(float(got["loss"]) - float(want["loss"])) <= 1e-5 * abs(float(want["loss"])), (got["loss"], want["loss"])
    for n, g in got["grads"].items():
        g, frac = _sasrec_grad(n, g, want["grads"][n])
        close(torch.from_numpy(np.ascontiguousarray(g)), want["grads"][n], "grad " + n, frac)


def test_sasrec_misses_an_oracle_with_two_counters_swapped():
    p = 0.5
    c0 = SASREC_C0[p]
    got = sasrec_kernel(p, c0)
    assert report(f"SASRec {SASREC_CFG} p {p}", sasrec_ratios(got, sasrec_oracle(p, c0))) <= 1.0
    v = report(f"SASRec {SASREC_CFG} p {p} swapped counters", sasrec_ratios(got, sasrec_oracle(p, c0, True)))
    assert v > 100.0, f"an oracle with two counters swapped is only {v:.1f} x the tolerance away"


if __name__ == "__main__":
    # The reference side alone, no GPU: the kink margin for C0 = 1..12 (the chosen one marked) and how far the swapped counters
    # move the oracle itself, in units of the tolerance.
    for (tag, p), c0 in TIGER_C0.items():
        if p > 0:
            margins = {c: tiger_oracle(tag, p, c)["kink"] for c in range(1, 13)}
            r = tiger_ratios(tiger_oracle(tag, p, c0, True), tiger_oracle(tag, p, c0))
            print(f"TIGER {tag} p {p}: C0 {c0} margin {margins[c0]:.2e}" + ("" if margins[c0] >= KINK else "  <-- BELOW") +
                  f"  (C0 1..12: {' '.join(f'{m:.1e}' for m in margins.values())}); swapped counters {max(r.values()):.0f} x")
    for p, c0 in SASREC_C0.items():
        if p > 0:
            margins = {c: sasrec_oracle(p, c)["kink"] for c in range(1, 13)}
            r = sasrec_ratios(sasrec_oracle(p, c0, True), sasrec_oracle(p, c0))
            print(f"SASRec {SASREC_CFG} p {p}: C0 {c0} margin {margins[c0]:.2e}" + ("" if margins[c0] >= KINK else "  <-- BELOW") +
                  f"  (C0 1..12: {' '.join(f'{m:.1e}' for m in margins.values())}); swapped counters {max(r.values()):.0f} x")
