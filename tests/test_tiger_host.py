"""TIGER without a GPU: the host-built bucket table against the reference's recording, the float64 oracle
(tests/tiger_oracle.py) against the three fixtures of tools/gen_golden_tiger.py, the model's state_dict layout, and the
data helpers (TigerSeqDataset, Trie, the collate function) on the reference's own two-user example."""
import importlib.util
import json
import os
import re

import numpy as np
import pytest
import torch

import tiger_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RTOL = 1e-9
F32 = torch.float32  # the reference takes the RMS norm's variance in float32 at any model dtype (tiger_oracle.rms_norm)


def load(name):
    return np.load(os.path.join(GOLDEN, name))


def model_fixture(tag):
    z = load(f"model_tiger_{tag}.npz")
    cfg = json.loads(str(z["cfg"]))
    arrays = {k[len("param/"):]: z[k] for k in z.files if k.startswith("param/")}
    # the recording holds each parameter once; the state_dict's other names of the embedding are that array again
    arrays = {k: arrays.get(k, arrays["shared.weight"]) for k in json.loads(str(z["keys"]))}
    return z, cfg, arrays


def near(got, want, what, rtol=RTOL):
    """The fixtures record the reference at float64: rtol 1e-9, with 1e-9 of the tensor's largest value as the floor."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=rtol * max(float(np.abs(want).max()), 1e-300), err_msg=what)


# ---- buckets ----------------------------------------------------------------------------------------------------------------
def test_bucket_table_equals_the_recording_at_every_distance():
    from torch_rechub_amd import ops
    z = load("tiger_layers.npz")
    rel = z["bucket.rel"]
    assert rel[0] == -1100 and rel[-1] == 1100
    for nb, md in z["bucket.cfgs"]:
        for bi in (True, False):
            want = z[f"bucket.{nb}_{md}_{int(bi)}"]
            # one table holds distances -(Lq - 1) .. Lk - 1: Lq = Lk = 1024 covers -1023..1023, and the two rectangular
            # extremes the distances beyond
            for Lq, Lk in ((1024, 1024), (1, 1024), (1024, 1), (5, 80), (1, 1)):
                table = ops.t5_relative_buckets(Lq, Lk, bi, int(nb), int(md))
                assert table.dtype == torch.int32 and table.shape == (Lq + Lk - 1,)
                lo = -(Lq - 1)
                np.testing.assert_array_equal(table.numpy(), want[lo + 1100:lo + 1100 + Lq + Lk - 1], err_msg=f"{nb} {md} {bi}")
            got = ops._t5_bucket_of(torch.as_tensor(rel.astype(np.int64)), bi, int(nb), int(md))
            np.testing.assert_array_equal(got.numpy(), want)
            np.testing.assert_array_equal(O.buckets(rel, bi, int(nb), int(md)), want)
    assert ops.t5_relative_buckets(5, 80, True, 32, 128) is ops.t5_relative_buckets(5, 80, True, 32, 128)  # cached


# ---- the oracle against the layer fixture ---------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["enc", "dec", "cross"])
def test_oracle_reproduces_the_recorded_attention(kind):
    z = load("tiger_layers.npz")
    cfg = json.loads(str(z["attn.cfg"]))
    H = cfg["num_heads"]
    pre = f"attn.{kind}."
    P = {n: torch.tensor(z[pre + "param." + n + ".weight"], dtype=torch.float64, requires_grad=True) for n in "qkvo"}
    table = None
    if pre + "param.relative_attention_bias.weight" in z.files:
        table = torch.tensor(z[pre + "param.relative_attention_bias.weight"], dtype=torch.float64, requires_grad=True)
    x = torch.tensor(z[pre + "x"], dtype=torch.float64, requires_grad=True)
    kv = torch.tensor(z[pre + "kv"], dtype=torch.float64, requires_grad=True) if kind == "cross" else x
    mask = None if kind == "dec" else z["attn.key_mask"][:x.shape[0]]
    a = O.attention(x @ P["q"].T, kv @ P["k"].T, kv @ P["v"].T, H, mask, kind == "dec", table, kind != "dec",
                    cfg["max_distance"])
    out = a @ P["o"].T
    (out * torch.tensor(z[pre + "gout"], dtype=torch.float64)).sum().backward()
    near(out.detach(), z[pre + "out"], "out")
    near(x.grad, z[pre + "g_x"], "g_x")
    if kind == "cross":
        near(kv.grad, z[pre + "g_kv"], "g_kv")
    for n in "qkvo":
        near(P[n].grad, z[pre + f"grad.{n}.weight"], n)
    if table is not None:
        near(table.grad, z[pre + "grad.relative_attention_bias.weight"], "table")
    if kind != "dec":  # the recorded weights: one valid key -> weight 1 on it; no valid key -> 1 / Lk on every key
        w = z[pre + "weights"]
        assert np.all(w[1, :, :, 0] == 1.0) and np.all(w[1, :, :, 1:] == 0.0)
        assert np.all(w[2] == 1.0 / w.shape[-1])
        assert np.all(w[3, :, :, :3] == 0.0)


# ---- the oracle against the model fixtures --------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["a", "b"])
def model_case(request):
    z, cfg, arrays = model_fixture(request.param)
    P = O.params(arrays, cfg["tie_word_embeddings"], requires_grad=True)
    return z, cfg, P


def test_oracle_reproduces_forward_losses_and_gradients(model_case):
    z, cfg, P = model_case
    ids, mask, labels = z["input_ids"], z["attention_mask"], z["labels"]
    logits, loss1 = O.forward(P, cfg, ids, mask, labels, 1.0, vdt=F32)
    near(logits.detach(), z["logits"], "logits")
    near(loss1.detach(), z["loss_t1"], "loss at temperature 1")
    _, loss = O.forward(P, cfg, ids, mask, labels, float(z["temperature"]), vdt=F32)
    near(loss.detach(), z["loss_t"], "loss at the temperature")
    loss.backward()
    names = [k[len("grad/"):] for k in z.files if k.startswith("grad/")]
    assert names
    for n in names:
        near(P[n].grad, z["grad/" + n], n)


def test_oracle_reproduces_the_beam_search(model_case):
    from torch_rechub_amd.utils.data import Trie
    z, cfg, P = model_case
    trie = Trie(z["beam.candidates"].tolist())
    seqs, scores = O.beam_search(P, cfg, z["input_ids"], z["attention_mask"], trie.def_prefix_allowed_tokens_fn(trie), 3, vdt=F32)
    np.testing.assert_array_equal(seqs, z["beam.sequences"])
    near(scores, z["beam.scores"], "beam scores")
    assert np.abs(np.diff(z["beam.scores"].reshape(-1, 3), axis=1)).min() > 1e-3


def test_oracle_adamw_steps(model_case):
    z, cfg, P = model_case
    leaves = list({id(t): t for t in P.values()}.values())
    opt = torch.optim.AdamW(leaves, lr=float(z["lr"]))
    losses = []
    for _ in range(3):
        opt.zero_grad()
        _, loss = O.forward(P, cfg, z["input_ids"], z["attention_mask"], z["labels"], float(z["temperature"]), vdt=F32)
        losses.append(float(loss.detach()))
        loss.backward()
        opt.step()
    near(losses, z["step_losses"], "AdamW losses")


# ---- the model's layout -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b"])
def test_state_dict_layout_and_strict_loading(tag):
    from torch_rechub_amd.models.generative import TIGERConfig, TIGERModel
    z, cfg, arrays = model_fixture(tag)
    model = TIGERModel(TIGERConfig.from_dict(cfg))
    want = json.loads(str(z["keys"]))
    sd = model.state_dict()
    assert list(sd.keys()) == list(want.keys())
    assert {k: list(v.shape) for k, v in sd.items()} == want
    model.load_state_dict({k: torch.tensor(v) for k, v in arrays.items()}, strict=True)
    for k, v in arrays.items():
        assert np.array_equal(model.state_dict()[k].numpy(), v), k
    tied = ["shared.weight", "encoder.embed_tokens.weight", "decoder.embed_tokens.weight"]
    if cfg["tie_word_embeddings"]:
        tied.append("lm_head.weight")
    assert len({model.state_dict()[k].data_ptr() for k in tied}) == 1
    if not cfg["tie_word_embeddings"]:
        assert model.lm_head.weight.data_ptr() != model.shared.weight.data_ptr()
    assert len(list(model.parameters())) == len([k for k in z.files if k.startswith("grad/")])
    rel = [k for k in sd if "relative_attention_bias" in k]
    assert rel == ["encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight",
                   "decoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight"]


def test_config_from_dict_and_refusals():
    from torch_rechub_amd.models.generative import TIGERConfig, TIGERModel
    cfg = TIGERConfig.from_dict({"vocab_size": 11, "d_model": 8, "d_kv": 3, "d_ff": 5, "num_layers": 1, "num_heads": 2,
                                 "model_type": "t5", "architectures": ["T5ForConditionalGeneration"], "use_cache": True})
    assert cfg.num_decoder_layers == 1 and cfg.vocab_size == 11 and cfg.decoder_start_token_id == 0
    with pytest.raises(ValueError, match="gated"):
        TIGERConfig.from_dict({"feed_forward_proj": "gated-gelu"})
    model = TIGERModel(cfg)
    model.set_hyper(0.7)
    assert model.temperature == 0.7
    shifted = model._shift_right(torch.tensor([[5, 6, -100], [7, -100, -100]]))
    assert shifted.tolist() == [[0, 5, 6], [0, 7, 0]]
    with pytest.raises(RuntimeError, match="HIP"):  # no CPU path
        model(torch.tensor([[1, 2]]), labels=torch.tensor([[3, 1]]))


@pytest.mark.skipif(importlib.util.find_spec("transformers") is None, reason="transformers is not installed")
def test_from_t5_copies_config_and_weights():
    from transformers.models.t5.configuration_t5 import T5Config
    from transformers.models.t5.modeling_t5 import T5ForConditionalGeneration

    from torch_rechub_amd.models.generative import TIGERModel
    z, cfg, arrays = model_fixture("b")
    ref = T5ForConditionalGeneration(T5Config(**cfg))
    ref.load_state_dict({k: torch.tensor(v) for k, v in arrays.items()})
    ref.temperature = 0.7
    model = TIGERModel.from_t5(ref)
    assert model.temperature == 0.7 and model.config.d_kv == 5
    assert model.config.tie_word_embeddings == ref.config.tie_word_embeddings and model.config.num_decoder_layers == 2
    for k, v in ref.state_dict().items():
        assert torch.equal(model.state_dict()[k], v), k


@pytest.mark.skipif(importlib.util.find_spec("transformers") is None, reason="transformers is not installed")
def test_from_t5_refuses_a_t5_that_ties_without_rescaling():
    """A plain T5 whose config ties the embeddings but does not rescale the decoder output computes another function than
    the reference's TIGERModel (which rescales whenever tie_word_embeddings is set): refused, not copied."""
    from transformers.models.t5.configuration_t5 import T5Config
    from transformers.models.t5.modeling_t5 import T5ForConditionalGeneration

    from torch_rechub_amd.models.generative import TIGERModel
    cfg = T5Config(vocab_size=11, d_model=8, d_kv=3, d_ff=5, num_layers=1, num_heads=2, feed_forward_proj="relu",
                   tie_word_embeddings=False)
    ref = T5ForConditionalGeneration(cfg)
    if getattr(cfg, "scale_decoder_outputs", None) is False and cfg.tie_word_embeddings:
        with pytest.raises(ValueError, match="rescale"):
            TIGERModel.from_t5(ref)
    else:  # a transformers that honours the field: an untied copy with its own head
        model = TIGERModel.from_t5(ref)
        assert not model.config.tie_word_embeddings and model.lm_head.weight.data_ptr() != model.shared.weight.data_ptr()


def test_model_output_attributes():
    from torch_rechub_amd.models.generative.tiger import ModelOutput
    out = ModelOutput(loss=None, logits=3)
    assert out.logits == 3 and out["logits"] == 3 and out.loss is None
    with pytest.raises(AttributeError):
        out.logit


# ---- data helpers: the reference's two-user example -----------------------------------------------------------------------
INTERS = {"u0": [1, 2, 3, 4, 5], "u1": [2, 3, 4, 5, 6]}
INDICES = {"1": ["<a_0>", "<b_0>"], "2": ["<a_0>", "<b_1>"], "3": ["<a_1>", "<b_0>"], "4": ["<a_1>", "<b_1>"],
           "5": ["<a_2>", "<b_0>"], "6": ["<a_2>", "<b_1>"]}


class StubTokenizer:
    """Each ``<x_y>`` token gets the next positive id; pads with 0; what ``get_collate_fn`` calls, nothing more."""
    pad_token_id = 0
    eos_token_id = 1
    model_max_length = 64

    def __init__(self):
        self.vocab = {}

    def ids(self, text):
        return [self.vocab.setdefault(tok, len(self.vocab) + 2) for tok in re.findall(r"<[^>]*>", text)]

    def __call__(self, texts, return_tensors=None, padding=None, max_length=None, truncation=None, return_attention_mask=None):
        if isinstance(texts, str):
            return {"input_ids": self.ids(texts)}
        seqs = [self.ids(t)[:max_length] for t in texts]
        width = max(len(s) for s in seqs)
        return {"input_ids": torch.tensor([s + [0] * (width - len(s)) for s in seqs]),
                "attention_mask": torch.tensor([[1] * len(s) + [0] * (width - len(s)) for s in seqs])}


def test_dataset_modes_and_truncation():
    from torch_rechub_amd.utils.data import TigerSeqDataset
    train = TigerSeqDataset(INTERS, INDICES, max_his_len=20, mode="train")
    assert len(train) == 4  # items[:-2] keeps three items per user: two (history, next) pairs each
    assert train[0] == {"input_ids": "<a_0><b_0>", "labels": "<a_0><b_1>"}
    assert train[1] == {"input_ids": "<a_0><b_0><a_0><b_1>", "labels": "<a_1><b_0>"}
    assert train[4] == train[0]  # the index wraps
    valid = TigerSeqDataset(INTERS, INDICES, max_his_len=20, mode="valid")
    test = TigerSeqDataset(INTERS, INDICES, max_his_len=20, mode="test")
    assert len(valid) == 2 and len(test) == 2
    assert valid[0]["labels"] == "<a_1><b_1>" and test[0]["labels"] == "<a_2><b_0>"
    assert test[0]["input_ids"] == "<a_0><b_0><a_0><b_1><a_1><b_0><a_1><b_1>"
    assert TigerSeqDataset(INTERS, INDICES, max_his_len=1, mode="test")[0]["input_ids"] == "<a_1><b_1>"
    assert len(TigerSeqDataset(INTERS, INDICES, max_his_len=20, mode="test", sample_num=1)) == 1
    with pytest.raises(NotImplementedError):
        TigerSeqDataset(INTERS, INDICES, max_his_len=20, mode="other")


def test_dataset_tokens_items_and_level_constraint():
    from torch_rechub_amd.utils.data import TigerSeqDataset
    data = TigerSeqDataset(INTERS, INDICES, max_his_len=20, mode="train")
    assert data.get_new_tokens() == ["<a_0>", "<a_1>", "<a_2>", "<b_0>", "<b_1>"]
    items = data.get_all_items()
    assert "<a_0><b_0>" in items and len(items) == 6
    tok = StubTokenizer()
    fn = data.get_prefix_allowed_tokens_fn(tok)
    a_ids = {tok.vocab[t] for t in ("<a_0>", "<a_1>", "<a_2>")}
    b_ids = {tok.vocab[t] for t in ("<b_0>", "<b_1>")}
    assert set(fn(0, torch.tensor([0]))) == a_ids
    assert set(fn(0, torch.tensor([0, min(a_ids)]))) == b_ids
    assert fn(0, torch.tensor([0, min(a_ids), min(b_ids)])) == [tok.eos_token_id]


def test_collate_pads_and_masks_label_slots():
    from torch_rechub_amd.utils.data import TigerSeqDataset
    collate = TigerSeqDataset(INTERS, INDICES, max_his_len=20, mode="train").get_collate_fn(StubTokenizer())
    out = collate([{"input_ids": "<a_0><b_0>", "labels": "<a_0>"},
                   {"input_ids": "<a_0><b_0><a_1>", "labels": "<a_0><b_1><c_2>"}])
    assert out["input_ids"].shape == (2, 3) and out["attention_mask"][0].tolist() == [1, 1, 0]
    assert out["labels"].shape == (2, 3) and out["labels"][0].tolist()[1:] == [-100, -100]
    assert int((out["labels"] == 0).sum()) == 0


def test_trie_continuations():
    from torch_rechub_amd.utils.data import Trie
    trie = Trie([[0, 10, 20], [0, 10, 21], [0, 11, 30]])
    assert sorted(trie.get([0, 10])) == [20, 21] and sorted(trie.get([0])) == [10, 11] and trie.get([]) == [0]
    assert trie.get([0, 10, 20]) == [] and trie.get([0, 12]) == [] and trie[[0, 11]] == [30]
    assert len(trie) == 3 and sorted(trie) == [[0, 10, 20], [0, 10, 21], [0, 11, 30]]
    fn = trie.def_prefix_allowed_tokens_fn(trie)
    assert sorted(fn(0, torch.tensor([0, 10]))) == [20, 21]
    trie.add([1, 2])
    assert len(trie) == 4 and len(Trie.load_from_dict(trie.trie_dict)) == 4
    other = Trie([[7, 8]])
    trie.append(other, 1)
    assert sorted(trie.get([])) == [0, 7] and trie.get([7]) == [8]


def test_integration_does_not_rebind_tiger():
    """The reference TIGERModel is a transformers PreTrainedModel (Trainer, from_pretrained): enable() leaves it alone;
    TIGERModel.from_t5 is the bridge."""
    from torch_rechub_amd import integration
    from torch_rechub_amd.models import generative
    assert "TIGERModel" not in integration._MODELS["generative"]
    assert hasattr(generative, "TIGERModel") and hasattr(generative, "TIGERConfig") and hasattr(generative.TIGERModel, "from_t5")


# ---- the oracle's dropout sites (tests/test_gpu_seq_models_dropout_oracle.py runs the model against it) ------------------
def test_an_all_ones_drop_reproduces_the_undropped_oracle_exactly_and_visits_the_sites_in_program_order(model_case):
    z, cfg, P = model_case
    ids, mask, labels = z["input_ids"], z["attention_mask"], z["labels"]
    B, L, T = ids.shape[0], ids.shape[1], labels.shape[1]
    H, D, F = cfg["num_heads"], cfg["d_model"], cfg["d_ff"]
    shapes, kink = [], []

    def drop(shape):
        shapes.append(tuple(shape))
        return torch.ones(shape, dtype=torch.float64)

    for t in {id(t): t for t in P.values()}.values():
        t.grad = None
    logits0, loss0 = O.forward(P, cfg, ids, mask, labels, 0.7)
    loss0.backward()
    grads0 = {n: t.grad.clone() for n, t in P.items()}
    for t in {id(t): t for t in P.values()}.values():
        t.grad = None
    logits1, loss1 = O.forward(P, cfg, ids, mask, labels, 0.7, drop=drop, kink=kink)
    loss1.backward()
    assert torch.equal(logits0, logits1) and torch.equal(loss0, loss1)
    assert all(torch.equal(grads0[n], P[n].grad) for n in P)
    enc = [(B, L, D)] + [(B, H, L, L), (B, L, D), (B, L, F), (B, L, D)] * cfg["num_layers"] + [(B, L, D)]
    dec = [(B, T, D)] + [(B, H, T, T), (B, T, D), (B, H, T, L), (B, T, D), (B, T, F), (B, T, D)] * cfg["num_decoder_layers"] \
        + [(B, T, D)]
    assert shapes == enc + dec
    assert len(kink) == cfg["num_layers"] + cfg["num_decoder_layers"] and all(0 < m < 1 for m in kink)
    for t in {id(t): t for t in P.values()}.values():
        t.grad = None
