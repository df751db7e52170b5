"""integration.enable() / disable() for HLLM: HLLMModel and HLLMTransformerBlock of the unmodified reference are rebound to
the HIP implementations and restored afterwards; state_dict keys, shapes and seeded initial tensors equal the reference's
(skips without the reference)."""
import pytest

from oracle.ref_import import available, import_reference

pytestmark = pytest.mark.skipif(not available(), reason="needs the unmodified reference torch_rechub package (RECHUB_REFERENCE): not present")


def test_enable_rebinds_and_disable_restores_hllm():
    import_reference()
    import torch_rechub.models.generative as RG
    import torch_rechub.models.generative.hllm as RH
    from torch_rechub_amd import integration
    from torch_rechub_amd.models.generative import HLLMModel
    from torch_rechub_amd.models.generative.hllm import HLLMTransformerBlock
    orig = (RG.HLLMModel, RH.HLLMModel, RH.HLLMTransformerBlock, RG.HSTUModel)
    try:
        names = integration.enable()
        for n in ("torch_rechub.models.generative.HLLMModel", "torch_rechub.models.generative.hllm.HLLMTransformerBlock",
                  "torch_rechub.models.generative.HSTUModel"):
            assert n in names, n
        assert RG.HLLMModel is HLLMModel and RH.HLLMModel is HLLMModel and RH.HLLMTransformerBlock is HLLMTransformerBlock
    finally:
        integration.disable()
    assert (RG.HLLMModel, RH.HLLMModel, RH.HLLMTransformerBlock, RG.HSTUModel) == orig


def test_state_dict_keys_and_shapes_match_the_reference():
    import_reference()
    import torch
    from torch_rechub.models.generative.hllm import HLLMModel as Ref

    from torch_rechub_amd.models.generative import HLLMModel
    emb = torch.randn(60, 24, generator=torch.Generator().manual_seed(1))
    for kw in (dict(), dict(use_rel_pos_bias=False), dict(use_time_embedding=False), dict(time_bucket_fn="log", n_heads=3)):
        args = dict(item_embeddings=emb, vocab_size=60, d_model=24, n_heads=2, n_layers=2, max_seq_len=16, num_time_buckets=8)
        args.update(kw)
        torch.manual_seed(3)
        ref = Ref(**args)
        torch.manual_seed(3)
        mine = HLLMModel(**args)
        rs, ms = ref.state_dict(), mine.state_dict()
        assert list(rs) == list(ms)
        for k in rs:  # same shapes and the same seeded initial tensors (parameter creation order)
            assert torch.equal(rs[k], ms[k]), k
        assert [n for n, _ in ref.named_parameters()] == [n for n, _ in mine.named_parameters()]
        ref.load_state_dict(ms)  # checkpoints load both ways
        mine.load_state_dict(rs)
        t = torch.randint(0, 10**6, (3, 7))
        assert torch.equal(ref._time_diff_to_bucket(t), mine._time_diff_to_bucket(t))
