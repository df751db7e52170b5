"""integration.enable() / disable() for the generative family: HSTULayer, HSTUBlock, HSTUModel and SeqTrainer of the
unmodified reference are rebound to the HIP implementations and restored afterwards (skips without the reference)."""
import pytest

from oracle.ref_import import available, import_reference

pytestmark = pytest.mark.skipif(not available(), reason="needs the unmodified reference torch_rechub package (RECHUB_REFERENCE): not present")


def test_enable_rebinds_and_disable_restores_the_generative_family():
    import_reference()
    import torch_rechub.basic.layers as RL
    import torch_rechub.models.generative.hstu as RH
    import torch_rechub.trainers as RT
    import torch_rechub.trainers.seq_trainer as RS
    from torch_rechub_amd import integration
    from torch_rechub_amd.basic import layers as AL
    from torch_rechub_amd.models.generative import HSTUModel
    from torch_rechub_amd.trainers import SeqTrainer
    orig = (RL.HSTULayer, RL.HSTUBlock, RH.HSTUModel, RH.HSTUBlock, RT.SeqTrainer, RS.SeqTrainer)
    try:
        names = integration.enable()
        for n in ("torch_rechub.basic.layers.HSTULayer", "torch_rechub.basic.layers.HSTUBlock",
                  "torch_rechub.models.generative.HSTUModel", "torch_rechub.trainers.SeqTrainer"):
            assert n in names, n
        assert RL.HSTULayer is AL.HSTULayer and RL.HSTUBlock is AL.HSTUBlock and RH.HSTUBlock is AL.HSTUBlock
        import torch_rechub.models.generative as RG
        assert RG.HSTUModel is HSTUModel and RT.SeqTrainer is SeqTrainer and RS.SeqTrainer is SeqTrainer
    finally:
        integration.disable()
    assert (RL.HSTULayer, RL.HSTUBlock, RH.HSTUModel, RH.HSTUBlock, RT.SeqTrainer, RS.SeqTrainer) == orig


def test_state_dict_keys_and_shapes_match_the_reference():
    import_reference()
    import torch
    from torch_rechub.models.generative.hstu import HSTUModel as Ref

    from torch_rechub_amd.models.generative import HSTUModel
    for kw in (dict(), dict(tie_embeddings=False, use_output_bias=False), dict(use_time_embedding=False)):
        args = dict(vocab_size=60, d_model=24, n_heads=2, n_layers=2, dqk=12, dv=10, max_seq_len=16, num_time_buckets=8,
                    **kw)
        torch.manual_seed(3)
        ref = Ref(**args).state_dict()
        torch.manual_seed(3)
        mine = HSTUModel(**args).state_dict()
        assert list(ref) == list(mine)
        for k in ref:  # same shapes and the same seeded initial tensors (parameter init order)
            assert torch.equal(ref[k], mine[k]), k
