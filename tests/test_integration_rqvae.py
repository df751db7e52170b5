"""integration.enable() for the RQ-VAE: the reference's RQVAEModel, its quantizer classes, the rqvae Trainer and
EmbDataset are rebound to the HIP implementations and restored by disable() (skips without the reference)."""
import pytest
import torch

from oracle.ref_import import available, import_reference

pytestmark = pytest.mark.skipif(not available(), reason="needs the unmodified reference torch_rechub package (RECHUB_REFERENCE): not present")


def _names():
    import torch_rechub.models.generative as RG
    import torch_rechub.models.generative.rqvae as RQ
    import torch_rechub.trainers.rqvae_trainer as RT
    import torch_rechub.utils.data as RD
    return {"model": (RG, "RQVAEModel"), "model in its module": (RQ, "RQVAEModel"), "vq": (RQ, "VectorQuantizer"),
            "rvq": (RQ, "ResidualVectorQuantizer"), "trainer": (RT, "Trainer"), "data": (RD, "EmbDataset")}


def test_enable_rebinds_the_rqvae_names_and_disable_restores_them():
    import_reference()
    from torch_rechub_amd import integration
    from torch_rechub_amd.models.generative import rqvae as AQ
    from torch_rechub_amd.trainers.rqvae_trainer import Trainer
    from torch_rechub_amd.utils.data import EmbDataset
    ours = {"model": AQ.RQVAEModel, "model in its module": AQ.RQVAEModel, "vq": AQ.VectorQuantizer,
            "rvq": AQ.ResidualVectorQuantizer, "trainer": Trainer, "data": EmbDataset}
    names = _names()
    orig = {k: getattr(mod, attr) for k, (mod, attr) in names.items()}
    assert all(orig[k] is not ours[k] for k in ours)
    try:
        done = integration.enable()
        for k, (mod, attr) in names.items():
            assert getattr(mod, attr) is ours[k], k
        assert "torch_rechub.trainers.rqvae_trainer.Trainer" in done and "torch_rechub.utils.data.EmbDataset" in done
        from torch_rechub.models.generative import RQVAEModel
        torch.manual_seed(3)
        mine = RQVAEModel(in_dim=12, num_emb_list=[4, 3], e_dim=4, layers=[8], sk_epsilons=[0.0, 0.0]).state_dict()
    finally:
        integration.disable()
    for k, (mod, attr) in names.items():
        assert getattr(mod, attr) is orig[k], k
    try:  # the data sets are a level of their own
        assert "torch_rechub.utils.data.EmbDataset" not in integration.enable(data=False)
        assert names["data"][0].EmbDataset is orig["data"] and names["model"][0].RQVAEModel is ours["model"]
    finally:
        integration.disable()
    torch.manual_seed(3)
    ref = orig["model"](in_dim=12, num_emb_list=[4, 3], e_dim=4, layers=[8], sk_epsilons=[0.0, 0.0]).state_dict()
    assert list(ref) == list(mine)
    for k in ref:
        assert torch.equal(ref[k], mine[k]), k
