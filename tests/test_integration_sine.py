"""integration.enable() for SINE: the unmodified reference class is rebound to the HIP implementation, builds with the
reference's state_dict keys and seeded initial tensors, and trains on the HIP path (skips without the reference)."""
import os
import subprocess
import sys

import pytest
import torch

from oracle.ref_import import available, import_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(not available(), reason="needs the unmodified reference torch_rechub package (RECHUB_REFERENCE): not present")


def _build(cls):
    return cls(["hist_item_id"], ["item_id"], ["neg_items"], 50, 16, 12, 6, 2, 7, temperature=0.1)


def _reference_state(tmp_path):
    """The seeded state_dict of the reference class, built in a fresh interpreter (as test_integration_session.py does)."""
    out = os.path.join(str(tmp_path), "ref.pt")
    code = ("import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from oracle.ref_import import import_reference; import_reference()\n"
            "import torch_rechub.models.matching as RM; from test_integration_sine import _build\n"
            "torch.manual_seed(5); torch.save(_build(RM.SINE).state_dict(), %r)\n" % (ROOT, os.path.join(ROOT, "tests"), out))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
    return torch.load(out)


def test_enable_rebinds_sine_and_keeps_the_reference_keys_and_initial_tensors(tmp_path):
    import_reference()
    import torch_rechub.models.matching as RM
    from torch_rechub_amd import integration
    from torch_rechub_amd.models import matching as AM
    orig = RM.SINE
    ref = _reference_state(tmp_path)
    try:
        integration.enable()
        assert RM.SINE is AM.SINE
        torch.manual_seed(5)
        mine = _build(RM.SINE).state_dict()
    finally:
        integration.disable()
    assert RM.SINE is orig and orig is not AM.SINE
    assert list(ref) == list(mine)
    for k in ref:
        assert torch.equal(ref[k], mine[k]), k


@pytest.mark.gpu
def test_patched_reference_sine_trains_on_the_hip_path():
    import_reference()
    import torch_rechub.models.matching as RM
    import torch_rechub.trainers as RT
    from torch_rechub_amd import integration, ops
    try:
        integration.enable()
        torch.manual_seed(1)
        model = _build(RM.SINE)
        with torch.no_grad():
            for table in (model.item_embedding, model.concept_embedding, model.position_embedding):
                table.weight.normal_(0, 0.1)
        trainer = RT.MatchTrainer(model, mode=2, optimizer_params={"lr": 1e-3, "weight_decay": 1e-6}, device="cuda:0")
        hist = torch.randint(1, 50, (32, 7))
        hist[1:, :3] = 0
        x = {"hist_item_id": hist, "item_id": torch.randint(1, 50, (32,)), "neg_items": torch.randint(1, 50, (32, 3))}
        calls = []
        orig = ops.sine_interests
        ops.sine_interests = lambda *a: calls.append(1) or orig(*a)
        before = model.concept_embedding.weight.detach().clone()
        try:
            loss = trainer.train_one_epoch([(x, torch.zeros(32, dtype=torch.long))])
        finally:
            ops.sine_interests = orig
        assert calls and loss > 0
        assert not torch.equal(before, model.concept_embedding.weight.detach().cpu())
    finally:
        integration.disable()
