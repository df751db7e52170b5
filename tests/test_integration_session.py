"""integration.enable() for the session-based family: the unmodified reference NARM / STAMP / GRU4Rec classes are
rebound to the HIP implementations, build with the reference's state_dict keys and seeded initial tensors, and train on
the HIP path (skips without the reference)."""
import os
import subprocess
import sys

import pytest
import torch

from oracle.ref_import import available, import_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(not available(), reason="needs the unmodified reference torch_rechub package (RECHUB_REFERENCE): not present")


def _features(mod):
    # (the feature classes the reference's EmbeddingLayer tests against: those bound in its layers module)
    import torch_rechub.basic.layers as RL
    SequenceFeature, SparseFeature = RL.SequenceFeature, RL.SparseFeature
    hist = SequenceFeature("hist_item_id", vocab_size=50, embed_dim=16, pooling="concat", shared_with="item_id")
    item = SparseFeature("item_id", vocab_size=50, embed_dim=16)
    user = [SparseFeature("user_id", vocab_size=9, embed_dim=16)]
    neg = [SequenceFeature("neg_items", vocab_size=50, embed_dim=16, pooling="concat", shared_with="item_id")]
    return {"NARM": lambda c: c(hist, 12, 0.0, 0.0), "STAMP": lambda c: c(hist, 0.05, 0.1),
            "GRU4Rec": lambda c: c(user, [hist], [item], neg, user_params={"dims": [16]})}[mod]


def _reference_state(name, tmp_path):
    """The seeded state_dict of the reference class, built in a fresh interpreter (an earlier enable() / disable() cycle in
    this process leaves the reference's feature bindings such that its EmbeddingLayer builds no tables)."""
    out = os.path.join(str(tmp_path), "ref.pt")
    code = ("import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from oracle.ref_import import import_reference; import_reference()\n"
            "import torch_rechub.models.matching as RM; from test_integration_session import _features\n"
            "torch.manual_seed(5); torch.save(_features(%r)(getattr(RM, %r)).state_dict(), %r)\n"
            % (ROOT, os.path.join(ROOT, "tests"), name, name, out))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
    return torch.load(out)


@pytest.mark.parametrize("name", ["NARM", "STAMP", "GRU4Rec"])
def test_enable_rebinds_and_models_keep_the_reference_keys_and_initial_tensors(name, tmp_path):
    import_reference()
    import torch_rechub.models.matching as RM
    from torch_rechub_amd import integration
    from torch_rechub_amd.models import matching as AM
    orig = getattr(RM, name)
    ref = _reference_state(name, tmp_path)
    try:
        integration.enable()
        assert getattr(RM, name) is getattr(AM, name)
        torch.manual_seed(5)
        mine = _features(name)(getattr(RM, name)).state_dict()
    finally:
        integration.disable()
    assert getattr(RM, name) is orig
    assert list(ref) == list(mine)
    for k in ref:
        assert torch.equal(ref[k], mine[k]), k


@pytest.mark.gpu
def test_patched_reference_narm_trains_on_the_hip_path():
    import_reference()
    import torch_rechub.models.matching as RM
    import torch_rechub.trainers as RT
    from torch_rechub_amd import integration, ops
    try:
        integration.enable()
        torch.manual_seed(1)
        model = _features("NARM")(RM.NARM)
        trainer = RT.MatchTrainer(model, mode=2, device="cuda:0")
        seq = torch.randint(1, 50, (32, 6))
        seq[1:, 4:] = 0
        y = torch.randint(0, 50, (32,))
        calls = []
        orig = ops.catalogue_cross_entropy
        ops.catalogue_cross_entropy = lambda *a: calls.append(1) or orig(*a)
        try:
            loss = trainer.train_one_epoch([({"hist_item_id": seq}, y)])
        finally:
            ops.catalogue_cross_entropy = orig
        assert calls and loss > 0
    finally:
        integration.disable()
