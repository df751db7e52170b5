"""integration.enable() for SASRec: the unmodified reference classes SASRec and PointWiseFeedForward are rebound to the
HIP implementation and build with the reference's state_dict keys and seeded initial tensors (skips without the
reference; the rebound class on the GPU is tests/test_gpu_sasrec.py's subject)."""
import os
import subprocess
import sys

import pytest
import torch

from oracle.ref_import import available, import_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(not available(), reason="needs the unmodified reference torch_rechub package (RECHUB_REFERENCE): not present")


def _build(cls, SequenceFeature):
    """Width 16: a kernel width, so the item table draws from the generator exactly as the reference's does."""
    feas = [SequenceFeature("seq", vocab_size=30, embed_dim=16, pooling="concat"),
            SequenceFeature("pos", vocab_size=30, embed_dim=16, pooling="concat", shared_with="seq"),
            SequenceFeature("neg", vocab_size=30, embed_dim=16, pooling="concat", shared_with="seq")]
    return cls(feas, max_len=8, dropout_rate=0.25, num_blocks=2, num_heads=2)


def _reference_state(tmp_path):
    """The seeded state_dict of the reference class, built in a fresh interpreter (as test_integration_sine.py does)."""
    out = os.path.join(str(tmp_path), "ref.pt")
    code = ("import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from oracle.ref_import import import_reference; import_reference()\n"
            "import torch_rechub.models.matching as RM; from torch_rechub.basic.features import SequenceFeature\n"
            "from test_integration_sasrec import _build\n"
            "torch.manual_seed(5); torch.save(_build(RM.SASRec, SequenceFeature).state_dict(), %r)\n" %
            (ROOT, os.path.join(ROOT, "tests"), out))
    subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT)
    return torch.load(out)


def test_enable_rebinds_sasrec_and_keeps_the_reference_keys_and_initial_tensors(tmp_path):
    import_reference()
    import torch_rechub.basic.features as RF
    import torch_rechub.models.matching as RM
    import torch_rechub.models.matching.sasrec as RS
    from torch_rechub_amd import integration
    from torch_rechub_amd.models import matching as AM
    from torch_rechub_amd.models.matching import sasrec as AS
    orig, orig_ffn = RM.SASRec, RS.PointWiseFeedForward
    ref = _reference_state(tmp_path)
    try:
        integration.enable()
        assert RM.SASRec is AM.SASRec and RS.SASRec is AM.SASRec and RS.PointWiseFeedForward is AS.PointWiseFeedForward
        torch.manual_seed(5)
        mine = _build(RM.SASRec, RF.SequenceFeature).state_dict()
    finally:
        integration.disable()
    assert RM.SASRec is orig and orig is not AM.SASRec
    assert RS.PointWiseFeedForward is orig_ffn and orig_ffn is not AS.PointWiseFeedForward
    assert list(ref) == list(mine)
    for k in ref:
        assert torch.equal(ref[k], mine[k]), k
