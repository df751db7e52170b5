"""integration.enable() for the three two-tower models: the unmodified reference names FaceBookDSSM, YoutubeSBC and
dssm_senet.DSSM are rebound to the HIP implementations, build with the reference examples' constructor calls and the
reference's state_dict keys, and are restored by disable() (skips without the reference; the rebound classes on the GPU are
tests/test_gpu_twotower.py's subject)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle.ref_import import available, import_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.skipif(not available(), reason="needs the unmodified reference torch_rechub package (RECHUB_REFERENCE): not present")


def _features(F):
    user = [F.SparseFeature("user_id", vocab_size=40, embed_dim=16), F.SparseFeature("gender", vocab_size=3, embed_dim=16),
            F.SequenceFeature("hist_cate_id", vocab_size=9, embed_dim=16, pooling="mean")]
    item = [F.SparseFeature("item_id", vocab_size=60, embed_dim=16), F.SparseFeature("cate_id", vocab_size=9, embed_dim=16)]
    neg = [F.SparseFeature("neg_item_id", vocab_size=60, embed_dim=16, shared_with="item_id"),
           F.SparseFeature("neg_cate_id", vocab_size=9, embed_dim=16, shared_with="cate_id")]
    return user, item, neg, [F.DenseFeature("sample_weight")]


def _build_all(RM, RS, F):
    """The constructor calls of examples/matching/run_ml_facebook_dssm.py, run_ml_youtube_sbc.py and a SENet DSSM script."""
    user, item, neg, weight = _features(F)
    tower = {"dims": [32, 16]}
    return (RM.FaceBookDSSM(user, item, neg, temperature=0.02, user_params=dict(tower), item_params=dict(tower)),
            RM.YoutubeSBC(user, item, weight, user_params=dict(tower), item_params=dict(tower), batch_size=32, n_neg=3,
                          temperature=0.02),
            RS.DSSM(user, item, temperature=0.02, user_params=dict(tower, activation="prelu"),
                    item_params=dict(tower, activation="prelu")))


def _reference_facts():
    """state_dict keys of the three reference classes and YoutubeSBC's index arrays, from a fresh interpreter (as
    test_integration_sasrec.py does: earlier tests of this process may have left reference modules rebound)."""
    code = ("import sys, json; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "from oracle.ref_import import import_reference; import_reference()\n"
            "import torch_rechub.basic.features as RF, torch_rechub.models.matching as RM\n"
            "import torch_rechub.models.matching.dssm_senet as RS\n"
            "from test_integration_twotower import _build_all\n"
            "ms = _build_all(RM, RS, RF)\n"
            "print(json.dumps({'keys': [list(m.state_dict()) for m in ms], 'index0': ms[1].index0.tolist(),"
            " 'index1': ms[1].index1.tolist()}))\n" % (ROOT, os.path.join(ROOT, "tests")))
    out = subprocess.run([sys.executable, "-c", code], check=True, cwd=ROOT, capture_output=True, text=True).stdout
    return json.loads(out.strip().splitlines()[-1])


def test_enable_rebinds_the_three_two_tower_models_and_disable_restores_them():
    import_reference()
    import torch_rechub.basic.features as RF
    import torch_rechub.models.matching as RM
    import torch_rechub.models.matching.dssm_facebook as RFB
    import torch_rechub.models.matching.dssm_senet as RS
    import torch_rechub.models.matching.youtube_sbc as RY
    from torch_rechub_amd import integration
    from torch_rechub_amd.models import matching as AM
    orig = (RM.FaceBookDSSM, RM.YoutubeSBC, RS.DSSM, RM.DSSM)
    ref = _reference_facts()
    try:
        integration.enable()
        assert RM.FaceBookDSSM is AM.FaceBookDSSM and RFB.FaceBookDSSM is AM.FaceBookDSSM
        assert RM.YoutubeSBC is AM.YoutubeSBC and RY.YoutubeSBC is AM.YoutubeSBC
        assert RS.DSSM is AM.DSSMSENet and RM.DSSM is AM.DSSM and AM.DSSM is not AM.DSSMSENet
        models = _build_all(RM, RS, RF)
    finally:
        integration.disable()
    assert (RM.FaceBookDSSM, RM.YoutubeSBC, RS.DSSM, RM.DSSM) == orig
    assert RFB.FaceBookDSSM is orig[0] and RY.YoutubeSBC is orig[1]
    assert [type(m) for m in models] == [AM.FaceBookDSSM, AM.YoutubeSBC, AM.DSSMSENet]
    assert [list(m.state_dict()) for m in models] == ref["keys"]
    sbc, senet = models[1], models[2]
    assert np.array_equal(sbc.index0, ref["index0"]) and np.array_equal(sbc.index1, ref["index1"])
    assert (senet.user_num_features, senet.item_num_features) == (3, 2) and senet.user_senet.fused
