"""Generate the DeepFFM / FAT-DeepFFM fixtures of tests/golden/ from the UNMODIFIED reference (CPU).

Run where the reference checkout exists:  ``python tools/gen_golden_ffm.py``
Uses oracle/gen_golden.py's recipe (seed 2022, dropout 0, B = 48, three batches through the reference ``CTRTrainer``)
by importing it: its ``gen_model`` runs with this file's model builder in place of its own.

  model_deepffm.npz         DeepFFM, F = 6 cross fields of width 16, width-1 linear features
  model_deepffm_criteo.npz  DeepFFM at the Criteo example's widths (linear 1, cross 10: both PaddedEmbedding tables)
  model_fatdeepffm.npz      FatDeepFFM, F = 6, width 16, reduction_ratio 3
  ffm_layers.npz            FFM (reduce_sum False / True) and CEN: inputs, parameters, outputs, gradients

Cross vocabularies are v * F (the reference's field-aware tables, examples/ranking/run_criteo.py:77-80) and the batch
indices are drawn below v (the linear features, drawn first, share the names).  The archives are written with a fixed
member timestamp, so the files regenerate byte-identically.
"""
import os
import sys
import zipfile

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as G  # noqa: E402
from oracle.ref_import import import_reference  # noqa: E402

VOCABS = [3, 4, 10, 27, 105, 305]
CONFIGS = {"deepffm": (16, None), "deepffm_criteo": (10, None), "fatdeepffm": (16, 3)}


def build_ffm_model(rh, cfg):
    from torch_rechub.basic.features import SparseFeature
    from torch_rechub.models.ranking import DeepFFM, FatDeepFFM
    D, ratio = CONFIGS[cfg]
    F = len(VOCABS)
    linear = [SparseFeature(f"C{i + 1}", vocab_size=v, embed_dim=1) for i, v in enumerate(VOCABS)]
    cross = [SparseFeature(f"C{i + 1}", vocab_size=v * F, embed_dim=D) for i, v in enumerate(VOCABS)]
    mlp = {"dims": [32, 16], "dropout": 0.0, "activation": "relu"}
    if ratio is None:
        model = DeepFFM(linear, cross, D, mlp)
    else:
        model = FatDeepFFM(linear, cross, D, ratio, mlp)
    return model, {"linear_features": linear, "cross_features": cross}


def gen_ffm_layers():
    from torch_rechub.basic.layers import CEN, FFM
    torch.manual_seed(G.SEED)
    g = torch.Generator().manual_seed(G.SEED)
    out = {}
    B, F, D = 37, 6, 10
    P = F * (F - 1) // 2
    x = torch.randn(B, F, F, D, generator=g)
    for rs in (False, True):
        xi = x.clone().requires_grad_(True)
        y = FFM(F, reduce_sum=rs)(xi)
        gy = torch.randn(y.shape, generator=g)
        y.backward(gy)
        k = f"ffm_rs{int(rs)}."
        out[k + "x"], out[k + "out"], out[k + "g_out"], out[k + "g_x"] = G.npy(x), G.npy(y), G.npy(gy), G.npy(xi.grad)
    cen = CEN(D, P, 3)
    cen.train()
    em = torch.randn(B, P, D, generator=g).requires_grad_(True)
    y = cen(em)
    gy = torch.randn(y.shape, generator=g)
    y.backward(gy)
    out["cen.em"], out["cen.out"], out["cen.g_out"], out["cen.g_em"] = G.npy(em), G.npy(y), G.npy(gy), G.npy(em.grad)
    for n, t in cen.state_dict().items():
        out["cen.sd." + n] = G.npy(t)
    for n, p in cen.named_parameters():
        out["cen.grad." + n] = G.npy(p.grad)
    return out


def _save_fixed(path, arrays=None, **kw):
    """np.savez_compressed with a fixed member timestamp (byte-identical regeneration)."""
    arrays = dict(arrays or {}, **kw)
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as zf:
        for name, arr in arrays.items():
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, "w", force_zip64=True) as fh:
                np.lib.format.write_array(fh, np.asanyarray(arr), allow_pickle=False)


def main():
    rh = import_reference()
    saved = (G.build_model, np.savez_compressed)
    G.build_model = build_ffm_model
    np.savez_compressed = _save_fixed
    try:
        for cfg in CONFIGS:
            G.gen_model(rh, cfg)
    finally:
        G.build_model, np.savez_compressed = saved
    _save_fixed(os.path.join(G.OUT, "ffm_layers.npz"), gen_ffm_layers())
    print("ffm_layers.npz")


if __name__ == "__main__":
    main()
