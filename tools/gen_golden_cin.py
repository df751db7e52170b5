"""Generate the CIN / xDeepFM fixtures of tests/golden/ from the UNMODIFIED reference (CPU).

Run where the reference checkout exists:  ``python tools/gen_golden_cin.py``

  cin_layers.npz             the reference ``CIN`` in float64 at (B, F, D, cin_size, split_half) = (37, 5, 10, [6, 4, 3], True)
                             and (37, 5, 10, [6, 5], False): input, state_dict, output, upstream gradient, input gradient,
                             parameter gradients, and the seed each configuration settled on
  model_xdeepfm.npz          xDeepFM, six sparse features of width 16 (deep = fm), cin_size [8, 6], split_half
  model_xdeepfm_criteo.npz   width 10 (PaddedEmbedding tables here), a dense feature in the deep list, cin_size [6, 6], no split

The reference has the layer but no xDeepFM class, so the model is composed below from the reference's own ``LR``, ``CIN``,
``MLP`` and ``EmbeddingLayer`` in DeepFM's shape (torch_rechub/models/ranking/deepfm.py:14-43 with FM replaced by CIN) and
goes through oracle/gen_golden.py's recipe (seed 2022, dropout 0, B = 48, three batches through the reference
``CTRTrainer``) by importing it: its ``gen_model`` runs with this file's model builder in place of its own.

The layer fixtures step their seed until no pre-activation of any layer lies within 1e-6 of that layer's largest magnitude
of zero (judged on the float64 numbers), so a float32 kernel decides every ReLU as the fixture did.  The archives are
written with a fixed member timestamp, so the files regenerate byte-identically.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden as G  # noqa: E402
from oracle.ref_import import import_reference  # noqa: E402
from tools.gen_golden_ffm import _save_fixed  # noqa: E402

VOCABS = [3, 4, 10, 27, 105, 305]
# cfg -> (embed_dim, dense features in the deep list, cin_size, split_half)
CONFIGS = {"xdeepfm": (16, 0, [8, 6], True), "xdeepfm_criteo": (10, 1, [6, 6], False)}
LAYER_CASES = {"split": (37, 5, 10, [6, 4, 3], True), "full": (37, 5, 10, [6, 5], False)}
RELU_MARGIN = 1e-6


def build_xdeepfm_model(rh, cfg):
    from torch_rechub.basic.features import DenseFeature, SparseFeature
    from torch_rechub.basic.layers import CIN, LR, MLP, EmbeddingLayer

    class xDeepFM(torch.nn.Module):

        def __init__(self, deep_features, fm_features, mlp_params, cin_size, split_half=True):
            super().__init__()
            self.deep_features = deep_features
            self.fm_features = fm_features
            self.deep_dims = sum(fea.embed_dim for fea in deep_features)
            self.fm_dims = sum(fea.embed_dim for fea in fm_features)
            self.linear = LR(self.fm_dims)
            self.cin = CIN(len(fm_features), cin_size, split_half)
            self.embedding = EmbeddingLayer(deep_features + fm_features)
            self.mlp = MLP(self.deep_dims, **mlp_params)

        def forward(self, x):
            input_deep = self.embedding(x, self.deep_features, squeeze_dim=True)
            input_fm = self.embedding(x, self.fm_features, squeeze_dim=False)
            y = self.linear(input_fm.flatten(start_dim=1)) + self.cin(input_fm) + self.mlp(input_deep)
            return torch.sigmoid(y.squeeze(1))

    D, n_dense, cin_size, split_half = CONFIGS[cfg]
    dense = [DenseFeature(f"I{i + 1}") for i in range(n_dense)]
    sparse = [SparseFeature(f"C{i + 1}", vocab_size=v, embed_dim=D) for i, v in enumerate(VOCABS)]
    mlp = {"dims": [32, 16], "dropout": 0.0, "activation": "relu"}
    model = xDeepFM(dense + sparse, sparse, mlp, cin_size, split_half)
    return model, {"deep_features": dense + sparse, "fm_features": sparse}


def run_cin_case(B, F, D, cin_size, split_half, seed):
    """The reference CIN in float64 under one seed: (arrays, smallest |pre-activation| / layer maximum over the layers)."""
    from torch_rechub.basic.layers import CIN
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    cin = CIN(F, cin_size, split_half).double()
    pre = []
    hooks = [conv.register_forward_hook(lambda mod, inp, out: pre.append(out.detach())) for conv in cin.conv_layers]
    x = torch.randn(B, F, D, generator=g, dtype=torch.float64).requires_grad_(True)
    y = cin(x)
    gy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(gy)
    for hk in hooks:
        hk.remove()
    margin = min(float((p.abs() / p.abs().max()).min()) for p in pre)
    out = {"x": G.npy(x), "out": G.npy(y), "g_out": G.npy(gy), "g_x": G.npy(x.grad), "seed": np.array(seed),
           "cin_size": np.array(cin_size), "split_half": np.array(int(split_half))}
    for n, t in cin.state_dict().items():
        out["sd." + n] = G.npy(t)
    for n, p in cin.named_parameters():
        out["grad." + n] = G.npy(p.grad)
    return out, margin


def gen_cin_layers():
    out = {}
    for tag, (B, F, D, cin_size, split_half) in LAYER_CASES.items():
        seed = G.SEED
        while True:
            arrays, margin = run_cin_case(B, F, D, cin_size, split_half, seed)
            if margin > RELU_MARGIN:
                break
            seed += 1
        print(f"cin_layers.{tag}: seed {seed}, smallest |pre-activation| / layer maximum {margin:.3e}")
        out.update({f"{tag}.{k}": v for k, v in arrays.items()})
    return out


def main():
    rh = import_reference()
    saved = (G.build_model, np.savez_compressed)
    G.build_model = build_xdeepfm_model
    np.savez_compressed = _save_fixed
    try:
        for cfg in CONFIGS:
            G.gen_model(rh, cfg)
    finally:
        G.build_model, np.savez_compressed = saved
    _save_fixed(os.path.join(G.OUT, "cin_layers.npz"), gen_cin_layers())
    print("cin_layers.npz")


if __name__ == "__main__":
    main()
