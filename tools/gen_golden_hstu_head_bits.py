"""Record the HSTU next-token head's outputs for tests/golden/hstu_head_bits.npz (needs an MI355X).

    python tools/gen_golden_hstu_head_bits.py --lib <librechub_hip.so of the commit to pin> [--out tests/golden/...]

Inputs are drawn on the CPU from a fixed seed and stored with the outputs: loss, dh, dW and d bias of rh_hstu_head_fwd /
rh_hstu_head_bwd (g_loss = 1) for three configurations that cover the forward's V split, the backward's row split,
NCE and the bias.  tests/test_gpu_session.py replays them through ops.next_token_loss and requires the same bits, so a
change to the shared streaming head cannot move HSTU's results.  The archive was recorded from the library of the
commit before the full-catalogue mode was added to the head (now csrc/stream_ce.hip).
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gen_golden_ffm import _save_fixed  # noqa: E402

# (M, D, V, t1, t2, nce, bias)
CASES = [(130, 50, 300, 0.05, 1.0, 0, True), (200, 24, 700, 1.0, 0.5, 1, False), (37, 10, 41, 2.0, 1.0, 0, True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "hstu_head_bits.npz"))
    a = ap.parse_args()
    lib = ctypes.CDLL(os.path.abspath(a.lib))
    P, I, F = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.rh_hstu_head_fwd.argtypes = [P, P, P, P, I, I, I, F, F, I, P, P, P, P, P, P, P]
    lib.rh_hstu_head_bwd.argtypes = [P, P, P, P, P, P, P, I, I, I, F, F, P, P, P, P, P]
    p = (lambda t: P(0) if t is None else P(t.data_ptr()))
    g = torch.Generator().manual_seed(2022)
    out = {}
    for ci, (M, D, V, t1, t2, nce, bias) in enumerate(CASES):
        h = torch.randn(M, D, generator=g)
        w = 0.3 * torch.randn(V, D, generator=g)
        b = 0.1 * torch.randn(V, generator=g) if bias else None
        lab = torch.randint(0, V, (M,), generator=g)
        lab[::5] = 0
        out.update({f"c{ci}.h": h.numpy(), f"c{ci}.w": w.numpy(), f"c{ci}.labels": lab.numpy(),
                    f"c{ci}.cfg": np.array([t1, t2, nce], np.float64)})
        if b is not None:
            out[f"c{ci}.bias"] = b.numpy()
        h, w, lab = h.cuda(), w.cuda(), lab.cuda()
        b = None if b is None else b.cuda()
        ns = lib.rh_hstu_head_nsplit(M, V)
        part = torch.empty((M, ns, 2), device="cuda")
        zl, lse, wr = (torch.empty(M, device="cuda") for _ in range(3))
        loss = torch.empty((), device="cuda")
        st = P(torch.cuda.current_stream().cuda_stream)
        assert lib.rh_hstu_head_fwd(p(h), p(w), p(b), p(lab), M, D, V, t1, t2, nce, p(part), p(zl), p(lse), p(wr), p(loss),
                                    P(0), st) == 0
        R = lib.rh_hstu_head_rsplit(M, D, V)
        part2 = torch.empty((R, V, D + 1) if R > 1 else (1,), device="cuda")
        gh, gw = torch.empty_like(h), torch.empty_like(w)
        gb = torch.empty(V, device="cuda") if b is not None else None
        one = torch.ones(1, device="cuda")
        assert lib.rh_hstu_head_bwd(p(h), p(w), p(b), p(lab), p(lse), p(wr), p(one), M, D, V, t1, t2, p(part2), p(gh), p(gw),
                                    p(gb), st) == 0
        torch.cuda.synchronize()
        out.update({f"c{ci}.loss": loss.cpu().numpy(), f"c{ci}.g_h": gh.cpu().numpy(), f"c{ci}.g_w": gw.cpu().numpy()})
        if gb is not None:
            out[f"c{ci}.g_bias"] = gb.cpu().numpy()
    _save_fixed(a.out, out)
    print(a.out, len(out), "arrays")


if __name__ == "__main__":
    main()
