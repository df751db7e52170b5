"""numpy restatement of one step of the constrained beam search over a flat trie (csrc/beam.hip, ops.beam_step).

The log-softmax of a row is taken in float64 from the float32 logits, over the whole vocabulary; a candidate (beam k, edge e
of k's node) scores float32(float64(running[b, k]) + logp[tok_e]); a candidate at -inf is none.  The K best per query under
(score descending, beam ascending, token ascending) fill the slots; fewer than K set the short flag and leave (-inf, -1,
-1, -1) behind.  ``gap`` is the smallest float64 distance between neighbouring candidates of the first K + 1 whose float64
scores are distinct: inputs with a gap above the margin are decided by the scores in any float32 evaluation order, and
candidates at distance 0 are equal by construction, so the tie rule decides."""
import numpy as np


def log_softmax64(logits):
    x = np.asarray(logits, dtype=np.float32).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = x.max(axis=-1, keepdims=True)
        return (x - m) - np.log(np.exp(x - m).sum(axis=-1, keepdims=True))


def candidates(logp, running, node, off, tok, child, b):
    """Query b's candidates in selection order: rows (score32, score64, beam, token, child node, logp)."""
    K = running.shape[1]
    out = []
    for k in range(K):
        n = int(node[b, k])
        if n < 0:
            continue
        for e in range(int(off[n]), int(off[n + 1])):
            t = int(tok[e])
            s64 = float(np.float64(running[b, k]) + logp[b * K + k, t])
            if s64 == -np.inf:
                continue
            out.append((float(np.float32(s64)), s64, k, t, int(child[e]), float(logp[b * K + k, t])))
    out.sort(key=lambda c: (-c[0], c[2], c[3]))
    return out


def step(logits, running, node, off, tok, child):
    """logits (B K, V) float32, running (B, K) float32, node (B, K) int; off, tok, child the trie's CSR arrays.  Returns a
    dict: running (B, K) float32, parent / token / node (B, K) int32, short (B,) int32, gap (float), head (per query the
    first K + 1 candidates, as ``candidates`` lists them)."""
    running = np.asarray(running, dtype=np.float32)
    node = np.asarray(node)
    B, K = running.shape
    logp = log_softmax64(logits)
    res = {"running": np.full((B, K), -np.inf, dtype=np.float32), "parent": np.full((B, K), -1, dtype=np.int32),
           "token": np.full((B, K), -1, dtype=np.int32), "node": np.full((B, K), -1, dtype=np.int32),
           "short": np.zeros(B, dtype=np.int32), "gap": np.inf, "head": []}
    for b in range(B):
        cands = candidates(logp, running, node, off, tok, child, b)
        for j, c in enumerate(cands[:K]):
            res["running"][b, j], res["parent"][b, j], res["token"][b, j], res["node"][b, j] = c[0], c[2], c[3], c[4]
        res["short"][b] = int(len(cands) < K)
        head = cands[:K + 1]
        res["head"].append(head)
        for x, y in zip(head, head[1:]):
            d = abs(x[1] - y[1])
            if d != 0 and d < res["gap"]:
                res["gap"] = d
    return res


def dense_step(logits, running, node, off, tok):
    """The same step as ``TIGERModel.generate`` forms it: a (B K, V) mask of -inf outside the children, and the K largest
    of float32(running + logp + mask) over (B, K V), an exact tie to the lower flat index.  -> (scores (B, K), flat index
    (B, K), -1 behind a -inf score)."""
    running = np.asarray(running, dtype=np.float32)
    B, K = running.shape
    logp = log_softmax64(logits)
    V = logp.shape[1]
    mask = np.full((B * K, V), -np.inf)
    for r in range(B * K):
        n = int(np.asarray(node).reshape(-1)[r])
        if n >= 0:
            mask[r, np.asarray(tok)[int(off[n]):int(off[n + 1])]] = 0.0
    cand = (running.reshape(B * K, 1).astype(np.float64) + logp + mask).astype(np.float32).reshape(B, K * V)
    idx = np.argsort(-cand, axis=1, kind="stable")[:, :K]
    top = np.take_along_axis(cand, idx, 1)
    return top, np.where(np.isinf(top), -1, idx)
