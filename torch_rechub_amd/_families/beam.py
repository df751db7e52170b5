"""TIGER's constrained beam search: one step on the device (csrc/beam.hip)."""
import torch

from .. import _lib
from .._opcore import _p, _stream, require_hip


def beam_step(logits, running, node, trie):
    """One step of the constrained beam search (csrc/beam.hip): ``logits`` (B K, V) float32 the beams' next-token logits
    (rows may be strided: the ``[:, -1, :]`` view of a decoder output is read in place), ``running`` (B, K) float32 their
    scores, ``node`` (B, K) int32 their nodes in ``trie`` (a ``utils.data.DeviceTrie`` on the same device), -1 = dead beam.
    Returns ``(running, parent, token, node, short)``: per query the K best continuations running + log_softmax(logits)[tok]
    over the children of the beams' nodes, by (score descending, beam ascending, token ascending) -- (B, K) float32 and
    three (B, K) int32 -- and ``short`` (B,) int32, 1 where fewer than K continuations exist (the unused slots are -inf,
    -1, -1, -1).  No autograd; no host synchronisation; runs on the current stream."""
    require_hip(logits, running, node, trie.child_off)
    if logits.dim() != 2 or running.dim() != 2 or tuple(node.shape) != tuple(running.shape):
        raise ValueError(f"beam_step: logits {tuple(logits.shape)}, running {tuple(running.shape)}, node {tuple(node.shape)}: "
                         "(B K, V), (B, K) and (B, K) expected")
    if logits.dtype != torch.float32 or running.dtype != torch.float32 or node.dtype != torch.int32:
        raise ValueError("beam_step: float32 logits and running and int32 node expected")
    B, K = (int(v) for v in running.shape)
    V = int(logits.shape[1])
    if int(logits.shape[0]) != B * K:
        raise ValueError(f"beam_step: {int(logits.shape[0])} logits rows for B K = {B} x {K} beams")
    if not (logits.device == running.device == node.device == trie.child_off.device):
        raise ValueError("beam_step: logits, running, node and the trie must be on one device")
    if not 1 <= K <= _lib.H.RH_BEAM_MAX_K or V < 1:
        raise ValueError(f"beam_step: K={K}, V={V} unsupported (1 <= K <= {_lib.H.RH_BEAM_MAX_K}, V >= 1)")
    if trie.max_token >= V:
        raise ValueError(f"beam_step: the trie holds token {trie.max_token}, outside the vocabulary V={V}")
    logits = logits.detach()
    if B * K > 0 and (logits.stride(1) != 1 or (B * K > 1 and logits.stride(0) < V)):
        logits = logits.contiguous()
    ld = int(logits.stride(0)) if B * K > 1 else V
    running, node = running.detach().contiguous(), node.contiguous()
    dev = logits.device
    out_run = torch.empty((B, K), dtype=torch.float32, device=dev)
    parent, tok, child = (torch.empty((B, K), dtype=torch.int32, device=dev) for _ in range(3))
    short = torch.empty((B,), dtype=torch.int32, device=dev)
    if B > 0:
        _lib.call("rh_beam_step", _p(logits), ld, _p(running), _p(node), _p(trie.child_off), _p(trie.child_tok),
                  _p(trie.child_node), int(trie.n_nodes), B, K, V, _p(out_run), _p(parent), _p(tok), _p(child), _p(short),
                  _stream())
    return out_run, parent, tok, child, short
