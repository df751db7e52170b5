"""Shared pieces of the session-based retrieval models (NARM, STAMP): input checks and the item-table lookup."""
import torch.nn.functional as F

from ... import ops


def session_counts(seq, check_full=False):
    """(mask (B, L) bool, counts (B,) int64) of an id matrix, 0 = padding.  Rows without any item raise as
    pack_padded_sequence does, and with ``check_full`` a batch whose longest row is shorter than L raises (the reference's
    broadcast of the (B, max_count, H) states against the (B, L) mask fails there): through the device error word
    (ops.session_lengths), at once in eager mode and at the trainer's error check after a replayed hipGraph step."""
    return seq != 0, ops.session_lengths(seq, check_full)


def lookup(table, ids):
    """nn.Embedding(padding_idx=0) lookup of ``ids`` in ``table`` (row 0 gets no gradient from the lookup)."""
    return F.embedding(ids, table.weight, padding_idx=0)


def check_dense_table(model):
    if getattr(model.item_emb, "_rh_shard", None) is not None:
        raise RuntimeError(f"torch_rechub_amd: {type(model).__name__} on a row-sharded item table is not supported")
