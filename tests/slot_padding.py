"""A second statement about the kernels that give a read a group of lanes, one that does not go through the rules' models: a read's K
slots followed by K' - K slots that hold nothing -- an aim_segment_t without AIM_SEG_VALID, a zero aim_sam_t, a zero class, the contig
of the read's slot 0 -- are the same read. Every output of rules 12c to 15c over the padded tables is then the output over the tables
themselves once slot numbers are renamed r * K + i -> r * K' + i (rule 14c's rescue index r * K + K -> r * K' + K'; UINT_MAX stays).
Plain numpy, no device: pad() and pad_tables() build the padded tables, unpad() takes the K slots back out, rename() renames slot
numbers, and records_renamed() / pairs_renamed() do so inside aim_map_record_t and aim_map_pair_t."""
import numpy as np

NONE = 0xFFFFFFFF
PAIRS = ((1, 4), (3, 4), (3, 8), (3, 16), (6, 8), (6, 16), (9, 16))      # (K, K') of the model test: into and across the three widths


def pad(rows, K, K2, n_reads, from_slot0=False):
    """rows[n_reads * K] as rows[n_reads * K2]: K2 - K zero rows behind every read's K (copies of its slot 0 with from_slot0)."""
    assert K2 >= K and len(rows) == n_reads * K
    a = np.ascontiguousarray(rows).reshape(n_reads, K)
    out = np.zeros((n_reads, K2), dtype=a.dtype)
    out[:, :K] = a
    if from_slot0:
        out[:, K:] = a[:, :1]
    return out.reshape(-1)


def unpad(rows, K, K2, n_reads):
    """(the K slots of every read, its K2 - K others) of rows[n_reads * K2]."""
    a = np.ascontiguousarray(rows).reshape(n_reads, K2)
    return a[:, :K].reshape(-1).copy(), a[:, K:].reshape(-1).copy()


def pad_tables(t, K, K2, n_reads):
    """pair_model.synthetic_tables' dict over K2 slots per read: seg, sam and cls padded with zero rows, contig (where there is one)
    with the read's slot 0; what is per read -- res_sam, read_len, reads -- and the contig layout are the same objects."""
    out = dict(t)
    for k in ("seg", "sam", "cls"):
        out[k] = pad(t[k], K, K2, n_reads)
    out["contig"] = pad(t["contig"], K, K2, n_reads, from_slot0=True) if t["contig"] is not None else None
    return out


def rename(slot, read, K, K2):
    """Slot numbers of the reads given, renamed: read * K + i -> read * K2 + i for i < K, read * K + K -> read * K2 + K2, UINT_MAX kept."""
    slot, read = np.asarray(slot, dtype=np.int64), np.asarray(read, dtype=np.int64)
    i = slot - read * K
    keep = slot == NONE
    assert ((i >= 0) & (i <= K) | keep).all(), "a slot that is not its read's"
    return np.where(keep, NONE, read * K2 + np.where(i == K, K2, i)).astype(np.uint32)


def records_renamed(rec, K, K2):
    """aim_map_record_t rows with `slot` renamed by the record's own read."""
    out = rec.copy()
    out["slot"] = rename(rec["slot"], rec["read"], K, K2)
    return out


def pairs_renamed(pairs, K, K2):
    """aim_map_pair_t rows with slot[x] renamed as a slot of read 2m + x."""
    out = pairs.copy()
    m = np.arange(len(pairs), dtype=np.int64)
    for x in (0, 1):
        out["slot"][:, x] = rename(pairs["slot"][:, x], 2 * m + x, K, K2)
    return out
