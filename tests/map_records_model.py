"""Rule 12c (include/aim_hip.h, AIM_FEATURE_MAPPER) in plain numpy, written from the text of the rule: the dense record list of a batch
from its slot-shaped aim_segment_t, aim_sam_t and aim_chain_class_t rows. One read at a time, no vectorising across reads: the point is
to be obviously the rule. synthetic_tables() builds the slot tables the GPU test feeds both sides."""
import numpy as np

SEG_DTYPE = np.dtype([("q_begin", "<u2"), ("q_end", "<u2"), ("read_len", "<u2"), ("flags", "u1"), ("cand", "u1")])
CLASS_DTYPE = np.dtype([("sub_score", "<u4"), ("parent", "u1"), ("flags", "u1"), ("mapq", "u1"), ("n_sub", "u1")])
SAM_DTYPE = np.dtype([("idx", "<u4"), ("score", "<i4"), ("pos", "<u8"), ("ref_span", "<u4"), ("nm", "<u4"), ("cigar_offset", "<u4"),
                      ("n_cigar", "<u4"), ("md_offset", "<u4"), ("md_len", "<u4"), ("flags", "<u2"), ("status", "<u2"), ("pad", "<u4")])
RECORD_DTYPE = np.dtype([("sam", SAM_DTYPE), ("read", "<u4"), ("q_begin", "<u2"), ("q_end", "<u2"), ("mapq", "u1"), ("seg_flags", "u1"), ("rank", "u1"),
                         ("n_records", "u1"), ("slot", "<u4")])
assert SEG_DTYPE.itemsize == 8 and CLASS_DTYPE.itemsize == 8 and SAM_DTYPE.itemsize == 48 and RECORD_DTYPE.itemsize == 64
SEG_VALID = 0x1
SAM_UNMAPPED, SAM_REVERSE, SAM_SUPPLEMENTARY, SAM_OVERFLOW = 0x4, 0x10, 0x800, 0x100


def mapped_slots(K, n_reads, seg, sam):
    """bool[n_reads][K]: VALID in the segment and not UNMAPPED in the row (an OVERFLOW row counts as mapped)."""
    m = ((seg["flags"][:n_reads * K] & SEG_VALID) != 0) & ((sam["flags"][:n_reads * K] & SAM_UNMAPPED) == 0)
    return m.reshape(n_reads, K)


def map_records(K, n_reads, seg, sam, cls):
    """(rec_offsets uint32[n_reads + 1], records RECORD_DTYPE[rec_offsets[n_reads]])."""
    mapped = mapped_slots(K, n_reads, seg, sam)
    counts = [max(int(mapped[r].sum()), 1) for r in range(n_reads)]
    offsets = np.zeros(n_reads + 1, dtype=np.uint32)
    for r in range(n_reads):
        offsets[r + 1] = offsets[r] + counts[r]
    rec = np.zeros(int(offsets[n_reads]), dtype=RECORD_DTYPE)
    for r in range(n_reads):
        cands = [i for i in range(K) if mapped[r, i]]
        at = int(offsets[r])
        if not cands:
            o = rec[at]
            row = sam[r * K]
            o["sam"]["idx"], o["sam"]["score"], o["sam"]["status"], o["sam"]["pad"] = row["idx"], row["score"], row["status"], row["pad"]
            o["sam"]["flags"] = SAM_UNMAPPED
            o["read"], o["slot"], o["n_records"] = r, r * K, 1
            continue
        order = sorted(cands, key=lambda i: (int(seg["q_begin"][r * K + i]), i))
        rep = min(cands)
        for rank, i in enumerate(order):
            slot = r * K + i
            o = rec[at + rank]
            o["sam"] = sam[slot]
            fl = int(sam["flags"][slot])
            o["sam"]["flags"] = (fl & ~SAM_SUPPLEMENTARY) if i == rep else (fl | SAM_SUPPLEMENTARY)
            o["read"], o["slot"] = r, slot
            o["q_begin"], o["q_end"], o["seg_flags"] = seg["q_begin"][slot], seg["q_end"][slot], seg["flags"][slot]
            o["mapq"] = cls["mapq"][slot]
            o["rank"], o["n_records"] = rank, len(cands)
    return offsets, rec


def synthetic_tables(seed, K, n_reads):
    """Random slot tables (seg, sam, cls) of n_reads * K rows whose every byte is set, with the cases rule 12c names planted in the
    first reads: read 0 has no mapped slot (VALID rows that are UNMAPPED, and rows that are not VALID), read 1 has all K slots mapped
    with equal q_begin, read 2 has candidate 0 unmapped and the last candidate mapped (where K > 1), read 3 has OVERFLOW rows. Every
    other read draws each slot's state at random; q_begin is drawn from a few values, so ties are common."""
    rng = np.random.default_rng([int(seed), K, n_reads, 0x6D6170])
    S = n_reads * K
    raw = lambda dt: rng.integers(0, 256, size=S * dt.itemsize, dtype=np.uint8).view(dt).copy()
    seg, sam, cls = raw(SEG_DTYPE), raw(SAM_DTYPE), raw(CLASS_DTYPE)
    seg["q_begin"] = rng.integers(0, 5, size=S) * 100
    valid = rng.random(S) < 0.55
    unm = rng.random(S) < 0.3
    over = rng.random(S) < 0.1

    def put(r, i, v, u, o=False):
        valid[r * K + i], unm[r * K + i], over[r * K + i] = v, u, o
    for i in range(K):
        if n_reads > 0:
            put(0, i, i % 2 == 0, True)
        if n_reads > 1:
            put(1, i, True, False)
            seg["q_begin"][K + i] = 300
        if n_reads > 2:
            put(2, i, i == K - 1 and K > 1, False)
        if n_reads > 3:
            put(3, i, True, False, True)
    if n_reads > 2:
        put(2, 0, True, True)
    seg["flags"] = (seg["flags"] & ~np.uint8(SEG_VALID)) | valid.astype(np.uint8)
    sam["flags"] = (sam["flags"] & ~np.uint16(SAM_UNMAPPED)) | (unm.astype(np.uint16) * SAM_UNMAPPED)
    sam["status"] = (sam["status"] & ~np.uint16(SAM_OVERFLOW)) | (over.astype(np.uint16) * SAM_OVERFLOW)
    return seg, sam, cls
