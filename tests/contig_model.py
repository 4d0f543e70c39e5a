"""Rule 13c (include/aim_hip.h, AIM_FEATURE_CONTIGS) in plain numpy, written from the text of the rule: the layout of several contigs in
one sequence, the contig of an anchor, the clip of a segment's window to its contig and the two changes to rule 12c's record. One slot
at a time: the point is to be obviously the rule. It reuses split_model's recovery of p_lo and map_records_model, and shares no code
with the library. Below the rule: the synthetic slot tables and the three-contig form of tests/mapper_batch.py that the CPU and GPU
tests share."""
import numpy as np

import chain_model as cm
import map_records_model as mm
import seed_model as m
import split_model as sm

MAX, NONE, CLIPPED = 1 << 20, 0xFFFFFFFF, 0x80
MINUS = 1 << 63


def spacer_for(band):
    return band + 64


# ---- rule 13c ----------------------------------------------------------------------------------------------------------------------
def layout(lens, spacer):
    """(starts uint32[n], ref_len)."""
    starts, at = [], 0
    for c, n in enumerate(lens):
        if c:
            at += spacer
        starts.append(at)
        at += int(n)
    return np.array(starts, dtype=np.uint32), at


def concat(seqs, spacer):
    starts, ref_len = layout([len(s) for s in seqs], spacer)
    out = np.full(ref_len, ord("N"), dtype=np.uint8)
    for s, at in zip(seqs, starts):
        out[int(at):int(at) + len(s)] = np.frombuffer(bytes(s), dtype=np.uint8) if isinstance(s, (bytes, bytearray)) else s
    return out


def lookup(starts, A):
    """max{ j : starts[j] <= A }."""
    c = 0
    for j in range(len(starts)):           # (the tests call this on small tables; clip() below uses the bisection)
        if int(starts[j]) <= A:
            c = j
    return c


def clip(K, read_size, flank, ref_len, starts, lens, read_len, req, text_pos, chains, seg_req, seg_text_pos, seg):
    """The clip over a batch: dict(seg_req, seg_text_pos, seg, contig, anchor) -- copies of the three segment buffers as
    aim_contig_clip_device leaves them, d_contig, and the anchor A of every valid slot (-1 elsewhere; not a device output)."""
    o_req, o_tp, o_seg = seg_req.copy(), seg_text_pos.copy(), seg.copy()
    n_slots = len(seg)
    contig = np.full(n_slots, NONE, dtype=np.uint32)
    anchor = np.full(n_slots, -1, dtype=np.int64)
    st = [int(x) for x in starts]
    for slot in range(n_slots):
        fl = int(seg["flags"][slot])
        if not fl & sm.VALID:
            continue
        L = min(max(int(read_len[slot // K]), 0), read_size)
        start, text_len = int(text_pos[slot]) & (MINUS - 1), int(req["text_len"][slot])
        seg_start = int(seg_text_pos[slot]) & (MINUS - 1)
        seg_end = seg_start + int(seg_req["text_len"][slot])
        p = None if fl & sm.LOOSE else sm.recover_p_lo(start, text_len, start + text_len, int(chains["q_lo"][slot]), int(chains["q_hi"][slot]),
                                                       int(chains["ref_span"][slot]), L, flank, read_size, ref_len)
        A = seg_start if p is None else p
        A = min(max(A, 0), ref_len - 1)
        c = int(np.searchsorted(starts, A, side="right")) - 1
        assert st[c] <= A and (c + 1 == len(st) or st[c + 1] > A)
        s2 = max(seg_start, st[c])
        e2 = max(s2, min(seg_end, st[c] + int(lens[c])))
        if s2 != seg_start or e2 != seg_end:
            o_tp[slot] = np.uint64(s2 | (int(seg_text_pos[slot]) & MINUS))
            o_req["text_len"][slot] = e2 - s2
            o_seg["flags"][slot] = fl | CLIPPED
        contig[slot], anchor[slot] = c, A
    return dict(seg_req=o_req, seg_text_pos=o_tp, seg=o_seg, contig=contig, anchor=anchor)


def records(K, n_reads, seg, sam, cls, contig, starts):
    """aim_map_records_contigs_device: rule 12c's (rec_offsets, records) with pos local to the contig and pad = the contig."""
    off, rec = mm.map_records(K, n_reads, seg, sam, cls)
    mapped = mm.mapped_slots(K, n_reads, seg, sam)
    for r in range(n_reads):
        for at in range(int(off[r]), int(off[r + 1])):
            o = rec[at]
            if not mapped[r].any():
                o["sam"]["pad"] = NONE
                continue
            c = int(contig[int(o["slot"])])
            if c < len(starts):
                o["sam"]["pos"] = (int(o["sam"]["pos"]) - int(starts[c])) & ((1 << 64) - 1)
            o["sam"]["pad"] = c
    return off, rec


# ---- synthetic slot tables -----------------------------------------------------------------------------------------------------------
SYN_READ_SIZE, SYN_FLANK, SYN_SPACER = 256, 16, 80


def synthetic_contigs(seed, n_contigs):
    """Contig lengths 1..3000 with a contig of one base second (where there are three or more), and their layout."""
    rng = np.random.default_rng([int(seed), n_contigs, 0x636F6E])
    lens = rng.integers(1, 3001, size=n_contigs).astype(np.uint32)
    short = rng.random(n_contigs) < 0.1
    lens[short] = rng.integers(1, 40, size=int(short.sum()))
    if n_contigs >= 3:
        lens[1] = 1
    starts, ref_len = layout(lens, SYN_SPACER)
    return lens, starts, ref_len


def synthetic_slots(seed, K, n_reads, lens, starts, ref_len, seg_flags=None):
    """Slot tables for the clip: dict(read_len, req, text_pos, chains, seg_req, seg_text_pos, seg), every byte of every table set. A
    valid slot aims its anchor at a contig's first base, its last base, the spacer behind it, its inside, or outside the reference
    (clamped), through either recovery path or as a LOOSE segment, and lays its segment window inside the contig, over its left edge,
    its right edge, both, or wholly outside; start == 0, both strands and a window of length 0 occur. Slots without AIM_SEG_VALID hold
    random bytes. seg_flags (uint8 per slot) presets aim_segment_t.flags, e.g. map_records_model's."""
    rs, flank = SYN_READ_SIZE, SYN_FLANK
    rng = np.random.default_rng([int(seed), K, n_reads, len(lens), 0x736C6F])
    S = n_reads * K
    raw = lambda dt, n: rng.integers(0, 256, size=n * dt.itemsize, dtype=np.uint8).view(dt).copy()
    req, chains, seg_req, seg = raw(m.REQUEST, S), raw(cm.CHAIN, S), raw(m.REQUEST, S), raw(sm.SEGMENT, S)
    text_pos, seg_tp = raw(np.dtype("<u8"), S), raw(np.dtype("<u8"), S)
    read_len = rng.integers(-4, rs + 20, size=n_reads).astype(np.int32)
    if seg_flags is None:
        kind = rng.integers(0, 8, size=S)
        flags = rng.integers(0, 256, size=S).astype(np.uint8) & np.uint8(0x7E)              # 0x80 is the clip's own bit
        flags[kind == 0] = 0                                                                # an empty slot
        flags[kind >= 2] |= np.uint8(sm.VALID)                                              # kind 1: bits without VALID (a secondary's leftovers)
        flags[(kind >= 2) & (rng.random(S) < 0.8)] &= np.uint8(0xFF ^ sm.LOOSE)
    else:
        flags = np.asarray(seg_flags, dtype=np.uint8).copy()
    seg["flags"] = flags
    n = len(lens)
    for slot in np.nonzero(flags & sm.VALID)[0]:
        r = slot // K
        L = min(max(int(read_len[r]), 0), rs)
        c = int(rng.integers(0, n)) if rng.integers(0, 4) else int(rng.integers(0, min(n, 3)))
        lo, hi = int(starts[c]), int(starts[c]) + int(lens[c])
        strand = int(rng.integers(0, 2))
        q_lo = int(rng.integers(0, rs))
        q_hi = int(rng.integers(q_lo, rs + 1))
        span = int(rng.integers(0, 2 * rs))
        ak = int(rng.integers(0, 6))
        A = (lo, hi - 1, hi + int(rng.integers(0, SYN_SPACER)), int(rng.integers(lo, hi)), -5, ref_len + 7)[ak]
        A = min(A, ref_len + 7)
        text_len = int(rng.integers(0, rs + 1))
        start = A - q_lo - flank
        if start <= 0 or rng.integers(0, 8) == 0:                                          # the second path, or what is not recoverable
            start = 0
            if rng.integers(0, 2) and L - q_hi + flank + span < rs:                        # E - (L - q_hi) - flank - span = A where it can
                text_len = max(A, 0) + (L - q_hi) + flank + span
                if not 0 < text_len < rs:
                    text_len = int(rng.integers(0, rs + 1))
        chains["q_lo"][slot], chains["q_hi"][slot], chains["ref_span"][slot] = q_lo, q_hi, span
        req["text_len"][slot] = text_len
        text_pos[slot] = np.uint64(start | (strand << 63))
        # the segment's window, about the contig the anchor aims at (a LOOSE segment's anchor is its own start)
        wk = int(rng.integers(0, 7))
        d1, d2 = int(rng.integers(1, 60)), int(rng.integers(1, 60))
        mid = lo + (hi - lo) // 2
        s, e = ((lo + min(d1, hi - lo - 1), hi), (lo - d1, mid + 1), (mid, hi + d2), (lo - d1, hi + d2), (hi + d1, hi + d1 + d2), (lo - d1 - d2, lo - d1),
                (lo, hi))[wk]
        if rng.integers(0, 16) == 0:
            s, e = 0, min(hi, rs)                                                           # start == 0
        s = max(s, 0)
        e = max(e, s)
        if rng.integers(0, 24) == 0:
            e = s                                                                           # a window of length 0 to begin with
        seg_req["text_len"][slot] = e - s
        seg_tp[slot] = np.uint64(s | (strand << 63))
    return dict(read_len=read_len, req=req, text_pos=text_pos, chains=chains, seg_req=seg_req, seg_text_pos=seg_tp, seg=seg)


def synthetic_clip(seed, K, n_reads, n_contigs, seg_flags=None):
    """(lens, starts, ref_len, slot tables, clip(...) of them)."""
    lens, starts, ref_len = synthetic_contigs(seed, n_contigs)
    d = synthetic_slots(seed, K, n_reads, lens, starts, ref_len, seg_flags)
    want = clip(K, SYN_READ_SIZE, SYN_FLANK, ref_len, starts, lens, d["read_len"], d["req"], d["text_pos"], d["chains"], d["seg_req"], d["seg_text_pos"], d["seg"])
    return lens, starts, ref_len, d, want


def coverage(lens, starts, d, want):
    """What a synthetic batch exercises, counted on the model's output."""
    seg, o = d["seg"], want
    valid = (seg["flags"] & sm.VALID) != 0
    clipped = (o["seg"]["flags"] & CLIPPED) != 0
    s0 = (d["seg_text_pos"] & np.uint64(MINUS - 1)).astype(np.int64)
    e0 = s0 + d["seg_req"]["text_len"]
    s1 = (o["seg_text_pos"] & np.uint64(MINUS - 1)).astype(np.int64)
    e1 = s1 + o["seg_req"]["text_len"]
    c = np.where(valid, o["contig"], 0).astype(np.int64)
    lo = starts[c].astype(np.int64)
    hi = lo + lens[c].astype(np.int64)
    A = o["anchor"]
    return {"valid": int(valid.sum()), "not_valid": int((~valid).sum()), "empty": int((seg["flags"] == 0).sum()),
            "left": int((valid & (s1 != s0) & (e1 == e0)).sum()), "right": int((valid & (s1 == s0) & (e1 != e0)).sum()),
            "both": int((valid & (s1 != s0) & (e1 != e0) & (e1 > s1)).sum()), "outside": int((valid & clipped & (e1 == s1)).sum()),
            "kept": int((valid & ~clipped).sum()), "first_base": int((valid & (A == lo)).sum()), "last_base": int((valid & (A == hi - 1)).sum()),
            "spacer": int((valid & (A >= hi)).sum()), "len1": int((valid & (hi - lo == 1)).sum()), "loose": int((valid & ((seg["flags"] & sm.LOOSE) != 0)).sum()),
            "start0": int((valid & (s0 == 0)).sum()), "minus": int((valid & ((d["seg_text_pos"] >> np.uint64(63)) != 0)).sum()),
            "plus": int((valid & ((d["seg_text_pos"] >> np.uint64(63)) == 0)).sum())}


# ---- tests/mapper_batch.py over three contigs --------------------------------------------------------------------------------------
# The reference of the shared batch is cut at CUTS into three contigs. The cut points lie where none of the 73 reads comes near: on the
# chain, split and contig models no slot of the batch is clipped (tests/test_contigs_cpu.py asserts that).
CUTS = (20000, 43000)
PLANT_TAIL, PLANT_PIECE, PLANT_SEED = 24, 300, 1313
N_PLANTED = 7


def batch_contigs(ref):
    """(names, [three uint8 arrays])."""
    a, b = CUTS
    return ["ctg0", "ctg1", "ctg2"], [ref[:a].copy(), ref[a:b].copy(), ref[b:].copy()]


def batch_layout(ref, band):
    """(lens, starts, ref_len, concatenation) of the three contigs with the mapper's spacer."""
    seqs = batch_contigs(ref)[1]
    lens = np.array([len(s) for s in seqs], dtype=np.uint32)
    starts, ref_len = layout(lens, spacer_for(band))
    return lens, starts, ref_len, concat(seqs, spacer_for(band))


def to_concat(pos):
    """A position of the uncut reference -> (contig, position inside it)."""
    a, b = CUTS
    return (0, pos) if pos < a else (1, pos - a) if pos < b else (2, pos - b)


def planted_reads(ref, read_size):
    """The edge reads: (rows, read_len, what) with what[r] = (the contigs of its records in read order, strand, bases beyond the edge).
    24 random bases in front of contig 1's first 300; contig 0's last 300 and 24 random bases behind; the reverse complements of
    both; contig 0's last 300 followed by contig 1's first 300; and the first two again with one base beyond the edge instead of 24.
    Against the spacer's 'N' a run of 24 costs more as mismatches (72) than as a gap (28), one base less (3 against 5): only the last
    two are reads that an alignment over the spacer would carry across the contig's edge."""
    seqs = batch_contigs(ref)[1]
    rng = np.random.default_rng(PLANT_SEED)
    head, tail = seqs[1][:PLANT_PIECE], seqs[0][-PLANT_PIECE:]
    other = {65: 67, 67: 71, 71: 84, 84: 65}

    def rnd(n, avoid_first=None, avoid_last=None):
        # the run has one place only: were its first (last) base the contig's first (last), an equal-cost alignment would start (end)
        # with a match and carry the run inside
        x = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].copy()
        if avoid_first is not None and x[0] == avoid_first:
            x[0] = other[int(x[0])]
        if avoid_last is not None and x[-1] == avoid_last:
            x[-1] = other[int(x[-1])]
        return x
    r0, r1 = np.concatenate([rnd(PLANT_TAIL, avoid_first=head[0]), head]), np.concatenate([tail, rnd(PLANT_TAIL, avoid_last=tail[-1])])
    s0, s1 = np.concatenate([rnd(1, avoid_first=head[0]), head]), np.concatenate([tail, rnd(1, avoid_last=tail[-1])])
    reads = [r0, r1, m.revcomp(r0), m.revcomp(r1), np.concatenate([tail, head]), s0, s1]
    what = [((1,), 0, PLANT_TAIL), ((0,), 0, PLANT_TAIL), ((1,), 1, PLANT_TAIL), ((0,), 1, PLANT_TAIL), ((0, 1), 0, 0), ((1,), 0, 1), ((0,), 0, 1)]
    rows, rl = np.zeros((len(reads), read_size), dtype=np.uint8), np.zeros(len(reads), dtype=np.int32)
    for i, s in enumerate(reads):
        rows[i, :len(s)], rl[i] = s, len(s)
    return rows, rl, what


_CACHE = {}


def batch_models():
    """The shared batch followed by the planted reads, through the chain, class, split and contig models on the concatenation:
    dict(lens, starts, ref_len, concat, rows, read_len, what, K, flank, n_batch, seeds, chains, cls, split (the four outputs of
    split_model.segments), clip (clip() of them))."""
    if "models" not in _CACHE:
        import chain_class_model as ccm
        import mapper_batch as mb
        import minimizer_model as mini
        b = mb.batch()
        k, stride, w, max_occ, band, flank, min_votes, K = ccm.CHIMERIC_ROW
        rs = ccm.CHIMERIC_SIZE
        lens, starts, ref_len, cat = batch_layout(b["ref"], band)
        p_rows, p_rl, what = planted_reads(b["ref"], rs)
        rows, rl = np.ascontiguousarray(np.concatenate([b["rows"], p_rows])), np.concatenate([b["read_len"], p_rl]).astype(np.int32)
        req, tpos, votes, seeds, chains = cm.seed_chain(rows, rl, mini.build_index(cat, k, w), ref_len, k, stride, w, max_occ, band, flank, min_votes, K, rs)
        cls = ccm.classify(K, rs, ccm.MASK_DEFAULT, rl, tpos, seeds, chains)
        split = sm.segments(K, rs, flank, ref_len, rl, rows, req, tpos, seeds, chains, cls)
        clipped = clip(K, rs, flank, ref_len, starts, lens, rl, req, tpos, chains, split[0], split[1], split[3])
        _CACHE["models"] = dict(lens=lens, starts=starts, ref_len=ref_len, concat=cat, rows=rows, read_len=rl, what=what, K=K, flank=flank, n_batch=len(b["read_len"]),
                                seeds=seeds, chains=chains, cls=cls, split=split, clip=clipped, req=req, text_pos=tpos)
    return _CACHE["models"]
