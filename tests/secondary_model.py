"""Rule 16c (include/aim_hip.h, AIM_FEATURE_SECONDARY) in plain Python / numpy, written from the text of the rule: the rows of the
secondaries (part 1), the winner of each locus and its MAPQ (part 2) and the record list over loci (part 3). One read at a time, no
vectorising across reads: the point is to be obviously the rule. It shares no code with the library. Below the rules: the synthetic
tables the CPU and GPU tests share, and the three classes of reads over a two-copy repeat that the end-to-end tests map."""
import numpy as np

import chain_class_model as ccm
import map_records_model as mm
import seed_model as m
import split_model as sm

SEC_SLOT = np.dtype([("role", "u1"), ("family", "u1"), ("mapq", "u1"), ("aln_mapq", "u1"), ("n_tied", "u1"), ("flags", "u1"), ("gap", "<u2")])
MAP_SEC = np.dtype([("family_slot", "<u4"), ("second_score", "<i4"), ("aln_mapq", "u1"), ("chain_mapq", "u1"), ("n_members", "u1"), ("n_tied", "u1"), ("flags", "<u4")])
assert SEC_SLOT.itemsize == 8 and MAP_SEC.itemsize == 16
SEC_MAX, SEC_RECORDS, SAM_SECONDARY, SWAPPED, COMPLETE = 15, 1, 0x100, 1, 2
INT32_MAX, CONTIG_NONE = 0x7FFFFFFF, 0xFFFFFFFF
KEPT = sm.VALID | sm.SUPPLEMENTARY | sm.LEFT_OPEN | sm.RIGHT_OPEN


def kind(cls, slot):
    """PRIMARY, SECONDARY, or 0 for anything else (an empty slot, both flags)."""
    k = int(cls["flags"][slot]) & (ccm.PRIMARY | ccm.SECONDARY)
    return k if k in (ccm.PRIMARY, ccm.SECONDARY) else 0


# ---- part 1 ----------------------------------------------------------------------------------------------------------------------
def rows(K, read_size, flank, ref_len, max_sec, read_len, reads, req, text_pos, seed, chains, cls, seg_req, seg_tp, seg_pat, seg):
    """The four segment buffers after aim_secondary_rows_device (copies), and the slots that got a row."""
    o_req, o_tp, o_pat, o_seg = seg_req.copy(), seg_tp.copy(), seg_pat.copy(), seg.copy()
    got = []
    for r in range(len(read_len)):
        L = min(max(int(read_len[r]), 0), read_size)
        n = min(int(seed["n_cands"][r]), K)
        seen = {}
        for i in range(n):
            slot = r * K + i
            if kind(cls, slot) != ccm.SECONDARY:
                continue
            j = int(cls["parent"][slot])
            t = seen.get(j, 0)
            seen[j] = t + 1
            if t >= max_sec or j >= n or kind(cls, r * K + j) != ccm.PRIMARY:
                continue
            ps = seg[r * K + j]
            qa, qb = int(ps["q_begin"]), int(ps["q_end"])
            if not int(ps["flags"]) & sm.VALID or not qa <= qb <= L:
                continue
            start = int(text_pos[slot]) & (sm.MINUS - 1)
            s = int(text_pos[slot]) >> 63
            text_len = int(req["text_len"][slot])
            q_lo, q_hi, span = int(chains["q_lo"][slot]), int(chains["q_hi"][slot]), int(chains["ref_span"][slot])
            p_lo = sm.recover_p_lo(start, text_len, start + text_len, q_lo, q_hi, span, L, flank, read_size, ref_len)
            if p_lo is None:
                continue
            u, v = (L - qb, L - qa) if s else (qa, qb)
            lo = p_lo + (u - q_lo) - flank
            hi = p_lo + span + (v - q_hi) + flank
            seg_start = min(max(lo, 0), ref_len)
            seg_end = max(seg_start, min(max(hi, 0), ref_len))
            o_req[slot] = (qb - qa, min(seg_end - seg_start, read_size), 0, int(req["idx"][slot]))
            o_tp[slot] = np.uint64(seg_start | (s << 63))
            o_pat[slot] = 0
            o_pat[slot, :qb - qa] = reads[r, qa:qb]
            o_seg[slot] = (qa, qb, L, int(ps["flags"]) & KEPT, i)
            got.append(slot)
    return o_req, o_tp, o_pat, o_seg, got


# ---- part 2 ----------------------------------------------------------------------------------------------------------------------
def aln_mapq(b, s2, n_tied, score_unit):
    if n_tied > 1:
        return 0
    if s2 is None:
        return 60
    return min(60, 6 * max(s2 - b, 0) // score_unit)


def kinds(cls):
    """kind() of every slot, as a list."""
    return [k if k in (ccm.PRIMARY, ccm.SECONDARY) else 0 for k in (cls["flags"] & (ccm.PRIMARY | ccm.SECONDARY)).tolist()]


def select(K, n_reads, seg, sam, cls, chains, max_score, score_unit):
    """aim_sec_slot_t[n_reads * K] as secondary_select_kernel writes it. (The columns as Python lists: one read at a time is slow enough.)"""
    out = np.zeros(n_reads * K, dtype=SEC_SLOT)
    kd, parent, n_sub, c_mapq = kinds(cls), cls["parent"].tolist(), cls["n_sub"].tolist(), cls["mapq"].tolist()
    seg_flags, sam_flags, status, score = seg["flags"].tolist(), sam["flags"].tolist(), sam["status"].tolist(), sam["score"].tolist()
    anchors, c_score = chains["n_anchors"].tolist(), chains["score"].tolist()
    for r in range(n_reads):
        sl = [r * K + i for i in range(K)]
        valid = [bool(seg_flags[x] & sm.VALID) for x in sl]
        mapped = [valid[i] and not sam_flags[sl[i]] & sm.SAM_UNMAPPED for i in range(K)]
        ok = [(status[x] & ~sm.SAM_OVERFLOW) == 0 for x in sl]
        e = [score[sl[i]] if mapped[i] else max_score + 1 for i in range(K)]
        for j in range(K):
            if kd[sl[j]] != ccm.PRIMARY:
                continue
            members = [j] + [i for i in range(K) if i != j and kd[sl[i]] == ccm.SECONDARY and valid[i] and parent[sl[i]] == j]
            cands = sorted((e[i], i) for i in members if mapped[i])
            if not cands:
                continue
            b, w = cands[0]
            others = [i for i in members if i != w and valid[i] and ok[i]]
            s2 = min(e[i] for i in others) if others else None
            n_tied = 1 + sum(e[i] == b for i in others)
            aln = aln_mapq(b, s2, n_tied, score_unit)
            cap = 6 * min(anchors[sl[w]], 10) if c_score[sl[w]] else 0
            complete = len(members) - 1 == n_sub[sl[j]]
            mapq = min(aln, cap) if complete else min(aln, cap, c_mapq[sl[j]])
            flags = (SWAPPED if w != j else 0) | (COMPLETE if complete else 0) | (len(members) - 1) << 4
            gap = 65535 if s2 is None else min(max(s2 - b, 0), 65534)
            for i in members:
                if mapped[i]:
                    out[sl[i]] = (1 if i == w else 2, j, mapq if i == w else 0, aln, n_tied, flags, gap)
    return out


# ---- part 3 ----------------------------------------------------------------------------------------------------------------------
def records(K, n_reads, options, seg, sam, cls, sec, contig=None, starts=None):
    """(rec_offsets uint32[n_reads + 1], records mm.RECORD_DTYPE[...], MAP_SEC[...]) as aim_map_records_secondary_device writes them."""
    per_read = []
    role, family, q_begin, score = sec["role"].tolist(), sec["family"].tolist(), seg["q_begin"].tolist(), sam["score"].tolist()
    for r in range(n_reads):
        sl = [r * K + i for i in range(K)]
        locus = sorted((i for i in range(K) if role[sl[i]] == 1), key=lambda i: (q_begin[sl[i]], family[sl[i]]))
        fam_rank = {family[sl[i]]: k for k, i in enumerate(locus)}
        second = []
        if locus and options & SEC_RECORDS:
            second = sorted((i for i in range(K) if role[sl[i]] == 2), key=lambda i: (fam_rank[family[sl[i]]], score[sl[i]], i))
        per_read.append((locus, second))
    offsets = np.zeros(n_reads + 1, dtype=np.uint32)
    for r, (locus, second) in enumerate(per_read):
        offsets[r + 1] = offsets[r] + max(len(locus) + len(second), 1)
    rec = np.zeros(int(offsets[n_reads]), dtype=mm.RECORD_DTYPE)
    msec = np.zeros(int(offsets[n_reads]), dtype=MAP_SEC)
    for r, (locus, second) in enumerate(per_read):
        at = int(offsets[r])
        if not locus:
            o, row = rec[at], sam[r * K]
            o["sam"]["idx"], o["sam"]["score"], o["sam"]["status"], o["sam"]["pad"] = row["idx"], row["score"], row["status"], row["pad"]
            if contig is not None:
                o["sam"]["pad"] = CONTIG_NONE
            o["sam"]["flags"] = sm.SAM_UNMAPPED
            o["read"], o["slot"], o["n_records"] = r, r * K, 1
            msec[at] = (r * K, INT32_MAX, 0, 0, 0, 0, 0)
            continue
        rep = min(int(sec["family"][r * K + i]) for i in locus)
        score_of = {int(sec["family"][r * K + i]): int(sam["score"][r * K + i]) for i in locus}
        for rank, i in enumerate(locus + second):
            slot = r * K + i
            x, o = sec[slot], rec[at + rank]
            j = int(x["family"])
            o["sam"] = sam[slot]
            fl = int(sam["flags"][slot])
            if rank >= len(locus):
                fl = (fl & ~sm.SAM_SUPPLEMENTARY) | SAM_SECONDARY
            else:
                fl = (fl & ~sm.SAM_SUPPLEMENTARY) if j == rep else (fl | sm.SAM_SUPPLEMENTARY)
            o["sam"]["flags"] = fl
            if contig is not None:
                c = int(contig[slot])
                o["sam"]["pos"] = (int(sam["pos"][slot]) - (int(starts[c]) if c < len(starts) else 0)) & 0xFFFFFFFFFFFFFFFF
                o["sam"]["pad"] = c
            o["read"], o["slot"] = r, slot
            o["q_begin"], o["q_end"], o["seg_flags"] = seg["q_begin"][slot], seg["q_end"][slot], seg["flags"][slot]
            o["mapq"] = int(x["mapq"]) if rank < len(locus) else 0
            o["rank"], o["n_records"] = rank, len(locus) + len(second)
            gap = int(x["gap"])
            second_score = INT32_MAX if gap == 65535 else min(score_of[j] + gap, INT32_MAX - 1)
            msec[at + rank] = (r * K + j, second_score, int(x["aln_mapq"]), int(cls["mapq"][r * K + j]), (int(x["flags"]) >> 4) + 1, int(x["n_tied"]),
                               int(x["flags"]) & (SWAPPED | COMPLETE))
    return offsets, rec, msec


# ---- synthetic tables ------------------------------------------------------------------------------------------------------------
SYN_MAX_SCORE, SYN_UNIT = 60, 3


def synthetic(seed, n_reads, K, read_size):
    """split_model.synthetic's chain-kernel outputs, classified and split by the models, with the cases rule 16c names planted in the
    first reads (where K allows): read 0 is one primary and K - 1 secondaries of it whose parent is extended on an inner side of no
    other primary (the whole family over [qa, qb) inside the read); read 1 the same with the first secondary's p_lo not recoverable
    (start 0, text_len 0) and the second one's window cut by position 0; read 2 with windows cut by ref_len; read 3 is a read of one
    primary alone. Returns the dict with "seg_req", "seg_tp", "seg_pat", "seg" (the split model's outputs, read 0's parent moved)."""
    d = sm.synthetic(seed, n_reads, K, read_size)
    rs = read_size
    for r in range(min(4, n_reads)):
        L = rs - 8 * r
        d["read_len"][r] = L
        n = 1 if r == 3 else K
        d["seed"]["n_cands"][r] = n
        for i in range(K):
            slot = r * K + i
            strand = (r + i) & 1
            q_lo, q_hi = 8 + i, L - 16 - i                     # all overlap candidate 0: candidates 1.. are its secondaries
            d["chains"][slot] = (400 - i, 12 - min(i, 8), 0, q_lo, q_hi, q_hi - q_lo + (i % 3) - 1)
            start = 5000 + 3000 * i
            text_len = min(L + 2 * sm.SYN_FLANK + (i % 3) - 1, rs - 1)
            if r == 1 and i == 1:
                start, text_len = 0, 0                         # p_lo is not recoverable
            elif r == 1 and i == 2:
                start, text_len = 0, rs // 2                   # recoverable from E; the window is cut by position 0
            elif r == 2 and i >= 1:
                start = sm.SYN_REF_LEN - text_len - i          # the right flank is cut by ref_len
            d["text_pos"][slot] = np.uint64(start | (strand << 63))
            d["req"][slot] = (L, text_len, 0, 1000 * r + i)
    d["cls"] = ccm.classify(K, rs, ccm.MASK_DEFAULT, d["read_len"], d["text_pos"], d["seed"], d["chains"])
    seg_req, seg_tp, seg_pat, seg = sm.synthetic_segments(d, K, rs)
    if n_reads > 0:                                            # read 0's parent as an extension would leave it: an inner interval
        seg["q_begin"][0], seg["q_end"][0] = 24, int(d["read_len"][0]) - 40
        seg_req["pattern_len"][0] = int(seg["q_end"][0]) - 24
    return dict(d, seg_req=seg_req, seg_tp=seg_tp, seg_pat=seg_pat, seg=seg)


def synthetic_rows(d, K, read_size, max_sec):
    return rows(K, read_size, sm.SYN_FLANK, sm.SYN_REF_LEN, max_sec, d["read_len"], d["reads"], d["req"], d["text_pos"], d["seed"], d["chains"], d["cls"],
                d["seg_req"], d["seg_tp"], d["seg_pat"], d["seg"])


def synthetic_sam(seed, K, n_reads, seg, cls):
    """Random aim_sam_t rows whose every byte is set, for slot tables behind part 1: scores from a few values (ties are common), some
    rows unmapped (over the cap: score SYN_MAX_SCORE + 1), a few with a status that is not OK, a few with OVERFLOW. Planted in read 0
    (K >= 2): candidate 0 unmapped over the cap, candidate 1 mapped -- a winner that is not the primary; read 2: equal scores."""
    rng = np.random.default_rng([int(seed), K, n_reads, 0x736563])
    S = n_reads * K
    sam = rng.integers(0, 256, size=S * mm.SAM_DTYPE.itemsize, dtype=np.uint8).view(mm.SAM_DTYPE).copy()
    sam["score"] = rng.integers(0, 8, size=S) * SYN_UNIT
    sam["pos"] = rng.integers(1 << 20, 1 << 30, size=S)
    unm = rng.random(S) < 0.2
    bad = rng.random(S) < 0.05
    over = rng.random(S) < 0.1
    for i in range(K):
        if n_reads > 0:
            unm[i], bad[i] = i == 0, False
        if n_reads > 2:
            unm[2 * K + i], bad[2 * K + i] = False, False
            sam["score"][2 * K + i] = 9
    sam["score"][unm] = SYN_MAX_SCORE + 1
    sam["flags"] = (sam["flags"] & ~np.uint16(sm.SAM_UNMAPPED | SAM_SECONDARY)) | (unm.astype(np.uint16) * sm.SAM_UNMAPPED)
    sam["status"] = np.where(bad, 1, 0).astype(np.uint16) | (over.astype(np.uint16) * sm.SAM_OVERFLOW)
    return sam


def synthetic_contigs(seed, K, n_reads, n_contigs=5):
    """(d_contig uint32[n_reads * K] with a few entries outside the table, starts uint32[n_contigs])."""
    rng = np.random.default_rng([int(seed), K, n_reads, 0x637467])
    contig = rng.integers(0, n_contigs, size=n_reads * K).astype(np.uint32)
    contig[rng.random(n_reads * K) < 0.05] = CONTIG_NONE
    return contig, (np.arange(n_contigs, dtype=np.uint32) * 1000 + 7).astype(np.uint32)


# ---- the reads over a two-copy repeat --------------------------------------------------------------------------------------------
REPEAT_REF_LEN, REPEAT_A, REPEAT_B, REPEAT_LEN = 20000, 4000, 12000, 600
REPEAT_SITES = tuple(100 + 70 * i for i in range(5))
N_REPEAT_READS, REPEAT_READ_LEN = 16, 300
TIE_OFFSETS, CONTROL_OFFSETS = (-14, -5, 6, 15), (-10, 10)
_BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def _other(base):
    """A base that is not `base`: the next of ACGT."""
    return _BASES[(int(np.nonzero(_BASES == base)[0][0]) + 1) % 4]


def repeat_reference(diverged=True):
    """20 000 random bases with ref[12000:12600] = ref[4000:4600]; copy B changed at the segment offsets REPEAT_SITES when diverged."""
    rng = np.random.default_rng(5)
    ref = _BASES[rng.integers(0, 4, size=REPEAT_REF_LEN)].copy()
    ref[REPEAT_B:REPEAT_B + REPEAT_LEN] = ref[REPEAT_A:REPEAT_A + REPEAT_LEN]
    if diverged:
        for s in REPEAT_SITES:
            ref[REPEAT_B + s] = _other(ref[REPEAT_B + s])
    return ref


def repeat_reads(ref, offsets, row_size=ccm.CHIMERIC_SIZE):
    """(rows, read_len, truth): 16 reads of 300 bases cut from copy B at segment offsets 20 + 5 r, a substitution at every covered
    site + each of `offsets` (inside the read), odd reads reverse-complemented; truth[r] = (lo, hi, strand, covered sites)."""
    rows, rl, truth = np.zeros((N_REPEAT_READS, row_size), dtype=np.uint8), np.full(N_REPEAT_READS, REPEAT_READ_LEN, dtype=np.int32), []
    for r in range(N_REPEAT_READS):
        at = 20 + 5 * r
        read = ref[REPEAT_B + at:REPEAT_B + at + REPEAT_READ_LEN].copy()
        covered = [s for s in REPEAT_SITES if at <= s < at + REPEAT_READ_LEN]
        for s in covered:
            for o in offsets:
                if 0 <= s + o - at < REPEAT_READ_LEN:
                    read[s + o - at] = _other(read[s + o - at])
        rows[r, :REPEAT_READ_LEN] = m.revcomp(read) if r % 2 else read
        truth.append((REPEAT_B + at, REPEAT_B + at + REPEAT_READ_LEN, r % 2, len(covered)))
    return rows, rl, truth


def repeat_classes():
    """{"tie" | "control" | "exact": (ref, rows, read_len, truth)}: the diverged repeat with errors that hide every site from the
    k-mers, with errors at site +- 10 only, and the exact repeat without errors."""
    div, same = repeat_reference(True), repeat_reference(False)
    return {"tie": (div,) + repeat_reads(div, TIE_OFFSETS), "control": (div,) + repeat_reads(div, CONTROL_OFFSETS), "exact": (same,) + repeat_reads(same, ())}


def in_copy(pos, copy_start):
    return copy_start <= pos < copy_start + REPEAT_LEN
