"""Split reads (include/aim_hip.h, AIM_FEATURE_SPLIT) in plain Python / numpy, written from the text of rule 10c and of
aim_sam_device_split: the open sides, the read interval, the recovered window and the segment rows; the expected split records from the
downloaded records of plain aim_sam_device. It shares no code with the library. Below the rules: the batches the CPU and GPU tests
share -- a synthetic batch of chain-kernel outputs for any row size, and the chimeric reads of chain_class_model with the truth about
each half."""
import numpy as np

import chain_class_model as ccm
import chain_model as cm
import seed_model as m

SEGMENT = np.dtype([("q_begin", "<u2"), ("q_end", "<u2"), ("read_len", "<u2"), ("flags", "u1"), ("cand", "u1")])
VALID, SUPPLEMENTARY, LEFT_OPEN, RIGHT_OPEN, LOOSE = 1, 2, 4, 8, 16
SAM_SUPPLEMENTARY, SAM_REVERSE, SAM_UNMAPPED, SAM_OVERFLOW = 0x800, 0x10, 0x4, 0x100
MINUS = 1 << 63
MAX_REF_LEN = 0xFE000000


# ---- rule 10c --------------------------------------------------------------------------------------------------------------------
def recover_p_lo(start, text_len, E, q_lo, q_hi, ref_span, L, flank, read_size, ref_len):
    """Rule 6c's p_lo from a candidate's window, or None where it is not recoverable."""
    if start > 0:
        return start + q_lo + flank
    if 0 < text_len < read_size and E < ref_len:
        return E - (L - q_hi) - flank - ref_span
    return None


def split_read(K, read_size, flank, ref_len, L, n, req, tpos, chains, cls):
    """One read: per slot i None (every other slot) or (a', b', seg_start, text_len, strand, flags). req, tpos, chains, cls are the
    read's K slots."""
    ivals, strands = [], []
    for i in range(K):
        s = int(tpos[i]) >> 63
        ivals.append(ccm.interval(int(chains["q_lo"][i]), int(chains["q_hi"][i]), s, L))
        strands.append(s)
    prim = [i for i in range(K) if i < n and int(cls["flags"][i]) & ccm.PRIMARY]
    out = [None] * K
    for i in prim:
        a, b = ivals[i]
        left_open = not any(ivals[j][0] < a for j in prim if j != i)
        right_open = not any(ivals[j][1] > b for j in prim if j != i)
        a2 = 0 if left_open else min(max(a, 0), L)                 # (the clamps act on malformed chains only)
        b2 = L if right_open else min(max(b, a2), L)
        s = strands[i]
        low_open, high_open = (right_open, left_open) if s else (left_open, right_open)
        start = int(tpos[i]) & (MINUS - 1)
        text_len = int(req["text_len"][i])
        E = start + text_len
        q_lo, q_hi, span = int(chains["q_lo"][i]), int(chains["q_hi"][i]), int(chains["ref_span"][i])
        p_lo = recover_p_lo(start, text_len, E, q_lo, q_hi, span, L, flank, read_size, ref_len)
        flags = VALID | (SUPPLEMENTARY if i else 0) | (LEFT_OPEN if left_open else 0) | (RIGHT_OPEN if right_open else 0)
        if p_lo is None:
            flags |= LOOSE
            seg_start, seg_end = start, max(start, E)
        else:
            p_hi = p_lo + span
            seg_start = start if low_open else min(max(p_lo, 0), ref_len)
            seg_end = max(seg_start, E if high_open else min(max(p_hi, 0), ref_len))
        out[i] = (a2, b2, seg_start, min(seg_end - seg_start, read_size), s, flags)
    return out


def segments(K, read_size, flank, ref_len, read_len, reads, req, text_pos, seed, chains, cls):
    """The whole batch: (aim_request_t[n * K], text_pos[n * K], patterns uint8[n * K][read_size], aim_segment_t[n * K]) as
    split_segments_kernel writes them."""
    n_reads = len(read_len)
    o_req = np.zeros(n_reads * K, dtype=m.REQUEST)
    o_tp = np.zeros(n_reads * K, dtype=np.uint64)
    o_pat = np.zeros((n_reads * K, read_size), dtype=np.uint8)
    o_seg = np.zeros(n_reads * K, dtype=SEGMENT)
    for r in range(n_reads):
        L = min(max(int(read_len[r]), 0), read_size)
        n = min(int(seed["n_cands"][r]), K)
        sl = slice(r * K, (r + 1) * K)
        rows = split_read(K, read_size, flank, ref_len, L, n, req[sl], text_pos[sl], chains[sl], cls[sl])
        for i, row in enumerate(rows):
            slot = r * K + i
            idx = int(req["idx"][slot])
            if row is None:
                o_req[slot] = (L, 0, 0, idx)
                o_pat[slot] = reads[r]
                continue
            a2, b2, seg_start, text_len, s, flags = row
            o_req[slot] = (b2 - a2, text_len, 0, idx)
            o_tp[slot] = np.uint64(seg_start | (s << 63))
            o_pat[slot, :b2 - a2] = reads[r, a2:b2]
            o_seg[slot] = (a2, b2, L, flags, i)
    return o_req, o_tp, o_pat, o_seg


# ---- aim_sam_device_split from aim_sam_device's records -------------------------------------------------------------------------
def sam_split(records, cigar, seg, text_pos, sel=None):
    """The records and CIGAR words aim_sam_device_split gives, from those of plain aim_sam_device over the same rows (records with their
    cigar_offset / n_cigar into `cigar`). Returns (records, [words of record r]): the expected records carry the plain records' offsets,
    which depend on scheduling and are not compared. The plain records must not have overflowed."""
    out = records.copy()
    words = []
    for r in range(len(records)):
        rec = records[r]
        assert not int(rec["status"]) & SAM_OVERFLOW
        c = r if sel is None else int(sel[r])
        w = [int(x) for x in cigar[int(rec["cigar_offset"]):int(rec["cigar_offset"]) + int(rec["n_cigar"])]]
        if c == 0xFFFFFFFF:
            words.append(w)
            continue
        sg = seg[c]
        if int(sg["flags"]) == 0:                                   # the record of a row without a candidate
            out[r]["pos"], out[r]["ref_span"], out[r]["nm"], out[r]["n_cigar"], out[r]["md_len"] = 0, 0, 0, 0, 0
            out[r]["flags"] = SAM_UNMAPPED
            words.append([])
            continue
        if int(rec["flags"]) & SAM_UNMAPPED:
            words.append(w)
            continue
        lead, trail = int(sg["q_begin"]), int(sg["read_len"]) - int(sg["q_end"])
        if int(text_pos[c]) >> 63:
            lead, trail = trail, lead
        if lead:
            w = [w[0] + (lead << 4)] + w[1:] if w[0] & 15 == 4 else [(lead << 4) | 4] + w
        if trail:
            w = w[:-1] + [w[-1] + (trail << 4)] if w[-1] & 15 == 4 else w + [(trail << 4) | 4]
        out[r]["n_cigar"] = len(w)
        if int(sg["flags"]) & SUPPLEMENTARY:
            out[r]["flags"] = int(rec["flags"]) | SAM_SUPPLEMENTARY
        words.append(w)
    return out, words


COMPARED = ("idx", "score", "pos", "ref_span", "nm", "n_cigar", "md_len", "flags", "status", "pad")


def check_split_records(got, got_cigar, got_md, want, want_words, plain, plain_md):
    """Every field but the two offsets, the CIGAR words and the MD bytes (those of the plain record) of every record."""
    for r in range(len(want)):
        for f in COMPARED:
            assert int(got[f][r]) == int(want[f][r]), (r, f, got[r], want[r])
        co = int(got["cigar_offset"][r])
        assert [int(x) for x in got_cigar[co:co + len(want_words[r])]] == want_words[r], (r, want_words[r])
        mo, po, ml = int(got["md_offset"][r]), int(plain["md_offset"][r]), int(want["md_len"][r])
        assert got_md[mo:mo + ml].tobytes() == plain_md[po:po + ml].tobytes(), r


def read_consumed(words):
    """The read bases a CIGAR consumes: M, I, S, =, X."""
    return sum(w >> 4 for w in words if w & 15 in (0, 1, 4, 7, 8))


# ---- the batches -----------------------------------------------------------------------------------------------------------------
SYN_REF_LEN, SYN_FLANK = 1 << 20, 16


def synthetic(seed, n_reads, K, read_size):
    """Random chain-kernel outputs and read rows for n_reads reads of K slots in rows of read_size, classified by the rule 8c model:
    dict(read_len, reads, req, text_pos, seed, chains, cls). Like chain_class_model.synthetic (both strands, n_cands from 0 to above
    K, read_len outside 0..read_size, malformed chains, chains beyond read_len), with disjoint intervals in every third read so that reads of three and more
    primaries occur, and with windows of every kind rule 10c tells apart: start 0 with a short text (recoverable), start 0 with
    text_len 0 or read_size or E >= ref_len (loose), E == ref_len, text_len == read_size away from the edges. The rows are random
    non-zero bytes, also behind read_len. Read r depends on (seed, K, read_size, r) only through the generator's sequence, so a prefix
    of a batch is the batch of fewer reads."""
    rng = np.random.default_rng([seed, K, read_size])
    rs = read_size
    read_len = np.zeros(n_reads, dtype=np.int32)
    text_pos = np.zeros(n_reads * K, dtype=np.uint64)
    seeds = np.zeros(n_reads, dtype=m.SEED)
    chains = np.zeros(n_reads * K, dtype=cm.CHAIN)
    req = np.zeros(n_reads * K, dtype=m.REQUEST)
    reads = np.zeros((n_reads, rs), dtype=np.uint8)
    for r in range(n_reads):
        kind = int(rng.integers(0, 16))
        L = (-5, rs + 40, 0)[kind] if kind < 3 else int(rng.integers(rs // 2, rs + 1))
        read_len[r] = L
        L = min(max(L, 0), rs)
        n = int(rng.integers(0, K + 1)) if rng.integers(0, 8) else K + int(rng.integers(1, 4))
        seeds[r] = (n, [int(rng.integers(0, 1024)), int(rng.integers(0, 1024))], int(rng.integers(0, 2)))
        scores = np.sort(rng.integers(11, 400, size=K))[::-1]
        reads[r] = rng.integers(1, 256, size=rs, dtype=np.uint8)
        cuts = np.sort(rng.integers(0, max(L, 1) + 1, size=2 * K))    # for the disjoint reads
        order = rng.permutation(K)
        top = rs if rng.integers(0, 8) == 0 else max(L, 1)             # one read in eight has chains that reach beyond read_len
        for i in range(K):
            slot = r * K + i
            if r % 3 == 0 and L >= 2 * K:
                q_lo, q_hi = int(cuts[2 * order[i]]), int(cuts[2 * order[i] + 1])
                if q_hi <= q_lo:                                       # (two equal cuts: one base)
                    q_hi = min(q_lo + 1, rs)
                    q_lo = q_hi - 1
            else:
                q_lo = int(rng.integers(0, top))
                q_hi = int(rng.integers(q_lo + 1, top + 1))
            score = int(scores[i])
            if rng.integers(0, 40) == 0:                               # malformed
                q_lo, q_hi, score = (q_hi, q_lo, score) if rng.integers(0, 2) else (q_lo, q_lo, 0)
            chains[slot] = (score, int(rng.integers(1, 30)), 0, q_lo, q_hi, int(rng.integers(0, 2 * rs)))
            strand = int(rng.integers(0, 2))
            wk = int(rng.integers(0, 8))
            text_len = (0, rs)[wk & 1] if wk in (2, 3) or rng.integers(0, 6) == 0 else int(rng.integers(1, rs))
            if wk < 3:
                start = 0
            elif wk == 3:
                start = SYN_REF_LEN - text_len                         # E == ref_len
            elif wk == 4:
                start = int(rng.integers(1, 2 * rs))                   # near the left edge: p_lo can fall below start
            else:
                start = int(rng.integers(1, SYN_REF_LEN - text_len))
            text_pos[slot] = np.uint64(start | (strand << 63))
            req[slot] = (L, text_len, 0, int(rng.integers(0, 1 << 32)))
    d = dict(read_len=read_len, text_pos=text_pos, seed=seeds, chains=chains)
    cls = ccm.classify(K, rs, ccm.MASK_DEFAULT, **d)
    return dict(d, reads=reads, req=req, cls=cls)


def prefix(d, n, K):
    return dict(read_len=d["read_len"][:n], reads=d["reads"][:n], req=d["req"][:n * K], text_pos=d["text_pos"][:n * K], seed=d["seed"][:n],
                chains=d["chains"][:n * K], cls=d["cls"][:n * K])


def synthetic_segments(d, K, read_size):
    return segments(K, read_size, SYN_FLANK, SYN_REF_LEN, d["read_len"], d["reads"], d["req"], d["text_pos"], d["seed"], d["chains"], d["cls"])


def chimeric(ref=None, seed=77):
    """chain_class_model.chimeric_reads' recipe restated, with the truth: (rows, read_len, halves) where halves[r] is a list of two
    dicts, one per half in the order of the recipe: ref_lo, ref_hi (the reference interval the half was drawn from), strand (of the half
    in the read as given), edits (planted), and q_lo, q_hi (the half's interval of the read as given). The rows are asserted equal to
    chimeric_reads()'s."""
    ref = m.make_reference() if ref is None else ref
    rng = np.random.default_rng(seed)
    n, h = 32, ccm.CHIMERIC_HALF
    rows, rl = np.zeros((n, ccm.CHIMERIC_SIZE), dtype=np.uint8), np.zeros(n, dtype=np.int32)
    halves = []
    for r in range(n):
        p1 = m.clean_position(rng, h)
        if r % 4 == 0:
            p2 = m.PLANT_AT[int(rng.integers(0, len(m.PLANT_AT)))] - 50
        else:
            p2 = m.clean_position(rng, h)
            while abs(p2 - p1) < 2 * h:
                p2 = m.clean_position(rng, h)
        first, second = m.edit(rng, ref[p1:p1 + h], ccm.CHIMERIC_EDITS), m.edit(rng, ref[p2:p2 + h], ccm.CHIMERIC_EDITS)
        s1, s2 = 0, r % 2
        if r % 2:
            second = m.revcomp(second)
        read = np.concatenate([first, second])
        assert len(read) <= ccm.CHIMERIC_SIZE
        L, cut = len(read), len(first)
        iv1, iv2 = (0, cut), (cut, L)
        if r % 8 == 0:
            read = m.revcomp(read)
            s1, s2 = s1 ^ 1, s2 ^ 1
            iv1, iv2 = (L - cut, L), (0, L - cut)
        rows[r, :L], rl[r] = read, L
        halves.append([dict(ref_lo=p1, ref_hi=p1 + h, strand=s1, edits=ccm.CHIMERIC_EDITS, q_lo=iv1[0], q_hi=iv1[1]),
                       dict(ref_lo=p2, ref_hi=p2 + h, strand=s2, edits=ccm.CHIMERIC_EDITS, q_lo=iv2[0], q_hi=iv2[1])])
    want_rows, want_rl = ccm.chimeric_reads(ref, seed)
    assert rows.tobytes() == want_rows.tobytes() and rl.tobytes() == want_rl.tobytes()
    return rows, rl, halves


def half_of(halves_r, q_begin, q_end):
    """The half a segment [q_begin, q_end) of the read belongs to: the one that holds its midpoint."""
    mid = (q_begin + q_end) // 2
    return next(hf for hf in halves_r if hf["q_lo"] <= mid < hf["q_hi"])
