"""Primary / secondary chains and MAPQ (include/aim_hip.h, AIM_FEATURE_CHAIN_CLASS) in plain Python / numpy, written from the text of
rules 8c and 9c: the read intervals, the overlap test, the parents, the flags, sub-scores and chain MAPQ, and the MAPQ of a read after
verification. It shares no code with the library. Below the rules: the batches the CPU and GPU tests share."""
import numpy as np

import chain_model as cm
import seed_model as m

CLASS = np.dtype([("sub_score", "<u4"), ("parent", "u1"), ("flags", "u1"), ("mapq", "u1"), ("n_sub", "u1")])
MAPQ = np.dtype([("slot", "<u4"), ("mapq", "u1"), ("chain_mapq", "u1"), ("aln_mapq", "u1"), ("flags", "u1")])
BEST = np.dtype([("best_pair", "<u4"), ("best_score", "<i4"), ("second_score", "<i4"), ("n_best", "<u4")])
MATE = np.dtype([("best_pair", "<u4", (2,)), ("score_sum", "<i4"), ("second_sum", "<i4"), ("n_best", "<u4"), ("flags", "<u4"), ("pad", "<u4", (2,))])
PRIMARY, SECONDARY, SUPPLEMENTARY = 1, 2, 4
UNMAPPED, MAPQ_SECONDARY, MAPQ_SUPPLEMENTARY, PROPER = 1, 2, 4, 8
MASK_DEFAULT = 128
MATE_PROPER = 1
NONE, INT32_MAX = 0xFFFFFFFF, 0x7FFFFFFF


# ---- rule 8c ---------------------------------------------------------------------------------------------------------------------
def interval(q_lo, q_hi, strand, L):
    """[a, b): the interval of the read as given."""
    return (L - q_hi, L - q_lo) if strand else (q_lo, q_hi)


def overlap(x, y, mask_q8):
    """Do the intervals x and y overlap at mask level mask_q8 / 256? Equality counts; an interval with len <= 0 overlaps nothing."""
    ov = min(x[1], y[1]) - max(x[0], y[0])
    lx, ly = x[1] - x[0], y[1] - y[0]
    return lx > 0 and ly > 0 and ov > 0 and 256 * ov >= mask_q8 * min(lx, ly)


def chain_mapq(f1, f2, n_anchors):
    if f1 == 0 or f2 > f1:
        return 0
    return min(60, (6 * min(n_anchors, 10) * (f1 - f2)) // f1)


def classify_read(ivals, scores, n_anchors, mask_q8):
    """One read's candidates in rank order: [(sub_score, parent, flags, mapq, n_sub)]."""
    n = len(ivals)
    parent, primary = [0] * n, [False] * n
    for i in range(n):
        over = [j for j in range(i) if primary[j] and overlap(ivals[i], ivals[j], mask_q8)]
        parent[i], primary[i] = (over[0], False) if over else (i, True)
    out = []
    for j in range(n):
        if not primary[j]:
            out.append((0, parent[j], SECONDARY, 0, 0))
            continue
        subs = [scores[i] for i in range(n) if i != j and parent[i] == j]
        sub = max(subs) if subs else 0
        out.append((sub, j, PRIMARY | (SUPPLEMENTARY if j else 0), chain_mapq(scores[j], sub, n_anchors[j]), len(subs)))
    return out


def classify(K, read_size, mask_q8, read_len, text_pos, seed, chains):
    """The whole batch: aim_chain_class_t[n_reads * K] as chain_class_kernel writes it."""
    n_reads = len(read_len)
    out = np.zeros(n_reads * K, dtype=CLASS)
    for r in range(n_reads):
        n = min(int(seed["n_cands"][r]), K)
        L = min(max(int(read_len[r]), 0), read_size)
        c = chains[r * K:r * K + n]
        ivals = [interval(int(c["q_lo"][i]), int(c["q_hi"][i]), int(text_pos[r * K + i]) >> 63, L) for i in range(n)]
        rows = classify_read(ivals, [int(x) for x in c["score"]], [int(x) for x in c["n_anchors"]], mask_q8)
        for i, row in enumerate(rows):
            out[r * K + i] = row
    return out


# ---- rule 9c ---------------------------------------------------------------------------------------------------------------------
def aln_mapq(b, s2, nb, score_unit):
    if nb > 1:
        return 0
    if s2 == INT32_MAX:
        return 60
    return min(60, 6 * max(s2 - b, 0) // score_unit)


def chosen(K, r, sel, cls):
    """(chain_mapq, class flags) of read r's chosen slot, or None where rule 9c calls the read unmapped."""
    if sel == NONE or ((sel - r * K) & 0xFFFFFFFF) >= K or cls["flags"][sel] == 0:
        return None
    parent = int(cls["parent"][sel])
    return (int(cls["mapq"][r * K + parent]) if parent < K else 0), int(cls["flags"][sel])


def read_mapq(K, score_unit, best, mates, cls):
    """aim_read_mapq_t[n_reads] as read_mapq_kernel writes it; mates is None or aim_mate_t[n_reads / 2]."""
    n_reads = len(best)
    out = np.zeros(n_reads, dtype=MAPQ)
    for r in range(n_reads):
        sel = int(best["best_pair"][r])
        ev = (int(best["best_score"][r]), int(best["second_score"][r]), int(best["n_best"][r]))
        proper, mate = False, None
        if mates is not None:
            mt = mates[r // 2]
            sel = int(mt["best_pair"][r & 1])
            if int(mt["flags"]) & MATE_PROPER:
                proper = True
                ev = (int(mt["score_sum"]), int(mt["second_sum"]), int(mt["n_best"]))
                mate = chosen(K, r ^ 1, int(mt["best_pair"][(r & 1) ^ 1]), cls)
        got = chosen(K, r, sel, cls)
        if got is None:
            out[r] = (sel, 0, 0, 0, UNMAPPED)
            continue
        chain, fl = got
        aln = aln_mapq(*ev, score_unit)
        anchored = max(chain, mate[0] if mate else 0) if proper else chain
        flags = (MAPQ_SECONDARY if fl & SECONDARY else 0) | (MAPQ_SUPPLEMENTARY if fl & SUPPLEMENTARY else 0) | (PROPER if proper else 0)
        out[r] = (sel, min(aln, anchored), chain, aln, flags)
    return out


# ---- the batches -----------------------------------------------------------------------------------------------------------------
SYN_READ_SIZE = 1024


def synthetic(seed, n_reads, K):
    """Random chain-kernel outputs for n_reads reads of K slots in rows of SYN_READ_SIZE: dict(read_len, text_pos, seed, chains).
    Scores descend within a read; both strands; n_cands from 0 to K and some above K; some read_len outside 0..read_size; every
    second read has its intervals on a grid of L / 8, so that 256 * ov == mask * min(len) occurs exactly; a few chains are malformed
    (q_hi <= q_lo, score 0). The slots from n_cands on hold noise, which the rule never looks at. Read r depends on (seed, K, r) only
    through the generator's sequence, so a prefix of a batch is the batch of fewer reads."""
    rng = np.random.default_rng([seed, K])
    rs = SYN_READ_SIZE
    read_len = np.zeros(n_reads, dtype=np.int32)
    text_pos = np.zeros(n_reads * K, dtype=np.uint64)
    seeds = np.zeros(n_reads, dtype=m.SEED)
    chains = np.zeros(n_reads * K, dtype=cm.CHAIN)
    for r in range(n_reads):
        kind = int(rng.integers(0, 16))
        L = (-5, rs + 40, 0)[kind] if kind < 3 else 8 * int(rng.integers(8, rs // 8 + 1))
        read_len[r] = L
        L = min(max(L, 0), rs)
        n = int(rng.integers(0, K + 1)) if rng.integers(0, 8) else K + int(rng.integers(1, 4))
        seeds[r] = (n, [int(rng.integers(0, 1024)), int(rng.integers(0, 1024))], int(rng.integers(0, 2)))
        scores = np.sort(rng.integers(11, 400 if r % 3 else 40, size=K))[::-1]
        for i in range(K):
            slot = r * K + i
            if r % 2 == 0 and L >= 64:                       # on the grid of L / 8
                g = L // 8
                a = int(rng.integers(0, 8))
                b = int(rng.integers(a + 1, 9))
                q_lo, q_hi = a * g, b * g
            else:
                q_lo = int(rng.integers(0, rs))
                q_hi = int(rng.integers(q_lo + 1, rs + 1))
            score = int(scores[i])
            if rng.integers(0, 40) == 0:                     # malformed
                q_lo, q_hi, score = (q_hi, q_lo, score) if rng.integers(0, 2) else (q_lo, q_lo, 0)
            chains[slot] = (score, int(rng.integers(1, 30)), 0, q_lo, q_hi, int(rng.integers(0, 2000)))
            text_pos[slot] = np.uint64(int(rng.integers(0, 1 << 32)) | (int(rng.integers(0, 2)) << 63))
    return dict(read_len=read_len, text_pos=text_pos, seed=seeds, chains=chains)


def synthetic_best(seed, n_reads, K):
    """(aim_best_t[n_reads], aim_mate_t[n_reads / 2]) over n_reads * K slots (n_reads even): n_best > 1, second_score == INT32_MAX,
    negative scores, best_pair == UINT32_MAX, a best_pair inside another read's slots (still inside the array), and proper and
    non-proper mates, whose chosen candidates need not be the reads' own."""
    assert n_reads % 2 == 0
    rng = np.random.default_rng([seed, K, 9])
    best = np.zeros(n_reads, dtype=BEST)
    mates = np.zeros(n_reads // 2, dtype=MATE)

    def pick(r):
        kind = int(rng.integers(0, 12))
        if kind == 0:
            return NONE
        if kind == 1:
            return int(rng.integers(0, n_reads * K))          # anywhere in the array: usually another read's slot
        return r * K + int(rng.integers(0, K))

    def scores():
        b = int(rng.integers(-300, 300))
        kind = int(rng.integers(0, 6))
        if kind == 0:
            return b, b, int(rng.integers(2, 5))              # a tie
        if kind == 1:
            return b, INT32_MAX, 1
        return b, b + int(rng.integers(0, 60)), 1
    for r in range(n_reads):
        sel = pick(r)
        best[r] = (sel,) + (scores() if sel != NONE else (INT32_MAX, INT32_MAX, 0))
    for p in range(n_reads // 2):
        proper = bool(rng.integers(0, 2))
        b, s2, nb = scores()
        if proper:
            mates[p] = ([pick(2 * p), pick(2 * p + 1)], b, s2, nb, MATE_PROPER, [0, 0])
        else:
            mates[p] = ([int(best["best_pair"][2 * p]), int(best["best_pair"][2 * p + 1])], b, INT32_MAX, 0, 0, [0, 0])
    return best, mates


CHIMERIC_SIZE, CHIMERIC_HALF, CHIMERIC_EDITS = 1024, 400, 12
CHIMERIC_ROW = (11, 1, 10, 8, 96, 16, 2, 4)        # (k, stride, w, max_occ, band, flank, min_votes, K)


def chimeric_reads(ref=None, seed=77):
    """32 reads in rows of 1 024 over seed_model's reference: 400 bases from a clean position plus 400 from a second locus, 12 edits
    per half. The second half is reverse-complemented in every odd read, the whole read in every eighth, and in every fourth read the
    second half is ref[at - 50, at + 350) around a planted copy, so that it has secondaries of its own. Returns (rows, read_len)."""
    ref = m.make_reference() if ref is None else ref
    rng = np.random.default_rng(seed)
    n, h = 32, CHIMERIC_HALF
    rows, rl = np.zeros((n, CHIMERIC_SIZE), dtype=np.uint8), np.zeros(n, dtype=np.int32)
    for r in range(n):
        p1 = m.clean_position(rng, h)
        if r % 4 == 0:
            p2 = m.PLANT_AT[int(rng.integers(0, len(m.PLANT_AT)))] - 50
        else:
            p2 = m.clean_position(rng, h)
            while abs(p2 - p1) < 2 * h:
                p2 = m.clean_position(rng, h)
        first, second = m.edit(rng, ref[p1:p1 + h], CHIMERIC_EDITS), m.edit(rng, ref[p2:p2 + h], CHIMERIC_EDITS)
        if r % 2:
            second = m.revcomp(second)
        read = np.concatenate([first, second])[:CHIMERIC_SIZE]
        if r % 8 == 0:
            read = m.revcomp(read)
        rows[r, :len(read)], rl[r] = read, len(read)
    return rows, rl


PLANTED_SIZE = 128


def planted_reads(ref=None, seed=78):
    """32 error-free reads of 100 bases from inside the 300-base planted segment, from any of its three copies, both strands, in rows
    of 128. Returns (rows, read_len)."""
    ref = m.make_reference() if ref is None else ref
    rng = np.random.default_rng(seed)
    n = 32
    rows, rl = np.zeros((n, PLANTED_SIZE), dtype=np.uint8), np.full(n, 100, dtype=np.int32)
    for r in range(n):
        at = m.PLANT_AT[r % 3] + int(rng.integers(0, m.PLANT_LEN - 100 + 1))
        read = ref[at:at + 100].copy()
        rows[r, :100] = m.revcomp(read) if r % 2 else read
    return rows, rl
