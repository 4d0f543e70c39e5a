"""Rule 14c (include/aim_hip.h, AIM_FEATURE_PAIRED) in plain numpy and Python integers, written from the text of the rule: the rescue
rows, the choice per read pair with apply, and the mate fields of the records. One read pair at a time, no vectorising: the point is to
be obviously the rule. synthetic_tables() builds the slot tables the CPU and GPU tests feed both sides."""
import numpy as np

import map_records_model as mm

SEG_DTYPE, CLASS_DTYPE, SAM_DTYPE, RECORD_DTYPE = mm.SEG_DTYPE, mm.CLASS_DTYPE, mm.SAM_DTYPE, mm.RECORD_DTYPE
REQUEST_DTYPE = np.dtype([("pattern_len", "<i4"), ("text_len", "<i4"), ("padding", "<i4"), ("idx", "<u4")])
PAIR_DTYPE = np.dtype([("slot", "<u4", (2,)), ("score_sum", "<i4"), ("second_sum", "<i4"), ("n_best", "<u4"), ("flags", "<u4"), ("span", "<i8")])
MATE_DTYPE = np.dtype([("mate_pos", "<u8"), ("tlen", "<i4"), ("mate_contig", "<u4")])
assert PAIR_DTYPE.itemsize == 32 and MATE_DTYPE.itemsize == 16 and REQUEST_DTYPE.itemsize == 16
SEG_VALID, SEG_LEFT_OPEN, SEG_RIGHT_OPEN = 0x1, 0x4, 0x8
SAM_UNMAPPED, SAM_REVERSE = mm.SAM_UNMAPPED, mm.SAM_REVERSE
RESCUE = 0x1
PROPER, TRIED_A, TRIED_B, RESCUED_A, RESCUED_B = 0x1, 0x2, 0x4, 0x8, 0x10
MINUS_STRAND = 1 << 63
CONTIG_NONE = 0xFFFFFFFF
INT_MAX = 2 ** 31 - 1
NONE = 0xFFFFFFFF


class Params:
    """aim_map_pair_params_t as the model reads it."""

    def __init__(self, min_span, max_span, unpaired_penalty=0, options=RESCUE, rescue_size=0):
        self.min_span, self.max_span, self.unpaired_penalty, self.options, self.rescue_size = min_span, max_span, unpaired_penalty, options, rescue_size


def clamp(v):
    return min(v, INT_MAX - 1)


def cand(sam_row, contig):
    """What the rule reads of a mapped slot or a rescue row."""
    return {"pos": int(sam_row["pos"]), "span": int(sam_row["ref_span"]), "score": int(sam_row["score"]), "rev": bool(sam_row["flags"] & SAM_REVERSE),
            "contig": contig}


def proper_span(pp, x, y):
    """The span of the combination of x (read 2m) and y (read 2m + 1) when it is proper, else None."""
    if x["contig"] != y["contig"] or x["rev"] == y["rev"]:
        return None
    f, r = (y, x) if x["rev"] else (x, y)
    span = r["pos"] + r["span"] - f["pos"]
    return span if f["pos"] <= r["pos"] and pp.min_span <= span <= pp.max_span else None


def read_cands(K, r, mapped, sam, contig):
    """{i: candidate} over the mapped slots of read r."""
    return {i: cand(sam[r * K + i], int(contig[r * K + i]) if contig is not None else 0) for i in range(K) if mapped[r, i]}


def best_of(pp, ca, cb, K=None):
    """(cost, i, j, n_best, second, span) over every proper combination of the candidates ca x cb but (K, K), or None: lowest cost, then
    lowest i, then lowest j; n_best combinations have that cost, and second is the lowest cost among the others (INT_MAX: none), as in
    aim_mate_t."""
    combos = []
    for i, x in ca.items():
        for j, y in cb.items():
            span = None if i == K and j == K else proper_span(pp, x, y)
            if span is not None:
                combos.append((clamp(x["score"] + y["score"]), i, j, span))
    if not combos:
        return None
    combos.sort()
    cost, i, j, span = combos[0]
    others = [c[0] for c in combos[1:]]            # every combination but the chosen one: with a tie, second is the cost itself
    return cost, i, j, sum(1 for c in combos if c[0] == cost), min(others) if others else INT_MAX, span


def proper_combos(pp, ca, cb, K=None):
    """[(cost, i, j, 1, INT_MAX, span)]: every proper combination of ca x cb but (K, K), each as the result of the set that holds it alone."""
    out = []
    for i, x in ca.items():
        for j, y in cb.items():
            span = None if i == K and j == K else proper_span(pp, x, y)
            if span is not None:
                out.append((clamp(x["score"] + y["score"]), i, j, 1, INT_MAX, span))
    return out


def combine(a, b):
    """The results of two disjoint sets of combinations (or None for an empty set) as the result of their union: what the lanes of a
    read pair do with their parts. Commutative and associative, so neither the order nor the split into parts shows in best_of's answer."""
    if a is None or b is None:
        return a if b is None else b
    lo, hi = (a, b) if a[:3] <= b[:3] else (b, a)
    tie = lo[0] == hi[0]
    return (lo[0], lo[1], lo[2], lo[3] + hi[3] if tie else lo[3], min(lo[4], hi[4], hi[0]), lo[5])


def read_length(read_len, read_size, r):
    return min(max(int(read_len[r]), 0), read_size)


def tried(pp, read_size, read_len, mapped, none_proper, b):
    """Whether the rescue of read b is tried; none_proper: no proper combination exists among the mapped slots of b and its mate."""
    return bool(pp.options & RESCUE) and bool(mapped[b ^ 1].any()) and none_proper and read_length(read_len, read_size, b) > 0


def rescue_rows(pp, K, read_size, ref_len, n_reads, read_len, reads, seg, sam, contig=None, starts=None, lens=None):
    """(requests REQUEST_DTYPE[n_reads], text_pos uint64[n_reads], {b: the read_size bytes written at b * rescue_size})."""
    mapped = mm.mapped_slots(K, n_reads, seg, sam)
    req = np.zeros(n_reads, dtype=REQUEST_DTYPE)
    tpos = np.zeros(n_reads, dtype=np.uint64)
    rows = {}
    for b in range(n_reads):
        req["idx"][b] = b
        if b % 2 == 0:
            none_proper = best_of(pp, read_cands(K, b, mapped, sam, contig), read_cands(K, b + 1, mapped, sam, contig)) is None
        if not tried(pp, read_size, read_len, mapped, none_proper, b):
            continue
        a = b ^ 1
        rep = int(np.nonzero(mapped[a])[0][0])
        A = cand(sam[a * K + rep], int(contig[a * K + rep]) if contig is not None else 0)
        L = read_length(read_len, read_size, b)
        c_lo, c_hi = 0, ref_len
        if contig is not None and A["contig"] < len(starts):
            c_lo = int(starts[A["contig"]])
            c_hi = c_lo + int(lens[A["contig"]])
        if A["rev"]:
            E = A["pos"] + A["span"]
            lo, hi, strand = max(E - pp.max_span, c_lo), min(E - pp.min_span + L, c_hi), 0
        else:
            lo, hi, strand = max(A["pos"] + pp.min_span - L, c_lo), min(A["pos"] + pp.max_span, c_hi), MINUS_STRAND
        if hi - lo >= L:
            req["pattern_len"][b], req["text_len"][b] = L, hi - lo
            tpos[b] = lo | strand
            rows[b] = np.array(reads[b][:read_size], dtype=np.uint8)
    return req, tpos, rows


def select(pp, K, read_size, n_reads, read_len, seg, sam, cls, contig, res_sam, cigar_base=0, md_base=0):
    """(pairs PAIR_DTYPE[n_reads / 2], seg, sam, cls, contig after apply); the inputs are not touched."""
    mapped = mm.mapped_slots(K, n_reads, seg, sam)
    seg, sam, cls = seg.copy(), sam.copy(), cls.copy()
    contig_in = contig
    contig = contig.copy() if contig is not None else None
    pairs = np.zeros(n_reads // 2, dtype=PAIR_DTYPE)
    for m in range(n_reads // 2):
        ra, rb = 2 * m, 2 * m + 1
        ca, cb = read_cands(K, ra, mapped, sam, contig_in), read_cands(K, rb, mapped, sam, contig_in)
        rep_a, rep_b = min(ca) if ca else None, min(cb) if cb else None
        best = best_of(pp, ca, cb)
        t_a, t_b = tried(pp, read_size, read_len, mapped, best is None, ra), tried(pp, read_size, read_len, mapped, best is None, rb)
        ea, eb = dict(ca), dict(cb)                    # ... plus index K for a mapped rescue row, on its anchor's contig
        if t_a and not res_sam["flags"][ra] & SAM_UNMAPPED:
            ea[K] = cand(res_sam[ra], cb[rep_b]["contig"])
        if t_b and not res_sam["flags"][rb] & SAM_UNMAPPED:
            eb[K] = cand(res_sam[rb], ca[rep_a]["contig"])
        if t_a or t_b:                                 # (a rescue is tried only where the mapped slots have no proper combination)
            best = best_of(pp, ea, eb, K)
        unpaired = clamp(ca[rep_a]["score"] + cb[rep_b]["score"] + pp.unpaired_penalty) if ca and cb else None
        o = pairs[m]
        o["flags"] = (TRIED_A if t_a else 0) | (TRIED_B if t_b else 0)
        if best is not None and (unpaired is None or best[0] <= unpaired):
            cost, i, j, n, second, span = best
            o["slot"] = (ra * K + i, rb * K + j)
            o["score_sum"], o["second_sum"], o["n_best"], o["span"] = cost, second, n, span
            o["flags"] |= PROPER | (RESCUED_A if i == K else 0) | (RESCUED_B if j == K else 0)
            for b, a, idx, rep in ((ra, rb, i, rep_b), (rb, ra, j, rep_a)):
                if idx != K:
                    continue
                row = res_sam[b].copy()                # apply
                row["cigar_offset"] = (int(row["cigar_offset"]) + cigar_base) & 0xFFFFFFFF
                row["md_offset"] = (int(row["md_offset"]) + md_base) & 0xFFFFFFFF
                sam[b * K] = row
                L = read_length(read_len, read_size, b)
                seg[b * K] = (0, L, L, SEG_VALID | SEG_LEFT_OPEN | SEG_RIGHT_OPEN, 0)
                for k in range(1, K):
                    seg["flags"][b * K + k] &= ~np.uint8(SEG_VALID)
                if contig is not None:
                    contig[b * K] = contig_in[a * K + rep]
                cls["mapq"][b * K] = cls["mapq"][a * K + rep]
        else:
            o["slot"] = (ra * K + rep_a if ca else NONE, rb * K + rep_b if cb else NONE)
            o["score_sum"] = unpaired if unpaired is not None else INT_MAX
            o["second_sum"] = best[0] if best is not None and unpaired is not None else INT_MAX
    return pairs, seg, sam, cls, contig


def mates(K, n_reads, pairs, seg, sam, contig, starts, rec_offsets, records):
    """(records with the paired flag bits, MATE_DTYPE per record) from the slot arrays as apply left them."""
    mapped = mm.mapped_slots(K, n_reads, seg, sam)
    rec = records.copy()
    out = np.zeros(len(rec), dtype=MATE_DTYPE)
    for t in range(int(rec_offsets[n_reads])):
        o = rec[t]
        r, slot = int(o["read"]), int(o["slot"])
        mate, p = r ^ 1, pairs[r >> 1]
        proper = bool(p["flags"] & PROPER)
        own, other = int(p["slot"][r & 1]), int(p["slot"][(r & 1) ^ 1])
        own = r * K if own == r * K + K else own
        other = mate * K if other == mate * K + K else other
        mate_mapped = bool(mapped[mate].any())
        ms = mate * K + int(np.nonzero(mapped[mate])[0][0]) if mate_mapped else None
        if mate_mapped and proper and mate * K <= other < mate * K + K:
            ms = other
        chosen = proper and slot == own
        flags = 0x1 | (0x80 if r & 1 else 0x40) | (0 if mate_mapped else 0x8) | (0x2 if chosen else 0)
        own_flags = int(o["sam"]["flags"])
        if mate_mapped:
            if sam["flags"][ms] & SAM_REVERSE:
                flags |= 0x20
            c = int(contig[ms]) if contig is not None else 0
            start = int(starts[c]) if contig is not None and c < len(starts) else 0
            out["mate_pos"][t], out["mate_contig"][t] = (int(sam["pos"][ms]) - start) & (2 ** 64 - 1), c
        elif not own_flags & SAM_UNMAPPED:
            out["mate_pos"][t], out["mate_contig"][t] = o["sam"]["pos"], (o["sam"]["pad"] if contig is not None else 0)
        else:
            out["mate_pos"][t], out["mate_contig"][t] = 0, (CONTIG_NONE if contig is not None else 0)
        span = min(int(p["span"]), INT_MAX)
        out["tlen"][t] = (-span if own_flags & SAM_REVERSE else span) if chosen else 0
        rec["sam"]["flags"][t] = own_flags | flags
    return rec, out


# ---- synthetic slot tables --------------------------------------------------------------------------------------------------------
MIN_SPAN, MAX_SPAN, READ_SIZE, RESCUE_SIZE = 300, 500, 104, 512
CONTIG_LENS, SPACER = (30000, 25000, 40000), 160


def layout():
    """(starts, lens uint32[3], ref_len): rule 13c's layout of the three contigs."""
    starts, at = [], 0
    for c, n in enumerate(CONTIG_LENS):
        at += SPACER if c else 0
        starts.append(at)
        at += n
    return np.array(starts, dtype=np.uint32), np.array(CONTIG_LENS, dtype=np.uint32), at


def params(unpaired_penalty=17, rescue=True):
    return Params(MIN_SPAN, MAX_SPAN, unpaired_penalty, RESCUE if rescue else 0, RESCUE_SIZE)


def synthetic_tables(seed, K, n_reads, contigs):
    """Random slot tables of n_reads * K rows whose every byte is set (aim_sam_t.flags: the bits the split path sets), shaped so that every branch of rule 14c occurs: a dict with seg,
    sam, cls, contig (None without contigs), res_sam, read_len, reads, starts, lens, ref_len. Positions lie inside the reference;
    scores come from a few values, so ties in cost are common; about a third of the read pairs carry a planted partner for some slot at
    a span drawn from {min_span - 1, min_span, inside, max_span, max_span + 1}; anchors are planted at position 0, at the end of the
    reference and at contig edges, so windows are cut on either side; the rescue records are placed relative to their anchor the same
    way. The first pairs are fixed cases: see the comments."""
    rng = np.random.default_rng([int(seed), K, n_reads, int(contigs), 0x70616972])
    starts, lens, ref_len = layout()
    S = n_reads * K
    raw = lambda dt, n: rng.integers(0, 256, size=n * dt.itemsize, dtype=np.uint8).view(dt).copy()
    seg, sam, cls, res_sam = raw(SEG_DTYPE, S), raw(SAM_DTYPE, S), raw(CLASS_DTYPE, S), raw(SAM_DTYPE, n_reads)
    contig_of = lambda pos: int(np.searchsorted(starts, pos, side="right") - 1)

    def put(row, pos, rev, score=None, span=None, unmapped=False):
        row["pos"] = min(max(int(pos), 0), ref_len - 1)
        row["ref_span"] = int(rng.integers(90, 111)) if span is None else span
        row["score"] = int(rng.choice([0, 3, 6, 6, 11, 40])) if score is None else score
        row["flags"] = (int(row["flags"]) & mm.SAM_SUPPLEMENTARY) | (SAM_REVERSE if rev else 0) | (SAM_UNMAPPED if unmapped else 0)   # the bits the split path sets
        row["cigar_offset"], row["md_offset"] = int(rng.integers(0, 1 << 20)), int(rng.integers(0, 1 << 20))

    def partner(row, other, kind):
        """`row` becomes the mate record of `other` at a span of the given kind."""
        span = {0: MIN_SPAN - 1, 1: MIN_SPAN, 2: int(rng.integers(MIN_SPAN, MAX_SPAN + 1)), 3: MAX_SPAN, 4: MAX_SPAN + 1}[kind]
        if other["flags"] & SAM_REVERSE:       # row is the forward one: pos_f = pos_r + ref_span_r - span
            put(row, int(other["pos"]) + int(other["ref_span"]) - span, False)
        else:
            rs = int(rng.integers(90, 111))
            put(row, int(other["pos"]) + span - rs, True, span=rs)

    edges = [0, 3, ref_len - 1, ref_len - 120, int(starts[1]), int(starts[1]) + 40, int(starts[1] - SPACER - 100), int(starts[2]) + 7, int(starts[0] + lens[0]) - 30]
    for s in range(S):
        pos = int(rng.choice(edges)) if rng.random() < 0.15 else int(rng.integers(0, ref_len))
        put(sam[s], pos, rng.random() < 0.5, unmapped=rng.random() < 0.25)
    valid = rng.random(S) < 0.6
    for m in range(n_reads // 2):
        if rng.random() < 0.35:
            i, j = int(rng.integers(0, K)), int(rng.integers(0, K))
            partner(sam[(2 * m + 1) * K + j], sam[2 * m * K + i], int(rng.integers(0, 5)))
            if rng.random() < 0.5 and K > 1:       # a second proper combination of the same scores: a tie in cost
                i2, j2 = (i + 1) % K, (j + 1) % K
                put(sam[2 * m * K + i2], sam["pos"][2 * m * K + i], bool(sam["flags"][2 * m * K + i] & SAM_REVERSE), score=int(sam["score"][2 * m * K + i]))
                partner(sam[(2 * m + 1) * K + j2], sam[2 * m * K + i2], 2)
                sam["score"][(2 * m + 1) * K + j2] = sam["score"][(2 * m + 1) * K + j]
    contig = np.zeros(S, dtype=np.uint32)
    for s in range(S):
        contig[s] = contig_of(int(sam["pos"][s])) if rng.random() < 0.9 else int(rng.integers(0, 3))
    read_len = rng.choice(np.array([100, 104, 100, 57, 0, -3, 120], dtype=np.int32), size=n_reads).astype(np.int32)

    def fix(m, a_slots, b_slots):
        """Pair m: slots (i, pos, rev, score) mapped as given, every other slot of the two reads not valid."""
        for r, slots in ((2 * m, a_slots), (2 * m + 1, b_slots)):
            valid[r * K:(r + 1) * K] = False
            read_len[r] = 100
            for i, pos, rev, score in slots:
                if i < K:
                    put(sam[r * K + i], pos, rev, score=score, span=100)
                    valid[r * K + i] = True
                    contig[r * K + i] = contig_of(int(sam["pos"][r * K + i]))
    mapped = valid.reshape(n_reads, K) & ((sam["flags"] & SAM_UNMAPPED) == 0).reshape(n_reads, K)
    for b in range(n_reads):                                                       # the rescue records, placed against their anchor
        a = b ^ 1
        put(res_sam[b], int(rng.integers(0, ref_len)), rng.random() < 0.5, unmapped=rng.random() < 0.3)
        if mapped[a].any() and rng.random() < 0.7:
            partner(res_sam[b], sam[a * K + int(np.nonzero(mapped[a])[0][0])], int(rng.integers(0, 5)))
    P = 1000
    end0 = int(starts[0] + lens[0])
    if n_reads >= 26:
        fix(0, [], [])                                                             # both reads without a mapped slot
        fix(1, [(0, P, False, 5)], [])                                             # b is rescued, and there is no unpaired cost
        put(res_sam[3], P + 250, True, score=9, span=100)
        fix(2, [(0, P, False, 5), (1, P + 10, False, 5)], [(0, P + 300, True, 5), (1, P + 310, True, 5)])       # four proper combinations of one cost
        fix(3, [(0, P, False, 0)], [(0, P + MIN_SPAN - 100, True, 0)])             # a span of exactly min_span
        fix(4, [(0, P + MAX_SPAN - 100, True, 0)], [(0, P, False, 0)])             # ... of max_span, the reverse record read 2m's
        fix(5, [(0, P, False, 0)], [(0, P + MIN_SPAN - 101, True, 0)])             # min_span - 1: rescue tried on both sides
        put(res_sam[10], P - 50, True, unmapped=True)
        put(res_sam[11], P + 200, True, score=2, span=100)
        fix(6, [(0, P, False, 0)], [(0, P + MAX_SPAN - 99, True, 0)])              # max_span + 1
        put(res_sam[12], P + 60, False, score=1, span=100)                          # ... and both rescue rows proper with the other's anchor: (0, K) before (K, 0)
        put(res_sam[13], P + 280, True, score=1, span=100)
        fix(7, [(0, 20000, False, 0), (1, P, False, 30)], [(0, 5000, True, 0), (1, P + 300, True, 30)])          # proper, but dearer than unpaired + penalty
        fix(8, [(0, 250, True, 4)], [(0, 20000, False, 4)])                        # read 1's window cut by position 0, read 0's by nothing
        fix(9, [(0, ref_len - 400, False, 4)], [(0, 40, True, 4)])                 # ... by ref_len; and a window that is cut away: an empty row
        fix(10, [(0, int(starts[1]) + 250, True, 4)], [(0, end0 - 400, False, 4)])                               # ... by a contig's start and by a contig's end
        fix(11, [(0, P, False, 5)], [(0, 25000, True, 5)])                         # the rescue record lands on the wrong strand: tried, not taken
        put(res_sam[23], P + 250, False, score=0, span=100)
        fix(12, [(0, end0 - 150, False, 5)], [(0, int(starts[1]) + 10, True, 5)])  # a proper span in the concatenation, over two contigs
        read_len[24], read_len[25] = 0, 100                                        # a read of length 0 is never rescued; its mate is
    seg["flags"] = (seg["flags"] & ~np.uint8(SEG_VALID)) | valid.astype(np.uint8)
    reads = rng.integers(0, 256, size=(n_reads, READ_SIZE), dtype=np.uint8)
    return {"seg": seg, "sam": sam, "cls": cls, "contig": contig if contigs else None, "res_sam": res_sam, "read_len": read_len, "reads": reads,
            "starts": starts, "lens": lens, "ref_len": ref_len}
