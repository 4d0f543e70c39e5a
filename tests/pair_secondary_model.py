"""Rule 17c (include/aim_hip.h, AIM_FEATURE_PAIR_SECONDARY) in plain numpy and Python integers, written from the text of the rule:
rule 14c's pairing over every slot that rule 16c part 2 gave a role -- secondaries included --, the per-read pair MAPQ from the
runner-up among the combinations, apply onto d_sec and the slot arrays, and the mate fields. One read pair at a time, no vectorising:
the point is to be obviously the rule. What rule 14c already says -- a candidate, a proper span, best_of, the windows -- is taken from
tests/pair_model.py; nothing is shared with the library."""
import numpy as np

import map_records_model as mm
import pair_model as pm
import secondary_model as scm

PAIR_MAPQ_DTYPE = np.dtype([("alt_sum", "<i4", (2,)), ("mapq", "u1", (2,)), ("pair_mapq", "u1", (2,)), ("own_mapq", "u1", (2,)), ("tied", "u1", (2,))])
assert PAIR_MAPQ_DTYPE.itemsize == 16
INT_MAX, NONE = pm.INT_MAX, pm.NONE
OWN_PLUS = 40              # bwa-mem's paired MAPQ: pairing lifts a read's own MAPQ by 40 at the most


def taking_part(K, n_reads, seg, sam, sec):
    """bool[n_reads, K]: the slots the combinations run over -- mapped (rule 12c) and with a role from rule 16c part 2, which gives one to
    every mapped slot the pipeline produces."""
    return mm.mapped_slots(K, n_reads, seg, sam) & (sec["role"].reshape(n_reads, K) != 0)


def representative(K, r, part, sec):
    """Candidate index of read r's representative -- the slot of role 1 in the family of lowest j that has a winner -- or None."""
    own = [(int(sec["family"][r * K + i]), i) for i in range(K) if part[r, i] and sec["role"][r * K + i] == 1]
    return min(own)[1] if own else None


def bounds(pp, est):
    """pp with the bounds of an aim_pair_estimate_t where one is given."""
    return pp if est is None else pm.Params(int(est["min_span"]), int(est["max_span"]), pp.unpaired_penalty, pp.options, pp.rescue_size)


def anchor_cap(chains, slot):
    return 6 * min(int(chains["n_anchors"][slot]), 10) if int(chains["score"][slot]) else 0


def rescue_rows(pp, K, read_size, ref_len, n_reads, read_len, reads, seg, sam, sec, contig=None, starts=None, lens=None, est=None):
    """(requests REQUEST_DTYPE[n_reads], text_pos uint64[n_reads], {b: the read_size bytes written at b * rescue_size}): rule 14c's rows
    with the representative above as the anchor, tried only where the slots that take part have no proper combination."""
    pp = bounds(pp, est)
    part = taking_part(K, n_reads, seg, sam, sec)
    req = np.zeros(n_reads, dtype=pm.REQUEST_DTYPE)
    tpos = np.zeros(n_reads, dtype=np.uint64)
    rows = {}
    for b in range(n_reads):
        req["idx"][b] = b
        if b % 2 == 0:
            none_proper = pm.best_of(pp, pm.read_cands(K, b, part, sam, contig), pm.read_cands(K, b + 1, part, sam, contig)) is None
        a = b ^ 1
        rep = representative(K, a, part, sec)
        L = pm.read_length(read_len, read_size, b)
        if not (pp.options & pm.RESCUE and rep is not None and none_proper and L > 0):
            continue
        A = pm.cand(sam[a * K + rep], int(contig[a * K + rep]) if contig is not None else 0)
        c_lo, c_hi = 0, ref_len
        if contig is not None and A["contig"] < len(starts):
            c_lo = int(starts[A["contig"]])
            c_hi = c_lo + int(lens[A["contig"]])
        if A["rev"]:
            E = A["pos"] + A["span"]
            lo, hi, strand = max(E - pp.max_span, c_lo), min(E - pp.min_span + L, c_hi), 0
        else:
            lo, hi, strand = max(A["pos"] + pp.min_span - L, c_lo), min(A["pos"] + pp.max_span, c_hi), pm.MINUS_STRAND
        if hi - lo >= L:
            req["pattern_len"][b], req["text_len"][b] = L, hi - lo
            tpos[b] = lo | strand
            rows[b] = np.array(reads[b][:read_size], dtype=np.uint8)
    return req, tpos, rows


def pair_mapq(combos, c, v, side, unpaired, rep, score_unit):
    """(alt, tied, pair_mapq) of one read: `side` 0 looks at i, 1 at j; v is the chosen index of that read and rep its representative."""
    others = [x[0] for x in combos if x[1 + side] != v]
    alt = min(others) if others else INT_MAX
    if unpaired is not None and rep != v:
        alt = min(alt, unpaired)
    tied = sum(1 for x in others if x == c)
    q = 0 if tied else 60 if alt == INT_MAX else min(60, 6 * max(alt - c, 0) // score_unit)
    return alt, tied, q


def select(pp, K, read_size, n_reads, read_len, seg, sam, cls, contig, sec, chains, res_sam, score_unit, cigar_base=0, md_base=0, est=None):
    """(pairs pm.PAIR_DTYPE[n_reads / 2], PAIR_MAPQ_DTYPE[n_reads / 2], seg, sam, cls, contig, sec after apply); inputs are not touched."""
    pp = bounds(pp, est)
    part = taking_part(K, n_reads, seg, sam, sec)
    seg, sam, cls, sec_in, sec = seg.copy(), sam.copy(), cls.copy(), sec, sec.copy()
    contig_in = contig
    contig = contig.copy() if contig is not None else None
    cls_in = cls.copy()
    pairs = np.zeros(n_reads // 2, dtype=pm.PAIR_DTYPE)
    pq = np.zeros(n_reads // 2, dtype=PAIR_MAPQ_DTYPE)
    pq["alt_sum"] = INT_MAX
    for m in range(n_reads // 2):
        ra, rb = 2 * m, 2 * m + 1
        ca, cb = pm.read_cands(K, ra, part, sam, contig_in), pm.read_cands(K, rb, part, sam, contig_in)
        rep_a, rep_b = representative(K, ra, part, sec_in), representative(K, rb, part, sec_in)
        none_proper = pm.best_of(pp, ca, cb) is None
        rescue = bool(pp.options & pm.RESCUE) and none_proper
        t_a = rescue and rep_b is not None and pm.read_length(read_len, read_size, ra) > 0
        t_b = rescue and rep_a is not None and pm.read_length(read_len, read_size, rb) > 0
        ea, eb = dict(ca), dict(cb)                    # ... plus index K for a mapped rescue row, on its anchor's contig
        if t_a and not res_sam["flags"][ra] & pm.SAM_UNMAPPED:
            ea[K] = pm.cand(res_sam[ra], cb[rep_b]["contig"])
        if t_b and not res_sam["flags"][rb] & pm.SAM_UNMAPPED:
            eb[K] = pm.cand(res_sam[rb], ca[rep_a]["contig"])
        best = pm.best_of(pp, ea, eb, K)
        both = rep_a is not None and rep_b is not None
        unpaired = pm.clamp(ca[rep_a]["score"] + cb[rep_b]["score"] + pp.unpaired_penalty) if both else None
        o = pairs[m]
        o["flags"] = (pm.TRIED_A if t_a else 0) | (pm.TRIED_B if t_b else 0)
        if best is None or (unpaired is not None and best[0] > unpaired):
            o["slot"] = (ra * K + rep_a if rep_a is not None else NONE, rb * K + rep_b if rep_b is not None else NONE)
            o["score_sum"] = unpaired if unpaired is not None else INT_MAX
            o["second_sum"] = best[0] if best is not None and unpaired is not None else INT_MAX
            continue
        cost, vi, vj, n, second, span = best
        o["slot"] = (ra * K + vi, rb * K + vj)
        o["score_sum"], o["second_sum"], o["n_best"], o["span"] = cost, second, n, span
        o["flags"] |= pm.PROPER | (pm.RESCUED_A if vi == K else 0) | (pm.RESCUED_B if vj == K else 0)
        # the per-read pair MAPQ
        combos = pm.proper_combos(pp, ea, eb, K)
        q = []
        for side, (r, v, rep) in enumerate(((ra, vi, rep_a), (rb, vj, rep_b))):
            alt, tied, pmq = pair_mapq(combos, cost, v, side, unpaired, rep, score_unit)
            own = int(sec_in["mapq"][r * K + v]) if v != K and sec_in["role"][r * K + v] == 1 else 0
            q.append({"alt": alt, "tied": tied, "pair": pmq, "own": own, "lifted": max(own, min(pmq, own + OWN_PLUS)),
                      "cap": anchor_cap(chains, r * K + v) if v != K else None})
        for x in q:                                    # a slot is capped by its own chain's anchors ...
            if x["cap"] is not None:
                x["mapq"] = min(x["lifted"], x["cap"])
        for x, y in ((q[0], q[1]), (q[1], q[0])):      # ... a rescue row by its mate's MAPQ, computed first ((K, K) is excluded)
            if x["cap"] is None:
                x["mapq"] = min(x["lifted"], y["mapq"])
        pq[m] = tuple((q[0][k], q[1][k]) for k in ("alt", "mapq", "pair", "own")) + ((min(q[0]["tied"], 255), min(q[1]["tied"], 255)),)
        # apply
        for b, a, v, rep, mapq in ((ra, rb, vi, rep_b, q[0]["mapq"]), (rb, ra, vj, rep_a, q[1]["mapq"])):
            if v == K:                                 # rule 14c's apply, and the read becomes a one-member family 0
                row = res_sam[b].copy()
                row["cigar_offset"] = (int(row["cigar_offset"]) + cigar_base) & 0xFFFFFFFF
                row["md_offset"] = (int(row["md_offset"]) + md_base) & 0xFFFFFFFF
                sam[b * K] = row
                L = pm.read_length(read_len, read_size, b)
                seg[b * K] = (0, L, L, pm.SEG_VALID | pm.SEG_LEFT_OPEN | pm.SEG_RIGHT_OPEN, 0)
                for k in range(1, K):
                    seg["flags"][b * K + k] &= ~np.uint8(pm.SEG_VALID)
                if contig is not None:
                    contig[b * K] = contig_in[a * K + rep]
                # the chain MAPQ the record kernel reports for slot b * K: that of the anchor's family
                cls["mapq"][b * K] = cls_in["mapq"][a * K + min(int(sec_in["family"][a * K + rep]), K - 1)]
                sec[b * K:(b + 1) * K] = np.zeros(K, dtype=scm.SEC_SLOT)
                sec[b * K] = (1, 0, mapq, 0, 1, scm.COMPLETE, 65535)
                continue
            s = b * K + v
            if sec_in["role"][s] == 1:
                sec["mapq"][s] = mapq
                continue
            j = int(sec_in["family"][s])               # a role-2 slot and its family's role-1 slot exchange roles
            for k in range(K):
                if part[b, k] and sec_in["role"][b * K + k] == 1 and sec_in["family"][b * K + k] == j:
                    sec["role"][b * K + k], sec["mapq"][b * K + k] = 2, 0
            sec["role"][s], sec["mapq"][s], sec["aln_mapq"][s], sec["gap"][s] = 1, mapq, 0, 0
            sec["flags"][s] = (int(sec_in["flags"][s]) & ~scm.SWAPPED) | (scm.SWAPPED if v != j else 0)
    return pairs, pq, seg, sam, cls, contig, sec


def mates(K, n_reads, pairs, sam, sec, contig, starts, rec_offsets, records):
    """(records with the paired flag bits, pm.MATE_DTYPE per record) from the slot arrays and d_sec as apply left them: rule 14c's mate
    fields with the representative read from d_sec; a 0x100 record never has 0x2 and its tlen is 0."""
    rec = records.copy()
    out = np.zeros(len(rec), dtype=pm.MATE_DTYPE)
    for t in range(int(rec_offsets[n_reads])):
        o = rec[t]
        r, slot = int(o["read"]), int(o["slot"])
        mate, p = r ^ 1, pairs[r >> 1]
        proper = bool(p["flags"] & pm.PROPER)
        own, other = int(p["slot"][r & 1]), int(p["slot"][(r & 1) ^ 1])
        own = r * K if own == r * K + K else own
        other = mate * K if other == mate * K + K else other
        reps = [(int(sec["family"][mate * K + i]), i) for i in range(K) if sec["role"][mate * K + i] == 1]
        mate_mapped = bool(reps)
        ms = mate * K + min(reps)[1] if mate_mapped else None
        if mate_mapped and proper and mate * K <= other < mate * K + K:
            ms = other
        own_flags = int(o["sam"]["flags"])
        chosen = proper and slot == own and not own_flags & scm.SAM_SECONDARY
        flags = 0x1 | (0x80 if r & 1 else 0x40) | (0 if mate_mapped else 0x8) | (0x2 if chosen else 0)
        if mate_mapped:
            if sam["flags"][ms] & pm.SAM_REVERSE:
                flags |= 0x20
            c = int(contig[ms]) if contig is not None else 0
            start = int(starts[c]) if contig is not None and c < len(starts) else 0
            out["mate_pos"][t], out["mate_contig"][t] = (int(sam["pos"][ms]) - start) & (2 ** 64 - 1), c
        elif not own_flags & pm.SAM_UNMAPPED:
            out["mate_pos"][t], out["mate_contig"][t] = o["sam"]["pos"], (o["sam"]["pad"] if contig is not None else 0)
        else:
            out["mate_pos"][t], out["mate_contig"][t] = 0, (pm.CONTIG_NONE if contig is not None else 0)
        span = min(int(p["span"]), INT_MAX)
        out["tlen"][t] = (-span if own_flags & pm.SAM_REVERSE else span) if chosen else 0
        rec["sam"]["flags"][t] = own_flags | flags
    return rec, out
