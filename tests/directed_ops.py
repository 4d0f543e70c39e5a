"""Directed ops rows for the SAM record kernels (sam_fields.hpp): one scenario on each side of every edge of the two mappings -- the
256-op tile of the wave mapping and its seven carries, the lane's quad and the row word of the fast path, the decimal digit counts of
the MD string, bytes other than M X I D, unmapped rows among mapped ones and the ends of the reference.

A scenario is a walk string (the ops in WALK order), a name and a claim: the CIGAR string without AIM_SAM_EQX and the MD string, in
which '?' stands for one reference byte. `lay` puts scenarios into rows: reversed for strand 1, at a chosen begin_offset mod 4, at
either end of the row, the rest of the row filled with a chosen byte. The expected tuples come from sam_model.row_fields.
Shared by test_directed_ops_cpu.py (the claims, the tile restatement and its mutants) and test_directed_ops_gpu.py (the kernels)."""
import collections
import re

import numpy as np

import sam_model

T = 256                                  # the wave mapping's tile, in ops
MINUS = 1 << 63
UINT32_MAX = 0xFFFFFFFF
MAX_SCORE = 5000
FILLERS = (ord("?"), ord("M"), ord("I"), ord("X"), 0xFF)
RESULT = np.dtype([("max_operations", "<i4"), ("begin_offset", "<i4"), ("end_offset", "<i4"), ("score", "<i4"), ("status", "<i4"), ("idx", "<u4")])
REF_LEN = 40000
PLANT_AT, PLANT = 20000, b"acgtNNnnACGTnacg"     # lower-case and N reference bytes at a known place
REF_TAIL = b"GaNt"                                # the last four reference bytes

# group, name, walk, CIGAR claim ("*": unmapped), MD claim, run with every filler, place: None | ("at", window start) | "end" (the
# window's last reference base, peeled ones included, is ref[ref_len - 1])
Scenario = collections.namedtuple("Scenario", "group name walk cigar md fill place")
# kind: "ok" | "empty" (end = begin) | "inverted" (end < begin) | "status" (not AIM_PAIR_OK) | "overcap" (WFA score MAX_SCORE + 1)
Row = collections.namedtuple("Row", "scn strand shift end filler kind")


def reference(n=REF_LEN):
    ref = sam_model.make_reference(3, n).copy()
    ref[PLANT_AT:PLANT_AT + len(PLANT)] = np.frombuffer(PLANT, dtype=np.uint8)
    ref[-len(REF_TAIL):] = np.frombuffer(REF_TAIL, dtype=np.uint8)
    return ref


def _mixed(n, unit):
    return (unit * (n // len(unit) + 1))[:n]


def _scenarios():
    out = []

    def add(group, name, walk, cigar, md, fill=None, place=None):
        fill = (walk[:1] == b"M" or walk[-1:] == b"M") if fill is None else fill
        out.append(Scenario(group, name, bytes(walk), cigar, md, fill, place))

    M, X, I, D = b"M", b"X", b"I", b"D"
    # ---- T: tile carries ------------------------------------------------------------------------------------------------------------
    for k in (T - 1, T, T + 1, 2 * T, 3 * T - 1):
        add("T", "run@%d" % k, M * k + D * 2 + M * 9, "%dM2I9M" % k, "%d" % (k + 9))
        add("T", "x@%d" % k, M * k + X + M * 9, "%dM" % (k + 10), "%d?9" % k)
        add("T", "del@%d" % k, M * k + I * 3 + M * 9, "%dM3D9M" % k, "%d^???9" % k)
    add("T", "del250-261", M * 250 + I * 12 + M * 20, "250M12D20M", "250^" + "?" * 12 + "20")
    add("T", "del-to-255-x256", M * 250 + I * 6 + X + M * 5, "250M6D6M", "250^??????0?5")
    for p in (254, 255, 256):
        add("T", "IDI@%d" % p, M * p + b"IDI" + M * 7, "%dM1D1I1D7M" % p, "%d^?0^?7" % p)
    add("T", "700M-x", M * 700 + X + M * 3, "704M", "700?3")
    add("T", "700I", M * 2 + I * 700 + M + X + M, "2M700D3M", "2^" + "?" * 700 + "1?1")
    for p in (255, 256, 257, 511, 512, 600):
        lead = _mixed(p, b"DDIDI")
        add("T", "lead%d" % p, lead + b"MMXMM", "%dS5M" % (p - lead.count(I)), "2?2")
        for last in (254, 255, 256):
            trail = _mixed(p, b"DIDDI")
            add("T", "trail%d-last%d" % (p, last), M * last + X + trail, "%dM%dS" % (last + 1, p - trail.count(I)), "%d?0" % last)
    add("T", "range1", M, "1M", "1")
    for n in (3, 4, 5, 255, 256, 257, 512):
        add("T", "range%d" % n, M * (n - 2) + X + M, "%dM" % n, "%d?1" % (n - 2))
    add("T", "core1-DDMII", b"DDMII", "2S1M", "1")
    add("T", "core1-X", X, "1M", "0?0")
    R = 3 * T // 2
    add("T", "MIx3T", b"MI" * R, "1M1D" * (R - 1) + "1M", "1^?" * (R - 1) + "1")
    add("T", "MXx3T", b"MX" * R, "%dM" % (2 * R), "1?" * R + "0")
    add("T", "MDx3T", b"MD" * R, "1M1I" * (R - 1) + "1M1S", "%d" % R)
    add("T", "XIx3T", b"XI" * R, "1M1D" * (R - 1) + "1M", "0?0^?" * (R - 1) + "0?0")
    add("T", "XDx3T", b"XD" * R, "1M1I" * (R - 1) + "1M1S", "0?" * R + "0")
    add("T", "Mx3T", M * (3 * T), "%dM" % (3 * T), "%d" % (3 * T))
    # ---- L: quad and word edges -----------------------------------------------------------------------------------------------------
    for r in range(4):
        add("L", "del@8+%d" % r, M * (8 + r) + I + M * 5, "%dM1D5M" % (8 + r), "%d^?5" % (8 + r))
        add("L", "x@8+%d" % r, M * (8 + r) + X + M * 6, "%dM" % (15 + r), "%d?6" % (8 + r))
        add("L", "ins@8+%d" % r, M * (8 + r) + D + M * 5, "%dM1I5M" % (8 + r), "%d" % (13 + r))
    for e in (1, 2, 3):
        add("L", "core-ends-%d-into-a-word" % e, X + M * (8 + e), "%dM" % (9 + e), "0?%d" % (8 + e))
    for n in (4, 8, 12):
        add("L", "core%dM" % n, M * n, "%dM" % n, "%d" % n)
    add("L", "8M-DD", M * 8 + D * 2, "8M2S", "8", fill=True)
    add("L", "II-8M", I * 2 + M * 8, "8M", "8", fill=True)
    # ---- D: decimal digits and zero counts ------------------------------------------------------------------------------------------
    for c in (0, 9, 10, 99, 100, 999, 1000):
        add("D", "%d-before-x" % c, X + M * c + X + M, "%dM" % (c + 3), "0?%d?1" % c, fill=True)
        add("D", "%d-before-del" % c, X + M * c + I + M, "%dM1D1M" % (c + 1), "0?%d^?1" % c, fill=True)
        add("D", "%d-final" % c, X + M * c, "%dM" % (c + 1), "0?%d" % c, fill=True)
    add("D", "x-first", b"XMM", "3M", "0?2")
    add("D", "x-last", b"MMX", "3M", "2?0")
    add("D", "xx", b"MXXM", "4M", "1?0?1")
    add("D", "x-behind-del", b"MIIXM", "1M2D2M", "1^??0?1")
    add("D", "del-behind-x", b"MXIIM", "2M2D1M", "1?0^??1")
    add("D", "9-10-99-100-in-a-tile", M * 9 + X + M * 10 + X + M * 99 + X + M * 100 + X + M * 3, "225M", "9?10?99?100?3")
    # the five- and six-digit counts (one batch at READ_SIZE 65528)
    add("DL", "99999x-10000del-10000", M * 99999 + X + M * 10000 + I + M * 10000, "110000M1D10000M", "99999?10000^?10000")
    add("DL", "10000x-99999del-9999", M * 10000 + X + M * 99999 + I + M * 9999, "110000M1D9999M", "10000?99999^?9999")
    add("DL", "100000x-9999del-10000", M * 100000 + X + M * 9999 + I + M * 10000, "110000M1D10000M", "100000?9999^?10000")
    add("DL", "9999x-100000del-1", M * 9999 + X + M * 100000 + I + M, "110000M1D1M", "9999?100000^?1")
    add("DL", "99999-final", X + M * 99999, "100000M", "0?99999")
    add("DL", "100000-final", X + M * 100000, "100001M", "0?100000")
    # ---- B: other bytes count as read-only bases ------------------------------------------------------------------------------------
    for byte in (0x00, 0xFF, ord("S"), ord("N"), ord("m"), ord("x")):
        o = bytes([byte])
        add("B", "peel-%02x" % byte, o * 2 + b"MMXM" + o, "2S4M1S", "2?1", fill=True)
        add("B", "core-%02x" % byte, b"MM" + o * 2 + b"XM", "2M2I2M", "2?1", fill=True)
    # ---- U: rows of gaps only (the other unmapped kinds are Row kinds) --------------------------------------------------------------
    add("U", "all-gap-IIDD", b"IIDD", "*", None, fill=True)
    add("U", "all-gap-D", D * 5, "*", None, fill=True)
    add("U", "all-gap-I-tile", I * (T + 3), "*", None, fill=True)
    add("U", "mapped", b"MMXMIMM", "4M1D2M", "2?1^?2", fill=True)
    # ---- R: reference bytes (exact claims: the bytes are planted) -------------------------------------------------------------------
    ref = reference()
    add("R", "window-at-0", b"IIMXM", "3M", "1%s1" % chr(int(ref[3])), fill=True, place=("at", 0))
    add("R", "last-base-mismatch", b"MMMX", "4M", "3t0", fill=True, place="end")
    # (a deletion never ends a core: its last base is the last but one of the reference, an X takes the last)
    add("R", "last-bases-deletion", b"MIIX", "1M2D1M", "1^aN0t0", fill=True, place="end")
    add("R", "last-bases-peeled", b"MXII", "2M", "1a0", fill=True, place="end")
    add("R", "lower-and-N", b"MMXMXMIIIIMX", "6M4D2M", "2a1g1^NNnn1C0", fill=True, place=("at", PLANT_AT - 2))
    add("R", "N-mismatch", b"MXXMIM", "4M1D1M", "1N0n1^A1", fill=True, place=("at", PLANT_AT + 4))
    return out


SCENARIOS = _scenarios()
GROUPS = ("T", "L", "D", "DL", "B", "U", "R")
BY_NAME = {(s.group, s.name): s for s in SCENARIOS}
assert len(BY_NAME) == len(SCENARIOS)


def md_regex(md):
    return re.compile(b"".join(b"[^0-9^]" if ch == "?" else re.escape(ch.encode()) for ch in md))


def claim_holds(scn, fields):
    """The scenario's claim against a sam_fields tuple without AIM_SAM_EQX."""
    pos, span, nm, words, md, flags = fields
    if scn.cigar == "*":
        return flags == sam_model.SAM_UNMAPPED and words == [] and md == b""
    return sam_model.cigar_string(words) == scn.cigar and md_regex(scn.md).fullmatch(md) is not None


def rows_of(groups, fillers=True, kinds=True):
    """The rows of the groups: every scenario on both strands at every begin_offset mod 4 with the '?' filler, alternating between the
    row's two ends so that on strand 1 begin_offset 0, 1, 2 and 3 themselves occur; the scenarios marked `fill` once more with each
    other filler, strand, shift and end rotating; and for U the unmapped kinds between mapped rows."""
    rows = []
    scns = [s for s in SCENARIOS if s.group in groups and s.group != "DL"]
    for i, s in enumerate(scns):
        for strand in (0, 1):
            for shift in range(4):
                rows.append(Row(s, strand, shift, "lo" if (i + shift + strand) & 1 else "hi", FILLERS[0], "ok"))
    if fillers:
        turn = 0
        for s in scns:
            if s.fill:
                for f in FILLERS[1:]:
                    rows.append(Row(s, turn & 1, (turn >> 1) & 3, "lo" if (turn >> 3) & 1 else "hi", f, "ok"))
                    turn += 1
                turn += 1        # (four fillers per scenario: one more step keeps the strands from pairing up with the fillers)
    if kinds and "U" in groups:
        mapped = BY_NAME["U", "mapped"]
        extra = [Row(mapped, t & 1, t & 3, "hi" if t & 4 else "lo", FILLERS[(t >> 1) % len(FILLERS)], kind)
                 for t, kind in enumerate(("empty", "inverted", "status", "overcap") * 4)]
        # between mapped rows: one unmapped kind after every third row
        mixed, it = [], iter(extra)
        for j, r in enumerate(rows):
            mixed.append(r)
            if j % 3 == 2:
                mixed.extend([x for x in [next(it, None)] if x is not None])
        rows = mixed + list(it)
    return rows


def long_rows():
    """The DL scenarios (READ_SIZE 65528): a handful of rows -- each on both strands, shift, end and filler rotating."""
    scns = [s for s in SCENARIOS if s.group == "DL"]
    return [Row(s, strand, (i + 2 * strand + 1) & 3, "lo" if (i + strand) & 1 else "hi", FILLERS[(2 * i + strand) % len(FILLERS)], "ok")
            for i, s in enumerate(scns) for strand in (0, 1)]


def rotate(rows, by):
    by %= max(len(rows), 1)
    return rows[by:] + rows[:by]


def ref_consumed(walk):
    return sum(walk.count(c) for c in (b"M", b"X", b"I"))


def lay(rows, rs, ref):
    """Rows -> dict(res, ops, tpos, rows): RESULT[n], uint8[n][2 rs], uint64[n]."""
    n, width = len(rows), 2 * rs
    res = np.zeros(n, dtype=RESULT)
    ops = np.zeros((n, width), dtype=np.uint8)
    tpos = np.zeros(n, dtype=np.uint64)
    for i, r in enumerate(rows):
        s = r.scn
        w = s.walk[::-1] if r.strand else s.walk
        ln = len(w)
        assert ln + 8 <= width, (s.name, rs)
        b = r.shift if r.end == "lo" else ((width - ln) & ~3) - 4 + r.shift
        assert b >= 0 and b % 4 == r.shift and b + ln <= width
        ops[i] = r.filler
        ops[i, b:b + ln] = np.frombuffer(w, dtype=np.uint8)
        e, score, status = b + ln, i % 7, 0
        if r.kind == "empty":
            e = b
        elif r.kind == "inverted":
            b, e = e, b
        elif r.kind == "status":
            status = 1 + i % 3
        elif r.kind == "overcap":
            score = MAX_SCORE + 1
        res[i] = (ln, b, e, score, status, 1000 + i)
        need = ref_consumed(s.walk)
        if s.place is None:
            ws = (100 + 37 * i) % (len(ref) - need)
        elif s.place == "end":
            ws = len(ref) - need
        else:
            ws = s.place[1]
        assert ws + need <= len(ref)
        tpos[i] = ws | (r.strand << 63)
    return dict(res=res, ops=ops, tpos=tpos, rows=rows, rs=rs)


def expected(batch, ref, eqx, sel=None):
    """sam_model over the batch's rows; sel[r] names row r's text_pos entry (UINT32_MAX: none)."""
    res, ops, tpos = batch["res"], batch["ops"], batch["tpos"]
    out = []
    for i in range(len(res)):
        c = i if sel is None else int(sel[i])
        out.append(sam_model.row_fields(res[i], ops[i], None if c == UINT32_MAX else tpos[c], ref, True, MAX_SCORE, eqx))
    return out


def need(exp):
    return sum(len(e[3]) for e in exp), sum(len(e[4]) for e in exp)


def build_read(walk, ref_slice):
    """A read (in walk = forward-reference orientation) that is consistent with the walk and the reference bases it consumes:
    matches copy the reference, a mismatch takes another byte, an insertion or clip base is 'A'."""
    out, rp = bytearray(), 0
    for c in walk:
        c = bytes([c])
        if c == b"M":
            out.append(ref_slice[rp])
            rp += 1
        elif c == b"X":
            out.append(ord("C") if ref_slice[rp] in b"Aa" else ord("A"))
            rp += 1
        elif c == b"I":
            rp += 1
        else:
            out.append(ord("A"))
    return bytes(out)
