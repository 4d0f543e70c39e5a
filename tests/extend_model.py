"""Segment extension (include/aim_hip.h, AIM_FEATURE_EXTEND) in plain numpy, written from the text of rule 11c: the banded gap-affine
cost D over prefix pairs, the stop level, the result cell and its ties (part 1), and the rewrite of the touched slots (part 2). It is a
dynamic program over rows, not a wavefront algorithm, and shares no code with the library. Below the rule: the directed batch the GPU
tests run, hand-made segment records over a random reference."""
from collections import namedtuple

import numpy as np

import seed_model as m
import split_model as sm

EXTEND = np.dtype([("dq", "<u2", (2,)), ("dr", "<u2", (2,)), ("stop", "<u2", (2,)), ("pad", "<u2", (2,)), ("score", "<i4", (2,))])
EXT_LEFT, EXT_RIGHT = 0x20, 0x40
MAX_UNIT, MAX_BAND, MAX_COST, MAX_EXT = 64, 31, 4095, 1024
INF = 1 << 28

Params = namedtuple("Params", "match mismatch gap_o gap_e xdrop max_cost band max_ext")

COMP = np.arange(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTacgt", b"TGCAtgca"):
    COMP[_a] = _b


def units(p):
    """(x', o', e') of Eizenga and Paten for match bonus a."""
    return 2 * (p.match + p.mismatch), 2 * p.gap_o, 2 * p.gap_e + p.match


def check_params(p):
    x2, o2, e2 = units(p)
    assert p.match >= 1 and p.mismatch >= 1 and p.gap_o >= 0 and p.gap_e >= 1 and p.xdrop >= 0
    assert 1 <= p.max_cost <= MAX_COST and 1 <= p.band <= MAX_BAND and 8 <= p.max_ext <= MAX_EXT and max(x2, o2 + e2) <= MAX_UNIT


# ---- rule 11c, part 1 ------------------------------------------------------------------------------------------------------------
def band_costs(p, Q, T, n, m_len):
    """D over the band for a batch of sides. Q uint8[S][maxn], T uint8[S][maxm], n and m_len int[S]. Returns int32[S][maxn + 1][W]:
    entry [s][v][j] is D(v, h) with h = v + j - band, INF outside the side's matrix."""
    x2, o2, e2 = units(p)
    oe = o2 + e2
    S, b = len(n), p.band
    W = 2 * b + 1
    maxn = int(n.max())
    k = np.arange(W) - b
    Tp = np.zeros((S, maxn + W + b + 1), dtype=np.uint8)            # b bytes of padding in front: Tp[:, b + h] = T[:, h]
    w = min(T.shape[1], Tp.shape[1] - b)
    Tp[:, b:b + w] = T[:, :w]
    out = np.full((S, maxn + 1, W), INF, dtype=np.int32)
    step = (np.arange(W) * e2).astype(np.int32)
    prevM = prevD = None
    for v in range(maxn + 1):
        h = v + k
        inside = (h[None, :] >= 0) & (h[None, :] <= m_len[:, None]) & (v <= n)[:, None]
        if v == 0:
            X = np.full((S, W), INF, dtype=np.int32)
            X[:, b] = 0
            Dn = np.full((S, W), INF, dtype=np.int32)
        else:
            sub = np.where(Q[:, v - 1][:, None] == Tp[:, v - 1:v - 1 + W], 0, x2).astype(np.int32)    # t[h - 1] sits at Tp[b + h - 1]
            diag = np.where(h[None, :] >= 1, prevM + sub, INF)
            Dn = np.full((S, W), INF, dtype=np.int32)
            Dn[:, :-1] = np.minimum(prevM[:, 1:] + oe, prevD[:, 1:] + e2)
            Dn = np.where(inside, np.minimum(Dn, INF), INF)
            X = np.minimum(diag, Dn)
        X = np.where(inside, np.minimum(X, INF), INF)
        # a run of text-consuming gap bases inside the row: I(j) = min over i < j of X(i) + o' + (j - i) e'
        P = np.minimum.accumulate(X - step[None, :], axis=1)
        I = np.full((S, W), INF, dtype=np.int32)
        I[:, 1:] = P[:, :-1] + o2 + step[None, 1:]
        M = np.where(inside, np.minimum(np.minimum(X, I), INF), INF)
        out[:, v] = M
        prevM, prevD = M, Dn
    return out


def pick(p, D, b):
    """The stop level and the result cell from one side's D (int32[n + 1][W]): (dq, dr, score, stop)."""
    a, Z, cap = p.match, p.xdrop, p.max_cost
    v, j = np.nonzero(D <= cap)
    d = D[v, j].astype(np.int64)
    anti = 2 * v + (j - b)                                           # v + h
    top = np.full(cap + 1, -1, dtype=np.int64)                       # the greatest v + h among the cells of exactly this cost
    np.maximum.at(top, d, anti)
    s = np.arange(cap + 1)
    R = np.maximum.accumulate(top)
    B = np.maximum.accumulate(np.where(top >= 0, a * top - s, -INF))
    fire = a * R - s < B - 2 * Z
    stop = int(np.argmax(fire)) if fire.any() else cap
    keep = d <= stop
    val = a * anti[keep] - d[keep]
    if val.max() <= 0:
        return 0, 0, 0, stop
    order = np.lexsort((j[keep], d[keep], -val))                    # greatest value, then smallest D, then smallest h - v
    i = order[0]
    vv, hh = int(v[keep][i]), int(v[keep][i] + j[keep][i] - b)
    assert int(val[i]) % 2 == 0
    return vv, hh, int(val[i]) // 2, stop


def extend_sides(p, sides):
    """sides: list of (q, t) uint8 arrays with len(q) >= 1 and len(t) >= 1. Returns a list of (dq, dr, score, stop)."""
    check_params(p)
    out = [None] * len(sides)
    order = sorted(range(len(sides)), key=lambda i: len(sides[i][0]))
    pos = 0
    while pos < len(order):
        n0 = len(sides[order[pos]][0])
        chunk = [i for i in order[pos:pos + max(1, (1 << 16) // (n0 + 1))] if len(sides[i][0]) <= 2 * n0 + 8]
        pos += len(chunk)
        n = np.array([len(sides[i][0]) for i in chunk])
        ml = np.array([len(sides[i][1]) for i in chunk])
        Q = np.zeros((len(chunk), int(n.max())), dtype=np.uint8)
        T = np.zeros((len(chunk), int(ml.max())), dtype=np.uint8)
        for c, i in enumerate(chunk):
            Q[c, :n[c]], T[c, :ml[c]] = sides[i]
        D = band_costs(p, Q, T, n, ml)
        for c, i in enumerate(chunk):
            out[i] = pick(p, D[c, :n[c] + 1], p.band)
    return out


def extend_side(p, q, t):
    """One side: (dq, dr, score, stop); zeros when either sequence is empty (the side is not run)."""
    if len(q) == 0 or len(t) == 0:
        return 0, 0, 0, 0
    return extend_sides(p, [(np.asarray(q, dtype=np.uint8), np.asarray(t, dtype=np.uint8))])[0]


# ---- the sides of a batch and rule 11c, part 2 -------------------------------------------------------------------------------------
def side_sequences(p, read_size, ref_len, L, read, ref, seg, text_pos, text_len):
    """The (side, up, q, t) of one slot that rule 11c runs: side 0 is the read's left, 1 its right."""
    fl = int(seg["flags"])
    qb, qe = int(seg["q_begin"]), int(seg["q_end"])
    start, minus = int(text_pos) & (sm.MINUS - 1), int(text_pos) >> 63
    if not fl & sm.VALID or fl & sm.LOOSE or qb > qe or qe > L or not 0 <= text_len <= read_size or start + text_len > ref_len:
        return []
    inner = [side for side, bit in ((0, sm.LEFT_OPEN), (1, sm.RIGHT_OPEN)) if not fl & bit]
    out = []
    for side in inner:
        q = read[qe:min(L, qe + p.max_ext)] if side else read[max(0, qb - p.max_ext):qb][::-1]
        up = bool(side) != bool(minus)
        room = ref_len - (start + text_len) if up else start
        ml = min(len(q) + p.band, room, (read_size - text_len) // len(inner))
        if len(q) == 0 or ml <= 0:
            continue
        t = ref[start + text_len:start + text_len + ml] if up else ref[start - ml:start][::-1]
        out.append((side, up, q, COMP[t] if minus else t))
    return out


def extend_segments(p, K, read_size, ref_len, read_len, reads, ref, seg_req, seg_tp, seg_pat, seg):
    """The whole batch: the four split outputs as aim_extend_segments_device leaves them (copies) and aim_extend_t per slot."""
    o_req, o_tp, o_pat, o_seg = seg_req.copy(), seg_tp.copy(), seg_pat.copy(), seg.copy()
    ext = np.zeros(len(seg), dtype=EXTEND)
    jobs = []
    for slot in range(len(seg)):
        r = slot // K
        L = min(max(int(read_len[r]), 0), read_size)
        for side, up, q, t in side_sequences(p, read_size, ref_len, L, reads[r], ref, seg[slot], seg_tp[slot], int(seg_req["text_len"][slot])):
            jobs.append((slot, side, up, q, t))
    res = extend_sides(p, [(q, t) for _, _, _, q, t in jobs]) if jobs else []
    for (slot, side, up, _, _), (dq, dr, score, stop) in zip(jobs, res):
        ext[slot]["dq"][side], ext[slot]["dr"][side], ext[slot]["stop"][side], ext[slot]["score"][side] = dq, dr, stop, score
    for slot in np.nonzero((ext["dq"] != 0).any(axis=1) | (ext["dr"] != 0).any(axis=1))[0]:
        r, e = slot // K, ext[slot]
        start, minus = int(seg_tp[slot]) & (sm.MINUS - 1), int(seg_tp[slot]) >> 63
        end = start + int(seg_req["text_len"][slot])
        qb, qe = int(seg["q_begin"][slot]) - int(e["dq"][0]), int(seg["q_end"][slot]) + int(e["dq"][1])
        fl = int(seg["flags"][slot])
        for side in (0, 1):
            if int(e["dq"][side]) or int(e["dr"][side]):
                fl |= EXT_RIGHT if side else EXT_LEFT
                if bool(side) != bool(minus):
                    end += int(e["dr"][side])
                else:
                    start -= int(e["dr"][side])
        o_req[slot]["pattern_len"], o_req[slot]["text_len"] = qe - qb, end - start
        o_tp[slot] = np.uint64(start | (minus << 63))
        o_seg[slot]["q_begin"], o_seg[slot]["q_end"], o_seg[slot]["flags"] = qb, qe, fl
        o_pat[slot] = 0
        o_pat[slot, :qe - qb] = reads[r, qb:qe]
    return (o_req, o_tp, o_pat, o_seg), ext


# ---- the directed batch ------------------------------------------------------------------------------------------------------------
DIR_REF_LEN = 1 << 16
PENALTIES = ((1, 3, 4, 1, 20), (1, 31, 0, 1, 40), (2, 6, 4, 2, 10))      # (a, x, o, e, Z): the usual set; x' = 64, a ring of 65 levels; gcd 2
JUNCTIONS = ("clean", "mismatch", "insertion", "deletion", "long_insertion", "long_deletion", "odd_bytes", "q0", "q1", "budget", "edge_low",
             "edge_high", "loose", "open", "invalid", "two_sides")


def directed_reference(seed=5):
    """64 Ki random bases with an 'N' or a lowercase base every few dozen."""
    rng = np.random.default_rng(seed)
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=DIR_REF_LEN)].copy()
    at = rng.integers(0, DIR_REF_LEN, size=DIR_REF_LEN // 40)
    ref[at[::2]] = ord("N")
    ref[at[1::2]] |= 0x20
    return ref


def _edit(rng, kind, t, at):
    """The read's side of a junction: the staged target t with the junction's edit planted near offset `at`."""
    t = t.copy()
    other = lambda c: np.uint8(b"ACGT"[(b"ACGT".find(bytes([c & 0xDF])) + 1) % 4])
    if kind == "mismatch":
        t[at] = other(int(t[at]))
        return t
    if kind in ("insertion", "long_insertion"):                       # the read has bases the reference lacks
        g = 3 if kind == "insertion" else 40
        return np.concatenate([t[:at], np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=g)], t[at:]])
    if kind in ("deletion", "long_deletion"):
        g = 2 if kind == "deletion" else 40
        return np.concatenate([t[:at], t[at + g:]])
    return t


def directed(seed, n_reads, K, read_size, ref=None):
    """Hand-made split outputs for n_reads reads of K slots: dict(read_len, reads, seg_req, seg_tp, seg_pat, seg, kinds). Read r plants
    junction JUNCTIONS[r % 16] on its designed slot (r % K), on strand (r // 16) & 1 and side (r // 32) & 1; the designed slot of
    "two_sides" is closed on both sides. The other slots are empty slots, random open or loose segments, or closed segments over random
    bases. A prefix of a batch is the batch of fewer reads."""
    ref = directed_reference() if ref is None else ref
    ref_len, rs = len(ref), read_size
    read_len = np.zeros(n_reads, dtype=np.int32)
    reads = np.zeros((n_reads, rs), dtype=np.uint8)
    seg_req = np.zeros(n_reads * K, dtype=m.REQUEST)
    seg_tp = np.zeros(n_reads * K, dtype=np.uint64)
    seg_pat = np.zeros((n_reads * K, rs), dtype=np.uint8)
    seg = np.zeros(n_reads * K, dtype=sm.SEGMENT)
    kinds = []
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    for r in range(n_reads):
        rng = np.random.default_rng([seed, K, rs, r])
        kind, minus, side = JUNCTIONS[r % 16], (r // 16) & 1, (r // 32) & 1
        kinds.append(kind)
        L = rs - int(rng.integers(0, 9))
        read_len[r] = L if r % 23 else rs + 7                          # (clamped like rule 10c's)
        L = min(L, rs)
        read = acgt[rng.integers(0, 4, size=rs)].copy()
        body = int(rng.integers(12, 20)) if rs < 512 else int(rng.integers(200, 400))
        # the designed segment: read[qb, qe) against ref[start, start + tl)
        qb = int(rng.integers(rs // 3, rs // 2)) if rs < 512 else int(rng.integers(300, 400))
        qe = qb + body
        if kind == "q0":
            qb, qe = (0, body) if side == 0 else (L - body, L)
        elif kind == "q1":
            qb, qe = (1, body + 1) if side == 0 else (L - body - 1, L - 1)
        tl = body + int(rng.integers(-2, 3))
        if kind == "budget":
            tl = rs - int(rng.integers(0, 4))
        start = int(rng.integers(2 * rs, ref_len - 3 * rs))
        up = bool(side) != bool(minus)
        if kind == "edge_low":
            start = int(rng.integers(0, 6)) if not up else start
            if up:
                start = ref_len - tl - int(rng.integers(0, 6))
        elif kind == "edge_high":
            start = ref_len - tl - int(rng.integers(0, 6)) if up else int(rng.integers(0, 6))
            if r % 3 == 0:
                start = ref_len - tl if up else 0
        flags = sm.VALID | (sm.SUPPLEMENTARY if r % K else 0)
        if kind != "two_sides":
            flags |= sm.RIGHT_OPEN if side == 0 else sm.LEFT_OPEN
        if kind == "loose":
            flags |= sm.LOOSE
        elif kind == "open":
            flags |= sm.LEFT_OPEN | sm.RIGHT_OPEN
        elif kind == "invalid":
            flags = 0 if r % 2 else flags
            if flags:
                qb, qe = qe, qb                                       # a malformed record: q_begin > q_end
        # plant the junction: the bases beyond the inner side(s) continue the reference for a while, with the junction's edit
        for sd in ((0, 1) if kind == "two_sides" else (side,)):
            u = bool(sd) != bool(minus)
            g = int(rng.integers(5, 30)) if rs < 512 else int(rng.integers(20, 120))
            lo, hi = (start + tl, min(start + tl + g + 48, ref_len)) if u else (max(start - g - 48, 0), start)
            t = ref[lo:hi] if u else ref[lo:hi][::-1]
            t = COMP[t] if minus else t
            cont = _edit(rng, kind, t, min(int(rng.integers(2, 12)), max(len(t) - 1, 0)))[:g] if len(t) else t
            if kind == "odd_bytes" and len(cont) > 6:
                cont = cont.copy()
                cont[3], cont[5] = ord("N"), cont[5] | 0x20
            a, b = min(qb, qe), max(qb, qe)
            if sd:
                w = min(len(cont), L - b)
                read[b:b + w] = cont[:w]
            else:
                w = min(len(cont), a)
                read[a - w:a] = cont[:w][::-1]
        reads[r] = read
        for i in range(K):
            slot = r * K + i
            idx = int(rng.integers(0, 1 << 32))
            if i == r % K:
                row = (qb, qe, start, tl, minus, flags)
            else:
                what = int(rng.integers(0, 6))
                if what < 3:
                    row = None
                else:
                    a = int(rng.integers(0, L))
                    b = int(rng.integers(a, L + 1))
                    tl2 = int(rng.integers(0, rs + 1))
                    fl = sm.VALID | sm.SUPPLEMENTARY | (0, sm.LEFT_OPEN | sm.RIGHT_OPEN, sm.LOOSE)[what - 3] | (sm.LEFT_OPEN if rng.integers(0, 2) else 0)
                    row = (a, b, int(rng.integers(0, ref_len - tl2 + 1)), tl2, int(rng.integers(0, 2)), fl)
            if row is None or not row[5]:
                seg_req[slot] = (L, 0, 0, idx)
                seg_pat[slot] = read
                continue
            a, b, st, tl2, mn, fl = row
            seg_req[slot] = (max(b - a, 0), tl2, 0, idx)
            seg_tp[slot] = np.uint64(st | (mn << 63))
            seg_pat[slot, :max(b - a, 0)] = read[a:max(a, b)]
            seg[slot] = (a, b, L, fl, i)
    return dict(read_len=read_len, reads=reads, seg_req=seg_req, seg_tp=seg_tp, seg_pat=seg_pat, seg=seg, kinds=kinds)


def directed_prefix(d, n, K):
    return dict(read_len=d["read_len"][:n], reads=d["reads"][:n], seg_req=d["seg_req"][:n * K], seg_tp=d["seg_tp"][:n * K], seg_pat=d["seg_pat"][:n * K],
                seg=d["seg"][:n * K], kinds=d["kinds"][:n])


def directed_expected(p, d, K, read_size, ref):
    return extend_segments(p, K, read_size, len(ref), d["read_len"], d["reads"], ref, d["seg_req"], d["seg_tp"], d["seg_pat"], d["seg"])


def inner_gaps(seg, halves, K):
    """Per inner side of every valid segment: (slot, side, true cut - segment end), positive while the segment stops short of the cut."""
    out = []
    for slot in np.nonzero(seg["flags"] & sm.VALID)[0]:
        sg = seg[slot]
        hf = sm.half_of(halves[slot // K], int(sg["q_begin"]), int(sg["q_end"]))
        if not int(sg["flags"]) & sm.LEFT_OPEN:
            out.append((int(slot), 0, int(sg["q_begin"]) - hf["q_lo"]))
        if not int(sg["flags"]) & sm.RIGHT_OPEN:
            out.append((int(slot), 1, hf["q_hi"] - int(sg["q_end"])))
    return out
