"""The DECOMPOSITION of the two record kernels of sam_fields.hpp in plain Python / numpy -- not the rule (that is sam_model.py): how each
mapping cuts a row up, and what it carries from piece to piece.

  lane  one row per lane: the two ends are peeled byte by byte, then the core is walked over row words, a whole word of 'M' that the
        walk meets at its first byte (in walk order) taken four ops at a time; once to count and once to write.
  wave  one row per wavefront: a search for the first and the last M / X, then a count sweep and a write sweep over tiles of 256 ops,
        64 lanes x 4 walk positions (sam_walk4: two word loads, a byte alignment, a byte reversal on strand 1, a mask past the end).
        Three counts per lane travel through one exclusive scan as 10-bit fields of one word; two running maxima place the open
        run's start and the last MD event; seven values carry from tile to tile: prev_q, mp_c, rp_c, nb_c, md_c, start_c, base_c.
        The lanes are numpy vectors of 64; the scans are cumulative sums and maxima over them.

`mutate` names exactly one thing to break (MUTANTS). tests/test_directed_ops_cpu.py shows that the directed rows of directed_ops.py
tell every mutant from the model, which is the evidence that those rows would catch a kernel that is wrong in the same way.
Both functions return the tuple of sam_model.sam_fields."""
import numpy as np

WAVE, TILE = 64, 256
SAM_REVERSE, SAM_UNMAPPED = 0x10, 0x4
SENTINEL_WORD, SENTINEL_BYTE = 0x7E7E7E7E, 0x7E

CARRIES = ("prev_q", "mp_c", "rp_c", "nb_c", "md_c", "start_c", "base_c")
WAVE_MUTANTS = tuple("drop_" + c for c in CARRIES) + ("pcls_lane0_class3", "fields_8_bits", "bnd_at_first", "no_trailing_loop", "no_valid_mask",
                                                      "rev_off_by_one", "no_w0_guard")
LANE_MUTANTS = ("fast_past_core", "fast_align_strand0")
BOTH_MUTANTS = ("ndig_le",)
MUTANTS = WAVE_MUTANTS + LANE_MUTANTS + BOTH_MUTANTS
# What the output cannot show: every consumer of sam_walk4 tests k + j < n itself, so the bytes the mask clears are never looked at,
# and a word below the row that the guard skips holds only such bytes. The guard keeps the LOAD inside the row, which is its purpose.
OUTPUT_EQUIVALENT = ("no_valid_mask", "no_w0_guard")

_POW10 = [10 ** i for i in range(1, 10)]


def ndig(x, mutate=None):
    x = int(x) & 0xFFFFFFFF
    if mutate == "ndig_le":
        return 1 + sum(1 for p in _POW10 if x > p)
    return 1 + sum(1 for p in _POW10 if x >= p)


def put_dec(dst, at, x, nd):
    x = int(x) & 0xFFFFFFFF
    for i in range(nd - 1, -1, -1):
        dst[at + i] = 0x30 + x % 10
        x //= 10


def sam_class(op):
    return 0 if op == 0x4D else 1 if op == 0x58 else 2 if op == 0x49 else 3


def bam_op(cls, eqx):
    return (7 if eqx else 0) if cls == 0 else (8 if eqx else 0) if cls == 1 else 2 if cls == 2 else 1


def ref_byte(ref, pos):
    if not len(ref):
        return ord("N")
    return int(ref[pos if pos < len(ref) else len(ref) - 1])


def _gather(store, count, sentinel):
    """What a buffer of `count` cells holds after the writes in `store`; a write outside it stays visible as extra cells."""
    top = max([count] + [k + 1 for k in store if k >= 0])
    out = [store.get(i, sentinel) for i in range(top)]
    return out + ([sentinel] if any(k < 0 for k in store) else [])


def _row(res_row, read_size, text_pos, algo_is_wfa, max_score):
    """sam_row: the clamped range, the strand, whether there is anything to walk."""
    if text_pos is None:
        return 0, False, 0, 0, False
    ws, rev = int(text_pos) & ((1 << 63) - 1), bool(int(text_pos) >> 63)
    b, e = max(int(res_row["begin_offset"]), 0), min(int(res_row["end_offset"]), 2 * read_size)
    over = algo_is_wfa and int(res_row["score"]) == max_score + 1
    return ws, rev, b, e, int(res_row["status"]) == 0 and e > b and not over


# ---- one row per lane ---------------------------------------------------------------------------------------------------------------
def _lane_core(write, rowp, b, e, rev, k0, k1, lead_clip, trail_clip, ws, lead_ref, ref, eqx, mutate, cg, md):
    nc = nmd = nm = span = cnt = 0
    run_op, run_len, prev_cls = 0xFF, 0, 0
    cw, word = -1, 0
    if lead_clip:
        if write:
            cg[nc] = (lead_clip << 4) | 4
        nc += 1
    k = k0
    while k < k1:
        i = e - 1 - k if rev else b + k
        if (i >> 2) != cw:
            cw = i >> 2
            word = int(rowp[cw])
        inside = True if mutate == "fast_past_core" else k + 4 <= k1
        first_byte = 0 if mutate == "fast_align_strand0" else (3 if rev else 0)
        whole = inside and (i & 3) == first_byte and word == 0x4D4D4D4D
        cls = 0 if whole else sam_class((word >> (8 * (i & 3))) & 0xFF)
        step = 4 if whole else 1
        bop = bam_op(cls, eqx)
        if bop != run_op:
            if run_len:
                if write:
                    cg[nc] = (run_len << 4) | run_op
                nc += 1
            run_op, run_len = bop, 0
        run_len += step
        if cls == 0:
            cnt += step
            span += step
        elif cls == 1:
            nd = ndig(cnt, mutate)
            if write:
                put_dec(md, nmd, cnt, nd)
                md[nmd + nd] = ref_byte(ref, ws + lead_ref + span)
            nmd += nd + 1
            cnt, span, nm = 0, span + 1, nm + 1
        elif cls == 2:
            if prev_cls != 2:
                nd = ndig(cnt, mutate)
                if write:
                    put_dec(md, nmd, cnt, nd)
                    md[nmd + nd] = ord("^")
                nmd += nd + 1
                cnt = 0
            if write:
                md[nmd] = ref_byte(ref, ws + lead_ref + span)
            nmd, span, nm = nmd + 1, span + 1, nm + 1
        else:
            nm += 1
        prev_cls = cls
        k += step
    if run_len:
        if write:
            cg[nc] = (run_len << 4) | run_op
        nc += 1
    if trail_clip:
        if write:
            cg[nc] = (trail_clip << 4) | 4
        nc += 1
    nd = ndig(cnt, mutate)
    if write:
        put_dec(md, nmd, cnt, nd)
    nmd += nd
    return nc, nmd, nm, span


def lane_fields(res_row, ops_row, text_pos, reference, algo_is_wfa, max_score, eqx=False, mutate=None):
    """sam_lane_wave for one row."""
    row = np.ascontiguousarray(ops_row, dtype=np.uint8)
    rowp = row.view("<u4")
    ws, rev, b, e, walk = _row(res_row, len(row) // 2, text_pos, algo_is_wfa, max_score)
    n = e - b if walk else 0

    def op_at(k):
        return int(row[e - 1 - k if rev else b + k])

    k0, k1, lead_ref, trail_ref = 0, n, 0, 0
    while k0 < n:
        cls = sam_class(op_at(k0))
        if cls < 2:
            break
        lead_ref += cls == 2
        k0 += 1
    while k1 > k0:
        cls = sam_class(op_at(k1 - 1))
        if cls < 2:
            break
        trail_ref += cls == 2
        k1 -= 1
    if k1 <= k0:
        return ws, 0, 0, [], b"", SAM_UNMAPPED
    lead_clip, trail_clip = k0 - lead_ref, (n - k1) - trail_ref
    args = (rowp, b, e, rev, k0, k1, lead_clip, trail_clip, ws, lead_ref, reference, eqx, mutate)
    nc, nmd, nm, span = _lane_core(False, *args, None, None)
    cg, md = {}, {}
    _lane_core(True, *args, cg, md)
    return ws + lead_ref, span, nm, _gather(cg, nc, SENTINEL_WORD), bytes(_gather(md, nmd, SENTINEL_BYTE)), SAM_REVERSE if rev else 0


# ---- one row per wavefront ----------------------------------------------------------------------------------------------------------
LANES = np.arange(WAVE, dtype=np.int64)


_CLS = np.array([sam_class(op) for op in range(256)], dtype=np.int64)
_BOP = {eqx: np.array([bam_op(c, eqx) for c in range(4)], dtype=np.int64) for eqx in (False, True)}


def _cls(op):
    return _CLS[op]


def _bop(cls, eqx):
    return _BOP[bool(eqx)][cls]


def _ndig(x, mutate):
    x = x & 0xFFFFFFFF
    nd = np.ones(len(x), dtype=np.int64)
    for p in _POW10:
        nd += (x > p) if mutate == "ndig_le" else (x >= p)
    return nd


def walk4(rowp, b, e, rev, n, k, mutate=None, filler=0):
    """sam_walk4 for the 64 lanes at once: the four ops at walk positions k .. k + 3, byte j = position k + j, as one word per lane."""
    valid = n - k
    o = (e - k - (3 if mutate == "rev_off_by_one" else 4)) if rev else b + k
    w0, sh = o >> 2, (o & 3).astype(np.uint64)

    def load(w, wanted, guarded):
        inside = (4 * w < e) & (w < len(rowp))
        ok = wanted & inside & (w >= 0)
        v = np.where(ok, rowp[np.clip(w, 0, len(rowp) - 1)], 0).astype(np.uint64)
        if not guarded:      # the load below the row, modelled as reading what lies in front of it: the filler
            v = np.where(wanted & inside & (w < 0), np.uint64(filler * 0x01010101), v)
        return v

    lo = load(w0, np.ones(WAVE, dtype=bool), mutate != "no_w0_guard")
    hi = load(w0 + 1, sh != 0, True)
    q = (((hi << np.uint64(32)) | lo) >> (np.uint64(8) * sh)) & np.uint64(0xFFFFFFFF)
    if rev:
        q = ((q & np.uint64(0xFF)) << np.uint64(24)) | ((q & np.uint64(0xFF00)) << np.uint64(8)) | ((q >> np.uint64(8)) & np.uint64(0xFF00)) | (q >> np.uint64(24))
    if mutate != "no_valid_mask":
        bits = (np.uint64(8) * np.clip(valid, 0, 4).astype(np.uint64))
        q = np.where(valid >= 4, q, q & ((np.uint64(1) << bits) - np.uint64(1)))
    return np.where(valid <= 0, np.uint64(0), q).astype(np.int64)


def _excl_sum32(v):
    """The shuffled scan over one 32-bit word per lane: (exclusive sums, total), modulo 2^32 like the registers."""
    incl = np.cumsum(v.astype(np.uint64)) & np.uint64(0xFFFFFFFF)
    return (incl - v.astype(np.uint64)) & np.uint64(0xFFFFFFFF), int(incl[-1])


def _excl_max(v):
    incl = np.maximum.accumulate(v)
    return np.concatenate([[-1], incl[:-1]]), int(incl[-1])


def _sweep(write, rowp, b, e, rev, n, first, last, lead_clip, trail_clip, ws, ref, eqx, mutate, filler, cg, md):
    W = 8 if mutate == "fields_8_bits" else 10
    MASK = (1 << W) - 1
    init = dict(prev_q=0, mp_c=0, rp_c=0, nb_c=0, md_c=0, start_c=first, base_c=0)
    c = dict(init)
    dropped = mutate[5:] if mutate and mutate.startswith("drop_") else None
    my_nm, my_lead, my_trail, my_md, my_span = (np.zeros(WAVE, dtype=np.int64) for _ in range(5))
    lead_s = 1 if lead_clip else 0
    for t0 in range(0, last + 1, TILE):
        if dropped and t0:
            c[dropped] = init[dropped]
        k = t0 + 4 * LANES
        q = walk4(rowp, b, e, rev, n, k, mutate, filler)
        up = np.concatenate([[c["prev_q"]], q[:-1]])
        pcls = _cls((up >> 24) & 0xFF)
        if mutate == "pcls_lane0_class3":
            pcls[0] = 3
        cls, core, bnd = [], [], []
        nM, nR, nB = (np.zeros(WAVE, dtype=np.int64) for _ in range(3))
        my_start = np.full(WAVE, -1, dtype=np.int64)
        for j in range(4):
            kk = k + j
            cj = np.where(kk < n, _cls((q >> (8 * j)) & 0xFF), 3)
            co = (kk >= first) & (kk <= last)
            cls.append(cj)
            core.append(co)
            nM += co & (cj == 0)
            nR += (kk < n) & (cj < 3)
            before = cls[j - 1] if j else pcls
            after_first = (kk >= first) if mutate == "bnd_at_first" else (kk > first)
            bj = after_first & (kk <= last) & (_bop(cj, eqx) != _bop(before, eqx))
            bnd.append(bj)
            nB += bj
            my_start = np.where(bj, kk, my_start)
            if not write:
                my_nm += co & (cj != 0)
                my_span += co & (cj != 3)
                my_lead += (kk < first) & (cj == 3)
                my_trail += (kk > last) & (kk < n) & (cj == 3)
        ex, tot = _excl_sum32(nM | (nR << W) | (nB << (2 * W)))
        ex = ex.astype(np.int64)
        mp = c["mp_c"] + (ex & MASK)
        rp0 = c["rp_c"] + ((ex >> W) & MASK)
        # the M count at this lane's last mismatch / deleted base
        my_base = np.full(WAVE, -1, dtype=np.int64)
        m = mp.copy()
        for j in range(4):
            m = m + (core[j] & (cls[j] == 0))
            my_base = np.where(core[j] & ((cls[j] == 1) | (cls[j] == 2)), m, my_base)
        ex_base, top_base = _excl_max(my_base)
        base = np.maximum(c["base_c"], ex_base)
        # MD bytes of this lane's ops
        nbytes = np.zeros(WAVE, dtype=np.int64)
        nd, cnt = [], []
        m, bs, before = mp.copy(), base.copy(), pcls
        for j in range(4):
            m = m + (core[j] & (cls[j] == 0))
            ev = core[j] & ((cls[j] == 1) | ((cls[j] == 2) & (before != 2)))
            cj = np.where(ev, (m - bs) & 0xFFFFFFFF, 0)
            dj = np.where(ev, _ndig(cj, mutate), 0) if ev.any() else cj      # (no lane has a count to print: all zero)
            cnt.append(cj)
            nd.append(dj)
            nbytes += np.where(ev, dj + 1, 0) + (core[j] & (cls[j] == 2))
            bs = np.where(core[j] & ((cls[j] == 1) | (cls[j] == 2)), m, bs)
            before = cls[j]
        if not write:
            my_md += nbytes
        else:
            ex_md, tot_md = _excl_sum32(nbytes)
            ex_start, top_start = _excl_max(my_start)
            cur_v = np.maximum(c["start_c"], ex_start)
            at_v = lead_s + c["nb_c"] + ((ex >> (2 * W)) & MASK)
            for ln in np.nonzero((nB > 0) | (nbytes > 0))[0]:       # (a lane without a boundary and without MD bytes stores nothing)
                cur, at, mo, rp, bef = int(cur_v[ln]), int(at_v[ln]), c["md_c"] + int(ex_md[ln]), int(rp0[ln]), int(pcls[ln])
                for j in range(4):
                    kk, cj, co = int(k[ln]) + j, int(cls[j][ln]), bool(core[j][ln])
                    if bnd[j][ln]:
                        cg[at] = (((kk - cur) & 0xFFFFFFF) << 4) | bam_op(bef, eqx)
                        at, cur = at + 1, kk
                    if co and cj == 1:
                        d = int(nd[j][ln])
                        put_dec(md, mo, cnt[j][ln], d)
                        md[mo + d] = ref_byte(ref, ws + rp)
                        mo += d + 1
                    elif co and cj == 2:
                        if bef != 2:
                            d = int(nd[j][ln])
                            put_dec(md, mo, cnt[j][ln], d)
                            md[mo + d] = ord("^")
                            mo += d + 1
                        md[mo] = ref_byte(ref, ws + rp)
                        mo += 1
                    rp += kk < n and cj < 3
                    bef = cj
            c["md_c"] += tot_md
            c["start_c"] = max(c["start_c"], top_start)
        c["mp_c"] += tot & MASK
        c["rp_c"] += (tot >> W) & MASK
        c["nb_c"] += (tot >> (2 * W)) & MASK
        c["base_c"] = max(c["base_c"], top_base)
        c["prev_q"] = int(q[WAVE - 1])
    tail = (c["mp_c"] - c["base_c"]) & 0xFFFFFFFF
    if not write:
        t_lead = int(my_lead.sum())
        # the ops behind the last tile of the core (a long trailing peel) are counted here
        if mutate != "no_trailing_loop":
            for t0 in range(((last >> 8) + 1) << 8, n, TILE):
                k = t0 + 4 * LANES
                q = walk4(rowp, b, e, rev, n, k, mutate, filler)
                for j in range(4):
                    my_trail += (k + j < n) & (_cls((q >> (8 * j)) & 0xFF) == 3)
        t_trail = int(my_trail.sum())
        n_cigar = c["nb_c"] + 1 + (1 if t_lead else 0) + (1 if t_trail else 0)
        return dict(lead_clip=t_lead, trail_clip=t_trail, n_cigar=n_cigar, md_len=int(my_md.sum()) + ndig(tail, mutate), nm=int(my_nm.sum()),
                    ref_span=int(my_span.sum()), lead_ref=first - t_lead)
    if lead_clip:
        cg[0] = (lead_clip << 4) | 4
    il = e - 1 - last if rev else b + last
    last_cls = sam_class((int(rowp[il >> 2]) >> (8 * (il & 3))) & 0xFF)
    at = lead_s + c["nb_c"]
    cg[at] = (((last + 1 - c["start_c"]) & 0xFFFFFFF) << 4) | bam_op(last_cls, eqx)
    if trail_clip:
        cg[at + 1] = (trail_clip << 4) | 4
    put_dec(md, c["md_c"], tail, ndig(tail, mutate))
    return None


def wave_fields(res_row, ops_row, text_pos, reference, algo_is_wfa, max_score, eqx=False, mutate=None, filler=0):
    """sam_wave_kernel for one row. `filler` is the byte the no_w0_guard mutant finds in front of the row."""
    row = np.ascontiguousarray(ops_row, dtype=np.uint8)
    rowp = row.view("<u4")
    ws, rev, b, e, walk = _row(res_row, len(row) // 2, text_pos, algo_is_wfa, max_score)
    n = e - b if walk else 0
    # the first and the last M / X of the walk
    fmin, lneg = np.full(WAVE, 0x7FFFFFFF, dtype=np.int64), np.full(WAVE, 0x7FFFFFFF, dtype=np.int64)
    for t0 in range(0, n, TILE):
        k = t0 + 4 * LANES
        q = walk4(rowp, b, e, rev, n, k, mutate, filler)
        for j in range(4):
            hit = (k + j < n) & (_cls((q >> (8 * j)) & 0xFF) < 2)
            fmin = np.where(hit, np.minimum(fmin, k + j), fmin)
            lneg = np.where(hit, np.minimum(lneg, -(k + j)), lneg)
    first, last = int(fmin.min()), -int(lneg.min())
    if first == 0x7FFFFFFF:
        return ws, 0, 0, [], b"", SAM_UNMAPPED
    args = (rowp, b, e, rev, n, first, last)
    c = _sweep(False, *args, 0, 0, ws, reference, eqx, mutate, filler, None, None)
    cg, md = {}, {}
    _sweep(True, *args, c["lead_clip"], c["trail_clip"], ws, reference, eqx, mutate, filler, cg, md)
    return (ws + c["lead_ref"], c["ref_span"], c["nm"], _gather(cg, c["n_cigar"], SENTINEL_WORD), bytes(b & 0xFF for b in _gather(md, c["md_len"], SENTINEL_BYTE)),
            SAM_REVERSE if rev else 0)


def fields(mapping, *args, **kw):
    if mapping == "lane":
        kw.pop("filler", None)
        return lane_fields(*args, **kw)
    return wave_fields(*args, **kw)
