"""Host-side mirror of the reference's host program over the C-ABI.

Names follow the reference (safaad/aim host.c): a *device set* is what
`struct dpu_set_t` was, `push` are the host->device scatters
(host.c:246-268), `launch` is `dpu_launch(DPU_SYNCHRONOUS)` (host.c:289) and
`pull` the gathers (host.c:316-326).  Pairs are split over the devices of a
set in contiguous blocks exactly like host.c:191-209 splits them over DPUs.
"""
import ctypes as C
import math

import numpy as np

from . import capi
from .capi import (ALGO_BY_NAME, ALGO_NW, ALGO_SWG, ALGO_WFA, FLAG_AFFINE2P, FLAG_BACKTRACE, FLAG_ENDSFREE, FLAG_LINEAR, FLAG_REDUCE,
                   FLAG_MATE_PAIRS, FLAG_READ_GROUPS, FLAG_REF_TEXTS, FLAG_REQ8, FLAG_RES8, FLAG_SWG_W16, FLAG_WFA_BIDIR, FLAG_WFA_ESCALATE, FLAG_WFA_W32, REQUEST8_DTYPE, REQUEST_DTYPE, RESULT8_DTYPE, RESULT_DTYPE, Affine2pParams, EndsFreeParams,
                   Params, params_ref)


def round_up_8(x):
    return ((x + 7) // 8) * 8


def launcher_sizes(algo, read_length, error, mismatch=3, gap_o=4, gap_e=1, gap=4):
    """(MAX_SCORE, READ_SIZE) as the reference launchers derive them."""
    lib = capi.load()
    ms, rs = C.c_int32(), C.c_int32()
    a = ALGO_BY_NAME[algo] if isinstance(algo, str) else algo
    capi.check(lib.aim_launcher_sizes(a, read_length, float(error), mismatch, gap_o, gap_e, gap, C.byref(ms), C.byref(rs)))
    return ms.value, rs.value


def features():
    """aim_features(): capability bits of the loaded library (capi.FEATURE_*)."""
    return int(capi.load().aim_features())


def make_params(algo, max_score, read_size, match=0, mismatch=3, gap_o=4, gap_e=1, gap=4, backtrace=False,
                reduce=False, swg_w16=False, req8=False, res8=False, gap_i=None, gap_d=None, ends_free=None, gap2=None, linear=False,
                w32=False, bidir=False, ref_texts=False, read_groups=False, escalate=False, mate_pairs=False, sam=False, top_hits=False):
    """`gap` is the launchers' single NW gap cost (run-nw-pim-wram.py: -DGAP_I = -DGAP_D); `gap_i` / `gap_d` set the two macros of
    nw.c:67-153 apart (NW/DPU-WRAM/common/common.h GAP_I, GAP_D). `ends_free=(PB, PE, TB, TE)`: ends-free WFA (AIM_FLAG_ENDSFREE);
    returns an EndsFreeParams then, which every call below accepts like Params. `gap2=(O2, E2)`: dual-cost gap-affine WFA
    (AIM_FLAG_AFFINE2P, gap_o / gap_e are piece 1); returns an Affine2pParams. The two cannot be combined. `linear=True`: gap-linear
    WFA (AIM_FLAG_LINEAR): a mismatch costs `mismatch`, every gap base `gap_e`, and gap_o is set to 0; not with ends_free, gap2 or
    reduce. `w32=True`: WFA with 32-bit wavefront offsets (AIM_FLAG_WFA_W32), read_size up to 2^24; combines with all of the above.
    `bidir=True`: bidirectional WFA (AIM_FLAG_WFA_BIDIR), CIGAR in O(MAX_SCORE) scratch; global gap-affine with backtrace only.
    `ref_texts=True`: texts named as windows of the device-resident reference (AIM_FLAG_REF_TEXTS); combines with everything.
    `read_groups=True`: batches of reads and their candidates, best candidate per read (AIM_FLAG_READ_GROUPS); combines with
    everything. `escalate=True`: WFA on a lane kernel at a low cap, the flag-less plan over the pairs that come back over it
    (AIM_FLAG_WFA_ESCALATE); results equal the flag-less ones; global gap-affine WFA without w32, bidir and read_groups.
    `mate_pairs=True`: reads 2m and 2m + 1 of a read-groups batch are mates and the device picks the best consistent pair of
    candidates (AIM_FLAG_MATE_PAIRS); needs read_groups and ref_texts. `sam=True`: SAM-ready records (POS, CIGAR, NM, MD) for every
    row of a submitted batch (AIM_FLAG_SAM_FIELDS); needs ref_texts and backtrace, not with genasm or res8. `top_hits=True`: the
    max_hits best candidates of every read of a read-groups batch, each a full row (AIM_FLAG_TOP_HITS); needs read_groups, not with
    mate_pairs or sam."""
    a = ALGO_BY_NAME[algo] if isinstance(algo, str) else algo
    gap_i = gap if gap_i is None else gap_i
    gap_d = gap if gap_d is None else gap_d
    flags = (FLAG_BACKTRACE if backtrace else 0) | (FLAG_REDUCE if reduce else 0) | (FLAG_SWG_W16 if swg_w16 else 0)
    flags |= (FLAG_REQ8 if req8 else 0) | (FLAG_RES8 if res8 else 0) | (FLAG_WFA_W32 if w32 else 0) | (FLAG_REF_TEXTS if ref_texts else 0)
    flags |= FLAG_READ_GROUPS if read_groups else 0
    if mate_pairs:
        for name, given in (("read_groups", read_groups), ("ref_texts", ref_texts)):
            if not given:
                raise ValueError("mate_pairs needs %s" % name)
        flags |= FLAG_MATE_PAIRS
    if sam:
        for name, given in (("ref_texts", ref_texts), ("backtrace", backtrace)):
            if not given:
                raise ValueError("sam needs %s" % name)
        if a == ALGO_BY_NAME["genasm"] or res8:
            raise ValueError("sam cannot be combined with %s" % ("res8" if res8 else "genasm"))
        flags |= capi.FLAG_SAM_FIELDS
    if top_hits:
        if not read_groups:
            raise ValueError("top_hits needs read_groups")
        for name, given in (("mate_pairs", mate_pairs), ("sam", sam)):
            if given:
                raise ValueError("top_hits cannot be combined with %s" % name)
        flags |= capi.FLAG_TOP_HITS
    if escalate:
        if a != ALGO_WFA:
            raise ValueError("escalate needs wfa")
        for name, given in (("ends_free", ends_free is not None), ("gap2", gap2 is not None), ("linear", linear), ("w32", w32), ("bidir", bidir),
                            ("read_groups", read_groups)):
            if given:
                raise ValueError("escalate cannot be combined with %s" % name)
        flags |= FLAG_WFA_ESCALATE
    if bidir:
        if not backtrace:
            raise ValueError("bidir needs backtrace")
        for name, given in (("reduce", reduce), ("ends_free", ends_free is not None), ("gap2", gap2 is not None), ("linear", linear)):
            if given:
                raise ValueError("bidir cannot be combined with %s" % name)
        flags |= FLAG_WFA_BIDIR
    if ends_free is not None and gap2 is not None:
        raise ValueError("ends_free and gap2 cannot be combined")
    if linear:
        for name, given in (("ends_free", ends_free is not None), ("gap2", gap2 is not None), ("reduce", reduce)):
            if given:
                raise ValueError("linear cannot be combined with %s" % name)
        return Params(a, match, mismatch, 0, gap_e, gap_i, gap_d, max_score, read_size, flags | FLAG_LINEAR)
    if gap2 is not None:
        o2, e2 = (int(x) for x in gap2)
        return Affine2pParams(Params(a, match, mismatch, gap_o, gap_e, gap_i, gap_d, max_score, read_size, flags | FLAG_AFFINE2P), o2, e2)
    if ends_free is not None:
        pb, pe, tb, te = (int(x) for x in ends_free)
        return EndsFreeParams(Params(a, match, mismatch, gap_o, gap_e, gap_i, gap_d, max_score, read_size, flags | FLAG_ENDSFREE),
                              pb, pe, tb, te)
    return Params(a, match, mismatch, gap_o, gap_e, gap_i, gap_d, max_score, read_size, flags)


def params_for(algo, read_length, error, **kw):
    """Params from launcher-style (-l, -e) arguments."""
    cost = {k: kw[k] for k in ("mismatch", "gap_o", "gap_e", "gap") if k in kw}
    ms, rs = launcher_sizes(algo, read_length, error, **cost)
    return make_params(algo, ms, rs, **kw)


def gen_pairs(seed, first_idx, n_pairs, length, error, read_size):
    """Seeded synthetic pairs in the wire layout (requests, patterns[n][rs], texts[n][rs])."""
    lib = capi.load()
    req = np.zeros(n_pairs, dtype=REQUEST_DTYPE)
    pat = np.zeros((n_pairs, read_size), dtype=np.uint8)
    txt = np.zeros((n_pairs, read_size), dtype=np.uint8)
    capi.check(lib.aim_gen_pairs(seed, first_idx, n_pairs, length, float(error), read_size, capi.ptr(req),
                                 capi.ptr(pat), capi.ptr(txt)))
    return req, pat, txt


def mixed_pairs(seed, n_pairs, length, e_clean, e_tail, tail_frac, read_size):
    """Seeded batch of mostly clean pairs with a noisy tail: pair i carries gen_pairs' edits at error e_tail when a hash of (seed, i)
    falls under tail_frac, at e_clean otherwise (both are gen_pairs(seed, 0, n_pairs, ...) rows, so a pair depends on (seed, i) only).
    Returns (requests, patterns, texts, is_tail)."""
    req, pat, txt = gen_pairs(seed, 0, n_pairs, length, e_clean, read_size)
    i = np.arange(n_pairs, dtype=np.uint64)
    h = (i + np.uint64(int(seed) & 0xFFFFFFFF) * np.uint64(0x9E3779B1)) * np.uint64(0x9E3779B97F4A7C15)   # (wraps mod 2^64)
    h ^= h >> np.uint64(29)
    h *= np.uint64(0xBF58476D1CE4E5B9)
    h ^= h >> np.uint64(32)
    tail = (h >> np.uint64(11)).astype(np.float64) * (1.0 / (1 << 53)) < float(tail_frac)
    if tail.any():
        req_t, pat_t, txt_t = gen_pairs(seed, 0, n_pairs, length, e_tail, read_size)
        req[tail], pat[tail], txt[tail] = req_t[tail], pat_t[tail], txt_t[tail]
    return req, pat, txt, tail


def flank_pairs(seed, first_idx, req, pat, txt, flank):
    """Ends-free inputs: `flank` seeded random A/C/G/T bases before and after every text (what a read mapper's reference window
    around a read looks like). Rows widen by 2 * flank (rounded to a multiple of 8); the bases depend on (seed, first_idx)."""
    n, rs = pat.shape
    rs2 = round_up_8(rs + 2 * flank)
    rng = np.random.default_rng([int(seed), int(first_idx), 0x666C616E6B])
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, 2 * flank))]
    req2 = req.copy()
    pat2 = np.zeros((n, rs2), dtype=np.uint8)
    txt2 = np.zeros((n, rs2), dtype=np.uint8)
    pat2[:, :rs] = pat
    for i in range(n):
        tl = int(req["text_len"][i])
        txt2[i, :flank] = bases[i, :flank]
        txt2[i, flank:flank + tl] = txt[i, :tl]
        txt2[i, flank + tl:2 * flank + tl] = bases[i, flank:]
    req2["text_len"] = req["text_len"] + 2 * flank
    return req2, pat2, txt2


def long_indel_pairs(seed, first_idx, req, pat, txt, long_indel):
    """Inputs for dual-cost gap-affine alignment: one seeded insertion or deletion of length in [L/2, L] (L = `long_indel`) put into
    every text at a seeded position, after the usual edits (the structural-variant-sized indel a long read carries). Rows widen by L
    (rounded to a multiple of 8); a deletion never empties a text. Each pair's indel depends on (seed, its pair index) only, like
    gen_pairs' edits, so any slice of a data set -- a text file's chunks or a packed file's batches -- carries the same indels."""
    n, rs = pat.shape
    L = int(long_indel)
    rs2 = round_up_8(rs + L)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    req2 = req.copy()
    pat2 = np.zeros((n, rs2), dtype=np.uint8)
    txt2 = np.zeros((n, rs2), dtype=np.uint8)
    pat2[:, :rs] = pat
    for i in range(n):
        rng = np.random.default_rng([int(seed), int(first_idx) + i, 0x6C6F6E67])
        length = int(rng.integers(max(1, L // 2), L + 1))
        is_ins = bool(rng.integers(0, 2))
        where = float(rng.random())
        tl = int(req["text_len"][i])
        t = txt[i, :tl]
        if is_ins:
            at = int(where * (tl + 1))
            row = np.concatenate([t[:at], acgt[rng.integers(0, 4, size=length)], t[at:]])
        else:
            d = min(length, tl - 1)
            at = int(where * (tl - d + 1))
            row = np.concatenate([t[:at], t[at + d:]])
        txt2[i, :len(row)] = row
        req2["text_len"][i] = len(row)
    return req2, pat2, txt2


_COMP = np.arange(256, dtype=np.uint8)
for _a, _b in (b"AT", b"CG", b"at", b"cg"):
    _COMP[_a], _COMP[_b] = _b, _a


def ref_window(reference, pos, length, minus):
    """The text AIM_FLAG_REF_TEXTS names: reference[pos, pos + length), reverse-complemented on the minus strand (A<->T, C<->G,
    a<->t, c<->g; every other byte unchanged). `reference` is a uint8 array."""
    w = np.asarray(reference[pos:pos + length], dtype=np.uint8)
    return _COMP[w[::-1]] if minus else w.copy()


def ref_pairs(seed, first_idx, n_pairs, length, error, reference, read_size, minus_fraction=0.5):
    """Seeded pairs against a reference (AIM_FLAG_REF_TEXTS): each text is a window of `length` bases at a seeded position, on the
    minus strand with probability `minus_fraction`; its pattern is that text after ceil(length * error) seeded edits with gen_pairs'
    model (uniform substitute / delete / insert at a uniform position; a substitution may re-draw the same base). Bytes of the
    window other than A/C/G/T stay in the pattern. Pair i depends only on (seed, first_idx + i) and the reference.
    Returns (requests, patterns[n][read_size], text_pos[n] uint64, texts[n][read_size]) -- the texts are the explicit rows the
    windows name, for comparison."""
    ref = np.frombuffer(reference, dtype=np.uint8) if isinstance(reference, (bytes, bytearray)) else np.asarray(reference, dtype=np.uint8)
    nedits = int(math.ceil(length * error))
    if length > len(ref):
        raise ValueError("reference shorter than a window")
    if length + nedits > read_size:
        raise ValueError("read_size %d too small for length %d + %d edits" % (read_size, length, nedits))
    acgt = b"ACGT"
    req = np.zeros(n_pairs, dtype=REQUEST_DTYPE)
    pat = np.zeros((n_pairs, read_size), dtype=np.uint8)
    txt = np.zeros((n_pairs, read_size), dtype=np.uint8)
    tpos = np.zeros(n_pairs, dtype=np.uint64)
    for i in range(n_pairs):
        rng = np.random.default_rng([int(seed), int(first_idx) + i, 0x726566])
        pos = int(rng.integers(0, len(ref) - length + 1))
        minus = bool(rng.random() < minus_fraction)
        t = ref_window(ref, pos, length, minus)
        p = bytearray(t.tobytes())
        for _ in range(nedits):
            kind, b, r = int(rng.integers(0, 3)), acgt[int(rng.integers(0, 4))], int(rng.integers(0, 1 << 32))
            if kind == 0 and p:
                p[r % len(p)] = b
            elif kind == 1 and p:
                del p[r % len(p)]
            else:
                p.insert(r % (len(p) + 1), b)
        txt[i, :length] = t
        pat[i, :len(p)] = np.frombuffer(bytes(p), dtype=np.uint8)
        req["pattern_len"][i], req["text_len"][i], req["idx"][i] = len(p), length, int(first_idx) + i
        tpos[i] = pos | ((1 << 63) if minus else 0)
    return req, pat, tpos, txt


def group_pairs(seed, first_read, n_reads, k, length, error, reference, read_size, minus_fraction=0.5, sizes=None, shift=8):
    """Seeded reads with candidate windows of `reference` (AIM_FLAG_READ_GROUPS). Read r (depending only on (seed, first_read + r) and
    the reference) is a window of `length` bases at a seeded position and strand (minus with probability `minus_fraction`) after
    ceil(length * error) edits of ref_pairs' model. Its candidates -- k of them, or sizes[r] -- are windows of `length` bases: the
    true window at a seeded slot; the others each either a copy of it moved by 1..`shift` bases (same strand) or a random window on
    either strand. Every candidate's pattern is the whole read.
    Returns (requests[n_pairs], read_rows[n_reads][read_size], read_offsets[n_reads + 1] uint32, text_pos[n_pairs] uint64,
    texts[n_pairs][read_size], patterns[n_pairs][read_size]) -- texts and patterns are the explicit per-candidate batch."""
    ref = np.frombuffer(reference, dtype=np.uint8) if isinstance(reference, (bytes, bytearray)) else np.asarray(reference, dtype=np.uint8)
    nedits = int(math.ceil(length * error))
    if length > len(ref):
        raise ValueError("reference shorter than a window")
    if length + nedits > read_size:
        raise ValueError("read_size %d too small for length %d + %d edits" % (read_size, length, nedits))
    counts = np.full(n_reads, k, dtype=np.int64) if sizes is None else np.asarray(sizes, dtype=np.int64)
    if len(counts) != n_reads or (counts < 1).any():
        raise ValueError("every read needs at least one candidate")
    offsets = np.zeros(n_reads + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum(counts)
    n = int(offsets[-1])
    acgt = b"ACGT"
    span = len(ref) - length + 1
    req = np.zeros(n, dtype=REQUEST_DTYPE)
    rows = np.zeros((n_reads, read_size), dtype=np.uint8)
    tpos = np.zeros(n, dtype=np.uint64)
    txt = np.zeros((n, read_size), dtype=np.uint8)
    for r in range(n_reads):
        rng = np.random.default_rng([int(seed), int(first_read) + r, 0x67727073])
        pos = int(rng.integers(0, span))
        minus = bool(rng.random() < minus_fraction)
        p = bytearray(ref_window(ref, pos, length, minus).tobytes())
        for _ in range(nedits):
            kind, b, x = int(rng.integers(0, 3)), acgt[int(rng.integers(0, 4))], int(rng.integers(0, 1 << 32))
            if kind == 0 and p:
                p[x % len(p)] = b
            elif kind == 1 and p:
                del p[x % len(p)]
            else:
                p.insert(x % (len(p) + 1), b)
        rows[r, :len(p)] = np.frombuffer(bytes(p), dtype=np.uint8)
        lo, cnt = int(offsets[r]), int(counts[r])
        true_at = int(rng.integers(0, cnt))
        for j in range(cnt):
            if j == true_at:
                cp, cm = pos, minus
            elif rng.random() < 0.5:
                cp, cm = min(max(pos + int(rng.choice([-1, 1])) * int(rng.integers(1, shift + 1)), 0), span - 1), minus
            else:
                cp, cm = int(rng.integers(0, span)), bool(rng.random() < 0.5)
            tpos[lo + j] = cp | ((1 << 63) if cm else 0)
            txt[lo + j, :length] = ref_window(ref, cp, length, cm)
        req["pattern_len"][lo:lo + cnt], req["text_len"][lo:lo + cnt] = len(p), length
    req["idx"] = np.arange(n, dtype=np.uint32)
    read_of = np.repeat(np.arange(n_reads), counts)
    return req, rows, offsets, tpos, txt, np.ascontiguousarray(rows[read_of])


MATE_TRUTH_DTYPE = np.dtype([("true", "<u4", (2,)), ("kind", "<u4")])   # mate_pairs: the true candidates of reads 2m / 2m + 1; kind below
MATE_UNIQUE, MATE_REPEAT, MATE_DISCORDANT = 0, 1, 2


def mate_pairs(seed, n_read_pairs, length, error, insert, k, repeat_frac, read_size=None, discordant_frac=0.05, shift=8):
    """Seeded paired-end reads with candidate windows (AIM_FLAG_MATE_PAIRS). The reference is built here: read pair m owns a region
    of random A/C/G/T that holds its fragment of insert +- insert // 10 bases, and a zone of planted exact repeats follows the
    regions. The mates are the fragment's two ends in FR orientation: one read is the first `length` bases on the plus strand, the
    other the last `length` bases on the minus strand (which of them is read 2m is seeded), each after ceil(length * error) edits
    of ref_pairs' model. With probability `repeat_frac` one mate's window is copied verbatim into the repeat zone and the copy is a
    candidate of that read: it scores exactly like the true window, and only the other mate tells the two apart. With probability
    `discordant_frac` the second read is taken from the plus strand too, so the pair has no proper combination at its true windows.
    Every read has k candidates of `length` bases in seeded order: the true window, the repeat copy if there is one, and decoys --
    each a copy of the true window moved by 1..`shift` bases (same strand) or a random window on either strand. Read pair m depends
    only on (seed, m) and n_read_pairs (the repeat zone's place).
    Returns (reference uint8[], requests[n_pairs], read_rows[2 * n_read_pairs][read_size], read_offsets uint32, text_pos uint64[n_pairs],
    texts[n_pairs][read_size], patterns[n_pairs][read_size], truth[n_read_pairs] of MATE_TRUTH_DTYPE)."""
    nedits = int(math.ceil(length * error))
    read_size = round_up_8(length + nedits) if read_size is None else int(read_size)
    jitter = insert // 10
    if insert - jitter < length:
        raise ValueError("insert %d too small for reads of %d bases" % (insert, length))
    if length + nedits > read_size:
        raise ValueError("read_size %d too small for length %d + %d edits" % (read_size, length, nedits))
    if k < 1:
        raise ValueError("every read needs at least one candidate")
    region = insert + jitter + 64
    zone = n_read_pairs * region
    ref = np.zeros(zone + n_read_pairs * length, dtype=np.uint8)
    span = len(ref) - length + 1
    acgt, bases = b"ACGT", np.frombuffer(b"ACGT", dtype=np.uint8)
    n_reads, n = 2 * n_read_pairs, 2 * n_read_pairs * k
    req = np.zeros(n, dtype=REQUEST_DTYPE)
    rows = np.zeros((n_reads, read_size), dtype=np.uint8)
    tpos = np.zeros(n, dtype=np.uint64)
    truth = np.zeros(n_read_pairs, dtype=MATE_TRUTH_DTYPE)
    plan = []
    for m in range(n_read_pairs):           # the reference first: a window may reach into a neighbour's region or the repeat zone
        rng = np.random.default_rng([int(seed), m, 0x6D617465])
        ref[m * region:(m + 1) * region] = bases[rng.integers(0, 4, size=region)]
        ref[zone + m * length:zone + (m + 1) * length] = bases[rng.integers(0, 4, size=length)]
        frag = insert + int(rng.integers(-jitter, jitter + 1))
        start = m * region + int(rng.integers(0, region - frag + 1))
        u = float(rng.random())
        kind = MATE_REPEAT if u < repeat_frac else (MATE_DISCORDANT if u < repeat_frac + discordant_frac else MATE_UNIQUE)
        wins = [(start, False), (start + frag - length, kind != MATE_DISCORDANT)]     # (position, minus) of the plus-end / minus-end read
        rep_of = int(rng.integers(0, 2)) if kind == MATE_REPEAT else -1
        if rep_of >= 0:
            ref[zone + m * length:zone + (m + 1) * length] = ref[wins[rep_of][0]:wins[rep_of][0] + length]
        plan.append((rng, wins, rep_of, bool(rng.integers(0, 2)), kind))
    for m, (rng, wins, rep_of, swap, kind) in enumerate(plan):
        truth["kind"][m] = kind
        for which in range(2):
            r = 2 * m + (which ^ int(swap))  # swap: the minus-end read is read 2m
            pos, minus = wins[which]
            p = bytearray(ref_window(ref, pos, length, minus).tobytes())
            for _ in range(nedits):
                kd, b, x = int(rng.integers(0, 3)), acgt[int(rng.integers(0, 4))], int(rng.integers(0, 1 << 32))
                if kd == 0 and p:
                    p[x % len(p)] = b
                elif kd == 1 and p:
                    del p[x % len(p)]
                else:
                    p.insert(x % (len(p) + 1), b)
            rows[r, :len(p)] = np.frombuffer(bytes(p), dtype=np.uint8)
            cands = [(pos, minus)]
            if which == rep_of and k >= 2:
                cands.append((zone + m * length, minus))
            while len(cands) < k:
                if rng.random() < 0.5:
                    cands.append((min(max(pos + int(rng.choice([-1, 1])) * int(rng.integers(1, shift + 1)), 0), span - 1), minus))
                else:
                    cands.append((int(rng.integers(0, span)), bool(rng.random() < 0.5)))
            order = rng.permutation(k)
            lo = r * k
            for slot, c in enumerate(order):
                cp, cm = cands[int(c)]
                tpos[lo + slot] = cp | ((1 << 63) if cm else 0)
                if c == 0:
                    truth["true"][m, r & 1] = lo + slot
            req["pattern_len"][lo:lo + k], req["text_len"][lo:lo + k] = len(p), length
    req["idx"] = np.arange(n, dtype=np.uint32)
    txt = np.zeros((n, read_size), dtype=np.uint8)
    for c in range(n):
        tp = int(tpos[c])
        txt[c, :length] = ref_window(ref, tp & ((1 << 63) - 1), length, bool(tp >> 63))
    offsets = np.arange(n_reads + 1, dtype=np.uint32) * np.uint32(k)
    return ref, req, rows, offsets, tpos, txt, np.ascontiguousarray(np.repeat(rows, k, axis=0)), truth


def align_device_groups(params, n_pairs, n_reads, d_requests, d_patterns, d_texts, d_text_pos, d_reference, ref_len, d_read_offsets, d_results,
                        d_ops, d_best, d_scratch, scratch_bytes, stream=None):
    """aim_align_device_groups on device pointers (integers, e.g. torch's data_ptr(); None = NULL): the stateless form of a
    AIM_FLAG_READ_GROUPS batch, e.g. on the buffers seed_candidates returned. Only enqueues work on `stream`."""
    capi.check(capi.load().aim_align_device_groups(params_ref(params), n_pairs, n_reads, d_requests, d_patterns, d_texts, d_text_pos, d_reference,
                                                   ref_len, d_read_offsets, d_results, d_ops, d_best, d_scratch, scratch_bytes, stream))


def align_device_mates(params, n_pairs, n_reads, d_requests, d_patterns, d_text_pos, d_reference, ref_len, d_read_offsets, d_results, d_ops,
                       d_best, mates, d_mates, d_scratch, scratch_bytes, stream=None):
    """aim_align_device_mates on device pointers (integers, e.g. torch's data_ptr(); None = NULL): the stateless form of a
    AIM_FLAG_MATE_PAIRS batch. mates = (min_span, max_span, unpaired_penalty). Only enqueues work on `stream`."""
    lo, hi, pen = (int(x) for x in mates)
    capi.check(capi.load().aim_align_device_mates(params_ref(params), n_pairs, n_reads, d_requests, d_patterns, None, d_text_pos, d_reference,
                                                  ref_len, d_read_offsets, d_results, d_ops, d_best, lo, hi, pen, d_mates, d_scratch,
                                                  scratch_bytes, stream))


def hits_offsets(read_offsets, max_hits):
    """aim_hits_offsets: hit_offsets[n_reads + 1] (uint32), the exclusive prefix sum of min(K_r, max_hits); H is its last entry."""
    ro = np.ascontiguousarray(read_offsets, dtype=np.uint32)
    ho = np.zeros(len(ro), dtype=np.uint32)
    capi.check(capi.load().aim_hits_offsets(len(ro) - 1, capi.ptr(ro), int(max_hits), capi.ptr(ho), None))
    return ho


def align_device_hits(params, n_pairs, n_reads, d_requests, d_patterns, d_texts, d_text_pos, d_reference, ref_len, d_read_offsets, d_results,
                      d_ops, d_best, max_hits, d_hit_offsets, n_hits, d_hit_pair, d_scratch, scratch_bytes, stream=None):
    """aim_align_device_hits on device pointers (integers, e.g. torch's data_ptr(); None = NULL): the stateless form of a
    AIM_FLAG_TOP_HITS batch. d_hit_offsets holds hits_offsets(read_offsets, max_hits) and n_hits its last entry; d_results and d_ops
    receive n_hits rows, d_hit_pair (may be None) the rows' candidates. Only enqueues work on `stream`."""
    capi.check(capi.load().aim_align_device_hits(params_ref(params), n_pairs, n_reads, d_requests, d_patterns, d_texts, d_text_pos, d_reference,
                                                 ref_len, d_read_offsets, d_results, d_ops, d_best, int(max_hits), d_hit_offsets, int(n_hits),
                                                 d_hit_pair, d_scratch, scratch_bytes, stream))


def index_sizes(k, ref_len):
    """aim_index_sizes: (bucket entries = 4^k + 1, pos capacity = ref_len - k + 1, 0 below k)."""
    be, pc = C.c_uint64(), C.c_uint64()
    capi.check(capi.load().aim_index_sizes(int(k), int(ref_len), C.byref(be), C.byref(pc)))
    return be.value, pc.value


def build_index(reference, k, threads=8):
    """aim_index_build on the host: (bucket[4^k + 1], pos[n_pos]) as uint32 arrays for `reference` (bytes or a uint8 array). The
    k-mer at p is reference[p, p + k), base i at bits [2i, 2i + 1] with code (ascii >> 1) & 3; only upper-case A C G T are indexed.
    The result does not depend on `threads`."""
    ref = np.ascontiguousarray(np.frombuffer(reference, dtype=np.uint8) if isinstance(reference, (bytes, bytearray)) else reference, dtype=np.uint8)
    be, pc = index_sizes(k, len(ref))
    bucket = np.zeros(be, dtype=np.uint32)
    pos = np.zeros(max(pc, 1), dtype=np.uint32)
    n = C.c_uint64()
    capi.check(capi.load().aim_index_build(capi.ptr(ref), len(ref), int(k), capi.ptr(bucket), capi.ptr(pos), C.byref(n), int(threads)))
    return bucket, pos[:n.value]


def index_build_minimizers(reference, k, w, threads=8):
    """aim_index_build_minimizers on the host: build_index over the (w, k) minimizers of `reference` alone. pos holds n_pos entries,
    about 2 / (w + 1) of the positions on random sequence; w = 1 gives build_index's arrays."""
    ref = np.ascontiguousarray(np.frombuffer(reference, dtype=np.uint8) if isinstance(reference, (bytes, bytearray)) else reference, dtype=np.uint8)
    be, pc = index_sizes(k, len(ref))
    bucket = np.zeros(be, dtype=np.uint32)
    pos = np.zeros(max(pc, 1), dtype=np.uint32)
    n = C.c_uint64()
    capi.check(capi.load().aim_index_build_minimizers(capi.ptr(ref), len(ref), int(k), int(w), capi.ptr(bucket), capi.ptr(pos), C.byref(n), int(threads)))
    return bucket, pos[:n.value].copy()     # (the capacity is an upper bound: keep pos[0, n_pos) alone)


def index_device_scratch(k, ref_len):
    """aim_index_device_scratch: bytes of device scratch build_index_device / aim_index_build_device need (0 below k)."""
    sb = C.c_uint64()
    capi.check(capi.load().aim_index_device_scratch(int(k), int(ref_len), C.byref(sb)))
    return sb.value


def index_build_device(d_reference, ref_len, k, d_bucket, d_pos, d_scratch, scratch_bytes, stream=None):
    """aim_index_build_device on device pointers (integers, e.g. torch's data_ptr(); None = NULL). Only enqueues work on `stream`."""
    capi.check(capi.load().aim_index_build_device(d_reference, int(ref_len), int(k), d_bucket, d_pos, d_scratch, int(scratch_bytes), stream))


def index_build_device_minimizers(d_reference, ref_len, k, w, d_bucket, d_pos, d_scratch, scratch_bytes, stream=None):
    """aim_index_build_device_minimizers on device pointers: index_build_device over the (w, k) minimizers of the reference alone."""
    capi.check(capi.load().aim_index_build_device_minimizers(d_reference, int(ref_len), int(k), int(w), d_bucket, d_pos, d_scratch, int(scratch_bytes),
                                                             stream))


def build_index_device(reference, k, device="cuda:0", stream=None, w=None):
    """The index of build_index, built on the device. `reference` is bytes, a uint8 numpy array, or a uint8 torch tensor that already
    lives on `device` with at least 16 bytes of slack behind the reference (then ref_len is its length minus 16). Returns
    (d_bucket, d_pos, n_pos): uint8 device tensors in the form seed_candidates accepts for `index`, and bucket[4^k]. d_pos has room
    for ref_len - k + 1 positions; the entries from n_pos on are unspecified. The scratch is allocated here and freed on return.
    With a window `w` the index holds the (w, k) minimizers alone (index_build_device_minimizers)."""
    import torch
    dev = torch.device(device)
    if isinstance(reference, torch.Tensor):
        if reference.dtype != torch.uint8 or reference.device != dev or not reference.is_contiguous() or reference.numel() < 16:
            raise ValueError("a device reference must be a contiguous uint8 tensor on %s with 16 bytes of slack" % dev)
        d_ref, ref_len = reference.reshape(-1), reference.numel() - 16
    else:
        raw = np.ascontiguousarray(np.frombuffer(reference, dtype=np.uint8) if isinstance(reference, (bytes, bytearray)) else reference, dtype=np.uint8)
        ref_len = len(raw)
        d_ref = torch.zeros(ref_len + 16, dtype=torch.uint8, device=dev)
        d_ref[:ref_len] = torch.from_numpy(raw.copy()).to(dev)
    be, pc = index_sizes(k, ref_len)
    sb = index_device_scratch(k, ref_len)
    d_bucket = torch.empty(be * 4, dtype=torch.uint8, device=dev)
    d_pos = torch.empty(max(pc, 1) * 4, dtype=torch.uint8, device=dev)
    d_scr = torch.empty(max(sb, 256), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        s = torch.cuda.current_stream(dev) if stream is None else stream
        if w is None:
            index_build_device(d_ref.data_ptr(), ref_len, k, d_bucket.data_ptr(), d_pos.data_ptr(), d_scr.data_ptr(), sb, s.cuda_stream)
        else:
            index_build_device_minimizers(d_ref.data_ptr(), ref_len, k, w, d_bucket.data_ptr(), d_pos.data_ptr(), d_scr.data_ptr(), sb, s.cuda_stream)
        s.synchronize()
    n_pos = int(d_bucket[(be - 1) * 4:].cpu().numpy().view(np.uint32)[0])
    return d_bucket, d_pos, n_pos


def seed_params(k, read_size, stride=1, max_occ=16, band=8, flank=8, min_votes=2, max_cands=4, idx_base=0, w=None, long_reads=False):
    """aim_seed_params_t, validated like make_params: ValueError names the field that is out of bounds. With a window `w` the seeds
    are the query's (w, k) minimizers (options = AIM_SEED_OPT_MINIMIZERS(w)); stride must then be 1 and the index one of the same
    (k, w). long_reads=True: the parameters are for seed_chain_long_device, whose read_size goes up to SEED_LONG_MAX_READ_SIZE."""
    bounds = (("k", k, 8, 14), ("stride", stride, 1, None), ("max_occ", max_occ, 1, None), ("band", band, 0, None), ("flank", flank, 0, None),
              ("min_votes", min_votes, 1, None), ("max_cands", max_cands, 1, capi.SEED_MAX_CANDS),
              ("read_size", read_size, 8, capi.SEED_LONG_MAX_READ_SIZE if long_reads else capi.SEED_MAX_READ_SIZE))
    for name, v, lo, hi in bounds:
        if int(v) != v or v < lo or (hi is not None and v > hi) or v >= 1 << 31:
            raise ValueError("%s %r is outside %d..%s" % (name, v, lo, "" if hi is None else hi))
    if read_size % 8:
        raise ValueError("read_size %d is not a multiple of 8" % read_size)
    options = 0
    if w is not None:
        if int(w) != w or w < 1 or w > capi.SEED_MAX_W:
            raise ValueError("w %r is outside 1..%d" % (w, capi.SEED_MAX_W))
        if stride != 1:
            raise ValueError("stride %r must be 1 with minimizers (w)" % (stride,))
        options = capi.SEED_OPT_MINIMIZERS(w)
    return capi.SeedParams(int(k), int(stride), int(max_occ), int(band), int(flank), int(min_votes), int(max_cands), int(read_size),
                           int(idx_base) & 0xFFFFFFFF, options)


def seed_groups_offsets(n_reads, max_cands):
    """aim_seed_groups_offsets: read_offsets[r] = r * K (uint32, n_reads + 1 entries), the CSR of the seeding kernel's slots."""
    ro = np.zeros(n_reads + 1, dtype=np.uint32)
    capi.check(capi.load().aim_seed_groups_offsets(int(n_reads), int(max_cands), capi.ptr(ro)))
    return ro


def seed_device(sp, n_reads, d_read_len, d_reads, d_bucket, d_pos, ref_len, d_requests, d_text_pos, d_votes, d_seed, stream=None):
    """aim_seed_device on device pointers (integers, e.g. torch's data_ptr(); None = NULL). Only enqueues work on `stream`."""
    capi.check(capi.load().aim_seed_device(C.byref(sp), int(n_reads), d_read_len, d_reads, d_bucket, d_pos, int(ref_len), d_requests,
                                           d_text_pos, d_votes, d_seed, stream))


def seed_chain_device(sp, n_reads, d_read_len, d_reads, d_bucket, d_pos, ref_len, d_requests, d_text_pos, d_votes, d_seed, d_chains=None, stream=None):
    """aim_seed_chain_device on device pointers: seed_device with the hits chained instead of voted (band <= SEED_CHAIN_MAX_BAND);
    d_chains (aim_chain_t per slot) may be None."""
    capi.check(capi.load().aim_seed_chain_device(C.byref(sp), int(n_reads), d_read_len, d_reads, d_bucket, d_pos, int(ref_len), d_requests,
                                                 d_text_pos, d_votes, d_seed, d_chains, stream))


def seed_chain_candidates(sp, index, ref_len, read_len, reads, device="cuda:0"):
    """seed_candidates through the chaining kernels: the same arguments and the same dict, where "votes" holds the chains' scores,
    plus numpy "chains" (CHAIN_DTYPE, one per slot) and the device tensor "d_chains"."""
    return seed_candidates(sp, index, ref_len, read_len, reads, device=device, chain=True)


def seed_chain_long_device(sp, max_hits, n_reads, d_read_len, d_reads, d_bucket, d_pos, ref_len, d_requests, d_text_pos, d_votes, d_seed, d_chains=None,
                           stream=None):
    """aim_seed_chain_long_device on device pointers: seed_chain_device over minimizer seeds with the hit cap `max_hits` (a power of two
    in 1024..SEED_LONG_MAX_HITS) and read_size up to SEED_LONG_MAX_READ_SIZE."""
    capi.check(capi.load().aim_seed_chain_long_device(C.byref(sp), int(max_hits), int(n_reads), d_read_len, d_reads, d_bucket, d_pos, int(ref_len),
                                                      d_requests, d_text_pos, d_votes, d_seed, d_chains, stream))


def seed_chain_long_candidates(sp, max_hits, index, ref_len, read_len, reads, device="cuda:0"):
    """seed_chain_candidates through seed_chain_long_kernel: the same dict, for the parameters of seed_params(..., long_reads=True) and
    the hit cap `max_hits`; `index` is a minimizer index of sp's (k, w)."""
    return seed_candidates(sp, index, ref_len, read_len, reads, device=device, chain=True, max_hits=int(max_hits))


def chain_classify_device(K, read_size, mask_q8, n_reads, d_read_len, d_text_pos, d_seed, d_chains, d_class, stream=None):
    """aim_chain_classify_device on device pointers (integers, e.g. torch's data_ptr(); None = NULL): rule 8c over the buffers of
    seed_chain_device / seed_chain_long_device -> aim_chain_class_t per slot in d_class. Only enqueues work on `stream`."""
    capi.check(capi.load().aim_chain_classify_device(int(K), int(read_size), int(mask_q8), int(n_reads), d_read_len, d_text_pos, d_seed, d_chains,
                                                     d_class, stream))


def read_mapq_device(K, n_reads, score_unit, d_best, d_mates, d_class, d_mapq, stream=None):
    """aim_read_mapq_device on device pointers: rule 9c over the aim_best_t rows (and the aim_mate_t rows, or None) of
    align_device_groups / align_device_mates and chain_classify_device's d_class -> aim_read_mapq_t per read in d_mapq."""
    capi.check(capi.load().aim_read_mapq_device(int(K), int(n_reads), int(score_unit), d_best, d_mates, d_class, d_mapq, stream))


def chain_classify(sp, cands, mask_q8=capi.CHAIN_MASK_DEFAULT):
    """Classifies the candidates of seed_chain_candidates / seed_chain_long_candidates where they live: takes the aim_seed_params_t of
    that call and the dict it returned, and adds numpy "class" (CHAIN_CLASS_DTYPE, one per slot) and the uint8 device tensor "d_class",
    which read_mapq_device takes after the alignment. Returns the dict."""
    import torch
    if "d_chains" not in cands:
        raise ValueError("chain_classify takes the dict of seed_chain_candidates or seed_chain_long_candidates: d_chains is missing")
    dev = cands["d_chains"].device
    n, K = len(cands["seed"]), sp.max_cands
    cands["d_class"] = torch.zeros(max(n * K, 1) * 8, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        chain_classify_device(K, sp.read_size, mask_q8, n, cands["d_read_len"].data_ptr(), cands["d_text_pos"].data_ptr(), cands["d_seed"].data_ptr(),
                              cands["d_chains"].data_ptr(), cands["d_class"].data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    cands["class"] = cands["d_class"].cpu().numpy().view(capi.CHAIN_CLASS_DTYPE)[:n * K]
    return cands


def split_segments_device(K, read_size, flank, ref_len, n_reads, d_read_len, d_reads, d_requests, d_text_pos, d_seed, d_chains, d_class, d_seg_requests,
                          d_seg_text_pos, d_seg_patterns, d_seg, stream=None):
    """aim_split_segments_device on device pointers (integers, e.g. torch's data_ptr(); None = NULL): rule 10c over the buffers of
    seed_chain_device / seed_chain_long_device and chain_classify_device -> one segment row per slot (request, text_pos, pattern row of
    read_size bytes, aim_segment_t). `flank` is the one the chains were built with. Only enqueues work on `stream`."""
    capi.check(capi.load().aim_split_segments_device(int(K), int(read_size), int(flank), int(ref_len), int(n_reads), d_read_len, d_reads, d_requests,
                                                     d_text_pos, d_seed, d_chains, d_class, d_seg_requests, d_seg_text_pos, d_seg_patterns, d_seg, stream))


def sam_device_split(params, n_rows, d_requests, d_text_pos, d_sel, d_results, d_ops, d_reference, ref_len, options, d_sam, d_cigar, cigar_cap,
                     d_md, md_cap, d_cursors, d_seg, stream=None):
    """aim_sam_device_split on device pointers: sam_device over aligned segment rows, with d_seg (aim_segment_t, indexed like
    d_text_pos) adding the rest of each read to the soft clips and SAM_SUPPLEMENTARY to the flags."""
    capi.check(capi.load().aim_sam_device_split(params_ref(params), n_rows, d_requests, d_text_pos, d_sel, d_results, d_ops, d_reference, ref_len,
                                                options, d_sam, d_cigar, cigar_cap, d_md, md_cap, d_cursors, d_seg, stream))


def split_segments(sp, cands, ref_len):
    """Splits the classified candidates of chain_classify where they live: takes the aim_seed_params_t of the chaining call, the dict
    chain_classify returned and the length of the reference the chains were built on, and adds the uint8 device tensors "d_seg_req", "d_seg_text_pos", "d_seg_patterns"
    and "d_seg" (one row per slot, for align_device_ref and sam_device_split) and their host copies "seg_req" (REQUEST_DTYPE),
    "seg_text_pos" (uint64), "seg_patterns" (uint8[n * K][read_size]) and "seg" (SEGMENT_DTYPE). Returns the dict."""
    import torch
    if "d_class" not in cands or "d_chains" not in cands:
        raise ValueError("split_segments takes the dict of chain_classify: d_class is missing")
    dev = cands["d_class"].device
    n, K, rs = len(cands["seed"]), sp.max_cands, sp.read_size
    slots = max(n * K, 1)
    cands["d_seg_req"] = torch.zeros(slots * 16, dtype=torch.uint8, device=dev)
    cands["d_seg_text_pos"] = torch.zeros(slots * 8, dtype=torch.uint8, device=dev)
    cands["d_seg_patterns"] = torch.zeros(slots * rs + 64, dtype=torch.uint8, device=dev)
    cands["d_seg"] = torch.zeros(slots * 8, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        split_segments_device(K, rs, sp.flank, int(ref_len), n, cands["d_read_len"].data_ptr(), cands["d_reads"].data_ptr(), cands["d_req"].data_ptr(),
                              cands["d_text_pos"].data_ptr(), cands["d_seed"].data_ptr(), cands["d_chains"].data_ptr(), cands["d_class"].data_ptr(),
                              cands["d_seg_req"].data_ptr(), cands["d_seg_text_pos"].data_ptr(), cands["d_seg_patterns"].data_ptr(), cands["d_seg"].data_ptr(),
                              torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    cands["seg_req"] = cands["d_seg_req"].cpu().numpy().view(capi.REQUEST_DTYPE)[:n * K]
    cands["seg_text_pos"] = cands["d_seg_text_pos"].cpu().numpy().view(np.uint64)[:n * K]
    cands["seg_patterns"] = cands["d_seg_patterns"].cpu().numpy()[:n * K * rs].reshape(n * K, rs)
    cands["seg"] = cands["d_seg"].cpu().numpy().view(capi.SEGMENT_DTYPE)[:n * K]
    return cands


def extend_params(match=1, mismatch=3, gap_o=4, gap_e=1, xdrop=20, max_cost=400, band=capi.EXTEND_MAX_BAND, max_ext=64):
    """aim_extend_params_t (rule 11c): the score (match +a, mismatch -x, a gap of g bases -(o + g e)), the x-drop Z, the cost cap,
    the band and the longest extension of a side. The library checks the bounds."""
    return capi.ExtendParams(int(match), int(mismatch), int(gap_o), int(gap_e), int(xdrop), int(max_cost), int(band), int(max_ext))


def extend_segments_device(ep, K, read_size, ref_len, n_reads, d_read_len, d_reads, d_reference, d_seg_requests, d_seg_text_pos, d_seg_patterns, d_seg,
                           d_ext, stream=None):
    """aim_extend_segments_device on device pointers (integers, e.g. torch's data_ptr(); None = NULL): rule 11c over the four outputs of
    split_segments_device, which it rewrites in place where an inner side moved, and aim_extend_t per slot in d_ext. d_reference is the
    resident reference of ref_len bytes. Only enqueues work on `stream`."""
    capi.check(capi.load().aim_extend_segments_device(C.byref(ep) if ep is not None else None, int(K), int(read_size), int(ref_len), int(n_reads), d_read_len,
                                                      d_reads, d_reference, d_seg_requests, d_seg_text_pos, d_seg_patterns, d_seg, d_ext, stream))


def extend_segments(sp, split_out, ref, ep=None):
    """Extends the inner sides of the segments of split_segments where they live: takes the aim_seed_params_t of the chaining call, the
    dict split_segments returned, the reference the chains were built on (a numpy uint8 array, or a uint8 torch tensor on the device;
    its length is ref_len) and aim_extend_params_t (extend_params(); None = its defaults). Updates "d_seg_req", "d_seg_text_pos", "d_seg_patterns", "d_seg"
    and their host copies "seg_req", "seg_text_pos", "seg_patterns", "seg", and adds "d_ext" and numpy "ext" (EXTEND_DTYPE, one per
    slot). Returns the dict."""
    import torch
    if "d_seg" not in split_out:
        raise ValueError("extend_segments takes the dict of split_segments: d_seg is missing")
    ep = extend_params() if ep is None else ep
    dev = split_out["d_seg"].device
    n, K, rs = len(split_out["seed"]), sp.max_cands, sp.read_size
    d_ref = ref if isinstance(ref, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ref, dtype=np.uint8)).to(dev)
    ref_len = int(d_ref.numel())
    split_out["d_ext"] = torch.zeros(max(n * K, 1) * 24, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        extend_segments_device(ep, K, rs, ref_len, n, split_out["d_read_len"].data_ptr(), split_out["d_reads"].data_ptr(), d_ref.data_ptr(),
                               split_out["d_seg_req"].data_ptr(), split_out["d_seg_text_pos"].data_ptr(), split_out["d_seg_patterns"].data_ptr(),
                               split_out["d_seg"].data_ptr(), split_out["d_ext"].data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    split_out["seg_req"] = split_out["d_seg_req"].cpu().numpy().view(capi.REQUEST_DTYPE)[:n * K]
    split_out["seg_text_pos"] = split_out["d_seg_text_pos"].cpu().numpy().view(np.uint64)[:n * K]
    split_out["seg_patterns"] = split_out["d_seg_patterns"].cpu().numpy()[:n * K * rs].reshape(n * K, rs)
    split_out["seg"] = split_out["d_seg"].cpu().numpy().view(capi.SEGMENT_DTYPE)[:n * K]
    split_out["ext"] = split_out["d_ext"].cpu().numpy().view(capi.EXTEND_DTYPE)[:n * K]
    return split_out


def map_records_scratch(n_reads):
    """aim_map_records_scratch: bytes of device scratch map_records_device needs."""
    return int(capi.load().aim_map_records_scratch(int(n_reads)))


def map_records_device(K, n_reads, d_seg, d_sam, d_class, d_rec_offsets, d_records, d_scratch, scratch_bytes, stream=None):
    """aim_map_records_device on device pointers (integers, e.g. torch's data_ptr(); None = NULL): rule 12c over the aim_segment_t rows of
    split_segments_device / extend_segments_device, the aim_sam_t rows of sam_device_split (d_sel = None) and chain_classify_device's
    d_class -> d_rec_offsets (uint32[n_reads + 1]) and the dense aim_map_record_t list in d_records (room for n_reads * K).
    Only enqueues work on `stream`."""
    capi.check(capi.load().aim_map_records_device(int(K), int(n_reads), d_seg, d_sam, d_class, d_rec_offsets, d_records, d_scratch, int(scratch_bytes), stream))


def _contig_arrays(seqs):
    """(uint8 arrays kept alive, lens uint32[n], a ctypes array of their addresses) for the `seqs` / `lens` arguments of rule 13c."""
    arrs = [np.ascontiguousarray(np.frombuffer(s, dtype=np.uint8) if isinstance(s, (bytes, bytearray)) else s, dtype=np.uint8) for s in seqs]
    lens = np.array([len(a) for a in arrs], dtype=np.uint32)
    ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
    return arrs, lens, ptrs


def contigs_layout(lens, spacer):
    """aim_contigs_layout: (starts uint32[n], ref_len) of contigs of these lengths with `spacer` 'N' bases between neighbours."""
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    starts = np.zeros(len(lens), dtype=np.uint32)
    ref_len = C.c_uint64()
    capi.check(capi.load().aim_contigs_layout(len(lens), capi.ptr(lens) if len(lens) else None, int(spacer), capi.ptr(starts) if len(lens) else None, C.byref(ref_len)))
    return starts, ref_len.value


def contigs_concat(seqs, spacer):
    """aim_contigs_concat: the concatenation (uint8 array) of rule 13c's layout, 'N' in the gaps."""
    arrs, lens, ptrs = _contig_arrays(seqs)
    ref_len = contigs_layout(lens, spacer)[1]
    out = np.zeros(ref_len, dtype=np.uint8)
    capi.check(capi.load().aim_contigs_concat(len(arrs), ptrs, capi.ptr(lens), int(spacer), capi.ptr(out)))
    return out


def contig_clip_device(K, read_size, flank, ref_len, n_contigs, d_contig_start, d_contig_len, n_reads, d_read_len, d_requests, d_text_pos, d_chains, d_seg_requests,
                       d_seg_text_pos, d_seg, d_contig, stream=None):
    """aim_contig_clip_device on device pointers (integers, e.g. torch's data_ptr(); None = NULL): rule 13c's clip over the segment
    buffers of split_segments_device / extend_segments_device, in place, from the candidates' own d_requests / d_text_pos / d_chains;
    d_contig (uint32 per slot) receives the contig of every valid slot. Only enqueues work on `stream`."""
    capi.check(capi.load().aim_contig_clip_device(int(K), int(read_size), int(flank), int(ref_len), int(n_contigs), d_contig_start, d_contig_len, int(n_reads), d_read_len,
                                                  d_requests, d_text_pos, d_chains, d_seg_requests, d_seg_text_pos, d_seg, d_contig, stream))


def map_records_contigs_device(K, n_reads, d_seg, d_sam, d_class, d_contig, n_contigs, d_contig_start, d_rec_offsets, d_records, d_scratch, scratch_bytes, stream=None):
    """aim_map_records_contigs_device: map_records_device with contig_clip_device's d_contig -- pos local to the contig, pad = the contig."""
    capi.check(capi.load().aim_map_records_contigs_device(int(K), int(n_reads), d_seg, d_sam, d_class, d_contig, int(n_contigs), d_contig_start, d_rec_offsets,
                                                          d_records, d_scratch, int(scratch_bytes), stream))


def mapper_device_bytes_contigs(mp, lens):
    """aim_mapper_device_bytes_contigs: the device memory a Mapper.from_contigs of these parameters and contig lengths takes at its peak."""
    lens = np.ascontiguousarray(lens, dtype=np.uint32)
    b = C.c_uint64()
    capi.check(capi.load().aim_mapper_device_bytes_contigs(C.byref(mp), len(lens), capi.ptr(lens) if len(lens) else None, C.byref(b)))
    return b.value


def pair_params(min_span, max_span, unpaired_penalty=0, rescue=True, rescue_size=0, rescue_cigar_cap=0, rescue_md_cap=0):
    """aim_map_pair_params_t (rule 14c): the span bounds in aligned coordinates, the penalty of the unpaired choice, and -- with rescue --
    the read_size of the rescue alignment (a multiple of 8, at least max_span - min_span + read_size) and the mapper's rescue regions."""
    return capi.MapPairParams(int(min_span), int(max_span), int(unpaired_penalty), capi.PAIR_RESCUE if rescue else 0, int(rescue_size), int(rescue_cigar_cap),
                              int(rescue_md_cap), 0)


def pair_rescue_rows_device(pp, K, read_size, ref_len, n_reads, d_read_len, d_reads, d_seg, d_sam, d_res_requests, d_res_text_pos, d_res_patterns, d_contig=None,
                            n_contigs=0, d_contig_start=None, d_contig_len=None, stream=None):
    """aim_pair_rescue_rows_device on device pointers (integers, e.g. torch's data_ptr(); None = NULL): rule 14c's rescue row per read --
    aim_request_t, text_pos and the pattern row at stride pp.rescue_size -- from the slot arrays behind sam_device_split. d_contig (with
    the contig table) for a reference of several sequences. Only enqueues work on `stream`."""
    capi.check(capi.load().aim_pair_rescue_rows_device(C.byref(pp), int(K), int(read_size), int(ref_len), int(n_contigs), d_contig_start, d_contig_len, int(n_reads),
                                                       d_read_len, d_reads, d_seg, d_sam, d_contig, d_res_requests, d_res_text_pos, d_res_patterns, stream))


def pair_select_device(pp, K, read_size, n_reads, d_read_len, d_seg, d_sam, d_class, d_res_sam, cigar_base, md_base, d_pairs, d_contig=None, stream=None):
    """aim_pair_select_device: rule 14c's choice per read pair -> d_pairs (capi.MAP_PAIR_DTYPE per pair), and apply: a chosen rescue row
    (d_res_sam, the sam_device records of the rescue rows) folded into d_seg / d_sam / d_class / d_contig in place. Only enqueues work."""
    capi.check(capi.load().aim_pair_select_device(C.byref(pp), int(K), int(read_size), int(n_reads), d_read_len, d_seg, d_sam, d_class, d_contig, d_res_sam,
                                                  int(cigar_base), int(md_base), d_pairs, stream))


def map_mates_device(K, n_reads, d_pairs, d_seg, d_sam, d_rec_offsets, d_records, d_mates, d_contig=None, n_contigs=0, d_contig_start=None, stream=None):
    """aim_map_mates_device, behind map_records_device / map_records_contigs_device: the paired flag bits into d_records and one
    capi.MAP_MATE_DTYPE per record into d_mates (room for n_reads * K). Only enqueues work."""
    capi.check(capi.load().aim_map_mates_device(int(K), int(n_reads), d_pairs, d_seg, d_sam, d_contig, int(n_contigs), d_contig_start, d_rec_offsets, d_records,
                                                d_mates, stream))


def pair_estimate_params(hist_size=2048, min_samples=64, min_mapq=20, min_slack=16):
    """aim_pair_est_params_t (rule 15c): the histogram's bins of one base (64..8192, a multiple of 64), the binned samples below which the
    estimate falls back to pair_params' own bounds, the MAPQ either mate of a sample needs, and the floor of the spread 3 * IQR."""
    return capi.PairEstParams(int(hist_size), int(min_samples), int(min_mapq), int(min_slack))


def pair_estimate_scratch(hist_size):
    """aim_pair_estimate_scratch: the bytes of d_scratch pair_estimate_device wants."""
    return int(capi.load().aim_pair_estimate_scratch(int(hist_size)))


def estimate_dict(e):
    """An aim_pair_estimate_t (capi.PairEstimate, or one item of capi.PAIR_ESTIMATE_DTYPE) as a dict of Python integers."""
    names = ("min_span", "max_span", "n_samples", "n_beyond", "p25", "p50", "p75", "flags")
    return {k: int(getattr(e, k) if isinstance(e, capi.PairEstimate) else e[k]) for k in names}


def pair_estimate_device(pp, ep, K, read_size, n_reads, d_seg, d_sam, d_class, d_est, d_scratch, scratch_bytes, d_contig=None, stream=None):
    """aim_pair_estimate_device on device pointers: rule 15c's span bounds of the batch, from the slot arrays behind sam_device_split, into
    the 48 bytes at d_est (capi.PAIR_ESTIMATE_DTYPE). d_scratch may hold anything. Only enqueues work on `stream`."""
    capi.check(capi.load().aim_pair_estimate_device(C.byref(pp), C.byref(ep), int(K), int(read_size), int(n_reads), d_seg, d_sam, d_class, d_contig, d_est, d_scratch,
                                                    int(scratch_bytes), stream))


def pair_rescue_rows_device_est(pp, K, read_size, ref_len, n_reads, d_read_len, d_reads, d_seg, d_sam, d_res_requests, d_res_text_pos, d_res_patterns, d_est,
                                d_contig=None, n_contigs=0, d_contig_start=None, d_contig_len=None, stream=None):
    """aim_pair_rescue_rows_device_est: pair_rescue_rows_device with min_span / max_span read from d_est on the device (rule 15c)."""
    capi.check(capi.load().aim_pair_rescue_rows_device_est(C.byref(pp), int(K), int(read_size), int(ref_len), int(n_contigs), d_contig_start, d_contig_len, int(n_reads),
                                                           d_read_len, d_reads, d_seg, d_sam, d_contig, d_res_requests, d_res_text_pos, d_res_patterns, d_est, stream))


def pair_select_device_est(pp, K, read_size, n_reads, d_read_len, d_seg, d_sam, d_class, d_res_sam, cigar_base, md_base, d_pairs, d_est, d_contig=None, stream=None):
    """aim_pair_select_device_est: pair_select_device with min_span / max_span read from d_est on the device (rule 15c)."""
    capi.check(capi.load().aim_pair_select_device_est(C.byref(pp), int(K), int(read_size), int(n_reads), d_read_len, d_seg, d_sam, d_class, d_contig, d_res_sam,
                                                      int(cigar_base), int(md_base), d_pairs, d_est, stream))


def mapper_pairing_device_bytes(mp, pp):
    """aim_mapper_pairing_device_bytes: the device memory Mapper.set_pairing adds, over all slots."""
    b = C.c_uint64()
    capi.check(capi.load().aim_mapper_pairing_device_bytes(C.byref(mp), C.byref(pp), C.byref(b)))
    return b.value


def secondary_params(max_sec=capi.SEC_MAX, records=True):
    """aim_map_sec_params_t (rule 16c): how many secondaries of a locus are aligned next to its primary (1..capi.SEC_MAX, in candidate
    order), and whether the mapped members that lost come back as SAM secondary records (0x100) behind the read's locus records."""
    return capi.MapSecParams(int(max_sec), capi.SEC_RECORDS if records else 0)


def secondary_rows_device(K, read_size, flank, ref_len, n_reads, d_read_len, d_reads, d_requests, d_text_pos, d_seed, d_chains, d_class, d_seg_requests,
                          d_seg_text_pos, d_seg_patterns, d_seg, max_sec, stream=None):
    """aim_secondary_rows_device on device pointers (integers, e.g. torch's data_ptr(); None = NULL): rule 16c part 1 over the four outputs
    of split_segments_device / extend_segments_device, in place -- a secondary whose parent has a segment gets a row over the parent's
    read interval; every other slot keeps every byte. Only enqueues work on `stream`."""
    capi.check(capi.load().aim_secondary_rows_device(int(K), int(read_size), int(flank), int(ref_len), int(n_reads), d_read_len, d_reads, d_requests, d_text_pos,
                                                     d_seed, d_chains, d_class, d_seg_requests, d_seg_text_pos, d_seg_patterns, d_seg, int(max_sec), stream))


def secondary_select_device(K, n_reads, d_seg, d_sam, d_class, d_chains, max_score, score_unit, d_sec, stream=None):
    """aim_secondary_select_device: rule 16c part 2 behind sam_device_split -- one capi.SEC_SLOT_DTYPE per slot in d_sec: the winner of
    each locus by alignment score, its MAPQ from the runner-up, and who becomes a secondary record. Only enqueues work on `stream`."""
    capi.check(capi.load().aim_secondary_select_device(int(K), int(n_reads), d_seg, d_sam, d_class, d_chains, int(max_score), int(score_unit), d_sec, stream))


def map_records_secondary_device(K, n_reads, options, d_seg, d_sam, d_class, d_sec, d_rec_offsets, d_records, d_sec_records, d_scratch, scratch_bytes,
                                 d_contig=None, n_contigs=0, d_contig_start=None, stream=None):
    """aim_map_records_secondary_device: rule 16c part 3 -- map_records_device over loci, keyed on d_sec: d_rec_offsets, the dense
    aim_map_record_t list and one capi.MAP_SEC_DTYPE per record in d_sec_records (room for n_reads * K each). options: capi.SEC_RECORDS.
    d_contig (with the contig table) for a reference of several sequences. Only enqueues work on `stream`."""
    capi.check(capi.load().aim_map_records_secondary_device(int(K), int(n_reads), int(options), d_seg, d_sam, d_class, d_sec, d_contig, int(n_contigs), d_contig_start,
                                                            d_rec_offsets, d_records, d_sec_records, d_scratch, int(scratch_bytes), stream))


def pair_rescue_rows_secondary_device(pp, K, read_size, ref_len, n_reads, d_read_len, d_reads, d_seg, d_sam, d_sec, d_res_requests, d_res_text_pos, d_res_patterns,
                                      d_est=None, d_contig=None, n_contigs=0, d_contig_start=None, d_contig_len=None, stream=None):
    """aim_pair_rescue_rows_secondary_device (rule 17c): pair_rescue_rows_device over the slots d_sec -- secondary_select_device's output --
    gave a role, anchored at the mate's representative. d_est (capi.PAIR_ESTIMATE_DTYPE on the device) replaces pp's span bounds."""
    capi.check(capi.load().aim_pair_rescue_rows_secondary_device(C.byref(pp), int(K), int(read_size), int(ref_len), int(n_contigs), d_contig_start, d_contig_len,
                                                                 int(n_reads), d_read_len, d_reads, d_seg, d_sam, d_contig, d_sec, d_res_requests, d_res_text_pos,
                                                                 d_res_patterns, d_est, stream))


def pair_select_secondary_device(pp, K, read_size, n_reads, d_read_len, d_seg, d_sam, d_class, d_sec, d_chains, score_unit, d_res_sam, cigar_base, md_base, d_pairs,
                                 d_pair_mapq, d_est=None, d_contig=None, stream=None):
    """aim_pair_select_secondary_device (rule 17c): rule 14c's choice over primaries and aligned secondaries -> d_pairs, the MAPQ of both
    reads from the pair's runner-up -> d_pair_mapq (capi.MAP_PAIR_MAPQ_DTYPE per pair), and apply: the chosen slots' MAPQ and roles into
    d_sec, a chosen rescue row into the slot arrays. Only enqueues work."""
    capi.check(capi.load().aim_pair_select_secondary_device(C.byref(pp), int(K), int(read_size), int(n_reads), d_read_len, d_seg, d_sam, d_class, d_contig, d_sec,
                                                            d_chains, int(score_unit), d_res_sam, int(cigar_base), int(md_base), d_pairs, d_pair_mapq, d_est, stream))


def map_mates_secondary_device(K, n_reads, d_pairs, d_seg, d_sam, d_sec, d_rec_offsets, d_records, d_mates, d_contig=None, n_contigs=0, d_contig_start=None,
                               stream=None):
    """aim_map_mates_secondary_device, behind map_records_secondary_device: map_mates_device with the mate's representative read from
    d_sec; 0x100 records get mate fields, never 0x2. Only enqueues work."""
    capi.check(capi.load().aim_map_mates_secondary_device(int(K), int(n_reads), d_pairs, d_seg, d_sam, d_sec, d_contig, int(n_contigs), d_contig_start, d_rec_offsets,
                                                          d_records, d_mates, stream))


def mapper_pairing_secondary_device_bytes(mp, pp, sc):
    """aim_mapper_pairing_secondary_device_bytes: the device memory Mapper.set_pairing_secondary adds, over all slots (without an estimate's)."""
    b = C.c_uint64()
    capi.check(capi.load().aim_mapper_pairing_secondary_device_bytes(C.byref(mp), C.byref(pp), C.byref(sc), C.byref(b)))
    return b.value


def mapper_secondary_device_bytes(mp, sc):
    """aim_mapper_secondary_device_bytes: the device memory Mapper.set_secondary adds, over all slots."""
    b = C.c_uint64()
    capi.check(capi.load().aim_mapper_secondary_device_bytes(C.byref(mp), C.byref(sc), C.byref(b)))
    return b.value


def mapper_params(sp, max_reads, max_score, mismatch=3, gap_o=4, gap_e=1, match=0, max_hits=0, mask_q8=capi.CHAIN_MASK_DEFAULT, extend=None, sam_options=0,
                  slots=2, cigar_cap=None, md_cap=None):
    """aim_mapper_params_t from the seed parameters of seed_params(..., w=...) (K is sp.max_cands, read_size sp.read_size), the batch
    size, and the WFA penalties and cap of the segment alignment. extend: extend_params() to run the segment extension (MAP_EXTEND), or
    None. cigar_cap / md_cap default to 64 words and 256 bytes per slot row. The library checks every bound."""
    K = int(sp.max_cands)
    ep = extend if extend is not None else capi.ExtendParams()
    return capi.MapperParams(sp, int(max_hits), int(mask_q8), ep, capi.MAP_EXTEND if extend is not None else 0, int(match), int(mismatch), int(gap_o),
                             int(gap_e), int(max_score), int(sam_options), int(max_reads), int(slots),
                             int(max_reads * K * 64 if cigar_cap is None else cigar_cap), int(max_reads * K * 256 if md_cap is None else md_cap))


def mapper_device_bytes(mp, ref_len):
    """aim_mapper_device_bytes: the device memory a Mapper of these parameters takes at its peak."""
    b = C.c_uint64()
    capi.check(capi.load().aim_mapper_device_bytes(C.byref(mp), int(ref_len), C.byref(b)))
    return b.value


def _view(addr, count, dtype):
    """A numpy view of `count` items of `dtype` at a host address (an empty array for none)."""
    if not count:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_char * (count * np.dtype(dtype).itemsize)).from_address(addr)
    return np.frombuffer(buf, dtype=dtype)


class Mapper:
    """aim_mapper_t: the reference, its minimizer index and per-slot buffers and streams on one device. submit(slot, read_len, reads)
    copies a batch in and enqueues every stage; wait(slot) returns a dict of numpy views of the slot's pinned buffers -- "records"
    (capi.MAP_RECORD_DTYPE), "rec_offsets" (uint32[n_reads + 1]), "cigar" (uint32 words) and "md" (uint8) -- which stay valid until the
    slot's next submit, plus "cigar_needed" / "md_needed". set_pairing(pp, estimate=pair_estimate_params(...)) (rule 15c) estimates the
    span bounds per batch on the device, pp's own being the fallback; wait's dict then has "pair_estimate", what pair_estimate(slot)
    returns. After set_pairing(pp) (rule 14c) reads 2m and 2m + 1 are mates: wait's dict
    gains what pairs(slot) returns, and where a rescue wrote something "cigar" / "md" reach to the end of the rescue region (which starts
    at cigar_cap / md_cap), so that a rescued record's cigar_offset / md_offset index them like any other. Such a widened view spans the
    gap between the main range's end (cigar_needed / md_needed, at most the capacity) and the region's start: that gap is never copied
    and holds whatever the pinned buffer held -- index the arrays by a record's offsets, do not hash or compare them whole. "rescue_cigar"
    and "rescue_md" are the rescue ranges alone, as views of their own."""
    pairing = None
    estimate = None
    secondaries = None
    combined = False

    def __init__(self, mp, reference, device=0):
        self.lib = capi.load()
        self.params = mp
        ref = np.ascontiguousarray(np.frombuffer(reference, dtype=np.uint8) if isinstance(reference, (bytes, bytearray)) else reference, dtype=np.uint8)
        self.ref_len = len(ref)
        self.contigs = None
        self.handle = C.c_void_p()
        capi.check(self.lib.aim_mapper_create(C.byref(mp), int(device), capi.ptr(ref) if len(ref) else None, len(ref), C.byref(self.handle)))

    @classmethod
    def from_contigs(cls, mp, seqs, device=0):
        """aim_mapper_create_contigs: a mapper over a reference of several sequences (rule 13c). seqs is a list of bytes or uint8 arrays,
        one per contig. The records' pos is local to the contig in rec["sam"]["pad"]; .contigs is (starts, lens), uint32 arrays of the
        layout inside the concatenation, and .ref_len the concatenation's length."""
        self = cls.__new__(cls)
        self.lib = capi.load()
        self.params = mp
        self.contigs = None
        self.handle = C.c_void_p()
        arrs, lens, ptrs = _contig_arrays(seqs)
        capi.check(self.lib.aim_mapper_create_contigs(C.byref(mp), int(device), len(arrs), ptrs, capi.ptr(lens), C.byref(self.handle)))
        n, st, ln = C.c_uint32(), C.c_void_p(), C.c_void_p()
        capi.check(self.lib.aim_mapper_contigs(self.handle, C.byref(n), C.byref(st), C.byref(ln)))
        view = lambda addr: np.frombuffer((C.c_uint32 * n.value).from_address(addr), dtype=np.uint32).copy()
        self.contigs = (view(st.value), view(ln.value))
        self.ref_len = int(self.contigs[0][-1]) + int(self.contigs[1][-1])
        return self

    def close(self):
        if self.handle:
            self.lib.aim_mapper_free(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def set_pairing(self, pp, estimate=None):
        """aim_mapper_set_pairing: once, while no slot is in flight. estimate: pair_estimate_params() for aim_mapper_set_pairing_estimated
        (rule 15c) -- the span bounds come from each batch, pp.min_span / pp.max_span are the fallback."""
        if estimate is None:
            capi.check(self.lib.aim_mapper_set_pairing(self.handle, C.byref(pp)))
        else:
            capi.check(self.lib.aim_mapper_set_pairing_estimated(self.handle, C.byref(pp), C.byref(estimate)))
        self.pairing = pp
        self.estimate = estimate

    def set_secondary(self, sc=None):
        """aim_mapper_set_secondary (rule 16c): once, while no slot is in flight. sc: secondary_params() (None = its defaults). wait's dict
        then has "sec" (capi.MAP_SEC_DTYPE per record), what secondary(slot) returns; records may carry capi.SAM_SECONDARY."""
        sc = secondary_params() if sc is None else sc
        capi.check(self.lib.aim_mapper_set_secondary(self.handle, C.byref(sc)))
        self.secondaries = sc

    def set_pairing_secondary(self, pp, sc=None, estimate=None):
        """aim_mapper_set_pairing_secondary (rule 17c): pairing, the estimate when pair_estimate_params() is given, and secondaries in one
        call on a mapper no other setter has touched. wait's dict then has everything set_pairing and set_secondary add plus "pair_mapq"
        (capi.MAP_PAIR_MAPQ_DTYPE per read pair): the MAPQ of both reads from the pair's runner-up."""
        sc = secondary_params() if sc is None else sc
        capi.check(self.lib.aim_mapper_set_pairing_secondary(self.handle, C.byref(pp), C.byref(estimate) if estimate is not None else None, C.byref(sc)))
        self.pairing, self.estimate, self.secondaries, self.combined = pp, estimate, sc, True

    def pair_mapq(self, slot):
        """aim_mapper_pair_mapq after wait(slot): a view of the capi.MAP_PAIR_MAPQ_DTYPE array parallel to "pairs"."""
        po, v = capi.MapperPairsOut(), C.c_void_p()
        capi.check(self.lib.aim_mapper_pair_mapq(self.handle, int(slot), C.byref(v)))
        capi.check(self.lib.aim_mapper_pairs(self.handle, int(slot), C.byref(po)))
        return _view(v.value, po.n_pairs, capi.MAP_PAIR_MAPQ_DTYPE)

    def secondary(self, slot):
        """aim_mapper_secondary after wait(slot): a view of the capi.MAP_SEC_DTYPE array parallel to "records"."""
        so = capi.MapperSecondaryOut()
        capi.check(self.lib.aim_mapper_secondary(self.handle, int(slot), C.byref(so)))
        return _view(so.sec, so.n_records, capi.MAP_SEC_DTYPE)

    def pair_estimate(self, slot):
        """aim_mapper_pair_estimate after wait(slot): the estimate of the slot's last batch as a dict -- "min_span", "max_span", "n_samples",
        "n_beyond", "p25", "p50", "p75" and "flags" (capi.PAIR_EST_*)."""
        e = capi.PairEstimate()
        capi.check(self.lib.aim_mapper_pair_estimate(self.handle, int(slot), C.byref(e)))
        return estimate_dict(e)

    def pairs(self, slot):
        """aim_mapper_pairs after wait(slot): "mates" (capi.MAP_MATE_DTYPE per record), "pairs" (capi.MAP_PAIR_DTYPE per read pair) and the
        rescue regions' "rescue_cigar_words" / "rescue_md_bytes" (copied) and "rescue_cigar_needed" / "rescue_md_needed"."""
        po = capi.MapperPairsOut()
        capi.check(self.lib.aim_mapper_pairs(self.handle, int(slot), C.byref(po)))
        return {"mates": _view(po.mates, po.n_records, capi.MAP_MATE_DTYPE), "pairs": _view(po.pairs, po.n_pairs, capi.MAP_PAIR_DTYPE),
                "rescue_cigar_words": po.rescue_cigar_words, "rescue_md_bytes": po.rescue_md_bytes, "rescue_cigar_needed": po.rescue_cigar_needed,
                "rescue_md_needed": po.rescue_md_needed}

    def submit(self, slot, read_len, reads):
        rl = np.ascontiguousarray(read_len, dtype=np.int32)
        rows = np.ascontiguousarray(reads, dtype=np.uint8)
        rs = self.params.seed.read_size
        if rows.size != len(rl) * rs:
            raise ValueError("reads must be uint8[%d][%d], got %r" % (len(rl), rs, rows.shape))
        capi.check(self.lib.aim_mapper_submit(self.handle, int(slot), len(rl), capi.ptr(rl) if len(rl) else None, capi.ptr(rows) if len(rl) else None))

    def wait(self, slot):
        out = capi.MapperOut()
        capi.check(self.lib.aim_mapper_wait(self.handle, int(slot), C.byref(out)))
        view = _view
        res = {"n_reads": out.n_reads, "records": view(out.records, out.n_records, capi.MAP_RECORD_DTYPE),
               "rec_offsets": view(out.rec_offsets, out.n_reads + 1, np.uint32), "cigar": view(out.cigar, out.cigar_words, np.uint32),
               "md": view(out.md, out.md_bytes, np.uint8), "cigar_needed": out.cigar_needed, "md_needed": out.md_needed}
        if self.pairing is not None:
            res.update(self.pairs(slot))
            if res["rescue_cigar_words"]:
                res["cigar"] = view(out.cigar, self.params.cigar_cap + res["rescue_cigar_words"], np.uint32)
            if res["rescue_md_bytes"]:
                res["md"] = view(out.md, self.params.md_cap + res["rescue_md_bytes"], np.uint8)
            res["rescue_cigar"] = res["cigar"][self.params.cigar_cap:] if res["rescue_cigar_words"] else np.zeros(0, dtype=np.uint32)
            res["rescue_md"] = res["md"][self.params.md_cap:] if res["rescue_md_bytes"] else np.zeros(0, dtype=np.uint8)
            if self.estimate is not None:
                res["pair_estimate"] = self.pair_estimate(slot)
        if self.secondaries is not None:
            res["sec"] = self.secondary(slot)
        if self.combined:
            res["pair_mapq"] = self.pair_mapq(slot)
        return res


def seed_candidates(sp, index, ref_len, read_len, reads, device="cuda:0", chain=False, max_hits=None):
    """The seeding kernel on torch device buffers. `index` is build_index's (bucket, pos) -- numpy arrays, or uint8 torch tensors
    that already live on the device (as the "d_bucket" / "d_pos" of an earlier call); read_len is int32[n_reads], reads the ASCII
    rows uint8[n_reads][read_size]. Returns a dict: numpy "req" (REQUEST_DTYPE), "text_pos" (uint64), "votes" (uint32) and "seed"
    (SEED_DTYPE), each in slot order r * K + i, and the uint8 device tensors "d_req", "d_text_pos", "d_votes", "d_seed", "d_reads",
    "d_read_len", "d_bucket", "d_pos" for feeding align_device_groups and its siblings without a copy through the host. chain=True
    is seed_chain_candidates, and with max_hits seed_chain_long_candidates."""
    import torch
    dev = torch.device(device)

    def put(x, slack=0):
        if isinstance(x, torch.Tensor):
            return x
        raw = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
        t = torch.zeros(max(len(raw) + slack, 16), dtype=torch.uint8, device=dev)
        t[:len(raw)] = torch.from_numpy(raw.copy()).to(dev)
        return t
    rl = np.ascontiguousarray(read_len, dtype=np.int32)
    rows = np.ascontiguousarray(reads, dtype=np.uint8)
    n, K = len(rl), sp.max_cands
    if rows.shape != (n, sp.read_size):
        raise ValueError("reads must be uint8[%d][%d], got %r" % (n, sp.read_size, rows.shape))
    d = {"d_bucket": put(index[0]), "d_pos": put(index[1]), "d_read_len": put(rl), "d_reads": put(rows, slack=64)}
    slots = max(n * K, 1)
    d["d_req"] = torch.zeros(slots * 16, dtype=torch.uint8, device=dev)
    d["d_text_pos"] = torch.zeros(slots * 8, dtype=torch.uint8, device=dev)
    d["d_votes"] = torch.zeros(slots * 4, dtype=torch.uint8, device=dev)
    d["d_seed"] = torch.zeros(max(n, 1) * 16, dtype=torch.uint8, device=dev)
    if chain:
        d["d_chains"] = torch.zeros(slots * 16, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize(dev)
    with torch.cuda.device(dev):
        args = (sp, n, d["d_read_len"].data_ptr(), d["d_reads"].data_ptr(), d["d_bucket"].data_ptr(), d["d_pos"].data_ptr(), ref_len,
                d["d_req"].data_ptr(), d["d_text_pos"].data_ptr(), d["d_votes"].data_ptr(), d["d_seed"].data_ptr())
        if chain and max_hits is not None:
            seed_chain_long_device(sp, max_hits, *args[1:], d["d_chains"].data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        elif chain:
            seed_chain_device(*args, d["d_chains"].data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        else:
            seed_device(*args, torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize(dev)
    if chain:
        d["chains"] = d["d_chains"].cpu().numpy().view(capi.CHAIN_DTYPE)[:n * K]
    d["req"] = d["d_req"].cpu().numpy().view(capi.REQUEST_DTYPE)[:n * K]
    d["text_pos"] = d["d_text_pos"].cpu().numpy().view(np.uint64)[:n * K]
    d["votes"] = d["d_votes"].cpu().numpy().view(np.uint32)[:n * K]
    d["seed"] = d["d_seed"].cpu().numpy().view(capi.SEED_DTYPE)[:n]
    return d


def sam_device(params, n_rows, d_requests, d_text_pos, d_sel, d_results, d_ops, d_reference, ref_len, options, d_sam, d_cigar, cigar_cap,
               d_md, md_cap, d_cursors, stream=None):
    """aim_sam_device on device pointers (integers, e.g. torch's data_ptr(); None = NULL): SAM records of rows that already live on the
    device, after any align_device* call with backtrace. d_sel = None: row r is candidate r. d_cursors: 2 dwords, zeroed by the call;
    afterwards the CIGAR words and MD bytes the batch needed. Only enqueues work on `stream`."""
    capi.check(capi.load().aim_sam_device(params_ref(params), n_rows, d_requests, d_text_pos, d_sel, d_results, d_ops, d_reference, ref_len,
                                          options, d_sam, d_cigar, cigar_cap, d_md, md_cap, d_cursors, stream))


def sam_kernel_name(params):
    """aim_sam_kernel_name: "sam_lane_kernel" or "sam_wave_kernel", the record kernel a launch with these params takes right now."""
    return capi.load().aim_sam_kernel_name(params_ref(params)).decode()


def sam_format_cigar(words):
    """aim_sam_format_cigar: BAM CIGAR words -> the SAM string ("*" for none)."""
    w = np.ascontiguousarray(words, dtype=np.uint32)
    buf = C.create_string_buffer(12 * len(w) + 2)
    n = capi.check(capi.load().aim_sam_format_cigar(w.ctypes.data if len(w) else None, len(w), buf, len(buf)))
    return buf.raw[:n].decode()


def sam_strings(sam, cigar, md):
    """Per row of `sam` (capi.SAM_DTYPE) the pair (CIGAR string, MD string) from the word and byte buffers; ("*", "") for an unmapped
    row or one marked SAM_OVERFLOW."""
    md = np.asarray(md, dtype=np.uint8)
    out = []
    for r in sam:
        co, nc, mo, ml = int(r["cigar_offset"]), int(r["n_cigar"]), int(r["md_offset"]), int(r["md_len"])
        out.append((sam_format_cigar(cigar[co:co + nc]), md[mo:mo + ml].tobytes().decode("latin-1")))
    return out


def to_request8(req):
    """aim_request_t[] -> aim_request8_t[] (the reference's own 8-byte WFA request_t; AIM_FLAG_REQ8)."""
    out = np.zeros(len(req), dtype=REQUEST8_DTYPE)
    out["pattern_len"], out["text_len"], out["idx"] = req["pattern_len"], req["text_len"], req["idx"]
    return out


def packed_row_dwords(read_size):
    return (read_size + 15) // 16


_CODE = np.full(256, 255, dtype=np.uint8)
for _c, _v in ((ord("A"), 0), (ord("C"), 1), (ord("T"), 2), (ord("G"), 3)):
    _CODE[_c] = _v


def pack_rows(req, rows, key):
    """2 bits per base (aim_hip.h, packed input): returns (packed[n][ceil(rs/16)] uint32, ok[n] bool); ok is False where a
    byte outside A/C/G/T lies inside the sequence (such pairs travel raw). Vectorised twin of aim_pack_sequence."""
    n, rs = rows.shape
    dw = packed_row_dwords(rs)
    lens = np.asarray(req[key], dtype=np.int64)
    inside = np.arange(rs)[None, :] < lens[:, None]
    codes = _CODE[rows]
    ok = ~((codes == 255) & inside).any(axis=1)
    c = np.where(inside & (codes != 255), codes, 0).astype(np.uint32)
    full = np.zeros((n, dw * 16), dtype=np.uint32)
    full[:, :rs] = c
    shifts = (2 * np.arange(16, dtype=np.uint32))[None, None, :]
    packed = (full.reshape(n, dw, 16) << shifts).sum(axis=2, dtype=np.uint64).astype(np.uint32)
    return np.ascontiguousarray(packed), ok


def pack_batch(req, pat, txt):
    """(packedP, packedT, raw_pairs, rawP, rawT) for aim_set_submit: pairs that cannot be packed go to the raw side list.
    txt=None (AIM_FLAG_REF_TEXTS): only the patterns are packed, packedT and rawT are None and a pair is raw when its pattern is."""
    pp, okp = pack_rows(req, pat, "pattern_len")
    if txt is None:
        raw = np.nonzero(~okp)[0].astype(np.uint32)
        return pp, None, raw, np.ascontiguousarray(pat[raw]), None
    pt, okt = pack_rows(req, txt, "text_len")
    raw = np.nonzero(~(okp & okt))[0].astype(np.uint32)
    return pp, pt, raw, np.ascontiguousarray(pat[raw]), np.ascontiguousarray(txt[raw])


def pack_batch_native(params, req, pat, txt, threads=8):
    """aim_pack_batch (host threads in libaim_hip.so): same result as pack_batch, for batches too large for numpy temporaries."""
    lib = capi.load()
    n, rs = len(req), params.read_size
    dw = packed_row_dwords(rs)
    if (params.flags & FLAG_REQ8) and req.dtype != REQUEST8_DTYPE:
        req = to_request8(req)
    with_txt = txt is not None      # (None: AIM_FLAG_REF_TEXTS, only the patterns are packed; packedT and rawT come back None)
    req, pat = np.ascontiguousarray(req), np.ascontiguousarray(pat)
    txt = np.ascontiguousarray(txt) if with_txt else None
    pp = np.zeros((n, dw), dtype=np.uint32)
    pt = np.zeros((n, dw), dtype=np.uint32) if with_txt else None
    cap = max(1, n // 8)
    raw, rawp = np.zeros(cap, dtype=np.uint32), np.zeros((cap, rs), dtype=np.uint8)
    rawt = np.zeros((cap, rs), dtype=np.uint8) if with_txt else None
    nr = C.c_uint32()
    capi.check(lib.aim_pack_batch(params_ref(params), n, capi.ptr(req), capi.ptr(pat), capi.ptr(txt), capi.ptr(pp), capi.ptr(pt),
                                  capi.ptr(raw), capi.ptr(rawp), capi.ptr(rawt), cap, C.byref(nr), threads))
    k = nr.value
    return pp, pt, raw[:k].copy(), rawp[:k].copy(), None if rawt is None else rawt[:k].copy()


def format_output_runs(cig, runs):
    """Output file of the reference host (host.c:339-349) from the compact CIGAR (aim_cigar_t headers + run buffer)."""
    lib = capi.load()
    out = []
    buf = C.create_string_buffer(1 << 16)
    for i in range(len(cig)):
        out.append(b"%d, %d, \n" % (int(cig["idx"][i]), int(cig["score"][i])))
        nr, off = int(cig["n_runs"][i]), int(cig["run_offset"][i])
        r = np.ascontiguousarray(runs[off:off + nr])
        if len(buf) < 12 * nr + 16:
            buf = C.create_string_buffer(12 * nr + 16)
        n = capi.check(lib.aim_cigar_format_runs(capi.ptr(r), nr, buf, len(buf)))
        out.append(buf.raw[:n])
    return b"".join(out)


def pairs_to_text(req, pat, txt):
    """Render pairs in the reference input format ('>'pattern / '<'text lines)."""
    out = []
    for i in range(len(req)):
        out.append(b">" + pat[i, : req["pattern_len"][i]].tobytes() + b"\n")
        out.append(b"<" + txt[i, : req["text_len"][i]].tobytes() + b"\n")
    return b"".join(out)


def parse_pairs(data, read_size, max_pairs=None, first_idx=0):
    """get_reads (host.c:91-134): two lines per pair, first character dropped,
    length = line length - 2 (a final line without newline loses its last base)."""
    lines = data.split(b"\n")
    if lines and lines[-1] == b"":
        lines.pop()
        terminated = True
    else:
        terminated = False
    n = len(lines) // 2
    if max_pairs is not None:
        n = min(n, max_pairs)
    req = np.zeros(n, dtype=REQUEST_DTYPE)
    pat = np.zeros((n, read_size), dtype=np.uint8)
    txt = np.zeros((n, read_size), dtype=np.uint8)
    for i in range(n):
        for arr, key, j in ((pat, "pattern_len", 2 * i), (txt, "text_len", 2 * i + 1)):
            ln = lines[j]
            full = len(ln) + (1 if (terminated or j < len(lines) - 1) else 0)   # getline length incl. '\n'
            length = full - 2
            if length > read_size:
                raise ValueError("READ LENGTH less than length of the input reads")
            seq = ln[1 : 1 + length]
            arr[i, : len(seq)] = np.frombuffer(seq, dtype=np.uint8)
            req[key][i] = length
        req["idx"][i] = first_idx + i
    return req, pat, txt


def cigar_of(ops_row, begin_offset, end_offset):
    lib = capi.load()
    buf = C.create_string_buffer(int(4 * max(16, int(end_offset) - int(begin_offset)) + 32))
    n = capi.check(lib.aim_cigar_format(capi.ptr(ops_row), int(begin_offset), int(end_offset), buf, len(buf)))
    return buf.raw[:n]


def format_output(results, ops, backtrace, ends_free=False):
    """Output file of the reference host (host.c:339-349): 'idx, score, \\n' [+ RLE CIGAR line]. ends_free: a pair with an empty
    CIGAR (ends-free over MAX_SCORE) prints an empty CIGAR line, like `host --ends-free`."""
    out = []
    for i in range(len(results)):
        out.append(b"%d, %d, \n" % (int(results["idx"][i]), int(results["score"][i])))
        if backtrace and ends_free and results["end_offset"][i] <= results["begin_offset"][i]:
            out.append(b"\n")
        elif backtrace:
            out.append(cigar_of(ops[i], results["begin_offset"][i], results["end_offset"][i]))
    return b"".join(out)


class DeviceSet:
    """struct dpu_set_t counterpart: nr_devices GPUs, one stream each."""

    def __init__(self, nr_devices=1, device_ids=None):
        self.lib = capi.load()
        self.handle = C.c_void_p()
        ids = None
        if device_ids is not None:
            ids = (C.c_int * len(device_ids))(*device_ids)
            nr_devices = len(device_ids)
        capi.check(self.lib.aim_set_alloc(nr_devices, ids, C.byref(self.handle)))
        self.nr_devices = nr_devices
        self.params = None
        self.max_pairs = 0

    def close(self):
        if self.handle:
            self.lib.aim_set_free(self.handle)
            self.handle = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def configure(self, params, max_pairs_per_device):
        capi.check(self.lib.aim_set_configure(self.handle, params_ref(params), max_pairs_per_device))
        self.params = params
        self.max_pairs = max_pairs_per_device

    def configure_slots(self, params, max_pairs_per_device, slots=2, max_raw=0, max_runs=0):
        capi.check(self.lib.aim_set_configure_slots(self.handle, params_ref(params), max_pairs_per_device, slots, max_raw, max_runs))
        self.params = params
        self.max_pairs = max_pairs_per_device
        self._inflight = {}

    def sam_capacity(self, max_cigar_words, max_md_bytes):
        """aim_set_sam_capacity: the per-slot device buffers of the SAM records (after configure_slots, before the first submit
        with sam=)."""
        capi.check(self.lib.aim_set_sam_capacity(self.handle, int(max_cigar_words), int(max_md_bytes)))

    def set_reference(self, seq):
        """aim_set_reference: upload `seq` (bytes or a uint8 array, taken verbatim) to every device of the set; replaces the
        previous reference. Batches then name their texts by text_pos (AIM_FLAG_REF_TEXTS)."""
        arr = np.frombuffer(seq, dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else np.ascontiguousarray(seq, dtype=np.uint8)
        capi.check(self.lib.aim_set_reference(self.handle, arr.ctypes.data if len(arr) else None, len(arr)))
        self.ref_len = len(arr)

    def submit(self, device, slot, req, pat=None, txt=None, packed=None, want_ops=False, cigar_runs_cap=0, text_pos=None,
               read_offsets=None, mates=None, sam=None, want_res=None, max_hits=None, hit_offsets=None):
        """aim_set_submit: ASCII rows (pat, txt) or a packed batch (pack_batch(...)); results / ops / compact CIGAR buffers
        are allocated here and returned by wait(). text_pos (AIM_FLAG_REF_TEXTS): the texts are windows of the reference; pass
        pat (or packed = pack_batch(req, pat, None)) and no texts. read_offsets (AIM_FLAG_READ_GROUPS): req and the texts are per
        candidate, pat holds one row per read; wait() returns one row per read and "best" (capi.BEST_DTYPE). mates = (min_span,
        max_span, unpaired_penalty) (AIM_FLAG_MATE_PAIRS, with read_offsets and text_pos): reads 2m and 2m + 1 are mates; wait() also
        returns "mates" (capi.MATE_DTYPE, one row per read pair) next to "best", which stays the independent selection.
        sam = (cigar_cap, md_cap, options) (AIM_FLAG_SAM_FIELDS): wait() also returns "sam" (capi.SAM_DTYPE, one record per output
        row), "sam_cigar" (BAM words) and "sam_md" (bytes); want_res=False then sends no result rows back.
        max_hits (AIM_FLAG_TOP_HITS, with read_offsets): every read's max_hits best candidates; wait() returns one row per hit, in
        rank order at [hit_offsets[r], hit_offsets[r + 1]), plus "hit_pair" (the rows' candidates) and "hit_offsets" -- computed here
        by hits_offsets() unless hit_offsets is given."""
        if (self.params.flags & FLAG_REQ8) and req.dtype != REQUEST8_DTYPE:
            req = to_request8(req)
        req = np.ascontiguousarray(req)
        n, rs = len(req), self.params.read_size
        hio = capi.BatchIOHits() if (self.params.flags & capi.FLAG_TOP_HITS) else None
        if (max_hits is not None) != (hio is not None):
            raise ValueError("max_hits= goes with params made with top_hits=True")
        if hio is not None and read_offsets is None:
            raise ValueError("max_hits needs read_offsets")
        sio = hio.sam if hio is not None else (capi.BatchIOSam() if (self.params.flags & capi.FLAG_SAM_FIELDS) else None)
        if mates is not None:
            if read_offsets is None:
                raise ValueError("mates needs read_offsets")
            mio = capi.BatchIOMates() if sio is None else sio.mates
            rio = mio.groups
            mio.min_span, mio.max_span, mio.unpaired_penalty = (int(x) for x in mates)
        else:
            mio = None
            rio = sio.mates.groups if sio is not None else (capi.BatchIOGroups() if read_offsets is not None else capi.BatchIORef())
        io = rio.base
        out = {}
        if read_offsets is not None:
            ro = np.ascontiguousarray(read_offsets, dtype=np.uint32)
            rio.n_reads, rio.read_offsets = len(ro) - 1, ro.ctypes.data
            out["best"] = np.zeros(len(ro) - 1, dtype=capi.BEST_DTYPE)
            rio.best = out["best"].ctypes.data
            n_out = len(ro) - 1
            if mio is not None:
                out["mates"] = np.zeros(n_out // 2, dtype=capi.MATE_DTYPE)
                mio.mates = out["mates"].ctypes.data
            if hio is not None:
                ho = hits_offsets(ro, max_hits) if hit_offsets is None else np.ascontiguousarray(hit_offsets, dtype=np.uint32)
                n_out = int(hits_offsets(ro, max_hits)[-1]) if len(ro) > 1 else 0     # (a wrong hit_offsets is the library's to refuse)
                out["hit_offsets"] = ho
                out["hit_pair"] = np.zeros(n_out, dtype=np.uint32)
                hio.max_hits, hio.hit_offsets, hio.hit_pair = int(max_hits), ho.ctypes.data, out["hit_pair"].ctypes.data
        else:
            ro, n_out = None, n
        io.n_pairs = n
        keep = [req, ro]
        io.requests = req.ctypes.data
        if text_pos is not None:
            tp = np.ascontiguousarray(text_pos, dtype=np.uint64)
            keep.append(tp)
            rio.text_pos = tp.ctypes.data
        addr = lambda x: None if x is None else x.ctypes.data
        if packed is not None:
            pp, pt, raw, rawp, rawt = [None if x is None else np.ascontiguousarray(x) for x in packed]
            keep += [pp, pt, raw, rawp, rawt]
            io.packed_patterns, io.packed_texts = addr(pp), addr(pt)
            io.n_raw = len(raw)
            if len(raw):
                io.raw_pairs, io.raw_patterns, io.raw_texts = addr(raw), addr(rawp), addr(rawt)
        else:
            pat = np.ascontiguousarray(pat)
            txt = None if txt is None else np.ascontiguousarray(txt)
            keep += [pat, txt]
            io.patterns, io.texts = addr(pat), addr(txt)
        if cigar_runs_cap:
            out["cig"] = np.zeros(n_out, dtype=capi.CIGAR_DTYPE)
            out["runs"] = np.zeros(cigar_runs_cap, dtype=np.uint32)
            io.cigars, io.runs, io.runs_cap = out["cig"].ctypes.data, out["runs"].ctypes.data, cigar_runs_cap
        if sam is not None:
            if sio is None:
                raise ValueError("sam= needs params made with sam=True")
            ccap, mcap, opts = (int(x) for x in sam)
            out["sam"] = np.zeros(n_out, dtype=capi.SAM_DTYPE)
            out["sam_cigar"] = np.zeros(max(ccap, 1), dtype=np.uint32)
            out["sam_md"] = np.zeros(max(mcap, 1), dtype=np.uint8)
            sio.sam, sio.sam_cigar, sio.sam_md = out["sam"].ctypes.data, out["sam_cigar"].ctypes.data, out["sam_md"].ctypes.data
            sio.sam_cigar_cap, sio.sam_md_cap, sio.sam_options = ccap, mcap, opts
        if want_res is None:
            want_res = not cigar_runs_cap or want_ops
        if want_res:
            out["res"] = np.zeros(n_out, dtype=RESULT8_DTYPE if (self.params.flags & FLAG_RES8) else RESULT_DTYPE)
            io.results = out["res"].ctypes.data
        if want_ops:
            out["ops"] = np.zeros((n_out, 2 * rs), dtype=np.uint8)
            io.ops = out["ops"].ctypes.data
        capi.check(self.lib.aim_set_submit(self.handle, device, slot, C.byref(io)))
        self._inflight[(device, slot)] = (hio if hio is not None else sio if sio is not None else (rio if mio is None else mio), keep, out)

    def wait(self, device, slot, check=True):
        io, keep, out = self._inflight.pop((device, slot), (None, None, {}))   # nothing in flight: the library reports AIM_ESTATE
        nr = C.c_uint32()
        rc = self.lib.aim_set_wait(self.handle, device, slot, C.byref(nr))
        if rc != capi.AIM_EALIGN or check:
            capi.check(rc)
        if "runs" in out:
            out["runs"] = out["runs"][: nr.value]
        return out

    def push(self, device, req, pat, txt=None, text_pos=None):
        """aim_set_push, or aim_set_push_ref when text_pos is given (AIM_FLAG_REF_TEXTS: the texts are windows of the reference)."""
        if (self.params.flags & FLAG_REQ8) and req.dtype != REQUEST8_DTYPE:
            req = to_request8(req)
        req = np.ascontiguousarray(req)
        pat = np.ascontiguousarray(pat)
        self._keep = getattr(self, "_keep", {})
        if text_pos is not None:
            tp = np.ascontiguousarray(text_pos, dtype=np.uint64)
            self._keep[device] = (req, pat, tp)   # host buffers must outlive the async copies
            capi.check(self.lib.aim_set_push_ref(self.handle, device, len(req), capi.ptr(req), capi.ptr(pat), capi.ptr(tp)))
        else:
            txt = np.ascontiguousarray(txt)
            self._keep[device] = (req, pat, txt)   # host buffers must outlive the async copies
            capi.check(self.lib.aim_set_push(self.handle, device, len(req), capi.ptr(req), capi.ptr(pat), capi.ptr(txt)))
        self._n = getattr(self, "_n", {})
        self._n[device] = len(req)

    def launch(self):
        capi.check(self.lib.aim_set_launch(self.handle))

    def pull(self, device, check=True):
        n = self._n[device]
        rs = self.params.read_size
        res = np.zeros(n, dtype=RESULT8_DTYPE if (self.params.flags & FLAG_RES8) else RESULT_DTYPE)
        ops = np.zeros((n, 2 * rs), dtype=np.uint8) if (self.params.flags & FLAG_BACKTRACE) else None
        rc = self.lib.aim_set_pull(self.handle, device, capi.ptr(res), capi.ptr(ops))
        if rc != capi.AIM_EALIGN or check:
            capi.check(rc)
        return res, ops

    def fallback_pairs(self, device=0):
        n = C.c_uint32()
        capi.check(self.lib.aim_set_fallback_pairs(self.handle, device, C.byref(n)))
        return n.value

    def plan_describe(self, device=0):
        """The plan line of the last launch on `device` (aim_set_plan_describe)."""
        buf = C.create_string_buffer(1024)
        capi.check(self.lib.aim_set_plan_describe(self.handle, device, buf, len(buf)))
        return buf.value.decode()

    def timers(self):
        a, b, c = C.c_float(), C.c_float(), C.c_float()
        capi.check(self.lib.aim_set_timers(self.handle, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def align(self, params, req, pat, txt, check=True, reference=None, text_pos=None):
        """Whole batch over all devices of the set: contiguous blocks (host.c:191-209), results in input order. With text_pos
        (params carry AIM_FLAG_REF_TEXTS) the texts are windows of `reference` (uploaded here when given, else the set's) and txt
        is not read."""
        n = len(req)
        per = max(1, math.ceil(n / self.nr_devices))
        if self.params is None or bytes(self.params) != bytes(params) or per > self.max_pairs:   # (EndsFreeParams: the extension too)
            self.configure(params, per)
        if reference is not None:
            self.set_reference(reference)
        blocks = []
        for d in range(self.nr_devices):
            lo, hi = min(n, d * per), min(n, (d + 1) * per)
            blocks.append((lo, hi))
            if text_pos is not None:
                self.push(d, req[lo:hi], pat[lo:hi], text_pos=text_pos[lo:hi])
            else:
                self.push(d, req[lo:hi], pat[lo:hi], txt[lo:hi])
        self.launch()
        parts = [self.pull(d, check=check) for d in range(self.nr_devices)]
        res = np.concatenate([p[0] for p in parts])
        ops = np.concatenate([p[1] for p in parts]) if parts[0][1] is not None else None
        return res, ops


def align(params, req, pat, txt, nr_devices=1, check=True, reference=None, text_pos=None):
    """One batch on a fresh set. reference + text_pos: the texts are windows of `reference` (params need AIM_FLAG_REF_TEXTS;
    txt may be None)."""
    with DeviceSet(nr_devices) as s:
        return s.align(params, req, pat, txt, check=check, reference=reference, text_pos=text_pos)
