"""SWG with a match bonus (match < 0): the int64 model of the reference recurrence, the table of kernel shapes the bonus is run on,
and the workers both match-bonus test modules use. Plain numpy; the library is only asked for plans and (by the callers) for
alignments. No device.

validate_params admits match <= 0 for SWG, as the reference launchers' -m does, and no reference digest uses it. With a bonus a
score is negative on most pairs (an identical pair scores match * READ_SIZE, the most negative value a cell can take), the register
kernel refuses the batch, and two int16 admission rules (dp_strip_exact_ok, dp_wave_exact_ok) depend on match * READ_SIZE. The
batches are full_rows.row_batch's: IDENTICAL, the twins, A_VS_C, the empty sequences and N_LAST are all there."""
import numpy as np

import full_rows as F

COSTS_A = (-1, 3, 4, 1)          # (match, mismatch, gap_o, gap_e)
COSTS_B = (-2, 5, 2, 3)
COSTS_EDGE = (-30, 3, 4, 1)      # match * READ_SIZE reaches the int16 admission rules' -32000 near READ_SIZE 1064


def _launcher(rs):
    return F.launcher_score(rs, 0.05, 5)


def model_max_score(costs):
    """A MAX_SCORE the border's "infinity" never wins with: above a gap of READ_SIZE + 2 bases plus READ_SIZE mismatches."""
    m, x, o, e = costs
    return lambda rs: 2 * o + (rs + 2) * e + x * rs


def _fam(costs, ms, w16=True, backtrace=False):
    return dict(costs=costs, ms=ms, w16=w16, backtrace=backtrace)


FAMILIES = {
    "a16": _fam(COSTS_A, _launcher), "a16_bt": _fam(COSTS_A, _launcher, backtrace=True),
    "b16": _fam(COSTS_B, _launcher), "b16_bt": _fam(COSTS_B, _launcher, backtrace=True),
    "edge": _fam(COSTS_EDGE, lambda rs: 300), "edge_bt": _fam(COSTS_EDGE, lambda rs: 300, backtrace=True),
    "a8_bt": _fam(COSTS_A, lambda rs: 100, w16=False, backtrace=True),      # MAX_SCORE 100 < 127: int8 cells, which wrap by design
    "a_model_bt": _fam(COSTS_A, model_max_score(COSTS_A), backtrace=True),
    "b_model_bt": _fam(COSTS_B, model_max_score(COSTS_B), backtrace=True),
}

_L = "swg_lane_kernel"
_G = F._G
_S = F._S
_DW = "dp_wave_kernel wavefronts_per_pair=%d"
# dp_group's line does not name its fallback kernel; its shape does: up to READ_SIZE 320 the to-do list goes to swg_lane_kernel (blocks
# of 64 threads, 64 pairs' rows in LDS: fb_lds is swg_lane's own lds at that READ_SIZE), from 328 on to dp_strip_kernel (a block per pair).
_FB_LANE, _FB_STRIP = " fb_block=64 fb_lds=82176", " fb_grid=136 fb_block=64 fb_lds=11296"
_SCORE = [(40, _L), (136, _L + " seq_lds=0"), (184, _G % 6), (320, _G % 8 + _FB_LANE), (328, _G % 9 + _FB_STRIP), (1024, _G % 32), (1544, _S % 2),
          (2568, _S % 3)]
_CIGAR = [(40, _L), (136, _L + " seq_lds=1"), (184, _G % 6), (320, _G % 10 + _FB_LANE), (328, _G % 11 + _FB_STRIP), (1024, _G % 32), (1032, _S % 1),
          (1288, _S % 2), (1544, _G % 49), (2568, _S % 3)]
_EDGE = [(1024, _G % 32), (1032, _DW % 2), (1064, _DW % 2), (1072, _DW % 2), (1096, _DW % 2)]
# family -> [(READ_SIZE, kernel name and shape tokens of aim_plan_describe at pairs_for(READ_SIZE) pairs, 16 GB, 256 CUs)], as in
# full_rows.TABLE; tests/test_match_bonus_cpu.py checks every entry against the planner.
TABLE = {
    "a16": _SCORE, "a16_bt": _CIGAR, "b16": _SCORE, "b16_bt": _CIGAR,
    "edge": _EDGE, "edge_bt": _EDGE,
    "a8_bt": [(40, _L), (136, _L + " seq_lds=1"), (800, _L + " seq_lds=0"), (1192, _L + " seq_lds=0"), (1200, _DW % 2)],
    "a_model_bt": [(136, _L + " seq_lds=1"), (184, _G % 6), (1024, _G % 32)],
    "b_model_bt": [(136, _L + " seq_lds=1"), (184, _G % 6), (1024, _G % 32)],
}
ROWS = [(fam, rs) for fam, rows in TABLE.items() for rs, _ in rows]
MODEL_ROWS = [(fam, rs) for fam, rs in ROWS if fam.endswith("_model_bt")]
# Rows on which the reference's cells wrap (the model's minimum or maximum over the three planes leaves the cell type on at least
# one pair): the int8 rows from READ_SIZE 136 on (IDENTICAL reaches -136 < -128; at READ_SIZE 40 every cell still fits) and the edge
# rows at READ_SIZE 1096 (30 * 1096 = 32 880 > 32 768). On these rows the oracle alone is the reference; everywhere else the model
# is held to it too.
WRAPPING = [(fam, rs) for fam, rs in ROWS if (fam == "a8_bt" and rs >= 136) or (fam.startswith("edge") and rs == 1096)]
FITTING = [r for r in ROWS if r not in WRAPPING]
SEED = F.SEED

# The two int16 admission rules (aim_capi.hip), restated: the lowest value a cell or a packed intermediate can take stays above
# -32000. The plan line does not say whether dp_wave runs its row scan or its literal path, so the literal edge is pinned here.
INT16_FLOOR = -32000


def dp_strip_exact_lo(costs, rs):
    m, x, o, e = costs
    return m * rs - (rs + 2) * e - 4 * (o + e)


def dp_wave_exact_lo(costs, rs):
    return costs[0] * rs


def expected_plan(fam, rs):
    return dict(TABLE[fam])[rs]


def row_params(fam, rs, **kw):
    from aim_amd import engine
    f = FAMILIES[fam]
    m, x, o, e = f["costs"]
    kw.setdefault("backtrace", f["backtrace"])
    return engine.make_params("swg", f["ms"](rs), rs, match=m, mismatch=x, gap_o=o, gap_e=e, swg_w16=f["w16"], **kw)


def cell_range(fam):
    """(lowest, highest) value of the family's cell type."""
    return (-32768, 32767) if FAMILIES[fam]["w16"] or FAMILIES[fam]["ms"](0) >= 127 else (-128, 127)


# Pairs on the to-do list (aim_set_fallback_pairs) per row, as first measured on an MI355X; zero and noise padding give the same
# count. dp_group hands on the two pairs with an empty sequence (2 of 130, and 2 of 40 at READ_SIZE 1544), on every row that reaches
# it; swg_lane, dp_strip and dp_wave keep no list and reported 0 on every row.
_TODO_BY_KERNEL = {"dp_group_kernel": 2}
_TODO = {}          # (no row needed an entry of its own)


def expected_todo(fam, rs):
    if (fam, rs) in _TODO:
        return _TODO[(fam, rs)]
    return _TODO_BY_KERNEL.get(expected_plan(fam, rs).split()[0], 0)


# ------------------------------------------------------------------ the model
def swg_model(req, pat, txt, match, x, o, e, max_score, mutant=None):
    """(score, lowest, highest) per pair, int64: the recurrence of swg.c:121-171 with no cell type. Text along h, pattern along v;
    cell (h, v) holds M, I (from (h - 1, v)) and D (from (h, v - 1)); M(0, 0) = 0; row 0 has D = M = o + v * e, I = MAX_SCORE;
    column 0 has I = M = o + h * e, D = MAX_SCORE. MAX_SCORE in a border cell is the reference's infinity and takes part like any
    other value: 'A' * 136 against 'C' * 136 at MAX_SCORE 33 scores 169 (the border's 33 + 136 * 1), not 136 * 3 = 408. The score
    is M(tlen, plen), 0 when either sequence is empty (the loops write nothing). lowest / highest are taken over the three planes,
    borders included, so they say whether the reference's cells would have wrapped.

    Valid where plen <= tlen: with a longer pattern the reference's flat table (row stride tlen + 1) aliases and its score is no
    longer the recurrence's. All pairs advance one text base per step; along the pattern D(h, v) = v * e + min(MAX_SCORE,
    min_{k < v} (best(h, k) + o - k * e)) with best = min(diagonal, I) -- a deletion run never opens from a deletion while o >= 0.

    mutant: None, or one of the wrong kernels of the mutation checks -- "no_bonus" (match taken as 0), "bonus_on_mismatch" (the bonus
    also added where the bases differ), "head_without_bonus" (no bonus in the cells of row 1 and column 1, a kernel's head path)."""
    assert o >= 0 and mutant in (None, "no_bonus", "bonus_on_mismatch", "head_without_bonus")
    n, rs = pat.shape
    pl = np.asarray(req["pattern_len"], dtype=np.int64)
    tl = np.asarray(req["text_len"], dtype=np.int64)
    ms = int(max_score)
    v = np.arange(rs + 1, dtype=np.int64)
    ve = v * e
    inside = v[None, :] <= pl[:, None]
    m_eq, m_ne = (0, x) if mutant == "no_bonus" else ((match, x + match) if mutant == "bonus_on_mismatch" else (match, x))
    M = np.tile(o + ve, (n, 1))
    M[:, 0] = 0
    I = np.full((n, rs + 1), ms, dtype=np.int64)
    D = np.tile(o + ve, (n, 1))
    D[:, 0] = ms
    big, small = np.int64(1) << 60, -(np.int64(1) << 60)
    planes = np.stack([M, I, D])
    lo = np.where(inside, planes.min(axis=0), big).min(axis=1)
    hi = np.where(inside, planes.max(axis=0), small).max(axis=1)
    score = np.zeros(n, dtype=np.int64)
    p = pat.astype(np.int64)
    rows = np.arange(n)
    for h in range(1, int(tl.max()) + 1 if n else 0):
        eq = p == txt[:, h - 1:h].astype(np.int64)
        sub = np.where(eq, m_eq, m_ne)
        if mutant == "head_without_bonus":
            if h == 1:
                sub = np.where(eq, 0, m_ne)
            else:
                sub[:, 0] = np.where(eq[:, 0], 0, m_ne)
        I = np.minimum(M + (o + e), I + e)
        I[:, 0] = o + h * e
        best = np.empty_like(M)
        best[:, 0] = o + h * e
        best[:, 1:] = np.minimum(M[:, :-1] + sub, I[:, 1:])
        acc = np.minimum.accumulate(best + o - ve, axis=1)
        D = np.empty_like(M)
        D[:, 0] = ms
        D[:, 1:] = np.minimum(acc[:, :-1], ms) + ve[1:]
        M = np.minimum(best, D)
        M[:, 0] = o + h * e
        live = inside & (h <= tl)[:, None]
        lo = np.minimum(lo, np.where(live, np.minimum(M, np.minimum(I, D)), big).min(axis=1))
        hi = np.maximum(hi, np.where(live, np.maximum(M, np.maximum(I, D)), small).max(axis=1))
        last = (tl == h) & (pl > 0)
        score[last] = M[rows[last], pl[last]]
    return score, lo, hi


def rescore(ops, match, x, o, e):
    """Cost of an op string: match per 'M', x per 'X', o + e * length per run of 'I' or of 'D'."""
    from endsfree_model import runs_of
    return sum(match * k if c == "M" else (x * k if c == "X" else o + e * k) for c, k in runs_of(ops))


def unaliased(req):
    """The pairs the model is valid on."""
    return np.nonzero(req["pattern_len"] <= req["text_len"])[0]


_MODEL = {}


def model_row(fam, rs):
    """(pairs, score, lowest, highest) of swg_model on the unaliased pairs of a row's batch; computed once per (costs, MAX_SCORE,
    READ_SIZE) and never changed afterwards."""
    f = FAMILIES[fam]
    key = (f["costs"], f["ms"](rs), rs)
    if key not in _MODEL:
        req, pat, txt = F.row_batch(rs, "zero")
        sel = unaliased(req)
        out = (sel,) + swg_model(req[sel], pat[sel], txt[sel], *f["costs"], f["ms"](rs))
        for a in out:
            a.flags.writeable = False
        _MODEL[key] = out
    return _MODEL[key]


# ------------------------------------------------------------------ the oracle
_ORACLE = {}


def oracle_of(params, req, pat, txt, algo="swg"):
    from oracle import oracle
    return oracle.align_batch(F.oracle_params(params, algo), req["pattern_len"], req["text_len"], pat, txt, nthreads=8)


def oracle_row(fam, rs, pad="zero"):
    """(results, ops) of the oracle on a row's batch; computed once per session and never changed afterwards."""
    key = (fam, rs, pad)
    if key not in _ORACLE:
        req, pat, txt = F.row_batch(rs, pad)
        res, ops, _ = oracle_of(row_params(fam, rs), req, pat, txt)
        res.flags.writeable = False
        if ops is not None:
            ops.flags.writeable = False
        _ORACLE[key] = (res, ops)
    return _ORACLE[key]


# ------------------------------------------------------------------ candidates of both signs for the selection flags
SEL_LENGTH, SEL_RS = 100, 112


def selection_params(**kw):
    """SWG, int16 cells, COSTS_A at READ_SIZE 112 with a MAX_SCORE no border wins with; `kw` as engine.make_params takes it."""
    from aim_amd import engine
    return engine.make_params("swg", model_max_score(COSTS_A)(SEL_RS), SEL_RS, **selection_kw(**kw))


def selection_kw(**kw):
    m, x, o, e = COSTS_A
    return dict(dict(match=m, mismatch=x, gap_o=o, gap_e=e, swg_w16=True), **kw)


def selection_batch(seed=20263, n_read_pairs=150):
    """(reference, requests, read_rows, read_offsets, text_pos, texts, patterns, kinds) in engine.mate_pairs' layout: paired-end
    reads of 100 bases at 2 % edits with 6, 7 or 8 candidate windows each. From engine.mate_pairs (shift 3) come the true window
    (about -90 at COSTS_A), in 40 % of the read pairs an exact repeat of one mate's window (a tie at that negative score), copies
    of the true window moved by 1..3 bases (less negative: two gaps) and random windows (positive). Added here: every fifth read
    gets a duplicate of its true window in the place of a decoy (a tie whatever the repeat case drew), every seventh read loses
    every related candidate (all its scores are positive). The true window is kept when a read is cut to 6 or 7 candidates.
    kinds[r]: 0 plain, 1 duplicate added, 2 no related candidate."""
    from aim_amd import engine
    k = 8
    ref, req, rows, offs, tpos, _, _, truth = engine.mate_pairs(seed, n_read_pairs, SEL_LENGTH, 0.02, 400, k, 0.4, read_size=SEL_RS, shift=3)
    rng = np.random.default_rng([seed, 0x73656C])
    n_reads = 2 * n_read_pairs
    span = len(ref) - SEL_LENGTH + 1
    kinds = np.zeros(n_reads, dtype=np.int64)
    keep, counts = [], []
    for r in range(n_reads):
        lo = r * k
        cand = [int(x) for x in tpos[lo:lo + k]]
        true = int(truth["true"][r // 2, r & 1]) - lo
        cnt = 6 + r % 3
        cand[0], cand[true] = cand[true], cand[0]                # the true window first, then cut, then a seeded order
        if r % 7 == 3:
            kinds[r] = 2
            cand = [int(rng.integers(0, span)) | (int(rng.integers(0, 2)) << 63) for _ in range(k)]
        elif r % 5 == 1:
            kinds[r] = 1
            cand[1] = cand[0]
        cand = cand[:cnt]
        keep += [cand[i] for i in rng.permutation(cnt)]
        counts.append(cnt)
    tpos = np.array(keep, dtype=np.uint64)
    offs = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    n = len(tpos)
    read_of = np.repeat(np.arange(n_reads), counts)
    out = np.zeros(n, dtype=req.dtype)
    out["pattern_len"] = req["pattern_len"][read_of * k]
    out["text_len"] = SEL_LENGTH
    out["idx"] = np.arange(n, dtype=np.uint32)
    txt = np.zeros((n, SEL_RS), dtype=np.uint8)
    for c in range(n):
        tp = int(tpos[c])
        txt[c, :SEL_LENGTH] = engine.ref_window(ref, tp & ((1 << 63) - 1), SEL_LENGTH, bool(tp >> 63))
    return ref, out, rows, offs, tpos, txt, np.ascontiguousarray(rows[read_of]), kinds


# ------------------------------------------------------------------ workers (their own process: knobs are environment variables)
def plan_lines():
    """{"family/READ_SIZE": aim_plan_describe's line} for every table row, and "reg/READ_SIZE" for the short rows with match = 0
    and with every bonus (the register kernel takes the first and refuses the others)."""
    from aim_amd import engine
    out = {"%s/%d" % (fam, rs): F.plan_line(row_params(fam, rs), F.pairs_for(rs)) for fam, rs in ROWS}
    for rs in (40, 136):
        for m in (0, -1, -2, -30):
            for bt in (False, True):
                p = engine.make_params("swg", _launcher(rs), rs, match=m, swg_w16=True, backtrace=bt)
                out["reg/%d/%d/%d" % (rs, m, bt)] = F.plan_line(p, F.pairs_for(rs))
    return out


def align_row(fam, rs, pad="zero"):
    """(results, ops, plan line, fallback pairs) of a row's batch on the device."""
    from aim_amd import engine
    req, pat, txt = F.row_batch(rs, pad)
    with engine.DeviceSet(1) as s:
        s.configure(row_params(fam, rs), len(req))
        s.push(0, req, pat, txt)
        s.launch()
        res, ops = s.pull(0, check=False)
        return res, ops, s.plan_describe(0), s.fallback_pairs(0)


if __name__ == "__main__":
    import json
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    if sys.argv[1] == "--plans":
        json.dump(plan_lines(), sys.stdout)
    elif sys.argv[1] == "--align":       # --align OUT.npz family/READ_SIZE ...: zero-padded rows, results, ops inside [begin, end), plan
        out = {}
        for key in sys.argv[3:]:
            fam, rs = key.split("/")
            res, ops, line, _ = align_row(fam, int(rs))
            out[key + "/res"] = res
            out[key + "/plan"] = np.frombuffer(line.encode(), dtype=np.uint8)
            if ops is not None:
                col = np.arange(ops.shape[1])[None, :]
                inside = (col >= res["begin_offset"][:, None]) & (col < res["end_offset"][:, None])
                out[key + "/ops"] = np.where(inside, ops, 0)
        np.savez(sys.argv[2], **out)
