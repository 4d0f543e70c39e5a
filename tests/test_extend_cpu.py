"""Segment extension without a GPU: rule 11c as tests/extend_model.py writes it down. The cost transformation against an independent
maximising gap-affine DP, the stop rule and the ties on hand-made pairs, part 2 by hand, what the model gives on the chimeric reads
(figures in that test's docstring), the end-to-end bound on the ENDSFREE model, what the directed batch of the GPU tests holds, the ABI
values, symbols and struct layouts, every refusal of aim_extend_segments_device by message and in order, and the code objects."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aim_hip.h")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from extend_model import inner_gaps  # noqa: E402

NEVER = 1 << 20                         # an x-drop no pair here can reach


def _lib():
    from aim_amd import capi
    return capi.load()


def _err():
    return _lib().aim_last_error().decode()


def _define(name):
    m = re.search(r"#define\s+%s\s+(\S+)" % name, open(HEADER).read())
    return int(m.group(1).rstrip("uUlL"), 0)


def _b(s):
    return np.frombuffer(s.encode(), dtype=np.uint8)


# ---- the transformation ----------------------------------------------------------------------------------------------------------
def best_prefix_score(q, t, a, x, o, e, band):
    """The maximising form, written on its own: match +a, mismatch -x, a gap of g bases -(o + g e), over cells with |h - v| <= band;
    returns the greatest score of any prefix pair (0 for the empty one)."""
    NEG = -(1 << 40)
    n, m = len(q), len(t)
    H = [[NEG] * (m + 1) for _ in range(n + 1)]       # best score ending anyhow
    E = [[NEG] * (m + 1) for _ in range(n + 1)]       # ending in a gap that consumes t
    F = [[NEG] * (m + 1) for _ in range(n + 1)]       # ending in a gap that consumes q
    H[0][0] = 0
    best = 0
    for v in range(n + 1):
        for h in range(m + 1):
            if abs(h - v) > band or (v == 0 and h == 0):
                continue
            if h > 0 and abs(h - 1 - v) <= band:
                E[v][h] = max(H[v][h - 1] - o - e, E[v][h - 1] - e)
            if v > 0 and abs(h - v + 1) <= band:
                F[v][h] = max(H[v - 1][h] - o - e, F[v - 1][h] - e)
            d = NEG
            if v > 0 and h > 0:
                d = H[v - 1][h - 1] + (a if q[v - 1] == t[h - 1] else -x)
            H[v][h] = max(d, E[v][h], F[v][h])
            best = max(best, H[v][h])
    return best


PENALTY_SETS = [(1, 3, 4, 1), (2, 30, 0, 1), (2, 6, 4, 2), (1, 1, 0, 1), (3, 5, 10, 4)]      # (2, 30, 0, 1): x' = 64, the ring bound


@pytest.mark.parametrize("pen", PENALTY_SETS, ids=lambda p: "a%d-x%d-o%d-e%d" % p)
def test_score_is_the_maximising_dp(pen):
    import extend_model as em
    a, x, o, e = pen
    assert max(em.units(em.Params(a, x, o, e, 0, 1, 1, 8))[0], 2 * o + 2 * e + a) <= em.MAX_UNIT
    rng = np.random.default_rng([7, a, x, o, e])
    pairs = [(_b("A"), _b("A")), (_b("A"), _b("C")), (_b("ACGTACGT"), _b("ACGTACGT")), (_b("AAAAAAAA"), _b("CCCCCCCC")), (_b("ACGTACGTAC"), _b("A")),
             (_b("A"), _b("ACGTACGTAC")), (_b("ACGTTTACGTAC"), _b("ACGACGTAC")), (_b("NNNNacgt"), _b("NNNNACGT"))]
    for _ in range(60):
        n = int(rng.integers(1, 22))
        q = rng.integers(0, 3, size=n).astype(np.uint8)
        t = list(q)
        for _ in range(int(rng.integers(0, 4))):
            at = int(rng.integers(0, len(t) + 1))
            kind = int(rng.integers(0, 3))
            if kind == 0 and at < len(t):
                t[at] = (t[at] + 1) % 3
            elif kind == 1:
                t[at:at] = [int(c) for c in rng.integers(0, 3, size=int(rng.integers(1, 4)))]
            else:
                del t[at:at + int(rng.integers(1, 4))]
        t = (t + [int(c) for c in rng.integers(0, 3, size=int(rng.integers(0, 6)))]) or [0]
        pairs.append((q, np.array(t, dtype=np.uint8)))
    sides, want = [], []
    for band in (2, 31):
        p = em.Params(a, x, o, e, NEVER, em.MAX_COST, band, 64)
        for q, t in pairs:
            t = t[:len(q) + band]                                  # rule 11c's m <= n + band
            dq, dr, score, stop = em.extend_side(p, q, t)
            assert stop == em.MAX_COST
            assert score == best_prefix_score(list(q), list(t), a, x, o, e, band), (pen, band, bytes(q), bytes(t))
            sides.append((q, t))
            want.append((dq, dr, score, stop))
        assert em.extend_sides(p, sides[-len(pairs):]) == want[-len(pairs):]             # batched or one by one: the same


# ---- the stop rule and the ties --------------------------------------------------------------------------------------------------
def _costs(p, q, t):
    import extend_model as em
    return em.band_costs(p, q[None, :], t[None, :], np.array([len(q)]), np.array([len(t)]))[0]


def test_stop_rule_by_hand():
    import extend_model as em
    # Z = 0: level 1 fires whatever the pair (a R - 1 < B), and the result is the exact run
    p = em.Params(1, 3, 4, 1, 0, 400, 31, 64)
    assert em.extend_side(p, _b("ACGTAAAA"), _b("ACGTCCCC")) == (4, 4, 4, 1)
    # a stop at a level no cell has: after 4 + 4 matched bases everything mismatches; with Z = 2 the test a R - s < B - 4 fires at
    # s = 5, and the costs that occur are 0, 8, 11, 14, ...
    p = em.Params(1, 3, 4, 1, 2, 400, 31, 64)
    q, t = _b("ACGTAAAAAAAA"), _b("ACGTCCCCCCCC")
    D = _costs(p, q, t)
    assert not (D == 5).any() and sorted(set(D[D < 12].tolist())) == [0, 8, 11]
    assert em.extend_side(p, q, t) == (4, 4, 4, 5)
    # the same pair with Z out of reach stops by max_cost, at 7 (below the first edit) and at 9 (above it): the result does not move
    assert em.extend_side(p._replace(xdrop=NEVER, max_cost=7), q, t) == (4, 4, 4, 7)
    assert em.extend_side(p._replace(xdrop=NEVER, max_cost=9), q, t) == (4, 4, 4, 9)
    # the x-drop lets a mismatch through when the matches behind it pay for it within Z: 4 matches, a mismatch, 6 matches
    q, t = _b("ACGTAGGTTCA"), _b("ACGTCGGTTCA")
    assert em.extend_side(p._replace(xdrop=1), q, t)[:2] == (4, 4)               # s = 3 fires before cost 8 is seen
    assert em.extend_side(p._replace(xdrop=4), q, t)[:3] == (11, 11, 7)         # (a * 22 - 8) / 2
    # nothing positive: (0, 0) with score 0, and stop is still reported
    assert em.extend_side(p, _b("AAAA"), _b("CCCC")) == (0, 0, 0, 5)
    # an empty side is not run
    assert em.extend_side(p, _b(""), _b("ACGT")) == (0, 0, 0, 0) and em.extend_side(p, _b("ACGT"), _b("")) == (0, 0, 0, 0)
    # gcd 2 ((2, 6, 4, 2): x' = 16, o' + e' = 14, e' = 6): the test fires at an odd level between two levels that exist
    p = em.Params(2, 6, 4, 2, 2, 400, 31, 64)
    q, t = _b("ACGTAAAAAAAA"), _b("ACGTCCCCCCCC")
    assert (_costs(p, q, t) % 2 == 0).all()
    assert em.extend_side(p, q, t) == (4, 4, 8, 5)


def test_ties_by_hand_and_by_search():
    import extend_model as em
    p = em.Params(1, 3, 4, 1, NEVER, em.MAX_COST, 31, 64)
    # 20 matches, a mismatch, 3 matches: a (v + h) - D is 40 at (20, 20) with D = 0 and 48 - 8 = 40 at (24, 24): the smallest D wins
    q, t = _b("A" * 20 + "C" + "GGG"), _b("A" * 20 + "T" + "GGG")
    assert em.extend_side(p, q, t) == (20, 20, 20, em.MAX_COST)
    # one more match behind the mismatch and the longer one wins
    assert em.extend_side(p, _b("A" * 20 + "C" + "GGGG"), _b("A" * 20 + "T" + "GGGG"))[:3] == (25, 25, 21)
    # the same cost on two diagonals: dropping the read's C (h - v = -1) or the reference's A (h - v = +1) -> the smallest h - v
    q, t = _b("G" * 10 + "CA" * 6), _b("G" * 10 + "AC" * 6)
    assert em.extend_side(p, q, t) == (22, 21, 16, em.MAX_COST)                  # (43 - 11) / 2
    # by search: pairs over two letters, every cell by plain loops
    rng = np.random.default_rng(11)
    seen = dict(cost=0, diagonal=0)
    for _ in range(400):
        n = int(rng.integers(2, 12))
        q, t = rng.integers(0, 2, size=n).astype(np.uint8), rng.integers(0, 2, size=int(rng.integers(1, n + 4))).astype(np.uint8)
        pp = p._replace(mismatch=1, gap_o=0, band=3, xdrop=int(rng.integers(0, 12)))       # cheap edits: many cells tie
        t = t[:n + 3]
        D = _costs(pp, q, t)
        dq, dr, score, stop = em.extend_side(pp, q, t)
        cells = [(-(v + v + j - 3 - int(D[v, j])), int(D[v, j]), j - 3, v) for v in range(n + 1) for j in range(7) if D[v, j] <= stop]
        top = min(cells)
        if top[0] >= 0:
            assert (dq, dr, score) == (0, 0, 0)
            continue
        assert (dq, dr, 2 * score) == (top[3], top[3] + top[2], -top[0]), (bytes(q), bytes(t))
        equal = [c for c in cells if c[0] == top[0]]
        seen["cost"] += len({c[1] for c in equal}) > 1
        seen["diagonal"] += len([c for c in equal if c[1] == top[1]]) > 1
    assert seen["cost"] >= 5 and seen["diagonal"] >= 5, seen


# ---- part 2 by hand --------------------------------------------------------------------------------------------------------------
RS, REF_LEN = 104, 4000


def _hand_ref():
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(3).integers(0, 4, size=REF_LEN)].copy()


def _other(c):
    return np.frombuffer(b"CGTA", dtype=np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), c)]


def _hand_read(ref, lo, hi, minus, lead=30, trail=30, L=100):
    """A read row whose bases [lead, L - trail) are ref[lo, hi) (reverse-complemented when minus) and whose other bases mismatch the
    reference's continuation, base by base."""
    import extend_model as em
    assert hi - lo == L - lead - trail
    ext = np.concatenate([_other(ref[lo - lead:lo]), ref[lo:hi], _other(ref[hi:hi + trail])])
    if minus:
        ext = em.COMP[ext][::-1]
    row = np.zeros(RS, dtype=np.uint8)
    row[:L] = ext
    return row


def _run(p, rows, L, slots, ref, read_size=RS):
    """The model over one read of len(slots) slots: (q_begin, q_end, start, text_len, minus, flags) each."""
    import extend_model as em
    import seed_model as m
    import split_model as sm
    K = len(slots)
    req, tp, pat, seg = np.zeros(K, dtype=m.REQUEST), np.zeros(K, dtype=np.uint64), np.zeros((K, read_size), dtype=np.uint8), np.zeros(K, dtype=sm.SEGMENT)
    for i, (qb, qe, start, tl, minus, fl) in enumerate(slots):
        req[i] = (qe - qb, tl, 0, 900 + i)
        tp[i] = np.uint64(start | (minus << 63))
        pat[i, :qe - qb] = rows[qb:qe]
        seg[i] = (qb, qe, L, fl, i)
    return em.extend_segments(p, K, read_size, len(ref), np.array([L], dtype=np.int32), rows[None, :], ref, req, tp, pat, seg), (req, tp, pat, seg)


@pytest.mark.parametrize("minus", (0, 1))
def test_apply_all_four_side_and_strand_cases(minus):
    """The read holds ref[1000, 1040); the chain stopped 6 bases short of the read's left end of it and 9 short of the right one. A
    segment closed on the left gets 6 bases back, one closed on the right 9, and the window grows on the side rule 11c names."""
    import extend_model as em
    import split_model as sm
    ref = _hand_ref()
    p = em.Params(1, 3, 4, 1, 20, 400, 31, 64)
    row = _hand_read(ref, 1000, 1040, minus)
    lo_gap, hi_gap = (9, 6) if minus else (6, 9)                # the gaps at the low and the high end of the reference interval
    start, tl = 1000 + lo_gap, 40 - lo_gap - hi_gap
    closed_left = (36, 61, start, tl, minus, sm.VALID | sm.RIGHT_OPEN)
    closed_right = (36, 61, start, tl, minus, sm.VALID | sm.SUPPLEMENTARY | sm.LEFT_OPEN)
    both = (36, 61, start, tl, minus, sm.VALID)
    ((req, tp, pat, seg), ext), before = _run(p, row, 100, [closed_left, closed_right, both], ref)
    assert ext["dq"].tolist() == [[6, 0], [0, 9], [6, 9]] and ext["dr"].tolist() == [[6, 0], [0, 9], [6, 9]] and ext["score"].tolist() == [[6, 0], [0, 9], [6, 9]]
    assert (ext["pad"] == 0).all() and ext["stop"][0][1] == 0 and ext["stop"][0][0] > 0
    # left: q_begin moves down; the reference bound is the low one on the plus strand and the high one on the minus strand
    assert tuple(seg[0])[:2] == (30, 61) and seg[0]["flags"] == sm.VALID | sm.RIGHT_OPEN | em.EXT_LEFT
    assert (int(tp[0]) & (sm.MINUS - 1), int(req["text_len"][0])) == ((start, tl + 6) if minus else (start - 6, tl + 6))
    assert tuple(seg[1])[:2] == (36, 70) and seg[1]["flags"] == sm.VALID | sm.SUPPLEMENTARY | sm.LEFT_OPEN | em.EXT_RIGHT
    assert (int(tp[1]) & (sm.MINUS - 1), int(req["text_len"][1])) == ((start - 9, tl + 9) if minus else (start, tl + 9))
    assert tuple(seg[2])[:2] == (30, 70) and seg[2]["flags"] == sm.VALID | em.EXT_LEFT | em.EXT_RIGHT
    assert (int(tp[2]) & (sm.MINUS - 1), int(req["text_len"][2])) == (1000, 40)
    for i in range(3):
        qb, qe = int(seg[i]["q_begin"]), int(seg[i]["q_end"])
        assert int(tp[i]) >> 63 == minus and int(req["pattern_len"][i]) == qe - qb and int(req["idx"][i]) == 900 + i and int(req["padding"][i]) == 0
        assert pat[i, :qe - qb].tobytes() == row[qb:qe].tobytes() and not pat[i, qe - qb:].any()
        assert (seg[i]["read_len"], seg[i]["cand"]) == (100, i)


def test_budget_edges_loose_and_open():
    import extend_model as em
    import split_model as sm
    ref = _hand_ref()
    p = em.Params(1, 3, 4, 1, 20, 400, 31, 64)
    row = _hand_read(ref, 1000, 1040, 0)
    # the read_size budget: text_len may grow to read_size and no further -- one inner side takes all of it, two share it
    for tl, fl, want in ((RS - 5, sm.VALID | sm.LEFT_OPEN, [[0, 0], [0, 5]]), (RS - 5, sm.VALID, [[2, 0], [0, 2]]), (RS, sm.VALID, [[0, 0], [0, 0]])):
        # (windows that end where the read's copy ends: the low bound lies far below, as a capped window's would)
        ((req, tp, pat, seg), ext), _ = _run(p, row, 100, [(36, 61, 1031 - tl, tl, 0, fl)], ref)
        left = _run(p, row, 100, [(36, 61, 1006, tl, 0, fl)], ref)[0][1]
        got = [[int(left["dr"][0][0]), 0], [0, int(ext["dr"][0][1])]]
        assert got == want, (tl, fl, got)
        assert int(req["text_len"][0]) <= RS
    # windows at reference position 0 and at ref_len: the side that would leave the reference has no room
    row0 = np.zeros(RS, dtype=np.uint8)
    row0[:100] = np.concatenate([_other(ref[:30]), ref[0:40], _other(ref[40:70])])     # the read's bases 30..70 are ref[0, 40)
    ((req, tp, pat, seg), ext), _ = _run(p, row0, 100, [(36, 61, 6, 25, 0, sm.VALID)], ref)
    assert ext["dq"].tolist() == [[6, 9]] and int(tp[0]) == 0 and int(req["text_len"][0]) == 40
    ((req, tp, pat, seg), ext), _ = _run(p, row0, 100, [(36, 61, 0, 31, 0, sm.VALID)], ref)     # seg_start 0: no room on the low side
    assert ext["dq"].tolist() == [[0, 9]] and ext["stop"].tolist()[0][0] == 0 and int(tp[0]) == 0
    rowN = np.zeros(RS, dtype=np.uint8)
    rowN[:100] = np.concatenate([_other(ref[REF_LEN - 70:REF_LEN - 40]), ref[REF_LEN - 40:], _other(ref[:30])])
    ((req, tp, pat, seg), ext), _ = _run(p, rowN, 100, [(36, 61, REF_LEN - 34, 25, 0, sm.VALID)], ref)
    assert ext["dq"].tolist() == [[6, 9]] and int(tp[0]) + int(req["text_len"][0]) == REF_LEN
    ((req, tp, pat, seg), ext), _ = _run(p, rowN, 100, [(36, 61, REF_LEN - 34, 34, 0, sm.VALID)], ref)  # seg_end == ref_len: no room up
    assert ext["dq"].tolist() == [[6, 0]] and int(tp[0]) + int(req["text_len"][0]) == REF_LEN
    # loose, open and invalid slots, and malformed records, keep every byte and get a zero aim_extend_t
    slots = [(36, 61, 1006, 25, 0, sm.VALID | sm.LOOSE), (36, 61, 1006, 25, 0, sm.VALID | sm.LEFT_OPEN | sm.RIGHT_OPEN), (36, 61, 1006, 25, 0, 0),
             (36, 101, 1006, 25, 0, sm.VALID), (36, 61, REF_LEN - 10, 25, 0, sm.VALID), (36, 61, 1006, RS + 1, 0, sm.VALID)]
    (after, ext), before = _run(p, row, 100, slots, ref)
    assert ext.tobytes() == bytes(24 * len(slots))
    for x, y in zip(after, before):
        assert x.tobytes() == y.tobytes()


# ---- the chimeric reads ----------------------------------------------------------------------------------------------------------
_CHIM = {}
CHIM_PARAMS = (1, 3, 4, 1, 20, 400, 31, 64)


def chimeric_model():
    """The chimeric reads through the chain, class, split and extend models: dict(rows, rl, halves, ref, K, flank, split, ext_out, ext)."""
    if not _CHIM:
        import chain_class_model as ccm
        import extend_model as em
        import seed_model as m
        import split_model as sm
        from pipeline_batches import model_chains
        ref = m.make_reference()
        rows, rl, halves = sm.chimeric(ref)
        k, stride, w, max_occ, band, flank, min_votes, K = ccm.CHIMERIC_ROW
        req, tpos, votes, seeds, chains = model_chains("chimeric", ccm.CHIMERIC_ROW, rows, rl, ccm.CHIMERIC_SIZE)
        cls = ccm.classify(K, ccm.CHIMERIC_SIZE, 128, rl, tpos, seeds, chains)
        split = sm.segments(K, ccm.CHIMERIC_SIZE, flank, len(ref), rl, rows, req, tpos, seeds, chains, cls)
        out, ext = em.extend_segments(em.Params(*CHIM_PARAMS), K, ccm.CHIMERIC_SIZE, len(ref), rl, rows, ref, *split)
        _CHIM.update(rows=rows, rl=rl, halves=halves, ref=ref, K=K, flank=flank, split=split, ext_out=out, ext=ext)
    return _CHIM


def test_chimeric_reads_recover_the_breakpoint():
    """The committed model on split_model.chimeric (32 reads, two halves of 400 bases with 12 edits each) with (a, x, o, e) = (1, 3, 4, 1),
    Z = 20, band 31, max_ext 64, max_cost 400. Figures of this model (printed by the test): 64 inner sides; 454 read bases between the
    inner ends and the true cuts before, up to 43 on one side; 440 recovered; sum |true cut - extended end| = 58; no side overshoots by
    more than 2 bases, none falls short by more than 7; 59 of the 64 sides change; the highest stop level is 142. Asserted with about a
    factor two of room: the sum afterwards is at most a quarter of the sum before, no overshoot above 5, two valid segments per read."""
    import split_model as sm
    c = chimeric_model()
    K = c["K"]
    before = inner_gaps(c["split"][3], c["halves"], K)
    after = inner_gaps(c["ext_out"][3], c["halves"], K)
    assert [b[:2] for b in before] == [a[:2] for a in after] and len(before) == 64
    ext = c["ext"]
    recovered = sum(int(ext["dq"][slot][side]) for slot, side, _ in before)
    changed = sum(bool(ext["dq"][slot][side] or ext["dr"][slot][side]) for slot, side, _ in before)
    sum_before, sum_after = sum(abs(g) for _, _, g in before), sum(abs(g) for _, _, g in after)
    over, short = max(-g for _, _, g in after), max(g for _, _, g in after)
    print("inner sides", len(before), "gap before", sum(g for _, _, g in before), "max", max(g for _, _, g in before), "recovered", recovered, "sum |d| before", sum_before,
          "after", sum_after, "max overshoot", over, "max short", short, "changed", changed, "max stop", int(ext["stop"].max()))
    assert 4 * sum_after <= sum_before and over <= 5
    assert ((c["ext_out"][3]["flags"].reshape(-1, K) & sm.VALID != 0).sum(axis=1) == 2).all()
    # what part 2 keeps: segments inside the read, windows inside the reference and within a row, patterns the read's bytes
    req, tp, pat, seg = c["ext_out"]
    for slot in np.nonzero(seg["flags"] & sm.VALID)[0]:
        qb, qe, L = int(seg["q_begin"][slot]), int(seg["q_end"][slot]), int(seg["read_len"][slot])
        assert 0 <= qb < qe <= L and int(req["pattern_len"][slot]) == qe - qb and pat[slot, :qe - qb].tobytes() == c["rows"][slot // K, qb:qe].tobytes()
        start = int(tp[slot]) & (sm.MINUS - 1)
        assert 0 <= start and start + int(req["text_len"][slot]) <= len(c["ref"]) and int(req["text_len"][slot]) <= pat.shape[1]


def test_extended_segments_stay_under_the_cap_of_the_whole_path():
    """What the GPU whole-path test relies on, on tests/endsfree_model.py: every extended segment aligns (WFA (3, 4, 1), 2 * flank of
    free text at both ends) within bound + x * (the overshoot of its inner sides past the true cut), bound = edits * max(x, o + e): below
    MAX_SCORE = bound + 16 while the overshoot is at most 5."""
    import chain_class_model as ccm
    import endsfree_model as efm
    import extend_model as em
    import split_model as sm
    c = chimeric_model()
    K, flank = c["K"], c["flank"]
    x, o, e = 3, 4, 1
    bound = ccm.CHIMERIC_EDITS * max(x, o + e)
    req, tp, pat, seg = c["ext_out"]
    over = {}
    for slot, side, g in inner_gaps(seg, c["halves"], K):
        over[slot] = over.get(slot, 0) + max(-g, 0)
    slots = np.nonzero(seg["flags"] & sm.VALID)[0]
    txt = np.zeros((len(slots), pat.shape[1]), dtype=np.uint8)
    for i, slot in enumerate(slots):
        start, minus = int(tp[slot]) & (sm.MINUS - 1), int(tp[slot]) >> 63
        text = c["ref"][start:start + int(req["text_len"][slot])]
        txt[i, :len(text)] = em.COMP[text][::-1] if minus else text
    scores = efm.dp_scores(req[slots], pat[slots], txt, x, o, e, ends_free=(0, 0, 2 * flank, 2 * flank))
    for slot, score in zip(slots, scores):
        assert score <= bound + x * over.get(int(slot), 0), (slot, score, bound, over.get(int(slot), 0))
    worst = int(scores.max())
    print("worst score", worst, "bound", bound, "cap", bound + 16)
    assert worst <= bound + 16


# ---- the directed batch ----------------------------------------------------------------------------------------------------------
def test_what_the_directed_batch_holds():
    import extend_model as em
    import split_model as sm
    ref = em.directed_reference()
    assert (ref == ord("N")).sum() > 100 and (ref >= 0x61).sum() > 100
    for K, rs, pen in ((4, 104, em.PENALTIES[0]), (16, 1024, em.PENALTIES[2])):
        d = em.directed(1, 192, K, rs, ref)
        p = em.Params(*pen[:4], pen[4], 400, 31, 64)
        (req, tp, pat, seg), ext = em.directed_expected(p, d, K, rs, ref)
        moved = (ext["dq"] != 0).any(axis=1)
        kinds = np.array(d["kinds"])
        designed = np.arange(192) * K + np.arange(192) % K
        count = {kd: int(moved[designed][kinds == kd].sum()) for kd in em.JUNCTIONS}
        print(K, rs, count, "moved", int(moved.sum()), "both", int(((ext["dq"] != 0).all(axis=1)).sum()))
        for kd in ("clean", "mismatch", "insertion", "deletion", "odd_bytes", "q1", "two_sides"):
            assert count[kd] >= 6, (kd, count)
        for kd in ("q0", "loose", "open", "invalid"):
            assert count[kd] == 0, (kd, count)
        assert ((ext["dq"] != 0).all(axis=1)).sum() >= 6 and (tp[moved] >> np.uint64(63) != 0).any() and (tp[moved] >> np.uint64(63) == 0).any()
        assert (~moved & (seg["flags"] & sm.VALID != 0)).any() and (seg["flags"] == 0).any()
        untouched = ~moved
        assert pat[untouched].tobytes() == d["seg_pat"][untouched].tobytes() and req[untouched].tobytes() == d["seg_req"][untouched].tobytes()
        assert (req["text_len"] <= rs).all() and (seg["q_end"] <= np.clip(d["read_len"], 0, rs).repeat(K))[seg["flags"] & sm.VALID != 0].sum() > 0


# ---- the interface ---------------------------------------------------------------------------------------------------------------
def test_constants_symbols_layouts_and_feature_bit(tmp_path):
    from aim_amd import capi, engine
    import extend_model as em
    import ctypes as C
    assert _define("AIM_FEATURE_EXTEND") == capi.FEATURE_EXTEND == 0x40000
    assert engine.features() & capi.FEATURE_EXTEND and engine.features() & capi.FEATURE_SPLIT
    assert _lib().aim_abi_version() == 2
    assert (_define("AIM_SEG_EXT_LEFT"), _define("AIM_SEG_EXT_RIGHT")) == (capi.SEG_EXT_LEFT, capi.SEG_EXT_RIGHT) == (em.EXT_LEFT, em.EXT_RIGHT) == (0x20, 0x40)
    assert tuple(_define("AIM_EXTEND_MAX_" + n) for n in ("UNIT", "COST", "BAND", "EXT")) == (em.MAX_UNIT, em.MAX_COST, em.MAX_BAND, em.MAX_EXT) == \
        (capi.EXTEND_MAX_UNIT, capi.EXTEND_MAX_COST, capi.EXTEND_MAX_BAND, capi.EXTEND_MAX_EXT) == (64, 4095, 31, 1024)
    assert _lib().aim_extend_kernel_names() == b"extend_sides_kernel,extend_apply_kernel"
    assert _lib().aim_split_kernel_names() == b"split_segments_kernel,sam_lane_split_kernel,sam_wave_split_kernel"      # the names that were there stay
    assert callable(engine.extend_params) and callable(engine.extend_segments_device) and callable(engine.extend_segments)
    assert capi.EXTEND_DTYPE == em.EXTEND and capi.EXTEND_DTYPE.itemsize == 24 and C.sizeof(capi.ExtendParams) == 32
    ep = engine.extend_params()
    assert (ep.match, ep.mismatch, ep.gap_o, ep.gap_e, ep.xdrop, ep.max_cost, ep.band, ep.max_ext) == (1, 3, 4, 1, 20, 400, 31, 64)
    src = tmp_path / "c.c"
    ext_fields = ("dq", "dr", "stop", "pad", "score")
    par_fields = ("match", "mismatch", "gap_o", "gap_e", "xdrop", "max_cost", "band", "max_ext")
    args = ", ".join(["sizeof(aim_extend_t)"] + ["offsetof(aim_extend_t, %s)" % f for f in ext_fields] + ["sizeof(aim_extend_params_t)"] +
                     ["offsetof(aim_extend_params_t, %s)" % f for f in par_fields])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "aim_hip.h"\nint main(void) { printf("%s\\n", %s); return 0; }\n' %
                   (" ".join(["%zu"] * (2 + len(ext_fields) + len(par_fields))), args))
    exe = tmp_path / "c"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [24] + [capi.EXTEND_DTYPE.fields[f][1] for f in ext_fields] + [32] + [getattr(capi.ExtendParams, f).offset for f in par_fields]


def _extend(K=4, read_size=128, ref_len=65536, n_reads=4, null_params=False, **kw):
    """aim_extend_segments_device with NULL buffers: the parameter checks come first, with or without a device."""
    import ctypes as C
    from aim_amd import engine
    ep = engine.extend_params(**kw)
    return _lib().aim_extend_segments_device(None if null_params else C.byref(ep), K, read_size, ref_len, n_reads, *([None] * 9))


EXTEND_BAD = [(dict(K=0), "K 0 is outside 1..16"), (dict(K=17), "K 17 is outside 1..16"), (dict(read_size=0), "read_size 0 must be"),
              (dict(read_size=100), "read_size 100 must be"), (dict(read_size=65536), "read_size 65536 must be"),
              (dict(n_reads=1 << 30), "n_reads 1073741824 * K 4 does not fit 32 bits"), (dict(null_params=True), "NULL parameters"),
              (dict(match=0), "match 0 must be >= 1"), (dict(mismatch=0), "mismatch 0 must be >= 1"), (dict(gap_o=-1), "gap_o -1 must be >= 0"),
              (dict(gap_e=0), "gap_e 0 must be >= 1"), (dict(xdrop=-1), "xdrop -1 must be >= 0"), (dict(max_cost=0), "max_cost 0 is outside 1..4095"),
              (dict(max_cost=4096), "max_cost 4096 is outside 1..4095"), (dict(band=0), "band 0 is outside 1..31"), (dict(band=32), "band 32 is outside 1..31"),
              (dict(max_ext=7), "max_ext 7 is outside 8..1024"), (dict(max_ext=1025), "max_ext 1025 is outside 8..1024"),
              (dict(match=2, mismatch=31), "max(x', o' + e') = 66 is above 64"), (dict(gap_o=30, gap_e=2), "max(x', o' + e') = 65 is above 64"),
              (dict(ref_len=0xFE000001), "ref_len 4261412865 is above 4261412864"), (dict(), "null device buffer")]


@pytest.mark.parametrize("kw,msg", EXTEND_BAD, ids=[m for _, m in EXTEND_BAD])
def test_extend_refusals(kw, msg):
    from aim_amd import capi
    assert _extend(**kw) == capi.AIM_EINVAL and _err().startswith("aim_extend_segments_device: " + msg), _err()


def test_refusal_order_and_bounds_that_pass():
    """Each refusal comes before those behind it in the header's list; the null buffer is the last; the largest legal values get that
    far; the Python layer raises with the message."""
    from aim_amd import capi, engine
    bad = [dict(K=17), dict(read_size=7), dict(n_reads=1 << 30), dict(match=0), dict(mismatch=0), dict(gap_o=-1), dict(gap_e=0), dict(xdrop=-1), dict(max_cost=0),
           dict(band=0), dict(max_ext=7), None, dict(ref_len=1 << 32)]
    words = ["K 17", "read_size 7", "n_reads", "match 0", "mismatch 0", "gap_o -1", "gap_e 0", "xdrop -1", "max_cost 0", "band 0", "max_ext 7", "max(x'", "ref_len"]
    for i in range(len(bad)):
        kw = {}
        for b in bad[i:]:
            kw.update(b if b is not None else {})
        if bad[i] is None:                                                   # the unit bound from legal single fields
            kw.update(mismatch=31, match=2)
        assert _extend(**kw) == capi.AIM_EINVAL and words[i] in _err(), (i, _err())
    assert _extend(K=16, read_size=65528, ref_len=0xFE000000, match=2, mismatch=30, gap_o=0, gap_e=1, xdrop=(1 << 31) - 1, max_cost=4095, band=31, max_ext=1024) == \
        capi.AIM_EINVAL and _err() == "aim_extend_segments_device: null device buffer"
    assert _extend(K=1, read_size=8, ref_len=0, match=1, mismatch=1, gap_o=0, gap_e=1, xdrop=0, max_cost=1, band=1, max_ext=8) == capi.AIM_EINVAL and \
        "null device buffer" in _err()
    assert _extend(match=31, mismatch=1, gap_o=0, gap_e=16) == capi.AIM_EINVAL and "null device buffer" in _err()      # x' = 64, o' + e' = 63
    with pytest.raises(capi.AimError) as e:
        engine.extend_segments_device(engine.extend_params(band=40), 4, 128, 1000, 4, *([None] * 8))
    assert "band 40" in str(e.value)


def test_extend_kernels_code_objects():
    """Each new kernel exists exactly once, uses no scratch and no static LDS and stays within kExtendMaxVgpr; every kernel
    test_split_kernels_code_objects lists is still there, once per instantiation."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_regs
    lib = os.path.join(ROOT, "aim_amd", "libaim_hip.so")
    if not os.path.exists(lib):
        pytest.fail("libaim_hip.so is missing: run the build")
    regs = codeobj_regs.kernel_regs(lib)
    names = _lib().aim_extend_kernel_names().decode().split(",")
    assert names == ["extend_sides_kernel", "extend_apply_kernel"]
    bound = int(re.search(r"constexpr int kExtendMaxVgpr = (\d+);", open(os.path.join(ROOT, "aim_amd", "csrc", "extend.hpp")).read()).group(1))
    for name in names:
        found = [n for n in regs if re.search(r"\baim::%s\(" % name, n)]
        assert len(found) == 1, (name, found)
        r = regs[found[0]]
        print(name, r)
        assert r["scratch_bytes"] == 0 and r["lds_static_bytes"] == 0 and 0 < r["vgpr"] + r["agpr"] <= bound <= 512 // 8, (name, r, bound)
    assert len([n for n in regs if re.search(r"\baim::split_segments_kernel<(16|64)>\(", n)]) == 2
    for name in ("sam_lane_split_kernel", "sam_wave_split_kernel", "seed_candidates_kernel", "seed_minimizer_kernel", "seed_chain_kernel",
                 "seed_chain_minimizer_kernel", "seed_chain_long_kernel", "chain_class_kernel", "read_mapq_kernel", "sam_lane_kernel", "sam_wave_kernel"):
        assert len([n for n in regs if re.search(r"\baim::%s\(" % name, n)]) == 1, name
