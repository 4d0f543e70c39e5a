"""SWG with a match bonus (tests/match_bonus.py), without a device: the table reaches the kernels it names and never the register
kernel, the int16 admission rules flip where the arithmetic says, the oracle agrees with an int64 model of swg.c's recurrence on
every row whose cells fit their type (and its CIGARs re-score to the score where MAX_SCORE cannot win), ignores the bytes behind a
length, and really wraps on the rows that are there for wrapping; the batches tell a kernel that drops, misplaces or partly forgets
the bonus from a right one; and the selection models order negative scores as a plain sort does."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import full_rows as F
import match_bonus as B
from conftest import ROOT

INT32_MAX = 2 ** 31 - 1
UINT32_MAX = 2 ** 32 - 1


# ------------------------------------------------------------------ plans
@pytest.fixture(scope="module")
def plans(built):
    env = {k: v for k, v in os.environ.items() if not k.startswith("AIM_") or k == "AIM_LIB"}
    env.update(AIM_SCRATCH_GB="16", AIM_CHIP_CUS="256")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "match_bonus.py"), "--plans"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_the_table_reaches_the_kernels_and_shapes_it_names(plans):
    """aim_plan_describe of every row (at the row's own pair count, 16 GB, 256 CUs) names the expected kernel and shape tokens.
    When a planner change moves an edge the new line is printed here: the row then takes the new first READ_SIZE of that shape."""
    rows = {"%s/%d" % r: r for r in B.ROWS}
    moved = ["%s: expected %r, the planner says %r" % (k, B.expected_plan(*rows[k]), plans[k]) for k in rows
             if not F.plan_matches(plans[k], B.expected_plan(*rows[k]))]
    assert not moved, "\n".join(moved)
    reached = {plans[k].split()[0] for k in rows}
    assert reached == {"swg_lane_kernel", "dp_group_kernel", "dp_strip_kernel", "dp_wave_kernel"}
    # both of dp_group's fallbacks, dp_strip at one, two and three wavefronts per pair, swg_lane with and without staged sequences
    lines = " ".join(plans[k] for k in rows)
    for token in (B._FB_LANE, B._FB_STRIP, " wavefronts_per_pair=1 ", " wavefronts_per_pair=2 ", " wavefronts_per_pair=3 ", " seq_lds=0", " seq_lds=1"):
        assert token in lines + " ", token


def test_the_register_kernel_is_never_chosen_with_a_bonus(plans):
    """swg_reg_supported refuses match != 0: the short rows plan on swg_reg_kernel with match = 0 and on swg_lane_kernel with
    every bonus; no row of the table reaches the register kernel."""
    for rs in (40, 136):
        for bt in (0, 1):
            assert plans["reg/%d/0/%d" % (rs, bt)].split()[0] == "swg_reg_kernel"
            for m in (-1, -2, -30):
                assert plans["reg/%d/%d/%d" % (rs, m, bt)].split()[0] == "swg_lane_kernel", (rs, m, bt)
    assert not [k for k, v in plans.items() if not k.startswith("reg/") and "swg_reg_kernel" in v]


def test_the_int16_admission_rules_flip_where_the_arithmetic_says(plans):
    """At (-30, 3, 4, 1): dp_strip_exact_ok holds up to READ_SIZE 1024 (31 * 1024 + 22 = 31 766) and fails from 1032 on, which
    the plan shows (dp_group, then dp_wave). dp_wave_exact_ok holds up to 1064 (31 920) and fails from 1072 on; the plan line
    names dp_wave_kernel on both sides and does not say which of its two paths runs (the kernel evaluates the rule itself), so
    that edge is pinned by the rule's arithmetic. Nothing wraps before READ_SIZE 1093 (30 * 1093 = 32 790 > 32 768)."""
    for fam in ("edge", "edge_bt"):
        assert [plans["%s/%d" % (fam, rs)].split()[0] for rs in (1024, 1032, 1064, 1072, 1096)] == ["dp_group_kernel"] + ["dp_wave_kernel"] * 4
    c = B.COSTS_EDGE
    assert B.dp_strip_exact_lo(c, 1024) == -31766 > B.INT16_FLOOR >= B.dp_strip_exact_lo(c, 1032)
    assert B.dp_wave_exact_lo(c, 1064) == -31920 > B.INT16_FLOOR >= B.dp_wave_exact_lo(c, 1072) == -32160 > -32768 > B.dp_wave_exact_lo(c, 1096)
    src = open(os.path.join(ROOT, "aim_amd", "csrc", "dp_wave.hpp")).read() + open(os.path.join(ROOT, "aim_amd", "csrc", "dp_strip.hpp")).read()
    assert "const long lo = (long)p.match * rs;" in src and "return hi < 32000 && lo > -32000 && p.max_score < 32000;" in src
    assert "const long lo = (long)p.match * rs - (rs + 2) * ge - 4L * (p.gap_o + p.gap_e);" in src and "return lo > -32000;" in src
    for costs in (B.COSTS_A, B.COSTS_B):          # the ordinary rows are far inside both rules
        assert B.dp_strip_exact_lo(costs, 2568) > B.INT16_FLOOR


# ------------------------------------------------------------------ the oracle against the model
def _fits(fam, lo, hi):
    cl, ch = B.cell_range(fam)
    return (lo >= cl) & (hi <= ch)


@pytest.mark.parametrize("fam,rs", B.FITTING, ids=lambda v: str(v))
def test_oracle_equals_the_model_where_the_cells_fit(built, fam, rs):
    """Every cell of every unaliased pair fits the cell type by the model's own minimum and maximum, and the oracle's scores of
    those pairs are the model's. The batch covers both signs: at least a quarter of its pairs score below 0 (IDENTICAL scores
    match * READ_SIZE), at least two above 0 (A_VS_C and the length-mismatched head pairs), the empty sequences 0."""
    sel, score, lo, hi = B.model_row(fam, rs)
    res, _ = B.oracle_row(fam, rs)
    req, _, _ = F.row_batch(rs, "zero")
    assert (res["status"] == 0).all()
    assert _fits(fam, lo, hi).all()
    assert {0, 2, 7, 8, 10, F.IDENTICAL, F.TWIN_A, F.TWIN_B, F.A_VS_C, F.N_LAST, len(req) - 1} <= set(sel.tolist())
    bad = np.nonzero(res["score"][sel] != score)[0]
    assert bad.size == 0, "pair %d: oracle %d, model %d" % (sel[bad[0]], res["score"][sel[bad[0]]], score[bad[0]])
    neg, pos = int((res["score"] < 0).sum()), int((res["score"] > 0).sum())
    print("%s/%d: %d of %d pairs negative, %d positive, %d zero" % (fam, rs, neg, len(req), pos, len(req) - neg - pos))
    assert 4 * neg >= len(req) and pos >= 2
    assert res["score"][F.IDENTICAL] == B.FAMILIES[fam]["costs"][0] * rs == lo.min()
    assert res["score"][F.A_VS_C] > 0 and res["score"][9] == 0 and res["score"][10] == 0


@pytest.mark.parametrize("fam,rs", B.WRAPPING, ids=lambda v: str(v))
def test_the_wrapping_rows_wrap(built, fam, rs):
    """The cap that keeps these rows honest: by the model at least one pair (IDENTICAL) holds a value below the cell type's
    minimum, and the oracle's score of that pair is not the recurrence's; where a pair's cells do fit, the oracle agrees."""
    sel, score, lo, hi = B.model_row(fam, rs)
    res, _ = B.oracle_row(fam, rs)
    fit = _fits(fam, lo, hi)
    at = sel.tolist().index(F.IDENTICAL)
    assert lo[at] == B.FAMILIES[fam]["costs"][0] * rs < B.cell_range(fam)[0] and not fit[at]
    assert res["score"][F.IDENTICAL] != score[at]
    assert np.array_equal(res["score"][sel][fit], score[fit])
    print("%s/%d: %d of %d unaliased pairs fit; IDENTICAL scores %d, the recurrence %d" % (fam, rs, fit.sum(), len(sel), res["score"][F.IDENTICAL], score[at]))
    if fam.startswith("edge"):
        assert res["score"][F.IDENTICAL] == -32744


@pytest.mark.parametrize("fam,rs", B.MODEL_ROWS, ids=lambda v: str(v))
def test_cigars_rescore_where_max_score_cannot_win(built, fam, rs):
    """MAX_SCORE above any path's cost: every unaliased pair's CIGAR uses up both sequences, tells 'M' from 'X' truthfully and
    re-scores with (match, mismatch, gap_o, gap_e) to the score. (An aliased pair's table is not the recurrence's, so its walk
    is only held to the kernels, not to this.)"""
    from endsfree_model import check_cigar
    res, ops = B.oracle_row(fam, rs)
    req, pat, txt = F.row_batch(rs, "zero")
    costs = B.FAMILIES[fam]["costs"]
    assert (res["status"] == 0).all()
    for i in B.unaliased(req):
        p, t = bytes(pat[i, :req["pattern_len"][i]]), bytes(txt[i, :req["text_len"][i]])
        s = bytes(ops[i, int(res["begin_offset"][i]):int(res["end_offset"][i])]).decode()
        assert res["max_operations"][i] == len(p) + len(t)
        if not p:          # (the loops wrote nothing: score 0 and a CIGAR of insertions)
            assert res["score"][i] == 0 and s == "I" * len(t)
            continue
        assert check_cigar(s, p, t) is None, (i, s)
        assert B.rescore(s, *costs) == res["score"][i], (i, s)
    assert B.rescore("MMXMIIMDM", -2, 5, 2, 3) == -2 * 5 + 5 + (2 + 6) + (2 + 3)


@pytest.mark.parametrize("fam,rs", B.ROWS, ids=lambda v: str(v))
def test_oracle_is_padding_independent(built, fam, rs):
    """Zero and noise padding give byte-identical results and identical ops inside [begin, end) on every row, the wrapping ones
    included."""
    zres, zops = B.oracle_row(fam, rs, "zero")
    nres, nops = B.oracle_row(fam, rs, "noise")
    assert zres.tobytes() == nres.tobytes()
    req, _, _ = F.row_batch(rs, "zero")
    F.compare(nres, nops, zres, zops, req, zops is not None, idx=False)
    assert (zres["max_operations"] == req["pattern_len"] + req["text_len"]).all()


# ------------------------------------------------------------------ the batches tell wrong kernels apart
@pytest.mark.parametrize("fam,rs", [("a16", 136), ("b16", 184)], ids=lambda v: str(v))
def test_comparison_catches_a_kernel_that_mishandles_the_bonus(built, fam, rs):
    """Three wrong kernels, each as swg_model's mutant in the place of the model: match taken as 0, and the bonus also added
    where the bases differ, each change the score of more than half of the row's pairs (the first IDENTICAL and the twins among
    them, the second every pair with a mismatch on its path); a head path without the bonus (the cells of row 1 and column 1)
    changes at least IDENTICAL and the twins. full_rows.compare, which the GPU module uses, passes the
    model's scores and fails each mutant's."""
    f = B.FAMILIES[fam]
    req, pat, txt = F.row_batch(rs, "zero")
    sel = B.unaliased(req)
    r, p, t = req[sel], np.ascontiguousarray(pat[sel]), np.ascontiguousarray(txt[sel])
    ores, _ = B.oracle_row(fam, rs)
    ores = ores[sel]
    good = ores.copy()
    good["score"] = B.swg_model(r, p, t, *f["costs"], f["ms"](rs))[0]
    F.compare(good, None, ores, None, r, False, idx=False)
    where = {k: sel.tolist().index(k) for k in (F.IDENTICAL, F.TWIN_A, F.TWIN_B)}
    for mutant, at_least in (("no_bonus", len(sel) // 2 + 1), ("bonus_on_mismatch", len(sel) // 2 + 1), ("head_without_bonus", 3)):
        bad = ores.copy()
        bad["score"] = B.swg_model(r, p, t, *f["costs"], f["ms"](rs), mutant=mutant)[0]
        wrong = bad["score"] != ores["score"]
        print("%s/%d %s: %d of %d scores change" % (fam, rs, mutant, wrong.sum(), len(sel)))
        assert wrong.sum() >= at_least, mutant
        if mutant == "bonus_on_mismatch":          # (an identical pair has no mismatch to misprice)
            assert not wrong[where[F.IDENTICAL]]
        else:
            assert all(wrong[i] for i in where.values()), mutant
        with pytest.raises(AssertionError, match="score differs at pair"):
            F.compare(bad, None, ores, None, r, False, idx=False)


# ------------------------------------------------------------------ the selection models take negative scores
def _groups():
    """(scores, status, read_offsets): hand-made reads. PAIR_OK is 0; 3 stands for any other status."""
    reads = [
        ([-90, 12, -95, -95, 40, -3], [0, 0, 0, 0, 0, 0]),            # mixed signs, a tie at the (negative) best
        ([-7, -7, -7], [0, 0, 0]),                                      # all tied and negative
        ([-100, -50, -1], [0, 0, 0]),                                   # all negative, no tie
        ([-200, -80, 5, -80], [3, 0, 0, 0]),                            # the most negative score belongs to a candidate that is not OK
        ([-5, -9], [3, 3]),                                             # no OK candidate at all
        ([0, -1, 1], [0, 0, 0]),                                        # around zero
        ([-2 ** 31 + 1, 2 ** 31 - 2, -1], [0, 0, 0]),                   # the ends of the score field next to AIM_SCORE_FAILED
        ([-2 ** 31, -4, -6], [3, 0, 0]),                                # AIM_SCORE_FAILED itself comes with a status that is not OK
        ([17], [0]), ([-17], [0]),
    ]
    scores = np.array([s for r in reads for s in r[0]], dtype=np.int64)
    status = np.array([s for r in reads for s in r[1]], dtype=np.int32)
    offs = np.concatenate([[0], np.cumsum([len(r[0]) for r in reads])]).astype(np.uint32)
    return scores, status, offs


def test_read_groups_model_orders_negative_scores_like_a_sort(built):
    import read_groups_model as m
    scores, status, offs = _groups()
    best, sel = m.select(scores, status, offs)
    for r in range(len(offs) - 1):
        ok = sorted((int(scores[i]), i) for i in range(offs[r], offs[r + 1]) if status[i] == 0)
        if not ok:
            assert tuple(best[r]) == (UINT32_MAX, INT32_MAX, INT32_MAX, 0) and sel[r] == offs[r]
            continue
        assert (best["best_pair"][r], best["best_score"][r], best["n_best"][r]) == (ok[0][1], ok[0][0], sum(1 for s, _ in ok if s == ok[0][0])), r
        assert best["second_score"][r] == (ok[1][0] if len(ok) > 1 else INT32_MAX) and sel[r] == ok[0][1], r
    assert best["best_score"][0] == -95 and best["n_best"][0] == 2 and best["second_score"][0] == -95 and best["best_pair"][0] == 2
    assert best["best_score"][3] == -80 and best["best_pair"][3] == offs[3] + 1          # not the -200 that is not OK


@pytest.mark.parametrize("max_hits", [1, 3, 8])
def test_top_hits_model_orders_negative_scores_like_a_sort(built, max_hits):
    import top_hits_model as m
    scores, status, offs = _groups()
    hoff, hit_pair = m.rank(scores, status, offs, max_hits)
    for r in range(len(offs) - 1):
        idx = range(offs[r], offs[r + 1])
        order = [i for _, i in sorted((int(scores[i]), i) for i in idx if status[i] == 0)] + [i for i in idx if status[i] != 0]
        assert hit_pair[hoff[r]:hoff[r + 1]].tolist() == order[:max_hits], r
    if max_hits >= 3:
        assert hit_pair[hoff[0]:hoff[0] + 3].tolist() == [2, 3, 0]          # -95, -95 (index order), -90


def test_mate_pairs_model_orders_negative_sums_like_a_sort(built):
    """Read pairs with candidates of both signs on both strands, every span allowed: the winner is the first of sorted((cost, i,
    j)) over the OK opposite-strand combinations when its cost is at most best + best + penalty -- below 0 here -- and the
    independent winners otherwise."""
    import mate_pairs_model as m
    minus = 1 << 63
    scores = np.array([-95, -95, 10, -96,   -80, -80, 7,   -50, -60,   -70, 30,   -200, -10,   -20], dtype=np.int64)
    status = np.array([0, 0, 0, 0,          0, 0, 0,       0, 0,       0, 0,      3, 0,        0], dtype=np.int32)
    strand = [0, 0, 0, 1,                   1, 1, 0,       0, 0,       0, 0,      0, 0,        1]
    offs = np.array([0, 4, 7, 9, 11, 13, 14], dtype=np.uint32)
    start = [100 + 10 * i for i in range(len(scores))]
    tpos = np.array([p | (minus if s else 0) for p, s in zip(start, strand)], dtype=np.uint64)
    tlen = np.full(len(scores), 100)

    def proper(i, j):
        f, r = (j, i) if strand[i] else (i, j)
        return status[i] == 0 and status[j] == 0 and strand[i] != strand[j] and start[f] <= start[r]

    for penalty in (0, 8, 30, 1000):
        sel, mates, best = m.select(scores, status, tpos, tlen, offs, 0, 1 << 40, penalty)
        for k in range(3):
            a, b = 2 * k, 2 * k + 1
            combos = sorted((int(scores[i] + scores[j]), i, j) for i in range(offs[a], offs[a + 1]) for j in range(offs[b], offs[b + 1]) if proper(i, j))
            unpaired = int(best["best_score"][a]) + int(best["best_score"][b]) + penalty
            if combos and combos[0][0] <= unpaired:
                assert mates["flags"][k] == 1 and tuple(mates["best_pair"][k]) == combos[0][1:] and mates["score_sum"][k] == combos[0][0], (penalty, k)
                assert mates["n_best"][k] == sum(1 for c in combos if c[0] == combos[0][0])
                assert mates["second_sum"][k] == (combos[1][0] if len(combos) > 1 else INT32_MAX)
                assert (sel[a], sel[b]) == combos[0][1:]
            else:
                assert mates["flags"][k] == 0 and mates["score_sum"][k] == unpaired, (penalty, k)
                assert mates["second_sum"][k] == (combos[0][0] if combos else INT32_MAX)
                assert (sel[a], sel[b]) == (best["best_pair"][a], best["best_pair"][b])
    # read pair 0: the independent winners (-96 and -80) share a strand; the best proper pairs cost -175, four of them tied
    sel, mates, best = m.select(scores, status, tpos, tlen, offs, 0, 1 << 40, 0)
    assert mates["flags"][0] == 0 and mates["score_sum"][0] == -176 and mates["second_sum"][0] == -175      # best + best + penalty < 0 wins
    sel, mates, best = m.select(scores, status, tpos, tlen, offs, 0, 1 << 40, 8)
    assert mates["flags"][0] == 1 and mates["score_sum"][0] == -175 and mates["n_best"][0] == 4 and tuple(mates["best_pair"][0]) == (0, 4)
    assert mates["flags"][1] == 0 and mates["score_sum"][1] == -122          # no proper pair: -60 + -70 + 8
    assert mates["flags"][2] == 1 and mates["score_sum"][2] == -30           # the -200 that is not OK does not count
