"""The table of tests/wfa_group_rows.py without a device: every row's plan names the wfa_group_kernel width and variant it is there
for and is the first READ_SIZE of its shape, the table holds every (kind, G, backtrace[, reduce]) the default planner reaches, every
row's batch has enough pairs on both sides of MAX_SCORE by the variant's model alone, and the comparison the GPU module uses fails
on a score that is one edit off and on a CIGAR byte that lies."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

import full_rows as F
import wfa_group_rows as W
from conftest import ROOT


@pytest.fixture()
def planner(built, monkeypatch):
    """plan(env): the AIM_* environment made the fixed chip's plus `env`."""
    from reference_rows import apply_env

    def plan(env):
        apply_env(monkeypatch, W.plan_env(env))
    plan({})
    return plan


def test_the_table_is_what_the_rules_give(planner):
    """make_table() under today's planner gives the committed table: every default row is the first READ_SIZE of its width under
    its MAX_SCORE rule, every forced row the smallest feasible one, and the escalation rows the first (penalty set, READ_SIZE,
    MAX_SCORE) of theirs. When a planner change moves an edge the differing rows are printed here."""
    made = W.make_table()
    moved = ["%r: the table has %r, the rules give %r" % (k, W.TABLE.get(k), made.get(k)) for k in sorted(set(made) | set(W.TABLE), key=str)
             if made.get(k) != W.TABLE.get(k)]
    assert not moved, "\n".join(moved)
    for kind in W.VARIANTS:          # all seven widths, with and without BACKTRACE
        assert {(k[1], k[2]) for k in W.TABLE if k[0] == kind} == {(G, bt) for G in W.WIDTHS for bt in (False, True)}, kind
    assert {k[1:] for k in W.TABLE if k[0] == "escalate"} == {(G, bt, red) for G in W.WIDTHS for bt in (False, True) for red in (False, True)}
    assert {k[1:] for k in W.TABLE if k[0] == "escalate_modrows"} == {(G, bt, True) for G in (8, 16) for bt in (False, True)}


def _rule_rate(key):
    rs, ms, pen, env = W.TABLE[key]
    return [r for r in (0.02, 0.10) if W.score_rule(key[0], rs, r, pen) == ms][0]


@pytest.mark.parametrize("key", list(W.TABLE), ids=W.row_id)
def test_rows_reach_the_widths_they_name(planner, key):
    """aim_plan_describe of the row (at its own pair count and knobs, 16 GB, 256 CUs) names wfa_group_kernel, G=<G> and the
    variant's token -- under escalation in the second stage, behind a lane kernel, with escalate=c, c > 0. READ_SIZE - 8 gives
    another width or another kernel (or the row's READ_SIZE is the smallest there is)."""
    rs, ms, pen, env = W.TABLE[key]
    planner(env)
    line = W.plan_of(key)
    assert W.line_width(key, line) == key[1] and W.row_token(key) in line, "%r: the planner says %r" % (key, line)
    esc = key[0].startswith("escalate")
    if esc:
        assert line.split()[0] in ("wfa_lane_kernel", "wfa_lane_packed_kernel") and 0 < W.escalate_cap(line) < ms, line
    if rs - 8 >= (W.LANE_READ_SIZES[0] if esc else 8):
        ms0 = ms if esc else W.score_rule(key[0], rs - 8, _rule_rate(key), pen)
        G0, line0 = W._plan_width(key[0].split("_")[0], rs - 8, ms0, pen, key[2], esc and key[3])
        assert G0 != key[1], "READ_SIZE %d is not the first of %r: %r" % (rs, key, line0)
    assert W.is_forced(key) == bool(env) and set(env) <= {"AIM_GROUP_G", "AIM_GROUP_WLDS"}


@pytest.mark.parametrize("key", [k for k in W.VARIANT_ROWS if W.degenerate_runs(k)], ids=W.row_id)
def test_degenerate_settings_plan_on_the_rows_width(planner, key):
    """No free end, two equal pieces, a second piece of MAX_SCORE + 1: held to the row's width with AIM_GROUP_G these run the row's
    own instantiation (their rows and rings are smaller, so the width is feasible) -- but for the second piece of MAX_SCORE + 1 where
    MAX_SCORE + 2 ring rows are more than wfa_group_kernel has, which is wfa_wave_kernel's."""
    from aim_amd import engine
    rs, ms, pen, env = W.TABLE[key]
    planner(dict(env, AIM_GROUP_G=str(key[1])))
    for name, kw in W.degenerate_runs(key):
        line = F.plan_line(engine.make_params("wfa", ms, rs, backtrace=key[2], **kw), F.pairs_for(rs))
        assert W.line_width(key, line) == key[1] or (name == "never" and ms + 1 > 31 and line.startswith("wfa_wave_kernel ")), line


@pytest.mark.parametrize("key", [k for k in W.TABLE if k[0] == "escalate_modrows"], ids=W.row_id)
def test_modulo_row_rows_run_on_rows_of_96(built, key):
    """The plan line does not say how the ring rows are addressed; AIM_PLAN_DEBUG's line does. The second stage of these rows
    runs on rows of 96 entries (no power of two: the modulo-row kernels) at the row's width."""
    env = dict(W.plan_env(W.TABLE[key][3]), AIM_PLAN_DEBUG="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wfa_group_rows.py"), "--plan", repr(key)], env=env, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert W.line_width(key, r.stdout.strip()) == key[1], r.stdout
    dbg = [l for l in r.stderr.splitlines() if l.startswith("[aim plan] wfa_group ") and " wcap=%d " % (2 * W.TABLE[key][1] + 3) in l]     # (the plans at MAX_SCORE)
    assert dbg and all(re.search(r" G=%d .* wlds=96 " % key[1], l) for l in dbg), r.stderr[-2000:]


def test_the_table_holds_every_width_the_default_planner_reaches(planner):
    """kind x READ_SIZE 8 .. 4096 x BACKTRACE x MAX_SCORE by the launchers' rule at 1, 2, 5 and 10 % under both penalty sets (the
    escalation pass: the lane kernels' READ_SIZEs and penalty sets x MAX_SCORE 11, 25, 50, 100 x REDUCE), no AIM_GROUP_* variable:
    every (kind, G, backtrace[, reduce]) whose plan is wfa_group_kernel has a table row, and none is listed as unreached."""
    t0 = time.time()
    reached = {}
    for kind in W.VARIANTS:
        for pen in W.PENALTIES[kind]:
            for bt in (False, True):
                for rate in W.RATES:
                    for rs in range(8, 4097, 8):
                        G, _ = W._plan_width(kind, rs, W.score_rule(kind, rs, rate, pen), pen, bt)
                        if G is not None:
                            reached.setdefault((kind, G, bt), (rs, rate))
    for pen in W.ESC_PENS:
        for bt in (False, True):
            for red in (False, True):
                for ms in W.ESC_SCORES:
                    for rs in W.LANE_READ_SIZES:
                        G, _ = W._plan_width("escalate", rs, ms, pen, bt, red)
                        if G is not None:
                            reached.setdefault(("escalate", G, bt, red), (rs, ms))
    print("reached by the default planner (first READ_SIZE, rate or MAX_SCORE):")
    for k in sorted(reached, key=str):
        print("  %-28s %r" % (W.row_id(k), reached[k]))
    print("forced rows:", ", ".join(W.row_id(k) for k in W.TABLE if W.is_forced(k)))
    print("unreached:", W.UNREACHED or "none")
    missing = sorted(set(reached) - set(W.TABLE), key=str)
    assert not missing, missing
    assert not set(reached) & {k for k, why in W.UNREACHED}
    for kind in W.VARIANTS:          # the widths no default plan gives are exactly the forced rows
        assert {k for k in W.TABLE if k[0] == kind and not W.is_forced(k)} == {k for k in reached if k[0] == kind}
    assert {k for k in W.TABLE if k[0] == "escalate" and not W.is_forced(k)} == {k for k in reached if k[0] == "escalate"}
    assert time.time() - t0 < 60


# ------------------------------------------------------------------ the batches, by the models alone
_MODEL_KEYS = {}
for _k in W.VARIANT_ROWS:            # rows that differ only in BACKTRACE share one model run
    _MODEL_KEYS.setdefault((_k[0], _k[1], W.TABLE[_k][0], W.TABLE[_k][1], tuple(sorted(W.TABLE[_k][2].items()))), _k)


@pytest.mark.parametrize("key", list(_MODEL_KEYS.values()), ids=W.row_id)
def test_variant_batches_have_pairs_on_both_sides_of_the_cap(built, key):
    """At least a third of a row's pairs score at most MAX_SCORE by the variant's DP model and at least three score over it."""
    rs, ms, pen, env = W.TABLE[key]
    want = W.model_row(key)
    n = len(want)
    print("%s: READ_SIZE %d MAX_SCORE %d: %d of %d pairs under the cap" % (W.row_id(key), rs, ms, (want <= ms).sum(), n))
    assert n == F.pairs_for(rs) and 3 * (want <= ms).sum() >= n and (want > ms).sum() >= 3
    req, pat, txt = W.row_batch(key, "noise")
    assert np.array_equal(W.variant_scores(key[0], req, pat, txt, pen), want)          # the padding is no part of a sequence


@pytest.mark.parametrize("key", W.ESCALATE_ROWS, ids=W.row_id)
def test_escalation_batches_leave_pairs_for_the_second_stage(planner, key):
    """At least ten pairs score over the first stage's cap by the oracle, in more than one 64-pair unit, and some stay under it."""
    rs, ms, pen, env = W.TABLE[key]
    planner(env)
    c = W.escalate_cap(W.plan_of(key))
    ores, _ = W.oracle_row(key)
    over = W.escalated(ores, c)
    print("%s: cap %d of %d: %d of %d pairs for the second stage" % (W.row_id(key), c, ms, over.size, len(ores)))
    assert over.size >= 10 and over[0] // 64 != over[-1] // 64 and over.size < len(ores)
    assert ((ores["score"] > c) & (ores["score"] <= ms)).sum() >= 3 or ms == c + 1


# ------------------------------------------------------------------ the comparison is sharp
def _flip(ops, res, i):
    """One 'M' of pair i's CIGAR becomes 'X' (or, without an 'M', one 'X' becomes 'M')."""
    b, e = int(res["begin_offset"][i]), int(res["end_offset"][i])
    row = ops[i, b:e]
    at = np.nonzero(row == ord("M"))[0]
    if at.size:
        ops[i, b + at[at.size // 2]] = ord("X")
    else:
        ops[i, b + np.nonzero(row == ord("X"))[0][0]] = ord("M")


@pytest.mark.parametrize("kind", W.VARIANTS)
def test_comparison_catches_a_score_one_edit_off_and_a_lying_cigar(built, kind):
    """check_variant() on results that are right by construction -- the oracle's global WFA, which ends-free with no free end and
    affine2p with two equal pieces must reproduce, and its NW for gap-linear -- passes; with one under-cap pair's score raised by
    the cheapest edit it fails on the score, with one CIGAR byte flipped 'M' <-> 'X' on the CIGAR."""
    from oracle import oracle
    rs = 112
    pen = W.PENALTIES[kind][1]
    req, pat, txt = F.full_row_batch(rs, F.MIN_PAIRS + 6, 17, "noise")
    if kind == "linear":             # (NW's flat table aliases where the pattern is longer than the text, and scores an empty pattern 0)
        flat = np.nonzero((req["pattern_len"] <= req["text_len"]) & (req["pattern_len"] > 0))[0]
        req, pat, txt = req[flat], np.ascontiguousarray(pat[flat]), np.ascontiguousarray(txt[flat])
        ms = 8 * rs
        op = oracle.params("nw", ms, rs, mismatch=pen["mismatch"], gap_i=pen["gap_e"], gap_d=pen["gap_e"], backtrace=True)
        kw = {}
    else:
        ms = W.score_rule(kind, rs, 0.02, pen)
        op = oracle.params("wfa", ms, rs, backtrace=True, **pen)
        kw = dict(ends_free=(0, 0, 0, 0), gap2=(pen["gap_o"], pen["gap_e"]))
    res, ops, _ = oracle.align_batch(op, req["pattern_len"], req["text_len"], pat, txt, nthreads=4)
    res, ops = res.copy(), ops.copy()
    res["idx"] = req["idx"]
    want = W.variant_scores(kind, req, pat, txt, pen, **kw)
    under = np.nonzero((want <= ms) & (want > 0))[0]
    assert under.size >= 3 and (kind == "linear" or (want > ms).sum() >= 3)
    if kind == "endsfree":           # the flag's over-cap result has an empty ops range, global WFA's one byte
        res["begin_offset"][want > ms] = res["end_offset"][want > ms]
    W.check_variant(kind, pen, ms, req, pat, txt, res, ops, True, want, **kw)
    W.check_variant(kind, pen, ms, req, pat, txt, res, None, False, want, **kw)
    i = int(under[under.size // 2])
    bad = res.copy()
    bad["score"][i] += W.cheapest_edit(kind, pen)
    for bt in (False, True):
        with pytest.raises(AssertionError, match="score differs at pair %d:" % i):
            W.check_variant(kind, pen, ms, req, pat, txt, bad, ops, bt, want, **kw)
    lie = ops.copy()
    _flip(lie, res, i)
    with pytest.raises(AssertionError, match="CIGAR of pair %d: [MX] on " % i):
        W.check_variant(kind, pen, ms, req, pat, txt, res, lie, True, want, **kw)
    with pytest.raises(AssertionError, match="ops differ at pair %d" % i):
        W.same_bytes((res, ops), (res, lie))
    if kind != "linear":             # ... and full_rows.compare, which the degenerate settings and the escalation rows go through
        with pytest.raises(AssertionError, match="score differs at pair %d" % i):
            F.compare(bad, ops, res, ops, req, True)
        with pytest.raises(AssertionError, match="ops differ at pair %d" % i):
            F.compare(res, lie, res, ops, req, True)
