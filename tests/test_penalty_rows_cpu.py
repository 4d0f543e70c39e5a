"""WFA across penalty sets (tests/penalty_rows.py), without a device: the oracle is the reference's rule on these sets (a second,
independent statement of it agrees pair by pair: tests/sentinel_model.py), the visibility rule holds as a property over a grid of
penalty sets, the batch shows the -10 on every visible row and nowhere else, the oracle's CIGARs there are valid alignments that
cost more than the score, the table reaches the plans it names, the rows would see a kernel that reads NULL for -10 or -10 for
NULL, and the three flags that promise a minimum cost are refused exactly where the -10 can show."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import full_rows as F
import penalty_rows as P
import sentinel_model as S
from conftest import ROOT

VISIBLE_PENS = sorted({P.ROWS[n]["pen"] for n in P.VISIBLE})
INVISIBLE_PENS = sorted({P.ROWS[n]["pen"] for n in P.INVISIBLE})


def _capped(scores, ms):
    return np.where(scores <= ms, scores, ms + 1)


# ------------------------------------------------------------------ the batch
def test_the_batch_is_what_it_says(built):
    req, pat, txt = P.batch()
    nreq, npat, ntxt = P.batch("noise")
    assert len(req) == P.N == 130 and pat.shape == (P.N, P.RS) and np.array_equal(req, nreq)
    tags = [c[2] for c in P.constructed_pairs(np.random.default_rng(0))]
    assert len(tags) == P.N_CONSTRUCTED == 72
    for i, (kind, k, place, mism) in enumerate(tags):
        assert req["pattern_len"][i] == P.PLEN and req["text_len"][i] == P.PLEN + (k if kind == "ins" else -k)
    assert np.array_equal(pat[P.IDENTICAL], txt[P.IDENTICAL]) and req["pattern_len"][P.IDENTICAL] == P.PLEN
    assert (pat[P.WITH_N] == ord("N")).sum() == 1 and (txt[P.WITH_N] == ord("N")).sum() == 1
    assert req["pattern_len"][P.EMPTY_PATTERN] == 0 and req["text_len"][P.EMPTY_PATTERN] > 0
    assert req["text_len"][P.EMPTY_TEXT] == 0 and req["pattern_len"][P.EMPTY_TEXT] > 0
    for i in range(P.FIRST_LEAD8, P.FIRST_RANDOM):
        assert req["text_len"][i] == P.PLEN - 8
    assert req["pattern_len"][P.FULL_ROW] == P.RS and req["text_len"][P.FULL_ROW] == P.RS
    col = np.arange(P.RS)[None, :]
    for rows, nrows, key in ((pat, npat, "pattern_len"), (txt, ntxt, "text_len")):
        inside = col < req[key].astype(np.int64)[:, None]
        assert np.array_equal(rows[inside], nrows[inside]) and (rows[~inside] == 0).all() and np.isin(nrows, F.ACGTN).all()


@pytest.mark.parametrize("name", list(P.ROWS))
def test_the_caps_of_a_row(built, name):
    """The oracle's largest score, its median with pairs on both sides of it, the median plus 1 where the unit is above 1."""
    sc = P.oracle_scores(P.ROWS[name]["pen"])
    caps = P.caps_of(name)
    assert caps[0] == sc.max() and (sc > caps[1]).sum() >= 40 and (sc <= caps[1]).sum() >= 40
    u = P.unit_of(P.ROWS[name]["pen"])
    if u > 1:
        assert caps[1] + 1 in caps and (caps[1] % u != 0 or (caps[1] + 1) % u != 0)
    x, o, e = P.ROWS[name]["pen"]
    assert P.ROWS[name]["visible"] == S.can_be_visible(x, o, e)
    assert sc.max() < P.UNCAPPED


# ------------------------------------------------------------------ model against oracle
@pytest.mark.parametrize("pen", VISIBLE_PENS + [P.ROWS[n]["pen"] for n in P.MODEL_INVISIBLE], ids=str)
def test_sentinel_model_equals_the_oracle(built, pen):
    """Pair by pair, at the largest score and at the median (the model's loop is the same up to the cap, so it is run once,
    uncapped, and capped here; the oracle is run at each cap)."""
    req, pat, txt = P.batch()
    x, o, e = pen
    got = S.scores(req, pat, txt, x, o, e, P.UNCAPPED)
    assert np.array_equal(got, P.oracle_scores(pen))
    sc = np.sort(got)
    for ms in (int(sc[-1]), int(sc[len(sc) // 2])):
        res, _ = P.oracle_run(pen, ms)
        assert np.array_equal(res["score"], _capped(got, ms)) and (res["status"] == 0).all(), ms


# ------------------------------------------------------------------ oracle against the gap-affine optimum
@pytest.mark.parametrize("pen", INVISIBLE_PENS, ids=str)
def test_oracle_is_the_optimum_on_invisible_rows(built, pen):
    assert np.array_equal(P.oracle_scores(pen), P.gotoh_scores(pen))


@pytest.mark.parametrize("pen", VISIBLE_PENS, ids=str)
def test_visible_rows_see_the_sentinel(built, pen):
    """A condition on the inputs: never above the optimum, at least 16 pairs strictly below it and at least 16 equal, so that no
    row can pass while seeing nothing."""
    sc, g = P.oracle_scores(pen), P.gotoh_scores(pen)
    print(pen, "below", int((sc < g).sum()), "equal", int((sc == g).sum()))
    assert (sc <= g).all() and (sc < g).sum() >= 16 and (sc == g).sum() >= 16


def test_visibility_rule_over_the_grid(built):
    """x 1 .. 6, o 1 .. 70, e 1 .. 6 on the single-gap pairs: the oracle differs from the gap-affine optimum exactly where
    sentinel_model.visible says so for the gap lengths of the batch, and never where can_be_visible is false. The inequality
    (10 + k) * x < o + k * e alone is necessary and not sufficient (see visible())."""
    from endsfree_model import dp_scores
    from oracle import oracle
    req, pat, txt = (a[:P.N_CONSTRUCTED] for a in P.batch())
    wrong, only_necessary = [], 0
    for x in range(1, 7):
        for o in range(1, 71):
            for e in range(1, 7):
                res, _, worst = oracle.align_batch(oracle.params("wfa", P.UNCAPPED, P.RS, mismatch=x, gap_o=o, gap_e=e), req["pattern_len"],
                                                   req["text_len"], pat, txt, nthreads=8)
                g = dp_scores(req, pat, txt, x=x, o=o, e=e)
                assert worst == 0 and (res["score"] <= g).all(), (x, o, e)
                differs = bool((res["score"] != g).any())
                if differs != S.visible(x, o, e, max(P.GAPS), gaps=P.GAPS):
                    wrong.append((x, o, e, differs))
                assert not differs or S.can_be_visible(x, o, e), (x, o, e)
                only_necessary += (not differs) and any((10 + k) * x < o + k * e for k in P.GAPS)
    assert not wrong, wrong[:20]
    print("sets where the inequality holds for a gap of the batch and nothing shows:", only_necessary)
    assert only_necessary > 0


# ------------------------------------------------------------------ CIGARs on visible rows
COST_ABOVE_AN_OPTIMAL_SCORE = {(1, 9, 2): (P.LEAD14,)}        # penalty set -> pairs at the optimum whose CIGAR costs more


@pytest.mark.parametrize("pen", VISIBLE_PENS + [P.ROWS[n]["pen"] for n in P.MODEL_INVISIBLE], ids=str)
@pytest.mark.parametrize("red", [False, True])
def test_oracle_cigars(built, pen, red):
    """Every finished pair's CIGAR is a valid alignment of the two sequences inside its row. It costs more than the score where
    the pair is below the optimum, and exactly the score everywhere else but on the pairs named in COST_ABOVE_AN_OPTIMAL_SCORE:
    there the score is the optimum and the walk still passes through cells that grew from a -10 ((1,9,2), the leading
    deletion of 14 bases: score 37 = 9 + 14 * 2, CIGAR cost 46)."""
    from endsfree_model import check_cigar, rescore
    req, pat, txt = P.batch()
    x, o, e = pen
    g = P.gotoh_scores(pen)
    plain = P.oracle_scores(pen)
    for ms in (int(plain.max()), int(np.sort(plain)[len(plain) // 2])):
        res, ops = P.oracle_run(pen, ms, True, red)
        assert (res["status"] == 0).all()
        seen_below = 0
        for i in np.nonzero(res["score"] <= ms)[0]:
            b, en = int(res["begin_offset"][i]), int(res["end_offset"][i])
            plen, tlen = int(req["pattern_len"][i]), int(req["text_len"][i])
            assert 0 <= b <= en == plen + tlen <= ops.shape[1], (i, b, en)
            s = bytes(ops[i, b:en]).decode("latin-1")
            err = check_cigar(s, bytes(pat[i, :plen]), bytes(txt[i, :tlen]))
            assert err is None, (i, err, s[-40:])
            cost = rescore(s, plen, tlen, x=x, o=o, e=e)
            if res["score"][i] < g[i]:
                seen_below += 1
                assert cost > res["score"][i], (i, cost, int(res["score"][i]))
            elif i in COST_ABOVE_AN_OPTIMAL_SCORE.get(pen, ()):
                assert res["score"][i] == g[i] and cost > res["score"][i], (i, cost, int(res["score"][i]))
            else:
                assert cost == res["score"][i], (i, cost, int(res["score"][i]))
        if ms == plain.max() and S.can_be_visible(x, o, e):      # (at the median the pairs below the optimum may all be over the cap)
            assert seen_below >= 16, seen_below


# ------------------------------------------------------------------ the table against the planner
@pytest.fixture(scope="module")
def described(built):
    """{case id: [plan tokens, debug tokens, scratch bytes, kernel name]} of every case; rows that share knobs share a process."""
    out = {}
    for env in sorted({tuple(sorted(r["env"].items())) for r in P.ROWS.values()}):
        names = [n for n, r in P.ROWS.items() if tuple(sorted(r["env"].items())) == env]
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "penalty_rows.py"), "--plans"] + names,
                           env=dict(P.plan_env(dict(env)), AIM_PLAN_DEBUG="1"), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        out.update(json.loads(r.stdout))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "penalty_rows.py"), "--flag-plans"],
                       env=dict(P.plan_env({}), AIM_PLAN_DEBUG="1"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    out.update(json.loads(r.stdout))
    return out


def test_the_table_reaches_the_plans_it_names(described):
    """Kernel name, G, ring=, w32 of aim_plan_describe's line and ring_m, ring_e, wlds, unit of AIM_PLAN_DEBUG's, for every
    case (at 130 pairs, 16 GB, 256 CUs). When a planner change moves one the new tokens are printed here."""
    pinned = P.pinned_plans()
    assert set(pinned) == set(described) == ({P.case_id(c) for n in P.ROWS for c in P.cases_of(n)} |
                                             {P.flag_case_id(c) for n in P.FLAG_ROWS for c in P.flag_cases(n)})
    moved = ["%s: pinned %r, the planner says %r" % (k, pinned[k], v[:2]) for k, v in described.items() if list(pinned[k]) != v[:2]]
    assert not moved, "\n".join(moved)


def _tok(s, name):
    m = re.search(r"(?:^| )%s=(\S+)" % name, s)
    return m.group(1) if m else None


def test_the_rows_reach_the_quantities_they_are_for(described):
    d = {k: (v[0], v[1]) for k, v in described.items()}
    # the flag rows: the dual-cost set's second piece makes a 32-row M ring wherever it runs on wfa_group_kernel (and a ring=32x
    # window on wfa_wave_kernel), the ends-free sets keep their global rows' depths
    a2p = [v for k, v in d.items() if k.startswith("flag-affine2p_4_8_3-")]
    assert len(a2p) == 4 and all(" affine2p=30,1" in " " + plan for plan, _ in a2p)
    assert all(_tok(dbg, "ring_m") == "32" if plan.startswith("wfa_group_kernel") else _tok(plan, "ring").startswith("32x") for plan, dbg in a2p)
    assert any(plan.startswith("wfa_group_kernel") for plan, _ in a2p)
    ef = {k: v for k, v in d.items() if k.startswith("flag-endsfree_")}
    assert len(ef) == 8 and all(" endsfree=3,0,16,5" in " " + plan for plan, _ in ef.values())
    assert any(plan.startswith("wfa_group_kernel") and _tok(dbg, "ring_m") == "32" and _tok(dbg, "ring_e") == "16"
               for k, (plan, dbg) in ef.items() if "15_16_15" in k)
    assert any(plan.startswith("wfa_group_kernel") and _tok(dbg, "ring_m") == "32" for k, (plan, dbg) in ef.items() if "31_28_3" in k)

    def of(name, **want):
        """The cases of the row whose tokens are all as wanted."""
        return [k for k, (plan, dbg) in d.items() if k.startswith(name + "-ms") and
                all((plan.split()[0] == v) if t == "kernel" else (_tok(plan + " " + dbg, t) == v) for t, v in want.items())]
    assert of("15_16_15", kernel="wfa_group_kernel", ring_m="32", ring_e="16")
    assert of("8_4_8", ring_e="16", unit="4")
    assert len(of("31_28_3", kernel="wfa_group_kernel", ring_m="32")) == len(P.cases_of("31_28_3"))
    for name, rows in (("32_28_3", "33"), ("16_15_16", "32"), ("63_40_3", "64"), ("64_40_3", "65"), ("70_40_3", "71"), ("1_31_1", "33")):
        got = of(name, kernel="wfa_wave_kernel")
        assert len(got) == len(P.cases_of(name)) and all(_tok(d[k][0], "ring").startswith(rows + "x") for k in got), name
    assert len(of("255_200_55", ring="256x16")) == 3 and len(of("256_200_56", ring="0x0")) == 3
    assert len(of("127_100_27_w32", ring="128x16")) == 2 and len(of("128_100_28_w32", ring="0x0")) == 3
    assert all(d[k][0].endswith(" w32") for k in d if "_w32-" in k)
    assert of("6_9_3", unit="3") and of("10_15_5", unit="5", ring_e="8") and of("2_24_2", unit="2")
    assert len(of("2_24_2_unit1", unit="1")) == len(P.cases_of("2_24_2_unit1"))
    assert of("1_12_1", kernel="wfa_group_kernel", G="64") and len(of("1_12_1_wave", kernel="wfa_wave_kernel")) == 8
    assert of("1_30_1", G="64", ring_m="32", wlds="251") and of("1_30_1", G="32", ring_m="32", wlds="128")
    assert of("1_30_1_G8", G="8", ring_m="32") and of("1_30_1_G16", G="16", ring_m="32")
    for name in ("3_4_2", "3_5_1", "4_4_1"):       # one step from the lane cost sets: never a lane kernel, MAX_SCORE 5 included
        cases = [k for k in described if k.startswith(name + "-ms")]
        assert any(k.endswith("-ms5") for k in cases)
        assert all("lane" not in described[k][3] and "lane" not in described[k][0] for k in cases), name


def test_scratch_stays_below_2_gib(described):
    worst = max(((k, v) for k, v in described.items() if len(v) > 2), key=lambda kv: kv[1][2])
    print("largest aim_scratch_bytes: %s, %d bytes" % (worst[0], worst[1][2]))
    assert worst[1][2] < 2 << 30


# ------------------------------------------------------------------ the rows see what they are for
@pytest.mark.parametrize("mutation", ["absent_reads_null", "out_of_range_reads_minus_10"])
def test_mutations_of_the_sentinel_model(built, mutation):
    """A kernel that reads NULL where the reference reads -10, and one that reads -10 where the reference reads NULL: each
    changes at least one score of every visible row and none of an invisible row."""
    kw = dict(absent=S.NULL) if mutation == "absent_reads_null" else dict(out_of_range=S.ABSENT)
    req, pat, txt = P.batch()
    for pen in VISIBLE_PENS + INVISIBLE_PENS:
        x, o, e = pen
        got = S.scores(req, pat, txt, x, o, e, P.UNCAPPED, **kw)
        changed = int((got != P.oracle_scores(pen)).sum())
        print(mutation, pen, "changes", changed, "scores")
        assert (changed > 0) == S.can_be_visible(x, o, e), (pen, changed)


# ------------------------------------------------------------------ the flags that promise a minimum cost
def _line(x, o, e, rs=112, **kw):
    from aim_amd import engine
    kw.setdefault("backtrace", bool(kw.get("bidir")))
    return F.plan_line(engine.make_params("wfa", 50, rs, mismatch=x, gap_o=o, gap_e=e, **kw), 130)


FLAGS = {"AIM_FLAG_ENDSFREE": dict(ends_free=(3, 0, 16, 5)), "AIM_FLAG_AFFINE2P": dict(gap2=(20, 1)), "AIM_FLAG_WFA_BIDIR": dict(bidir=True)}


@pytest.mark.parametrize("flag", list(FLAGS))
def test_flags_are_refused_where_the_sentinel_can_show(built, flag):
    """o + e = 11 x and e = x accepted, one more refused with AIM_EINVAL and a message that names the rule, at every READ_SIZE;
    without the flag, and gap-linear, the same sets plan."""
    kw = FLAGS[flag]
    for pen, ok in (((1, 10, 1), True), ((1, 11, 1), False), ((2, 5, 2), True), ((2, 5, 3), False), ((3, 4, 1), True), ((15, 16, 15), True)):
        for rs in (8, 112, 1024, 4096):
            line = _line(*pen, rs=rs, **kw)
            if ok:
                assert not line.startswith("error"), (pen, rs, line)
            else:
                assert line.startswith("error -1: " + flag + " needs gap_o + gap_e <= 11 * mismatch and gap_e <= mismatch"), (pen, rs, line)
                assert "-10" in line
        assert not _line(*pen).startswith("error") and not _line(*pen, backtrace=True).startswith("error")
    assert not _line(2, 0, 3, linear=True).startswith("error")


def test_bidir_scope_limit_keeps_its_message(built):
    assert not _line(61, 50, 11, rs=1024, bidir=True).startswith("error")
    assert _line(62, 50, 11, rs=1024, bidir=True) == "error -1: AIM_FLAG_WFA_BIDIR needs max(x, o + e) < 62"


def test_no_penalty_set_in_use_is_refused(built):
    """The penalty sets the suite, the tools and the launch module run the three flags on, as far as they can be listed: the
    tables of the row modules, make_params' defaults, and -- a heuristic -- the source lines that set one of the flags and
    literal penalties on the same line (a call spread over several lines, or penalties passed through a dict that is not one
    of those tables, is not seen)."""
    import wfa_group_rows as W
    sets = {(p["mismatch"], p["gap_o"], p["gap_e"]) for kind in ("endsfree", "affine2p") for p in W.PENALTIES[kind]}
    sets |= {(3, 4, 1)}                                    # make_params' defaults (full_rows.FEATURES, the launchers' defaults)
    files = [os.path.join(ROOT, d, f) for d in ("tests", "tools") for f in sorted(os.listdir(os.path.join(ROOT, d))) if f.endswith(".py")]
    files.append(os.path.join(ROOT, "aim_amd", "launch.py"))
    for path in files:
        if os.path.basename(path) in ("test_penalty_rows_cpu.py", "penalty_rows.py"):
            continue
        for ln in open(path).read().splitlines():
            if not re.search(r"ends_free\s*=|gap2\s*=|bidir\s*=\s*True", ln):
                continue
            lit = {k: re.search(r"\b%s\s*=\s*(\d+)" % k, ln) for k in ("mismatch", "gap_o", "gap_e")}
            if any(lit.values()):
                sets.add(tuple(int(lit[k].group(1)) if lit[k] else d for k, d in (("mismatch", 3), ("gap_o", 4), ("gap_e", 1))))
    print(sorted(sets))
    assert len(sets) >= 2
    for x, o, e in sets:
        assert not S.can_be_visible(x, o, e), (x, o, e)
        for kw in FLAGS.values():
            assert not _line(x, o, e, **kw).startswith("error -1: AIM_FLAG") or "max(x, o + e)" in _line(x, o, e, **kw), (x, o, e)
