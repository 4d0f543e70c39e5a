"""Low-complexity inputs (tests/low_complexity.py), without a device: the builder builds what it says; the batches leave most pairs
under every row's cap with something to align; the oracle, which the reference cannot pin on such inputs, agrees with models it
shares no code with and does not read behind a length; the inputs tell the six NW traceback tie orders apart in every repeat
class; and the MAX_SCORE 10 rows plan on the lane kernels."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import full_rows as F
import low_complexity as L
from conftest import ROOT

MODEL_MAX_RS = 184


# ------------------------------------------------------------------ the builder
@pytest.mark.parametrize("rs", [8, 16, 40, 112, 1032])
@pytest.mark.parametrize("ms", [5, 100])
def test_builder_builds_the_classes(built, rs, ms):
    n = F.pairs_for(rs)
    req, pat, txt, cls, light = L.low_complexity_batch(rs, n, 7, ms, "zero")
    nreq, npat, ntxt, _, _ = L.low_complexity_batch(rs, n, 7, ms, "noise")
    assert len(req) == n and np.array_equal(req, nreq) and req["idx"][0] != 0 and np.array_equal(np.diff(req["idx"]), np.ones(n - 1))
    assert np.array_equal(cls, np.arange(n) % 9) and len(L.CLASSES) == 9 == len(L.CLASSES_DOC)
    col = np.arange(rs)[None, :]
    for rows, nrows, key in ((pat, npat, "pattern_len"), (txt, ntxt, "text_len")):
        inside = col < req[key].astype(np.int64)[:, None]
        assert np.array_equal(rows[inside], nrows[inside]) and np.isin(rows[inside], F.ACGTN).all()
        assert (rows[~inside] == 0).all() and np.isin(nrows, F.ACGTN).all()
        assert (req[key] >= 1).all() and (req[key] <= rs).all()
    longer = np.maximum(req["pattern_len"], req["text_len"]).astype(np.int64)
    rounds = np.arange(n) // 9
    full = rounds % 4 == 3
    l = max(1, (rs - 8) * 100 // 104)
    assert (longer[full] == rs).all() and (longer[~full] == l).all()
    assert np.array_equal(light, np.array([L.round_is_light(r, ms) for r in rounds]))
    for r4 in range(0, rounds.max() - 2, 4):        # whole blocks of four rounds
        assert sum(L.round_is_light(r, ms) for r in range(r4, r4 + 4)) == (3 if ms <= 10 else 2)
    # the light form: one substitution, one 1-base indel or nothing
    d = req["text_len"].astype(np.int64) - req["pattern_len"]
    assert (np.abs(d[light]) <= 1).all()
    for i in np.nonzero(light & (d == 0))[0]:
        assert (pat[i] != txt[i]).sum() <= 1
    # the same pair in the same form, whatever the cap
    oreq, opat, otxt, _, olight = L.low_complexity_batch(rs, n, 7, 105 - ms, "zero")
    same = light == olight
    assert same.any() and (~same).any()
    assert np.array_equal(pat[same], opat[same]) and np.array_equal(txt[same], otxt[same]) and np.array_equal(req[same], oreq[same])
    assert not np.array_equal(pat, L.low_complexity_batch(rs, n, 8, ms, "zero")[1])
    with pytest.raises(ValueError):
        L.low_complexity_batch(rs, n, 7, ms, "ones")


def _runs(s):
    """[(byte, length)] of the runs of equal bytes."""
    edge = np.flatnonzero(np.r_[True, s[1:] != s[:-1], True])
    return [(int(s[a]), int(b - a)) for a, b in zip(edge[:-1], edge[1:])]


@pytest.mark.parametrize("rs", [16, 112, 544])
def test_builder_classes_are_what_they_say(built, rs):
    """The heavy forms, class by class (l is large enough at READ_SIZE 112 and 544 for no clamp but l // 3 and l // 2 to act)."""
    n = 130
    req, pat, txt, cls, light = L.low_complexity_batch(rs, n, 11, 100, "zero")
    seen = set()
    for i in np.nonzero(~light)[0]:
        p, t = pat[i, :req["pattern_len"][i]], txt[i, :req["text_len"][i]]
        lo, hi = (p, t) if len(p) <= len(t) else (t, p)
        Lh, d, name = len(hi), len(hi) - len(lo), L.CLASSES[cls[i]]
        seen.add(name)
        if name == "homo_len":
            assert len(set(hi.tolist())) == 1 and set(lo.tolist()) == set(hi.tolist()) and d <= 3
        elif name == "homo_foreign":
            assert d == 0 and all(np.bincount(s).max() == Lh - 1 for s in (p, t))
        elif name == "dinuc":
            assert 1 <= d <= 3 and hi[0] != hi[1] and np.array_equal(hi, L._tandem(hi[:2], Lh))
        elif name == "tandem_copy":
            assert d in (3, 5, 7, 13, 17, 31, 33) or d == max(1, Lh // 3)
            assert np.array_equal(hi, L._tandem(hi[:d], Lh)) and np.array_equal(lo, hi[:Lh - d])
        elif name == "tandem_rot":
            assert d == 0 and any(np.array_equal(t, np.roll(p, -k)) for k in (1, 2, 3))
        elif name == "tandem_sub":
            assert d == 0 and (p != t).sum() == max(1, Lh // 100)
            assert any(np.array_equal(p, L._tandem(p[:u], Lh)) for u in (3, 4, 6, 11, 16, 32, max(1, Lh // 3)))
        elif name == "homo_island":
            assert 1 <= d <= 3 or Lh < 24
            assert max(k for _, k in _runs(hi)) >= min(12, Lh // 2) and max(k for _, k in _runs(hi)) <= 40 + 3
        elif name == "two_letter":
            assert d == 1 and set(p.tolist()) | set(t.tolist()) <= {ord("A"), ord("T")}
            assert Lh < 40 or (hi == ord("A")).mean() > 0.6
        elif name == "n_run":
            nr = [k for b, k in _runs(hi) if b == ord("N")]
            assert d == 1 and len(nr) == 1 and min(4, Lh // 2) <= nr[0] <= 19
            assert (lo == ord("N")).sum() == nr[0] - 1 and (lo != ord("N")).sum() == (hi != ord("N")).sum()
    assert seen == set(L.CLASSES)


# ------------------------------------------------------------------ coverage conditions
def _uncapped(fam, rs):
    """NW has no cap of its own; the launcher's rule gives it MAX_SCORE 4 at READ_SIZE 40, where a row is then judged by
    status 0 and a non-zero score alone."""
    return L.FAMILIES[fam]["algo"] == "nw" and L.FAMILIES[fam]["ms"](rs) < 5


_COVER_ROWS = [(fam, rs) for fam, rs in L.ROWS if L.FAMILIES[fam]["ms"](rs) >= 5 or _uncapped(fam, rs)]
_EXEMPT = sorted({rs for fam, rs in L.ROWS if (fam, rs) not in _COVER_ROWS and L.FAMILIES[fam]["algo"] != "genasm"})


def test_rows_exempt_from_the_coverage_conditions():
    """Rows whose MAX_SCORE is below 5 are exempt: one gap already costs 5, so nothing but substitutions could be under the cap.
    These are the READ_SIZE 8 and 16 rows of the WFA families, and GenASM, whose MAX_SCORE is 0 by definition. The NW rows at
    READ_SIZE 40 stay in (_uncapped)."""
    assert _EXEMPT == [8, 16]
    assert [rs for fam, rs in _COVER_ROWS if _uncapped(fam, rs)] == [40, 40]


@pytest.mark.parametrize("fam,rs", _COVER_ROWS, ids=lambda v: str(v))
def test_batches_leave_most_pairs_under_the_cap(built, fam, rs):
    """Conditions on the inputs, judged by the oracle's results alone: at least 75 % of the pairs end with status 0 and a score
    within MAX_SCORE, at least 50 % do so with a non-zero score, and in rows of 130 pairs every class has three such pairs."""
    ms = L.FAMILIES[fam]["ms"](rs)
    req, _, _, cls, _ = L.row_batch(fam, rs)
    res, _ = L.oracle_row(fam, rs)
    ok = (res["status"] == 0) & ((res["score"] <= ms) | _uncapped(fam, rs))
    nz = ok & (res["score"] != 0)
    per = [int(nz[cls == c].sum()) for c in range(len(L.CLASSES))]
    print("%s/%d MAX_SCORE %d: within the cap %.2f, and non-zero %.2f, per class %s" % (fam, rs, ms, ok.mean(), nz.mean(), per))
    assert ok.mean() >= 0.75 and nz.mean() >= 0.50
    if len(req) == 130:
        assert min(per) >= 3, per


# ------------------------------------------------------------------ the oracle against models
def _cigar(res, ops, i):
    return bytes(ops[i, int(res["begin_offset"][i]):int(res["end_offset"][i])]).decode()


def check_against_models(algo, params, req, pat, txt, res, ops):
    """The oracle's (or a kernel's) results of one batch against the plain models; returns how many pairs each check saw.
    Left out of the score and CIGAR checks: WFA pairs over the cap (no traceback exists); SWG pairs whose optimum is above
    MAX_SCORE, and every pair of an int8 SWG row whose cells can wrap; and, for NW and SWG, the pairs with plen > tlen on which
    the flat table's aliasing changes the score ('aliased' in the result). Measured on the rows up to READ_SIZE 184: 32 to 36
    of a row's 130 pairs have plen > tlen, and the aliasing changes 0 to 2 of them, all with plen - tlen = 3 and an optimum that
    does not end in deletions; the others, the heavy length-changing pairs among them, are held to the models like the rest."""
    from aim_amd import capi
    from endsfree_model import check_cigar, rescore
    from test_genasm import _check_alignment
    n = len(req)
    done = res["status"] == 0
    flat = req["pattern_len"] <= req["text_len"]
    seen = dict(score=0, cigar=0)
    if algo == "nw":
        x, gi, gd = params.mismatch, params.gap_i, params.gap_d
        want = F.nw_model(req, pat, txt, x, gi, gd)
        assert done.all()
        assert np.array_equal(res["score"][flat], want[flat]), np.nonzero(flat & (res["score"] != want))[0][:5]
        cost = lambda s, pl, tl: s.count("X") * x + s.count("I") * gi + s.count("D") * gd
        # Beyond plen <= tlen the flat table aliases, the oracle's own definition (nw.c:67-153): a column past tlen + 1 reads its
        # insertion and diagonal predecessors from the current row. The walk is held to the model wherever the score still is.
        walked = flat | (res["score"] == want)
        seen["score"], seen["aliased"] = int(walked.sum()), int((~walked).sum())
    elif algo == "genasm":
        assert done.all()
        assert (res["score"] >= F.nw_model(req, pat, txt, 1, 1, 1)).all()
        seen["score"] = n
        if ops is not None:
            _check_alignment(req, pat, txt, res, ops)
        cost = lambda s, pl, tl: len(s) - s.count("M")
        walked = done
    else:
        want = F.affine_model(req, pat, txt, params.mismatch, params.gap_o, params.gap_e)
        if algo == "wfa":          # over the cap the oracle stops at MAX_SCORE + 1, status 0 and no traceback (wfa.c:368-376)
            within = done & (res["score"] <= params.max_score)
            assert (res["score"][done & ~within] == params.max_score + 1).all()
            if params.flags & capi.FLAG_REDUCE:
                assert (res["score"][within] >= want[within]).all()
            else:
                assert np.array_equal(within, want <= params.max_score), np.nonzero(within != (want <= params.max_score))[0][:5]
                assert np.array_equal(res["score"][within], want[within])
            seen["score"] = int(within.sum())
        else:                  # SWG: its flat table aliases like NW's, and MAX_SCORE is its infinity (swg.c:45-171: the borders' I / D cells hold
            # MAX_SCORE itself), so a pair whose optimum is above the cap gets a smaller score and a walk that does not re-score to it
            # With 8-bit cells (no SWG_W16, MAX_SCORE < 127) a cell wraps on store once it passes 127; the model holds where none can.
            w8 = not (params.flags & capi.FLAG_SWG_W16) and params.max_score < 127
            wraps = w8 and max(params.max_score, params.gap_o + params.read_size * params.gap_e) + params.gap_o + params.gap_e > 127
            seen["wraps"] = wraps
            capped = done & (want <= params.max_score) & (not wraps)
            under = capped & (flat | (res["score"] == want))          # (plen > tlen: as for NW)
            assert np.array_equal(res["score"][under], want[under]), np.nonzero(under & (res["score"] != want))[0][:5]
            seen["score"] = int(under.sum())
            seen["aliased"] = int((capped & ~under).sum())
        cost = lambda s, pl, tl: rescore(s, pl, tl, params.mismatch, params.gap_o, params.gap_e)
        walked = under if algo == "swg" else within
    if ops is not None:
        for i in np.nonzero(walked)[0]:
            pl, tl = int(req["pattern_len"][i]), int(req["text_len"][i])
            s = _cigar(res, ops, i)
            assert res["max_operations"][i] == pl + tl
            assert check_cigar(s, bytes(pat[i, :pl]), bytes(txt[i, :tl])) is None, (i, s)
            assert cost(s, pl, tl) == res["score"][i], (i, s, int(res["score"][i]))
        seen["cigar"] = int(np.count_nonzero(walked))
    return seen


_MODEL_KEYS = {}
for _fam, _rs in L.ROWS:      # rows that differ only in a knob share one oracle run and one model
    _f = L.FAMILIES[_fam]
    if _rs <= MODEL_MAX_RS:
        _MODEL_KEYS.setdefault((_f["algo"], _f["ms"](_rs), tuple(sorted(_f["kw"].items())), _rs), (_fam, _rs))


@pytest.mark.parametrize("fam,rs", sorted(_MODEL_KEYS.values()), ids=lambda v: str(v))
def test_oracle_agrees_with_the_models(built, fam, rs):
    """Every row up to READ_SIZE 184. NW's score is the plain recurrence where plen <= tlen (beyond that the flat table aliases:
    the oracle's own definition); WFA without the reduction and SWG with 16-bit cells give the gap-affine optimum within the
    cap, and WFA finishes exactly the pairs whose optimum is within it; WFA with the reduction never goes below the optimum;
    GenASM never below the edit distance. Every CIGAR uses up both sequences truthfully and re-scores to the reported score."""
    req, pat, txt, _, _ = L.row_batch(fam, rs)
    res, ops = L.oracle_row(fam, rs)
    seen = check_against_models(L.FAMILIES[fam]["algo"], L.row_params(fam, rs), req, pat, txt, res, ops)
    print("%s/%d: %s" % (fam, rs, seen))
    if seen.get("wraps"):
        assert fam == "swg8_bt" and rs > 40 and seen["score"] == 0
    elif L.FAMILIES[fam]["algo"] != "wfa" or L.FAMILIES[fam]["ms"](rs) >= 5:      # (WFA at MAX_SCORE 1 and 2 finishes few pairs)
        assert seen["score"] >= len(req) // 3 and (ops is None or seen["cigar"] >= len(req) // 3), seen


@pytest.mark.parametrize("fam", ["nw_bt", "nw_bt_733", "swg16_bt", "wfa2_bt", "wfa2_red_bt", "genasm_bt"])
def test_oracle_agrees_with_the_models_at_1024(built, fam):
    """One light and one heavy pair of each class at READ_SIZE 1024."""
    rs = 1024
    req, pat, txt, _, _ = L.one_of_each(rs, L.SEED)
    params = L.row_params(fam, rs)
    algo = L.FAMILIES[fam]["algo"]
    res, ops, _ = L.oracle_of(params, algo, req, pat, txt)
    seen = check_against_models(algo, params, req, pat, txt, res, ops)
    assert seen["score"] >= 6 and seen["cigar"] >= 6, seen


@pytest.mark.parametrize("fam,rs", sorted(_MODEL_KEYS.values()) + [("nw_bt", 1024), ("swg16_bt", 1024), ("wfa2_red_bt", 3000), ("genasm_bt", 1000)],
                         ids=lambda v: str(v))
def test_oracle_is_padding_independent(built, fam, rs):
    """Zero and noise padding give byte-identical results and identical ops inside [begin, end)."""
    zres, zops = L.oracle_row(fam, rs, "zero")
    nres, nops = L.oracle_row(fam, rs, "noise")
    assert zres.tobytes() == nres.tobytes()
    req = L.row_batch(fam, rs)[0]
    F.compare(nres, nops, zres, zops, req, zops is not None, idx=False)
    if zops is not None:
        for i in range(len(zres)):
            b, e = int(zres["begin_offset"][i]), int(zres["end_offset"][i])
            assert np.array_equal(zops[i, b:e], nops[i, b:e]), i
    assert (zres["max_operations"] == req["pattern_len"] + req["text_len"]).all()


# ------------------------------------------------------------------ tie orders
TIE_CLASSES = ("homo_len", "dinuc", "tandem_copy", "homo_island")


def _changed_by_order(req, pat, txt, res, ops, order, costs):
    """Pairs with plen <= tlen whose ops under `order` differ from the oracle's."""
    out = []
    for i in np.nonzero(req["pattern_len"] <= req["text_len"])[0]:
        p, t = pat[i, :req["pattern_len"][i]], txt[i, :req["text_len"][i]]
        if L.nw_traceback(p, t, order, *costs) != bytes(ops[i, int(res["begin_offset"][i]):int(res["end_offset"][i])]):
            out.append(int(i))
    return out


TIE_COSTS = ((3, 4, 4), (7, 3, 3))


@pytest.fixture(scope="module")
def tie_rows(built):
    """READ_SIZE 112: the low-complexity batch of the nw_bt row and the random body of its full-row batch, with the oracle's
    results under the default costs and under mismatch 7 / gaps 3 + 3 (nw_bt_733's)."""
    from aim_amd import engine
    from oracle import oracle
    rs = 112
    req, pat, txt, cls, _ = L.row_batch("nw_bt", rs)
    breq, bpat, btxt = engine.gen_pairs(F.SEED, 0, F.pairs_for(rs) - F.MIN_PAIRS, (rs - 8) * 100 // 104, 0.02, rs)
    out = {}
    for x, gi, gd in TIE_COSTS:
        op = oracle.params("nw", L.FAMILIES["nw_bt"]["ms"](rs), rs, mismatch=x, gap_i=gi, gap_d=gd, backtrace=True)
        out[(x, gi, gd)] = tuple(oracle.align_batch(op, r["pattern_len"], r["text_len"], p, t, nthreads=8)[:2]
                                 for r, p, t in ((req, pat, txt), (breq, bpat, btxt)))
    return (req, pat, txt, cls), (breq, bpat, btxt), out


def test_the_oracle_order_reproduces_the_oracle(tie_rows):
    """A plain NW traceback with the order among deletion, insertion and diagonal as a parameter: with aim_oracle.c's order
    (deletion, insertion, diagonal) it reproduces the oracle's ops on every pair with plen <= tlen, low-complexity and random,
    under both cost sets."""
    (req, pat, txt, _), (breq, bpat, btxt), oracles = tie_rows
    for costs, ((res, ops), (bres, bops)) in oracles.items():
        assert (res["status"] == 0).all() and (bres["status"] == 0).all()
        assert _changed_by_order(req, pat, txt, res, ops, L.ORACLE_ORDER, costs) == []
        assert _changed_by_order(breq, bpat, btxt, bres, bops, L.ORACLE_ORDER, costs) == []


@pytest.mark.parametrize("order", [o for o in L.ORDERS if o != L.ORACLE_ORDER])
def test_the_inputs_tell_tie_orders_apart(tie_rows, order):
    """Each of the other five orders changes the ops of at least one pair in each of homo_len, dinuc, tandem_copy and
    homo_island: an indel inside a run of equal bases costs the same at either end of the run, and preferring the gap or the
    diagonal picks different ends. Asserted per cost set: 'DMI', 'MDI' and 'MID' separate the four classes at 3 / 4 / 4, the
    costs the kernels run by default, and all five orders do at 7 / 3 / 3. Under 3 / 4 / 4, on pairs with plen <= tlen, the place of the deletion in the order hardly matters: 'IDM' differs from the oracle's
    'DIM' only at a cell that a deletion and an insertion both explain, and between two runs of one base the table is
    GAP * |h - v|, where exactly one of them does (measured: 'IDM' changes 0 of 95 pairs, 'IMD' 1; 'DMI', 'MDI' and 'MID' 20
    each, in every class). With mismatch 7 > 3 + 3 a foreign base is aligned as a deletion plus an insertion, whose order is such
    a tie ('IDM' then changes 25 of 95 pairs, the others 28 to 60). The random body of the full-row batch of the same row is
    counted for the record (3 / 4 / 4: 'DMI' 30, 'IDM' 0, 'IMD' 7, 'MDI' 34, 'MID' 34 of 68 pairs): random pairs at 2 % edits
    have indels next to an equal base often enough to tell gap-first from diagonal-first, but not a class of repeats apart."""
    (req, pat, txt, cls), (breq, bpat, btxt), oracles = tie_rows
    for costs, ((res, ops), (bres, bops)) in oracles.items():
        changed = _changed_by_order(req, pat, txt, res, ops, order, costs)
        per = {c: sum(1 for i in changed if L.CLASSES[cls[i]] == c) for c in L.CLASSES}
        random_changed = _changed_by_order(breq, bpat, btxt, bres, bops, order, costs)
        print("order %s, costs %s: %d of %d low-complexity pairs change %s; %d of %d random pairs" % (
            order, costs, len(changed), int((req["pattern_len"] <= req["text_len"]).sum()), per, len(random_changed),
            int((breq["pattern_len"] <= breq["text_len"]).sum())))
        # per cost set, what holds there: the orders that move the diagonal against a gap separate all four classes at the
        # default costs already; every order does at 7 / 3 / 3
        if costs == (7, 3, 3) or order in ("DMI", "MDI", "MID"):
            for c in TIE_CLASSES:
                assert per[c] >= 1, (order, costs, c, per)
        else:
            assert order in ("IDM", "IMD") and len(changed) <= 1, (order, costs, changed)


# ------------------------------------------------------------------ planner
def test_wfa10_rows_plan_on_the_lane_kernels(built):
    """aim_plan_describe of the MAX_SCORE 10 rows under the planner settings of test_full_rows_cpu.py (16 GB, 256 CUs)."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("AIM_") or k == "AIM_LIB"}
    env.update(AIM_SCRATCH_GB="16", AIM_CHIP_CUS="256")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "low_complexity.py"), "--plans"], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    plans = json.loads(r.stdout)
    assert len(plans) == len(L.WFA10_ROWS) == 8
    moved = ["%s: expected %r, the planner says %r" % (k, L.expected_plan(k.split("/")[0], int(k.split("/")[1])), v)
             for k, v in plans.items() if not F.plan_matches(v, L.expected_plan(k.split("/")[0], int(k.split("/")[1])))]
    assert not moved, "\n".join(moved)
    assert {v.split()[0] for v in plans.values()} == {"wfa_lane_kernel", "wfa_lane_packed_kernel"}
    assert L.ROWS[:len(F.ROWS)] == F.ROWS and L.TABLE["wfa5"] is F.TABLE["wfa5"]
