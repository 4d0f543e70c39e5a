"""Sequences that fill READ_SIZE (tests/full_rows.py), without a device: the builder builds what it says, the oracle does not read
behind a length (so it is a valid reference for rows without zero padding -- no algorithm needed an exception), plain models agree
with it on the full rows, the table reaches the kernels and shapes it names, and the comparison the GPU module uses catches a
kernel that drops the last column or stops an extend on a pad byte."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import full_rows as F
from conftest import ROOT

MODEL_RS = (112, 184, 1000, 1032)


def _oracle(algo, ms, rs, req, pat, txt, **kw):
    from oracle import oracle
    return oracle.align_batch(oracle.params(algo, ms, rs, **kw), req["pattern_len"], req["text_len"], pat, txt, nthreads=8)


@pytest.mark.parametrize("rs", [8, 112, 184, 1032])
def test_builder_fills_the_rows(built, rs):
    n = F.pairs_for(rs)
    req, pat, txt = F.full_row_batch(rs, n, 7, "zero")
    nreq, npat, ntxt = F.full_row_batch(rs, n, 7, "noise")
    assert np.array_equal(req, nreq) and len(req) == n
    assert [(int(a), int(b)) for a, b in zip(req["pattern_len"][:F.HEAD], req["text_len"][:F.HEAD])] == F.head_lengths(rs)
    col = np.arange(rs)[None, :]
    for rows, nrows, key in ((pat, npat, "pattern_len"), (txt, ntxt, "text_len")):
        inside = col < req[key].astype(np.int64)[:, None]
        assert np.array_equal(rows[inside], nrows[inside]) and (rows[inside] != 0).all()
        assert (rows[~inside] == 0).all() and np.isin(nrows, F.ACGTN).all()
        assert req[key][n - 1] == rs and req[key][F.IDENTICAL] == rs
    assert (req["pattern_len"] <= rs).all() and (req["text_len"] <= rs).all()
    assert np.array_equal(pat[F.IDENTICAL], txt[F.IDENTICAL])
    assert np.array_equal(pat[F.TWIN_A], pat[F.TWIN_B]) and np.array_equal(txt[F.TWIN_A], txt[F.TWIN_B])
    assert np.array_equal(pat[F.AFTER_TWINS], pat[F.TWIN_B]) and pat[F.AFTER_TWINS, 0] != txt[F.AFTER_TWINS, 0]
    assert (pat[F.A_VS_C] == ord("A")).all() and (txt[F.A_VS_C] == ord("C")).all()
    assert pat[F.N_LAST, rs - 1] == ord("N") and txt[F.N_LAST, rs - 1] == ord("N")
    same = (npat == ntxt) & (col >= req["pattern_len"].astype(np.int64)[:, None]) & (col >= req["text_len"].astype(np.int64)[:, None])
    both = (col >= req["pattern_len"].astype(np.int64)[:, None]) & (col >= req["text_len"].astype(np.int64)[:, None])
    assert same.any() and (both & ~same).any()          # pads that match across the arrays, pads that do not
    with pytest.raises(ValueError):
        F.full_row_batch(rs, F.MIN_PAIRS - 1, 7, "zero")


_ORACLE_KEYS = {}
for _fam, _rs in F.ROWS:      # rows that differ only in a knob share one oracle run
    _f = F.FAMILIES[_fam]
    _ORACLE_KEYS.setdefault((_f["algo"], tuple(sorted(_f["kw"].items())), _rs), (_fam, _rs))


@pytest.mark.parametrize("fam,rs", sorted(_ORACLE_KEYS.values()), ids=lambda v: str(v))
def test_oracle_is_padding_independent(built, fam, rs):
    """Zero and noise padding give byte-identical results and identical ops inside [begin, end), for every family and READ_SIZE
    of the table. No algorithm needed an exception."""
    zres, zops = F.oracle_row(fam, rs, "zero")
    nres, nops = F.oracle_row(fam, rs, "noise")
    assert zres.tobytes() == nres.tobytes()
    if zops is not None:
        for i in range(len(zres)):
            b, e = int(zres["begin_offset"][i]), int(zres["end_offset"][i])
            assert np.array_equal(zops[i, b:e], nops[i, b:e]), i
    req, _, _ = F.row_batch(rs, "zero")
    F.compare(nres, nops, zres, zops, req, zops is not None, idx=False)
    assert (zres["max_operations"] == req["pattern_len"] + req["text_len"]).all()


@pytest.mark.parametrize("rs", [rs for fam, rs in F.ROWS if fam == "nw_bt_733"])
def test_the_ops_row_of_a_vs_c_is_completely_full(built, rs):
    """NW with mismatch 7 > gap_i 3 + gap_d 3: 'A' * rs against 'C' * rs aligns as rs deletions plus rs insertions, 2 * rs
    operations from begin_offset 0."""
    res, ops = F.oracle_row("nw_bt_733", rs, "noise")
    r = res[F.A_VS_C]
    assert r["status"] == 0 and r["score"] == 6 * rs
    assert r["begin_offset"] == 0 and r["end_offset"] - r["begin_offset"] == 2 * rs == ops.shape[1]
    row = ops[F.A_VS_C].tobytes()
    assert row.count(b"D") == rs and row.count(b"I") == rs


@pytest.mark.parametrize("rs", MODEL_RS)
def test_models_agree_with_the_oracle_on_unaliased_full_rows(built, rs):
    """Where plen <= tlen the flat table does not alias: NW equals the plain recurrence (also with the costs apart), SWG with
    16-bit cells and uncapped WFA (with and without the reduction's CIGAR path) the three-state gap-affine DP."""
    req, pat, txt = F.full_row_batch(rs, F.MIN_PAIRS, 3, "noise")
    flat = np.nonzero(req["pattern_len"] <= req["text_len"])[0]
    assert {0, 2, 7, 8, 10, F.IDENTICAL, F.TWIN_A, F.A_VS_C, F.N_LAST, F.MIN_PAIRS - 1} <= set(flat.tolist())
    r, p, t = req[flat], np.ascontiguousarray(pat[flat]), np.ascontiguousarray(txt[flat])
    some = r["pattern_len"] > 0     # nw.c's score is the last cell its loops wrote: 0 for an empty pattern, not tlen * GAP_I
    for x, gi, gd in ((3, 4, 4), (7, 3, 3), (3, 2, 7)):
        res, _, worst = _oracle("nw", 100, rs, r, p, t, mismatch=x, gap_i=gi, gap_d=gd, backtrace=True)
        assert worst == 0 and (res["status"] == 0).all()
        assert np.array_equal(res["score"][some], F.nw_model(r, p, t, x, gi, gd)[some]) and (res["score"][~some] == 0).all()
    want = F.affine_model(r, p, t)
    cap = 4 * rs + 16
    assert want.max() <= cap and want[list(flat).index(F.IDENTICAL)] == 0
    for algo, kw in (("swg", dict(swg_cell_bytes=2)), ("swg", dict(swg_cell_bytes=2, backtrace=True)), ("wfa", dict()), ("wfa", dict(backtrace=True))):
        res, _, worst = _oracle(algo, cap, rs, r, p, t, **kw)
        assert worst == 0 and (res["status"] == 0).all(), (algo, kw)
        assert np.array_equal(res["score"][some], want[some]), (algo, kw)
        assert (res["score"][~some] == (0 if algo == "swg" else want[~some])).all(), (algo, kw)     # (swg.c: the same loops)
    # all lengths (aliased ones too) finish: worst == 0 and status 0 for NW, SWG-w16, WFA and WFA + REDUCE with CIGAR
    for algo, ms, kw in (("nw", 100, {}), ("swg", cap, dict(swg_cell_bytes=2)), ("wfa", cap, {}), ("wfa", cap, dict(reduce=True))):
        res, _, worst = _oracle(algo, ms, rs, req, pat, txt, backtrace=True, **kw)
        assert worst == 0 and (res["status"] == 0).all(), (algo, kw)


def test_flag_models_agree_on_the_head_pairs(built):
    """The models of the flagged WFA modes, on the head pairs of a full-row batch, where they must coincide: ends-free with no
    free end, dual-cost with a second piece that never wins, the banded (w32) model and BiWFA's model give the gap-affine optimum
    (= the oracle's uncapped WFA); the gap-linear model gives NW's recurrence. Free ends and a cheaper second piece only lower it."""
    import affine2p_model, bidir_model, endsfree_model, linear_model, w32_model
    rs = 112
    req, pat, txt = F.head_only(*F.full_row_batch(rs, F.MIN_PAIRS, 5, "noise"), extra=(F.IDENTICAL, F.N_LAST))
    cap = 2 * rs + 8
    want = F.affine_model(req, pat, txt)
    res, _, worst = _oracle("wfa", cap, rs, req, pat, txt)
    assert worst == 0 and np.array_equal(res["score"], want) and want.max() <= cap
    assert np.array_equal(endsfree_model.dp_scores(req, pat, txt), want)
    assert np.array_equal(affine2p_model.dp_scores(req, pat, txt, o2=4, e2=1), want)
    assert np.array_equal(w32_model.dp_scores(req, pat, txt, cap), want)
    for i in range(len(req)):
        P, T = pat[i, :req["pattern_len"][i]].tobytes().decode(), txt[i, :req["text_len"][i]].tobytes().decode()
        s, ops = bidir_model.align(P, T, max_score=cap)
        assert s == want[i] and endsfree_model.check_cigar(ops, P.encode(), T.encode()) is None, i
    lin = linear_model.dp_scores(req, pat, txt, x=2, g=3)
    assert np.array_equal(lin, F.nw_model(req, pat, txt, 2, 3, 3))
    assert np.array_equal(w32_model.dp_scores(req, pat, txt, 6 * rs, linear=True, x=2, e=3), lin)
    ef = endsfree_model.dp_scores(req, pat, txt, **{"ends_free": F.FEATURES["endsfree"]["ends_free"]})
    a2 = affine2p_model.dp_scores(req, pat, txt, o2=24, e2=1)
    assert (ef <= want).all() and (ef < want).any() and (a2 <= want).all()


@pytest.fixture(scope="module")
def plans(built):
    env = {k: v for k, v in os.environ.items() if not k.startswith("AIM_") or k == "AIM_LIB"}
    env.update(AIM_SCRATCH_GB="16", AIM_CHIP_CUS="256")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "full_rows.py"), "--plans"], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_the_table_reaches_the_kernels_and_shapes_it_names(plans):
    """aim_plan_describe of every table row (at the row's own pair count, 16 GB, 256 CUs) names the expected kernel and shape
    token. When a planner change moves an edge the new line is printed here: the row then takes the new first READ_SIZE of the
    shape it was there for."""
    moved = ["%s: expected %r, the planner says %r" % (k, F.expected_plan(k.split("/")[0], int(k.split("/")[1])), v)
             for k, v in plans.items() if not F.plan_matches(v, F.expected_plan(k.split("/")[0], int(k.split("/")[1])))]
    assert not moved, "\n".join(moved)
    assert len(plans) == len(F.ROWS)
    tokens = ("lanes_per_pair=", "wavefronts_per_pair=", "cells_per_lane=", "G=", "seq_lds=", "pack_first=")
    seen = {t for line in plans.values() for t in tokens if (" " + t) in line}
    assert seen == set(tokens)


def test_every_kernel_name_is_reached(plans):
    """kernel_name() (capi_plan.hip) lists 13 kernels; wfa_wave and nw_lane are reached through AIM_FORCE_WAVE / AIM_NO_NW_REG,
    wfa_bidir through its flag (a feature row)."""
    src = open(os.path.join(ROOT, "aim_amd", "csrc", "capi_plan.hip")).read()
    body = src[src.index("const char *kernel_name("):]
    body = body[:body.index("\n}\n")]
    import re
    names = set(re.findall(r'"(\w+_kernel)"', body))
    assert names == set(F.KERNEL_NAMES)
    reached = {line.split()[0] for line in plans.values()}
    for f, rs in F.FEATURE_ROWS:
        reached.add(F.plan_line(F.feature_params(f, rs), F.HEAD).split()[0])
    assert reached == names, sorted(names - reached)


# ------------------------------------------------------------------ the comparison catches kernels that are wrong at these edges
@pytest.mark.parametrize("rs", [112, 192])
def test_comparison_catches_a_dropped_last_column(built, rs):
    """Mutation 1: a kernel that leaves out column tlen when tlen == READ_SIZE. Its scores differ on full texts only, and
    compare() names the first of them; the unmutated model passes the same comparison."""
    req, pat, txt = F.full_row_batch(rs, F.MIN_PAIRS, 11, "noise")
    flat = np.nonzero((req["pattern_len"] <= req["text_len"]) & (req["pattern_len"] > 0))[0]
    r, p, t = req[flat], np.ascontiguousarray(pat[flat]), np.ascontiguousarray(txt[flat])
    ores, _, _ = _oracle("nw", 100, rs, r, p, t)
    good, bad = ores.copy(), ores.copy()
    good["score"] = F.nw_model(r, p, t)
    bad["score"] = F.nw_model(r, p, t, drop_last_column=True)
    F.compare(good, None, ores, None, r, False, idx=False)
    with pytest.raises(AssertionError, match="score differs at pair 0"):
        F.compare(bad, None, ores, None, r, False, idx=False)
    full = r["text_len"] == rs
    assert ((bad["score"] != ores["score"]) <= full).all() and (bad["score"] != ores["score"])[full].sum() >= 5


@pytest.mark.parametrize("pad", ["zero", "noise"])
@pytest.mark.parametrize("algo,ms", [("wfa", 400), ("nw", 100)])
def test_comparison_catches_an_extend_that_stops_on_a_pad_byte(built, algo, ms, pad):
    """Mutation 2: a kernel that finds a sequence's end by its 0 byte. With noise padding every pair but the last is wrong; with zero padding
    the full rows still are (the byte behind them is the next pair's first base), the twins among them."""
    rs = 112
    req, pat, txt = F.full_row_batch(rs, F.MIN_PAIRS, 13, pad)
    ores, oops, _ = _oracle(algo, ms, rs, req, pat, txt, backtrace=True)
    mreq, mpat, mtxt = F.extend_stops_on_zero(req, pat, txt)
    mres, mops, _ = _oracle(algo, ms, mpat.shape[1], mreq, mpat, mtxt, backtrace=True)
    with pytest.raises(AssertionError, match="differs at pair"):
        F.compare(mres, mops, ores, oops, req, True, idx=False)
    wrong = (mres["score"] != ores["score"]) | (mres["max_operations"] != ores["max_operations"])
    if pad == "noise":
        assert wrong[:-1].all()             # (nothing follows the last pair)
    else:
        assert wrong[F.TWIN_A] and wrong[F.MIN_PAIRS - 2]
        assert not wrong[F.HEAD - 2]        # (rs, 0) then (0, rs): zero padding hides the mutation on short rows
