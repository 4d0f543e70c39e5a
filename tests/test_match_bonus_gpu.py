"""SWG with a match bonus (tests/match_bonus.py) on the GPU: every table row against the oracle pair by pair and, where the cells
fit their type, against the int64 model; NW, WFA and GenASM, which ignore `match`; the RES8 / REQ8 / packed / compact transports,
the selection flags and SAM_FIELDS over negative scores; the host program; and the planner and poison knobs.
tests/test_match_bonus_cpu.py holds the oracle to the model first, and shows that these batches tell a kernel that drops,
misplaces or partly forgets the bonus from a right one."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import full_rows as F
import match_bonus as B
from conftest import ROOT

pytestmark = pytest.mark.gpu

SCORE_FAILED = -2 ** 31          # AIM_SCORE_FAILED


@pytest.fixture(scope="module")
def gpu(built):
    import ctypes as C
    from aim_amd import capi
    lib = capi.load()
    n = C.c_int()
    assert lib.aim_device_count(C.byref(n)) == 0 and n.value >= 1, lib.aim_last_error()
    return lib


# ------------------------------------------------------------------ every row
def _row_against_the_oracle(fam, rs, pad):
    req, _, _ = F.row_batch(rs, pad)
    res, ops, line, todo = B.align_row(fam, rs, pad)
    print("%s/%d %s: %s; to-do list %d of %d pairs; %d scores negative" % (fam, rs, pad, line, todo, len(req), (res["score"] < 0).sum()))
    assert F.plan_matches(line, B.expected_plan(fam, rs)), line
    ores, oops = B.oracle_row(fam, rs, pad)
    F.compare(res, ops, ores, oops, req, B.FAMILIES[fam]["backtrace"])
    assert todo == B.expected_todo(fam, rs), (todo, B.expected_todo(fam, rs))
    return res


@pytest.mark.parametrize("fam,rs", B.ROWS, ids=lambda v: str(v))
def test_rows_match_the_oracle(gpu, fam, rs):
    """Every pair of the row's batch: score, max_operations, end_offset and status, and with CIGAR begin_offset and the ops bytes
    of [begin_offset, end_offset); the plan line names the row's kernel and shape, and the to-do list holds the row's pinned
    number of pairs. On the rows whose cells fit their type the scores of the unaliased pairs are also the int64 model's, so a
    reading of swg.c that the oracle and a kernel shared could not hide."""
    res = _row_against_the_oracle(fam, rs, "zero")
    if (fam, rs) in B.FITTING:
        sel, score, _, _ = B.model_row(fam, rs)
        bad = np.nonzero(res["score"][sel] != score)[0]
        assert bad.size == 0, "pair %d: got %d, model %d" % (sel[bad[0]], res["score"][sel[bad[0]]], score[bad[0]])
        assert res["score"][F.IDENTICAL] == B.FAMILIES[fam]["costs"][0] * rs


def _noise_rows():
    """The first row of each kernel, and of dp_wave's three regimes: the row scan (edge 1032), the literal path without a wrap
    (1072) and with one (1096)."""
    first = {}
    for fam, rs in B.ROWS:
        first.setdefault(B.expected_plan(fam, rs).split()[0], (fam, rs))
    return sorted(set(first.values()) | {("edge_bt", 1032), ("edge_bt", 1072), ("edge_bt", 1096)})


@pytest.mark.parametrize("fam,rs", _noise_rows(), ids=lambda v: str(v))
def test_rows_with_noise_padding(gpu, fam, rs):
    """Seeded A/C/G/T/N behind every length instead of zeros; same plan, same to-do count."""
    _row_against_the_oracle(fam, rs, "noise")


# ------------------------------------------------------------------ match is inert where the reference ignores it
INERT = [("nw", 104, "nw_reg_kernel"), ("nw_bt", 104, "nw_reg_kernel"), ("nw", 1024, "dp_group_kernel"), ("nw_bt", 1024, "dp_group_kernel"),
         ("nw", 1800, "dp_strip_kernel"), ("nw_bt", 1288, "dp_strip_kernel"), ("wfa2", 112, "wfa_group_kernel"), ("wfa2_bt", 112, "wfa_group_kernel"),
         ("wfa2", 1024, "wfa_group_kernel"), ("wfa2_bt", 1024, "wfa_group_kernel"), ("wfa5", 112, "wfa_lane_kernel"),
         ("wfa5_bt", 112, "wfa_lane_kernel"), ("wfa_wave", 544, "wfa_wave_kernel"), ("wfa_wave_red_bt", 544, "wfa_wave_kernel"),
         ("genasm", 128, "genasm_wave_kernel"), ("genasm_bt", 128, "genasm_wave_kernel")]


def _no_budget(line):
    return re.sub(r" budget=\d+", "", line)      # (the bound follows the device's free memory at configure time)


@pytest.mark.parametrize("fam,rs,kernel", INERT, ids=lambda v: str(v))
def test_match_is_inert_where_the_reference_ignores_it(gpu, fam, rs, kernel):
    """nw.c adds a literal 0 on equal bases, WFA and GenASM have no match cost at all: match = -2 gives the result bytes, the ops
    bytes inside [begin_offset, end_offset) and the plan line of match = 0 (whose results test_full_rows_gpu.py holds to the
    oracle), on the register, group, strip, lane and wave kernels."""
    from aim_amd import engine
    f = F.FAMILIES[fam]
    req, pat, txt = F.row_batch(rs, "noise")
    got = []
    F._with_env(f["env"])
    try:
        for match in (0, -2):
            params = engine.make_params(f["algo"], f["ms"](rs), rs, match=match, **f["kw"])
            with engine.DeviceSet(1) as s:
                res, ops = s.align(params, req, pat, txt, check=False)
                line = s.plan_describe(0)
            if ops is not None:
                col = np.arange(ops.shape[1])[None, :]
                ops = np.where((col >= res["begin_offset"][:, None]) & (col < res["end_offset"][:, None]), ops, 0)
            got.append((res.tobytes(), None if ops is None else ops.tobytes(), _no_budget(line)))
    finally:
        F._without_env(f["env"])
    assert got[0][2].split()[0] == kernel, got[0][2]
    assert got[1][2] == got[0][2]
    assert got[1][0] == got[0][0] and got[1][1] == got[0][1]


# ------------------------------------------------------------------ result layouts
def _oracle_of(params, req, pat, txt):
    return B.oracle_of(params, req, pat, txt)


@pytest.mark.parametrize("rs", [136, 1024])
def test_req8_res8_carry_negative_scores(gpu, rs):
    """{idx, score} rows (RES8) return every negative score as it is -- the score field is shared with AIM_SCORE_FAILED
    (INT32_MIN), which no finished pair reads -- and 8-byte requests (REQ8) change nothing, on swg_lane (136) and dp_group (1024)."""
    from aim_amd import engine
    req, pat, txt = F.row_batch(rs, "noise")
    ores, _, _ = _oracle_of(B.row_params("a16", rs), req, pat, txt)
    assert (ores["status"] == 0).all() and 4 * (ores["score"] < 0).sum() >= len(req)
    for req8, res8 in ((True, True), (True, False), (False, True)):
        res, _ = engine.align(B.row_params("a16", rs, req8=req8, res8=res8), req, pat, txt, check=False)
        assert np.array_equal(res["idx"], req["idx"])
        if res8:
            assert res.dtype.names == ("idx", "score")
            assert np.array_equal(res["score"], ores["score"]) and (res["score"] != SCORE_FAILED).all()
        else:
            F.compare(res, None, ores, None, req, False)
    bres, bops = engine.align(B.row_params("a16_bt", rs, req8=True), req, pat, txt, check=False)
    ores, oops, _ = _oracle_of(B.row_params("a16_bt", rs), req, pat, txt)
    F.compare(bres, bops, ores, oops, req, True)


@pytest.mark.parametrize("rs", [136, 1024])
def test_packed_input_and_compact_runs(gpu, rs):
    """aim_set_submit with 2-bit packed rows (the N pair travels raw) and device-side run lists: results equal the oracle's, the
    run lists' headers carry the negative scores and print the CIGAR the ops rows print ('M' runs are what the bonus pays for)."""
    from aim_amd import engine
    req, pat, txt = F.row_batch(rs, "noise")
    n = len(req)
    params = B.row_params("a16_bt", rs)
    ores, oops = B.oracle_row("a16_bt", rs, "noise")
    assert (ores["status"] == 0).all()
    packed = engine.pack_batch(req, pat, txt)
    assert F.N_LAST in packed[2].tolist() and len(packed[2]) < n // 2
    with engine.DeviceSet(1) as s:
        s.configure_slots(params, n, slots=2, max_raw=n, max_runs=n * 2 * rs)
        s.submit(0, 0, req, packed=packed, want_ops=True)
        out = s.wait(0, 0, check=False)
        F.compare(out["res"], out["ops"], ores, oops, req, True)
        want = engine.format_output(out["res"], out["ops"], True)
        for slot, pk in ((1, None), (0, packed)):
            if pk is None:
                s.submit(0, slot, req, pat, txt, cigar_runs_cap=n * 2 * rs, want_ops=True)
            else:
                s.submit(0, slot, req, packed=pk, cigar_runs_cap=n * 2 * rs, want_ops=True)
            out = s.wait(0, slot, check=False)
            F.compare(out["res"], out["ops"], ores, oops, req, True)
            assert np.array_equal(out["cig"]["score"], ores["score"]) and np.array_equal(out["cig"]["idx"], req["idx"])
            assert np.array_equal(out["cig"]["status"], ores["status"].astype(np.uint16))
            assert engine.format_output_runs(out["cig"], out["runs"]) == want


# ------------------------------------------------------------------ selection over negative scores
@pytest.fixture(scope="module")
def sel_batch(gpu):
    return B.selection_batch()


def _sel_sizes():
    return B.model_max_score(B.COSTS_A)(B.SEL_RS), B.SEL_RS


SEL_MODES = [dict(backtrace=True), dict(res8=True)]          # full rows with ops and run lists; {idx, score} rows


@pytest.mark.parametrize("mode", SEL_MODES, ids=["cigar", "res8"])
def test_read_groups_over_negative_scores(gpu, sel_batch, mode):
    """aim_best_t (winner, runner-up score, tie count) equals read_groups_model on the flag-less scores, the returned rows, ops and
    run lists are the winner's flag-less ones -- over reads whose best score is negative (ties at it included), reads with only
    positive scores, and runner-ups of either sign."""
    import test_read_groups_gpu as rg
    from aim_amd import engine
    ref, req, rows, offs, tpos, txt, pats, kinds = sel_batch
    ms, rs = _sel_sizes()
    kw = B.selection_kw(**mode)
    bt = bool(mode.get("backtrace"))
    runs_cap = 256 * len(req) if bt else 0
    exp = rg.expected("swg", ms, rs, kw, req, pats, txt, offs, runs_cap=runs_cap)
    got = rg.run_groups(engine.make_params("swg", ms, rs, read_groups=True, ref_texts=True, **kw), req, rows, offs, tpos=tpos, ref=ref, runs_cap=runs_cap)
    assert got["plan"].endswith(" groups=1")
    rg.assert_groups_equal(got, exp, bt, bt)
    best = exp["best"]
    assert np.array_equal(got["res"]["score"], best["best_score"]) and (got["res"]["score"] != SCORE_FAILED).all()
    assert (best["best_score"][kinds != 2] < 0).all() and (best["best_score"][kinds == 2] > 0).all() and (kinds == 2).sum() > 30
    assert (best["n_best"][kinds == 1] >= 2).all() and ((best["n_best"] >= 2) & (best["best_score"] < 0)).sum() > 60
    assert ((best["second_score"] < 0) & (best["second_score"] > best["best_score"])).sum() > 60 and (best["second_score"] > 0).sum() > 30


@pytest.mark.parametrize("mode", SEL_MODES, ids=["cigar", "res8"])
@pytest.mark.parametrize("max_hits", [1, 3, 8])
def test_top_hits_over_negative_scores(gpu, sel_batch, max_hits, mode):
    """hit_pair equals top_hits_model on the flag-less scores (the order key must sort negative below positive), each hit row is
    the candidate's flag-less row, and aim_best_t is unchanged."""
    import test_top_hits_gpu as th
    from aim_amd import engine
    ref, req, rows, offs, tpos, txt, pats, kinds = sel_batch
    ms, rs = _sel_sizes()
    kw = B.selection_kw(**mode)
    bt = bool(mode.get("backtrace"))
    runs_cap = 256 * len(req) if bt else 0
    exp = th.expected(("match_bonus", "swg", bt), "swg", ms, rs, kw, req, pats, txt, offs, runs_cap=runs_cap)
    got = th.run_hits(engine.make_params("swg", ms, rs, read_groups=True, top_hits=True, ref_texts=True, **kw), max_hits, req, rows, offs, tpos=tpos,
                      ref=ref, runs_cap=runs_cap)
    assert got["plan"].endswith(" groups=1 hits=1")
    hoff, hit_pair = th.assert_hits_equal(got, exp, offs, max_hits, bt, bt)
    assert int(hoff[-1]) == int(np.minimum(np.diff(offs.astype(np.int64)), max_hits).sum())
    s = exp["res1"]["score"][hit_pair].astype(np.int64)          # ascending inside every read; with all 6..8 hits both signs in most reads
    assert all((np.diff(s[hoff[r]:hoff[r + 1]]) >= 0).all() for r in range(len(offs) - 1))
    if max_hits == 8:
        assert sum(1 for r in range(len(offs) - 1) if s[hoff[r]] < 0 < s[hoff[r + 1] - 1]) > 100


@pytest.mark.parametrize("mode", SEL_MODES, ids=["cigar", "res8"])
def test_mate_pairs_over_negative_sums(gpu, sel_batch, mode):
    """aim_mate_t (cost, runner-up cost, tie count, the pair) equals mate_pairs_model on the flag-less scores: proper pairs of
    negative cost, and read pairs that stay unpaired at best + best + unpaired_penalty, below 0 in some of them."""
    import test_mate_pairs_gpu as mp
    from aim_amd import engine
    ref, req, rows, offs, tpos, txt, pats, kinds = sel_batch
    ms, rs = _sel_sizes()
    kw = B.selection_kw(**mode)
    bt = bool(mode.get("backtrace"))
    mates = (340, 460, 10)
    runs_cap = 256 * len(req) if bt else 0
    exp = mp.expected("swg", ms, rs, kw, req, pats, txt, offs, tpos, mates, runs_cap=runs_cap)
    got = mp.run_mates(engine.make_params("swg", ms, rs, read_groups=True, ref_texts=True, mate_pairs=True, **kw), req, rows, offs, tpos, ref, mates,
                       runs_cap=runs_cap)
    assert got["plan"].endswith(" groups=1 mates=1")
    mp.assert_mates_equal(got, exp, bt, bt)
    proper = (exp["mates"]["flags"] & 1) != 0
    cost = exp["mates"]["score_sum"]
    print("%d read pairs: proper %d, unpaired %d (%d of them below 0), choice moved by the mate in %d" % (
        len(proper), proper.sum(), (~proper).sum(), ((~proper) & (cost < 0)).sum(), mp._differs(exp).sum()))
    assert proper.sum() > 60 and (cost[proper] < 0).all() and (exp["mates"]["n_best"][proper] >= 2).sum() > 10
    assert ((~proper) & (cost < 0)).sum() >= 5 and ((~proper) & (cost > 0)).sum() >= 5
    assert mp._differs(exp).sum() >= 5


def test_sam_fields_of_the_winners(gpu, sel_batch):
    """AIM_FLAG_SAM_FIELDS with READ_GROUPS: the records of the winners (POS, CIGAR, NM and MD come from the ops) equal
    tests/sam_model.py on the flag-less rows, and carry the negative scores."""
    import test_sam_fields_gpu as S
    ref, req, rows, offs, tpos, txt, pats, kinds = sel_batch
    ms, rs = _sel_sizes()
    out0, out1, exps, _ = S.both(B.selection_kw(read_groups=True), ms, rs, "swg", ref, req, rows, tpos, read_offsets=offs)
    assert len(exps[0]) == len(offs) - 1
    assert (out1[0]["sam"]["score"][kinds != 2] < 0).all() and (out1[0]["sam"]["score"][kinds == 2] > 0).all()


# ------------------------------------------------------------------ the host program
def _cli_input(tmp_path):
    from aim_amd import engine
    ms, rs = engine.launcher_sizes("swg", 100, 0.02, mismatch=5, gap_o=2, gap_e=3)
    req, pat, txt = engine.gen_pairs(4242, 0, 200, 100, 0.02, rs)
    inp = tmp_path / "in.seq"
    inp.write_bytes(engine.pairs_to_text(req, pat, txt))
    return inp, ms, rs


@pytest.mark.parametrize("w16", [True, False], ids=["int16", "int8"])
@pytest.mark.parametrize("bt", [False, True], ids=["score", "cigar"])
def test_host_cli_with_a_match_bonus(gpu, tmp_path, bt, w16):
    """`host --algo swg --match -2 --mismatch 5 --gap-o 2 --gap-e 3` writes the bytes oracle_cli writes with -m -2 -x 5 -g 2 -a 3,
    with int16 cells and with the launchers' int8 cells (MAX_SCORE 10 < 127, where -2 * 100 wraps by design: the two programs
    then agree on the exit status, and on the bytes when it is 0)."""
    inp, ms, rs = _cli_input(tmp_path)
    host = [os.path.join(ROOT, "aim_amd", "host", "host"), str(inp), str(tmp_path / "h.out"), "200", "--algo", "swg", "--max-score", str(ms),
            "--read-size", str(rs), "--nr-dpus", "1", "--match", "-2", "--mismatch", "5", "--gap-o", "2", "--gap-e", "3"]
    cli = [os.path.join(ROOT, "oracle", "oracle_cli"), "swg", "-i", str(inp), "-o", str(tmp_path / "o.out"), "-n", "200", "-l", "100", "-e", "0.02",
           "-d", "1", "-m", "-2", "-x", "5", "-g", "2", "-a", "3"]
    rh = subprocess.run(host + (["--backtrace"] if bt else []) + (["--swg-w16"] if w16 else []), capture_output=True, text=True, cwd=tmp_path, timeout=120)
    ro = subprocess.run(cli + (["-b"] if bt else []) + (["--swg-cell", "2"] if w16 else []), capture_output=True, text=True, cwd=tmp_path, timeout=120)
    assert (rh.returncode == 0) == (ro.returncode == 0), rh.stdout[-1000:] + rh.stderr[-1000:] + ro.stdout[-500:] + ro.stderr[-500:]
    if w16:
        assert ro.returncode == 0
    if ro.returncode == 0:
        data = (tmp_path / "o.out").read_bytes()
        assert (tmp_path / "h.out").read_bytes() == data
        scores = [int(line.split(b",")[1]) for line in data.split(b"\n") if b"," in line]
        assert len(scores) == 200 and (not w16 or sum(s < 0 for s in scores) == 200)


def test_launcher_passes_the_bonus_through(gpu, tmp_path):
    """`python -m aim_amd.launch swg -m -2 -x 5 -g 2 -a 3 --mram -b` reaches the same output."""
    inp, ms, rs = _cli_input(tmp_path)
    common = ["-i", str(inp), "-l", "100", "-e", "0.02", "-n", "200", "-d", "1", "-b", "-m", "-2", "-x", "5", "-g", "2", "-a", "3"]
    rh = subprocess.run([sys.executable, "-m", "aim_amd.launch", "swg", "-o", str(tmp_path / "h.out"), "--mram"] + common, capture_output=True, text=True,
                        cwd=tmp_path, env=dict(os.environ, PYTHONPATH=ROOT), timeout=120)
    ro = subprocess.run([os.path.join(ROOT, "oracle", "oracle_cli"), "swg", "-o", str(tmp_path / "o.out"), "--swg-cell", "2"] + common, capture_output=True,
                        text=True, cwd=tmp_path, timeout=120)
    assert rh.returncode == 0 and ro.returncode == 0, rh.stdout[-1000:] + rh.stderr[-1000:] + ro.stderr[-500:]
    assert "-DMATCH=-2" in rh.stdout
    assert (tmp_path / "h.out").read_bytes() == (tmp_path / "o.out").read_bytes()


# ------------------------------------------------------------------ knobs
KNOB_ROWS = ["a16/136", "a16_bt/136", "a16/184", "a16_bt/184", "a16/1024", "a16_bt/1024"]
_LANE, _GROUP, _STRIP, _WAVE = "swg_lane_kernel", "dp_group_kernel", "dp_strip_kernel", "dp_wave_kernel"
_DEFAULT = {136: _LANE, 184: _GROUP, 1024: _GROUP}
# (environment, the kernel each READ_SIZE then plans on, a token the READ_SIZE 1024 line then holds)
KNOBS = [({"AIM_NO_DP_GROUP": "1"}, {136: _LANE, 184: _LANE, 1024: _STRIP}, "cells_per_lane=20"),
         ({"AIM_FORCE_DPWAVE": "1"}, {136: _STRIP, 184: _STRIP, 1024: _STRIP}, "cells_per_lane=20"),
         ({"AIM_DPW_LEGACY": "1"}, {136: _LANE, 184: _LANE, 1024: _WAVE}, "wavefronts_per_pair=2"),
         ({"AIM_STRIP_K": "32"}, {136: _LANE, 184: _LANE, 1024: _STRIP}, "cells_per_lane=32"),
         ({"AIM_DEBUG_POISON_SCRATCH": "0"}, _DEFAULT, "lanes_per_pair=32"), ({"AIM_DEBUG_POISON_SCRATCH": "255"}, _DEFAULT, "lanes_per_pair=32"),
         ({"AIM_DEBUG_POISON_LDS": "0"}, _DEFAULT, "lanes_per_pair=32"), ({"AIM_DEBUG_POISON_LDS": "255"}, _DEFAULT, "lanes_per_pair=32")]


def _align_in_a_process(tmp_path, name, env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("AIM_") or k == "AIM_LIB"}
    e.update(env)
    out = str(tmp_path / (name + ".npz"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "match_bonus.py"), "--align", out] + KNOB_ROWS, env=e, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    return np.load(out)


def _plan_of(npz, key):
    return npz[key + "/plan"].tobytes().decode()


@pytest.fixture(scope="module")
def default_knobs(gpu, tmp_path_factory):
    """The knob rows in a process with no knob set: the table's plans and the oracle's results."""
    got = _align_in_a_process(tmp_path_factory.mktemp("knobs"), "default", {})
    for key in KNOB_ROWS:
        fam, rs = key.split("/")
        assert F.plan_matches(_plan_of(got, key), B.expected_plan(fam, int(rs))), _plan_of(got, key)
        ores, oops = B.oracle_row(fam, int(rs))
        assert np.array_equal(got[key + "/res"]["score"], ores["score"]), key
    return got


@pytest.mark.parametrize("env,kernels,token", KNOBS, ids=["+".join("%s=%s" % kv for kv in k[0].items()) for k in KNOBS])
def test_knobs_change_the_plan_and_nothing_else(gpu, default_knobs, tmp_path, env, kernels, token):
    """The (-1, 3, 4, 1) rows at READ_SIZE 136, 184 and 1024, score-only and with CIGAR, in a process of their own per setting:
    the plan names the kernel the knob asks for, results and the ops bytes inside [begin_offset, end_offset) are byte-equal to
    the default process's."""
    got = _align_in_a_process(tmp_path, "knob", env)
    assert sorted(got.files) == sorted(default_knobs.files)
    for key in KNOB_ROWS:
        rs = int(key.split("/")[1])
        line = _plan_of(got, key)
        assert line.split()[0] == kernels[rs], (key, line)
        if rs == 1024:
            assert token in line.split(), (key, line)
        assert (line.split()[0] != _plan_of(default_knobs, key).split()[0]) == (kernels[rs] != _DEFAULT[rs])
        assert got[key + "/res"].tobytes() == default_knobs[key + "/res"].tobytes(), key
        if key + "/ops" in got.files:
            assert got[key + "/ops"].tobytes() == default_knobs[key + "/ops"].tobytes(), key
