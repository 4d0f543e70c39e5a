"""WFA across penalty sets on the GPU (tests/penalty_rows.py): every row of the table through engine.DeviceSet -- configure, push,
launch, pull -- under the plan line its table entry names, every per-pair output against the oracle (score, max_operations, begin
and end offsets, status and every ops byte), and the to-do list's length. The rows where the reference's -10 is visible promise
the reference's bytes: a score that can lie below the cost of the CIGAR printed next to it. Rows that need environment knobs run
in a process of their own. tests/test_penalty_rows_cpu.py shows that the table reaches what it names, that the oracle is the
reference's rule on these sets and that these rows would see a kernel that reads NULL for -10 or -10 for NULL."""
import os
import subprocess
import sys

import numpy as np
import pytest

import full_rows as F
import penalty_rows as P
from conftest import ROOT

pytestmark = pytest.mark.gpu
KINDS = ("score", "cigar")


@pytest.fixture(scope="module")
def gpu(built):
    import ctypes as C
    from aim_amd import capi
    lib = capi.load()
    n = C.c_int()
    assert lib.aim_device_count(C.byref(n)) == 0 and n.value >= 1, lib.aim_last_error()
    return lib


def _worker(tmp_path, env, kind, names, pad="zero"):
    out = str(tmp_path / "out.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "penalty_rows.py"), "--run", out, pad, kind] + list(names),
                       env=P.run_env(env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-3000:]
    z = np.load(out)
    return {f: z[f] for f in z.files}


def _run(monkeypatch, tmp_path, name, kind):
    env = P.ROWS[name]["env"]
    if env:
        return _worker(tmp_path, env, kind, [name])
    for k in [k for k in os.environ if k.startswith("AIM_") and k != "AIM_LIB"]:
        monkeypatch.delenv(k)
    return P.run_rows([name], bt=kind == "cigar")


def _cases(name, kind):
    return [c for c in P.cases_of(name) if c[2] == (kind == "cigar")]


ROW_CASES = [(name, kind) for name in P.ROWS for kind in KINDS if _cases(name, kind)]


@pytest.mark.parametrize("name,kind", ROW_CASES, ids=lambda v: str(v))
def test_rows(gpu, monkeypatch, tmp_path, name, kind):
    """One row of the table, without (score) or with BACKTRACE (cigar), with and without REDUCE, at every MAX_SCORE of the row:
    the oracle's largest score of the batch, its median (about half the pairs come back at MAX_SCORE + 1), the median plus 1 where
    the set's unit is above 1, and the row's extra caps."""
    out = _run(monkeypatch, tmp_path, name, kind)
    for case in _cases(name, kind):
        P.check_case(case, out)


@pytest.mark.parametrize("kind", KINDS)
def test_w32_equals_the_flagless_run(gpu, monkeypatch, tmp_path, kind):
    """(1,12,1) with AIM_FLAG_WFA_W32: every result row and every ops byte equal to the flag-less run's."""
    from wfa_group_rows import same_bytes
    a = _run(monkeypatch, tmp_path, "1_12_1", kind)
    b = _run(monkeypatch, tmp_path, "1_12_1_w32", kind)
    for case in _cases("1_12_1_w32", kind):
        k, k0 = P.case_id(case), P.case_id(("1_12_1",) + case[1:])
        same_bytes((a[k0 + "/res"], a.get(k0 + "/ops")), (b[k + "/res"], b.get(k + "/ops")))


POISON = {"AIM_CHIP_CUS": "1", "AIM_DEBUG_POISON_SCRATCH": "165", "AIM_DEBUG_POISON_LDS": "90"}


@pytest.mark.parametrize("name", ["1_30_1", "15_16_15"])
@pytest.mark.parametrize("kind", KINDS)
def test_deepest_rings_on_one_cu_with_poisoned_lds_and_scratch(gpu, tmp_path, name, kind):
    """The 32-row M ring (and the 16-row I / D ring) with LDS and scratch filled with a byte pattern at kernel entry and every
    workgroup on one CU, so that each reuses LDS another has left: a ring that is one row too shallow reads a stale row."""
    out = _worker(tmp_path, POISON, kind, [name])
    for case in _cases(name, kind):
        P.check_case(case, out, pinned=False)


def test_fused_runs_equal_the_rle_of_the_ops_rows(gpu, monkeypatch):
    """(1,12,1) with compact CIGAR output: the run lists wfa_group_tb_kernel writes itself (runs_out=1) are the run-length
    encoding of the ops rows the same batch gives through push / pull, and both are the oracle's."""
    from aim_amd import engine
    from endsfree_model import runs_of
    from oracle import oracle
    for k in [k for k in os.environ if k.startswith("AIM_") and k != "AIM_LIB"]:
        monkeypatch.delenv(k)
    req, pat, txt = P.batch()
    n = len(req)
    for case in [c for c in P.cases_of("1_12_1") if c[2] and c[1] != 620]:
        params = P.case_params(case)
        res, ops, _, _ = P.align(params, req, pat, txt)
        with engine.DeviceSet(1) as s:
            s.configure_slots(params, n, slots=1, max_raw=n, max_runs=2 * P.RS * n)
            s.submit(0, 0, req, packed=engine.pack_batch(req, pat, txt), cigar_runs_cap=2 * P.RS * n)
            out = s.wait(0, 0, check=False)
            line = s.plan_describe(0)
        print(P.case_id(case), line)
        assert line.startswith("wfa_group_kernel") and " runs_out=1" in line, line
        cig, runs = out["cig"], out["runs"]
        ores, oops = P.oracle_run(P.ROWS["1_12_1"]["pen"], case[1], True, case[3])
        assert np.array_equal(cig["score"], ores["score"]) and np.array_equal(cig["idx"], req["idx"]) and (cig["status"] == 0).all()
        want = ores.copy()
        want["idx"] = req["idx"]
        assert engine.format_output_runs(cig, runs) == engine.format_output(res, ops, True) == oracle.format_output(want, oops, True)
        for i in range(n):
            b, e = int(res["begin_offset"][i]), int(res["end_offset"][i])
            assert int(cig["n_runs"][i]) == len(runs_of(bytes(ops[i, b:e]).decode("latin-1"))), i


@pytest.mark.parametrize("name", ["4_4_1", "1_30_1", "1_31_1"])
@pytest.mark.parametrize("kind", KINDS)
def test_rows_with_noise_behind_the_lengths(gpu, tmp_path, name, kind):
    """The same batch with seeded A / C / G / T / N bytes behind every length instead of zeros, on the narrow widths that stage
    their rows in LDS in 16-byte chunks (4_4_1: G = 2 to 8), on the 32-row ring and on wfa_wave_kernel: an extend that ran past
    a length would keep matching there."""
    out = _worker(tmp_path, {}, kind, [name], pad="noise")
    for case in _cases(name, kind):
        P.check_case(case, out, pad="noise")


# ------------------------------------------------------------------ the flags that promise a minimum cost, on deep invisible sets
# (AIM_FLAG_WFA_BIDIR at its scope limit, (61,50,11) at READ_SIZE 1024, has no row here: see DESIGN.md, "Penalty sets")
@pytest.mark.parametrize("name", list(P.FLAG_ROWS))
@pytest.mark.parametrize("bt", [False, True], ids=["score", "cigar"])
def test_flags_on_deep_invisible_sets(gpu, monkeypatch, name, bt):
    """penalty_rows.FLAG_ROWS under the plan the table pins: scores equal the flag's DP model, capped, at the model's largest
    score and at its median; with BACKTRACE every CIGAR is valid and costs its score (wfa_group_rows.check_variant)."""
    import wfa_group_rows as W
    for k in [k for k in os.environ if k.startswith("AIM_") and k != "AIM_LIB"]:
        monkeypatch.delenv(k)
    req, pat, txt = P.batch()
    kind, pen = P.FLAG_ROWS[name]
    pd = dict(mismatch=pen[0], gap_o=pen[1], gap_e=pen[2])
    want = P.flag_scores(name)
    glob = P.gotoh_scores(pen)
    assert (want <= glob).all() and (want < glob).sum() >= 8          # the flag changes scores on this batch
    for case in [c for c in P.flag_cases(name) if c[2] == bt]:
        res, ops, line, todo = P.align(P.flag_params(case), req, pat, txt)
        print(P.flag_case_id(case), line)
        pinned = P.pinned_plans()[P.flag_case_id(case)][0]
        assert F.plan_matches(line, pinned), "ran under %r, the table says %r" % (line, pinned)
        W.check_variant(kind, pd, case[1], req, pat, txt, res, ops, bt, want, ends_free=P.FLAG_ENDS_FREE, gap2=P.FLAG_GAP2)
