"""The reference digests (judge r01..r06) on every kernel they reach. The judge-r06 rows on the default plan and through the host
CLI; every reference row on each distinct plan the knob list of tests/reference_rows.py gives it (the README's "none changes
results", checked against the reference's bytes rather than the oracle); and the WFA flags documented to reduce to global WFA
(AIM_FLAG_WFA_W32, ENDSFREE with zero free lengths, AFFINE2P with piece 2 = piece 1) against the same digests."""
import pytest

from conftest import judge_costs, md5
from reference_rows import (KNOBS, all_reference_rows, apply_env, distinct_plans, judge_r06_abort_cases, judge_r06_cases,
                            knob_env, plan_key, plan_line, row_id, row_input, row_oracle, row_params)
from test_gpu_parity import _host_cli

pytestmark = pytest.mark.gpu

KNOB_ENV = dict(KNOBS)


@pytest.fixture(scope="module")
def gpu(built):
    from aim_amd import capi
    import ctypes as C
    lib = capi.load()
    n = C.c_int()
    rc = lib.aim_device_count(C.byref(n))
    assert rc == 0 and n.value >= 1, "no HIP device visible: %s" % lib.aim_last_error()
    return lib


def _run(params, case):
    """(results, ops, plan line of the launch) of one row through aim_set_* on device 0."""
    from aim_amd import engine
    _, req, pat, txt = row_input(case)
    with engine.DeviceSet(1) as s:
        res, ops = s.align(params, req, pat, txt, check=False)
        return res, ops, s.plan_describe(0)


def _first_difference(case, res, ops):
    """Where a digest row's HIP results first leave the oracle's (the oracle reproduces every digest: test_oracle_golden)."""
    import numpy as np
    ores, oops, _ = row_oracle(case)
    for f in ("score", "status", "begin_offset", "end_offset"):
        bad = np.nonzero(res[f] != ores[f])[0]
        if bad.size and (f in ("score", "status") or case["backtrace"]):
            return "%s of pair %d: %d, oracle %d" % (f, bad[0], res[f][bad[0]], ores[f][bad[0]])
    if case["backtrace"]:
        for i in range(len(res)):
            b, e = int(res["begin_offset"][i]), int(res["end_offset"][i])
            if bytes(ops[i, b:e]) != bytes(oops[i, b:e]):
                return "CIGAR of pair %d" % i
    return "no pair differs from the oracle"


def _check(case, res, ops, ends_free=False):
    """None when a row's results are the reference's, else what differs. Digest rows: the md5 of the output file. Abort rows:
    the per-pair statuses equal the oracle's, and every pair without one equals the oracle."""
    import numpy as np
    from aim_amd import engine
    if "abort" not in case:
        if md5(engine.format_output(res, ops, case["backtrace"], ends_free=ends_free)) == case["output_md5"]:
            return None
        return "digest differs (" + _first_difference(case, res, ops) + ")"
    ores, oops, _ = row_oracle(case)
    if not np.array_equal(res["status"], ores["status"]):
        i = int(np.nonzero(res["status"] != ores["status"])[0][0])
        return "status of pair %d: %d, oracle %d" % (i, res["status"][i], ores["status"][i])
    for i in np.nonzero(ores["status"] == 0)[0]:
        for f in ("score", "begin_offset", "end_offset"):
            if res[f][i] != ores[f][i]:
                return "%s of pair %d: %d, oracle %d" % (f, i, res[f][i], ores[f][i])
        b, e = int(res["begin_offset"][i]), int(res["end_offset"][i])
        if bytes(ops[i, b:e]) != bytes(oops[i, b:e]):
            return "CIGAR of pair %d" % i
    return None


# ------------------------------------------------------------------ judge r06 on the default plan and through the host CLI
@pytest.mark.parametrize("case", judge_r06_cases(), ids=row_id)
def test_judge_r06_reference_digests_through_hip(gpu, case):
    from aim_amd import engine
    _, req, pat, txt = row_input(case)
    res, ops = engine.align(row_params(case), req, pat, txt)
    assert md5(engine.format_output(res, ops, case["backtrace"])) == case["output_md5"]


@pytest.mark.parametrize("case", judge_r06_abort_cases(), ids=row_id)
def test_judge_r06_abort_case_through_hip(gpu, case, tmp_path):
    """int8 SWG with CIGAR at READ_SIZE 512: HIP reports AIM_PAIR_SWG_NO_OP on exactly the oracle's pairs and equals the oracle on
    the others; the CLI prints the reference's message and exits 1 on every output path."""
    from aim_amd import capi, engine
    data, req, pat, txt = row_input(case)
    res, ops = engine.align(row_params(case), req, pat, txt, check=False)
    assert (res["status"] == capi.PAIR_SWG_NO_OP).any()
    assert _check(case, res, ops) is None
    inp, out = tmp_path / "in", tmp_path / "out"
    inp.write_bytes(data)
    for extra in ((), ("--full-ops",), ("--no-pack", "--full-ops")):
        r = _host_cli(case, inp, out, tmp_path, extra)
        assert r.returncode == 1 and case["abort"] in r.stdout, (extra, r.stdout, r.stderr)


@pytest.mark.parametrize("case", [c for c in judge_r06_cases() if c["name"].startswith("tails_")], ids=row_id)
def test_judge_r06_tail_heavy_digests_through_the_host_cli(gpu, case, tmp_path):
    """The long `tails_v1` rows (plen > 2 tlen at READ_SIZE 1248..5112: dp_group's and dp_strip's tail cells) through the drop-in
    CLI on both wire formats, and split into several batches on several host threads."""
    inp, out = tmp_path / "in", tmp_path / "out"
    inp.write_bytes(row_input(case)[0])
    batch = str(case["gen"]["n"] // 3 + 1)
    for extra in ((), ("--no-pack", "--full-ops") if case["backtrace"] else ("--no-pack",), ("--batch", batch, "--threads", "3")):
        r = _host_cli(case, inp, out, tmp_path, extra)
        assert r.returncode == 0, (extra, r.stdout, r.stderr)
        assert md5(out.read_bytes()) == case["output_md5"], extra


# ------------------------------------------------------------------ every reference row on every kernel it reaches
@pytest.mark.parametrize("case", all_reference_rows(), ids=row_id)
def test_reference_row_on_every_kernel_it_reaches(gpu, case, monkeypatch):
    """One launch per distinct plan of the knob list (settings that plan alike run once; settings that cannot plan are left
    out). The launch must follow the plan it was given -- so a knob the library stopped honouring cannot quietly re-run the
    default -- and its output must be the reference's. All failing (knobs, plan) pairs of the row are reported together."""
    plans = distinct_plans(monkeypatch, case)
    assert plans, "no knob setting plans %s" % case["name"]
    failures = []
    for names, key in plans:
        apply_env(monkeypatch, knob_env(KNOB_ENV[names[0]]))
        res, ops, launched = _run(row_params(case), case)
        if plan_key(launched) != key:
            failures.append("%s: planned %s, launched %s" % ("/".join(names), key, plan_key(launched)))
            continue
        why = _check(case, res, ops)
        if why:
            failures.append("%s: %s: %s" % ("/".join(names), key, why))
    assert not failures, "%d of %d plans of %s are wrong:\n  %s" % (len(failures), len(plans), case["name"],
                                                                      "\n  ".join(failures))


# ------------------------------------------------------------------ WFA flags that must reduce to global WFA
WFA_ROWS = [c for c in all_reference_rows() if c["algo"] == "wfa"]


def _variants():
    """(row, variant, knob name): W32 on every WFA row; ENDSFREE (0, 0, 0, 0) and AFFINE2P with piece 2 = piece 1 on the rows
    without REDUCE (neither combines with it), on the default plan and on wfa_wave."""
    out = [pytest.param(c, "w32", "default", id=c["name"] + "-w32") for c in WFA_ROWS]
    for c in WFA_ROWS:
        if not c.get("reduce"):
            for v in ("endsfree0", "affine2p_eq"):
                for k in ("default", "AIM_FORCE_WAVE"):
                    out.append(pytest.param(c, v, k, id="%s-%s-%s" % (c["name"], v, k)))
    return out


@pytest.mark.parametrize("case,variant,knob", _variants())
def test_wfa_flags_that_reduce_to_global_wfa_match_the_reference_digests(gpu, case, variant, knob, monkeypatch):
    """AIM_FLAG_WFA_W32 below READ_SIZE 32 760, ENDSFREE with four zero free lengths and AFFINE2P with (gap_o2, gap_e2) =
    (gap_o, gap_e) are documented to give global WFA's bytes (include/aim_hip.h), so they give the reference's digests."""
    from aim_amd import capi, engine
    c = judge_costs(case)
    extra = {"w32": dict(w32=True), "endsfree0": dict(ends_free=(0, 0, 0, 0)),
             "affine2p_eq": dict(gap2=(c.get("gap_o", 4), c.get("gap_e", 1)))}[variant]
    need = {"w32": capi.FEATURE_WFA_W32, "endsfree0": capi.FEATURE_ENDSFREE, "affine2p_eq": capi.FEATURE_AFFINE2P}[variant]
    assert engine.features() & need
    apply_env(monkeypatch, knob_env(KNOB_ENV[knob]))
    params = row_params(case, **extra)
    rc, planned = plan_line(params, case["gen"]["n"])
    assert rc == 0, planned
    res, ops, launched = _run(params, case)
    assert plan_key(launched) == plan_key(planned)
    if knob == "AIM_FORCE_WAVE" or variant == "w32":
        assert launched.startswith("wfa_wave_kernel"), launched
    why = _check(case, res, ops, ends_free=variant == "endsfree0")
    assert why is None, "%s on %s: %s" % (variant, launched, why)
