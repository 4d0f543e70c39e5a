"""AIM_FLAG_WFA_ESCALATE, what needs no GPU: the premise on the CPU oracle (a pair of score <= c has the same result row and ops bytes
under cap c as under a larger cap; a pair reported c + 1 at cap c scores over c), the feature bit, every refusal through the library,
make_params and the host binary, the plan lines, the scratch, the selection kernels' code objects and the launcher."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

LANE_PENALTIES = [(3, 4, 1), (4, 6, 2), (2, 3, 1), (5, 4, 2)]   # wfa_lane.hpp AIM_LANE_COST_SETS
CAPS = [4, 5, 6, 8, 10]
FULL = 40


def _batches(sample_bytes):
    from aim_amd import engine
    rs = 112
    out = {}
    for e in (0.01, 0.02, 0.05, 0.10):
        out["e=%g" % e] = engine.gen_pairs(5, 0, 600, 100, e, rs)
    out["sample"] = engine.parse_pairs(b"\n".join(sample_bytes.split(b"\n")[:2000]) + b"\n", rs)
    out["mixed"] = engine.mixed_pairs(6, 1500, 100, 0.01, 0.05, 0.2, rs)[:3]
    return rs, out


@pytest.mark.parametrize("pen", LANE_PENALTIES, ids=lambda p: "%d-%d-%d" % p)
@pytest.mark.parametrize("reduce", [False, True], ids=["exact", "reduce"])
@pytest.mark.parametrize("bt", [False, True], ids=["score", "cigar"])
def test_premise_on_the_oracle(built, sample_bytes, pen, reduce, bt):
    from oracle import oracle
    x, o, e = pen
    rs, batches = _batches(sample_bytes)
    for name, (req, pat, txt) in batches.items():
        run = lambda cap: oracle.align_batch(oracle.params("wfa", cap, rs, mismatch=x, gap_o=o, gap_e=e, backtrace=bt, reduce=reduce),
                                             req["pattern_len"], req["text_len"], pat, txt, nthreads=4)
        full, fops, _ = run(FULL)
        for c in CAPS:
            low, lops, _ = run(c)
            keep = full["score"] <= c
            # A: final at the low cap
            assert np.array_equal(low[keep], full[keep]), (name, c)
            if bt:
                cols = np.arange(2 * rs)[None, :]
                inside = (cols >= full["begin_offset"][:, None]) & (cols < full["end_offset"][:, None]) & keep[:, None]
                assert np.array_equal(lops[inside], fops[inside]), (name, c)
            # B: what the low cap reports as c + 1 is over c at the full cap (and nothing else is)
            assert np.array_equal(low["score"] == c + 1, full["score"] > c), (name, c)


# ---- the library ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(built):
    from aim_amd import capi
    return capi.load()


@pytest.fixture()
def fixed_chip(monkeypatch):
    monkeypatch.setenv("AIM_SCRATCH_GB", "16")
    monkeypatch.setenv("AIM_CHIP_CUS", "256")


def _describe(lib, params, n=2048):
    from aim_amd import capi
    buf = C.create_string_buffer(1024)
    rc = lib.aim_plan_describe(capi.params_ref(params), n, buf, len(buf))
    return rc, buf.value.decode() if rc == 0 else lib.aim_last_error().decode()


def _validate(lib, params):
    from aim_amd import capi
    rc = lib.aim_scratch_bytes(capi.params_ref(params), 1000)
    return rc, lib.aim_last_error().decode() if rc == 0 else ""


def _esc(p):
    from aim_amd import capi
    base = p.base if hasattr(p, "base") else p
    base.flags |= capi.FLAG_WFA_ESCALATE
    return p


def test_features_bit_and_constants(lib):
    from aim_amd import capi, engine
    assert capi.FLAG_WFA_ESCALATE == 0x1000 and capi.FEATURE_WFA_ESCALATE == 0x80
    assert engine.features() & capi.FEATURE_WFA_ESCALATE
    assert engine.features() & capi.FEATURE_READ_GROUPS
    assert lib.aim_abi_version() == 2
    hdr = open(__import__("os").path.join(__import__("conftest").ROOT, "include", "aim_hip.h")).read()
    assert "#define AIM_FLAG_WFA_ESCALATE 0x1000u" in hdr and "#define AIM_FEATURE_WFA_ESCALATE 0x80u" in hdr


def test_rejections(lib):
    from aim_amd import engine
    for algo in ("nw", "swg", "genasm"):
        assert _validate(lib, _esc(engine.make_params(algo, 25, 112))) == (0, "AIM_FLAG_WFA_ESCALATE needs AIM_ALGO_WFA"), algo
    for kw, name in ((dict(ends_free=(0, 0, 10, 10)), "AIM_FLAG_ENDSFREE"), (dict(gap2=(24, 1)), "AIM_FLAG_AFFINE2P"), (dict(linear=True), "AIM_FLAG_LINEAR"),
                     (dict(w32=True), "AIM_FLAG_WFA_W32"), (dict(backtrace=True, bidir=True), "AIM_FLAG_WFA_BIDIR"),
                     (dict(read_groups=True), "AIM_FLAG_READ_GROUPS (a follow-up)")):
        assert _validate(lib, _esc(engine.make_params("wfa", 25, 112, **kw))) == (0, "AIM_FLAG_WFA_ESCALATE cannot be combined with %s" % name), kw
    for kw in (dict(), dict(reduce=True), dict(backtrace=True), dict(req8=True, res8=True), dict(ref_texts=True), dict(backtrace=True, reduce=True, req8=True)):
        assert _validate(lib, engine.make_params("wfa", 25, 112, escalate=True, **kw))[0] > 0, kw


def test_make_params_escalate():
    from aim_amd import capi, engine
    assert engine.make_params("wfa", 25, 112, escalate=True).flags == capi.FLAG_WFA_ESCALATE
    assert engine.make_params("wfa", 25, 112, escalate=True, backtrace=True, reduce=True).flags == capi.FLAG_WFA_ESCALATE | capi.FLAG_BACKTRACE | capi.FLAG_REDUCE
    assert engine.make_params("wfa", 25, 112).flags == 0
    with pytest.raises(ValueError, match="escalate needs wfa"):
        engine.make_params("nw", 25, 112, escalate=True)
    for kw in (dict(ends_free=(1, 2, 3, 4)), dict(gap2=(24, 1)), dict(linear=True), dict(w32=True), dict(backtrace=True, bidir=True), dict(read_groups=True)):
        with pytest.raises(ValueError, match="escalate cannot be combined with"):
            engine.make_params("wfa", 25, 112, escalate=True, **kw)


def _lane_cap(lib, ms, rs, **kw):
    """c by its definition, from flag-less plan lines only: the largest cap below MAX_SCORE whose flag-less plan is a lane plan"""
    from aim_amd import engine
    for c in range(ms - 1, 0, -1):
        rc, line = _describe(lib, engine.make_params("wfa", c, rs, **kw))
        assert rc == 0
        if line.startswith("wfa_lane_kernel ") or line.startswith("wfa_lane_packed_kernel "):
            return c, line
    return 0, None


@pytest.mark.parametrize("kw", [dict(), dict(reduce=True), dict(backtrace=True), dict(req8=True, res8=True), dict(mismatch=4, gap_o=6, gap_e=2),
                                dict(mismatch=4, gap_o=6, gap_e=2, backtrace=True), dict(mismatch=2, gap_o=3, gap_e=1), dict(mismatch=5, gap_o=4, gap_e=2)],
                         ids=lambda k: ",".join("%s=%s" % i for i in k.items()) or "score")
@pytest.mark.parametrize("ms,rs", [(25, 112), (25, 80), (30, 168)])
def test_two_stage_plan_line(lib, fixed_chip, kw, ms, rs):
    from aim_amd import capi, engine
    c, line1 = _lane_cap(lib, ms, rs, **kw)
    rc, full = _describe(lib, engine.make_params("wfa", ms, rs, **kw))
    assert rc == 0 and c > 0 and not full.startswith("wfa_lane")
    p = engine.make_params("wfa", ms, rs, escalate=True, **kw)
    rc, line = _describe(lib, p)
    assert rc == 0, line
    # (stage 2 plans under the budget stage 1 leaves: the lines are compared without their budget= fields)
    key = lambda l: re.sub(r" budget=\d+", "", l)
    assert key(line) == key("%s | %s escalate=%d" % (line1, full, c)), line
    assert lib.aim_kernel_name(capi.params_ref(p)).decode() == line1.split()[0]
    # aim_scratch_bytes covers both stages and the list
    scratch = lambda l: int(l.split(" scratch=")[1].split()[0])
    assert lib.aim_scratch_bytes(capi.params_ref(p), 2048) >= scratch(line1) + scratch(full) + 4 * (16 + 2048)


def test_the_caps_of_the_default_penalties(lib, fixed_chip):
    """(3, 4, 1), MAX_SCORE 25, READ_SIZE 112: score-only runs the dynamic lane shape at cap 10 first. With CIGAR the planner takes caps
    6..10 on wfa_lane_packed_kernel behind pack_rows_kernel, so the first stage's cap is 10 there too (wfa_lane_kernel itself stops at 5)."""
    from aim_amd import engine
    rc, line = _describe(lib, engine.make_params("wfa", 25, 112, escalate=True))
    assert rc == 0 and line.startswith("wfa_lane_kernel ") and " | wfa_group_kernel " in line and line.endswith(" escalate=10"), line
    rc, line = _describe(lib, engine.make_params("wfa", 25, 112, escalate=True, backtrace=True))
    assert rc == 0 and line.startswith("wfa_lane_packed_kernel ") and " | wfa_group_kernel " in line and line.endswith(" escalate=10"), line
    rc, line = _describe(lib, engine.make_params("wfa", 6, 112, escalate=True, mismatch=7, gap_o=2, gap_e=1))   # no lane kernel for these penalties
    assert rc == 0 and line.endswith(" escalate=0"), line


@pytest.mark.parametrize("ms,rs,kw", [(5, 112, dict()), (10, 112, dict()), (5, 112, dict(backtrace=True)), (250, 1056, dict()), (250, 1056, dict(backtrace=True)),
                                      (1, 112, dict())])
def test_one_stage_plan_line(lib, fixed_chip, ms, rs, kw):
    """a lane plan already, or no lane kernel for the shape (l = 1000): the flag-less line and " escalate=0", the flag-less scratch"""
    from aim_amd import capi, engine
    p0, p = engine.make_params("wfa", ms, rs, **kw), engine.make_params("wfa", ms, rs, escalate=True, **kw)
    rc, full = _describe(lib, p0)
    assert (rc, full + " escalate=0") == _describe(lib, p)
    assert lib.aim_scratch_bytes(capi.params_ref(p0), 2048) == lib.aim_scratch_bytes(capi.params_ref(p), 2048)


def test_plan_debug_prints_the_line(built, fixed_chip):
    import os
    import sys
    code = ("import ctypes as C\nfrom aim_amd import capi, engine\nlib = capi.load()\nb = C.create_string_buffer(1024)\n"
            "p = engine.make_params('wfa', 25, 112, escalate=True)\nassert lib.aim_plan_describe(capi.params_ref(p), 2048, b, 1024) == 0\nprint(b.value.decode())\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=dict(os.environ, AIM_PLAN_DEBUG="1"),
                       cwd=__import__("conftest").ROOT)
    assert r.returncode == 0, r.stderr
    assert "[aim plan] " + r.stdout.strip() in r.stderr and r.stdout.strip().endswith(" escalate=10")


def test_no_flag_changes_nothing(lib, fixed_chip):
    from aim_amd import capi, engine
    for kw in (dict(), dict(backtrace=True)):
        p = engine.make_params("wfa", 25, 112, **kw)
        before = _describe(lib, p), lib.aim_scratch_bytes(capi.params_ref(p), 2048)
        _describe(lib, engine.make_params("wfa", 25, 112, escalate=True, **kw))
        assert (_describe(lib, p), lib.aim_scratch_bytes(capi.params_ref(p), 2048)) == before
        assert "escalate" not in before[0][1]


def test_code_objects(built):
    """The selection kernels use no scratch memory, and the to-do-input variants of wfa_group_kernel spill no more than the variants they mirror."""
    import os
    import sys
    sys.path.insert(0, os.path.join(__import__("conftest").ROOT, "tools"))
    import codeobj_regs
    regs = codeobj_regs.kernel_regs()
    for k in ("escalate_select_kernel", "escalate_list_kernel"):
        r = [v for n, v in regs.items() if k in n]
        assert len(r) == 1 and r[0]["scratch_bytes"] == 0, (k, r)
    todo = {n: v for n, v in regs.items() if "wfa_group_kernel<" in n and n.rstrip(">)( ").split("(")[0].rstrip("> ").endswith("true")}
    plain = {n: v for n, v in regs.items() if "wfa_group_kernel<" in n and n not in todo}
    assert len(todo) >= 28, sorted(todo)
    assert max(v["scratch_bytes"] for v in todo.values()) <= max(v["scratch_bytes"] for v in plain.values())


def _host(args):
    from aim_amd import build
    return subprocess.run([build.HOST_BIN] + args, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("extra,msg", [(["--algo", "nw"], "--escalate needs --algo wfa"),
                                       (["--algo", "wfa", "--ends-free", "1,1,1,1"], "--escalate cannot be combined with --ends-free"),
                                       (["--algo", "wfa", "--gap2", "24,1"], "--escalate cannot be combined with --gap2"),
                                       (["--algo", "wfa", "--linear"], "--escalate cannot be combined with --linear"),
                                       (["--algo", "wfa", "--w32"], "--escalate cannot be combined with --w32"),
                                       (["--algo", "wfa", "--backtrace", "--bidir"], "--escalate cannot be combined with --bidir")])
def test_host_escalate_refusals(built, tmp_path, extra, msg):
    inp = tmp_path / "in.txt"
    inp.write_text(">ACGT\n<ACGT\n" * 4)
    p = _host([str(inp), str(tmp_path / "o"), "4", "--max-score", "10", "--read-size", "16", "--escalate"] + extra + ["--pack-only", str(tmp_path / "d")])
    assert p.returncode == 1 and p.stderr.strip().splitlines() == [msg], p.stdout + p.stderr


def test_launcher_passes_escalate(built):
    from aim_amd import launch
    cfg = launch.parse("wfa", ["-i", "in", "-o", "out", "-l", "100", "-e", "0.05", "-n", "4", "--escalate"])
    assert cfg["escalate"] and launch.host_command(cfg)[-1] == "--escalate"
    cfg = launch.parse("wfa", ["-i", "in", "-o", "out", "-l", "100", "-e", "0.05", "-n", "4"])
    assert not cfg["escalate"] and "--escalate" not in launch.host_command(cfg)
    with pytest.raises(SystemExit):
        launch.parse("swg", ["-i", "in", "-o", "out", "-l", "100", "-e", "0.01", "-n", "4", "--escalate"])


def test_mixed_pairs_is_seeded_and_built_on_gen_pairs(built):
    from aim_amd import engine
    rs = 112
    a = engine.mixed_pairs(9, 4000, 100, 0.01, 0.05, 0.25, rs)
    b = engine.mixed_pairs(9, 4000, 100, 0.01, 0.05, 0.25, rs)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    req, pat, txt, tail = a
    assert 0.2 < tail.mean() < 0.3
    clean, noisy = engine.gen_pairs(9, 0, 4000, 100, 0.01, rs), engine.gen_pairs(9, 0, 4000, 100, 0.05, rs)
    assert np.array_equal(txt[tail], noisy[2][tail]) and np.array_equal(txt[~tail], clean[2][~tail])
    assert np.array_equal(req[tail], noisy[0][tail]) and np.array_equal(pat, clean[1])
    assert not engine.mixed_pairs(9, 100, 100, 0.01, 0.05, 0.0, rs)[3].any() and engine.mixed_pairs(9, 100, 100, 0.01, 0.05, 1.0, rs)[3].all()
    assert not np.array_equal(engine.mixed_pairs(10, 4000, 100, 0.01, 0.05, 0.25, rs)[3], tail)
