"""Gap-linear WFA, AIM_FLAG_LINEAR: what needs no GPU -- the feature bit, the plans it gets, validation, the history size, the
bindings, the CLI's argument checks, and the DP model (tests/linear_model.py) the GPU tests check against, itself checked against a
brute-force recursion and the oracle's NW."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from linear_model import brute_score, check_cigar, dp_scores, max_score_rule, rescore

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PENS = [(1, 1), (4, 2), (2, 3), (5, 2)]


@pytest.fixture(scope="module")
def lib(built):
    from aim_amd import capi
    return capi.load()


def _describe(lib, params, n=100000):
    from aim_amd import capi
    buf = C.create_string_buffer(512)
    rc = lib.aim_plan_describe(capi.params_ref(params), n, buf, len(buf))
    return rc, buf.value.decode()


def test_features_bit(lib):
    from aim_amd import capi, engine
    assert engine.features() & capi.FEATURE_LINEAR
    assert engine.features() & capi.FEATURE_AFFINE2P and engine.features() & capi.FEATURE_ENDSFREE
    assert lib.aim_abi_version() == 2


@pytest.mark.parametrize("pen", [(1, 1), (4, 2)])
def test_plans_accept_linear_over_a_grid(lib, pen):
    from aim_amd import capi, engine
    x, g = pen
    seen = set()
    for rs in (80, 112, 160, 256, 1016, 2048, 8192, 16368, 16376, 32752):
        for err in (0.01, 0.05, 0.10):
            ms = max_score_rule(rs, err, x, g)
            for kw in (dict(), dict(backtrace=True), dict(req8=True), dict(res8=True), dict(req8=True, res8=True),
                       dict(req8=True, backtrace=True)):
                p = engine.make_params("wfa", ms, rs, mismatch=x, gap_e=g, linear=True, **kw)
                rc, line = _describe(lib, p)
                assert rc == 0, (rs, err, kw, lib.aim_last_error())
                kernel = line.split()[0]
                assert kernel in ("wfa_group_kernel", "wfa_wave_kernel"), line
                assert line.endswith(" linear"), line
                assert lib.aim_scratch_bytes(capi.params_ref(p), 100000) > 0
                seen.add(kernel)
    assert seen == {"wfa_group_kernel", "wfa_wave_kernel"}


def test_plan_never_lane_kernels(lib, monkeypatch):
    """The shapes the lane kernels take for global WFA go to wfa_group with the flag."""
    from aim_amd import engine
    for rs, ms, bt in ((112, 4, False), (112, 4, True), (80, 10, False), (160, 8, True)):
        rc, line = _describe(lib, engine.make_params("wfa", ms, rs, mismatch=4, gap_e=2, backtrace=bt, linear=True))
        assert rc == 0 and line.startswith("wfa_group_kernel"), line
    for knob in ("AIM_FORCE_WAVE", "AIM_NO_GROUP"):
        monkeypatch.setenv(knob, "1")
        rc, line = _describe(lib, engine.make_params("wfa", 4, 112, mismatch=4, gap_e=2, linear=True))
        assert rc == 0 and line.startswith("wfa_wave_kernel") and line.endswith(" linear"), (knob, line)
        monkeypatch.delenv(knob)
    p = engine.make_params("wfa", 200, 1016, mismatch=4, gap_e=2, backtrace=True, linear=True)
    rc, wide = _describe(lib, p)
    monkeypatch.setenv("AIM_GROUP_WLDS", "32")   # narrow rows: a smaller history region (rows x 32 cells)
    rc2, narrow = _describe(lib, p)
    assert rc == 0 and rc2 == 0 and narrow.startswith("wfa_group_kernel") and narrow.endswith(" linear"), narrow
    assert _hist(narrow) < _hist(wide), (narrow, wide)


def test_plan_debug_line_ends_with_linear(lib, capfd):
    """AIM_PLAN_DEBUG: the wfa_group line and the plan line both end with ' linear' (subprocess: the knob is read once per process)."""
    code = ("import ctypes as C; from aim_amd import capi, engine; lib = capi.load(); "
            "p = engine.make_params('wfa', 40, 1016, mismatch=4, gap_e=2, backtrace=True, linear=True); "
            "b = C.create_string_buffer(512); print(lib.aim_plan_describe(capi.params_ref(p), 10000, b, 512))")
    env = dict(os.environ, AIM_PLAN_DEBUG="1")
    r = subprocess.run(["python", "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "0", r.stderr
    lines = [l for l in r.stderr.splitlines() if l.startswith("[aim plan]")]
    assert any(l.startswith("[aim plan] wfa_group G=") for l in lines), lines
    assert lines and all(l.endswith(" linear") for l in lines), lines


VALIDATION = [
    (dict(algo="nw"), "AIM_FLAG_LINEAR needs AIM_ALGO_WFA"),
    (dict(algo="swg"), "AIM_FLAG_LINEAR needs AIM_ALGO_WFA"),
    (dict(algo="genasm"), "AIM_FLAG_LINEAR needs AIM_ALGO_WFA"),
    (dict(flag="reduce"), "AIM_FLAG_LINEAR cannot be combined with AIM_FLAG_REDUCE"),
    (dict(flag="endsfree"), "AIM_FLAG_LINEAR cannot be combined with AIM_FLAG_ENDSFREE"),
    (dict(flag="affine2p"), "AIM_FLAG_LINEAR cannot be combined with AIM_FLAG_AFFINE2P"),
    (dict(gap_o=1), "gap-linear penalties must be m <= 0, gap_o = 0 and x, gap_e > 0 (got 0,4,1,2)"),
    (dict(gap_o=-1), "gap-linear penalties must be m <= 0, gap_o = 0 and x, gap_e > 0 (got 0,4,-1,2)"),
    (dict(mismatch=0), "gap-linear penalties must be m <= 0, gap_o = 0 and x, gap_e > 0 (got 0,0,0,2)"),
    (dict(gap_e=0), "gap-linear penalties must be m <= 0, gap_o = 0 and x, gap_e > 0 (got 0,4,0,0)"),
    (dict(gap_e=-2), "gap-linear penalties must be m <= 0, gap_o = 0 and x, gap_e > 0 (got 0,4,0,-2)"),
    (dict(match=1), "gap-linear penalties must be m <= 0, gap_o = 0 and x, gap_e > 0 (got 1,4,0,2)"),
]


@pytest.mark.parametrize("case,msg", VALIDATION)
def test_validation(lib, case, msg):
    from aim_amd import capi, engine
    kw = dict(mismatch=4, gap_e=2)
    for k in ("mismatch", "gap_e", "match"):
        if k in case:
            kw[k] = case[k]
    if case.get("flag") == "endsfree":
        p = engine.make_params("wfa", 20, 112, ends_free=(0, 0, 0, 0), **kw)
        p.flags |= capi.FLAG_LINEAR
        p.gap_o = 0
    elif case.get("flag") == "affine2p":
        p = engine.make_params("wfa", 20, 112, gap2=(24, 1), **kw)
        p.flags |= capi.FLAG_LINEAR
        p.gap_o = 0
    else:
        p = engine.make_params(case.get("algo", "wfa"), 20, 112, linear=True, **kw)
        if case.get("flag") == "reduce":
            p.flags |= capi.FLAG_REDUCE
        if "gap_o" in case:
            p.gap_o = case["gap_o"]
    rc, _ = _describe(lib, p)
    assert rc == capi.AIM_EINVAL
    assert lib.aim_last_error().decode() == msg
    assert lib.aim_scratch_bytes(capi.params_ref(p), 1000) == 0
    assert lib.aim_kernel_name(capi.params_ref(p)) == b""


def test_gap_o_zero_without_flag_still_rejected(lib):
    from aim_amd import capi, engine
    p = engine.make_params("wfa", 20, 112, mismatch=4, gap_o=0, gap_e=2)
    rc, _ = _describe(lib, p)
    assert rc == capi.AIM_EINVAL
    assert "Wrong affine gap penalties" in lib.aim_last_error().decode()


def _hist(line):
    return int(re.search(r" hist=(\d+)", line).group(1))


@pytest.mark.parametrize("l,err", [(1000, 0.05), (1000, 0.10), (2000, 0.05)])
def test_history_is_smaller_than_global(lib, l, err):
    """2-byte cells against global WFA's 8-byte {M, I, D, -}: LIN (4, 2) and global (4, 2, 2) share the unit 2 and the shape."""
    from aim_amd import engine
    ms = max_score_rule(l, err, 4, 2)
    rs = (l + l // 10 + 7) // 8 * 8
    n = 4096
    rc, lin = _describe(lib, engine.make_params("wfa", ms, rs, mismatch=4, gap_e=2, backtrace=True, linear=True), n)
    rc0, glob = _describe(lib, engine.make_params("wfa", ms, rs, mismatch=4, gap_o=2, gap_e=2, backtrace=True), n)
    assert rc == 0 and rc0 == 0
    assert lin.startswith("wfa_group_kernel") and glob.startswith("wfa_group_kernel"), (lin, glob)
    assert " chunk=%d " % n in lin and " chunk=%d " % n in glob, (lin, glob)
    assert _hist(lin) <= 0.3 * _hist(glob), (lin, glob)


def _random_pairs(rng, n, lmax):
    from aim_amd.capi import REQUEST_DTYPE
    rs = (lmax + 7) // 8 * 8 + 8
    req = np.zeros(n, dtype=REQUEST_DTYPE)
    pat = np.zeros((n, rs), dtype=np.uint8)
    txt = np.zeros((n, rs), dtype=np.uint8)
    a = np.frombuffer(b"ACGT", dtype=np.uint8)
    for i in range(n):
        pl, tl = int(rng.integers(0, lmax + 1)), int(rng.integers(0, lmax + 1))
        pat[i, :pl] = a[rng.integers(0, 4, pl)]
        txt[i, :tl] = a[rng.integers(0, 4, tl)]
        req["pattern_len"][i], req["text_len"][i], req["idx"][i] = pl, tl, i
    return req, pat, txt


@pytest.mark.parametrize("pen", PENS)
def test_model_equals_brute_force_on_tiny_pairs(pen):
    rng = np.random.default_rng(sum(pen))
    req, pat, txt = _random_pairs(rng, 400, 9)
    want = [brute_score(bytes(pat[i, :req["pattern_len"][i]]), bytes(txt[i, :req["text_len"][i]]), *pen) for i in range(len(req))]
    assert np.array_equal(dp_scores(req, pat, txt, *pen), want)


@pytest.mark.parametrize("pen", PENS)
@pytest.mark.parametrize("l,err", [(100, 0.05), (1000, 0.05)])
def test_model_equals_oracle_nw(built, pen, l, err):
    """NW with mismatch x and gap g is the same optimum; pairs with pattern_len > text_len are left out (NW's N1 row aliasing
    reproduces the reference there, not the optimum)."""
    from aim_amd import engine
    from oracle import oracle
    x, g = pen
    _, rs = engine.launcher_sizes("wfa", l, err)
    req, pat, txt = engine.gen_pairs(40 + l, 0, 600 if l < 1000 else 150, l, err, rs)
    keep = req["pattern_len"] <= req["text_len"]
    req, pat, txt = req[keep], pat[keep], txt[keep]
    assert len(req) > 40
    op = oracle.params("nw", 10 ** 4, rs, mismatch=x, gap=g)
    ores, _, _ = oracle.align_batch(op, req["pattern_len"], req["text_len"], pat, txt, nthreads=4)
    assert np.array_equal(dp_scores(req, pat, txt, x, g), ores["score"])


def test_cigar_checker():
    assert check_cigar("MMXM", b"ACGT", b"ACTT") is None and rescore("MMXM", 4, 2) == 4
    assert check_cigar("MMDMM", b"ACGTA", b"ACTA") is None and rescore("MMDMM", 4, 2) == 2
    assert check_cigar("MMIMM", b"ACTA", b"ACGTA") is None and rescore("MMIMM", 1, 1) == 1
    assert check_cigar("MMMM", b"ACGT", b"ACTT") is not None
    assert check_cigar("MMM", b"ACGT", b"ACGT") is not None
    assert max_score_rule(100, 0.01, 1, 1) == 1 and max_score_rule(1000, 0.05, 4, 2) == 200
    assert max_score_rule(100, 0.05, 5, 2) == 20 and max_score_rule(100, 0.05, 2, 3) == 15


def test_make_params_linear():
    from aim_amd import capi, engine
    p = engine.make_params("wfa", 20, 112, mismatch=1, gap_e=1, backtrace=True, linear=True)
    assert isinstance(p, capi.Params)
    assert p.flags == capi.FLAG_LINEAR | capi.FLAG_BACKTRACE and p.gap_o == 0 and p.mismatch == 1 and p.gap_e == 1
    for kw in (dict(ends_free=(0, 0, 1, 1)), dict(gap2=(24, 1)), dict(reduce=True)):
        with pytest.raises(ValueError):
            engine.make_params("wfa", 20, 112, linear=True, **kw)


def test_host_linear_arguments(built, tmp_path):
    host = os.path.join(ROOT, "aim_amd", "host", "host")
    if not os.path.exists(host):
        pytest.fail("host binary missing")
    base = [host, "in.txt", "out.txt", "1", "--max-score", "20", "--read-size", "112"]
    for extra, msg in ((["--algo", "nw", "--linear"], "--linear needs --algo wfa"), (["--algo", "swg", "--linear"], "--linear needs --algo wfa"),
                       (["--algo", "wfa", "--linear", "--gap2", "24,1"], "--linear cannot be combined with --gap2"),
                       (["--algo", "wfa", "--linear", "--ends-free", "0,0,1,1"], "--linear cannot be combined with --ends-free"),
                       (["--algo", "wfa", "--linear", "--reduce"], "--linear cannot be combined with --reduce")):
        r = subprocess.run(base + extra, cwd=tmp_path, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    # accepted: the run gets as far as opening its input (which does not exist here)
    r = subprocess.run(base + ["--algo", "wfa", "--linear", "--mismatch", "1", "--gap-e", "1", "--gap-o", "6"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "couldn't be opened" in r.stdout + r.stderr, r.stdout + r.stderr
