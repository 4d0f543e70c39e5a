"""Dual-cost gap-affine WFA, AIM_FLAG_AFFINE2P: what needs no GPU -- the feature bit, validation, the plan it picks, the bindings,
the CLI's argument checks, the data generator, and the DP model (tests/affine2p_model.py) the GPU tests check against, itself
checked against a brute-force recursion and the oracle's global WFA."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from affine2p_model import brute_score, check_cigar, dp_scores, gap_cost, rescore, single_affine_scores

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    assert engine.features() & capi.FEATURE_AFFINE2P
    assert engine.features() & capi.FEATURE_ENDSFREE
    assert lib.aim_abi_version() == 2


@pytest.mark.parametrize("l,err", [(100, 0.01), (100, 0.05), (1000, 0.05)])
def test_plan_is_group_kernel_with_affine2p(lib, l, err):
    from aim_amd import capi, engine
    ms, rs = engine.launcher_sizes("wfa", l, err)
    for bt in (False, True):
        p = engine.make_params("wfa", ms, rs, backtrace=bt, gap2=(24, 1))
        rc, line = _describe(lib, p)
        assert rc == 0, line
        assert line.startswith("wfa_group_kernel") and line.endswith("affine2p=24,1"), line
        assert lib.aim_kernel_name(capi.params_ref(p)) == b"wfa_group_kernel"


def test_plan_never_lane_kernels(lib):
    from aim_amd import engine
    # shapes the lane kernels take for global WFA (cfg2, packed rows, byte-compact layouts)
    for kw in (dict(), dict(backtrace=True), dict(req8=True, res8=True), dict(req8=True, backtrace=True)):
        glob = engine.make_params("wfa", 5, 112, **kw)
        rc, line = _describe(lib, glob)
        assert rc == 0 and line.startswith("wfa_lane"), line
        p = engine.make_params("wfa", 5, 112, gap2=(12, 1), **kw)
        rc, line = _describe(lib, p)
        assert rc == 0 and line.startswith("wfa_group_kernel") and "affine2p=12,1" in line, line


def test_plan_lds_too_small_is_wave_kernel(lib):
    from aim_amd import engine
    # M ring of o2 + e2 + 1 rows: beyond the group kernel's 32
    rc, line = _describe(lib, engine.make_params("wfa", 50, 112, backtrace=True, gap2=(40, 1)))
    assert rc == 0 and line.startswith("wfa_wave_kernel") and line.endswith("affine2p=40,1"), line
    # rows of 2 * MAX_SCORE + 3 diagonals that LDS cannot hold
    rc, line = _describe(lib, engine.make_params("wfa", 3000, 16000, backtrace=True, gap2=(24, 1)))
    assert rc == 0 and line.startswith("wfa_wave_kernel") and "affine2p=24,1" in line, line
    # and a forced wave run
    os.environ["AIM_FORCE_WAVE"] = "1"
    try:
        rc, line = _describe(lib, engine.make_params("wfa", 20, 112, gap2=(24, 1)))
    finally:
        del os.environ["AIM_FORCE_WAVE"]
    assert rc == 0 and line.startswith("wfa_wave_kernel"), line


def test_plan_scratch_at_least_global(lib):
    from aim_amd import capi, engine
    for l, err in ((100, 0.05), (1000, 0.05)):
        ms, rs = engine.launcher_sizes("wfa", l, err)
        glob = engine.make_params("wfa", ms, rs, backtrace=True)
        a2p = engine.make_params("wfa", ms, rs, backtrace=True, gap2=(24, 1))
        sg = lib.aim_scratch_bytes(capi.params_ref(glob), 10000)
        sa = lib.aim_scratch_bytes(capi.params_ref(a2p), 10000)
        assert sg > 0 and sa >= sg, (l, sg, sa)


def test_affine2p_params_write_through_to_base():
    from aim_amd import capi, engine
    p = engine.make_params("wfa", 5, 112, gap2=(24, 2))
    p.flags |= capi.FLAG_BACKTRACE
    assert p.base.flags == capi.FLAG_AFFINE2P | capi.FLAG_BACKTRACE and p.flags == p.base.flags
    p.max_score = 9
    assert p.base.max_score == 9 and p.max_score == 9
    p.gap_e2 = 3
    assert p.gap_e2 == 3 and bytes(p)[-4:] == (3).to_bytes(4, "little")
    assert (p.gap_o2, p.gap_o, p.gap_e) == (24, 4, 1)
    with pytest.raises(ValueError):
        engine.make_params("wfa", 5, 112, gap2=(24, 1), ends_free=(0, 0, 1, 1))


@pytest.mark.parametrize("case", ["nw", "swg", "genasm", "reduce", "endsfree", "o2_zero", "e2_zero", "o2_negative"])
def test_invalid_combinations(lib, case):
    from aim_amd import capi, engine
    gap2 = (24, 1)
    algo = "wfa"
    kw = {}
    if case in ("nw", "swg", "genasm"):
        algo = case
    elif case == "reduce":
        kw["reduce"] = True
    elif case == "o2_zero":
        gap2 = (0, 1)
    elif case == "e2_zero":
        gap2 = (24, 0)
    elif case == "o2_negative":
        gap2 = (-3, 1)
    p = engine.make_params(algo, 5, 112, gap2=gap2, **kw)
    if case == "endsfree":   # an affine2p struct with both flags
        p.flags |= capi.FLAG_ENDSFREE
    rc, _ = _describe(lib, p)
    assert rc == capi.AIM_EINVAL
    assert lib.aim_scratch_bytes(capi.params_ref(p), 1000) == 0
    assert lib.aim_kernel_name(capi.params_ref(p)) == b""


def test_extension_not_read_without_flag(lib):
    """Without the flag the entry points read only aim_params_t: the plan is the global one whatever follows it."""
    from aim_amd import capi, engine
    for o2, e2 in ((24, 1), (0, 0), (-5, -5)):
        p = engine.make_params("wfa", 5, 112, gap2=(max(o2, 1), max(e2, 1)))
        p.gap_o2, p.gap_e2 = o2, e2
        p.base.flags &= ~capi.FLAG_AFFINE2P
        rc, line = _describe(lib, p)
        rc0, line0 = _describe(lib, engine.make_params("wfa", 5, 112))
        assert rc == 0 and line == line0 and "affine2p" not in line


def _random_pairs(rng, n, lmax, alphabet=b"ACGT"):
    from aim_amd.capi import REQUEST_DTYPE
    rs = (lmax + 7) // 8 * 8 + 8
    req = np.zeros(n, dtype=REQUEST_DTYPE)
    pat = np.zeros((n, rs), dtype=np.uint8)
    txt = np.zeros((n, rs), dtype=np.uint8)
    a = np.frombuffer(alphabet, dtype=np.uint8)
    for i in range(n):
        pl, tl = int(rng.integers(0, lmax + 1)), int(rng.integers(0, lmax + 1))
        pat[i, :pl] = a[rng.integers(0, len(a), pl)]
        txt[i, :tl] = a[rng.integers(0, len(a), tl)]
        req["pattern_len"][i], req["text_len"][i], req["idx"][i] = pl, tl, i
    return req, pat, txt, rs


@pytest.mark.parametrize("pen", [(3, 4, 1, 12, 1), (4, 4, 2, 24, 1), (2, 3, 2, 6, 1), (3, 4, 1, 4, 1), (5, 2, 3, 9, 1)])
def test_model_equals_brute_force_on_tiny_pairs(pen):
    rng = np.random.default_rng(sum(pen) * 13 + 3)
    req, pat, txt, _ = _random_pairs(rng, 250, 8, alphabet=b"ACG")
    got = dp_scores(req, pat, txt, *pen)
    for i in range(len(req)):
        p = bytes(pat[i, :req["pattern_len"][i]])
        t = bytes(txt[i, :req["text_len"][i]])
        assert got[i] == brute_score(p, t, *pen), (p, t, pen)


@pytest.mark.parametrize("pen", [(3, 4, 1), (4, 6, 2)])
def test_model_equal_pieces_equals_oracle_global_wfa(built, sample_bytes, pen):
    from aim_amd import engine
    from oracle import oracle
    x, o, e = pen
    ms, rs = engine.launcher_sizes("wfa", 100, 0.01)
    req, pat, txt = engine.parse_pairs(sample_bytes, rs, max_pairs=1500)
    op = oracle.params("wfa", 10 ** 4, rs, mismatch=x, gap_o=o, gap_e=e)
    ores, _, _ = oracle.align_batch(op, req["pattern_len"], req["text_len"], pat, txt, nthreads=4)
    assert np.array_equal(dp_scores(req, pat, txt, x, o, e, o, e), ores["score"])


def test_model_beats_single_affine_on_long_indels():
    from aim_amd import engine
    req, pat, txt = engine.gen_pairs(9, 0, 200, 200, 0.01, 208)
    req, pat, txt = engine.long_indel_pairs(9, 0, req, pat, txt, 60)
    dual = dp_scores(req, pat, txt, 4, 4, 2, 24, 1)
    single = single_affine_scores(req, pat, txt, 4, 4, 2)
    assert (dual <= single).all()
    assert (dual < single).mean() > 0.9
    # a constructed pair: one 40-base deletion
    from aim_amd.capi import REQUEST_DTYPE
    rng = np.random.default_rng(1)
    p = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 120)]
    t = np.concatenate([p[:50], p[90:]])
    r1 = np.zeros(1, dtype=REQUEST_DTYPE)
    r1["pattern_len"], r1["text_len"] = 120, 80
    P = np.zeros((1, 128), dtype=np.uint8)
    T = np.zeros((1, 128), dtype=np.uint8)
    P[0, :120], T[0, :80] = p, t
    assert dp_scores(r1, P, T, 4, 4, 2, 24, 1)[0] <= 24 + 40
    assert single_affine_scores(r1, P, T, 4, 4, 2)[0] > 64


def test_cigar_cost_function():
    assert check_cigar("MM", b"AC", b"AC") is None
    assert check_cigar("MX", b"AC", b"AC") is not None
    assert check_cigar("IIMM", b"AC", b"GGAC") is None
    assert rescore("MXM", 3, 4, 1, 24, 1) == 3
    assert rescore("M" + "D" * 30 + "M", 3, 4, 1, 24, 1) == min(4 + 30, 24 + 30)
    assert rescore("M" + "I" * 100 + "M", 4, 4, 2, 24, 1) == 124
    assert rescore("IIDD", 4, 4, 2, 24, 1) == 16


def test_host_gap2_argument_errors(built):
    host = os.path.join(ROOT, "aim_amd", "host", "host")
    if not os.path.exists(host):
        pytest.fail("host binary missing")
    base = [host, "in.txt", "out.txt", "1", "--algo", "wfa", "--max-score", "20", "--read-size", "112"]
    for extra, msg in (([ "--gap2", "24"], "--gap2 O2,E2"), (["--gap2", "24,x"], "--gap2 O2,E2"), (["--gap2", "0,1"], "--gap2 O2,E2"),
                       (["--gap2", "24,1,3"], "--gap2 O2,E2"), (["--gap2", "24,1", "--ends-free", "0,0,1,1"], "--ends-free"),
                       (["--gap2", "24,1", "--reduce"], "--reduce")):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=60)
        assert r.returncode != 0 and msg in r.stderr, (extra, r.stderr)
    r = subprocess.run([host, "in.txt", "out.txt", "1", "--algo", "nw", "--gap2", "24,1"], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "--gap2 needs --algo wfa" in r.stderr, r.stderr


def test_gen_dataset_without_long_indel_unchanged(tmp_path):
    from aim_amd import engine, gen_dataset
    out = tmp_path / "a.txt"
    assert gen_dataset.main(["-n", "50", "-l", "100", "-e", "0.02", "-o", str(out), "-s", "5"]) == 0
    req, pat, txt = engine.gen_pairs(5, 0, 50, 100, 0.02, 112)
    assert out.read_bytes() == engine.pairs_to_text(req, pat, txt)
    pk = tmp_path / "a.pk"
    assert gen_dataset.main(["-n", "50", "-l", "100", "-e", "0.02", "-o", str(pk), "-s", "5", "--packed"]) == 0
    pk2 = tmp_path / "b.pk"
    assert gen_dataset.main(["-n", "50", "-l", "100", "-e", "0.02", "-o", str(pk2), "-s", "5", "--packed", "--long-indel", "0"]) == 0
    assert pk.read_bytes() == pk2.read_bytes()


def test_long_indels_depend_on_pair_index_only():
    """A slice of a data set carries the same indels as the whole: text chunks and packed batches of one data set agree."""
    from aim_amd import engine
    req, pat, txt = engine.gen_pairs(4, 0, 300, 100, 0.01, 112)
    whole = engine.long_indel_pairs(4, 0, req, pat, txt, 30)
    r2, p2, t2 = engine.gen_pairs(4, 100, 200, 100, 0.01, 112)
    part = engine.long_indel_pairs(4, 100, r2, p2, t2, 30)
    assert np.array_equal(whole[0][100:], part[0])
    assert np.array_equal(whole[2][100:], part[2])


def test_gen_dataset_long_indel(tmp_path):
    from aim_amd import engine, gen_dataset
    out = tmp_path / "l.txt"
    assert gen_dataset.main(["-n", "40", "-l", "100", "-e", "0.0", "-o", str(out), "--long-indel", "30"]) == 0
    req, pat, txt = engine.parse_pairs(out.read_bytes(), 144)
    r0, p0, t0 = engine.gen_pairs(42, 0, 40, 100, 0.0, 104)
    assert np.array_equal(req["pattern_len"], r0["pattern_len"])
    d = req["text_len"].astype(int) - r0["text_len"].astype(int)
    assert ((np.abs(d) >= 15) & (np.abs(d) <= 30)).all() and (d > 0).any() and (d < 0).any()
    # the indel is the only change: the model scores it as one gap
    want = np.array([gap_cost(abs(int(k)), 4, 2, 24, 1) for k in d])
    assert (dp_scores(req, pat, txt, 4, 4, 2, 24, 1) == want).all()
