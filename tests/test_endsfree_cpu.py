"""Ends-free (semi-global) WFA, AIM_FLAG_ENDSFREE: what needs no GPU -- the feature bit, validation, the plan it picks, and the
DP model (tests/endsfree_model.py) the GPU tests check against, itself checked against the oracle's global WFA and a brute-force
recursion."""
import ctypes as C

import numpy as np
import pytest

from endsfree_model import brute_score, check_cigar, dp_scores, rescore


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
    assert engine.features() & capi.FEATURE_ENDSFREE
    assert lib.aim_abi_version() == 2


def test_plan_cfg2_shape_is_group_kernel_with_endsfree(lib):
    from aim_amd import capi, engine
    glob = engine.make_params("wfa", 5, 112)
    rc, line = _describe(lib, glob)
    assert rc == 0 and line.startswith("wfa_lane_kernel") and "endsfree" not in line
    for bt in (False, True):
        ef = engine.make_params("wfa", 5, 112, backtrace=bt, ends_free=(0, 0, 16, 16))
        rc, line = _describe(lib, ef)
        assert rc == 0, line
        assert line.startswith("wfa_group_kernel") and line.endswith("endsfree=0,0,16,16"), line
        assert lib.aim_kernel_name(capi.params_ref(ef)) == b"wfa_group_kernel"


def test_plan_free_span_too_wide_for_lds_is_wave_kernel(lib):
    from aim_amd import engine
    # rows of 2 * MAX_SCORE + 3 + PB + TB diagonals: ~16 000 here, far beyond a workgroup's LDS
    for ef in ((8000, 0, 8000, 0), (1 << 30, 0, 1 << 30, 0)):
        rc, line = _describe(lib, engine.make_params("wfa", 50, 8000, backtrace=True, ends_free=ef))
        assert rc == 0 and line.startswith("wfa_wave_kernel") and ("endsfree=%d,%d,%d,%d" % ef) in line, line
    # the same shape with moderate free lengths fits the group kernel
    rc, line = _describe(lib, engine.make_params("wfa", 50, 8000, backtrace=True, ends_free=(0, 0, 50, 50)))
    assert rc == 0 and line.startswith("wfa_group_kernel"), line


def test_plan_packed_batches_skip_lane_kernels(lib):
    from aim_amd import engine
    # the byte-compact layouts of a cfg2 batch: the group kernel, never a lane kernel (packed input is checked on the GPU)
    ef = engine.make_params("wfa", 5, 112, req8=True, res8=True, ends_free=(0, 0, 8, 8))
    rc, line = _describe(lib, ef)
    assert rc == 0 and line.startswith("wfa_group_kernel"), line


def test_endsfree_params_write_through_to_base():
    from aim_amd import capi, engine
    ef = engine.make_params("wfa", 5, 112, ends_free=(1, 2, 3, 4))
    ef.flags |= capi.FLAG_BACKTRACE
    assert ef.base.flags == capi.FLAG_ENDSFREE | capi.FLAG_BACKTRACE and ef.flags == ef.base.flags
    ef.max_score = 9
    assert ef.base.max_score == 9
    ef.text_end_free = 7
    assert ef.text_end_free == 7 and bytes(ef)[-4:] == (7).to_bytes(4, "little")


@pytest.mark.parametrize("case", ["nw", "swg", "genasm", "reduce", "negative_pb", "negative_te"])
def test_invalid_combinations(lib, case):
    from aim_amd import capi, engine
    kw = dict(ends_free=(0, 0, 4, 4))
    algo = "wfa"
    if case in ("nw", "swg", "genasm"):
        algo = case
    elif case == "reduce":
        kw["reduce"] = True
    elif case == "negative_pb":
        kw["ends_free"] = (-1, 0, 4, 4)
    else:
        kw["ends_free"] = (0, 0, 4, -3)
    p = engine.make_params(algo, 5, 112, **kw)
    rc, _ = _describe(lib, p)
    assert rc == capi.AIM_EINVAL
    assert lib.aim_scratch_bytes(capi.params_ref(p), 1000) == 0
    assert lib.aim_kernel_name(capi.params_ref(p)) == b""


def test_flag_without_extension_fields_is_not_read_without_flag(lib):
    """Without the flag the entry points read only aim_params_t: the plan is the global one whatever follows it."""
    from aim_amd import capi, engine
    ef = engine.make_params("wfa", 5, 112, ends_free=(0, 0, 16, 16))
    ef.base.flags &= ~capi.FLAG_ENDSFREE
    rc, line = _describe(lib, ef)
    assert rc == 0 and line.startswith("wfa_lane_kernel") and "endsfree" not in line


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


@pytest.mark.parametrize("pen", [(3, 4, 1), (4, 6, 2)])
def test_model_zero_free_equals_oracle_global_wfa(built, pen):
    from aim_amd import engine
    from oracle import oracle
    x, o, e = pen
    ms, rs = 60, 112
    req, pat, txt = engine.gen_pairs(11 + x, 0, 1000, 100, 0.04, rs)
    rng = np.random.default_rng(5)
    req2, pat2, txt2, rs2 = _random_pairs(rng, 1000, 24)
    op = oracle.params("wfa", 10 ** 4, rs, mismatch=x, gap_o=o, gap_e=e)
    ores, _, _ = oracle.align_batch(op, req["pattern_len"], req["text_len"], pat, txt, nthreads=4)
    assert np.array_equal(dp_scores(req, pat, txt, x, o, e), ores["score"])
    op2 = oracle.params("wfa", 10 ** 4, rs2, mismatch=x, gap_o=o, gap_e=e)
    ores2, _, _ = oracle.align_batch(op2, req2["pattern_len"], req2["text_len"], pat2, txt2, nthreads=4)
    assert np.array_equal(dp_scores(req2, pat2, txt2, x, o, e), ores2["score"])


@pytest.mark.parametrize("ef", [(0, 0, 2, 2), (2, 1, 0, 0), (1, 2, 3, 0), (6, 6, 6, 6), (0, 3, 1, 0), (9, 9, 9, 9)])
def test_model_equals_brute_force_on_tiny_pairs(ef):
    rng = np.random.default_rng(sum(ef) * 7 + 1)
    req, pat, txt, _ = _random_pairs(rng, 300, 6, alphabet=b"ACG")
    for pen in ((3, 4, 1), (4, 6, 2)):
        got = dp_scores(req, pat, txt, *pen, ends_free=ef)
        for i in range(len(req)):
            p = bytes(pat[i, :req["pattern_len"][i]])
            t = bytes(txt[i, :req["text_len"][i]])
            assert got[i] == brute_score(p, t, *pen, ends_free=ef), (p, t, pen, ef)


def test_ends_free_never_above_global():
    from aim_amd import engine
    req, pat, txt = engine.gen_pairs(3, 0, 400, 100, 0.05, 112)
    req, pat, txt = engine.flank_pairs(3, 0, req, pat, txt, 8)
    g = dp_scores(req, pat, txt)
    for ef in ((0, 0, 8, 8), (3, 3, 0, 0), (100, 100, 100, 100)):
        assert (dp_scores(req, pat, txt, ends_free=ef) <= g).all()
    # the flanks are free: the score is that of the pair without them at most
    req0, pat0, txt0 = engine.gen_pairs(3, 0, 400, 100, 0.05, 112)
    assert (dp_scores(req, pat, txt, ends_free=(0, 0, 8, 8)) <= dp_scores(req0, pat0, txt0)).all()


def test_cigar_checkers():
    assert check_cigar("MM", b"AC", b"AC") is None
    assert check_cigar("MX", b"AC", b"AC") is not None
    assert check_cigar("IIMM", b"AC", b"GGAC") is None
    assert rescore("IIMM", 2, 4, ends_free=(0, 0, 2, 0)) == 0
    assert rescore("IIIMM", 2, 5, ends_free=(0, 0, 2, 0)) == 5
    assert rescore("MMDD", 4, 2, ends_free=(0, 1, 0, 0)) == 5
    assert rescore("IIII", 0, 4, ends_free=(0, 0, 1, 2)) == 5


def test_gen_dataset_flank(tmp_path):
    from aim_amd import engine, gen_dataset
    out = tmp_path / "f.txt"
    assert gen_dataset.main(["-n", "5", "-l", "100", "-e", "0.01", "-o", str(out), "--flank", "16"]) == 0
    req, pat, txt = engine.parse_pairs(out.read_bytes(), 152)
    r0, p0, t0 = engine.gen_pairs(42, 0, 5, 100, 0.01, 112)
    assert np.array_equal(req["pattern_len"], r0["pattern_len"])
    assert np.array_equal(req["text_len"], r0["text_len"] + 32)
    for i in range(5):
        tl = int(r0["text_len"][i])
        assert bytes(txt[i, 16:16 + tl]) == bytes(t0[i, :tl])
        assert set(bytes(txt[i, :16]) + bytes(txt[i, 16 + tl:32 + tl])) <= set(b"ACGT")
