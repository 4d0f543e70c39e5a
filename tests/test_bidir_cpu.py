"""Bidirectional WFA, AIM_FLAG_WFA_BIDIR: what needs no GPU -- the BiWFA model (tests/bidir_model.py) against a brute-force Gotoh DP,
the oracle's flag-less WFA score against the same DP (the "score and status" premise of the flag), the feature bit, validation,
the plan line, the scratch it needs, the bindings and the command lines."""
import ctypes as C
import random
import subprocess

import pytest

import affine2p_model
import bidir_model as bm

PENALTIES = [(3, 4, 1), (4, 6, 2), (1, 1, 1), (7, 2, 1)]   # the last one: x > o + e


def _mutate(s, err, rng):
    out = []
    for c in s:
        r = rng.random()
        if r < err / 3:
            continue
        if r < 2 * err / 3:
            out.append(rng.choice(b"ACGT"))
            out.append(c)
        elif r < err:
            out.append(rng.choice(b"ACGT"))
        else:
            out.append(c)
    return bytes(out)


def _cases(seed, n):
    """Seeded pairs at l <= 60: random edits, N bytes, long indels across the middle, empty and very unequal sides."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        l = rng.randint(0, 60)
        P = bytes(rng.choice(b"ACGTN") if rng.random() < 0.02 else rng.choice(b"ACGT") for _ in range(l))
        T = _mutate(P, rng.choice([0.05, 0.2, 0.4]), rng)
        if i % 5 == 0 and len(T) > 10:   # a long indel across the middle
            m, L = len(T) // 2, rng.randint(5, 25)
            T = T[:max(m - L // 2, 0)] + T[m + L // 2:] if rng.random() < 0.5 else T[:m] + bytes(rng.choice(b"ACGT") for _ in range(L)) + T[m:]
        if i % 11 == 0:
            T = T[:rng.randint(0, 3)]      # tlen << plen, or empty
        if i % 13 == 0:
            P = P[:rng.randint(0, 3)]      # plen << tlen, or empty
        out.append((P, T, PENALTIES[i % len(PENALTIES)]))
    return out


CASES = _cases(2023, 2400)


@pytest.mark.parametrize("part", range(4))
def test_model_equals_gotoh(part):
    """Score = DP (or MAX_SCORE + 1 over a cap), CIGAR valid and re-scored; small T and short-side limits force deep recursion."""
    rng = random.Random(part)
    comps = []
    for P, T, (x, o, e) in CASES[part::4]:
        d = bm.gotoh(P, T, x, o, e)
        cap = rng.choice([1 << 30, d, max(d - 1, 0), d + 1, d // 2])   # (MAX_SCORE >= 0)
        s, ops = bm.align(P, T, x, o, e, max_score=cap, base_t=rng.choice([0, 2, 5]), short=rng.choice([0, 1, 4]), stats=comps)
        assert s == (d if d <= cap else cap + 1), (P, T, (x, o, e), cap)
        if s <= cap:
            assert affine2p_model.check_cigar(ops, P, T) is None, (P, T, ops)
            assert affine2p_model.rescore(ops, x, o, e, o, e) == s, (P, T, ops)
        else:
            assert ops is None
    # breakpoints land in all three components: the halves start and end inside gaps
    assert comps.count(bm.M) > 0 and comps.count(bm.I) > 0 and comps.count(bm.D) > 0, comps


def test_model_base_case_components():
    """The base case that starts and ends inside a gap: a run crossing either end costs no open at the start and one at the end."""
    for P, T, (x, o, e) in CASES[:300]:
        for cs in (bm.M, bm.I, bm.D):
            for ce in (bm.M, bm.I, bm.D):
                s, ops = bm.wf_align(P, T, x, o, e, cs, ce, 400)
                if s is None:
                    continue
                assert affine2p_model.check_cigar(ops, P, T) is None
                cost = affine2p_model.rescore(ops, x, o, e, o, e)
                lead = len(ops) - len(ops.lstrip("I" if cs == bm.I else "D")) if cs != bm.M else 0
                assert s == cost - (o if lead else 0), (P, T, cs, ce, ops)
                if ce != bm.M and (P or T):
                    assert ops and ops[-1] == ("I" if ce == bm.I else "D"), (cs, ce, ops)


def test_oracle_wfa_equals_gotoh(built):
    """The reference's flag-less WFA score is the in-matrix Gotoh optimum on the same pairs (so bidir can return it)."""
    import numpy as np
    from oracle import oracle
    rs = 128
    for pen in PENALTIES:
        cases = [(P, T) for P, T, p in CASES if p == pen]
        n = len(cases)
        pat = np.zeros((n, rs), dtype=np.uint8)
        txt = np.zeros((n, rs), dtype=np.uint8)
        for i, (P, T) in enumerate(cases):
            pat[i, :len(P)] = np.frombuffer(P, dtype=np.uint8)
            txt[i, :len(T)] = np.frombuffer(T, dtype=np.uint8)
        plen = np.array([len(P) for P, _ in cases], dtype=np.int32)
        tlen = np.array([len(T) for _, T in cases], dtype=np.int32)
        x, o, e = pen
        res, _, _ = oracle.align_batch(oracle.params("wfa", 400, rs, mismatch=x, gap_o=o, gap_e=e), plen, tlen, pat, txt, nthreads=4)
        want = [bm.gotoh(P, T, x, o, e) for P, T in cases]
        assert list(res["score"]) == want, pen


# ---- the library ------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib(built):
    from aim_amd import capi
    return capi.load()


def _describe(lib, params, n=2048):
    from aim_amd import capi
    buf = C.create_string_buffer(512)
    rc = lib.aim_plan_describe(capi.params_ref(params), n, buf, len(buf))
    return rc, buf.value.decode() if rc == 0 else lib.aim_last_error().decode()


def _validate(lib, params):
    from aim_amd import capi
    rc = lib.aim_scratch_bytes(capi.params_ref(params), 1000)
    return rc, lib.aim_last_error().decode() if rc == 0 else ""


def _bidir(p):
    from aim_amd import capi
    base = p.base if hasattr(p, "base") else p
    base.flags |= capi.FLAG_WFA_BIDIR
    return p


def test_features_bit(lib):
    from aim_amd import capi, engine
    assert capi.FLAG_WFA_BIDIR == 0x200 and capi.FEATURE_WFA_BIDIR == 0x10
    assert engine.features() & capi.FEATURE_WFA_BIDIR
    assert engine.features() & capi.FEATURE_WFA_W32
    assert lib.aim_abi_version() == 2


def test_rejections(lib):
    from aim_amd import engine
    for algo in ("nw", "swg", "genasm"):
        assert _validate(lib, _bidir(engine.make_params(algo, 100, 1000, backtrace=True))) == (0, "AIM_FLAG_WFA_BIDIR needs AIM_ALGO_WFA"), algo
    assert _validate(lib, _bidir(engine.make_params("wfa", 100, 1000))) == (
        0, "AIM_FLAG_WFA_BIDIR needs AIM_FLAG_BACKTRACE (score-only WFA is O(s) already)")
    for kw, name in ((dict(reduce=True), "AIM_FLAG_REDUCE"), (dict(ends_free=(0, 0, 10, 10)), "AIM_FLAG_ENDSFREE"),
                     (dict(gap2=(24, 1)), "AIM_FLAG_AFFINE2P"), (dict(linear=True), "AIM_FLAG_LINEAR")):
        p = _bidir(engine.make_params("wfa", 100, 1000, backtrace=True, **kw))
        assert _validate(lib, p) == (0, "AIM_FLAG_WFA_BIDIR cannot be combined with %s" % name), kw
    # the rules of the other flags stand with it
    p = engine.make_params("wfa", 100, 32760, backtrace=True, w32=True, req8=True, bidir=True)
    assert _validate(lib, p) == (0, "AIM_FLAG_REQ8 carries int16 lengths: read_size must be < 32760")
    p = engine.make_params("wfa", 100, 40000, backtrace=True, bidir=True)
    assert _validate(lib, p) == (0, "WFA offsets (common.h:98-100) are int16: read_size must be < 32760")
    assert _validate(lib, engine.make_params("wfa", 100, 32752, backtrace=True, req8=True, bidir=True))[0] > 0
    assert _validate(lib, engine.make_params("wfa", 100, 1 << 24, backtrace=True, w32=True, bidir=True))[0] > 0


@pytest.mark.parametrize("l,err,w32", [(100, 0.01, False), (150, 0.02, False), (1000, 0.05, False), (10000, 0.01, False),
                                       (16000, 0.05, False), (40000, 0.01, True), (100000, 0.01, True), (100000, 0.02, True)])
def test_plan_line(lib, l, err, w32):
    from aim_amd import capi, engine
    ms, rs = engine.launcher_sizes("wfa", l, err)
    p = engine.make_params("wfa", ms, rs, backtrace=True, w32=w32, bidir=True)
    rc, line = _describe(lib, p)
    assert rc == 0, line
    assert line.startswith("wfa_bidir_kernel ") and " block=64 " in line, line
    t = int(line.split(" bidir=")[1].split()[0])
    assert t >= 250
    assert line.endswith(" bidir=%d w32" % t if w32 else " bidir=%d" % t), line
    assert lib.aim_scratch_bytes(capi.params_ref(p), 2048) > 0


# Flag-less plan lines and aim_scratch_bytes of the library before the flag existed (AIM_SCRATCH_GB=16, AIM_CHIP_CUS=256, 2 048
# pairs, CIGAR): one shape per kernel family the WFA planner picks (the committed sweep, test_plan_sweep_cpu.py, checks every plan).
FLAGLESS = [
    (100, 0.01, False, 'wfa_lane_kernel n=2048 grid=32 block=64 lds=16896 scratch=256 budget=17179869184', 256),
    (150, 0.02, False, 'wfa_group_kernel n=2048 grid=256 block=64 lds=6440 scratch=11018496 budget=17179869184 G=8 hist=5767168 chunk=2048 fb_grid=2048 packed_in=0 runs_out=0', 11018496),
    (1000, 0.05, False, 'wfa_group_kernel n=2048 grid=1024 block=64 lds=21376 scratch=1846550784 budget=17179869184 G=32 hist=1049100288 chunk=2048 fb_grid=2048 packed_in=0 runs_out=0', 1846550784),
    (10000, 0.01, False, 'wfa_group_kernel n=2048 grid=1536 block=64 lds=25244 scratch=6101803264 budget=17179869184 G=64 hist=4145545216 chunk=2048 fb_grid=1280 packed_in=0 runs_out=0', 6101803264),
    (10000, 0.05, False, 'wfa_wave_kernel n=2048 grid=320 block=64 lds=27696 scratch=12044943360 budget=17179869184 pool_cap=18780076 ring=6x128 seq_lds=1', 12044943360),
    (100000, 0.01, True, 'wfa_wave_kernel n=2048 grid=512 block=64 lds=11264 scratch=17179738112 budget=17179869184 pool_cap=8348528 ring=6x128 seq_lds=0 w32', 17179738112),
]


def test_no_flag_changes_nothing(lib, monkeypatch):
    from aim_amd import capi, engine
    monkeypatch.setenv("AIM_SCRATCH_GB", "16")
    monkeypatch.setenv("AIM_CHIP_CUS", "256")
    for l, err, w32, line, scratch in FLAGLESS:
        ms, rs = engine.launcher_sizes("wfa", l, err)
        p = engine.make_params("wfa", ms, rs, backtrace=True, w32=w32)
        assert _describe(lib, p) == (0, line), (l, err)
        assert lib.aim_scratch_bytes(capi.params_ref(p), 2048) == scratch, (l, err)
        # and planning with the flag in between changes neither
        _describe(lib, engine.make_params("wfa", ms, rs, backtrace=True, w32=w32, bidir=True))
        assert _describe(lib, p) == (0, line), (l, err)


def test_code_object_matches_the_plan(built):
    """wfa_bidir_kernel spills nothing, and its VGPRs allow the 4 waves per SIMD (16 workgroups per CU) the plan assumes."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import codeobj_regs
    regs = {k: v for k, v in codeobj_regs.kernel_regs().items() if "wfa_bidir_kernel" in k}
    assert len(regs) == 2, regs   # int16 and int32 offsets
    for name, r in regs.items():
        assert r["scratch_bytes"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 512 // 4, (name, r)


def test_max_score_at_most_t_skips_the_second_stage(lib, monkeypatch):
    """MAX_SCORE <= T: only the first stage runs; the plan line says grid=0 and the scratch is the first stage's, even under a bound
    too small for one bidirectional workgroup at a larger MAX_SCORE."""
    from aim_amd import capi, engine
    ms, rs = engine.launcher_sizes("wfa", 1000, 0.05)
    assert ms == 250
    rc, line = _describe(lib, engine.make_params("wfa", ms, rs, backtrace=True, bidir=True))
    assert rc == 0 and " grid=0 " in line and line.endswith(" bidir=250"), line
    rc, line = _describe(lib, engine.make_params("wfa", 251, rs, backtrace=True, bidir=True))
    assert rc == 0 and " grid=0 " not in line, line
    monkeypatch.setenv("AIM_SCRATCH_GB", "0.25")
    rs = 1 << 24
    assert _describe(lib, engine.make_params("wfa", 1 << 23, rs, backtrace=True, w32=True, bidir=True))[0] != 0
    p = engine.make_params("wfa", 200, rs, backtrace=True, w32=True, bidir=True)
    rc, line = _describe(lib, p, 8)
    assert rc == 0 and " grid=0 " in line, line
    assert lib.aim_scratch_bytes(capi.params_ref(p), 8) > 0


def test_scratch_is_o_of_max_score(lib, monkeypatch):
    """l = 100 000, MAX_SCORE 5 000, 2 048 pairs, a bound large enough for the flag-less history: bidir needs under 1/50 of it."""
    from aim_amd import capi, engine
    monkeypatch.setenv("AIM_SCRATCH_GB", "100000")
    ms, rs = engine.launcher_sizes("wfa", 100000, 0.01)
    assert ms == 5000
    flagless = lib.aim_scratch_bytes(capi.params_ref(engine.make_params("wfa", ms, rs, backtrace=True, w32=True)), 2048)
    bidir = lib.aim_scratch_bytes(capi.params_ref(engine.make_params("wfa", ms, rs, backtrace=True, w32=True, bidir=True)), 2048)
    assert 0 < bidir * 50 < flagless, (bidir, flagless)


def test_enomem_when_one_workgroup_does_not_fit(lib, monkeypatch):
    from aim_amd import engine
    monkeypatch.setenv("AIM_SCRATCH_GB", "0.25")
    rs = 1 << 24   # two windows of about 2 x 2^23 diagonals: more than the whole bound
    rc, err = _describe(lib, engine.make_params("wfa", 1 << 23, rs, backtrace=True, w32=True, bidir=True))
    assert rc != 0 and "scratch budget too small" in err, err


def test_make_params_bidir():
    from aim_amd import capi, engine
    p = engine.make_params("wfa", 100, 1000, backtrace=True, bidir=True)
    assert p.flags == capi.FLAG_BACKTRACE | capi.FLAG_WFA_BIDIR
    p = engine.make_params("wfa", 100, 40000, backtrace=True, w32=True, bidir=True)
    assert p.flags == capi.FLAG_BACKTRACE | capi.FLAG_WFA_BIDIR | capi.FLAG_WFA_W32
    with pytest.raises(ValueError, match="needs backtrace"):
        engine.make_params("wfa", 100, 1000, bidir=True)
    for kw in (dict(reduce=True), dict(ends_free=(1, 2, 3, 4)), dict(gap2=(24, 1)), dict(linear=True)):
        with pytest.raises(ValueError, match="bidir cannot be combined"):
            engine.make_params("wfa", 100, 1000, backtrace=True, bidir=True, **kw)
    assert engine.make_params("wfa", 100, 1000, backtrace=True).flags == capi.FLAG_BACKTRACE


def _host(args):
    from aim_amd import build
    return subprocess.run([build.HOST_BIN] + args, capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("extra,msg", [(["--algo", "nw", "--backtrace"], "--bidir needs --algo wfa"),
                                       (["--algo", "wfa"], "--bidir needs --backtrace"),
                                       (["--algo", "wfa", "--backtrace", "--reduce"], "--bidir cannot be combined with --reduce"),
                                       (["--algo", "wfa", "--backtrace", "--ends-free", "1,1,1,1"], "--bidir cannot be combined with --ends-free"),
                                       (["--algo", "wfa", "--backtrace", "--gap2", "24,1"], "--bidir cannot be combined with --gap2"),
                                       (["--algo", "wfa", "--backtrace", "--linear"], "--bidir cannot be combined with --linear")])
def test_host_bidir_refusals(built, tmp_path, extra, msg):
    inp = tmp_path / "in.txt"
    inp.write_text(">ACGT\n<ACGT\n" * 4)
    p = _host([str(inp), str(tmp_path / "o"), "4", "--max-score", "10", "--read-size", "16", "--bidir"] + extra +
              ["--pack-only", str(tmp_path / "d")])
    assert p.returncode == 1 and msg in p.stderr, p.stdout + p.stderr


def test_launcher_passes_bidir(built):
    from aim_amd import launch
    cfg = launch.parse("wfa", ["-i", "in", "-o", "out", "-l", "1000", "-e", "0.05", "-n", "4", "-b", "--bidir"])
    assert cfg["bidir"] and launch.host_command(cfg)[-1] == "--bidir"
    cfg = launch.parse("wfa", ["-i", "in", "-o", "out", "-l", "100", "-e", "0.01", "-n", "4", "-b"])
    assert not cfg["bidir"] and "--bidir" not in launch.host_command(cfg)
    with pytest.raises(SystemExit):
        launch.parse("swg", ["-i", "in", "-o", "out", "-l", "100", "-e", "0.01", "-n", "4", "--bidir"])
