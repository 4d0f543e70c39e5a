"""32-bit WFA offsets, AIM_FLAG_WFA_W32: what needs no GPU -- the feature bit, validation, the plans it gets, the bindings, the CLI's
argument checks, and the banded DP model (tests/w32_model.py) the GPU tests check long reads against, itself checked against the
full-width models and the oracle's global WFA."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import affine2p_model
import endsfree_model
import linear_model
import w32_model

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


def _validate(lib, params):
    from aim_amd import capi
    rc = lib.aim_scratch_bytes(capi.params_ref(params), 1000)
    return rc, lib.aim_last_error().decode() if rc == 0 else ""


def test_features_bit(lib):
    from aim_amd import capi, engine
    assert capi.FLAG_WFA_W32 == 0x100 and capi.FEATURE_WFA_W32 == 0x8
    assert engine.features() & capi.FEATURE_WFA_W32
    assert engine.features() & capi.FEATURE_LINEAR and engine.features() & capi.FEATURE_AFFINE2P
    assert engine.features() & capi.FEATURE_ENDSFREE
    assert lib.aim_abi_version() == 2


def test_read_size_40000_accepted(lib):
    from aim_amd import engine
    p = engine.make_params("wfa", 2000, 40000, backtrace=True, w32=True)
    rc, line = _describe(lib, p, 16)
    assert rc == 0, lib.aim_last_error()
    assert line.startswith("wfa_wave_kernel ") and line.endswith(" w32"), line


@pytest.mark.parametrize("rs", [32760, 65536, 1 << 24])
def test_read_sizes_up_to_2_24(lib, rs):
    from aim_amd import engine
    for kw in (dict(), dict(backtrace=True), dict(reduce=True), dict(res8=True)):
        p = engine.make_params("wfa", 100, rs, w32=True, **kw)
        rc, err = _validate(lib, p)
        assert rc > 0, (rs, kw, err)


def test_rejections(lib):
    from aim_amd import engine
    p = engine.make_params("wfa", 100, (1 << 24) + 8, w32=True)
    assert _validate(lib, p) == (0, "read_size must be <= 2^24")
    for algo in ("nw", "swg", "genasm"):
        p = engine.make_params(algo, 100, 1000, w32=True)
        assert _validate(lib, p) == (0, "AIM_FLAG_WFA_W32 needs AIM_ALGO_WFA"), algo
    # int16 lengths on the wire keep their bound
    p = engine.make_params("wfa", 100, 32760, w32=True, req8=True)
    assert _validate(lib, p) == (0, "AIM_FLAG_REQ8 carries int16 lengths: read_size must be < 32760")
    assert _validate(lib, engine.make_params("wfa", 100, 32752, w32=True, req8=True))[0] > 0
    # the other flags' rules stand with the flag
    p = engine.make_params("wfa", 100, 40000, w32=True, backtrace=True, res8=True)
    assert _validate(lib, p) == (0, "AIM_FLAG_RES8 (idx, score results) cannot be combined with AIM_FLAG_BACKTRACE")
    p = engine.make_params("wfa", 100, 40000, w32=True, ends_free=(0, 0, 10, 10), reduce=True)
    assert _validate(lib, p) == (0, "AIM_FLAG_ENDSFREE cannot be combined with AIM_FLAG_REDUCE")
    p = engine.make_params("wfa", 100, 40000, w32=True, gap2=(24, 1), reduce=True)
    assert _validate(lib, p) == (0, "AIM_FLAG_AFFINE2P cannot be combined with AIM_FLAG_REDUCE")


def test_no_flag_message_unchanged(lib):
    from aim_amd import engine
    for rs in (32760, 40000):
        assert _validate(lib, engine.make_params("wfa", 100, rs)) == (0, "WFA offsets (common.h:98-100) are int16: read_size must be < 32760")
    assert _validate(lib, engine.make_params("nw", 100, 32760)) == (0, "NW/SWG cells are int16: read_size must be < 32760")
    rc, line = _describe(lib, engine.make_params("wfa", 100, 1000))
    assert rc == 0 and not line.endswith(" w32"), line


MODES = [dict(), dict(reduce=True), dict(ends_free=(0, 0, 50, 50)), dict(gap2=(24, 1)), dict(linear=True, mismatch=1, gap_e=1)]


@pytest.mark.parametrize("mode", range(len(MODES)))
@pytest.mark.parametrize("bt", [False, True])
def test_plans_are_wave_w32(lib, mode, bt):
    """Every mode, every READ_SIZE (the lane / group kernels' shapes included): wfa_wave_kernel alone, no fallback stage."""
    from aim_amd import capi, engine
    for l, err in ((100, 0.01), (100, 0.05), (150, 0.02), (1000, 0.05), (10000, 0.01), (16000, 0.01), (40000, 0.01),
                   (100000, 0.01)):
        ms, rs = engine.launcher_sizes("wfa", l, err)
        for kw in (dict(), dict(req8=True), dict(res8=True)):
            if ("req8" in kw and rs >= 32760) or ("res8" in kw and bt):
                continue
            p = engine.make_params("wfa", ms, rs, backtrace=bt, w32=True, **MODES[mode], **kw)
            rc, line = _describe(lib, p, 4096)
            assert rc == 0, (l, err, kw, lib.aim_last_error())
            assert line.startswith("wfa_wave_kernel ") and line.endswith(" w32"), line
            assert lib.aim_scratch_bytes(capi.params_ref(p), 4096) > 0


def test_w32_pool_in_int32_bytes(lib, monkeypatch):
    """The ring cap, ring bytes and pool are sized by 4-byte offsets: a W32 plan's LDS ring holds half the diagonals of int16's at
    the same shape, or its scratch is larger."""
    from aim_amd import engine
    ms, rs = engine.launcher_sizes("wfa", 10000, 0.01)
    fields = []
    monkeypatch.setenv("AIM_FORCE_WAVE", "1")
    for w32 in (False, True):
        rc, line = _describe(lib, engine.make_params("wfa", ms, rs, backtrace=True, w32=w32), 64)
        assert rc == 0 and line.startswith("wfa_wave_kernel"), line
        kv = dict(t.split("=", 1) for t in line.split() if "=" in t)
        fields.append(kv)
    a, b = fields
    slots_a, w_a = (int(v) for v in a["ring"].split("x"))
    slots_b, w_b = (int(v) for v in b["ring"].split("x"))
    assert slots_a * w_a * 2 <= 24 * 1024 and slots_b * w_b * 4 <= 24 * 1024
    assert int(b["scratch"]) / int(b["grid"]) > int(a["scratch"]) / int(a["grid"])


def test_make_params_w32():
    from aim_amd import capi, engine
    p = engine.make_params("wfa", 100, 40000, w32=True)
    assert p.flags == capi.FLAG_WFA_W32
    p = engine.make_params("wfa", 100, 40000, w32=True, backtrace=True, reduce=True)
    assert p.flags == capi.FLAG_WFA_W32 | capi.FLAG_BACKTRACE | capi.FLAG_REDUCE
    for kw, flag in ((dict(ends_free=(1, 2, 3, 4)), capi.FLAG_ENDSFREE), (dict(gap2=(24, 1)), capi.FLAG_AFFINE2P),
                     (dict(linear=True), capi.FLAG_LINEAR)):
        p = engine.make_params("wfa", 100, 40000, w32=True, **kw)
        base = p.base if hasattr(p, "base") else p
        assert base.flags == capi.FLAG_WFA_W32 | flag, kw
    assert engine.make_params("wfa", 100, 1000).flags == 0


def _host(args):
    from aim_amd import build
    return subprocess.run([build.HOST_BIN] + args, capture_output=True, text=True, timeout=60)


def test_host_w32_arguments(built, tmp_path):
    inp = tmp_path / "in.txt"
    inp.write_text(">ACGT\n<ACGT\n" * 4)
    p = _host([str(inp), str(tmp_path / "o"), "4", "--algo", "nw", "--max-score", "10", "--read-size", "40000", "--w32"])
    assert p.returncode == 1 and "--w32 needs --algo wfa" in p.stderr, p.stdout + p.stderr
    p = _host([str(inp), str(tmp_path / "o"), "4", "--algo", "wfa", "--max-score", "10", "--read-size", "40000", "--w32x", "1"])
    assert p.returncode == 1 and "unknown flag --w32x" in p.stderr


def test_launcher_passes_w32(built):
    from aim_amd import launch
    cfg = launch.parse("wfa", ["-i", "in", "-o", "out", "-l", "50000", "-e", "0.01", "-n", "4", "--w32"])
    assert cfg["w32"] and cfg["read_size"] >= 50000
    assert launch.host_command(cfg)[-1] == "--w32"
    cfg = launch.parse("wfa", ["-i", "in", "-o", "out", "-l", "100", "-e", "0.01", "-n", "4"])
    assert not cfg["w32"] and "--w32" not in launch.host_command(cfg)
    with pytest.raises(SystemExit):
        launch.parse("swg", ["-i", "in", "-o", "out", "-l", "100", "-e", "0.01", "-n", "4", "--w32"])


@pytest.mark.parametrize("length,extra", [(50000, []), (100000, []), (50000, ["--long-indel", "400"])])
def test_gen_dataset_long_reads(built, tmp_path, length, extra):
    """Text and packed files of rows of 50 kb and 100 kb: lengths beyond int16 and 16-byte requests in the packed file."""
    from aim_amd import engine, gen_dataset
    txt_out, pk_out = tmp_path / "in.txt", tmp_path / "in.pk"
    base = ["-n", "3", "-l", str(length), "-e", "0.01", "-s", "5"] + extra
    assert gen_dataset.main(base + ["-o", str(txt_out)]) == 0
    assert gen_dataset.main(base + ["-o", str(pk_out), "--packed"]) == 0
    lines = txt_out.read_bytes().split(b"\n")
    assert len(lines) == 7 and all(len(x) - 1 >= length - length // 50 for x in lines[:6])
    hdr = np.frombuffer(pk_out.read_bytes()[8:32], dtype="<u4")
    assert hdr[0] == 1 and hdr[1] >= length and hdr[2] == 16, hdr
    req, _, _ = engine.parse_pairs(txt_out.read_bytes(), engine.round_up_8(length + length // 50 + 800))
    assert (req["pattern_len"] == length).all() and (req["text_len"] > 32767).all()


# ---- the banded model -------------------------------------------------------------------------------------------------------

def _pairs(seed, n, l, err):
    from aim_amd import engine
    _, rs = engine.launcher_sizes("wfa", l, err)
    return engine.gen_pairs(seed, 0, n, l, err, rs)


def _agrees(banded, exact, cap):
    """Exact at or below the cap, above the cap elsewhere."""
    return bool(np.all(np.where(exact <= cap, banded == exact, banded > cap)))


@pytest.mark.parametrize("l,err", [(150, 0.05), (1000, 0.02), (2000, 0.01)])
def test_band_exact_global_and_affine2p(built, l, err):
    req, pat, txt = _pairs(900 + l, 24, l, err)
    assert (req["pattern_len"] != req["text_len"]).any()
    for x, o, e in ((3, 4, 1), (4, 6, 2)):
        exact = affine2p_model.single_affine_scores(req, pat, txt, x, o, e)
        for cap in (int(exact.min()), int(np.median(exact)), int(exact.max()), int(exact.max()) + 7):   # pairs at and near the cap
            assert _agrees(w32_model.dp_scores(req, pat, txt, cap, x, o, e), exact, cap), (x, o, e, cap)
    exact = affine2p_model.dp_scores(req, pat, txt, 4, 4, 2, 24, 1)
    for cap in (int(exact.min()), int(np.median(exact)), int(exact.max())):
        assert _agrees(w32_model.dp_scores(req, pat, txt, cap, 4, 4, 2, gap2=(24, 1)), exact, cap), cap


@pytest.mark.parametrize("l,err", [(150, 0.05), (2000, 0.01)])
def test_band_exact_affine2p_long_indel(built, l, err):
    from aim_amd import engine
    req, pat, txt = _pairs(300 + l, 16, l, err)
    req, pat, txt = engine.long_indel_pairs(3, 0, req, pat, txt, 60)
    exact = affine2p_model.dp_scores(req, pat, txt, 4, 4, 2, 24, 1)
    for cap in (int(np.median(exact)), int(exact.max())):
        assert _agrees(w32_model.dp_scores(req, pat, txt, cap, 4, 4, 2, gap2=(24, 1)), exact, cap), cap


@pytest.mark.parametrize("pen", [(1, 1), (4, 2), (2, 3)])
def test_band_exact_linear(built, pen):
    req, pat, txt = _pairs(41, 24, 1000, 0.03)
    exact = linear_model.dp_scores(req, pat, txt, *pen)
    for cap in (int(exact.min()), int(np.median(exact)), int(exact.max())):
        assert _agrees(w32_model.dp_scores(req, pat, txt, cap, pen[0], 0, pen[1], linear=True), exact, cap), cap


@pytest.mark.parametrize("ef", [(0, 0, 16, 16), (3, 5, 16, 10), (7, 0, 0, 9)])
def test_band_exact_endsfree(built, ef):
    from aim_amd import engine
    req, pat, txt = _pairs(61, 24, 1000, 0.02)
    req, pat, txt = engine.flank_pairs(61, 0, req, pat, txt, 16)
    exact = endsfree_model.dp_scores(req, pat, txt, 3, 4, 1, ef)
    for cap in (int(exact.min()), int(np.median(exact)), int(exact.max())):
        assert _agrees(w32_model.dp_scores(req, pat, txt, cap, 3, 4, 1, ends_free=ef), exact, cap), (ef, cap)


@pytest.mark.parametrize("l,err", [(100, 0.05), (1000, 0.05), (2000, 0.02)])
def test_band_equals_oracle_wfa(built, l, err):
    from aim_amd import engine
    from oracle import oracle
    ms, rs = engine.launcher_sizes("wfa", l, err)
    req, pat, txt = engine.gen_pairs(123 + l, 0, 64, l, err, rs)
    full, _, _ = oracle.align_batch(oracle.params("wfa", ms, rs), req["pattern_len"], req["text_len"], pat, txt, nthreads=4)
    cap = int(np.median(full["score"]))   # about half the pairs over the cap
    op = oracle.params("wfa", cap, rs)
    ores, _, _ = oracle.align_batch(op, req["pattern_len"], req["text_len"], pat, txt, nthreads=4)
    banded = w32_model.dp_scores(req, pat, txt, cap)
    under = ores["score"] <= cap
    assert under.any() and (~under).any()
    assert np.array_equal(banded[under], ores["score"][under])
    assert (banded[~under] > cap).all()
