"""Dual-cost gap-affine WFA on the GPU (AIM_FLAG_AFFINE2P): a piece 2 equal to piece 1, or one that never fits under MAX_SCORE,
reproduces global WFA (and the oracle) byte for byte; long-indel pairs match the DP model of tests/affine2p_model.py, with CIGARs
that use up both sequences and re-score to the reported score; every path (wfa_group, wfa_wave, the to-do list, history chunks,
packed input, compact runs, the host CLI) agrees."""
import os
import re
import subprocess

import numpy as np
import pytest

from affine2p_model import check_cigar, dp_scores, rescore, single_affine_scores

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(built):
    import ctypes as C
    from aim_amd import capi
    lib = capi.load()
    n = C.c_int()
    assert lib.aim_device_count(C.byref(n)) == 0 and n.value >= 1, lib.aim_last_error()
    return lib


def _ops_str(ops, r):
    return bytes(ops[int(r["begin_offset"]):int(r["end_offset"])]).decode()


def _plan(params, n):
    from aim_amd import engine
    with engine.DeviceSet(1) as s:
        s.configure(params, n)
        return s.plan_describe(0)


def _same_as_global(req, pat, txt, ms, rs, bt, pen, gap2):
    from aim_amd import engine
    from oracle import oracle
    x, o, e = pen
    kw = dict(mismatch=x, gap_o=o, gap_e=e, backtrace=bt)
    a2p = engine.make_params("wfa", ms, rs, gap2=gap2, **kw)
    assert ("affine2p=%d,%d" % gap2) in _plan(a2p, len(req))
    res, ops = engine.align(a2p, req, pat, txt)
    gres, gops = engine.align(engine.make_params("wfa", ms, rs, **kw), req, pat, txt)
    op = oracle.params("wfa", ms, rs, mismatch=x, gap_o=o, gap_e=e, backtrace=bt)
    ores, oops, _ = oracle.align_batch(op, req["pattern_len"], req["text_len"], pat, txt, nthreads=8)
    ok = ores["score"] <= ms
    assert ok.sum() > 0.5 * len(req)
    assert np.array_equal(res["score"], gres["score"])
    assert np.array_equal(res["score"][ok], ores["score"][ok])
    assert (res["status"] == 0).all()
    if bt:
        for f in ("max_operations", "begin_offset", "end_offset"):
            assert np.array_equal(res[f], gres[f]), f
            assert np.array_equal(res[f][ok], ores[f][ok]), f
        for i in range(len(req)):
            b, e_ = int(res["begin_offset"][i]), int(res["end_offset"][i])
            assert bytes(ops[i, b:e_]) == bytes(gops[i, b:e_]), i
            if ok[i]:
                assert bytes(ops[i, b:e_]) == bytes(oops[i, b:e_]), i


@pytest.mark.parametrize("piece2", ["equal", "over_cap"])
@pytest.mark.parametrize("l,err,bt,pen", [(100, 0.01, False, (3, 4, 1)), (100, 0.01, True, (3, 4, 1)), (100, 0.05, True, (4, 6, 2)),
                                          (100, 0.05, False, (4, 6, 2)), (1000, 0.05, True, (3, 4, 1))])
def test_degenerate_piece2_equals_global_wfa(gpu, l, err, bt, pen, piece2):
    from aim_amd import engine
    ms, rs = engine.launcher_sizes("wfa", l, err, mismatch=pen[0], gap_o=pen[1], gap_e=pen[2])
    n = 400 if l >= 1000 else 3000
    req, pat, txt = engine.gen_pairs(91 + l, 0, n, l, err, rs)
    gap2 = (pen[1], pen[2]) if piece2 == "equal" else (ms, 1)   # o2 + e2 = MAX_SCORE + 1: piece 2 never fires
    _same_as_global(req, pat, txt, ms, rs, bt, pen, gap2)


def _long(seed, n, l, err, L):
    from aim_amd import engine
    _, rs = engine.launcher_sizes("wfa", l, err)
    req, pat, txt = engine.gen_pairs(seed, 0, n, l, err, rs)
    return engine.long_indel_pairs(seed, 0, req, pat, txt, L)


def _check(req, pat, txt, res, ops, ms, pen, scores_only=False):
    want = dp_scores(req, pat, txt, *pen)
    want = np.where(want <= ms, want, ms + 1)
    assert (res["score"] == want).all(), np.nonzero(res["score"] != want)[0][:10]
    if scores_only:
        return
    assert (res["status"] == 0).all()
    for i in range(len(req)):
        r = res[i]
        plen, tlen = int(req["pattern_len"][i]), int(req["text_len"][i])
        assert r["max_operations"] == plen + tlen and r["end_offset"] == plen + tlen
        if r["score"] > ms:   # global WFA's over-cap result
            assert r["begin_offset"] == r["end_offset"] - 1, i
            continue
        s = _ops_str(ops[i], r)
        err = check_cigar(s, bytes(pat[i, :plen]), bytes(txt[i, :tlen]))
        assert err is None, (i, err, s)
        assert rescore(s, *pen) == r["score"], (i, s)


# (x, o1, e1, o2, e2). The second set never lets piece 2 pay off (e2 == e1, o2 > o1); the third has e2 < e1 and a score unit of 2.
PENS = [(4, 4, 2, 24, 1), (3, 4, 1, 12, 1), (4, 2, 4, 10, 2)]
ACTIVE = [PENS[0], PENS[2]]   # the sets where piece 2 is cheaper for long gaps


def _ms(pen, ms):
    """MAX_SCORE for a penalty set: a long gap costs about e2 per base."""
    return ms * pen[4]


@pytest.mark.parametrize("pen", PENS)
@pytest.mark.parametrize("l,err,L,ms", [(150, 0.01, 40, 80), (150, 0.01, 60, 120), (200, 0.02, 120, 200), (400, 0.01, 300, 360)])
def test_long_indel_pairs_match_dp_model(gpu, pen, l, err, L, ms):
    from aim_amd import engine
    n = 300 if L >= 300 else 800
    req, pat, txt = _long(7 * L + l, n, l, err, L)
    rs = pat.shape[1]
    ms = _ms(pen, ms)
    params = engine.make_params("wfa", ms, rs, mismatch=pen[0], gap_o=pen[1], gap_e=pen[2], backtrace=True, gap2=pen[3:])
    res, ops = engine.align(params, req, pat, txt)
    _check(req, pat, txt, res, ops, ms, pen)
    single = np.minimum(single_affine_scores(req, pat, txt, *pen[:3]), ms + 1)
    if pen[4] < pen[2]:   # piece 2 acts: most pairs score below single-affine
        assert (res["score"] < single).mean() > 0.5
    else:                 # e2 == e1 and o2 > o1: piece 2 never pays off, the scores are single-affine's
        assert np.array_equal(res["score"], single)
    res8, _ = engine.align(engine.make_params("wfa", ms, rs, mismatch=pen[0], gap_o=pen[1], gap_e=pen[2], res8=True, gap2=pen[3:]),
                           req, pat, txt)
    assert np.array_equal(res8["score"], res["score"])


@pytest.mark.parametrize("pen", PENS)
@pytest.mark.parametrize("bt", [True, False])
def test_wave_kernel_agrees(gpu, monkeypatch, pen, bt):
    from aim_amd import engine
    req, pat, txt = _long(5, 600, 150, 0.01, 60)
    ms, rs = _ms(pen, 120), pat.shape[1]
    params = engine.make_params("wfa", ms, rs, mismatch=pen[0], gap_o=pen[1], gap_e=pen[2], backtrace=bt, gap2=pen[3:])
    assert _plan(params, len(req)).startswith("wfa_group_kernel")
    monkeypatch.setenv("AIM_FORCE_WAVE", "1")
    assert _plan(params, len(req)).startswith("wfa_wave_kernel")
    res, ops = engine.align(params, req, pat, txt)
    _check(req, pat, txt, res, ops, ms, pen, scores_only=not bt)


@pytest.mark.parametrize("pen", PENS)
def test_pairs_with_n_bases(gpu, pen):
    from aim_amd import engine
    req, pat, txt = _long(9, 800, 150, 0.01, 40)
    rng = np.random.default_rng(9)
    for i in range(0, 800, 7):
        pat[i, rng.integers(0, req["pattern_len"][i])] = ord("N")
        txt[i, rng.integers(0, req["text_len"][i])] = ord("N")
    ms, rs = _ms(pen, 100), pat.shape[1]
    params = engine.make_params("wfa", ms, rs, mismatch=pen[0], gap_o=pen[1], gap_e=pen[2], backtrace=True, gap2=pen[3:])
    assert _plan(params, len(req)).startswith("wfa_group_kernel")
    res, ops = engine.align(params, req, pat, txt)
    _check(req, pat, txt, res, ops, ms, pen)


@pytest.mark.parametrize("pen", ACTIVE)
@pytest.mark.parametrize("bt", [True, False])
def test_narrow_rows_overflow_to_wave(gpu, monkeypatch, bt, pen):
    """Rows of 32 entries (AIM_GROUP_WLDS): every pair whose wavefront outgrows 30 diagonals leaves for the general kernel."""
    from aim_amd import engine
    req, pat, txt = _long(11, 800, 150, 0.02, 40)
    ms, rs = _ms(pen, 100), pat.shape[1]
    params = engine.make_params("wfa", ms, rs, mismatch=pen[0], gap_o=pen[1], gap_e=pen[2], backtrace=bt, gap2=pen[3:])
    monkeypatch.setenv("AIM_GROUP_WLDS", "32")
    assert _plan(params, len(req)).startswith("wfa_group_kernel")
    res, ops = engine.align(params, req, pat, txt)
    _check(req, pat, txt, res, ops, ms, pen, scores_only=not bt)


def _hist_pair_bytes(ms):
    rows = ms + 2                                    # unit 1
    pool_off = 16 + rows * 8
    runs_off = (pool_off + rows * rows * 16 + 15) & ~15
    return (runs_off + (2 * ms + 16) * 4 + 255) & ~255


def test_history_in_several_chunks(gpu, monkeypatch):
    from aim_amd import engine
    pen = (3, 4, 1, 12, 1)
    ms, rs = engine.launcher_sizes("wfa", 100, 0.05)
    n = 12000
    req, pat, txt = engine.gen_pairs(31, 0, n, 100, 0.05, rs)
    params = engine.make_params("wfa", ms, rs, backtrace=True, gap2=pen[3:])
    res0, ops0 = engine.align(params, req, pat, txt)
    _check(req[:2000], pat[:2000], txt[:2000], res0[:2000], ops0[:2000], ms, pen)
    fit = 5000                                       # pairs per history buffer: three launches of the compute + traceback pair
    monkeypatch.setenv("AIM_SCRATCH_GB", "%.6f" % (4.0 * fit * _hist_pair_bytes(ms) / (1 << 30) + 0.02))
    line = _plan(params, n)
    assert line.startswith("wfa_group_kernel"), line
    chunk = int(re.search(r" chunk=(\d+)", line).group(1))
    assert 0 < chunk < n // 2, line                  # the batch really runs as several launches
    res1, ops1 = engine.align(params, req, pat, txt)
    assert np.array_equal(res0, res1)
    assert engine.format_output(res0, ops0, True) == engine.format_output(res1, ops1, True)


def test_packed_input_and_compact_runs(gpu):
    from aim_amd import engine
    pen = (4, 4, 2, 24, 1)
    req, pat, txt = _long(21, 2048, 150, 0.01, 40)
    for i in range(0, 2048, 50):
        txt[i, 3] = ord("N")
    ms, rs = 100, pat.shape[1]
    kw = dict(mismatch=pen[0], gap_o=pen[1], gap_e=pen[2], backtrace=True, gap2=pen[3:])
    ref, rops = engine.align(engine.make_params("wfa", ms, rs, **kw), req, pat, txt)
    _check(req, pat, txt, ref, rops, ms, pen)
    want = engine.format_output(ref, rops, True)
    params = engine.make_params("wfa", ms, rs, req8=True, **kw)
    cap = 16 * 2048
    with engine.DeviceSet(1) as s:
        s.configure_slots(params, 2048, slots=2, max_raw=2048, max_runs=cap)
        assert "affine2p=24,1" in s.plan_describe(0)
        s.submit(0, 0, req, packed=engine.pack_batch(req, pat, txt), cigar_runs_cap=cap)
        s.submit(0, 1, req, pat, txt, cigar_runs_cap=cap, want_ops=True)
        a = s.wait(0, 0)
        b = s.wait(0, 1)
    for out in (a, b):
        assert np.array_equal(out["cig"]["score"], ref["score"])
        assert engine.format_output_runs(out["cig"], out["runs"]) == want
    assert np.array_equal(b["res"]["score"], ref["score"])


@pytest.mark.parametrize("pen,ms", [(PENS[0], 60), (PENS[2], 80)])
@pytest.mark.parametrize("wave", [False, True])
def test_over_cap_pairs_like_global_wfa(gpu, monkeypatch, wave, pen, ms):
    from aim_amd import engine
    req, pat, txt = _long(3, 1000, 150, 0.02, 40)
    rs = pat.shape[1]
    if wave:
        monkeypatch.setenv("AIM_FORCE_WAVE", "1")
    res, ops = engine.align(engine.make_params("wfa", ms, rs, mismatch=pen[0], gap_o=pen[1], gap_e=pen[2], backtrace=True,
                                               gap2=pen[3:]), req, pat, txt)
    over = res["score"] > ms
    assert over.sum() > 100 and (~over).sum() > 100
    assert (res["score"][over] == ms + 1).all() and (res["status"] == 0).all()
    assert (res["begin_offset"][over] == res["end_offset"][over] - 1).all()
    _check(req, pat, txt, res, ops, ms, pen)


def test_debug_poison_changes_nothing(gpu, monkeypatch):
    from aim_amd import engine
    req, pat, txt = _long(17, 1000, 150, 0.01, 40)
    ms, rs = 100, pat.shape[1]
    params = engine.make_params("wfa", ms, rs, mismatch=4, gap_o=4, gap_e=2, backtrace=True, gap2=(24, 1))
    res0, ops0 = engine.align(params, req, pat, txt)
    for k, v in (("AIM_DEBUG_POISON_SCRATCH", "165"), ("AIM_DEBUG_POISON_LDS", "90"), ("AIM_DEBUG_POISON_OPS", "7")):
        monkeypatch.setenv(k, v)
    res1, ops1 = engine.align(params, req, pat, txt)
    assert np.array_equal(res0, res1)
    assert engine.format_output(res0, ops0, True) == engine.format_output(res1, ops1, True)


@pytest.mark.parametrize("bt", [True, False])
def test_host_cli_gap2(gpu, tmp_path, bt):
    from aim_amd import build, engine, gen_dataset
    n, l, e, L = 3000, 150, 0.01, 40
    txt_in = tmp_path / "in.txt"
    pk_in = tmp_path / "in.pk"
    assert gen_dataset.main(["-n", str(n), "-l", str(l), "-e", str(e), "-o", str(txt_in), "--long-indel", str(L), "-s", "8"]) == 0
    assert gen_dataset.main(["-n", str(n), "-l", str(l), "-e", str(e), "-o", str(pk_in), "--long-indel", str(L), "-s", "8", "--packed"]) == 0
    _, rs0 = engine.launcher_sizes("wfa", l, e)
    rs = engine.round_up_8(rs0 + L)
    ms = 60   # some pairs over the cap
    pen = (4, 4, 2, 24, 1)
    req, pat, txt = engine.parse_pairs(txt_in.read_bytes(), rs)
    res, ops = engine.align(engine.make_params("wfa", ms, rs, mismatch=4, gap_o=4, gap_e=2, backtrace=bt, gap2=(24, 1)), req, pat, txt)
    _check(req, pat, txt, res, ops, ms, pen, scores_only=not bt)
    want = engine.format_output(res, ops, bt)
    outs = []
    for src, extra in ((txt_in, []), (pk_in, ["--packed-input"]), (txt_in, ["--full-ops"] if bt else ["--no-pack"])):
        out = tmp_path / ("out%d" % len(outs))
        cmd = [build.HOST_BIN, str(src), str(out), str(n), "--algo", "wfa", "--max-score", str(ms), "--read-size", str(rs),
               "--mismatch", "4", "--gap-o", "4", "--gap-e", "2", "--gap2", "24,1", "--threads", "4"] + (["--backtrace"] if bt else []) + extra
        p = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        assert "wfa_group_kernel" in p.stdout, p.stdout
        outs.append(out.read_bytes())
    assert outs[0] == want
    assert outs[1] == outs[0]
    assert outs[2] == outs[0]
