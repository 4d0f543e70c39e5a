"""Ends-free (semi-global) WFA on the GPU (AIM_FLAG_ENDSFREE): zero free lengths reproduce the oracle's global WFA bit for bit;
flanked pairs match the DP model of tests/endsfree_model.py, with CIGARs that use up both sequences and re-score to the reported
score; every output path (default ABI, RES8, compact runs, packed input, the host CLI) agrees."""
import os
import subprocess

import numpy as np
import pytest

from endsfree_model import check_cigar, dp_scores, rescore

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


def _zero_free_vs_oracle(req, pat, txt, ms, rs, bt, pen=(3, 4, 1)):
    from aim_amd import engine
    from oracle import oracle
    x, o, e = pen
    params = engine.make_params("wfa", ms, rs, mismatch=x, gap_o=o, gap_e=e, backtrace=bt, ends_free=(0, 0, 0, 0))
    res, ops = engine.align(params, req, pat, txt)
    op = oracle.params("wfa", ms, rs, mismatch=x, gap_o=o, gap_e=e, backtrace=bt)
    ores, oops, _ = oracle.align_batch(op, req["pattern_len"], req["text_len"], pat, txt, nthreads=8)
    ok = ores["score"] <= ms
    assert ok.sum() > 0.5 * len(req)
    assert np.array_equal(res["score"][ok], ores["score"][ok])
    assert (res["score"][~ok] == ms + 1).all()
    assert (res["status"] == 0).all()
    if bt:
        for f in ("max_operations", "begin_offset", "end_offset"):
            assert np.array_equal(res[f][ok], ores[f][ok]), f
        for i in np.nonzero(ok)[0]:
            b, e_ = int(res["begin_offset"][i]), int(res["end_offset"][i])
            assert bytes(ops[i, b:e_]) == bytes(oops[i, b:e_]), i


@pytest.mark.parametrize("l,err,bt,pen", [(100, 0.01, False, (3, 4, 1)), (100, 0.01, True, (3, 4, 1)), (100, 0.02, True, (4, 6, 2)),
                                          (150, 0.02, True, (3, 4, 1)), (1000, 0.05, True, (3, 4, 1))])
def test_zero_free_lengths_equal_global_wfa(gpu, l, err, bt, pen):
    from aim_amd import engine
    ms, rs = engine.launcher_sizes("wfa", l, err, mismatch=pen[0], gap_o=pen[1], gap_e=pen[2])
    n = 600 if l >= 1000 else 4000
    req, pat, txt = engine.gen_pairs(71 + l, 0, n, l, err, rs)
    _zero_free_vs_oracle(req, pat, txt, ms, rs, bt, pen)


@pytest.mark.parametrize("fixture", ["sample_bytes", "err_bytes"])
def test_zero_free_lengths_equal_global_wfa_fixtures(gpu, request, fixture):
    from aim_amd import engine
    ms, rs = engine.launcher_sizes("wfa", 100, 0.01)
    req, pat, txt = engine.parse_pairs(request.getfixturevalue(fixture), rs, max_pairs=3000)
    _zero_free_vs_oracle(req, pat, txt, ms, rs, True)


def _flanked(seed, n, l, err, flank):
    from aim_amd import engine
    ms, rs = engine.launcher_sizes("wfa", l, err)
    req, pat, txt = engine.gen_pairs(seed, 0, n, l, err, rs)
    req, pat, txt = engine.flank_pairs(seed, 0, req, pat, txt, flank)
    return ms, pat.shape[1], req, pat, txt


def _check_ef(req, pat, txt, res, ops, ms, ef, scores_only=False):
    want = dp_scores(req, pat, txt, ends_free=ef)
    want = np.where(want <= ms, want, ms + 1)
    assert (res["score"] == want).all(), np.nonzero(res["score"] != want)[0][:10]
    if scores_only:
        return
    assert (res["status"] == 0).all()
    for i in range(len(req)):
        r = res[i]
        if r["score"] > ms:
            assert r["begin_offset"] == r["end_offset"], i
            continue
        p = bytes(pat[i, :req["pattern_len"][i]])
        t = bytes(txt[i, :req["text_len"][i]])
        s = _ops_str(ops[i], r)
        assert r["max_operations"] == len(p) + len(t)
        err = check_cigar(s, p, t)
        assert err is None, (i, err, s)
        assert rescore(s, len(p), len(t), ends_free=ef) == r["score"], (i, s)


@pytest.mark.parametrize("l,err,flank", [(100, 0.01, 8), (100, 0.01, 16), (100, 0.05, 50), (150, 0.02, 16), (1000, 0.05, 50),
                                         (1000, 0.01, 8)])
def test_flanked_pairs_match_dp_model(gpu, l, err, flank):
    from aim_amd import engine
    n = 200 if l >= 1000 else 1500
    ms, rs, req, pat, txt = _flanked(13 * flank + l, n, l, err, flank)
    ef = (0, 0, flank, flank)
    res, ops = engine.align(engine.make_params("wfa", ms, rs, backtrace=True, ends_free=ef), req, pat, txt)
    _check_ef(req, pat, txt, res, ops, ms, ef)
    res8, _ = engine.align(engine.make_params("wfa", ms, rs, res8=True, ends_free=ef), req, pat, txt)
    assert np.array_equal(res8["score"], res["score"])


@pytest.mark.parametrize("l,err,flank", [(100, 0.01, 16), (150, 0.02, 16), (1000, 0.05, 50)])
def test_general_kernel_agrees(gpu, monkeypatch, l, err, flank):
    """The same flanked pairs on wfa_wave_kernel (AIM_FORCE_WAVE=1): the DP model's scores, valid CIGARs."""
    from aim_amd import engine
    n = 200 if l >= 1000 else 1000
    ms, rs, req, pat, txt = _flanked(3 * flank + l, n, l, err, flank)
    ef = (0, 0, flank, flank)
    params = engine.make_params("wfa", ms, rs, backtrace=True, ends_free=ef)
    with engine.DeviceSet(1) as s:
        s.configure(params, n)
        assert s.plan_describe(0).startswith("wfa_group_kernel")
    monkeypatch.setenv("AIM_FORCE_WAVE", "1")
    with engine.DeviceSet(1) as s:
        res, ops = s.align(params, req, pat, txt)
        assert s.plan_describe(0).startswith("wfa_wave_kernel")
    _check_ef(req, pat, txt, res, ops, ms, ef)


@pytest.mark.parametrize("ef", [(4, 4, 16, 16), (16, 0, 0, 16), (0, 16, 16, 0), (10 ** 6, 10 ** 6, 10 ** 6, 10 ** 6)])
def test_pattern_side_and_oversized_free_lengths(gpu, ef):
    from aim_amd import engine
    ms, rs, req, pat, txt = _flanked(5, 1000, 100, 0.02, 16)
    res, ops = engine.align(engine.make_params("wfa", ms, rs, backtrace=True, ends_free=ef), req, pat, txt)
    _check_ef(req, pat, txt, res, ops, ms, ef)


def test_pairs_with_n_bases(gpu):
    from aim_amd import engine
    ms, rs, req, pat, txt = _flanked(9, 1000, 100, 0.02, 16)
    rng = np.random.default_rng(9)
    for i in range(0, 1000, 7):
        pat[i, rng.integers(0, req["pattern_len"][i])] = ord("N")
        txt[i, rng.integers(0, req["text_len"][i])] = ord("N")
    ef = (0, 0, 16, 16)
    res, ops = engine.align(engine.make_params("wfa", ms, rs, backtrace=True, ends_free=ef), req, pat, txt)
    _check_ef(req, pat, txt, res, ops, ms, ef)


def test_packed_input_and_compact_runs(gpu):
    from aim_amd import engine
    ms, rs, req, pat, txt = _flanked(21, 2048, 100, 0.01, 16)
    for i in range(0, 2048, 50):
        txt[i, 3] = ord("N")
    ef = (0, 0, 16, 16)
    params = engine.make_params("wfa", ms, rs, backtrace=True, req8=True, ends_free=ef)
    ref, rops = engine.align(engine.make_params("wfa", ms, rs, backtrace=True, ends_free=ef), req, pat, txt)
    _check_ef(req, pat, txt, ref, rops, ms, ef)
    want = engine.format_output(ref, rops, True, ends_free=True)
    cap = 16 * 2048
    with engine.DeviceSet(1) as s:
        s.configure_slots(params, 2048, slots=2, max_raw=2048, max_runs=cap)
        assert "endsfree=0,0,16,16" in s.plan_describe(0)
        s.submit(0, 0, req, packed=engine.pack_batch(req, pat, txt), cigar_runs_cap=cap)
        s.submit(0, 1, req, pat, txt, cigar_runs_cap=cap, want_ops=True)
        a = s.wait(0, 0)
        b = s.wait(0, 1)
    for out in (a, b):
        assert np.array_equal(out["cig"]["score"], ref["score"])
        over = out["cig"]["score"] > ms
        assert (out["cig"]["n_runs"][over] == 0).all()
        lines = []
        for i in range(2048):
            lines.append(b"%d, %d, \n" % (out["cig"]["idx"][i], out["cig"]["score"][i]))
            nr, off = int(out["cig"]["n_runs"][i]), int(out["cig"]["run_offset"][i])
            if nr == 0:
                lines.append(b"\n")
            else:
                lines.append(engine.format_output_runs(out["cig"][i:i + 1], out["runs"]).split(b"\n", 1)[1])
        assert b"".join(lines) == want
    assert np.array_equal(b["res"]["score"], ref["score"])


def test_exact_embedding_scores_zero(gpu):
    from aim_amd import engine
    from aim_amd.capi import REQUEST_DTYPE
    rng = np.random.default_rng(1)
    n, plen, tb, te = 512, 100, 20, 30
    rs = engine.round_up_8(plen + tb + te)
    req = np.zeros(n, dtype=REQUEST_DTYPE)
    pat = np.zeros((n, rs), dtype=np.uint8)
    txt = np.zeros((n, rs), dtype=np.uint8)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    lr = []
    for i in range(n):
        L, R = int(rng.integers(0, tb + 1)), int(rng.integers(0, te + 1))
        p = acgt[rng.integers(0, 4, plen)]
        pat[i, :plen] = p
        txt[i, :L] = acgt[rng.integers(0, 4, L)]
        txt[i, L:L + plen] = p
        txt[i, L + plen:L + plen + R] = acgt[rng.integers(0, 4, R)]
        req[i] = (plen, L + plen + R, 0, i)
        lr.append((L, R))
    res, ops = engine.align(engine.make_params("wfa", 4, rs, backtrace=True, ends_free=(0, 0, tb, te)), req, pat, txt)
    assert (res["score"] == 0).all()
    for i, (L, R) in enumerate(lr):
        s = _ops_str(ops[i], res[i])
        # the leftmost embedding is found first when the flank repeats the pattern's start: any zero-cost placement is exact
        assert check_cigar(s, bytes(pat[i, :plen]), bytes(txt[i, :L + plen + R])) is None
        lead, trail = len(s) - len(s.lstrip("I")), len(s) - len(s.rstrip("I"))
        assert s == "I" * lead + "M" * plen + "I" * trail, (i, s)
        if bytes(txt[i, :L + plen + R]).count(bytes(pat[i, :plen])) == 1:
            assert s == "I" * L + "M" * plen + "I" * R, (i, L, R)


def test_over_cap_pairs_report_cap_plus_one_and_empty_cigar(gpu):
    from aim_amd import engine
    _, rs, req, pat, txt = _flanked(3, 1000, 100, 0.05, 16)
    ms = 3
    ef = (0, 0, 16, 16)
    res, ops = engine.align(engine.make_params("wfa", ms, rs, backtrace=True, ends_free=ef), req, pat, txt)
    over = res["score"] > ms
    assert over.sum() > 100
    assert (res["score"][over] == ms + 1).all() and (res["status"] == 0).all()
    assert (res["begin_offset"][over] == res["end_offset"][over]).all()
    _check_ef(req, pat, txt, res, ops, ms, ef)


def test_debug_poison_changes_nothing(gpu, monkeypatch):
    from aim_amd import engine
    ms, rs, req, pat, txt = _flanked(17, 1000, 100, 0.02, 16)
    params = engine.make_params("wfa", ms, rs, backtrace=True, ends_free=(2, 2, 16, 16))
    res0, ops0 = engine.align(params, req, pat, txt)
    for k, v in (("AIM_DEBUG_POISON_SCRATCH", "165"), ("AIM_DEBUG_POISON_LDS", "90"), ("AIM_DEBUG_POISON_OPS", "7")):
        monkeypatch.setenv(k, v)
    res1, ops1 = engine.align(params, req, pat, txt)
    assert np.array_equal(res0, res1)
    assert engine.format_output(res0, ops0, True, ends_free=True) == engine.format_output(res1, ops1, True, ends_free=True)


@pytest.mark.parametrize("bt", [True, False])
def test_host_cli_ends_free(gpu, tmp_path, bt):
    from aim_amd import build, engine, gen_dataset
    n, l, e, flank = 3000, 100, 0.02, 16
    txt_in = tmp_path / "in.txt"
    pk_in = tmp_path / "in.pk"
    assert gen_dataset.main(["-n", str(n), "-l", str(l), "-e", str(e), "-o", str(txt_in), "--flank", str(flank), "-s", "8"]) == 0
    assert gen_dataset.main(["-n", str(n), "-l", str(l), "-e", str(e), "-o", str(pk_in), "--flank", str(flank), "-s", "8", "--packed"]) == 0
    ms, rs0 = engine.launcher_sizes("wfa", l, e)
    rs = engine.round_up_8(rs0 + 2 * flank)
    ms = 4   # some pairs over the cap: their empty CIGAR lines too
    ef = (0, 0, flank, flank)
    req, pat, txt = engine.parse_pairs(txt_in.read_bytes(), rs)
    res, ops = engine.align(engine.make_params("wfa", ms, rs, backtrace=bt, ends_free=ef), req, pat, txt)
    want = engine.format_output(res, ops, bt, ends_free=True)
    outs = []
    for src, extra in ((txt_in, []), (pk_in, ["--packed-input"]), (txt_in, ["--full-ops"] if bt else ["--no-pack"])):
        out = tmp_path / ("out%d" % len(outs))
        cmd = [build.HOST_BIN, str(src), str(out), str(n), "--algo", "wfa", "--max-score", str(ms), "--read-size", str(rs),
               "--ends-free", "0,0,%d,%d" % (flank, flank), "--threads", "4"] + (["--backtrace"] if bt else []) + extra
        p = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append(out.read_bytes())
    assert outs[0] == want
    assert outs[1] == outs[0]
    assert outs[2] == outs[0]
