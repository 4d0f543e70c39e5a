"""32-bit WFA offsets on the GPU (AIM_FLAG_WFA_W32). Below READ_SIZE 32 760 the W32 kernels give byte-identical results to the int16
batch (itself oracle-checked elsewhere) in every mode; beyond it the exact modes equal the banded DP model of tests/w32_model.py,
REDUCE stays at or above it, edit distance stays at or below GenASM's, every CIGAR uses up both sequences and re-scores to the
reported score, and the paths (over-cap pairs, N bases, packed input, compact runs, RES8, aim_align_device, a small history arena,
debug poison, the host CLI) agree."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import affine2p_model
import endsfree_model
import linear_model
import w32_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# mode name -> (make_params keywords, model keywords, penalties (x, o, e))
MODES = {
    "global": (dict(), dict(), (3, 4, 1)),
    "reduce": (dict(reduce=True), None, (3, 4, 1)),
    "ef": (dict(ends_free=(0, 0, 24, 24)), dict(ends_free=(0, 0, 24, 24)), (3, 4, 1)),
    "a2p": (dict(gap2=(24, 1), mismatch=4, gap_o=4, gap_e=2), dict(gap2=(24, 1)), (4, 4, 2)),
    "lin": (dict(linear=True, mismatch=1, gap_e=1), dict(linear=True), (1, 0, 1)),
}


@pytest.fixture(scope="module")
def gpu(built):
    from aim_amd import capi
    lib = capi.load()
    n = C.c_int()
    assert lib.aim_device_count(C.byref(n)) == 0 and n.value >= 1, lib.aim_last_error()
    return lib


def _plan(params, n):
    from aim_amd import engine
    with engine.DeviceSet(1) as s:
        s.configure(params, n)
        return s.plan_describe(0)


def _pairs(seed, n, l, err, mode="global", long_indel=0):
    from aim_amd import engine
    ms, rs = engine.launcher_sizes("wfa", l, err)
    req, pat, txt = engine.gen_pairs(seed, 0, n, l, err, rs)
    if long_indel:
        req, pat, txt = engine.long_indel_pairs(seed, 0, req, pat, txt, long_indel)
    if mode == "ef":
        req, pat, txt = engine.flank_pairs(seed, 0, req, pat, txt, 24)
    return req, pat, txt, ms, pat.shape[1]


def _params(mode, ms, rs, **kw):
    from aim_amd import engine
    return engine.make_params("wfa", ms, rs, **MODES[mode][0], **kw)


def _same(a, b):
    (res0, ops0), (res1, ops1) = a, b
    assert np.array_equal(res0, res1)
    if ops0 is not None:
        for i in range(len(res0)):
            lo, hi = int(res0["begin_offset"][i]), int(res0["end_offset"][i])
            assert bytes(ops0[i, lo:hi]) == bytes(ops1[i, lo:hi]), i


def _rescore(mode, s, plen, tlen):
    x, o, e = MODES[mode][2]
    if mode == "a2p":
        return affine2p_model.rescore(s, x, o, e, 24, 1)
    if mode == "lin":
        return linear_model.rescore(s, x, e)
    if mode == "ef":
        return endsfree_model.rescore(s, plen, tlen, x, o, e, (0, 0, 24, 24))
    return affine2p_model.rescore(s, x, o, e, o, e)


def _check_cigars(mode, req, pat, txt, res, ops, ms):
    assert (res["status"] == 0).all(), res["status"]
    for i in range(len(req)):
        r = res[i]
        plen, tlen = int(req["pattern_len"][i]), int(req["text_len"][i])
        assert r["max_operations"] == plen + tlen and r["end_offset"] == plen + tlen
        if r["score"] > ms:
            continue
        s = bytes(ops[i, int(r["begin_offset"]):int(r["end_offset"])]).decode()
        err = affine2p_model.check_cigar(s, bytes(pat[i, :plen]), bytes(txt[i, :tlen]))
        assert err is None, (i, err)
        assert _rescore(mode, s, plen, tlen) == r["score"], i


def _model(mode, req, pat, txt, ms):
    x, o, e = MODES[mode][2]
    return w32_model.dp_scores(req, pat, txt, ms, x, o, e, **(MODES[mode][1] or {}))


# ---- 1. W32 against int16, below the cap: byte-identical ---------------------------------------------------------------------

@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("l,err,n", [(100, 0.05, 2000), (1000, 0.05, 200), (10000, 0.01, 16), (16000, 0.01, 8)])
def test_w32_equals_int16(gpu, mode, l, err, n):
    from aim_amd import engine
    req, pat, txt, ms, rs = _pairs(700 + l, n, l, err, mode)
    for bt in (False, True):
        a = engine.align(_params(mode, ms, rs, backtrace=bt), req, pat, txt)
        p32 = _params(mode, ms, rs, backtrace=bt, w32=True)
        line = _plan(p32, n)
        assert line.startswith("wfa_wave_kernel ") and line.endswith(" w32"), line
        b = engine.align(p32, req, pat, txt)
        _same(a, b)


# ---- 2. beyond the old cap, exact modes: the banded model ----------------------------------------------------------------------

LONG = [("global", 33000, 0.01, dict(), 3), ("global", 40000, 0.005, dict(mismatch=4, gap_o=6, gap_e=2), 3),
        ("a2p", 34000, 0.005, dict(), 3), ("lin", 36000, 0.01, dict(), 4), ("ef", 33000, 0.005, dict(), 3)]


@pytest.mark.parametrize("case", range(len(LONG)))
def test_long_reads_equal_model(gpu, case):
    from aim_amd import engine
    mode, l, err, pen, n = LONG[case]
    req, pat, txt, ms, rs = _pairs(40 + case, n, l, err, mode, long_indel=400 if mode == "a2p" else 0)
    assert rs >= 32760 and (req["text_len"] > 32767).all()
    saved = MODES[mode]
    if pen:   # global (4, 6, 2)
        MODES[mode] = (dict(pen), saved[1], (pen["mismatch"], pen["gap_o"], pen["gap_e"]))
        ms, _ = engine.launcher_sizes("wfa", l, err, mismatch=4, gap_o=6, gap_e=2)
    try:
        if mode == "lin":
            ms = linear_model.max_score_rule(l, err, 1, 1)
        if mode == "a2p":   # piece-1 costs of the edits, plus the long indel on piece 2
            ms = engine.launcher_sizes("wfa", l, err, mismatch=4, gap_o=4, gap_e=2)[0] + 24 + 400
        want = _model(mode, req, pat, txt, ms)
        want = np.where(want <= ms, want, ms + 1)
        res, ops = engine.align(_params(mode, ms, rs, backtrace=True, w32=True), req, pat, txt)
        assert np.array_equal(res["score"], want), (res["score"], want)
        assert (res["score"] <= ms).all()
        _check_cigars(mode, req, pat, txt, res, ops, ms)
        res_s, _ = engine.align(_params(mode, ms, rs, w32=True), req, pat, txt)
        assert np.array_equal(res_s["score"], res["score"])
    finally:
        MODES[mode] = saved


# ---- 3. REDUCE beyond the cap --------------------------------------------------------------------------------------------------

def test_reduce_long_reads(gpu):
    from aim_amd import engine
    req, pat, txt, ms, rs = _pairs(91, 4, 35000, 0.01)
    exact = _model("global", req, pat, txt, ms)
    res, ops = engine.align(_params("reduce", ms, rs, backtrace=True, w32=True), req, pat, txt)
    assert (res["score"] >= np.minimum(exact, ms + 1)).all(), (res["score"], exact)
    _check_cigars("reduce", req, pat, txt, res, ops, ms)
    res_s, _ = engine.align(_params("reduce", ms, rs, w32=True), req, pat, txt)
    assert np.array_equal(res_s["score"], res["score"])


# ---- 4. edit distance against GenASM at l = 100 000 ----------------------------------------------------------------------------

def test_edit_distance_bounded_by_genasm(gpu):
    from aim_amd import engine
    l, err, n = 100000, 0.01, 8
    _, rs = engine.launcher_sizes("genasm", l, err)
    req, pat, txt = engine.gen_pairs(5, 0, n, l, err, rs)
    ga, _ = engine.align(engine.make_params("genasm", 0, rs), req, pat, txt)
    ms = linear_model.max_score_rule(l, err, 1, 1)
    res, _ = engine.align(_params("lin", ms, rs, w32=True), req, pat, txt)
    assert (res["score"] <= ms).all(), res["score"]
    assert (res["score"] <= ga["score"]).all(), (res["score"], ga["score"])


# ---- 5. paths ------------------------------------------------------------------------------------------------------------------

def test_over_cap_pairs_keep_global_result(gpu):
    from aim_amd import engine
    req, pat, txt, ms, rs = _pairs(13, 6, 33000, 0.005)
    exact = _model("global", req, pat, txt, ms)
    cap = int(np.median(exact))
    res, ops = engine.align(_params("global", cap, rs, backtrace=True, w32=True), req, pat, txt)
    over = res["score"] > cap
    assert over.any() and (~over).any()
    assert (res["score"][over] == cap + 1).all() and (res["begin_offset"][over] == res["end_offset"][over] - 1).all()
    assert np.array_equal(res["score"][~over], exact[~over])
    _check_cigars("global", req, pat, txt, res, ops, cap)


def test_pairs_with_n_bases(gpu):
    from aim_amd import engine
    req, pat, txt, ms, rs = _pairs(17, 4, 33000, 0.005)
    txt[:, 7] = ord("N")
    pat[1, 30000] = ord("N")
    want = _model("global", req, pat, txt, ms)
    res, ops = engine.align(_params("global", ms, rs, backtrace=True, w32=True), req, pat, txt)
    assert np.array_equal(res["score"], want)
    _check_cigars("global", req, pat, txt, res, ops, ms)


@pytest.mark.parametrize("mode", ["global", "ef"])
def test_packed_input_and_compact_runs(gpu, mode):
    from aim_amd import engine
    n = 6
    req, pat, txt, ms, rs = _pairs(21, n, 33000, 0.005, mode)
    txt[2, 11] = ord("N")   # one pair on the raw side list
    ref, rops = engine.align(_params(mode, ms, rs, backtrace=True, w32=True), req, pat, txt)
    want = engine.format_output(ref, rops, True)
    cap = rs // 4 * n
    with engine.DeviceSet(1) as s:
        s.configure_slots(_params(mode, ms, rs, backtrace=True, w32=True), n, slots=2, max_raw=n, max_runs=cap)
        assert s.plan_describe(0).endswith(" w32")
        s.submit(0, 0, req, packed=engine.pack_batch(req, pat, txt), cigar_runs_cap=cap)
        s.submit(0, 1, req, pat, txt, cigar_runs_cap=cap, want_ops=True)
        a = s.wait(0, 0)
        b = s.wait(0, 1)
    for out in (a, b):
        assert np.array_equal(out["cig"]["score"], ref["score"])
        assert engine.format_output_runs(out["cig"], out["runs"]) == want
    # score-only, {idx, score} results, packed rows in
    with engine.DeviceSet(1) as s:
        s.configure_slots(_params(mode, ms, rs, res8=True, w32=True), n, slots=1, max_raw=n, max_runs=0)
        s.submit(0, 0, req, packed=engine.pack_batch(req, pat, txt))
        c = s.wait(0, 0)
    assert np.array_equal(c["res"]["score"], ref["score"])


def test_res8_below_and_beyond_the_old_cap(gpu):
    from aim_amd import engine
    for l, n in ((1000, 300), (33000, 3)):
        req, pat, txt, ms, rs = _pairs(29, n, l, 0.01)
        a, _ = engine.align(_params("global", ms, rs, w32=True), req, pat, txt)
        b, _ = engine.align(_params("global", ms, rs, w32=True, res8=True), req, pat, txt)
        assert np.array_equal(a["score"], b["score"]) and np.array_equal(a["idx"], b["idx"])


def test_small_history_arena_nomem_for_one_pair(gpu, monkeypatch):
    """A BACKTRACE arena shrunk by the scratch bound: the pair whose history outgrows it reports AIM_PAIR_NOMEM, the others align."""
    from aim_amd import capi, engine
    l = 33000
    _, rs = engine.launcher_sizes("wfa", l, 0.03)
    req, pat, txt = engine.gen_pairs(3, 0, 8, l, 0.002, rs)
    hreq, hpat, htxt = engine.gen_pairs(4, 0, 1, l, 0.03, rs)
    req[5], pat[5], txt[5] = hreq[0], hpat[0], htxt[0]
    req["idx"] = np.arange(len(req))
    ms = 5000
    monkeypatch.setenv("AIM_SCRATCH_GB", "0.25")
    line = _plan(_params("global", ms, rs, backtrace=True, w32=True), len(req))
    assert line.startswith("wfa_wave_kernel") and line.endswith(" w32"), line
    res, ops = engine.align(_params("global", ms, rs, backtrace=True, w32=True), req, pat, txt, check=False)
    assert res["status"][5] == capi.PAIR_NOMEM, res["status"]
    ok = np.arange(len(req)) != 5
    assert (res["status"][ok] == 0).all(), res["status"]
    want = _model("global", req[ok], pat[ok], txt[ok], 600)   # (a narrower band than ms = 5000: exact up to 600)
    assert (want <= 600).all() and np.array_equal(res["score"][ok], want)


def test_debug_poison_changes_nothing(gpu, monkeypatch):
    from aim_amd import engine
    req, pat, txt, ms, rs = _pairs(19, 3, 33000, 0.005)
    params = _params("global", ms, rs, backtrace=True, w32=True)
    a = engine.align(params, req, pat, txt)
    for k, v in (("AIM_DEBUG_POISON_SCRATCH", "165"), ("AIM_DEBUG_POISON_LDS", "90"), ("AIM_DEBUG_POISON_OPS", "7")):
        monkeypatch.setenv(k, v)
    b = engine.align(params, req, pat, txt)
    _same(a, b)


ALIGN_DEVICE = '''
import sys
import torch
torch.cuda.init()   # (before the library: the device buffers are torch's)
sys.path.insert(0, "tests")
import test_w32_gpu as t
t.align_device_matches_set_api()
print("ALIGN_DEVICE_OK")
'''


def test_align_device(gpu):
    """aim_align_device on torch-allocated device buffers (in a child process that brings up torch before the library)."""
    p = subprocess.run([sys.executable, "-c", ALIGN_DEVICE], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ALIGN_DEVICE_OK" in p.stdout, p.stdout + p.stderr


def align_device_matches_set_api():
    import torch
    from aim_amd import capi, engine
    lib = capi.load()
    req, pat, txt, ms, rs = _pairs(41, 4, 33000, 0.005)
    n = len(req)
    params = _params("global", ms, rs, backtrace=True, w32=True)
    dev = torch.device("cuda:0")
    d_req = torch.from_numpy(req.view(np.uint8).copy()).to(dev)
    d_pat = torch.from_numpy(np.ascontiguousarray(pat)).to(dev)
    d_txt = torch.from_numpy(np.ascontiguousarray(txt)).to(dev)
    d_res = torch.zeros(n * capi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_ops = torch.zeros(n * 2 * rs, dtype=torch.uint8, device=dev)
    sb = lib.aim_scratch_bytes(capi.params_ref(params), n)
    assert sb > 0
    d_scr = torch.zeros(sb, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rc = lib.aim_align_device(capi.params_ref(params), n, d_req.data_ptr(), d_pat.data_ptr(), d_txt.data_ptr(), d_res.data_ptr(),
                              d_ops.data_ptr(), d_scr.data_ptr(), sb, None)
    assert rc == 0, lib.aim_last_error()
    torch.cuda.synchronize()
    res = d_res.cpu().numpy().view(capi.RESULT_DTYPE)
    ops = d_ops.cpu().numpy().reshape(n, 2 * rs)
    ref, rops = engine.align(params, req, pat, txt)
    assert np.array_equal(res, ref)
    assert engine.format_output(res, ops, True) == engine.format_output(ref, rops, True)


# ---- 6. host CLI ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bt", [False, True])
def test_host_cli_w32(gpu, tmp_path, bt):
    from aim_amd import build, engine, gen_dataset
    n, l, e = 4, 50000, 0.005
    txt_in, pk_in = tmp_path / "in.txt", tmp_path / "in.pk"
    assert gen_dataset.main(["-n", str(n), "-l", str(l), "-e", str(e), "-o", str(txt_in), "-s", "8"]) == 0
    assert gen_dataset.main(["-n", str(n), "-l", str(l), "-e", str(e), "-o", str(pk_in), "-s", "8", "--packed"]) == 0
    ms, rs = engine.launcher_sizes("wfa", l, e)
    req, pat, txt = engine.parse_pairs(txt_in.read_bytes(), rs)
    res, ops = engine.align(_params("global", ms, rs, backtrace=bt, w32=True), req, pat, txt)
    want = engine.format_output(res, ops, bt)
    outs = []
    for src, extra in ((txt_in, []), (pk_in, ["--packed-input"])):
        out = tmp_path / ("out%d" % len(outs))
        cmd = [build.HOST_BIN, str(src), str(out), str(n), "--algo", "wfa", "--max-score", str(ms), "--read-size", str(rs),
               "--mismatch", "3", "--gap-o", "4", "--gap-e", "1", "--nr-dpus", "1", "--w32", "--threads", "4"] + (["--backtrace"] if bt else []) + extra
        p = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=180)
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append(out.read_bytes())
    assert outs[0] == want
    assert outs[1] == outs[0]
