"""Bidirectional WFA on the GPU (AIM_FLAG_WFA_BIDIR). Scores and statuses equal the flag-less batch; every CIGAR uses up both
sequences, puts 'M' on equal and 'X' on unequal bytes and re-scores to the reported score; pairs of score <= T keep the flag-less
bytes; results do not depend on the offset width, the grid or debug poison; the entry points agree; and a batch whose flag-less
CIGAR reports AIM_PAIR_NOMEM under a small scratch bound aligns every pair with the flag."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import affine2p_model
import reference_rows as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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


def _T(line):
    return int(line.split(" bidir=")[1].split()[0])


def _pairs(seed, n, l, err, long_indel=0):
    from aim_amd import engine
    ms, rs = engine.launcher_sizes("wfa", l, err)
    req, pat, txt = engine.gen_pairs(seed, 0, n, l, err, rs)
    if long_indel:
        req, pat, txt = engine.long_indel_pairs(seed, 0, req, pat, txt, long_indel)
    return req, pat, txt, ms, pat.shape[1]


def _params(ms, rs, x=3, o=4, e=1, **kw):
    from aim_amd import engine
    return engine.make_params("wfa", ms, rs, mismatch=x, gap_o=o, gap_e=e, backtrace=True, **kw)


def _check_cigars(req, pat, txt, res, ops, ms, x=3, o=4, e=1):
    for i in range(len(req)):
        r = res[i]
        plen, tlen = int(req["pattern_len"][i]), int(req["text_len"][i])
        assert r["max_operations"] == plen + tlen and r["end_offset"] == plen + tlen
        if r["score"] > ms:
            assert r["begin_offset"] == r["end_offset"] - 1, i
            continue
        s = bytes(ops[i, int(r["begin_offset"]):int(r["end_offset"])]).decode()
        err = affine2p_model.check_cigar(s, bytes(pat[i, :plen]), bytes(txt[i, :tlen]))
        assert err is None, (i, err)
        assert affine2p_model.rescore(s, x, o, e, o, e) == r["score"], i


def _compare(ref, got, T):
    """Same results but for the CIGAR of pairs over T; the same bytes for the pairs of score <= T."""
    (r0, o0), (r1, o1) = ref, got
    for f in ("score", "status", "idx", "max_operations", "end_offset"):
        assert np.array_equal(r0[f], r1[f]), f
    low = r0["score"] <= T
    assert np.array_equal(r0["begin_offset"][low], r1["begin_offset"][low])
    for i in np.nonzero(low)[0]:
        lo, hi = int(r0["begin_offset"][i]), int(r0["end_offset"][i])
        assert bytes(o0[i, lo:hi]) == bytes(o1[i, lo:hi]), i


def _same(a, b):
    (r0, o0), (r1, o1) = a, b
    assert np.array_equal(r0, r1)
    for i in range(len(r0)):
        lo, hi = int(r0["begin_offset"][i]), int(r0["end_offset"][i])
        assert bytes(o0[i, lo:hi]) == bytes(o1[i, lo:hi]), i


# ---- 1. against the flag-less batch ----------------------------------------------------------------------------------------------

# (l, err, n, long indel, MAX_SCORE override): the launchers' MAX_SCORE, and raised caps so that pairs go past T at short lengths
CASES = [(100, 0.01, 4000, 0, None), (100, 0.05, 4000, 0, None), (100, 0.10, 2000, 0, None), (1000, 0.05, 400, 0, None),
         (1000, 0.05, 200, 400, 2000), (1000, 0.15, 200, 0, 900), (10000, 0.01, 16, 0, None), (10000, 0.05, 8, 0, None)]


@pytest.mark.parametrize("case", range(len(CASES)))
def test_equals_flagless(gpu, case):
    from aim_amd import engine
    l, err, n, li, ms_over = CASES[case]
    req, pat, txt, ms, rs = _pairs(500 + case, n, l, err, li)
    ms = ms_over or ms
    line = _plan(_params(ms, rs, bidir=True), n)
    assert line.startswith("wfa_bidir_kernel ") and " bidir=" in line, line
    T = _T(line)
    assert T >= 250
    ref = engine.align(_params(ms, rs), req, pat, txt, check=False)
    got = engine.align(_params(ms, rs, bidir=True), req, pat, txt, check=False)
    _compare(ref, got, T)
    assert (got[0]["status"] == 0).all()
    _check_cigars(req, pat, txt, got[0], got[1], ms)
    if ms_over:
        assert (ref[0]["score"] > T).any()


def _global_bt_rows():
    out = []
    for c in rr.all_reference_rows():
        if c["algo"] == "wfa" and c["backtrace"] and not c.get("reduce", False) and not c.get("ends_free") and not c.get("gap2"):
            out.append(c)
    return out


# Every reference row of global WFA with CIGAR (no REDUCE) has MAX_SCORE <= 250 = T: these rows check the first stage (wfa_wave_kernel
# at MAX_SCORE min(MAX_SCORE, T)) and the plan, not wfa_bidir_kernel itself; the rows of MAX_SCORE 500 all use REDUCE, which the flag
# rejects. The bidirectional kernel is covered by the synthetic cases above and below.
@pytest.mark.parametrize("case", _global_bt_rows(), ids=rr.row_id)
def test_reference_rows(gpu, case):
    from aim_amd import engine
    _, req, pat, txt = rr.row_input(case)
    p = rr.row_params(case)
    pb = rr.row_params(case)
    pb.flags |= 0x200
    ref = engine.align(p, req, pat, txt, check=False)
    got = engine.align(pb, req, pat, txt, check=False)
    _compare(ref, got, _T(_plan(pb, len(req))))
    x, o, e = pb.mismatch, pb.gap_o, pb.gap_e
    ok = got[0]["status"] == 0
    _check_cigars(req[ok], pat[ok], txt[ok], got[0][ok], got[1][ok], case["max_score"], x, o, e)


# ---- 2. long reads, W32 --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("l,n", [(40000, 4), (100000, 2)])
def test_long_reads_w32(gpu, l, n):
    from aim_amd import engine
    req, pat, txt, ms, rs = _pairs(70 + n, n, l, 0.01)
    score_only, _ = engine.align(engine.make_params("wfa", ms, rs, w32=True), req, pat, txt)
    res, ops = engine.align(_params(ms, rs, w32=True, bidir=True), req, pat, txt)
    assert np.array_equal(res["score"], score_only["score"]) and (res["status"] == 0).all()
    assert (res["score"] > 250).all()
    _check_cigars(req, pat, txt, res, ops, ms)


# ---- 3. determinism --------------------------------------------------------------------------------------------------------------

def test_int16_w32_req8_grids_poison_identical(gpu, monkeypatch):
    """The same bytes with int32 offsets, with 8-byte requests, on a grid of 16 workgroups (each workgroup aligns four pairs in
    turn: the per-pair state of its persistent loop is reset) and of 64, and under debug poison."""
    from aim_amd import engine
    req, pat, txt, ms, rs = _pairs(33, 64, 10000, 0.05)
    monkeypatch.setenv("AIM_CHIP_CUS", "256")
    params = _params(ms, rs, bidir=True)
    wide = _plan(params, len(req))
    a = engine.align(params, req, pat, txt)
    assert (a[0]["score"] > _T(wide)).sum() >= 48, a[0]["score"]
    _same(a, engine.align(_params(ms, rs, bidir=True, w32=True), req, pat, txt))
    _same(a, engine.align(_params(ms, rs, bidir=True, req8=True), req, pat, txt))
    monkeypatch.setenv("AIM_CHIP_CUS", "1")
    narrow = _plan(params, len(req))
    assert " grid=64 " in wide and " grid=16 " in narrow, (wide, narrow)
    _same(a, engine.align(params, req, pat, txt))
    monkeypatch.setenv("AIM_CHIP_CUS", "256")
    for k, v in (("AIM_DEBUG_POISON_SCRATCH", "165"), ("AIM_DEBUG_POISON_LDS", "90"), ("AIM_DEBUG_POISON_OPS", "7")):
        monkeypatch.setenv(k, v)
    _same(a, engine.align(params, req, pat, txt))


# ---- 4. edge pairs -------------------------------------------------------------------------------------------------------------

def test_over_cap_n_bases_and_empty(gpu):
    from aim_amd import engine
    req, pat, txt, ms, rs = _pairs(9, 12, 3000, 0.05)
    txt[1, 5:40] = ord("N")
    pat[2, 100:900] = ord("N")
    req["text_len"][3] = 0
    req["pattern_len"][4] = 0
    req["pattern_len"][5] = 0
    req["text_len"][5] = 0
    full, _ = engine.align(engine.make_params("wfa", 20000, rs), req, pat, txt)
    cap = int(np.median(full["score"]))
    assert cap > 250
    for c in (cap, 20000):
        ref = engine.align(_params(c, rs), req, pat, txt, check=False)
        got = engine.align(_params(c, rs, bidir=True), req, pat, txt, check=False)
        _compare(ref, got, 250)
        _check_cigars(req, pat, txt, got[0], got[1], c)
    assert (got[0]["score"] > 250).sum() >= 3


# ---- 5. entry points -------------------------------------------------------------------------------------------------------------

def test_packed_input_and_compact_runs(gpu):
    from aim_amd import engine
    n = 8
    req, pat, txt, ms, rs = _pairs(21, n, 5000, 0.05)
    txt[2, 11] = ord("N")
    params = _params(ms, rs, bidir=True)
    ref, rops = engine.align(params, req, pat, txt)
    assert (ref["score"] > 250).any()
    want = engine.format_output(ref, rops, True)
    cap = rs // 2 * n
    with engine.DeviceSet(1) as s:
        s.configure_slots(params, n, slots=2, max_raw=n, max_runs=cap)
        assert s.plan_describe(0).startswith("wfa_bidir_kernel")
        s.submit(0, 0, req, packed=engine.pack_batch(req, pat, txt), cigar_runs_cap=cap)
        s.submit(0, 1, req, pat, txt, cigar_runs_cap=cap, want_ops=True)
        a = s.wait(0, 0)
        b = s.wait(0, 1)
    for out in (a, b):
        assert np.array_equal(out["cig"]["score"], ref["score"])
        assert engine.format_output_runs(out["cig"], out["runs"]) == want


ALIGN_DEVICE = '''
import sys
import torch
torch.cuda.init()   # (before the library: the device buffers are torch's)
sys.path.insert(0, "tests")
import test_bidir_gpu as t
t.align_device_matches_set_api()
print("ALIGN_DEVICE_OK")
'''


def test_align_device(gpu):
    p = subprocess.run([sys.executable, "-c", ALIGN_DEVICE], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ALIGN_DEVICE_OK" in p.stdout, p.stdout + p.stderr


def align_device_matches_set_api():
    import torch
    from aim_amd import capi, engine
    lib = capi.load()
    req, pat, txt, ms, rs = _pairs(41, 6, 5000, 0.05)
    n = len(req)
    params = _params(ms, rs, bidir=True)
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


def test_host_cli_bidir(gpu, tmp_path):
    from aim_amd import build, engine, gen_dataset
    n, l, e = 6, 5000, 0.05
    txt_in = tmp_path / "in.txt"
    assert gen_dataset.main(["-n", str(n), "-l", str(l), "-e", str(e), "-o", str(txt_in), "-s", "8"]) == 0
    ms, rs = engine.launcher_sizes("wfa", l, e)
    req, pat, txt = engine.parse_pairs(txt_in.read_bytes(), rs)
    res, ops = engine.align(_params(ms, rs, bidir=True), req, pat, txt)
    want = engine.format_output(res, ops, True)
    out = tmp_path / "out"
    cmd = [build.HOST_BIN, str(txt_in), str(out), str(n), "--algo", "wfa", "--max-score", str(ms), "--read-size", str(rs),
           "--mismatch", "3", "--gap-o", "4", "--gap-e", "1", "--nr-dpus", "1", "--backtrace", "--bidir", "--threads", "4"]
    p = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stdout + p.stderr
    assert out.read_bytes() == want


# ---- 6. the capability: no AIM_PAIR_NOMEM because of the score --------------------------------------------------------------------

def test_bidir_aligns_where_history_runs_out(gpu, monkeypatch):
    from aim_amd import capi, engine
    req, pat, txt, ms, rs = _pairs(7, 64, 100000, 0.01)
    monkeypatch.setenv("AIM_SCRATCH_GB", "1")
    res0, _ = engine.align(_params(ms, rs, w32=True), req, pat, txt, check=False)
    assert (res0["status"] == capi.PAIR_NOMEM).any(), res0["status"]
    res, ops = engine.align(_params(ms, rs, w32=True, bidir=True), req, pat, txt, check=False)
    assert (res["status"] == 0).all(), res["status"]
    monkeypatch.delenv("AIM_SCRATCH_GB")
    score_only, _ = engine.align(engine.make_params("wfa", ms, rs, w32=True), req, pat, txt)
    assert np.array_equal(res["score"], score_only["score"])
    _check_cigars(req, pat, txt, res, ops, ms)
