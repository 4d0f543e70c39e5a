"""Gap-linear WFA on the GPU (AIM_FLAG_LINEAR): scores equal the DP model of tests/linear_model.py and the GPU NW path, CIGARs use
up both sequences and re-score to the reported score, and every path (wfa_group, wfa_wave, the to-do list, narrow rows, history
chunks, packed input, compact runs, RES8 / REQ8, aim_align_device, the host CLI) gives the same bytes."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

from linear_model import check_cigar, dp_scores, max_score_rule, rescore

pytestmark = pytest.mark.gpu

# edit distance; a score unit of 2; a ring depth set by g; x > 2g (a mismatch never beats I + D)
PENS = [(1, 1), (4, 2), (2, 3), (5, 2)]


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


def _pairs(seed, n, l, err):
    from aim_amd import engine
    _, rs = engine.launcher_sizes("wfa", l, err)
    req, pat, txt = engine.gen_pairs(seed, 0, n, l, err, rs)
    return req, pat, txt, rs


def _params(ms, rs, pen, **kw):
    from aim_amd import engine
    return engine.make_params("wfa", ms, rs, mismatch=pen[0], gap_e=pen[1], linear=True, **kw)


def _check(req, pat, txt, res, ops, ms, pen, scores_only=False, want=None):
    want = dp_scores(req, pat, txt, *pen) if want is None else want
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
        s = bytes(ops[i, int(r["begin_offset"]):int(r["end_offset"])]).decode()
        err = check_cigar(s, bytes(pat[i, :plen]), bytes(txt[i, :tlen]))
        assert err is None, (i, err, s)
        assert rescore(s, *pen) == r["score"], (i, s)


def _same(a, b):
    (res0, ops0), (res1, ops1) = a, b
    assert np.array_equal(res0, res1)
    if ops0 is not None:
        for i in range(len(res0)):
            lo, hi = int(res0["begin_offset"][i]), int(res0["end_offset"][i])
            assert bytes(ops0[i, lo:hi]) == bytes(ops1[i, lo:hi]), i


@pytest.mark.parametrize("pen", PENS)
@pytest.mark.parametrize("l,err,n", [(100, 0.01, 3000), (100, 0.05, 3000), (1000, 0.05, 400)])
def test_scores_and_cigars_match_model(gpu, pen, l, err, n):
    from aim_amd import engine
    req, pat, txt, rs = _pairs(100 + l + int(1000 * err), n, l, err)
    ms = max_score_rule(l, err, *pen)
    want = dp_scores(req, pat, txt, *pen)
    line = _plan(_params(ms, rs, pen, backtrace=True), n)
    assert line.startswith("wfa_group_kernel") and line.endswith(" linear"), line
    res, ops = engine.align(_params(ms, rs, pen, backtrace=True), req, pat, txt)
    _check(req, pat, txt, res, ops, ms, pen, want=want)
    res_s, _ = engine.align(_params(ms, rs, pen), req, pat, txt)
    assert np.array_equal(res_s["score"], res["score"])
    res8, _ = engine.align(_params(ms, rs, pen, res8=True, req8=True), req, pat, txt)
    assert np.array_equal(res8["score"], res["score"])


@pytest.mark.parametrize("pen", PENS)
def test_long_reads_on_both_kernels(gpu, monkeypatch, pen):
    """l = 10 000 e = 1 %: the plan's kernel and wfa_wave give the model's scores and the same CIGAR bytes."""
    from aim_amd import engine
    req, pat, txt, rs = _pairs(77, 6, 10000, 0.01)
    ms = max_score_rule(10000, 0.01, *pen)
    want = dp_scores(req, pat, txt, *pen)
    out = []
    for force in ("0", "1"):
        monkeypatch.setenv("AIM_FORCE_WAVE", force)
        line = _plan(_params(ms, rs, pen, backtrace=True), len(req))
        assert line.startswith("wfa_wave_kernel" if force == "1" else ("wfa_group_kernel", "wfa_wave_kernel")), line
        res, ops = engine.align(_params(ms, rs, pen, backtrace=True), req, pat, txt)
        _check(req, pat, txt, res, ops, ms, pen, want=want)
        res_s, _ = engine.align(_params(ms, rs, pen), req, pat, txt)
        assert np.array_equal(res_s["score"], res["score"])
        out.append((res, ops))
    _same(out[0], out[1])


@pytest.mark.parametrize("pen", PENS)
@pytest.mark.parametrize("l,err,n", [(100, 0.05, 3000), (1000, 0.05, 400)])
def test_scores_equal_gpu_nw(gpu, pen, l, err, n):
    from aim_amd import engine
    req, pat, txt, rs = _pairs(300 + l, n, l, err)
    keep = req["pattern_len"] <= req["text_len"]
    req, pat, txt = req[keep], pat[keep], txt[keep]
    ms = max_score_rule(l, err, *pen)
    res, _ = engine.align(_params(ms, rs, pen), req, pat, txt)
    nres, _ = engine.align(engine.make_params("nw", 10 ** 4, rs, mismatch=pen[0], gap=pen[1]), req, pat, txt)
    ok = res["score"] <= ms
    assert ok.sum() > 0.5 * len(req)
    assert np.array_equal(res["score"][ok], nres["score"][ok])


@pytest.mark.parametrize("pen", PENS)
@pytest.mark.parametrize("bt", [True, False])
def test_wave_kernel_identical(gpu, monkeypatch, pen, bt):
    from aim_amd import engine
    req, pat, txt, rs = _pairs(5, 1500, 150, 0.03)
    ms = max_score_rule(150, 0.03, *pen)
    params = _params(ms, rs, pen, backtrace=bt)
    assert _plan(params, len(req)).startswith("wfa_group_kernel")
    a = engine.align(params, req, pat, txt)
    _check(req, pat, txt, a[0], a[1], ms, pen, scores_only=not bt)
    monkeypatch.setenv("AIM_FORCE_WAVE", "1")
    assert _plan(params, len(req)).startswith("wfa_wave_kernel")
    _same(a, engine.align(params, req, pat, txt))


@pytest.mark.parametrize("pen", PENS)
@pytest.mark.parametrize("bt", [True, False])
def test_narrow_rows_overflow_to_wave(gpu, monkeypatch, pen, bt):
    """Rows of 32 entries (AIM_GROUP_WLDS): every pair whose wavefront outgrows 30 diagonals leaves for the general kernel."""
    from aim_amd import engine
    req, pat, txt, rs = _pairs(11, 800, 600, 0.05)
    ms = max_score_rule(600, 0.05, *pen)
    params = _params(ms, rs, pen, backtrace=bt)
    a = engine.align(params, req, pat, txt)
    _check(req, pat, txt, a[0], a[1], ms, pen, scores_only=not bt)
    monkeypatch.setenv("AIM_GROUP_WLDS", "32")
    with engine.DeviceSet(1) as s:
        s.configure(params, len(req))
        assert s.plan_describe(0).startswith("wfa_group_kernel")
        b = s.align(params, req, pat, txt)
        assert s.fallback_pairs(0) > 0
    _same(a, b)


@pytest.mark.parametrize("pen", PENS)
def test_pairs_with_n_bases(gpu, monkeypatch, pen):
    from aim_amd import engine
    req, pat, txt, rs = _pairs(9, 1500, 150, 0.02)
    rng = np.random.default_rng(9)
    for i in range(0, len(req), 7):
        pat[i, rng.integers(0, req["pattern_len"][i])] = ord("N")
        txt[i, rng.integers(0, req["text_len"][i])] = ord("N")
    ms = max_score_rule(150, 0.02, *pen) + 4 * pen[0]
    params = _params(ms, rs, pen, backtrace=True)
    assert _plan(params, len(req)).startswith("wfa_group_kernel")
    a = engine.align(params, req, pat, txt)
    _check(req, pat, txt, a[0], a[1], ms, pen)
    monkeypatch.setenv("AIM_FORCE_WAVE", "1")
    _same(a, engine.align(params, req, pat, txt))


def _hist_pair_bytes(ms, unit):
    rows = ms // unit + 2
    pool_off = 16 + rows * 8
    runs_off = (pool_off + rows * rows * 2 + 15) & ~15
    return (runs_off + (2 * ms + 16) * 4 + 255) & ~255


def test_history_in_several_chunks(gpu, monkeypatch):
    from aim_amd import engine
    pen = (4, 2)
    n = 12000
    req, pat, txt, rs = _pairs(31, n, 1000, 0.05)   # (regions of ~23 KB: several chunks fit above the planner's smallest budget)
    ms = max_score_rule(1000, 0.05, *pen)
    params = _params(ms, rs, pen, backtrace=True)
    a = engine.align(params, req, pat, txt)
    _check(req[:300], pat[:300], txt[:300], a[0][:300], a[1][:300], ms, pen)
    fit = 5000                                       # pairs per history buffer: three launches of the compute + traceback pair
    monkeypatch.setenv("AIM_SCRATCH_GB", "%.6f" % (4.0 * fit * _hist_pair_bytes(ms, 2) / (1 << 30) + 0.02))
    line = _plan(params, n)
    assert line.startswith("wfa_group_kernel"), line
    chunk = int(re.search(r" chunk=(\d+)", line).group(1))
    assert 0 < chunk < n // 2, line                  # the batch really runs as several launches
    _same(a, engine.align(params, req, pat, txt))


@pytest.mark.parametrize("pen", [(1, 1), (4, 2)])
def test_packed_input_and_compact_runs(gpu, pen):
    from aim_amd import engine
    n = 2048
    req, pat, txt, rs = _pairs(21, n, 150, 0.02)
    for i in range(0, n, 50):
        txt[i, 3] = ord("N")
    ms = max_score_rule(150, 0.02, *pen)
    ref, rops = engine.align(_params(ms, rs, pen, backtrace=True), req, pat, txt)
    _check(req, pat, txt, ref, rops, ms, pen)
    want = engine.format_output(ref, rops, True)
    params = _params(ms, rs, pen, backtrace=True, req8=True)
    cap = 16 * n
    with engine.DeviceSet(1) as s:
        s.configure_slots(params, n, slots=2, max_raw=n, max_runs=cap)
        assert s.plan_describe(0).endswith(" linear")
        s.submit(0, 0, req, packed=engine.pack_batch(req, pat, txt), cigar_runs_cap=cap)
        s.submit(0, 1, req, pat, txt, cigar_runs_cap=cap, want_ops=True)
        a = s.wait(0, 0)
        b = s.wait(0, 1)
    for out in (a, b):
        assert np.array_equal(out["cig"]["score"], ref["score"])
        assert engine.format_output_runs(out["cig"], out["runs"]) == want
    assert np.array_equal(b["res"]["score"], ref["score"])
    # score-only, packed rows in
    sparams = _params(ms, rs, pen, req8=True, res8=True)
    with engine.DeviceSet(1) as s:
        s.configure_slots(sparams, n, slots=1, max_raw=n, max_runs=0)
        s.submit(0, 0, req, packed=engine.pack_batch(req, pat, txt))
        c = s.wait(0, 0)
    assert np.array_equal(c["res"]["score"], ref["score"])


ALIGN_DEVICE = '''
import sys
import numpy as np
import torch
torch.cuda.init()   # (before the library: the device buffers are torch's)
sys.path.insert(0, "tests")
import test_linear_gpu as t
t.align_device_matches_set_api()
print("ALIGN_DEVICE_OK")
'''


def test_align_device(gpu):
    """aim_align_device on torch-allocated device buffers (in a child process that brings up torch before the library)."""
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", ALIGN_DEVICE], cwd=root, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ALIGN_DEVICE_OK" in p.stdout, p.stdout + p.stderr


def align_device_matches_set_api():
    import torch
    from aim_amd import capi, engine
    lib = capi.load()
    pen = (4, 2)
    n = 1000
    req, pat, txt, rs = _pairs(41, n, 100, 0.05)
    ms = max_score_rule(100, 0.05, *pen)
    params = _params(ms, rs, pen, backtrace=True)
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
    _check(req, pat, txt, ref, rops, ms, pen)
    assert np.array_equal(res["score"], ref["score"]) and np.array_equal(res["begin_offset"], ref["begin_offset"])
    assert engine.format_output(res, ops, True) == engine.format_output(ref, rops, True)


@pytest.mark.parametrize("pen", [(1, 1), (5, 2)])
@pytest.mark.parametrize("wave", [False, True])
def test_over_cap_pairs_like_global_wfa(gpu, monkeypatch, wave, pen):
    from aim_amd import engine
    _, rs = engine.launcher_sizes("wfa", 150, 0.04)
    parts = [engine.gen_pairs(3 + i, 0, 750, 150, err, rs) for i, err in enumerate((0.01, 0.04))]   # half the pairs over the cap
    req, pat, txt = (np.concatenate([p[j] for p in parts]) for j in range(3))
    req["idx"] = np.arange(len(req))
    ms = max_score_rule(150, 0.02, *pen)
    if wave:
        monkeypatch.setenv("AIM_FORCE_WAVE", "1")
    res, ops = engine.align(_params(ms, rs, pen, backtrace=True), req, pat, txt)
    over = res["score"] > ms
    assert over.sum() > 100 and (~over).sum() > 100
    assert (res["score"][over] == ms + 1).all() and (res["status"] == 0).all()
    assert (res["begin_offset"][over] == res["end_offset"][over] - 1).all()
    _check(req, pat, txt, res, ops, ms, pen)


def test_debug_poison_changes_nothing(gpu, monkeypatch):
    from aim_amd import engine
    req, pat, txt, rs = _pairs(17, 1500, 150, 0.02)
    params = _params(max_score_rule(150, 0.02, 4, 2), rs, (4, 2), backtrace=True)
    a = engine.align(params, req, pat, txt)
    for k, v in (("AIM_DEBUG_POISON_SCRATCH", "165"), ("AIM_DEBUG_POISON_LDS", "90"), ("AIM_DEBUG_POISON_OPS", "7")):
        monkeypatch.setenv(k, v)
    b = engine.align(params, req, pat, txt)
    assert engine.format_output(a[0], a[1], True) == engine.format_output(b[0], b[1], True)
    _same(a, b)


@pytest.mark.parametrize("bt", [True, False])
def test_host_cli_linear(gpu, tmp_path, bt):
    from aim_amd import build, engine, gen_dataset
    n, l, e = 3000, 150, 0.02
    txt_in = tmp_path / "in.txt"
    pk_in = tmp_path / "in.pk"
    assert gen_dataset.main(["-n", str(n), "-l", str(l), "-e", str(e), "-o", str(txt_in), "-s", "8"]) == 0
    assert gen_dataset.main(["-n", str(n), "-l", str(l), "-e", str(e), "-o", str(pk_in), "-s", "8", "--packed"]) == 0
    _, rs = engine.launcher_sizes("wfa", l, e)
    ms = max_score_rule(l, 0.01, 4, 2)   # some pairs over the cap
    req, pat, txt = engine.parse_pairs(txt_in.read_bytes(), rs)
    res, ops = engine.align(_params(ms, rs, (4, 2), backtrace=bt), req, pat, txt)
    _check(req, pat, txt, res, ops, ms, (4, 2), scores_only=not bt)
    assert (res["score"] > ms).any()
    want = engine.format_output(res, ops, bt)
    outs = []
    for src, extra in ((txt_in, []), (pk_in, ["--packed-input"]), (txt_in, ["--full-ops"] if bt else ["--no-pack"])):
        out = tmp_path / ("out%d" % len(outs))
        cmd = [build.HOST_BIN, str(src), str(out), str(n), "--algo", "wfa", "--max-score", str(ms), "--read-size", str(rs),
               "--mismatch", "4", "--gap-e", "2", "--linear", "--threads", "4"] + (["--backtrace"] if bt else []) + extra
        p = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, p.stdout + p.stderr
        assert "wfa_group_kernel" in p.stdout, p.stdout
        outs.append(out.read_bytes())
    assert outs[0] == want
    assert outs[1] == outs[0]
    assert outs[2] == outs[0]
