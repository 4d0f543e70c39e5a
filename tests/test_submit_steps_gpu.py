"""aim_set_submit is a sequence of steps over one slot (check, reset, inputs, text rows, alignment, raw side pass, outputs), and the launch
of a plan takes its buffers by name (capi_launch.hip). What the per-shape launcher tests do not run is state carried on a slot between
batches of different shape: here one slot takes a packed batch with both outputs, a one-pair ASCII batch, an empty batch, a refused
submit and an ASCII batch with the compact CIGAR, one after the other; the same under AIM_FLAG_REF_TEXTS; and a wfa_group launch in
several history chunks through the stateless entry point (the device's shared aux stream) and through a slot (its own). Everything is
compared with the oracle, and the batches of the reused slot with what a fresh set gives for each of them alone, byte for byte."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

L, ERR, RS = 100, 0.01, 112
MAX_PAIRS = 65
RUNS_CAP = 2 * RS * MAX_PAIRS


def _oracle_text(algo, params, req, pat, txt):
    import test_gpu_parity as gp
    return gp._oracle_text(algo, params, req, pat, txt)


def _wfa(rs, **kw):
    from aim_amd import engine
    return engine.make_params("wfa", engine.launcher_sizes("wfa", L, ERR)[0], rs, **kw)


def _assert_oracle(out, ores, want):
    from aim_amd import engine
    if "res" in out:
        assert np.array_equal(out["res"]["score"], ores["score"])
        assert engine.format_output(out["res"], out["ops"], True) == want
    if "cig" in out:
        assert np.array_equal(out["cig"]["score"], ores["score"])
        assert int(out["cig"]["n_runs"].sum()) <= len(out["runs"])
        assert engine.format_output_runs(out["cig"], out["runs"]) == want


def _assert_same_bytes(a, b):
    """Two outputs of one batch: result rows whole, ops rows inside [begin_offset, end_offset), headers and runs in pair order (the
    place of a pair's runs in a bump-allocated run buffer depends on scheduling)."""
    assert sorted(a) == sorted(b)
    if "res" in a:
        assert np.array_equal(a["res"], b["res"])
        for i in range(len(a["res"])):
            lo, hi = int(a["res"]["begin_offset"][i]), int(a["res"]["end_offset"][i])
            assert bytes(a["ops"][i, lo:hi]) == bytes(b["ops"][i, lo:hi]), i
    if "cig" in a:
        for f in ("idx", "score", "n_runs", "status"):
            assert np.array_equal(a["cig"][f], b["cig"][f]), f
        for i in range(len(a["cig"])):
            ra, rb = (o["runs"][int(o["cig"]["run_offset"][i]):int(o["cig"]["run_offset"][i]) + int(o["cig"]["n_runs"][i])] for o in (a, b))
            assert np.array_equal(ra, rb), i


def _configure(s, params):
    s.configure_slots(params, MAX_PAIRS, slots=2, max_raw=MAX_PAIRS, max_runs=RUNS_CAP)


def _alone(params, req, kw):
    from aim_amd import engine
    with engine.DeviceSet(1) as s:
        _configure(s, params)
        s.submit(0, 0, req, **kw)
        return s.wait(0, 0, check=False)


def test_one_slot_takes_batches_of_different_shape():
    from aim_amd import capi, engine
    params = _wfa(RS, backtrace=True)
    # 1: packed, one raw pair, compact CIGAR and result rows + ops rows out of the same submit
    req1, pat1, txt1 = engine.gen_pairs(51, 0, MAX_PAIRS, L, ERR, RS)
    pat1[MAX_PAIRS // 2, 5] = ord("N")
    packed1 = engine.pack_batch(req1, pat1, txt1)
    assert packed1[2].tolist() == [MAX_PAIRS // 2]
    kw1 = dict(packed=packed1, cigar_runs_cap=RUNS_CAP, want_ops=True)
    # 2: one ASCII pair, result rows + ops rows; 5: 63 ASCII pairs, compact CIGAR only
    req2, pat2, txt2 = engine.gen_pairs(52, 0, 1, L, ERR, RS)
    kw2 = dict(pat=pat2, txt=txt2, want_ops=True)
    req5, pat5, txt5 = engine.gen_pairs(55, 0, 63, L, ERR, RS)
    kw5 = dict(pat=pat5, txt=txt5, cigar_runs_cap=RUNS_CAP)
    want1, want2, want5 = (_oracle_text("wfa", params, r, p, t) for r, p, t in ((req1, pat1, txt1), (req2, pat2, txt2), (req5, pat5, txt5)))
    with engine.DeviceSet(1) as s:
        _configure(s, params)
        s.submit(0, 0, req1, **kw1)
        s.submit(0, 1, req2, **kw2)               # slot 1 while slot 0 holds batch 1 unwaited; waited in the reverse order
        out2_slot1 = s.wait(0, 1, check=False)
        out1 = s.wait(0, 0, check=False)
        print(s.plan_describe(0))
        s.submit(0, 0, req2, **kw2)
        out2 = s.wait(0, 0, check=False)
        # 3: an empty batch needs submit and wait and produces nothing
        s.submit(0, 0, req2[:0], pat=pat2[:0], txt=txt2[:0], want_ops=True)
        out3 = s.wait(0, 0, check=False)
        assert len(out3["res"]) == 0 and len(out3["ops"]) == 0
        # 4: refused before anything is enqueued; the slot does not count as submitted
        bad = (packed1[0], packed1[1], np.array([MAX_PAIRS], dtype=np.uint32), packed1[3], packed1[4])
        with pytest.raises(capi.AimError) as e:
            s.submit(0, 0, req1, packed=bad, want_ops=True)
        assert e.value.code == capi.AIM_EINVAL and "raw_pairs[0] = %d is outside the batch" % MAX_PAIRS in str(e.value)
        rc = s.lib.aim_set_wait(s.handle, 0, 0, None)
        assert rc == capi.AIM_ESTATE and b"slot 0 of device" in s.lib.aim_last_error() and b"holds no batch" in s.lib.aim_last_error()
        s.submit(0, 0, req5, **kw5)
        out5 = s.wait(0, 0, check=False)
    for out, (ores, want) in ((out1, want1), (out2, want2), (out2_slot1, want2), (out5, want5)):
        _assert_oracle(out, ores, want)
    _assert_same_bytes(out1, _alone(params, req1, kw1))
    alone2 = _alone(params, req2, kw2)
    _assert_same_bytes(out2, alone2)
    _assert_same_bytes(out2_slot1, alone2)
    _assert_same_bytes(out5, _alone(params, req5, kw5))


def test_one_slot_takes_ref_texts_batches_of_different_shape():
    """A packed batch with an N inside one window and an N in one pattern (the fused gather, the to-do tail and the side list's
    gather), then an ASCII batch on the same slot; a packed batch at READ_SIZE 120 on a second set, where the planner has no packed
    kernel. All against the flag-less oracle over the gathered texts."""
    import test_ref_texts_gpu as rt
    from aim_amd import engine
    ref = rt.make_reference(56, 100000, specials=False)
    rp = {}
    for key, seed, n, rs in (("packed", 56, MAX_PAIRS, RS), ("ascii", 57, 63, RS), ("packed120", 58, MAX_PAIRS, 120)):
        rp[key] = list(engine.ref_pairs(seed, 0, n, L, ERR, ref, rs, minus_fraction=0.5))
    for key in ("packed", "packed120"):
        ref[(int(rp[key][2][0]) & ((1 << 63) - 1)) + 9] = ord("N")           # an N inside the first pair's window ...
        rp[key][1][MAX_PAIRS - 1, 5] = ord("N")                               # ... and one in the last pair's pattern
    want = {}
    for key, (req, pat, tpos, _) in rp.items():
        rs = pat.shape[1]
        rp[key][3] = txt = rt.texts_of(ref, req, tpos, rs)                    # (the windows of the reference as it is now)
        want[key] = _oracle_text("wfa", _wfa(rs, backtrace=True), req, pat, txt)
    for key in ("packed", "packed120"):
        assert ord("N") in rp[key][3][0, :int(rp[key][0]["text_len"][0])]
    out = {}
    with engine.DeviceSet(1) as s:
        s.configure_slots(_wfa(RS, backtrace=True, ref_texts=True), MAX_PAIRS, slots=1, max_raw=MAX_PAIRS, max_runs=RUNS_CAP)
        s.set_reference(ref)
        req, pat, tpos, _ = rp["packed"]
        s.submit(0, 0, req, packed=engine.pack_batch(req, pat, None), cigar_runs_cap=RUNS_CAP, text_pos=tpos)
        out["packed"] = s.wait(0, 0, check=False)
        plan = s.plan_describe(0)
        print(plan)
        assert plan.startswith("wfa_lane_packed_kernel"), plan
        req, pat, tpos, _ = rp["ascii"]
        s.submit(0, 0, req, pat=pat, text_pos=tpos, want_ops=True)
        out["ascii"] = s.wait(0, 0, check=False)
    with engine.DeviceSet(1) as s:
        s.configure_slots(_wfa(120, backtrace=True, ref_texts=True), MAX_PAIRS, slots=1, max_raw=MAX_PAIRS, max_runs=2 * 120 * MAX_PAIRS)
        s.set_reference(ref)
        req, pat, tpos, _ = rp["packed120"]
        s.submit(0, 0, req, packed=engine.pack_batch(req, pat, None), cigar_runs_cap=2 * 120 * MAX_PAIRS, text_pos=tpos)
        out["packed120"] = s.wait(0, 0, check=False)
        print(s.plan_describe(0))
    for key in rp:
        _assert_oracle(out[key], *want[key])


def test_chunked_wfa_group_stateless_and_on_a_slot(monkeypatch):
    """wfa_group with CIGAR in several history chunks: the traceback of a chunk runs on a second stream, the device's shared one for
    aim_align_device and the slot's own for a DeviceSet. The scratch bound is test_linear_gpu.py::test_history_in_several_chunks'
    formula -- room for four history buffers of `fit` pairs, of which the plan gives the two alternating ones half -- with the history
    bytes of a pair read from the unbounded plan line (gap-affine here, which the oracle aligns), and that test's n."""
    from aim_amd import capi, engine
    lib = capi.load()
    n, fit = 12000, 5000
    ms, rs = engine.launcher_sizes("wfa", 1000, 0.05)
    params = engine.make_params("wfa", ms, rs, backtrace=True, reduce=True)
    req, pat, txt = engine.gen_pairs(31, 0, n, 1000, 0.05, rs)
    ores, want = _oracle_text("wfa", params, req, pat, txt)

    def plan_line():
        with engine.DeviceSet(1) as s:
            s.configure(params, n)
            return s.plan_describe(0)

    line = plan_line()
    assert line.startswith("wfa_group_kernel"), line
    hist, chunk = (int(re.search(r" %s=(\d+)" % k, line).group(1)) for k in ("hist", "chunk"))
    assert chunk == n, line
    monkeypatch.setenv("AIM_SCRATCH_GB", "%.6f" % (4.0 * fit * (hist // n) / (1 << 30) + 0.02))
    line = plan_line()
    assert line.startswith("wfa_group_kernel"), line
    chunk = int(re.search(r" chunk=(\d+)", line).group(1))
    assert 0 < chunk < n // 2, line                  # the batch really runs as several launches
    # the stateless entry point, on device buffers of the HIP runtime the library loaded (the scratch as hipMalloc leaves it)
    import test_sam_fields_gpu as S
    h = S.Hip()
    try:
        d_req, d_pat, d_txt = h.up(req), h.up(pat, slack=64), h.up(txt, slack=64)
        d_res, d_ops = h.up(np.zeros(n * capi.RESULT_DTYPE.itemsize, dtype=np.uint8)), h.up(np.zeros(n * 2 * rs, dtype=np.uint8), slack=64)
        sb = int(lib.aim_scratch_bytes(capi.params_ref(params), n))
        assert sb > 0
        d_scr = C.c_void_p()
        assert h.lib.hipMalloc(C.byref(d_scr), sb) == 0
        h.bufs.append(d_scr)
        rc = lib.aim_align_device(capi.params_ref(params), n, d_req, d_pat, d_txt, d_res, d_ops, d_scr, sb, None)
        assert rc == 0, lib.aim_last_error()
        res = h.down(d_res, n * capi.RESULT_DTYPE.itemsize).view(capi.RESULT_DTYPE)
        ops = h.down(d_ops, n * 2 * rs).reshape(n, 2 * rs)
    finally:
        h.free()
    assert np.array_equal(res["score"], ores["score"])
    assert engine.format_output(res, ops, True) == want
    # a DeviceSet batch of the same pairs
    with engine.DeviceSet(1) as s:
        s.configure_slots(params, n, slots=1)
        s.submit(0, 0, req, pat=pat, txt=txt, want_ops=True)
        out = s.wait(0, 0, check=False)
        assert re.search(r" chunk=%d " % chunk, s.plan_describe(0)), s.plan_describe(0)
    assert np.array_equal(out["res"]["score"], ores["score"])
    assert engine.format_output(out["res"], out["ops"], True) == want
