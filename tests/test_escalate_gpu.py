"""AIM_FLAG_WFA_ESCALATE on the GPU: every per-pair output of a call with the flag equals that of the same call without it (result
rows, ops[begin_offset, end_offset), {idx, score} rows, compact headers and runs, the run total), over mixed clean / noisy batches, every
input and output layout, the entry points, the debugging knobs -- and equals the CPU oracle."""
import ctypes as C
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

MS, L = 25, 100          # the launchers' -e 0.05 cap at l = 100, default penalties


def _batch(seed, n, tail_frac, l=L, e_tail=0.05, n_bytes=True, over=True):
    """mixed_pairs + pairs with a byte outside A/C/G/T in the clean part and in the tail + one pair far over the full cap"""
    from aim_amd import engine
    rs = engine.launcher_sizes("wfa", l, e_tail)[1]
    req, pat, txt, tail = engine.mixed_pairs(seed, n, l, 0.01, e_tail, tail_frac, rs)
    if n_bytes and n >= 8:
        for i in list(np.flatnonzero(tail)[:2]) + list(np.flatnonzero(~tail)[:2]):
            pat[i, 7] = ord("N")
            txt[i, 3] = ord("N")
    if over and n >= 4:
        i = n // 2
        txt[i, :req["text_len"][i]] = np.frombuffer(b"ACGT" * 64, dtype=np.uint8)[:req["text_len"][i]]
        pat[i, :req["pattern_len"][i]] = np.frombuffer(b"TTGA" * 64, dtype=np.uint8)[:req["pattern_len"][i]]
    return req, pat, txt, rs


def _same_rows(a, ra, b, rb):
    """result rows equal; ops equal inside [begin_offset, end_offset)"""
    assert np.array_equal(a, b), np.flatnonzero(a != b)[:8]
    if ra is not None:
        cols = np.arange(ra.shape[1])[None, :]
        inside = (cols >= a["begin_offset"][:, None]) & (cols < a["end_offset"][:, None])
        assert np.array_equal(np.where(inside, ra, 0), np.where(inside, rb, 0))


def _same_cigars(a, b):
    for f in ("idx", "score", "n_runs", "status"):
        assert np.array_equal(a["cig"][f], b["cig"][f]), f
    assert len(a["runs"]) == len(b["runs"])          # the run total
    for x, y in ((a, b),):
        ra = [x["runs"][o:o + k] for o, k in zip(x["cig"]["run_offset"], x["cig"]["n_runs"])]
        rb = [y["runs"][o:o + k] for o, k in zip(y["cig"]["run_offset"], y["cig"]["n_runs"])]
        assert all(np.array_equal(p, q) for p, q in zip(ra, rb))


def _params(rs, escalate, ms=MS, **kw):
    from aim_amd import engine
    return engine.make_params("wfa", ms, rs, escalate=escalate, **kw)


@pytest.mark.parametrize("tail_frac", [0.0, 0.05, 0.5, 1.0])
@pytest.mark.parametrize("kw", [dict(), dict(reduce=True), dict(backtrace=True), dict(backtrace=True, reduce=True), dict(res8=True, req8=True)],
                         ids=["score", "score-reduce", "ops", "ops-reduce", "req8-res8"])
def test_push_launch_pull(tail_frac, kw):
    from aim_amd import engine
    req, pat, txt, rs = _batch(11, 5000, tail_frac)
    with engine.DeviceSet(1) as s:
        a, oa = s.align(_params(rs, True, **kw), req, pat, txt)
        line = s.plan_describe(0)
    assert " | wfa_group_kernel " in line and line.endswith(" escalate=10"), line
    b, ob = engine.align(_params(rs, False, **kw), req, pat, txt)
    _same_rows(a, oa, b, ob)
    if tail_frac == 1.0 and not kw.get("res8"):
        assert (b["score"] > 10).sum() > len(b) // 2   # the second stage did most of this batch


def test_equals_the_oracle():
    from aim_amd import engine
    from oracle import oracle
    req, pat, txt, rs = _batch(12, 4000, 0.2)
    res, ops = engine.align(_params(rs, True, backtrace=True), req, pat, txt)
    ores, oops, worst = oracle.align_batch(oracle.params("wfa", MS, rs, backtrace=True), req["pattern_len"], req["text_len"], pat, txt, nthreads=4)
    assert worst == 0
    assert np.array_equal(res["score"], ores["score"])
    assert (res["score"] == MS + 1).any() and ((res["score"] > 10) & (res["score"] <= MS)).any() and (res["score"] <= 10).any()
    assert engine.format_output(res, ops, True) == oracle.format_output(ores, oops, True)


@pytest.mark.parametrize("n", [1, 63, 65, 100000])
def test_batch_sizes(n):
    from aim_amd import engine
    req, pat, txt, rs = _batch(13, n, 0.05)
    for kw in (dict(), dict(backtrace=True)):
        a, oa = engine.align(_params(rs, True, **kw), req, pat, txt)
        b, ob = engine.align(_params(rs, False, **kw), req, pat, txt)
        _same_rows(a, oa, b, ob)


def _submit(params, req, pat, txt, packed, runs, slots=1, want_ops=False):
    from aim_amd import engine
    n = len(req)
    with engine.DeviceSet(1) as s:
        s.configure_slots(params, n, slots=slots, max_raw=n, max_runs=2 * params.read_size * n if runs else 0)
        outs = []
        for k in range(slots):
            if packed:
                s.submit(0, k, req, packed=engine.pack_batch(req, pat, txt), cigar_runs_cap=16 * n if runs else 0, want_ops=want_ops)
            else:
                s.submit(0, k, req, pat, txt, cigar_runs_cap=16 * n if runs else 0, want_ops=want_ops)
        for k in range(slots):
            outs.append(s.wait(0, k))
        return outs, s.plan_describe(0)


@pytest.mark.parametrize("l", [100, 150])
@pytest.mark.parametrize("packed", [False, True], ids=["ascii", "packed"])
@pytest.mark.parametrize("out", ["score", "ops", "runs", "runs+ops"])
def test_submit_layouts(l, packed, out):
    """aim_set_submit: ASCII and packed input; {idx, score}, result + ops rows, compact runs; two slots in flight"""
    e = 0.05 if l == 100 else 0.04
    req, pat, txt, rs = _batch(14 + l, 3000, 0.05, l=l, e_tail=e)
    from aim_amd import engine
    ms = engine.launcher_sizes("wfa", l, e)[0]
    kw = dict(res8=True, req8=True) if out == "score" else dict(backtrace=True, req8=True)
    runs, want_ops = out.startswith("runs"), out.endswith("ops")
    a, line = _submit(_params(rs, True, ms=ms, **kw), req, pat, txt, packed, runs, slots=2, want_ops=want_ops)
    assert line.endswith(" escalate=10"), line
    s1, s2 = line.split(" | ")
    assert s2.startswith("wfa_group_kernel ") and (" packed_in=%d runs_out=0" % int(packed)) in s2, line
    if packed:     # the fused packed lane kernel first, the group kernel reads the packed rows of the listed pairs itself
        assert s1.startswith("wfa_lane_packed_kernel ") and " pack_first=0 " in s1, line
    elif l == 100 and out == "score":
        assert s1.startswith("wfa_lane_kernel "), line
    else:          # ASCII rows of a shape only the packed lane kernel takes: packed on the device first
        assert s1.startswith("wfa_lane_packed_kernel ") and " pack_first=1 " in s1, line
    b, line0 = _submit(_params(rs, False, ms=ms, **kw), req, pat, txt, packed, runs, slots=1, want_ops=want_ops)
    assert "escalate" not in line0
    for x in a:
        if runs:
            _same_cigars(x, b[0])
        if "res" in x:
            _same_rows(x["res"], x.get("ops"), b[0]["res"], b[0].get("ops"))


def test_ref_texts():
    from aim_amd import engine
    rs = engine.launcher_sizes("wfa", L, 0.05)[1]
    req, pat, txt, tail = engine.mixed_pairs(21, 3000, L, 0.01, 0.05, 0.1, rs)
    # a reference made of the texts, one window per pair
    tl = req["text_len"].astype(np.int64)
    pos = np.concatenate([[0], np.cumsum(tl)[:-1]]).astype(np.uint64)
    reference = np.concatenate([txt[i, :tl[i]] for i in range(len(req))])
    for kw in (dict(), dict(backtrace=True)):
        a, oa = engine.align(_params(rs, True, ref_texts=True, **kw), req, pat, None, reference=reference, text_pos=pos)
        b, ob = engine.align(_params(rs, False, **kw), req, pat, txt)
        _same_rows(a, oa, b, ob)


def _ref_batch(seed, n):
    """pairs against a reference with N bases in it: clean reads with a noisy tail, windows on both strands"""
    from aim_amd import engine
    rs = engine.launcher_sizes("wfa", L, 0.05)[1]
    rng = np.random.default_rng(seed)
    reference = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=1 << 18)].copy()
    reference[rng.integers(0, len(reference), size=64)] = ord("N")
    clean = engine.ref_pairs(seed, 0, n, L, 0.01, reference, rs)
    noisy = engine.ref_pairs(seed, 0, n, L, 0.05, reference, rs)
    tail = engine.mixed_pairs(seed, n, L, 0.01, 0.05, 0.1, rs)[3]
    req, pat, pos, txt = [x.copy() for x in clean]
    for dst, src in zip((req, pat, pos, txt), noisy):
        dst[tail] = src[tail]
    return reference, req, pat, pos, txt, rs


@pytest.mark.parametrize("out", ["score", "runs", "runs+ops"])
def test_ref_texts_packed_submit(out):
    """packed patterns + text_pos through aim_set_submit: the plan goes back to ASCII rows after the gather; same outputs as flag-less"""
    from aim_amd import engine
    reference, req, pat, pos, txt, rs = _ref_batch(22, 3000)
    n = len(req)
    kw = dict(res8=True, req8=True) if out == "score" else dict(backtrace=True, req8=True)
    runs, want_ops = out.startswith("runs"), out.endswith("ops")
    got = []
    for esc in (True, False):
        with engine.DeviceSet(1) as s:
            s.configure_slots(_params(rs, esc, ref_texts=True, **kw), n, slots=1, max_raw=n, max_runs=2 * rs * n if runs else 0)
            s.set_reference(reference)
            s.submit(0, 0, req, packed=engine.pack_batch(req, pat, None), cigar_runs_cap=16 * n if runs else 0, want_ops=want_ops, text_pos=pos)
            got.append((s.wait(0, 0), s.plan_describe(0)))
    (a, line), (b, line0) = got
    assert line.endswith(" ref=1 escalate=10") and " | wfa_group_kernel " in line and " packed_in=0 " in line, line
    assert "escalate" not in line0
    if runs:
        _same_cigars(a, b)
    if "res" in a:
        _same_rows(a["res"], a.get("ops"), b["res"], b.get("ops"))
    # and the flag-less run with explicit texts
    c, oc = engine.align(_params(rs, False, **{k: v for k, v in kw.items() if k != "req8"}), req, pat, txt)
    if "res" in a:
        assert np.array_equal(a["res"]["score"], c["score"])
    else:
        assert np.array_equal(a["cig"]["score"], c["score"])


ALIGN_DEVICE_REF = r"""
import numpy as np, torch
from aim_amd import capi, engine
import sys
sys.path.insert(0, "tests")
from test_escalate_gpu import _ref_batch, _params, _same_rows
lib = capi.load()
reference, req, pat, pos, txt, rs = _ref_batch(23, 5000)
n = len(req)
dev = torch.device("cuda:0")
d_ref = torch.zeros(len(reference) + 64, dtype=torch.uint8, device=dev)
d_ref[: len(reference)] = torch.from_numpy(reference).to(dev)
out = []
for esc in (True, False):
    params = _params(rs, esc, backtrace=True, ref_texts=True)
    d_req = torch.from_numpy(req.view(np.uint8).copy()).to(dev)
    d_pat = torch.from_numpy(np.ascontiguousarray(pat)).to(dev)
    d_tp = torch.from_numpy(pos.view(np.uint8).copy()).to(dev)
    d_res = torch.zeros(n * capi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_ops = torch.zeros(n * 2 * rs, dtype=torch.uint8, device=dev)
    sb = lib.aim_scratch_bytes(capi.params_ref(params), n)
    assert sb > 0
    d_scr = torch.full((sb,), 0x5A, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rc = lib.aim_align_device_ref(capi.params_ref(params), n, d_req.data_ptr(), d_pat.data_ptr(), d_tp.data_ptr(), d_ref.data_ptr(), len(reference),
                                  d_res.data_ptr(), d_ops.data_ptr(), d_scr.data_ptr(), sb, None)
    assert rc == 0, lib.aim_last_error()
    torch.cuda.synchronize()
    out.append((d_res.cpu().numpy().view(capi.RESULT_DTYPE), d_ops.cpu().numpy().reshape(n, 2 * rs)))
_same_rows(out[0][0], out[0][1], out[1][0], out[1][1])
ref, rops = engine.align(_params(rs, False, backtrace=True), req, pat, txt)
_same_rows(out[0][0], out[0][1], ref, rops)
assert (out[0][0]["score"] > 10).any() and (out[0][0]["score"] <= 10).any()
print("ALIGN_DEVICE_REF_OK")
"""


def test_align_device_ref():
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", ALIGN_DEVICE_REF], cwd=root, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ALIGN_DEVICE_REF_OK" in p.stdout, p.stdout + p.stderr


# ---- the reference's own bytes ------------------------------------------------------------------------------------------------------

def _wfa_rows():
    from reference_rows import all_reference_rows
    return [c for c in all_reference_rows() if c["algo"] == "wfa"]


@pytest.mark.parametrize("case", _wfa_rows(), ids=lambda c: c["name"])
def test_reference_rows_with_the_flag(case, monkeypatch):
    """Every WFA reference row run with the flag gives the reference's digest (abort rows: the oracle's statuses and rows), as the
    flag-less run does, and the launch follows the plan line aim_plan_describe gives. Rows whose shape has no lane cap below their
    MAX_SCORE plan escalate=0 and run the flag-less plan; they are checked all the same."""
    from reference_rows import apply_env, knob_env, plan_key, plan_line, row_params
    from test_reference_rows_gpu import _check, _run
    apply_env(monkeypatch, knob_env({}))
    params = row_params(case, escalate=True)
    rc, planned = plan_line(params, case["gen"]["n"])
    assert rc == 0 and " escalate=" in planned, planned
    res, ops, launched = _run(params, case)
    assert plan_key(launched) == plan_key(planned)
    why = _check(case, res, ops)
    assert why is None, "%s: %s" % (launched, why)


def test_reference_rows_reach_two_stages(monkeypatch):
    """... and enough of them have a first stage: the rows above do not all plan escalate=0"""
    from reference_rows import apply_env, knob_env, plan_line, row_params
    apply_env(monkeypatch, knob_env({}))
    two = [c["name"] for c in _wfa_rows() if not plan_line(row_params(c, escalate=True), c["gen"]["n"])[1].endswith(" escalate=0")]
    assert len(two) >= 5, two


ALIGN_DEVICE = r"""
import numpy as np, torch
from aim_amd import capi, engine
import sys
sys.path.insert(0, "tests")
from test_escalate_gpu import _batch, _params, _same_rows
lib = capi.load()
req, pat, txt, rs = _batch(31, 5000, 0.1)
n = len(req)
dev = torch.device("cuda:0")
out = []
for esc in (True, False):
    params = _params(rs, esc, backtrace=True)
    d_req = torch.from_numpy(req.view(np.uint8).copy()).to(dev)
    d_pat = torch.from_numpy(np.ascontiguousarray(pat)).to(dev)
    d_txt = torch.from_numpy(np.ascontiguousarray(txt)).to(dev)
    d_res = torch.zeros(n * capi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_ops = torch.zeros(n * 2 * rs, dtype=torch.uint8, device=dev)
    sb = lib.aim_scratch_bytes(capi.params_ref(params), n)
    assert sb > 0
    d_scr = torch.full((sb,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rc = lib.aim_align_device(capi.params_ref(params), n, d_req.data_ptr(), d_pat.data_ptr(), d_txt.data_ptr(), d_res.data_ptr(),
                              d_ops.data_ptr(), d_scr.data_ptr(), sb, None)
    assert rc == 0, lib.aim_last_error()
    torch.cuda.synchronize()
    out.append((d_res.cpu().numpy().view(capi.RESULT_DTYPE), d_ops.cpu().numpy().reshape(n, 2 * rs)))
_same_rows(out[0][0], out[0][1], out[1][0], out[1][1])
assert (out[0][0]["score"] > 10).any()
print("ALIGN_DEVICE_OK")
"""


def test_align_device():
    import os
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-c", ALIGN_DEVICE], cwd=root, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ALIGN_DEVICE_OK" in p.stdout, p.stdout + p.stderr


@pytest.mark.parametrize("env", [{"AIM_DEBUG_POISON_SCRATCH": "165"}, {"AIM_DEBUG_POISON_OPS": "90"}, {"AIM_DEBUG_POISON_LDS": "255"},
                                 {"AIM_CHIP_CUS": "64"}, {"AIM_CHIP_CUS": "304"}, {"AIM_GROUP_OVERLAP": "1", "AIM_SCRATCH_GB": "0.25"}],
                         ids=lambda e: "+".join(e))
def test_knobs_change_nothing(env, monkeypatch):
    from aim_amd import engine
    req, pat, txt, rs = _batch(41, 20000, 0.3)
    want = {}
    for name, kw in (("score", dict()), ("ops", dict(backtrace=True))):
        want[name] = engine.align(_params(rs, False, **kw), req, pat, txt)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for name, kw in (("score", dict()), ("ops", dict(backtrace=True))):
        a, oa = engine.align(_params(rs, True, **kw), req, pat, txt)
        _same_rows(a, oa, want[name][0], want[name][1])


@pytest.mark.parametrize("packed_wire", [False, True], ids=["text", "packed-file"])
@pytest.mark.parametrize("bt", [False, True], ids=["score", "cigar"])
def test_host_cli(tmp_path, packed_wire, bt):
    """host --escalate writes the file the flag-less run writes, on both wire formats"""
    from aim_amd import build, engine
    req, pat, txt, rs = _batch(51, 4000, 0.1)
    lines = []
    for i in range(len(req)):
        lines.append(b">" + pat[i, :req["pattern_len"][i]].tobytes())
        lines.append(b"<" + txt[i, :req["text_len"][i]].tobytes())
    inp = tmp_path / "in.txt"
    inp.write_bytes(b"\n".join(lines) + b"\n")
    base = [str(len(req)), "--algo", "wfa", "--max-score", str(MS), "--read-size", str(rs), "--mismatch", "3", "--gap-o", "4", "--gap-e", "1",
            "--nr-dpus", "1", "--threads", "4"] + (["--backtrace"] if bt else [])
    src = str(inp)
    if packed_wire:
        pk = tmp_path / "in.pk"
        p = subprocess.run([build.HOST_BIN, str(inp), str(tmp_path / "unused")] + base + ["--pack-only", str(pk)], cwd=tmp_path, capture_output=True, text=True, timeout=180)
        assert p.returncode == 0, p.stdout + p.stderr
        src, base = str(pk), base + ["--packed-input"]
    outs = []
    for extra in (["--escalate"], []):
        out = tmp_path / ("out" + str(len(extra)))
        p = subprocess.run([build.HOST_BIN, src, str(out)] + base + extra, cwd=tmp_path, capture_output=True, text=True, timeout=180)
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append(out.read_bytes())
    assert outs[0] == outs[1] and len(outs[0]) > 0
