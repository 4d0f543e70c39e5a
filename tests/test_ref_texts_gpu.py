"""Texts named by (position, strand) into a device-resident reference (AIM_FLAG_REF_TEXTS) on the GPU. The whole contract is
equality: results (every field), ops rows [begin_offset, end_offset), compact runs and headers equal the explicit-text run of the
same pairs, on every algorithm and mode, on both strands, at the reference's ends, and for windows holding N and lowercase bytes
(which must take the same to-do / raw routes as explicit texts). Then the entry points: aim_set_push_ref, aim_set_submit with two
slots, packed patterns, a raw side list and compact runs, aim_align_device_ref on torch tensors, a replaced reference, a
reference beyond 4 GiB, the fused headline plan, and out-of-range windows refused before anything is enqueued."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_reference(seed, length, specials=True):
    """Random A/C/G/T with (specials) runs of N and lowercase stretches: the bytes a soft-masked genome holds."""
    rng = np.random.default_rng([seed, 0x7265664C])
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=length)].copy()
    if specials:
        for _ in range(max(1, length // 20000)):
            at = int(rng.integers(0, length - 64))
            ref[at:at + int(rng.integers(1, 40))] = ord("N")
            at = int(rng.integers(0, length - 512))
            span = slice(at, at + int(rng.integers(16, 500)))
            ref[span] = ref[span] | 0x20
    return ref


def uppercase_acgt(req, pat):
    """Patterns with every byte outside A/C/G/T inside the sequence replaced by an upper-case base: their pairs are packable
    patterns whose texts may still hold N / lowercase (the to-do route instead of the raw side list)."""
    out = pat.copy()
    for i in range(len(req)):
        row = out[i, :int(req["pattern_len"][i])]
        up = row & 0xDF
        ok = np.isin(up, np.frombuffer(b"ACGT", dtype=np.uint8))
        row[:] = np.where(ok, up, ord("A"))
    return out


def edge_windows(req, tpos, ref_len):
    """Pairs 0 / 1 start at position 0 (both strands), pairs 2 / 3 end exactly at ref_len."""
    tp = tpos.copy()
    for i, minus in ((0, 0), (1, 1), (2, 0), (3, 1)):
        start = 0 if i < 2 else ref_len - int(req["text_len"][i])
        tp[i] = np.uint64(start | (minus << 63))
    return tp


def texts_of(ref, req, tpos, rs):
    from aim_amd import engine
    txt = np.zeros((len(req), rs), dtype=np.uint8)
    for i in range(len(req)):
        tl = int(req["text_len"][i])
        w = engine.ref_window(ref, int(tpos[i]) & ((1 << 63) - 1), tl, bool(int(tpos[i]) >> 63))
        txt[i, :tl] = w
    return txt


def assert_same(res, ops, res0, ops0, bt):
    assert np.array_equal(res, res0)
    if bt:
        for i in range(len(res)):
            b, e = int(res0["begin_offset"][i]), int(res0["end_offset"][i])
            assert np.array_equal(ops[i, b:e], ops0[i, b:e]), i


def assert_same_runs(a, b):
    ca, cb = a["cig"], b["cig"]
    for k in ("idx", "score", "n_runs", "status"):
        assert np.array_equal(ca[k], cb[k]), k
    for i in range(len(ca)):
        oa, ob, n = int(ca["run_offset"][i]), int(cb["run_offset"][i]), int(ca["n_runs"][i])
        assert np.array_equal(a["runs"][oa:oa + n], b["runs"][ob:ob + n]), i


# (algo, length, error, pairs, make_params keywords)
CASES = [
    ("nw", 100, 0.02, 3000, dict(backtrace=True)),
    ("nw", 1000, 0.05, 256, dict()),
    ("swg", 100, 0.02, 3000, dict(backtrace=True)),
    ("swg", 100, 0.02, 2000, dict(backtrace=True, swg_w16=True)),
    ("swg", 1000, 0.02, 256, dict(res8=True)),
    ("wfa", 100, 0.01, 4000, dict(backtrace=True)),
    ("wfa", 100, 0.01, 4000, dict(reduce=True, res8=True)),
    ("wfa", 100, 0.05, 3000, dict(reduce=True, backtrace=True, req8=True)),
    ("wfa", 150, 0.02, 2000, dict(backtrace=True)),
    ("wfa", 1000, 0.05, 512, dict(backtrace=True)),
    ("wfa", 10000, 0.01, 48, dict(backtrace=True)),
    ("wfa", 300, 0.03, 1000, dict(backtrace=True, ends_free=(0, 0, 20, 20))),
    ("wfa", 300, 0.03, 1000, dict(backtrace=True, gap2=(24, 1), mismatch=4, gap_o=4, gap_e=2)),
    ("wfa", 300, 0.03, 1000, dict(backtrace=True, linear=True, mismatch=1, gap_e=1)),
    ("wfa", 1000, 0.02, 256, dict(backtrace=True, w32=True)),
    ("wfa", 1000, 0.05, 256, dict(backtrace=True, bidir=True)),
    ("genasm", 1000, 0.05, 128, dict(backtrace=True)),
    ("genasm", 10000, 0.02, 16, dict()),
]


@pytest.mark.parametrize("algo,length,error,n,kw", CASES, ids=["%s-l%d-%s" % (c[0], c[1], "-".join(sorted(c[4]))) for c in CASES])
def test_ref_texts_equal_explicit_texts(algo, length, error, n, kw):
    from aim_amd import engine
    ref = make_reference(length, 400000)
    if algo == "genasm":
        ms, rs = 0, engine.round_up_8(int(length * (1 + error)) + 8)
    else:
        cost = {k: kw[k] for k in ("mismatch", "gap_o", "gap_e") if k in kw}
        ms, rs = engine.launcher_sizes(algo, length, error, **cost)
        if "ends_free" in kw:
            rs += 48
    req, pat, tpos, txt = engine.ref_pairs(length, 0, n, length, error, ref, rs, minus_fraction=0.5)
    half = n // 2
    pat[:half] = uppercase_acgt(req[:half], pat[:half])     # texts with N / lowercase behind ACGT patterns (to-do route)
    tpos = edge_windows(req, tpos, len(ref))
    txt = texts_of(ref, req, tpos, rs)
    p0 = engine.make_params(algo, ms, rs, **kw)
    p1 = engine.make_params(algo, ms, rs, ref_texts=True, **kw)
    res0, ops0 = engine.align(p0, req, pat, txt, check=False)
    res1, ops1 = engine.align(p1, req, pat, None, check=False, reference=ref, text_pos=tpos)
    assert_same(res1, ops1, res0, ops0, kw.get("backtrace", False))


def test_w32_40000():
    from aim_amd import engine
    ref = make_reference(7, 300000)
    length, error = 40000, 0.01
    ms, rs = engine.launcher_sizes("wfa", length, error)
    req, pat, tpos, txt = engine.ref_pairs(40, 0, 4, length, error, ref, rs)
    p0 = engine.make_params("wfa", ms, rs, w32=True)
    p1 = engine.make_params("wfa", ms, rs, w32=True, ref_texts=True)
    res0, _ = engine.align(p0, req, pat, txt, check=False)
    res1, _ = engine.align(p1, req, pat, None, check=False, reference=ref, text_pos=tpos)
    assert np.array_equal(res1, res0)


def _submit_both(params0, params1, ref, req, pat, tpos, txt, packed, runs, want_ops=False, slots=2, chunks=3, runs_per_pair=8):
    """The same batches through aim_set_submit (two slots, alternating) with explicit texts and with text_pos."""
    from aim_amd import engine
    n = len(req)
    outs = []
    for params, use_ref in ((params0, False), (params1, True)):
        got = []
        with engine.DeviceSet(1) as s:
            s.configure_slots(params, n, slots=slots, max_raw=n if packed else 0, max_runs=runs_per_pair * n if runs else 0)
            if use_ref:
                s.set_reference(ref)
            bounds = np.linspace(0, n, chunks + 1).astype(int)
            for c in range(chunks):
                lo, hi = bounds[c], bounds[c + 1]
                sl = slice(lo, hi)
                kw = dict(cigar_runs_cap=runs_per_pair * n if runs else 0, want_ops=want_ops)
                if use_ref:
                    kw["text_pos"] = tpos[sl]
                    if packed:
                        kw["packed"] = engine.pack_batch(req[sl], pat[sl], None)
                    else:
                        kw["pat"] = pat[sl]
                else:
                    if packed:
                        kw["packed"] = engine.pack_batch(req[sl], pat[sl], txt[sl])
                    else:
                        kw["pat"], kw["txt"] = pat[sl], txt[sl]
                s.submit(0, c % slots, req[sl], **kw)
                if c >= slots - 1:
                    got.append(s.wait(0, (c - slots + 1) % slots, check=False))
            for c in range(max(0, chunks - slots + 1), chunks):
                got.append(s.wait(0, c % slots, check=False))
            plan = s.plan_describe(0)
        outs.append((got, plan))
    return outs


@pytest.mark.parametrize("kw,runs", [(dict(reduce=True, backtrace=True, req8=True), True), (dict(reduce=True, res8=True), False),
                                     (dict(backtrace=True), True), (dict(backtrace=True), False)],
                         ids=["adaptive-cigar-runs", "adaptive-res8", "wfa-cigar-runs", "wfa-cigar-ops"])
def test_submit_packed_headline(kw, runs):
    """WFA at l = 100 with packed patterns: the fused wfa_lane_packed_kernel runs under the flag as without it; non-ACGT patterns
    travel on the raw side list, non-ACGT windows take the to-do route; every output equals the explicit-text batches'."""
    from aim_amd import engine
    ref = make_reference(11, 200000)
    ms, rs = engine.launcher_sizes("wfa", 100, 0.01)
    n = 6000
    req, pat, tpos, txt = engine.ref_pairs(100, 0, n, 100, 0.01, ref, rs)
    pat[: n // 2] = uppercase_acgt(req[: n // 2], pat[: n // 2])
    tpos = edge_windows(req, tpos, len(ref))
    txt = texts_of(ref, req, tpos, rs)
    p0 = engine.make_params("wfa", ms, rs, **kw)
    p1 = engine.make_params("wfa", ms, rs, ref_texts=True, **kw)
    (g0, plan0), (g1, plan1) = _submit_both(p0, p1, ref, req, pat, tpos, txt, packed=True, runs=runs, want_ops=not runs and kw.get("backtrace", False))
    assert plan0.startswith("wfa_lane_packed_kernel"), plan0
    assert plan1.split()[0] == plan0.split()[0], (plan0, plan1)
    assert plan1.endswith(" ref=1")
    raw_txt = sum(1 for i in range(n) if not set(txt[i, :int(req["text_len"][i])].tobytes()) <= set(b"ACGT"))
    assert raw_txt > 20                                        # the to-do route was taken
    for a, b in zip(g0, g1):
        if runs:
            assert_same_runs(b, a)
        else:
            assert np.array_equal(b["res"], a["res"])
            if "ops" in a:
                assert_same(b["res"], b["ops"], a["res"], a["ops"], True)


@pytest.mark.parametrize("algo,length,error,kw,packed", [("nw", 1000, 0.05, dict(backtrace=True), True),
                                                         ("wfa", 1000, 0.02, dict(backtrace=True), True),
                                                         ("swg", 100, 0.02, dict(backtrace=True), False)])
def test_submit_other_plans(algo, length, error, kw, packed):
    from aim_amd import engine
    ref = make_reference(13, 300000)
    ms, rs = engine.launcher_sizes(algo, length, error)
    n = 600
    req, pat, tpos, txt = engine.ref_pairs(length, 5, n, length, error, ref, rs)
    p0 = engine.make_params(algo, ms, rs, **kw)
    p1 = engine.make_params(algo, ms, rs, ref_texts=True, **kw)
    (g0, _), (g1, plan1) = _submit_both(p0, p1, ref, req, pat, tpos, txt, packed=packed, runs=True, runs_per_pair=256)
    assert plan1.endswith(" ref=1")
    for a, b in zip(g0, g1):
        assert_same_runs(b, a)


ALIGN_DEVICE_REF = '''
import sys
import torch
torch.cuda.init()   # (before the library: the device buffers are torch's)
sys.path.insert(0, "tests")
import test_ref_texts_gpu as t
t.align_device_ref_torch()
print("ALIGN_DEVICE_REF_OK")
'''


def test_align_device_ref_torch():
    """aim_align_device_ref on torch-allocated device buffers (in a child process that brings up torch before the library)."""
    p = subprocess.run([sys.executable, "-c", ALIGN_DEVICE_REF], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ALIGN_DEVICE_REF_OK" in p.stdout, p.stdout + p.stderr


def align_device_ref_torch():
    import torch
    from aim_amd import capi, engine
    lib = capi.load()
    ref = make_reference(17, 100000)
    ms, rs = engine.launcher_sizes("wfa", 100, 0.02)
    n = 3000
    req, pat, tpos, txt = engine.ref_pairs(3, 0, n, 100, 0.02, ref, rs)
    tpos = edge_windows(req, tpos, len(ref))
    txt = texts_of(ref, req, tpos, rs)
    params = engine.make_params("wfa", ms, rs, backtrace=True, ref_texts=True)
    p0 = engine.make_params("wfa", ms, rs, backtrace=True)
    dev = torch.device("cuda:0")
    d_req = torch.from_numpy(req.view(np.uint8).copy()).to(dev)
    d_pat = torch.from_numpy(np.ascontiguousarray(pat)).to(dev)
    d_tp = torch.from_numpy(tpos.view(np.uint8).copy()).to(dev)
    d_ref = torch.zeros(len(ref) + 64, dtype=torch.uint8, device=dev)
    d_ref[: len(ref)] = torch.from_numpy(ref).to(dev)
    d_res = torch.zeros(n * capi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_ops = torch.zeros(n * 2 * rs, dtype=torch.uint8, device=dev)
    sb = lib.aim_scratch_bytes(capi.params_ref(params), n)
    assert sb > 0
    d_scr = torch.zeros(sb, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    rc = lib.aim_align_device_ref(capi.params_ref(params), n, d_req.data_ptr(), d_pat.data_ptr(), d_tp.data_ptr(), d_ref.data_ptr(), len(ref),
                                  d_res.data_ptr(), d_ops.data_ptr(), d_scr.data_ptr(), sb, None)
    assert rc == 0, lib.aim_last_error()
    torch.cuda.synchronize()
    res = d_res.cpu().numpy().view(capi.RESULT_DTYPE)
    ops = d_ops.cpu().numpy().reshape(n, 2 * rs)
    res0, ops0 = engine.align(p0, req, pat, txt)
    assert_same(res, ops, res0, ops0, True)


def test_reference_replaced_between_batches():
    from aim_amd import engine
    ms, rs = engine.launcher_sizes("wfa", 100, 0.02)
    p0 = engine.make_params("wfa", ms, rs, backtrace=True)
    p1 = engine.make_params("wfa", ms, rs, backtrace=True, ref_texts=True)
    with engine.DeviceSet(1) as s:
        for k in range(3):
            ref = make_reference(100 + k, 50000 + 1000 * k)
            req, pat, tpos, txt = engine.ref_pairs(k, 0, 1500, 100, 0.02, ref, rs)
            res1, ops1 = s.align(p1, req, pat, None, reference=ref, text_pos=tpos)
            res0, ops0 = engine.align(p0, req, pat, txt)
            assert_same(res1, ops1, res0, ops0, True)
            assert s.plan_describe(0).endswith(" ref=1")


def test_reference_beyond_4gib():
    from aim_amd import engine
    L = (1 << 32) + (1 << 28)
    ref = np.full(L, ord("A"), dtype=np.uint8)
    tail = make_reference(23, 1 << 20)
    ref[L - len(tail):] = tail
    head = make_reference(24, 1 << 16)
    ref[:len(head)] = head
    ms, rs = engine.launcher_sizes("wfa", 100, 0.02)
    n = 2000
    req, pat, tpos, _ = engine.ref_pairs(29, 0, n, 100, 0.02, tail, rs)
    tpos = tpos + np.uint64(L - len(tail))                      # (bit 63 is unchanged: no carry reaches it)
    tpos[:2] = [np.uint64(5), np.uint64(7 | (1 << 63))]
    tpos[2] = np.uint64(L - int(req["text_len"][2]))
    assert int((tpos & np.uint64((1 << 63) - 1)).max()) > (1 << 32)
    txt = texts_of(ref, req, tpos, rs)
    p0 = engine.make_params("wfa", ms, rs, backtrace=True)
    p1 = engine.make_params("wfa", ms, rs, backtrace=True, ref_texts=True)
    res1, ops1 = engine.align(p1, req, pat, None, reference=ref, text_pos=tpos)
    del ref
    res0, ops0 = engine.align(p0, req, pat, txt)
    assert_same(res1, ops1, res0, ops0, True)


def test_out_of_range_windows_refused():
    from aim_amd import capi, engine
    ref = make_reference(31, 20000)
    ms, rs = engine.launcher_sizes("wfa", 100, 0.01)
    req, pat, tpos, txt = engine.ref_pairs(31, 0, 64, 100, 0.01, ref, rs)
    bad = tpos.copy()
    bad[17] = np.uint64((len(ref) - 99) | (1 << 63))
    p1 = engine.make_params("wfa", ms, rs, reduce=True, backtrace=True, ref_texts=True)
    with engine.DeviceSet(1) as s:
        s.configure_slots(p1, 64, slots=2, max_raw=64, max_runs=8 * 64)
        s.set_reference(ref)
        with pytest.raises(capi.AimError) as e:
            s.push(0, req, pat, text_pos=bad)
        assert e.value.code == capi.AIM_EINVAL and "pair 17" in str(e.value)
        with pytest.raises(capi.AimError) as e:
            s.submit(0, 1, req, packed=engine.pack_batch(req, pat, None), cigar_runs_cap=8 * 64, text_pos=bad)
        assert e.value.code == capi.AIM_EINVAL and "pair 17" in str(e.value)
        with pytest.raises(capi.AimError) as e:                 # nothing is in flight on the slot
            s.wait(0, 1)
        assert e.value.code == capi.AIM_ESTATE
        s.submit(0, 1, req, packed=engine.pack_batch(req, pat, None), cigar_runs_cap=8 * 64, text_pos=tpos)
        out = s.wait(0, 1)
    p0 = engine.make_params("wfa", ms, rs, reduce=True, backtrace=True)
    res0, ops0 = engine.align(p0, req, pat, txt)
    assert engine.format_output_runs(out["cig"], out["runs"]) == engine.format_output(res0, ops0, True)
