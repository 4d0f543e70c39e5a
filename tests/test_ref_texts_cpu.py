"""AIM_FLAG_REF_TEXTS without a GPU: the ABI values and layouts, the scratch and plan-line accounting, aim_ref_windows_check,
the refusals, aim_pack_batch over patterns only, the window model against ref_pairs' explicit texts, and the gather kernels'
code object (no scratch, no LDS)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aim_hip.h")


def _lib():
    from aim_amd import capi
    return capi.load()


def _define(name):
    m = re.search(r"#define\s+%s\s+(\S+)" % name, open(HEADER).read())
    return int(m.group(1).rstrip("uUlL"), 0)


def test_feature_bit_and_flag_values():
    from aim_amd import capi, engine
    assert _define("AIM_FEATURE_REF_TEXTS") == capi.FEATURE_REF_TEXTS == 0x20
    assert _define("AIM_FLAG_REF_TEXTS") == capi.FLAG_REF_TEXTS == 0x400
    assert engine.features() & capi.FEATURE_REF_TEXTS
    assert engine.make_params("wfa", 5, 112, ref_texts=True).flags == capi.FLAG_REF_TEXTS
    assert capi.REF_MINUS_STRAND == 1 << 63


def test_struct_layouts():
    from aim_amd import capi
    assert capi.REQUEST_DTYPE.itemsize == 16 and capi.REQUEST_DTYPE.names == ("pattern_len", "text_len", "padding", "idx")
    assert C.sizeof(capi.BatchIO) == 120
    assert C.sizeof(capi.BatchIORef) == C.sizeof(capi.BatchIO) + 8
    assert capi.BatchIORef.text_pos.offset == C.sizeof(capi.BatchIO)
    src = open(HEADER).read()
    assert re.search(r"typedef struct aim_batch_io_ref \{\s*aim_batch_io_t base;[^}]*const uint64_t \*text_pos;[^}]*\} aim_batch_io_ref_t;", src)


def _configs():
    from aim_amd import engine
    out = []
    for algo, l, e, kw in (("nw", 100, 0.02, dict(backtrace=True)), ("swg", 100, 0.02, dict()), ("swg", 1000, 0.02, dict(swg_w16=True)),
                           ("wfa", 100, 0.01, dict(reduce=True)), ("wfa", 100, 0.01, dict(backtrace=True, req8=True)),
                           ("wfa", 1000, 0.05, dict(backtrace=True)), ("wfa", 300, 0.02, dict(ends_free=(0, 0, 8, 8))),
                           ("wfa", 300, 0.02, dict(gap2=(24, 1))), ("wfa", 300, 0.02, dict(linear=True)),
                           ("wfa", 1000, 0.02, dict(w32=True)), ("wfa", 1000, 0.05, dict(backtrace=True, bidir=True))):
        ms, rs = engine.launcher_sizes(algo, l, e)
        out.append((engine.make_params(algo, ms, rs, **kw), engine.make_params(algo, ms, rs, ref_texts=True, **kw)))
    out.append((engine.make_params("genasm", 0, 1 << 16, backtrace=True), engine.make_params("genasm", 0, 1 << 16, backtrace=True, ref_texts=True)))
    return out


@pytest.mark.parametrize("n", [1, 1000, 65536])
def test_scratch_bytes_include_the_text_rows(n):
    from aim_amd import capi
    lib = _lib()
    for p0, p1 in _configs():
        s0 = lib.aim_scratch_bytes(capi.params_ref(p0), n)
        s1 = lib.aim_scratch_bytes(capi.params_ref(p1), n)
        assert s0 > 0
        assert s1 == ((s0 + 255) // 256) * 256 + n * p0.read_size + 256, (p0.algo, p0.flags)


def test_plan_line_suffix():
    from aim_amd import capi
    lib = _lib()
    for p0, p1 in _configs():
        b0, b1 = C.create_string_buffer(512), C.create_string_buffer(512)
        capi.check(lib.aim_plan_describe(capi.params_ref(p0), 4096, b0, 512))
        capi.check(lib.aim_plan_describe(capi.params_ref(p1), 4096, b1, 512))
        assert b1.value.decode() == b0.value.decode() + " ref=1"
        assert lib.aim_kernel_name(capi.params_ref(p1)) == lib.aim_kernel_name(capi.params_ref(p0))


def _check(params, req, tpos, ref_len):
    from aim_amd import capi
    bad = C.c_uint32(0xFFFFFFFF)
    rc = _lib().aim_ref_windows_check(capi.params_ref(params), len(req), capi.ptr(req), capi.ptr(tpos), ref_len, C.byref(bad))
    return rc, bad.value


@pytest.mark.parametrize("req8", [False, True])
def test_windows_check(req8):
    from aim_amd import capi, engine
    p = engine.make_params("wfa", 5, 112, ref_texts=True, req8=req8)
    req = np.zeros(6, dtype=capi.REQUEST_DTYPE)
    req["pattern_len"], req["text_len"], req["idx"] = 100, [100, 100, 100, 0, 50, 100], np.arange(6)
    if req8:
        req = engine.to_request8(req)
    ref_len = 1000
    m = np.uint64(1 << 63)
    tpos = np.array([0, 900, 900 | (1 << 63), 1000, 950, 123 | (1 << 63)], dtype=np.uint64)   # ends exactly at ref_len; empty window at the end
    assert _check(p, req, tpos, ref_len) == (capi.AIM_OK, 0xFFFFFFFF)
    t = tpos.copy(); t[4] = 951                                    # 951 + 50 > 1000
    assert _check(p, req, t, ref_len) == (capi.AIM_EINVAL, 4)
    assert "pair 4" in _lib().aim_last_error().decode()
    t = tpos.copy(); t[2] = np.uint64(901) | m; t[5] = 10 ** 9     # the first bad pair is named; bit 63 is the strand, not the position
    assert _check(p, req, t, ref_len) == (capi.AIM_EINVAL, 2)
    t = tpos.copy(); t[1] = m | np.uint64(900)                     # strand bit alone never makes a window bad
    assert _check(p, req, t, ref_len)[0] == capi.AIM_OK
    t = tpos.copy(); t[3] = np.uint64(1 << 62)                    # text_len 0: nothing is read, any position passes
    assert _check(p, req, t, ref_len)[0] == capi.AIM_OK
    assert _check(p, req[:0], tpos[:0], 0)[0] == capi.AIM_OK
    t = tpos.copy(); t[0] = 1                                      # 1 + 100 > ref_len 100
    assert _check(p, req, t, 100) == (capi.AIM_EINVAL, 0)
    r = req.copy(); r["text_len"][3] = 113                         # lengths against read_size first
    assert _check(p, r, tpos, ref_len) == (capi.AIM_EINVAL, 3)


def test_windows_check_large_batch_names_first_bad_pair():
    from aim_amd import capi, engine
    p = engine.make_params("nw", 5, 104, ref_texts=True)
    n = 1 << 20
    req = np.zeros(n, dtype=capi.REQUEST_DTYPE)
    req["pattern_len"], req["text_len"] = 100, 100
    tpos = (np.arange(n, dtype=np.uint64) % np.uint64(1 << 40)) | np.uint64(1 << 63)
    ref_len = (1 << 40) + 100
    assert _check(p, req, tpos, ref_len)[0] == capi.AIM_OK
    tpos[777777] = np.uint64(ref_len - 99)
    tpos[900000] = np.uint64(ref_len)
    assert _check(p, req, tpos, ref_len) == (capi.AIM_EINVAL, 777777)


def test_refusals_without_a_device():
    """Refusals that come before any device work; an unflagged call is unchanged."""
    from aim_amd import capi, engine
    lib = _lib()
    p0 = engine.make_params("wfa", 5, 112)
    p1 = engine.make_params("wfa", 5, 112, ref_texts=True)
    # aim_align_device_ref without the flag / with null device buffers
    rc = lib.aim_align_device_ref(capi.params_ref(p0), 1, None, None, None, None, 0, None, None, None, 0, None)
    assert rc == capi.AIM_EINVAL and b"needs AIM_FLAG_REF_TEXTS" in lib.aim_last_error()
    rc = lib.aim_align_device_ref(capi.params_ref(p1), 1, None, None, None, None, 0, None, None, None, 0, None)
    assert rc == capi.AIM_EINVAL and b"null device buffer" in lib.aim_last_error()
    # the set entry points: a NULL set is refused as before
    assert lib.aim_set_push_ref(None, 0, 0, None, None, None) == capi.AIM_EINVAL
    assert lib.aim_set_reference(None, None, 0) == capi.AIM_EINVAL
    # aim_pack_batch: texts NULL is refused without the flag, exactly as before
    req = np.zeros(1, dtype=capi.REQUEST_DTYPE)
    req["pattern_len"], req["text_len"] = 4, 4
    pat = np.zeros((1, 112), dtype=np.uint8)
    pat[0, :4] = np.frombuffer(b"ACGT", dtype=np.uint8)
    pp = np.zeros((1, 7), dtype=np.uint32)
    raw, rawp = np.zeros(1, dtype=np.uint32), np.zeros((1, 112), dtype=np.uint8)
    nr = C.c_uint32()
    rc = lib.aim_pack_batch(capi.params_ref(p0), 1, capi.ptr(req), capi.ptr(pat), None, capi.ptr(pp), None, capi.ptr(raw), capi.ptr(rawp),
                            None, 1, C.byref(nr), 1)
    assert rc == capi.AIM_EINVAL
    rc = lib.aim_pack_batch(capi.params_ref(p1), 1, capi.ptr(req), capi.ptr(pat), None, capi.ptr(pp), None, capi.ptr(raw), capi.ptr(rawp),
                            None, 1, C.byref(nr), 1)
    assert rc == capi.AIM_OK and nr.value == 0


def test_refusals_in_the_library_source():
    """The messages of the refusals that need a configured set (checked on the GPU where a device exists)."""
    src = open(os.path.join(ROOT, "aim_amd", "csrc", "aim_capi.hip")).read()
    for msg in ("AIM_FLAG_REF_TEXTS is set: the texts are named by text_pos (aim_set_push_ref)",
                "aim_set_push_ref needs AIM_FLAG_REF_TEXTS",
                "AIM_FLAG_REF_TEXTS: texts, packed_texts and raw_texts must be NULL (the texts are named by text_pos)",
                "text window of pair %u is outside the reference"):
        assert msg in src


@pytest.mark.parametrize("native", [False, True])
def test_pack_batch_patterns_only(native):
    from aim_amd import engine
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(5).integers(0, 4, size=20000)].copy()
    ref[5000:5010] = ord("N")
    ref[9000:9100] |= 0x20
    ms, rs = engine.launcher_sizes("wfa", 100, 0.02)
    req, pat, tpos, txt = engine.ref_pairs(5, 0, 300, 100, 0.02, ref, rs)
    pat[::15, 7] = ord("N")
    params = engine.make_params("wfa", ms, rs, ref_texts=True)
    if native:
        pp, pt, raw, rawp, rawt = engine.pack_batch_native(params, req, pat, None)
    else:
        pp, pt, raw, rawp, rawt = engine.pack_batch(req, pat, None)
    assert pt is None and rawt is None
    _, okp = engine.pack_rows(req, pat, "pattern_len")
    assert raw.tolist() == np.nonzero(~okp)[0].tolist()
    assert np.array_equal(rawp, pat[raw])
    full = engine.pack_batch(req, pat, txt)
    ok = np.setdiff1d(np.arange(len(req)), raw)              # (the packed rows of raw pairs are unspecified)
    assert np.array_equal(pp[ok], full[0][ok])
    assert set(full[2].tolist()) >= set(raw.tolist())       # explicit texts add the non-ACGT windows


def _model_window(ref, pos, length, minus):
    comp = {ord("A"): ord("T"), ord("T"): ord("A"), ord("C"): ord("G"), ord("G"): ord("C"),
            ord("a"): ord("t"), ord("t"): ord("a"), ord("c"): ord("g"), ord("g"): ord("c")}
    w = [int(b) for b in ref[pos:pos + length]]
    return bytes(comp.get(b, b) for b in reversed(w)) if minus else bytes(w)


def test_window_model_matches_ref_pairs():
    from aim_amd import engine
    rng = np.random.default_rng(3)
    ref = rng.integers(0, 256, size=20000).astype(np.uint8)        # every byte value; complement touches ACGTacgt only
    ref[:4000] = np.frombuffer(b"ACGTacgtNnRY"[:12], dtype=np.uint8)[rng.integers(0, 12, size=4000)]
    ms, rs = engine.launcher_sizes("nw", 150, 0.05)
    req, pat, tpos, txt = engine.ref_pairs(9, 100, 400, 150, 0.05, ref, rs, minus_fraction=0.4)
    minus = (tpos >> np.uint64(63)).astype(bool)
    assert 0.25 < minus.mean() < 0.55
    for i in range(len(req)):
        pos, tl = int(tpos[i]) & ((1 << 63) - 1), int(req["text_len"][i])
        assert tl == 150 and pos + tl <= len(ref)
        assert txt[i, :tl].tobytes() == _model_window(ref, pos, tl, bool(minus[i]))
        assert not txt[i, tl:].any() and not pat[i, int(req["pattern_len"][i]):].any()
        assert abs(int(req["pattern_len"][i]) - tl) <= 8
    again = engine.ref_pairs(9, 100 + 17, 5, 150, 0.05, ref, rs, minus_fraction=0.4)   # pair i depends on (seed, first_idx + i)
    assert np.array_equal(again[2], tpos[17:22]) and np.array_equal(again[1], pat[17:22])


def test_gather_code_objects_have_no_scratch_no_lds():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_regs
    lib = os.path.join(ROOT, "aim_amd", "libaim_hip.so")
    if not os.path.exists(lib):
        pytest.fail("libaim_hip.so is missing: run the build")
    regs = codeobj_regs.kernel_regs(lib)
    names = [k for k in regs if "gather_text_rows_kernel" in k or "gather_text_packed_kernel" in k or "gather_todo_rows_kernel" in k]
    assert len(names) == 4, names
    for k in names:
        assert regs[k]["scratch_bytes"] == 0 and regs[k]["lds_static_bytes"] == 0, (k, regs[k])
