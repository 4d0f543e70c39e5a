"""AIM_FLAG_READ_GROUPS without a GPU: the ABI values and layouts, aim_groups_check, the refusals, the scratch and plan-line
accounting of the two passes, the selection model against a brute-force selection, and the new kernels' code objects."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aim_hip.h")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from aim_amd import capi
    return capi.load()


def _define(name):
    m = re.search(r"#define\s+%s\s+(\S+)" % name, open(HEADER).read())
    return int(m.group(1).rstrip("uUlL"), 0)


def test_feature_bit_and_flag_values():
    from aim_amd import capi, engine
    assert _define("AIM_FEATURE_READ_GROUPS") == capi.FEATURE_READ_GROUPS == 0x40
    assert _define("AIM_FLAG_READ_GROUPS") == capi.FLAG_READ_GROUPS == 0x800
    assert engine.features() & 0x40
    assert engine.make_params("wfa", 5, 112, read_groups=True).flags == capi.FLAG_READ_GROUPS
    p = engine.make_params("wfa", 5, 112, read_groups=True, ref_texts=True, backtrace=True, req8=True)
    assert p.flags == capi.FLAG_READ_GROUPS | capi.FLAG_REF_TEXTS | capi.FLAG_BACKTRACE | capi.FLAG_REQ8
    assert engine.make_params("wfa", 5, 112, read_groups=True, ends_free=(0, 0, 4, 4)).flags == capi.FLAG_READ_GROUPS | capi.FLAG_ENDSFREE


def test_make_params_errors():
    from aim_amd import engine
    with pytest.raises(ValueError):
        engine.make_params("wfa", 5, 112, read_groups=True, bidir=True)            # bidir needs backtrace, with or without groups
    with pytest.raises(ValueError):
        engine.make_params("wfa", 5, 112, read_groups=True, linear=True, reduce=True)


def test_struct_layouts():
    from aim_amd import capi
    assert capi.BEST_DTYPE.itemsize == 16
    assert capi.BEST_DTYPE.names == ("best_pair", "best_score", "second_score", "n_best")
    assert C.sizeof(capi.BatchIO) == 120
    assert capi.BatchIOGroups.base.offset == capi.BatchIORef.base.offset == 0
    assert capi.BatchIOGroups.text_pos.offset == capi.BatchIORef.text_pos.offset == 120
    assert capi.BatchIOGroups.n_reads.offset == 128
    assert capi.BatchIOGroups.read_offsets.offset == 136 and capi.BatchIOGroups.best.offset == 144
    assert C.sizeof(capi.BatchIOGroups) == 152
    src = open(HEADER).read()
    assert re.search(r"typedef struct aim_best \{\s*uint32_t best_pair;[^;]*?int32_t best_score;\s*int32_t second_score;\s*uint32_t n_best;\s*\} aim_best_t;", src)
    assert re.search(r"typedef struct aim_batch_io_groups \{\s*aim_batch_io_t base;[^}]*const uint64_t \*text_pos;[^}]*uint32_t n_reads;[^}]*"
                     r"const uint32_t \*read_offsets;[^}]*aim_best_t \*best;[^}]*\} aim_batch_io_groups_t;", src)


def _check(n_pairs, offsets):
    from aim_amd import capi
    ro = np.ascontiguousarray(offsets, dtype=np.uint32)
    bad = C.c_uint32(0xFFFFFFFF)
    rc = _lib().aim_groups_check(n_pairs, len(ro) - 1, capi.ptr(ro) if len(ro) else None, C.byref(bad))
    return rc, bad.value


def test_groups_check():
    from aim_amd import capi
    assert _check(10, [0, 3, 4, 10]) == (capi.AIM_OK, 0xFFFFFFFF)
    assert _check(1, [0, 1]) == (capi.AIM_OK, 0xFFFFFFFF)
    assert _check(0, [0]) == (capi.AIM_OK, 0xFFFFFFFF)
    assert _check(10, [1, 3, 4, 10]) == (capi.AIM_EINVAL, 0)            # does not start at 0
    assert "read 0" in _lib().aim_last_error().decode()
    assert _check(10, [0, 3, 2, 10]) == (capi.AIM_EINVAL, 1)            # decreasing
    assert _check(10, [0, 3, 3, 10]) == (capi.AIM_EINVAL, 1)            # an empty read
    assert "read 1" in _lib().aim_last_error().decode()
    assert _check(10, [0, 3, 4, 9]) == (capi.AIM_EINVAL, 2)             # last offset != n_pairs
    assert _check(10, [0, 3, 4, 11]) == (capi.AIM_EINVAL, 2)            # ... past n_pairs
    assert _check(10, [0, 3, 3, 2, 11]) == (capi.AIM_EINVAL, 1)         # the first bad read is named
    rc, _ = _check(5, [0])                                               # candidates without a read
    assert rc == capi.AIM_EINVAL


def test_groups_check_large():
    from aim_amd import capi
    n_reads = 1 << 19
    ro = np.arange(n_reads + 1, dtype=np.uint32) * 8
    assert _check(8 * n_reads, ro)[0] == capi.AIM_OK
    ro[300001] = ro[300000]
    assert _check(8 * n_reads, ro) == (capi.AIM_EINVAL, 300000)


def test_refusals_without_a_device():
    from aim_amd import capi, engine
    lib = _lib()
    p0 = engine.make_params("wfa", 5, 112)
    p1 = engine.make_params("wfa", 5, 112, read_groups=True)
    p1r = engine.make_params("wfa", 5, 112, read_groups=True, ref_texts=True)
    args = (None, None, None, None, None, 0, None, None, None, None, None, 0, None)
    rc = lib.aim_align_device_groups(capi.params_ref(p0), 4, 2, *args)
    assert rc == capi.AIM_EINVAL and b"needs AIM_FLAG_READ_GROUPS" in lib.aim_last_error()
    rc = lib.aim_align_device_groups(capi.params_ref(p1), 4, 2, *args)
    assert rc == capi.AIM_EINVAL and b"null device buffer" in lib.aim_last_error()
    rc = lib.aim_align_device_groups(capi.params_ref(p1), 4, 5, *args)
    assert rc == capi.AIM_EINVAL and b"does not fit" in lib.aim_last_error()
    rc = lib.aim_align_device(capi.params_ref(p1), 1, None, None, None, None, None, None, 0, None)
    assert rc == capi.AIM_EINVAL and b"aim_align_device_groups" in lib.aim_last_error()
    rc = lib.aim_align_device_ref(capi.params_ref(p1r), 1, None, None, None, None, 0, None, None, None, 0, None)
    assert rc == capi.AIM_EINVAL and b"aim_align_device_groups" in lib.aim_last_error()


def test_refusals_in_the_library_source():
    """The messages of the refusals that need a configured set (checked on the GPU where a device exists)."""
    src = open(os.path.join(ROOT, "aim_amd", "csrc", "aim_capi.hip")).read()        # push / launch / pull refuse a groups set here
    groups = open(os.path.join(ROOT, "aim_amd", "csrc", "capi_groups.hip")).read()  # ... and submit_groups refuses its batches here
    assert "AIM_FLAG_READ_GROUPS is set: batches go through aim_set_submit with an aim_batch_io_groups_t" in src
    assert "AIM_FLAG_READ_GROUPS: packed batches need AIM_FLAG_REF_TEXTS (packed explicit texts are a follow-up)" in groups
    assert src.count("kGroupsSubmitOnly") == 4      # the definition, aim_set_push(_ref), aim_set_launch, aim_set_pull


def _al(x):
    return (x + 255) // 256 * 256


def _configs():
    from aim_amd import engine
    out = []
    for algo, l, e, kw in (("nw", 100, 0.02, dict(backtrace=True)), ("swg", 100, 0.02, dict()), ("swg", 100, 0.02, dict(backtrace=True)),
                           ("wfa", 100, 0.01, dict(reduce=True, res8=True)), ("wfa", 100, 0.01, dict(reduce=True, backtrace=True, req8=True)),
                           ("wfa", 1000, 0.05, dict(backtrace=True)), ("wfa", 300, 0.02, dict(ends_free=(0, 0, 8, 8), backtrace=True)),
                           ("wfa", 300, 0.02, dict(gap2=(24, 1))), ("wfa", 300, 0.02, dict(linear=True, backtrace=True)),
                           ("wfa", 1000, 0.02, dict(w32=True)), ("wfa", 1000, 0.05, dict(backtrace=True, bidir=True))):
        ms, rs = engine.launcher_sizes(algo, l, e)
        out.append((algo, ms, rs, kw))
    out.append(("genasm", 0, 1 << 12, dict(backtrace=True)))
    return out


def _pass_kw(kw):
    return {k: v for k, v in kw.items() if k not in ("backtrace", "bidir", "res8")}


@pytest.mark.parametrize("n", [1, 1000, 65536])
@pytest.mark.parametrize("ref", [False, True])
def test_scratch_bytes(n, ref):
    from aim_amd import capi, engine
    lib = _lib()
    for algo, ms, rs, kw in _configs():
        s1 = lib.aim_scratch_bytes(capi.params_ref(engine.make_params(algo, ms, rs, **_pass_kw(kw))), n)
        bt = kw.get("backtrace", False)
        s2 = lib.aim_scratch_bytes(capi.params_ref(engine.make_params(algo, ms, rs, **kw)), n) if bt else 0
        assert s1 > 0
        rows = _al(n * rs + 256)
        want = _al(max(s1, s2)) + rows * (2 if ref else 1) + _al(24 * n) + 2 * _al(4 * n)
        if bt:
            want += _al(16 * n) + 2 * rows
        got = lib.aim_scratch_bytes(capi.params_ref(engine.make_params(algo, ms, rs, read_groups=True, ref_texts=ref, **kw)), n)
        assert got == want, (algo, kw, got, want)


def _describe(params, n):
    from aim_amd import capi
    b = C.create_string_buffer(1024)
    capi.check(_lib().aim_plan_describe(capi.params_ref(params), n, b, 1024))
    return b.value.decode()


def test_plan_line():
    from aim_amd import capi, engine
    for algo, ms, rs, kw in _configs():
        pg = engine.make_params(algo, ms, rs, read_groups=True, **kw)
        line = _describe(pg, 4096)
        first = _describe(engine.make_params(algo, ms, rs, **_pass_kw(kw)), 4096)
        second = _describe(engine.make_params(algo, ms, rs, **kw), 4096) if kw.get("backtrace") else "no second pass n=4096"
        assert line == first + " | " + second + " groups=1", line
        assert line.endswith(" groups=1")
        assert _lib().aim_kernel_name(capi.params_ref(pg)) == _lib().aim_kernel_name(capi.params_ref(engine.make_params(algo, ms, rs, **_pass_kw(kw))))


def test_plan_debug_prints_the_same_line():
    import subprocess
    code = ("import sys, ctypes as C; sys.path.insert(0, %r)\n"
            "from aim_amd import capi, engine\n"
            "p = engine.make_params('wfa', 5, 112, read_groups=True, reduce=True, backtrace=True)\n"
            "b = C.create_string_buffer(1024); capi.check(capi.load().aim_plan_describe(capi.params_ref(p), 777, b, 1024))\n"
            "print(b.value.decode())\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, AIM_PLAN_DEBUG="1"), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "[aim plan] " + r.stdout.strip() in r.stderr


def _brute(scores, ok, offsets):
    out = []
    for r in range(len(offsets) - 1):
        cands = [(int(scores[i]), i) for i in range(offsets[r], offsets[r + 1]) if ok[i]]
        if not cands:
            out.append((2 ** 32 - 1, 2 ** 31 - 1, 2 ** 31 - 1, 0, offsets[r]))
            continue
        b = min(cands)                                             # lowest score, then lowest index
        rest = [s for s, i in cands if i != b[1]]
        out.append((b[1], b[0], min(rest) if rest else 2 ** 31 - 1, sum(1 for s, _ in cands if s == b[0]), b[1]))
    return out


@pytest.mark.parametrize("seed", range(6))
def test_model_against_brute_force(seed):
    import read_groups_model as m
    from aim_amd import capi
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, [2, 5, 70, 200, 3, 65][seed], size=300)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    n = int(offsets[-1])
    scores = rng.integers(0, [3, 8, 40, 5, 2, 10][seed], size=n)        # narrow ranges: many exact ties
    status = np.where(rng.random(n) < 0.15, capi.PAIR_SWG_NO_OP, capi.PAIR_OK)
    best, sel = m.select(scores, status, offsets)
    want = _brute(scores, status == capi.PAIR_OK, offsets)
    for r, w in enumerate(want):
        assert tuple(int(x) for x in best[r]) == w[:4], (r, best[r], w)
        assert int(sel[r]) == w[4]
    assert (best["n_best"] >= 2).any() and (best["n_best"] == 0).any() or seed in (0, 4)


def test_group_pairs_model():
    from aim_amd import engine
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(2).integers(0, 4, size=30000)].copy()
    ms, rs = engine.launcher_sizes("wfa", 100, 0.02)
    req, rows, offs, tpos, txt, pats = engine.group_pairs(3, 10, 50, 6, 100, 0.02, ref, rs)
    assert len(req) == 300 and offs.tolist() == list(range(0, 301, 6))
    for i in range(len(req)):
        r = i // 6
        assert np.array_equal(pats[i], rows[r]) and int(req["pattern_len"][i]) == int(np.count_nonzero(rows[r]))
        pos, minus = int(tpos[i]) & ((1 << 63) - 1), bool(int(tpos[i]) >> 63)
        assert np.array_equal(txt[i, :100], engine.ref_window(ref, pos, 100, minus)) and not txt[i, 100:].any()
    again = engine.group_pairs(3, 12, 3, 6, 100, 0.02, ref, rs)                    # read r depends on (seed, first_read + r)
    assert np.array_equal(again[1], rows[2:5]) and np.array_equal(again[3], tpos[12:30])
    _, _, offs2, _, _, _ = engine.group_pairs(1, 0, 4, 0, 100, 0.0, ref, rs, sizes=[1, 65, 3, 1])
    assert offs2.tolist() == [0, 1, 66, 69, 70]


def test_new_kernels_code_objects():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_regs
    lib = os.path.join(ROOT, "aim_amd", "libaim_hip.so")
    if not os.path.exists(lib):
        pytest.fail("libaim_hip.so is missing: run the build")
    regs = codeobj_regs.kernel_regs(lib)
    names = [k for k in regs if re.search(r"aim::group_(map|rows|select|results|raw_slot|unpack)_kernel", k)]
    assert len(names) == 7, names
    for k in names:
        assert regs[k]["scratch_bytes"] == 0 and regs[k]["lds_static_bytes"] == 0, (k, regs[k])
    sel = [k for k in names if "group_select_kernel" in k][0]
    assert 0 < regs[sel]["vgpr"] <= 64, regs[sel]
