"""AIM_FLAG_TOP_HITS without a GPU: the ABI values and layouts, aim_hits_offsets, the refusals by message, the feature bit, the plan
line and scratch accounting (unchanged without the flag), the ranking model against a brute-force sort -- candidates that are not OK
included, which the score-only pass cannot produce on the GPU -- and the new kernel's code object."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aim_hip.h")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def _lib():
    from aim_amd import capi
    return capi.load()


def _err():
    return _lib().aim_last_error().decode()


def _define(name):
    m = re.search(r"#define\s+%s\s+(\S+)" % name, open(HEADER).read())
    return int(m.group(1).rstrip("uUlL"), 0)


def test_constants_and_feature_bit():
    from aim_amd import capi, engine
    assert _define("AIM_FLAG_TOP_HITS") == capi.FLAG_TOP_HITS == 0x8000
    assert _define("AIM_FEATURE_TOP_HITS") == capi.FEATURE_TOP_HITS == 0x400
    assert _define("AIM_TOP_HITS_MAX") == capi.TOP_HITS_MAX == 8
    assert engine.features() & capi.FEATURE_TOP_HITS
    p = engine.make_params("wfa", 5, 112, read_groups=True, top_hits=True, reduce=True, backtrace=True)
    assert p.flags == capi.FLAG_TOP_HITS | capi.FLAG_READ_GROUPS | capi.FLAG_REDUCE | capi.FLAG_BACKTRACE
    assert not engine.make_params("wfa", 5, 112, read_groups=True).flags & capi.FLAG_TOP_HITS
    for kw in (dict(), dict(read_groups=True, ref_texts=True, mate_pairs=True), dict(read_groups=True, ref_texts=True, backtrace=True, sam=True)):
        with pytest.raises(ValueError):
            engine.make_params("wfa", 5, 112, top_hits=True, **kw)


def test_struct_layout(tmp_path):
    """aim_batch_io_hits_t as ctypes and as a C compiler lay it out."""
    from aim_amd import capi
    h = capi.BatchIOHits
    assert h.sam.offset == 0 and C.sizeof(capi.BatchIOSam) == 224
    assert (h.max_hits.offset, h.pad.offset, h.hit_offsets.offset, h.hit_pair.offset, C.sizeof(h)) == (224, 228, 232, 240, 248)
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "aim_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", sizeof(aim_batch_io_sam_t), offsetof(aim_batch_io_hits_t, sam),\n'
                   'offsetof(aim_batch_io_hits_t, max_hits), offsetof(aim_batch_io_hits_t, pad), offsetof(aim_batch_io_hits_t, hit_offsets),\n'
                   'offsetof(aim_batch_io_hits_t, hit_pair), sizeof(aim_batch_io_hits_t)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["224", "0", "224", "228", "232", "240", "248"]


def _offsets(read_offsets, max_hits):
    from aim_amd import capi
    ro = np.ascontiguousarray(read_offsets, dtype=np.uint32)
    ho = np.full(len(ro), 0xDEADBEEF, dtype=np.uint32)
    n = C.c_uint32(0xFFFFFFFF)
    rc = _lib().aim_hits_offsets(len(ro) - 1, capi.ptr(ro), max_hits, capi.ptr(ho), C.byref(n))
    return rc, ho, n.value


def test_hits_offsets_against_the_model():
    import top_hits_model as m
    from aim_amd import capi, engine
    rng = np.random.default_rng(5)
    for max_hits in range(1, 9):
        sizes = np.concatenate([[max_hits, max_hits + 1, max(1, max_hits - 1), 1, 5000], rng.integers(1, 2 * max_hits + 2, size=300)])
        ro = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
        rc, ho, n = _offsets(ro, max_hits)
        want = m.hit_offsets(ro, max_hits)
        assert rc == capi.AIM_OK and np.array_equal(ho, want) and n == int(want[-1])
        assert np.array_equal(engine.hits_offsets(ro, max_hits), want)
        assert (np.diff(want) == np.minimum(sizes, max_hits)).all() and n <= int(ro[-1])
    assert _offsets([0, 3, 4, 10], 1)[1].tolist() == [0, 1, 2, 3]              # max_hits = 1: one row per read
    assert _offsets([0, 3, 4, 10], 4)[1].tolist() == [0, 3, 4, 8]
    rc, ho, n = _offsets([0], 3)                                               # no reads
    assert rc == capi.AIM_OK and ho.tolist() == [0] and n == 0
    for bad in (0, 9, 0xFFFFFFFF):
        rc, _, _ = _offsets([0, 3, 4, 10], bad)
        assert rc == capi.AIM_EINVAL and "AIM_FLAG_TOP_HITS: max_hits %d is outside 1..8" % bad in _err()
    assert _lib().aim_hits_offsets(1, None, 2, None, None) == capi.AIM_EINVAL and "AIM_FLAG_TOP_HITS" in _err()


def _describe(params, n):
    from aim_amd import capi
    b = C.create_string_buffer(1024)
    rc = _lib().aim_plan_describe(capi.params_ref(params), n, b, 1024)
    return rc, b.value.decode()


def test_the_flag_needs_read_groups_and_refuses_mates_and_sam():
    from aim_amd import capi
    lib = _lib()
    hargs = (None, None, None, None, None, 0, None, None, None, None, 2, None, 2, None, None, 0, None)
    G, R, M, S, B = capi.FLAG_READ_GROUPS, capi.FLAG_REF_TEXTS, capi.FLAG_MATE_PAIRS, capi.FLAG_SAM_FIELDS, capi.FLAG_BACKTRACE
    for flags, msg in ((0, "AIM_FLAG_TOP_HITS needs AIM_FLAG_READ_GROUPS"), (R | B, "AIM_FLAG_TOP_HITS needs AIM_FLAG_READ_GROUPS"),
                       (G | R | M, "AIM_FLAG_TOP_HITS cannot be combined with AIM_FLAG_MATE_PAIRS (a follow-up)"),
                       (G | R | B | S, "AIM_FLAG_TOP_HITS cannot be combined with AIM_FLAG_SAM_FIELDS (a follow-up: aim_sam_device works on hit rows "
                                       "with d_sel = d_hit_pair)")):
        p = capi.Params(capi.ALGO_WFA, 0, 3, 4, 1, 4, 4, 5, 112, capi.FLAG_TOP_HITS | flags)
        rc, _ = _describe(p, 64)
        assert rc == capi.AIM_EINVAL and _err() == msg, _err()
        assert lib.aim_scratch_bytes(capi.params_ref(p), 64) == 0
        assert lib.aim_kernel_name(capi.params_ref(p)) == b""
        rc = lib.aim_align_device_hits(capi.params_ref(p), 4, 2, *hargs)
        assert rc == capi.AIM_EINVAL and _err() == msg, _err()


def test_refusals_without_a_device():
    from aim_amd import capi, engine
    lib = _lib()
    ph = engine.make_params("wfa", 5, 112, read_groups=True, top_hits=True)
    phr = engine.make_params("wfa", 5, 112, read_groups=True, ref_texts=True, top_hits=True)
    pg = engine.make_params("wfa", 5, 112, read_groups=True)
    gargs = (None, None, None, None, None, 0, None, None, None, None, None, 0, None)
    rc = lib.aim_align_device_groups(capi.params_ref(ph), 4, 2, *gargs)
    assert rc == capi.AIM_EINVAL and _err() == "AIM_FLAG_TOP_HITS is set: use aim_align_device_hits"
    # every entry point that refuses AIM_FLAG_READ_GROUPS refuses the flag (it needs AIM_FLAG_READ_GROUPS)
    rc = lib.aim_align_device(capi.params_ref(ph), 1, None, None, None, None, None, None, 0, None)
    assert rc == capi.AIM_EINVAL and "AIM_FLAG_READ_GROUPS is set" in _err()
    rc = lib.aim_align_device_ref(capi.params_ref(phr), 1, None, None, None, None, 0, None, None, None, 0, None)
    assert rc == capi.AIM_EINVAL and "AIM_FLAG_READ_GROUPS is set" in _err()
    rc = lib.aim_align_device_mates(capi.params_ref(phr), 4, 2, None, None, None, None, None, 0, None, None, None, None, 0, 10, 0, None, None, 0, None)
    assert rc == capi.AIM_EINVAL and "needs AIM_FLAG_MATE_PAIRS" in _err()
    hargs = lambda max_hits, n_hits, hoff=None: (None, None, None, None, None, 0, None, None, None, None, max_hits, hoff, n_hits, None, None, 0, None)
    rc = lib.aim_align_device_hits(capi.params_ref(pg), 4, 2, *hargs(2, 3))
    assert rc == capi.AIM_EINVAL and _err() == "aim_align_device_hits needs AIM_FLAG_TOP_HITS"
    for bad in (0, 9):
        rc = lib.aim_align_device_hits(capi.params_ref(ph), 4, 2, *hargs(bad, 3))
        assert rc == capi.AIM_EINVAL and "AIM_FLAG_TOP_HITS: max_hits %d is outside 1..8" % bad in _err()
    for n_hits in (5, 1):                                            # more hits than candidates, fewer than reads
        rc = lib.aim_align_device_hits(capi.params_ref(ph), 4, 2, *hargs(2, n_hits))
        assert rc == capi.AIM_EINVAL and "AIM_FLAG_TOP_HITS: n_hits %d does not fit" % n_hits in _err()
    rc = lib.aim_align_device_hits(capi.params_ref(ph), 4, 2, *hargs(2, 3))
    assert rc == capi.AIM_EINVAL and "AIM_FLAG_TOP_HITS: null d_hit_offsets" in _err()
    rc = lib.aim_align_device_hits(capi.params_ref(ph), 4, 2, *hargs(2, 3, C.c_void_p(64)))
    assert rc == capi.AIM_EINVAL and "null device buffer" in _err()


def test_refusals_in_the_library_source():
    """The messages of the refusal that needs a configured set (checked on the GPU where a device exists)."""
    src = open(os.path.join(ROOT, "aim_amd", "csrc", "capi_groups.hip")).read()
    for msg in ("AIM_FLAG_TOP_HITS: hit_offsets[%u] = %u, but the hits of read %u start at row %u (aim_hits_offsets)",
                "AIM_FLAG_TOP_HITS: hit_offsets[%u] = %u, but the hits of read %u end at row %u (aim_hits_offsets)",
                "AIM_FLAG_TOP_HITS: null hit_offsets"):
        assert msg in src


def _configs():
    from aim_amd import engine
    out = []
    for algo, l, e, kw in (("nw", 100, 0.02, dict(backtrace=True)), ("swg", 100, 0.02, dict()), ("swg", 100, 0.02, dict(backtrace=True, swg_w16=True)),
                           ("wfa", 100, 0.01, dict(reduce=True, res8=True)), ("wfa", 100, 0.01, dict(reduce=True, backtrace=True, req8=True)),
                           ("wfa", 100, 0.01, dict(backtrace=True)), ("wfa", 1000, 0.05, dict(backtrace=True)),
                           ("wfa", 300, 0.02, dict(ends_free=(0, 0, 8, 8), backtrace=True))):
        ms, rs = engine.launcher_sizes(algo, l, e)
        out.append((algo, ms, rs, kw))
    return out


def _al(x):
    return (x + 255) // 256 * 256


@pytest.mark.parametrize("n", [1, 4096, 65536])
@pytest.mark.parametrize("ref", [False, True])
def test_plan_line_and_scratch(n, ref):
    """The plan line is READ_GROUPS' with " hits=1" appended; the scratch is READ_GROUPS' plus the hit list, 4 bytes per candidate
    rounded up to 256. Planning with the flag in between leaves the flag-less and the READ_GROUPS-only answers as they were."""
    from aim_amd import capi, engine
    lib = _lib()
    for algo, ms, rs, kw in _configs():
        p0 = engine.make_params(algo, ms, rs, ref_texts=ref, **kw)
        pg = engine.make_params(algo, ms, rs, read_groups=True, ref_texts=ref, **kw)
        ph = engine.make_params(algo, ms, rs, read_groups=True, ref_texts=ref, top_hits=True, **kw)
        before = [_describe(p0, n), lib.aim_scratch_bytes(capi.params_ref(p0), n), _describe(pg, n), lib.aim_scratch_bytes(capi.params_ref(pg), n)]
        assert before[0][0] == 0 and before[2][0] == 0 and before[1] > 0 and before[3] > 0
        rc, line = _describe(ph, n)
        assert rc == 0 and line.endswith(" groups=1 hits=1") and line == before[2][1] + " hits=1", line
        assert lib.aim_scratch_bytes(capi.params_ref(ph), n) == before[3] + _al(4 * n)
        assert lib.aim_kernel_name(capi.params_ref(ph)) == lib.aim_kernel_name(capi.params_ref(pg))
        after = [_describe(p0, n), lib.aim_scratch_bytes(capi.params_ref(p0), n), _describe(pg, n), lib.aim_scratch_bytes(capi.params_ref(pg), n)]
        assert after == before
        assert "hits" not in before[0][1] and "hits" not in before[2][1]


def _brute(scores, ok, offsets, max_hits):
    out = []
    for r in range(len(offsets) - 1):
        cands = list(range(int(offsets[r]), int(offsets[r + 1])))
        good = sorted((int(scores[i]), i) for i in cands if ok[i])       # (score, index) ascending
        order = [i for _, i in good] + [i for i in cands if not ok[i]]   # ... then the others by index
        out.append(order[:max_hits])
    return out


@pytest.mark.parametrize("seed", range(6))
def test_model_against_brute_force(seed):
    import read_groups_model as g
    import top_hits_model as m
    from aim_amd import capi
    rng = np.random.default_rng(seed)
    sizes = rng.integers(1, [2, 5, 70, 200, 12, 65][seed], size=300)
    offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    n = int(offsets[-1])
    scores = rng.integers([0, 0, 0, 0, -3, 0][seed], [3, 8, 40, 5, 2, 10][seed], size=n)     # narrow ranges: many exact ties
    status = np.where(rng.random(n) < [0.15, 0.15, 0.15, 0.5, 0.9, 0.0][seed], capi.PAIR_SWG_NO_OP, capi.PAIR_OK)
    scores = np.where(status != capi.PAIR_OK, rng.integers(-50, 50, size=n), scores)           # a score that must not count
    _, sel = g.select(scores, status, offsets)
    for max_hits in (1, 2, 3, 8):
        hoff, hit_pair = m.rank(scores, status, offsets, max_hits)
        want = _brute(scores, status == capi.PAIR_OK, offsets, max_hits)
        assert np.array_equal(hoff, m.hit_offsets(offsets, max_hits))
        for r, w in enumerate(want):
            assert hit_pair[int(hoff[r]):int(hoff[r + 1])].tolist() == w, (r, max_hits)
        assert np.array_equal(hit_pair[hoff[:-1]], sel)                  # rank 0 is AIM_FLAG_READ_GROUPS' sel
        if max_hits == 1:
            assert np.array_equal(hit_pair, sel)
    if seed != 5:
        assert (status != capi.PAIR_OK).any()


def test_hit_select_kernel_code_object():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_regs
    lib = os.path.join(ROOT, "aim_amd", "libaim_hip.so")
    if not os.path.exists(lib):
        pytest.fail("libaim_hip.so is missing: run the build")
    regs = codeobj_regs.kernel_regs(lib)
    names = [k for k in regs if "aim::hit_select_kernel" in k]
    assert len(names) == 1, names
    r = regs[names[0]]
    assert r["scratch_bytes"] == 0 and r["lds_static_bytes"] == 0, r
    assert 0 < r["vgpr"] <= 64, r
