"""AIM_FLAG_MATE_PAIRS without a GPU: the ABI values and layouts, aim_mates_check, the refusals, the plan line and scratch accounting,
the Python binding, the selection kernel's code object, the model against hand-made cases, and the generator scored by the CPU oracle
(all three outcomes occur: proper and equal to the independent winners, proper but different -- a repeat resolved by the mate -- and
the unpaired fallback)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aim_hip.h")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

INT32_MAX = 2 ** 31 - 1
UINT32_MAX = 2 ** 32 - 1
MINUS = 1 << 63


def _lib():
    from aim_amd import capi
    return capi.load()


def _define(name):
    m = re.search(r"#define\s+%s\s+(\S+)" % name, open(HEADER).read())
    return int(m.group(1).rstrip("uUlL"), 0)


def _err():
    return _lib().aim_last_error().decode()


def test_feature_bit_and_flag_values():
    from aim_amd import capi, engine
    assert _define("AIM_FLAG_MATE_PAIRS") == capi.FLAG_MATE_PAIRS == 0x2000
    assert _define("AIM_FEATURE_MATE_PAIRS") == capi.FEATURE_MATE_PAIRS == 0x100
    assert _define("AIM_MATE_PROPER") == capi.MATE_PROPER == 1
    assert engine.features() & 0x100
    assert _lib().aim_abi_version() == 2


def test_struct_layouts():
    from aim_amd import capi
    assert C.sizeof(capi.BatchIOGroups) == 152
    assert capi.BatchIOMates.groups.offset == 0
    assert [getattr(capi.BatchIOMates, f).offset for f in ("min_span", "max_span", "unpaired_penalty", "pad", "mates")] == [152, 160, 168, 172, 176]
    assert C.sizeof(capi.BatchIOMates) == 184
    assert capi.MATE_DTYPE.itemsize == 32
    assert capi.MATE_DTYPE.names == ("best_pair", "score_sum", "second_sum", "n_best", "flags", "pad")
    assert [capi.MATE_DTYPE.fields[k][1] for k in capi.MATE_DTYPE.names] == [0, 8, 12, 16, 20, 24]
    src = open(HEADER).read()
    assert re.search(r"typedef struct aim_mate \{[^}]*uint32_t best_pair\[2\];[^}]*int32_t\s+score_sum;[^}]*int32_t\s+second_sum;[^}]*uint32_t n_best;"
                     r"[^}]*uint32_t flags;[^}]*uint32_t pad\[2\];[^}]*\} aim_mate_t;", src)
    assert re.search(r"typedef struct aim_batch_io_mates \{\s*aim_batch_io_groups_t groups;[^}]*int64_t\s+min_span, max_span;[^}]*"
                     r"int32_t\s+unpaired_penalty;[^}]*uint32_t pad;[^}]*aim_mate_t \*mates;[^}]*\} aim_batch_io_mates_t;", src)


def test_header_layout_by_the_c_compiler(tmp_path):
    """sizeof / offsetof as a C compiler lays the header out."""
    import subprocess
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "aim_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(aim_batch_io_groups_t), sizeof(aim_mate_t),\n'
                   'offsetof(aim_batch_io_mates_t, min_span), offsetof(aim_batch_io_mates_t, max_span),\n'
                   'offsetof(aim_batch_io_mates_t, unpaired_penalty), offsetof(aim_batch_io_mates_t, pad), offsetof(aim_batch_io_mates_t, mates),\n'
                   'sizeof(aim_batch_io_mates_t)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["152", "32", "152", "160", "168", "172", "176", "184"]


def test_mates_check():
    from aim_amd import capi
    lib = _lib()
    assert lib.aim_mates_check(0, 0, 0, 0) == capi.AIM_OK
    assert lib.aim_mates_check(10, 100, 100, 0) == capi.AIM_OK
    assert lib.aim_mates_check(2, 0, (1 << 62) - 1, INT32_MAX) == capi.AIM_OK
    assert lib.aim_mates_check(7, 100, 500, 5) == capi.AIM_EINVAL
    assert "n_reads 7 is odd" in _err()
    assert lib.aim_mates_check(8, 501, 500, 5) == capi.AIM_EINVAL
    assert "bad span [501, 500]" in _err() and "0 <= min_span <= max_span < 2^62" in _err()
    assert lib.aim_mates_check(8, -1, 500, 5) == capi.AIM_EINVAL and "bad span" in _err()
    assert lib.aim_mates_check(8, 0, 1 << 62, 5) == capi.AIM_EINVAL and "bad span" in _err()
    assert lib.aim_mates_check(8, 100, 500, -1) == capi.AIM_EINVAL
    assert "unpaired_penalty -1 is negative" in _err()


def test_make_params():
    from aim_amd import capi, engine
    p = engine.make_params("wfa", 5, 112, read_groups=True, ref_texts=True, mate_pairs=True, reduce=True, backtrace=True, req8=True)
    assert p.flags == (capi.FLAG_MATE_PAIRS | capi.FLAG_READ_GROUPS | capi.FLAG_REF_TEXTS | capi.FLAG_REDUCE | capi.FLAG_BACKTRACE |
                       capi.FLAG_REQ8)
    assert engine.make_params("nw", 4, 112, read_groups=True, ref_texts=True, mate_pairs=True).flags == 0x2000 | 0x800 | 0x400
    for kw in (dict(), dict(read_groups=True), dict(ref_texts=True)):
        with pytest.raises(ValueError):
            engine.make_params("wfa", 5, 112, mate_pairs=True, **kw)
    assert not engine.make_params("wfa", 5, 112, read_groups=True, ref_texts=True).flags & capi.FLAG_MATE_PAIRS


def _describe(params, n):
    from aim_amd import capi
    b = C.create_string_buffer(1024)
    rc = _lib().aim_plan_describe(capi.params_ref(params), n, b, 1024)
    return rc, b.value.decode()


def test_the_flag_needs_read_groups_and_ref_texts():
    from aim_amd import capi
    lib = _lib()
    for flags, missing in ((0x2000, "AIM_FLAG_READ_GROUPS"), (0x2000 | 0x400, "AIM_FLAG_READ_GROUPS"), (0x2000 | 0x800, "AIM_FLAG_REF_TEXTS")):
        p = capi.Params(capi.ALGO_WFA, 0, 3, 4, 1, 4, 4, 5, 112, flags)
        rc, _ = _describe(p, 64)
        assert rc == capi.AIM_EINVAL and _err() == "AIM_FLAG_MATE_PAIRS needs " + missing, _err()
        assert lib.aim_scratch_bytes(capi.params_ref(p), 64) == 0
        assert lib.aim_kernel_name(capi.params_ref(p)) == b""
        rc = lib.aim_align_device_mates(capi.params_ref(p), 4, 2, None, None, None, None, None, 0, None, None, None, None, 0, 10, 0, None, None, 0, None)
        assert rc == capi.AIM_EINVAL and _err() == "AIM_FLAG_MATE_PAIRS needs " + missing
        # the flag-less entry points refuse it whichever flag is missing
        rc = lib.aim_align_device(capi.params_ref(p), 1, None, None, None, None, None, None, 0, None)
        assert rc == capi.AIM_EINVAL and ("use aim_align_device_mates" in _err() or "use aim_align_device_groups" in _err())


def test_refusals_without_a_device():
    from aim_amd import capi, engine
    lib = _lib()
    pm = engine.make_params("wfa", 5, 112, read_groups=True, ref_texts=True, mate_pairs=True)
    pg = engine.make_params("wfa", 5, 112, read_groups=True, ref_texts=True)
    gargs = (None, None, None, None, None, 0, None, None, None, None, None, 0, None)
    rc = lib.aim_align_device_groups(capi.params_ref(pm), 4, 2, *gargs)
    assert rc == capi.AIM_EINVAL and _err() == "AIM_FLAG_MATE_PAIRS is set: use aim_align_device_mates"
    rc = lib.aim_align_device(capi.params_ref(pm), 1, None, None, None, None, None, None, 0, None)
    assert rc == capi.AIM_EINVAL and "AIM_FLAG_READ_GROUPS is set" in _err()
    rc = lib.aim_align_device_ref(capi.params_ref(pm), 1, None, None, None, None, 0, None, None, None, 0, None)
    assert rc == capi.AIM_EINVAL and "AIM_FLAG_READ_GROUPS is set" in _err()
    margs = lambda n_reads, lo, hi, pen, txt=None: (None, None, txt, None, None, 0, None, None, None, None, lo, hi, pen, None, None, 0, None)
    rc = lib.aim_align_device_mates(capi.params_ref(pg), 4, 2, *margs(2, 0, 10, 0))
    assert rc == capi.AIM_EINVAL and _err() == "aim_align_device_mates needs AIM_FLAG_MATE_PAIRS"
    rc = lib.aim_align_device_mates(capi.params_ref(pm), 4, 3, *margs(3, 0, 10, 0))
    assert rc == capi.AIM_EINVAL and "n_reads 3 is odd" in _err()
    rc = lib.aim_align_device_mates(capi.params_ref(pm), 4, 2, *margs(2, 11, 10, 0))
    assert rc == capi.AIM_EINVAL and "bad span [11, 10]" in _err()
    rc = lib.aim_align_device_mates(capi.params_ref(pm), 4, 2, *margs(2, 0, 10, -3))
    assert rc == capi.AIM_EINVAL and "unpaired_penalty -3 is negative" in _err()
    rc = lib.aim_align_device_mates(capi.params_ref(pm), 4, 2, *margs(2, 0, 10, 0, txt=C.c_void_p(64)))
    assert rc == capi.AIM_EINVAL and "d_texts must be NULL" in _err()
    rc = lib.aim_align_device_mates(capi.params_ref(pm), 4, 2, *margs(2, 0, 10, 0))
    assert rc == capi.AIM_EINVAL and "null device buffer" in _err()
    rc = lib.aim_align_device_mates(capi.params_ref(pm), 4, 6, *margs(6, 0, 10, 0))
    assert rc == capi.AIM_EINVAL and "does not fit" in _err()


def _configs():
    from aim_amd import engine
    out = []
    for algo, l, e, kw in (("nw", 150, 0.02, dict(backtrace=True)), ("swg", 100, 0.02, dict()),
                           ("wfa", 100, 0.01, dict(reduce=True, res8=True)), ("wfa", 100, 0.01, dict(reduce=True, backtrace=True, req8=True)),
                           ("wfa", 100, 0.01, dict(backtrace=True)), ("wfa", 1000, 0.05, dict(backtrace=True, bidir=True)),
                           ("wfa", 300, 0.02, dict(ends_free=(0, 0, 8, 8), backtrace=True))):
        ms, rs = engine.launcher_sizes(algo, l, e)
        out.append((algo, ms, rs, kw))
    return out


def _al(x):
    return (x + 255) // 256 * 256


@pytest.mark.parametrize("n", [2, 4096, 65536])
def test_plan_line_and_scratch(n):
    """The plan line is READ_GROUPS' with " mates=1" appended; the scratch is READ_GROUPS' plus the aim_best_t copy. Planning with the
    flag in between leaves the flag-less and the READ_GROUPS-only answers as they were."""
    from aim_amd import capi, engine
    lib = _lib()
    for algo, ms, rs, kw in _configs():
        p0 = engine.make_params(algo, ms, rs, ref_texts=True, **kw)
        pg = engine.make_params(algo, ms, rs, read_groups=True, ref_texts=True, **kw)
        pm = engine.make_params(algo, ms, rs, read_groups=True, ref_texts=True, mate_pairs=True, **kw)
        before = [_describe(p0, n), lib.aim_scratch_bytes(capi.params_ref(p0), n), _describe(pg, n), lib.aim_scratch_bytes(capi.params_ref(pg), n)]
        assert before[0][0] == 0 and before[2][0] == 0 and before[1] > 0 and before[3] > 0
        rc, line = _describe(pm, n)
        assert rc == 0 and line.endswith(" groups=1 mates=1") and line == before[2][1] + " mates=1", line
        assert lib.aim_scratch_bytes(capi.params_ref(pm), n) == before[3] + _al(16 * n)
        assert lib.aim_kernel_name(capi.params_ref(pm)) == lib.aim_kernel_name(capi.params_ref(pg))
        after = [_describe(p0, n), lib.aim_scratch_bytes(capi.params_ref(p0), n), _describe(pg, n), lib.aim_scratch_bytes(capi.params_ref(pg), n)]
        assert after == before
        assert "mates" not in before[0][1] and "mates" not in before[2][1]


def test_mate_select_kernel_code_object():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_regs
    lib = os.path.join(ROOT, "aim_amd", "libaim_hip.so")
    if not os.path.exists(lib):
        pytest.fail("libaim_hip.so is missing: run the build")
    regs = codeobj_regs.kernel_regs(lib)
    names = [k for k in regs if "aim::mate_select_kernel" in k]
    assert len(names) == 1, names
    r = regs[names[0]]
    assert r["scratch_bytes"] == 0 and r["lds_static_bytes"] == 0, r
    assert 0 < r["vgpr"] <= 64, r


def test_device_code_uses_vector_stores_only():
    src = open(os.path.join(ROOT, "aim_amd", "csrc", "mates.hpp")).read()
    code = re.sub(r"//[^\n]*", "", src)
    for word in ("atomic", "__shared__", "asm", "while (true)", "__syncthreads"):
        assert word not in code, word


# ---- the model on hand-made read pairs -------------------------------------------------------------------------------------------
def _run_model(cands_a, cands_b, lo, hi, pen):
    """cands: (score, ok, start, minus, text_len) per candidate of read 0 / read 1."""
    import mate_pairs_model as mm
    from aim_amd import capi
    c = list(cands_a) + list(cands_b)
    scores = [x[0] for x in c]
    status = [capi.PAIR_OK if x[1] else capi.PAIR_NOMEM for x in c]
    tpos = [x[2] | (MINUS if x[3] else 0) for x in c]
    tlen = [x[4] for x in c]
    sel, mates, best = mm.select(scores, status, tpos, tlen, [0, len(cands_a), len(c)], lo, hi, pen)
    m = mates[0]
    return [int(x) for x in sel], (int(m["best_pair"][0]), int(m["best_pair"][1]), int(m["score_sum"]), int(m["second_sum"]), int(m["n_best"]), int(m["flags"]))


def test_model_by_hand():
    F, R = False, True
    # a repeat: read 0's two copies tie, only the second is at a proper distance from the mate
    sel, m = _run_model([(2, True, 9000, F, 100), (2, True, 1000, F, 100)], [(3, True, 1300, R, 100)], 300, 500, 10)
    assert sel == [1, 2] and m == (1, 2, 5, INT32_MAX, 1, 1)
    # the same with the mate on the same strand: no proper combination, the independent winners, the unpaired cost
    sel, m = _run_model([(2, True, 9000, F, 100), (2, True, 1000, F, 100)], [(3, True, 1300, F, 100)], 300, 500, 10)
    assert sel == [0, 2] and m == (0, 2, 15, INT32_MAX, 0, 0)
    # the strand-1 window left of the strand-0 window is not proper, whatever the span
    sel, m = _run_model([(0, True, 1300, F, 100)], [(0, True, 1000, R, 100)], 0, 10 ** 6, 0)
    assert m[5] == 0 and m[2] == 0
    # read 0 on the minus strand: f is read 1's candidate
    sel, m = _run_model([(1, True, 1300, R, 100)], [(1, True, 1000, F, 100)], 400, 400, 0)
    assert sel == [0, 1] and m == (0, 1, 2, INT32_MAX, 1, 1)
    sel, m = _run_model([(1, True, 1300, R, 100)], [(1, True, 1000, F, 100)], 401, 500, 7)
    assert m == (0, 1, 9, INT32_MAX, 0, 0)
    # a proper combination that costs more than unpaired + penalty loses; a tie goes to proper; second_sum reports it either way
    a = [(0, True, 50000, F, 100), (6, True, 1000, F, 100)]
    b = [(0, True, 1300, R, 100)]
    assert _run_model(a, b, 300, 500, 5) == ([0, 2], (0, 2, 5, 6, 0, 0))
    assert _run_model(a, b, 300, 500, 6) == ([1, 2], (1, 2, 6, INT32_MAX, 1, 1))
    # ties among proper combinations: lowest i, then lowest j; n_best counts them, second_sum equals the cost
    a = [(4, True, 1000, F, 100), (4, True, 1001, F, 100)]
    b = [(1, True, 1300, R, 100), (1, True, 1301, R, 100), (2, True, 1302, R, 100)]
    assert _run_model(a, b, 300, 500, 0) == ([0, 2], (0, 2, 5, 5, 4, 1))
    # a mate without an OK candidate: the other keeps its independent winner
    sel, m = _run_model([(4, False, 1000, F, 100), (3, False, 1000, F, 100)], [(9, True, 1300, R, 100), (1, True, 7, R, 100)], 300, 500, 0)
    assert sel == [0, 3] and m == (UINT32_MAX, 3, INT32_MAX, INT32_MAX, 0, 0)
    # a candidate that is not OK never pairs, a zero-width window does (span = start_r - start_f)
    sel, m = _run_model([(0, False, 1000, F, 100), (5, True, 1000, F, 0)], [(1, True, 1400, R, 0)], 400, 400, 100)
    assert sel == [1, 2] and m == (1, 2, 6, INT32_MAX, 1, 1)
    # sums are clamped to INT32_MAX - 1: a very large penalty still loses only to a proper combination
    sel, m = _run_model([(2, True, 9000, F, 100)], [(3, True, 1300, F, 100)], 300, 500, INT32_MAX)
    assert m == (0, 1, INT32_MAX - 1, INT32_MAX, 0, 0)
    sel, m = _run_model([(INT32_MAX - 5, True, 1000, F, 100)], [(INT32_MAX - 5, True, 1300, R, 100)], 300, 500, INT32_MAX)
    assert m == (0, 1, INT32_MAX - 1, INT32_MAX, 1, 1)


# ---- the generator, scored by the CPU oracle ---------------------------------------------------------------------------------
REPEAT_FRAC = 0.4       # the mate-resolved share is about half of it (the copy listed first wins the independent tie)


def test_generator_layout():
    from aim_amd import engine
    ms, rs = engine.launcher_sizes("wfa", 100, 0.01)
    ref, req, rows, offs, tpos, txt, pats, truth = engine.mate_pairs(5, 40, 100, 0.01, 400, 8, REPEAT_FRAC, read_size=rs)
    assert len(req) == 640 and rows.shape == (80, rs) and offs.tolist() == list(range(0, 641, 8)) and len(truth) == 40
    assert set(np.unique(ref).tolist()) <= set(b"ACGT")
    for c in range(len(req)):
        pos, minus = int(tpos[c]) & (MINUS - 1), bool(int(tpos[c]) >> 63)
        assert pos + 100 <= len(ref)
        assert np.array_equal(txt[c, :100], engine.ref_window(ref, pos, 100, minus)) and not txt[c, 100:].any()
        assert np.array_equal(pats[c], rows[c // 8]) and int(req["pattern_len"][c]) == int(np.count_nonzero(rows[c // 8]))
    for m in range(40):
        ta, tb = (int(x) for x in truth["true"][m])
        assert ta // 8 == 2 * m and tb // 8 == 2 * m + 1
        sa, sb = int(tpos[ta]) >> 63, int(tpos[tb]) >> 63
        pa, pb = int(tpos[ta]) & (MINUS - 1), int(tpos[tb]) & (MINUS - 1)
        if truth["kind"][m] == engine.MATE_DISCORDANT:
            assert sa == sb == 0
        else:                                      # FR: the plus-strand read first, the fragment inside insert +- 10 %
            assert sa != sb
            f, r = (pa, pb) if sb else (pb, pa)
            assert f <= r and 360 <= r + 100 - f <= 440
        if truth["kind"][m] == engine.MATE_REPEAT:  # exactly one read has a second candidate with the true window's bytes
            twins = [sum(1 for c in range(8 * r, 8 * r + 8) if np.array_equal(txt[c], txt[t])) for r, t in ((2 * m, ta), (2 * m + 1, tb))]
            assert sorted(twins) == [1, 2]
    again = engine.mate_pairs(5, 40, 100, 0.01, 400, 8, REPEAT_FRAC, read_size=rs)
    assert all(np.array_equal(x, y) for x, y in zip(again, (ref, req, rows, offs, tpos, txt, pats, truth)))
    assert set(truth["kind"].tolist()) == {engine.MATE_UNIQUE, engine.MATE_REPEAT, engine.MATE_DISCORDANT}


def test_generator_and_model_with_the_oracle():
    """WFA-adaptive l = 100, e = 1 %, K = 8, insert 400: every candidate scored by the CPU oracle, then the model. All three outcomes
    occur, and at least 10 % of the read pairs are proper with a choice that differs from the independent winners."""
    import mate_pairs_model as mm
    from aim_amd import engine
    from oracle import oracle
    oracle.build()
    ms, rs = engine.launcher_sizes("wfa", 100, 0.01)
    n_mates = 300
    ref, req, rows, offs, tpos, txt, pats, truth = engine.mate_pairs(11, n_mates, 100, 0.01, 400, 8, REPEAT_FRAC, read_size=rs)
    op = oracle.params("wfa", ms, rs, backtrace=False, reduce=True)
    ores, _, worst = oracle.align_batch(op, req["pattern_len"], req["text_len"], pats, txt, nthreads=4)
    assert worst == 0
    sel, mates, best = mm.select(ores["score"], ores["status"], tpos, req["text_len"], offs, 340, 460, 2 * (ms + 1))
    ind = best["best_pair"].reshape(-1, 2)
    proper = (mates["flags"] & 1) != 0
    same = (mates["best_pair"] == ind).all(axis=1)
    n_same, n_diff, n_unpaired = int((proper & same).sum()), int((proper & ~same).sum()), int((~proper).sum())
    print("proper and equal %d, proper and different %d, unpaired %d of %d" % (n_same, n_diff, n_unpaired, n_mates))
    assert n_same > 0 and n_diff > 0 and n_unpaired > 0
    assert n_diff >= n_mates // 10
    assert np.array_equal(sel.reshape(-1, 2), mates["best_pair"])
    # the mate resolves the repeat: wherever the choice is proper it is the true windows (or ties them in score at a proper distance)
    true = truth["true"]
    hit = (mates["best_pair"] == true).all(axis=1)
    rep = truth["kind"] == engine.MATE_REPEAT
    assert proper[rep].all() and hit[rep].mean() > 0.9
    assert (ind[rep] == true[rep]).all(axis=1).mean() < 0.75        # ... which the independent selection cannot do
    assert not proper[truth["kind"] == engine.MATE_DISCORDANT].any()
    assert (mates["score_sum"][~proper] == best["best_score"].reshape(-1, 2).sum(axis=1)[~proper] + 2 * (ms + 1)).all()
