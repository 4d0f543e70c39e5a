"""AIM_FLAG_SAM_FIELDS without a GPU: the model (tests/sam_model.py) checked by round trip -- the reference slice rebuilt from the READ,
the CIGAR and the MD -- on pairs aligned by the CPU oracle, hand-written rows, then the ABI values and layouts, every refusal, the
plan line, aim_sam_format_cigar, the Python binding and the kernels' code objects."""
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

import sam_model  # noqa: E402
from sam_model import BAM_D, BAM_EQ, BAM_I, BAM_M, BAM_S, BAM_X  # noqa: E402

MINUS = 1 << 63


def _lib():
    from aim_amd import capi
    return capi.load()


def _define(name):
    m = re.search(r"#define\s+%s\s+(\S+)" % name, open(HEADER).read())
    return int(m.group(1).rstrip("uUlL"), 0)


def _err():
    return _lib().aim_last_error().decode()


def _describe(params, n=4096):
    from aim_amd import capi
    b = C.create_string_buffer(2048)
    rc = _lib().aim_plan_describe(capi.params_ref(params), n, b, 2048)
    return rc, b.value.decode()


@pytest.fixture(autouse=True)
def feature_bit():
    """Every test of this module is about the feature: the model tests below format their CIGARs through the library too."""
    from aim_amd import capi, engine
    assert engine.features() & capi.FEATURE_SAM_FIELDS


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def _reference(seed, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng([seed, 0x73616D]).integers(0, 4, size=n)].copy()


def _flanked(engine, ref, req, tpos, rs, flank):
    """The same reads against windows widened by `flank` bases on both sides (clamped to the reference)."""
    req2 = req.copy()
    tp2 = tpos.copy()
    rs2 = engine.round_up_8(rs + 2 * flank)
    txt2 = np.zeros((len(req), rs2), dtype=np.uint8)
    for i in range(len(req)):
        tl = int(req["text_len"][i]) + 2 * flank
        pos = min(max((int(tpos[i]) & (MINUS - 1)) - flank, 0), len(ref) - tl)
        minus = int(tpos[i]) >> 63
        tp2[i] = pos | (minus << 63)
        req2["text_len"][i] = tl
        txt2[i, :tl] = engine.ref_window(ref, pos, tl, bool(minus))
    return req2, tp2, txt2, rs2


@pytest.mark.parametrize("algo", ["wfa", "nw", "swg"])
@pytest.mark.parametrize("flank", [0, 8])
def test_model_round_trip_on_oracle_alignments(built, algo, flank):
    """l = 100, e = 5 %, both strands: the reference slice [pos, pos + ref_span) rebuilt from the read, the CIGAR and the MD is the
    reference; lengths and NM follow from the CIGAR alone. With flanks the global alignment itself carries terminal gap runs."""
    from aim_amd import engine
    from oracle import oracle
    n, length, err = 48, 100, 0.05
    ref = _reference(11 + flank, 20000)
    ms, rs = engine.launcher_sizes(algo, length, err)
    req, pat, tpos, txt = engine.ref_pairs(5 + flank, 0, n, length, err, ref, rs)
    if flank:
        req, tpos, txt, rs2 = _flanked(engine, ref, req, tpos, rs, flank)
        pat = np.concatenate([pat, np.zeros((n, rs2 - rs), dtype=np.uint8)], axis=1)
        rs = rs2
        if algo == "wfa":
            ms += 2 * (4 + flank)      # the terminal gaps of a global alignment are not free
    op = oracle.params(algo, ms, rs, backtrace=True)
    res, ops, worst = oracle.align_batch(op, req["pattern_len"], req["text_len"], pat, txt, nthreads=4)
    assert worst == 0
    strands = set()
    for i in range(n):
        tp = int(tpos[i])
        ws, strand = tp & (MINUS - 1), tp >> 63
        b, e = int(res["begin_offset"][i]), int(res["end_offset"][i])
        pos, span, nm, words, md, flags = sam_model.sam_fields(ops[i], b, e, strand, ws, ref)
        _, _, nm_x, words_x, md_x, _ = sam_model.sam_fields(ops[i], b, e, strand, ws, ref, eqx=True)
        assert flags == (sam_model.SAM_REVERSE if strand else 0) and words, i
        assert engine.sam_format_cigar(words) == sam_model.cigar_string(words) and engine.sam_format_cigar(words_x) == sam_model.cigar_string(words_x)
        read = pat[i, :int(req["pattern_len"][i])]
        read = engine.ref_window(read, 0, len(read), True) if strand else read      # the read on the forward strand
        rebuilt, used = sam_model.rebuild_reference(read.tobytes(), words, md, strict=algo == "wfa")
        assert rebuilt == ref[pos:pos + span].tobytes(), (i, sam_model.cigar_string(words), md)
        assert sam_model.rebuild_reference(read.tobytes(), words_x, md_x)[0] == rebuilt
        by_op = lambda ws_, ops_: sum(w >> 4 for w in ws_ if (w & 15) in ops_)
        assert by_op(words, (BAM_M, BAM_I, BAM_S, BAM_EQ, BAM_X)) == len(read) == used, i
        assert by_op(words, (BAM_M, BAM_D, BAM_EQ, BAM_X)) == span, i
        assert nm == nm_x == by_op(words_x, (BAM_X, BAM_I, BAM_D)), i
        assert md == md_x and (words[0] & 15) not in (BAM_I, BAM_D) and (words[-1] & 15) not in (BAM_I, BAM_D)
        assert all((a & 15) != (b_ & 15) for a, b_ in zip(words, words[1:])), "adjacent equal ops are merged"
        assert ws <= pos and pos + span <= ws + int(req["text_len"][i])
        strands.add(strand)
    assert strands == {0, 1}


REF = np.frombuffer(b"ACGTACGTTTGACCAGTAGGCATCGA", dtype=np.uint8)


def _w(*runs):
    return [(n << 4) | op for n, op in runs]


HAND = [
    # (ops, strand, window start, eqx) -> (pos, span, nm, words, md)
    ("all gaps", b"IIIDDDII", 0, 3, False, None),
    ("only clips", b"DDDD", 0, 3, False, None),
    ("plain", b"MMMM", 0, 2, False, (2, 4, 0, _w((4, BAM_M)), b"4")),
    ("adjacent mismatches", b"MXXM", 0, 0, False, (0, 4, 2, _w((4, BAM_M)), b"1C0G1")),
    ("leading mismatch", b"XMM", 0, 4, False, (4, 3, 1, _w((3, BAM_M)), b"0A2")),
    ("deletion then mismatch", b"MMIIXM", 0, 0, False, (0, 6, 3, _w((2, BAM_M), (2, BAM_D), (2, BAM_M)), b"2^GT0A1")),
    ("insertion keeps the count", b"MMDDMM", 0, 0, False, (0, 4, 2, _w((2, BAM_M), (2, BAM_I), (2, BAM_M)), b"4")),
    ("deletions split by an insertion", b"MIDIM", 0, 0, False, (0, 4, 3, _w((1, BAM_M), (1, BAM_D), (1, BAM_I), (1, BAM_D), (1, BAM_M)), b"1^C0^G1")),
    ("alternating terminal runs", b"IDIDDMXMDIID", 0, 1, False, (3, 3, 1, _w((3, BAM_S), (3, BAM_M), (2, BAM_S)), b"1A1")),
    ("eqx", b"MXXMIM", 0, 0, True, (0, 6, 3, _w((1, BAM_EQ), (2, BAM_X), (1, BAM_EQ), (1, BAM_D), (1, BAM_EQ)), b"1C0G1^A1")),
    # strand 1: the row is walked from its end; dropped reference bases at the row's END move pos
    ("reverse", b"DDIMMXMII", 1, 4, False, (6, 4, 1, _w((4, BAM_M), (2, BAM_S)), b"1T2")),
    ("reverse deletion then mismatch", b"MXIIMM", 1, 0, False, (0, 6, 3, _w((2, BAM_M), (2, BAM_D), (2, BAM_M)), b"2^GT0A1")),
]


@pytest.mark.parametrize("name,ops,strand,ws,eqx,want", HAND, ids=[h[0] for h in HAND])
def test_model_hand_written(name, ops, strand, ws, eqx, want):
    row = np.frombuffer(b"??" + ops + b"??", dtype=np.uint8)          # the range sits inside a row of other bytes
    got = sam_model.sam_fields(row, 2, 2 + len(ops), strand, ws, REF, eqx)
    from aim_amd import engine
    assert engine.sam_format_cigar(got[3]) == sam_model.cigar_string(got[3])
    if want is None:
        assert got == (ws, 0, 0, [], b"", sam_model.SAM_UNMAPPED)
    else:
        assert got == want + (sam_model.SAM_REVERSE if strand else 0,), (got, want)


def test_model_unmapped_rows():
    from aim_amd import capi
    res = np.zeros(1, dtype=capi.RESULT_DTYPE)
    row = np.frombuffer(b"MMMM", dtype=np.uint8)
    res["end_offset"] = 4
    assert sam_model.row_fields(res[0], row, 7, REF, True, 10)[:2] == (7, 4)
    assert sam_model.row_fields(res[0], row, None, REF, True, 10) == (0, 0, 0, [], b"", 4)
    res["score"] = 11
    assert sam_model.row_fields(res[0], row, 7 | MINUS, REF, True, 10) == (7, 0, 0, [], b"", 4)
    assert sam_model.row_fields(res[0], row, 7, REF, False, 10)[1] == 4          # NW / SWG have no cap
    res["score"], res["status"] = 0, 3
    assert sam_model.row_fields(res[0], row, 7, REF, True, 10)[5] == 4
    res["status"], res["begin_offset"] = 0, 4
    assert sam_model.row_fields(res[0], row, 7, REF, True, 10)[5] == 4


# ---- the ABI -----------------------------------------------------------------------------------------------------------------------
def test_feature_bit_and_flag_values():
    from aim_amd import capi, engine
    assert _define("AIM_FLAG_SAM_FIELDS") == capi.FLAG_SAM_FIELDS == 0x4000
    assert _define("AIM_FEATURE_SAM_FIELDS") == capi.FEATURE_SAM_FIELDS == 0x200
    assert (_define("AIM_SAM_EQX"), _define("AIM_SAM_REVERSE"), _define("AIM_SAM_UNMAPPED"), _define("AIM_SAM_OVERFLOW")) == \
        (capi.SAM_EQX, capi.SAM_REVERSE, capi.SAM_UNMAPPED, capi.SAM_OVERFLOW) == (1, 0x10, 4, 0x100)
    assert engine.features() & 0x200
    assert _lib().aim_abi_version() == 2


def test_struct_layouts():
    from aim_amd import capi
    assert capi.SAM_DTYPE.itemsize == 48
    assert capi.SAM_DTYPE.names == ("idx", "score", "pos", "ref_span", "nm", "cigar_offset", "n_cigar", "md_offset", "md_len", "flags", "status", "pad")
    assert [capi.SAM_DTYPE.fields[k][1] for k in capi.SAM_DTYPE.names] == [0, 4, 8, 16, 20, 24, 28, 32, 36, 40, 42, 44]
    assert (C.sizeof(capi.BatchIO), C.sizeof(capi.BatchIORef), C.sizeof(capi.BatchIOGroups), C.sizeof(capi.BatchIOMates)) == (120, 128, 152, 184)
    assert capi.BatchIOSam.mates.offset == 0 and capi.BatchIOSam.sam.offset == 184
    assert [getattr(capi.BatchIOSam, f).offset for f in ("sam", "sam_cigar", "sam_cigar_cap", "sam_md", "sam_md_cap", "sam_options")] == \
        [184, 192, 200, 208, 216, 220]
    assert C.sizeof(capi.BatchIOSam) == 224


def test_header_layout_by_the_c_compiler(tmp_path):
    import subprocess
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "aim_hip.h"\n'
                   'int main(void) { printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\\n", sizeof(aim_sam_t), offsetof(aim_sam_t, pos),\n'
                   'offsetof(aim_sam_t, cigar_offset), offsetof(aim_sam_t, flags), offsetof(aim_sam_t, status), offsetof(aim_sam_t, pad),\n'
                   'sizeof(aim_batch_io_t), sizeof(aim_batch_io_groups_t), sizeof(aim_batch_io_mates_t), offsetof(aim_batch_io_sam_t, sam),\n'
                   'offsetof(aim_batch_io_sam_t, sam_md), offsetof(aim_batch_io_sam_t, sam_options), sizeof(aim_batch_io_sam_t)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert subprocess.check_output([str(exe)], text=True).split() == ["48", "8", "24", "40", "42", "44", "120", "152", "184", "184", "208", "220", "224"]


def test_make_params():
    from aim_amd import capi, engine
    p = engine.make_params("wfa", 20, 112, ref_texts=True, backtrace=True, sam=True)
    assert p.flags == capi.FLAG_SAM_FIELDS | capi.FLAG_REF_TEXTS | capi.FLAG_BACKTRACE
    for kw in (dict(), dict(ref_texts=True), dict(backtrace=True), dict(ref_texts=True, backtrace=True, res8=True)):
        with pytest.raises(ValueError):
            engine.make_params("wfa", 20, 112, sam=True, **kw)
    with pytest.raises(ValueError):
        engine.make_params("genasm", 0, 112, sam=True, ref_texts=True, backtrace=True)
    assert not engine.make_params("wfa", 20, 112, ref_texts=True, backtrace=True).flags & capi.FLAG_SAM_FIELDS
    p = engine.make_params("wfa", 20, 112, ref_texts=True, backtrace=True, sam=True, read_groups=True, mate_pairs=True, ends_free=(0, 0, 8, 8))
    assert p.flags & capi.FLAG_SAM_FIELDS and p.flags & capi.FLAG_MATE_PAIRS and p.flags & capi.FLAG_ENDSFREE


def test_refusals():
    """Every refusal of the flag and of aim_sam_device, with its message; none needs a device."""
    from aim_amd import capi
    lib = _lib()
    F, REF_T, BT, RES8 = capi.FLAG_SAM_FIELDS, capi.FLAG_REF_TEXTS, capi.FLAG_BACKTRACE, capi.FLAG_RES8
    mk = lambda algo, flags: capi.Params(algo, 0, 3, 4, 1, 4, 4, 20, 112, flags)
    for p, msg in ((mk(capi.ALGO_WFA, F | BT), "AIM_FLAG_SAM_FIELDS needs AIM_FLAG_REF_TEXTS"),
                   (mk(capi.ALGO_WFA, F | REF_T), "AIM_FLAG_SAM_FIELDS needs AIM_FLAG_BACKTRACE"),
                   (mk(capi.ALGO_NW, F), "AIM_FLAG_SAM_FIELDS needs AIM_FLAG_REF_TEXTS"),
                   (mk(capi.ALGO_SWG, F | REF_T | RES8), "AIM_FLAG_SAM_FIELDS cannot be combined with AIM_FLAG_RES8"),
                   (mk(capi.ALGO_GENASM, F | REF_T | BT), "AIM_FLAG_SAM_FIELDS cannot be combined with AIM_ALGO_GENASM")):
        rc, _ = _describe(p)
        assert rc == capi.AIM_EINVAL and _err().startswith(msg), (_err(), msg)
        assert lib.aim_scratch_bytes(capi.params_ref(p), 64) == 0
        assert lib.aim_kernel_name(capi.params_ref(p)) == b""
    dev = lambda p, opts=0: lib.aim_sam_device(capi.params_ref(p), 4, None, None, None, None, None, None, 0, opts, None, None, 0, None, 0, None, None)
    assert dev(mk(capi.ALGO_GENASM, BT)) == capi.AIM_EINVAL and "AIM_ALGO_GENASM" in _err() and "begin_offset = 0" in _err()
    assert dev(mk(capi.ALGO_WFA, 0)) == capi.AIM_EINVAL and "needs AIM_FLAG_BACKTRACE" in _err()
    assert dev(mk(capi.ALGO_WFA, RES8)) == capi.AIM_EINVAL and "AIM_FLAG_BACKTRACE" in _err()
    assert dev(mk(capi.ALGO_SWG, BT | RES8)) == capi.AIM_EINVAL and "AIM_FLAG_RES8" in _err()
    assert dev(mk(capi.ALGO_WFA, BT), 2) == capi.AIM_EINVAL and "unknown options" in _err()
    assert dev(mk(capi.ALGO_WFA, BT)) == capi.AIM_EINVAL and "null device buffer" in _err()
    # the 32-bit offsets: the bound depends on the row count and READ_SIZE only and is refused before a device is needed
    big = capi.Params(capi.ALGO_WFA, 0, 3, 4, 1, 4, 4, 20, 10112, BT)
    rc = lib.aim_sam_device(capi.params_ref(big), 106200, None, None, None, None, None, None, 0, 0, None, None, 0, None, 0, C.c_void_p(64), None)
    assert rc == capi.AIM_EINVAL and "exceed the 32-bit offsets" in _err() and "split the batch" in _err()
    # the stateless alignment calls refuse the flag: their rows go through aim_sam_device
    ok = mk(capi.ALGO_WFA, F | REF_T | BT)
    assert lib.aim_align_device(capi.params_ref(ok), 1, None, None, None, None, None, None, 0, None) == capi.AIM_EINVAL and "aim_sam_device" in _err()
    assert lib.aim_align_device_ref(capi.params_ref(ok), 1, None, None, None, None, 0, None, None, None, 0, None) == capi.AIM_EINVAL and "aim_sam_device" in _err()
    okg = mk(capi.ALGO_WFA, F | REF_T | BT | capi.FLAG_READ_GROUPS)
    gargs = (None, None, None, None, None, 0, None, None, None, None, None, 0, None)
    assert lib.aim_align_device_groups(capi.params_ref(okg), 4, 2, *gargs) == capi.AIM_EINVAL and "aim_sam_device" in _err()
    okm = mk(capi.ALGO_WFA, F | REF_T | BT | capi.FLAG_READ_GROUPS | capi.FLAG_MATE_PAIRS)
    margs = (None, None, None, None, None, 0, None, None, None, None, 0, 10, 0, None, None, 0, None)
    assert lib.aim_align_device_mates(capi.params_ref(okm), 4, 2, *margs) == capi.AIM_EINVAL and "aim_sam_device" in _err()
    # the follow-ups named in the header stay refused under the flag
    esc_groups = mk(capi.ALGO_WFA, F | REF_T | BT | capi.FLAG_WFA_ESCALATE | capi.FLAG_READ_GROUPS)
    assert _describe(esc_groups)[0] == capi.AIM_EINVAL and "AIM_FLAG_WFA_ESCALATE cannot be combined with AIM_FLAG_READ_GROUPS" in _err()
    assert _describe(mk(capi.ALGO_WFA, F | REF_T | BT | capi.FLAG_MATE_PAIRS))[0] == capi.AIM_EINVAL and "AIM_FLAG_MATE_PAIRS needs AIM_FLAG_READ_GROUPS" in _err()


FAMILIES = [   # one shape per kernel family: (algo, l, e, make_params keywords)
    ("wfa", 100, 0.01, dict(reduce=True)), ("wfa", 100, 0.05, dict()), ("wfa", 1000, 0.05, dict()), ("wfa", 1000, 0.05, dict(bidir=True)),
    ("wfa", 100, 0.05, dict(escalate=True)), ("wfa", 100, 0.05, dict(ends_free=(0, 0, 8, 8))), ("wfa", 100, 0.05, dict(read_groups=True)),
    ("wfa", 100, 0.05, dict(read_groups=True, mate_pairs=True)), ("nw", 100, 0.05, dict()), ("swg", 100, 0.05, dict()),
    ("nw", 1000, 0.05, dict()), ("swg", 300, 0.05, dict()),
]


@pytest.mark.parametrize("algo,length,err,kw", FAMILIES, ids=["%s-l%d-%s" % (f[0], f[1], "-".join(sorted(f[3])) or "plain") for f in FAMILIES])
def test_plan_line_and_scratch(algo, length, err, kw, monkeypatch):
    """' sam=1' ends the line under the flag and is all that differs; the flag-less line and aim_scratch_bytes do not move, planned
    before and after the flag."""
    from aim_amd import capi, engine
    monkeypatch.setenv("AIM_SCRATCH_GB", "16")
    monkeypatch.setenv("AIM_CHIP_CUS", "256")
    lib = _lib()
    ms, rs = engine.launcher_sizes(algo, length, err)
    p0 = engine.make_params(algo, ms, rs, backtrace=True, ref_texts=True, **kw)
    p1 = engine.make_params(algo, ms, rs, backtrace=True, ref_texts=True, sam=True, **kw)
    rc, before = _describe(p0)
    assert rc == 0 and "sam=" not in before
    s0 = lib.aim_scratch_bytes(capi.params_ref(p0), 4096)
    rc, line = _describe(p1)
    assert rc == 0 and line == before + " sam=1", (line, before)
    assert lib.aim_scratch_bytes(capi.params_ref(p1), 4096) == s0 > 0
    assert lib.aim_kernel_name(capi.params_ref(p1)) == lib.aim_kernel_name(capi.params_ref(p0))
    assert _describe(p0) == (0, before) and lib.aim_scratch_bytes(capi.params_ref(p0), 4096) == s0


def test_mapping_by_read_size(monkeypatch):
    """The kernel a launch takes: one row per lane below kSamWaveMinReadSize, one row per wavefront from it; AIM_SAM_WAVE_MIN overrides."""
    from aim_amd import engine
    hpp = open(os.path.join(ROOT, "aim_amd", "csrc", "sam_fields.hpp")).read()
    switch = int(re.search(r"kSamWaveMinReadSize = (\d+);", hpp).group(1))
    assert switch % 8 == 0
    name = lambda rs: engine.sam_kernel_name(engine.make_params("wfa", 20, rs, backtrace=True, ref_texts=True))
    monkeypatch.delenv("AIM_SAM_WAVE_MIN", raising=False)
    assert (name(112), name(switch - 8), name(switch), name(10112)) == ("sam_lane_kernel", "sam_lane_kernel", "sam_wave_kernel", "sam_wave_kernel")
    monkeypatch.setenv("AIM_SAM_WAVE_MIN", "0")
    assert name(112) == "sam_wave_kernel"
    monkeypatch.setenv("AIM_SAM_WAVE_MIN", "1000000")
    assert name(10112) == "sam_lane_kernel"


def test_sam_format_cigar():
    from aim_amd import capi, engine
    lib = _lib()
    assert engine.sam_format_cigar([]) == "*"
    words = [(3 << 4) | 4, (100 << 4) | 0, (1 << 4) | 1, (70 << 4) | 2, (5 << 4) | 7, (2 << 4) | 8, ((1 << 28) - 1) << 4]
    assert engine.sam_format_cigar(words) == "3S100M1I70D5=2X268435455M" == sam_model.cigar_string(words)
    w = np.array(words, dtype=np.uint32)
    buf = C.create_string_buffer(64)
    assert lib.aim_sam_format_cigar(w.ctypes.data, 2, buf, 7) == 6 and buf.value == b"3S100M"
    assert lib.aim_sam_format_cigar(w.ctypes.data, 2, buf, 6) == capi.AIM_EINVAL and "too small" in _err()
    assert lib.aim_sam_format_cigar(None, 0, buf, 1) == capi.AIM_EINVAL
    bad = np.array([(4 << 4) | 9], dtype=np.uint32)
    assert lib.aim_sam_format_cigar(bad.ctypes.data, 1, buf, 64) == capi.AIM_EINVAL and "op 9" in _err()
    sam = np.zeros(2, dtype=capi.SAM_DTYPE)
    sam["cigar_offset"], sam["n_cigar"], sam["md_offset"], sam["md_len"] = [5, 0], [2, 0], [1, 0], [3, 0]
    assert engine.sam_strings(sam, np.array([0] * 5 + words[:2], dtype=np.uint32), np.frombuffer(b"x9A1zz", dtype=np.uint8)) == \
        [("3S100M", "9A1"), ("*", "")]


def test_code_object_matches_the_launch_bounds(built):
    """Both mappings spill nothing, use no LDS, and stay within 64 VGPRs: 8 wavefronts per SIMD, whichever the workgroup size."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_regs
    regs = {k: v for k, v in codeobj_regs.kernel_regs().items() if "sam_lane_kernel" in k or "sam_wave_kernel" in k}
    assert len(regs) == 2, regs
    for name, r in regs.items():
        assert r["scratch_bytes"] == 0 and r["lds_static_bytes"] == 0, (name, r)
        assert r["vgpr"] + r["agpr"] <= 512 // 8, (name, r)
