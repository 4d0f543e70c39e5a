"""References of several sequences without a GPU: the feature bit and the layouts, rule 13c's numpy model on synthetic slot tables (every
clipped window inside its contig, every other slot unchanged, the cases the GPU test relies on present), the layout and concatenation
of the library against the model, every refusal by its message and without a device, aim_amd.samout over records of two contigs with
the whole text compared, load_contigs and the command line's switch, the code objects of the two new kernels, and the premises of the
GPU test's batch on the chain, split and contig models."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aim_hip.h")


def _lib():
    from aim_amd import capi
    return capi.load()


def _err():
    return _lib().aim_last_error().decode()


def _define(name):
    m = re.search(r"#define\s+%s\s+(\S+)" % name, open(HEADER).read())
    return int(m.group(1).rstrip("uUlL"), 0)


def test_feature_bit_abi_and_layouts():
    from aim_amd import capi, engine
    import contig_model as cg
    assert _define("AIM_FEATURE_CONTIGS") == capi.FEATURE_CONTIGS == 0x100000 and engine.features() & capi.FEATURE_CONTIGS
    assert _define("AIM_SEG_CONTIG_CLIPPED") == capi.SEG_CONTIG_CLIPPED == cg.CLIPPED == 0x80
    assert _define("AIM_CONTIG_NONE") == capi.CONTIG_NONE == cg.NONE == 0xFFFFFFFF
    assert re.search(r"#define AIM_CONTIG_MAX \(1u << 20\)", open(HEADER).read()) and capi.CONTIG_MAX == cg.MAX == 1 << 20
    assert re.search(r"#define AIM_CONTIG_SPACER\(band\) \(\(uint32_t\)\(band\) \+ 64u\)", open(HEADER).read())
    assert capi.CONTIG_SPACER(96) == cg.spacer_for(96) == 160
    assert _lib().aim_abi_version() == 2 and C.sizeof(capi.MapperParams) == 124 and C.sizeof(capi.MapperOut) == 56
    assert _lib().aim_contig_kernel_names() == b"contig_clip_kernel,map_records_contig_kernel"
    assert _lib().aim_mapper_kernel_names() == b"map_count_kernel,map_records_kernel"
    # every flag bit of aim_segment_t is now taken, each once
    bits = [capi.SEG_VALID, capi.SEG_SUPPLEMENTARY, capi.SEG_LEFT_OPEN, capi.SEG_RIGHT_OPEN, capi.SEG_LOOSE, capi.SEG_EXT_LEFT, capi.SEG_EXT_RIGHT, capi.SEG_CONTIG_CLIPPED]
    assert sorted(bits) == [1 << i for i in range(8)]


def test_layout_and_concat_equal_the_model():
    from aim_amd import engine
    import contig_model as cg
    for lens, spacer in (([5], 1), ([1, 1, 1], 1), ([7, 1, 300, 2], 160), ([3] * 1025, 65)):
        starts, ref_len = engine.contigs_layout(lens, spacer)
        w_starts, w_len = cg.layout(lens, spacer)
        assert starts.tolist() == w_starts.tolist() and ref_len == w_len and starts[0] == 0
        rng = np.random.default_rng(len(lens))
        seqs = [np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)] for n in lens]
        cat = engine.contigs_concat(seqs, spacer)
        assert cat.tobytes() == cg.concat(seqs, spacer).tobytes() and len(cat) == ref_len
        for c, s in enumerate(seqs):
            assert cat[starts[c]:starts[c] + lens[c]].tobytes() == s.tobytes()
        assert (cat == ord("N")).sum() == spacer * (len(lens) - 1)
    assert engine.contigs_concat([b"AC", b"G"], 3).tobytes() == b"ACNNNG"
    assert [cg.lookup([0, 5, 9], a) for a in (0, 4, 5, 8, 9, 100)] == [0, 0, 1, 1, 2, 2]


@pytest.mark.parametrize("K,n_reads,n_contigs", [(1, 65, 1), (4, 301, 2), (4, 301, 3), (16, 65, 1025), (4, 2100, 5000)])
def test_model_properties(K, n_reads, n_contigs):
    """Every clipped window lies inside its contig, a slot that is not clipped keeps every byte, and the batch holds the cases the GPU
    test is there for."""
    import contig_model as cg
    import split_model as sm
    lens, starts, ref_len, d, o = cg.synthetic_clip(7, K, n_reads, n_contigs)
    seg = d["seg"]
    valid = (seg["flags"] & sm.VALID) != 0
    clipped = (o["seg"]["flags"] & cg.CLIPPED) != 0
    assert not (clipped & ~valid).any() and (o["contig"][~valid] == cg.NONE).all() and (o["contig"][valid] < n_contigs).all()
    keep = ~clipped
    for name in ("seg_req", "seg_text_pos", "seg"):
        a, b = d[name], o[name]
        assert a[keep].tobytes() == b[keep].tobytes(), name
    # a clipped slot changes text_len, text_pos and the flag alone
    assert (o["seg_req"]["pattern_len"] == d["seg_req"]["pattern_len"]).all() and (o["seg_req"]["idx"] == d["seg_req"]["idx"]).all()
    assert (o["seg"]["q_begin"] == seg["q_begin"]).all() and (o["seg"]["q_end"] == seg["q_end"]).all() and ((o["seg"]["flags"] & 0x7F) == (seg["flags"] & 0x7F)).all()
    assert ((o["seg_text_pos"] >> np.uint64(63)) == (d["seg_text_pos"] >> np.uint64(63)))[valid].all()
    c = o["contig"][valid].astype(np.int64)
    s1 = (o["seg_text_pos"][valid] & np.uint64(cg.MINUS - 1)).astype(np.int64)
    e1 = s1 + o["seg_req"]["text_len"][valid]
    s0 = (d["seg_text_pos"][valid] & np.uint64(cg.MINUS - 1)).astype(np.int64)
    e0 = s0 + d["seg_req"]["text_len"][valid]
    lo, hi = starts[c].astype(np.int64), starts[c].astype(np.int64) + lens[c]
    inside = (s0 >= lo) & ((e0 <= hi) | (e0 == s0))          # (an empty window has no bound to move on the right)
    assert (inside == ~clipped[valid]).all()
    assert (e1 >= s1).all() and ((e1 == s1) | ((s1 >= lo) & (e1 <= hi))).all() and (s1 >= s0).all() and (e1 - s1 <= np.maximum(e0 - s0, 0)).all()
    A = o["anchor"][valid]
    assert (starts[c] <= A).all() and ((c + 1 == n_contigs) | (starts[np.minimum(c + 1, n_contigs - 1)] > A)).all() and (A >= 0).all() and (A < ref_len).all()
    cov = cg.coverage(lens, starts, d, o)
    print(cov)
    for k in ("valid", "not_valid", "empty", "right", "outside", "kept", "first_base", "last_base", "loose", "start0", "minus", "plus"):
        assert cov[k] > 0, (k, cov)
    if n_contigs > 1:
        assert cov["left"] > 0 and cov["both"] > 0 and cov["spacer"] > 0, cov
    if n_contigs >= 3:
        assert cov["len1"] > 0, cov


def test_record_model():
    """Rule 12c's records with pos moved into the contig and the contig in pad; AIM_CONTIG_NONE for an unmapped read."""
    import contig_model as cg
    import map_records_model as mm
    K, n = 4, 301
    seg, sam, cls = mm.synthetic_tables(5, K, n)
    lens, starts, ref_len, d, o = cg.synthetic_clip(5, K, n, 40, seg_flags=seg["flags"])
    off0, rec0 = mm.map_records(K, n, o["seg"], sam, cls)
    off, rec = cg.records(K, n, o["seg"], sam, cls, o["contig"], starts)
    assert off.tobytes() == off0.tobytes() and len(rec) == len(rec0)
    un = rec0["sam"]["flags"] == mm.SAM_UNMAPPED
    assert un.any() and (~un).any() and (rec["sam"]["pad"][un] == cg.NONE).all() and (rec["sam"]["pos"][un] == 0).all()
    c = o["contig"][rec["slot"][~un]]
    assert (rec["sam"]["pad"][~un] == c).all() and (rec["sam"]["pos"][~un] == rec0["sam"]["pos"][~un] - starts[c].astype(np.uint64)).all()
    a, b = rec.copy(), rec0.copy()
    for x in (a, b):
        x["sam"]["pos"] = 0
        x["sam"]["pad"] = 0
    assert a.tobytes() == b.tobytes()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------
def _params(**kw):
    from mapper_batch import params_with as base
    return base(**kw)


def _u32(xs):
    return np.array(xs, dtype=np.uint32)


LAYOUT_REFUSALS = [
    (dict(n=0), "n_contigs 0 is outside 1..1048576"),
    (dict(n=(1 << 20) + 1), "n_contigs 1048577 is outside 1..1048576"),
    (dict(lens=None), "lens is NULL"),
    (dict(lens=[5, 0, 7]), "lens[1] is 0"),
    (dict(lens=[0xF0000000, 0x0E000000]), "contig 1 ends at"),
    (dict(lens=[0xFE000001]), "contig 0 ends at 4261412865: ref_len is above 4261412864"),
]


@pytest.mark.parametrize("case", LAYOUT_REFUSALS, ids=lambda c: "-".join("%s" % k for k in c[0]))
def test_layout_refusals_from_every_entry_point(case):
    """The contig bounds, from the layout, the concatenation and the two mapper entry points, each under its own name, before the
    mapper's own checks (the parameters here break one of those too) and before any device query."""
    from aim_amd import capi
    lib = _lib()
    kw, text = case
    lens = kw.get("lens", [5, 6, 7])
    n = kw.get("n", len(lens) if lens is not None else 3)
    arr = _u32(lens) if lens is not None else None
    starts, rl, b, h = np.zeros(max(n, 1) if n < 100 else 1, dtype=np.uint32), C.c_uint64(), C.c_uint64(), C.c_void_p()
    mp = _params(mask_q8=0)
    calls = (("aim_contigs_layout", lambda: lib.aim_contigs_layout(n, capi.ptr(arr), 7, capi.ptr(starts), C.byref(rl))),
             ("aim_contigs_concat", lambda: lib.aim_contigs_concat(n, None, capi.ptr(arr), 7, None)),
             ("aim_mapper_device_bytes_contigs", lambda: lib.aim_mapper_device_bytes_contigs(C.byref(mp), n, capi.ptr(arr), C.byref(b))),
             ("aim_mapper_create_contigs", lambda: lib.aim_mapper_create_contigs(C.byref(mp), 0, n, None, capi.ptr(arr), C.byref(h))))
    for fn, call in calls:
        assert call() == capi.AIM_EINVAL and not h.value
        assert _err().startswith(fn + ": ") and text in _err(), (fn, _err())


def test_layout_refusals_of_its_own_arguments():
    from aim_amd import capi
    lib = _lib()
    lens, starts, rl = _u32([5, 6]), np.zeros(2, dtype=np.uint32), C.c_uint64()
    assert lib.aim_contigs_layout(2, capi.ptr(lens), 0, capi.ptr(starts), C.byref(rl)) == capi.AIM_EINVAL and _err() == "aim_contigs_layout: spacer 0 must be >= 1"
    assert lib.aim_contigs_layout(2, capi.ptr(lens), 1, None, C.byref(rl)) == capi.AIM_EINVAL and _err() == "aim_contigs_layout: starts is NULL"
    assert lib.aim_contigs_layout(2, capi.ptr(lens), 1, capi.ptr(starts), None) == capi.AIM_EINVAL and _err() == "aim_contigs_layout: ref_len is NULL"
    assert lib.aim_contigs_concat(2, None, capi.ptr(lens), 1, None) == capi.AIM_EINVAL and _err() == "aim_contigs_concat: seqs is NULL"
    seqs = (C.c_void_p * 2)(1 << 12, None)
    out = np.zeros(12, dtype=np.uint8)
    assert lib.aim_contigs_concat(2, seqs, capi.ptr(lens), 1, capi.ptr(out)) == capi.AIM_EINVAL and _err() == "aim_contigs_concat: seqs[1] is NULL"
    assert lib.aim_contigs_concat(2, seqs, capi.ptr(lens), 1, None) == capi.AIM_EINVAL and _err() == "aim_contigs_concat: out is NULL"
    assert lib.aim_contigs_layout(2, capi.ptr(lens), 0xFFFFFFFF, capi.ptr(starts), C.byref(rl)) == capi.AIM_EINVAL and "contig 1 ends at 4294967306" in _err()


def test_every_mapper_refusal_comes_back_for_contigs():
    """Behind the contig bounds, every check of aim_mapper_device_bytes / aim_mapper_create on the laid-out ref_len, under the new
    names; then the arguments of the two entry points."""
    from aim_amd import capi, engine
    from mapper_batch import REFUSALS
    lib = _lib()
    lens = _u32([9000, 1, 500])
    b, h = C.c_uint64(), C.c_void_p()
    for kw, text in REFUSALS:
        mp = _params(**kw)
        assert lib.aim_mapper_device_bytes_contigs(C.byref(mp), 3, capi.ptr(lens), C.byref(b)) == capi.AIM_EINVAL
        assert _err().startswith("aim_mapper_device_bytes_contigs: ") and text in _err(), (kw, _err())
        assert lib.aim_mapper_create_contigs(C.byref(mp), 0, 3, None, capi.ptr(lens), C.byref(h)) == capi.AIM_EINVAL and not h.value
        assert _err().startswith("aim_mapper_create_contigs: ") and text in _err(), (kw, _err())
    mp = _params()
    # the spacer counts: two contigs that fit AIM_SEED_MAX_REF_LEN side by side, but not with band + 64 between them
    big = _u32([0x7F000000, 0x7F000000])
    assert lib.aim_mapper_device_bytes_contigs(C.byref(mp), 2, capi.ptr(big), C.byref(b)) == capi.AIM_EINVAL
    assert "contig 1 ends at %d: ref_len is above 4261412864" % (0xFE000000 + 160) in _err(), _err()
    assert lib.aim_mapper_device_bytes_contigs(None, 3, capi.ptr(lens), C.byref(b)) == capi.AIM_EINVAL and _err() == "aim_mapper_device_bytes_contigs: params is NULL"
    assert lib.aim_mapper_device_bytes_contigs(C.byref(mp), 3, capi.ptr(lens), None) == capi.AIM_EINVAL and _err() == "aim_mapper_device_bytes_contigs: bytes is NULL"
    assert lib.aim_mapper_create_contigs(None, 0, 3, None, capi.ptr(lens), C.byref(h)) == capi.AIM_EINVAL and _err() == "aim_mapper_create_contigs: params is NULL"
    assert lib.aim_mapper_create_contigs(C.byref(mp), 0, 3, None, capi.ptr(lens), None) == capi.AIM_EINVAL and _err() == "aim_mapper_create_contigs: mapper is NULL"
    assert lib.aim_mapper_create_contigs(C.byref(mp), 0, 3, None, capi.ptr(lens), C.byref(h)) == capi.AIM_EINVAL and _err() == "aim_mapper_create_contigs: seqs is NULL"
    seqs = (C.c_void_p * 3)(1 << 12, 1 << 12, None)
    assert lib.aim_mapper_create_contigs(C.byref(mp), 0, 3, seqs, capi.ptr(lens), C.byref(h)) == capi.AIM_EINVAL and _err() == "aim_mapper_create_contigs: seqs[2] is NULL"
    assert lib.aim_mapper_contigs(None, None, None, None) == capi.AIM_EINVAL and _err() == "aim_mapper_contigs: mapper is NULL"
    # accepted: the table's 8 bytes per contig and d_contig's 4 bytes per slot come on top of the one-sequence mapper of the same length
    ref_len = engine.contigs_layout(lens, capi.CONTIG_SPACER(mp.seed.band))[1]
    one, many = engine.mapper_device_bytes(mp, ref_len), engine.mapper_device_bytes_contigs(mp, lens)
    per_slot = (4 * mp.max_reads * mp.seed.max_cands + 255) // 256 * 256
    assert many - one == 8 * 3 + mp.slots * per_slot, (one, many)


def test_clip_and_record_refusals_need_no_device():
    from aim_amd import capi
    lib = _lib()
    ok = 1 << 12           # any aligned address: nothing is dereferenced before the device probe
    clip = lambda K=4, rs=256, flank=16, ref_len=1000, nc=3, st=ok, ln=ok, n=8, rl=ok, rq=ok, tp=ok, ch=ok, sr=ok, stp=ok, sg=ok, ct=ok: \
        lib.aim_contig_clip_device(K, rs, flank, ref_len, nc, st, ln, n, rl, rq, tp, ch, sr, stp, sg, ct, None)
    for kw, text in ((dict(K=0), "K 0 is outside 1..16"), (dict(K=17), "K 17 is outside 1..16"), (dict(rs=100), "read_size 100 must be a positive multiple of 8"),
                     (dict(K=16, n=1 << 28), "n_reads 268435456 * K 16 does not fit 32 bits"), (dict(flank=-1), "flank -1 must be >= 0"),
                     (dict(ref_len=0), "ref_len must be >= 1"), (dict(ref_len=0xFE000001), "ref_len 4261412865 is above 4261412864"),
                     (dict(nc=0), "n_contigs 0 is outside 1..1048576"), (dict(nc=(1 << 20) + 1), "n_contigs 1048577 is outside"),
                     (dict(st=None), "d_contig_start or d_contig_len is NULL"), (dict(ln=None, n=0), "d_contig_start or d_contig_len is NULL"),
                     (dict(rl=None), "null device buffer"), (dict(rq=None), "null device buffer"), (dict(tp=None), "null device buffer"),
                     (dict(ch=None), "null device buffer"), (dict(sr=None), "null device buffer"), (dict(stp=None), "null device buffer"),
                     (dict(sg=None), "null device buffer"), (dict(ct=None), "null device buffer")):
        assert clip(**kw) == capi.AIM_EINVAL and _err().startswith("aim_contig_clip_device: ") and text in _err(), (kw, _err())
    rec = lambda K=4, n=8, seg=ok, sam=ok, cls=ok, ct=ok, nc=3, st=ok, off=ok, rc=ok, scr=ok, sb=8192: \
        lib.aim_map_records_contigs_device(K, n, seg, sam, cls, ct, nc, st, off, rc, scr, sb, None)
    for kw, text in ((dict(K=0), "K 0 is outside 1..16"), (dict(K=16, n=1 << 28), "does not fit 32 bits"), (dict(off=None), "d_rec_offsets is NULL"),
                     (dict(nc=0), "n_contigs 0 is outside 1..1048576"), (dict(ct=None), "null device buffer"), (dict(st=None), "null device buffer"),
                     (dict(seg=None), "null device buffer"), (dict(sam=ok + 8), "d_sam and d_records must be 16-byte aligned"),
                     (dict(sb=8191), "scratch_bytes 8191 is below the 8192")):
        assert rec(**kw) == capi.AIM_EINVAL and _err().startswith("aim_map_records_contigs_device: ") and text in _err(), (kw, _err())


def test_contig_kernels_code_objects():
    """Each new kernel exists exactly once, uses no scratch and stays within kContigMaxVgpr; the clip's LDS is its 4 KB table."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_regs
    lib = os.path.join(ROOT, "aim_amd", "libaim_hip.so")
    if not os.path.exists(lib):
        pytest.fail("libaim_hip.so is missing: run the build")
    regs = codeobj_regs.kernel_regs(lib)
    bound = int(re.search(r"constexpr int kContigMaxVgpr = (\d+);", open(os.path.join(ROOT, "aim_amd", "csrc", "contig.hpp")).read()).group(1))
    lds = {"contig_clip_kernel": 4096, "map_records_contig_kernel": 0}
    for name in _lib().aim_contig_kernel_names().decode().split(","):
        found = [n for n in regs if re.search(r"\baim::%s\(" % name, n)]
        assert len(found) == 1, (name, found)
        r = regs[found[0]]
        print(name, r)
        assert r["scratch_bytes"] == 0 and r["lds_static_bytes"] == lds[name] and 0 < r["vgpr"] + r["agpr"] <= bound <= 512 // 8, (name, r, bound)


# ---- samout --------------------------------------------------------------------------------------------------------------------------
def _two_contig_records():
    from aim_amd import capi
    from mapper_batch import record as _record
    M, S = 0, 4
    w = lambda n, op: (n << 4) | op
    cigar, md = [], []
    recs = [_record(0, 0, 1, 0, 99, 60, 1, 3, [w(8, M)], "3A4", cigar, md),
            _record(1, 0, 1, 4, 0, 0, 0, 77, [], "", cigar, md),
            _record(2, 0, 2, 16, 899, 50, 0, 0, [w(4, M), w(6, S)], "4", cigar, md),
            _record(2, 1, 2, 0x800, 4, 20, 0, 0, [w(4, S), w(6, M)], "6", cigar, md),
            _record(3, 0, 1, 16, 0, 37, 0, 0, [w(2, S), w(5, M)], "5", cigar, md)]
    for rec, pad in zip(recs, (0, capi.CONTIG_NONE, 0, 1, 1)):
        rec["sam"]["pad"] = pad
    out = {"records": np.array(recs, dtype=capi.MAP_RECORD_DTYPE), "rec_offsets": np.array([0, 1, 2, 4, 5], dtype=np.uint32),
           "cigar": np.array(cigar, dtype=np.uint32), "md": np.frombuffer(bytes(md), dtype=np.uint8)}
    return out, ["fwd", "none", "split", "rev"], [b"ACGTACGT", b"TTTT", b"AAAACCCCGG", b"GATTACA"], [8, 4, 10, 7], ["IIIIHHHH", "!!!!", None, None]


def test_samout_two_contigs_whole_text():
    """One @SQ per contig, RNAME from the record's pad, and a split read whose halves lie on different contigs: each SA entry names
    its own record's contig."""
    from aim_amd import samout
    out, names, reads, lens, quals = _two_contig_records()
    text = samout.header(["chrA", "chrB"], [5000, 70], command_line="cmd --contigs") + \
        "".join(l + "\n" for l in samout.record_lines(out, names, reads, lens, ["chrA", "chrB"], quals))
    assert text == (
        "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chrA\tLN:5000\n@SQ\tSN:chrB\tLN:70\n@PG\tID:aim_amd\tPN:aim_amd\tVN:1\tCL:cmd --contigs\n"
        "fwd\t0\tchrA\t100\t60\t8M\t*\t0\t0\tACGTACGT\tIIIIHHHH\tNM:i:1\tMD:Z:3A4\tAS:i:-3\n"
        "none\t4\t*\t0\t0\t*\t*\t0\t0\tTTTT\t!!!!\n"
        "split\t16\tchrA\t900\t50\t4M6S\t*\t0\t0\tCCGGGGTTTT\t*\tNM:i:0\tMD:Z:4\tAS:i:0\tSA:Z:chrB,5,+,4S6M,20,0;\n"
        "split\t2048\tchrB\t5\t20\t4S6M\t*\t0\t0\tAAAACCCCGG\t*\tNM:i:0\tMD:Z:6\tAS:i:0\tSA:Z:chrA,900,-,4M6S,50,0;\n"
        "rev\t16\tchrB\t1\t37\t2S5M\t*\t0\t0\tTGTAATC\t*\tNM:i:0\tMD:Z:5\tAS:i:0\n")


def test_samout_with_one_name_is_unchanged():
    """A str where the list goes gives the text it always gave: the pad is not looked at."""
    from aim_amd import samout
    out, names, reads, lens, quals = _two_contig_records()
    assert samout.header("chrT", 5000, command_line="c") == "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chrT\tLN:5000\n@PG\tID:aim_amd\tPN:aim_amd\tVN:1\tCL:c\n"
    assert samout.header("chrT", 5000) == samout.header(["chrT"], [5000])
    lines = samout.record_lines(out, names, reads, lens, "chrT", quals)
    zero = dict(out, records=out["records"].copy())
    zero["records"]["sam"]["pad"] = 0
    assert lines == samout.record_lines(zero, names, reads, lens, "chrT", quals) == samout.record_lines(zero, names, reads, lens, ["chrT"], quals)
    assert lines[2].split("\t")[2] == "chrT" and lines[2].endswith("SA:Z:chrT,5,+,4S6M,20,0;")


# ---- the readers and the command line ------------------------------------------------------------------------------------------------
def test_load_contigs_and_the_switch(tmp_path):
    from aim_amd import map as amap
    fa = tmp_path / "two.fa"
    fa.write_bytes(b">a first\nACgt\nnn\n>b\nGGCC\n")
    names, seqs = amap.load_contigs(str(fa))
    assert names == ["a", "b"] and [s.tobytes() for s in seqs] == [b"ACGTNN", b"GGCC"] and seqs[0].dtype == np.uint8
    one = tmp_path / "one.fa"
    one.write_bytes(b">chr\nacgt\n")
    assert amap.load_contigs(str(one))[0] == ["chr"] and amap.load_reference(str(one))[1].tobytes() == b"ACGT"
    bad = tmp_path / "bad.fa"
    bad.write_bytes(b">a\nAC\n>empty\n")
    with pytest.raises(ValueError, match="'empty' is empty"):
        amap.load_contigs(str(bad))
    bad.write_bytes(b"")
    with pytest.raises(ValueError, match="holds no sequence"):
        amap.load_contigs(str(bad))
    assert amap.parser().parse_args(["--ref", "r", "--reads", "q", "-o", "o", "--contigs"]).contigs
    assert not amap.parser().parse_args(["--ref", "r", "--reads", "q", "-o", "o"]).contigs
    # without the switch the refusal stands, and now says what to do
    fq = tmp_path / "r.fq"
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    p = subprocess.run([sys.executable, "-m", "aim_amd.map", "--ref", str(fa), "--reads", str(fq), "-o", str(tmp_path / "o.sam")], cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 2 and "holds 2 sequences" in p.stderr and "contig table" in p.stderr and "--contigs" in p.stderr and not (tmp_path / "o.sam").exists(), p.stderr
    # with it the reader's own refusals come back the same way, before any device
    p = subprocess.run([sys.executable, "-m", "aim_amd.map", "--contigs", "--ref", str(bad), "--reads", str(fq), "-o", str(tmp_path / "o.sam")], cwd=ROOT,
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "holds no sequence" in p.stderr and not (tmp_path / "o.sam").exists(), p.stderr


# ---- the premises of the GPU batch ---------------------------------------------------------------------------------------------------
def test_batch_premises_on_the_models():
    """At the two cut points no slot of the shared 73 reads is clipped (the cap on records left out of the GPU comparison is zero), every
    read keeps the segments it has on the uncut reference, and the planted reads do what they are there for: one clipped segment each
    on the right contig, two unclipped ones on contigs 0 and 1 for the junction read, and an ends-free cost within MAX_SCORE."""
    import chain_class_model as ccm
    import contig_model as cg
    import endsfree_model as ef
    import mapper_batch as mb
    import seed_model as m
    import split_model as sm
    mo = cg.batch_models()
    K, nb, flank, rs = mo["K"], mo["n_batch"], mo["flank"], ccm.CHIMERIC_SIZE
    assert nb == 73 and len(mo["read_len"]) == nb + cg.N_PLANTED and mo["starts"].tolist() == [0, cg.CUTS[0] + 160, cg.CUTS[1] + 320]
    seg0, seg1 = mo["split"][3], mo["clip"]["seg"]
    valid = ((seg0["flags"] & sm.VALID) != 0).reshape(-1, K)
    clipped = ((seg1["flags"] & cg.CLIPPED) != 0).reshape(-1, K)
    assert not clipped[:nb].any()
    assert valid[:nb].sum(axis=1).tolist() == [2] * mb.N_CHIMERIC + [1] * mb.N_UNBROKEN + [0] * mb.N_RANDOM
    for name, i in (("seg_req", 0), ("seg_text_pos", 1)):
        assert mo["clip"][name][:nb * K].tobytes() == mo["split"][i][:nb * K].tobytes()
    # every segment of the batch lies on the contig its truth says
    b = mb.batch()
    contig = mo["clip"]["contig"].reshape(-1, K)
    for r in range(mb.N_CHIMERIC + mb.N_UNBROKEN):
        for i in np.nonzero(valid[r])[0]:
            sg = seg0[r * K + i]
            lo = sm.half_of(b["halves"][r], int(sg["q_begin"]), int(sg["q_end"]))["ref_lo"] if r < mb.N_CHIMERIC else b["truth"][r - mb.N_CHIMERIC][0]
            assert contig[r, i] == cg.to_concat(lo)[0], (r, i)
    # the planted reads
    one = [[1, 0, 0, 0]]
    assert valid[nb:].astype(int).tolist() == one * 4 + [[1, 1, 0, 0]] + one * 2 and clipped[nb:].astype(int).tolist() == one * 4 + [[0] * 4] + one * 2
    assert contig[nb:, 0].tolist() == [1, 0, 1, 0, 1, 1, 0] and contig[nb + 4, 1] == 0
    cat = mo["concat"]
    L = mo["read_len"]
    assert mo["rows"][nb, 0] != cat[mo["starts"][1]] and mo["rows"][nb + 1, L[nb + 1] - 1] != cat[mo["starts"][0] + mo["lens"][0] - 1]   # one place for the run of 24
    assert mo["rows"][nb + 2, :L[nb + 2]].tobytes() == m.revcomp(mo["rows"][nb, :L[nb]]).tobytes() and L[nb:].tolist() == [324] * 4 + [600, 301, 301]
    assert mo["rows"][nb + 5, 0] != cat[mo["starts"][1]] and mo["rows"][nb + 6, 300] != cat[mo["starts"][0] + mo["lens"][0] - 1]
    rows = []
    for slot in [(nb + j) * K for j in (0, 1, 2, 3, 5, 6, 4)] + [(nb + 4) * K + 1]:
        tp, tl = int(mo["clip"]["seg_text_pos"][slot]), int(mo["clip"]["seg_req"]["text_len"][slot])
        s, c = tp & (cg.MINUS - 1), int(mo["clip"]["contig"][slot])
        assert int(mo["starts"][c]) <= s and s + tl <= int(mo["starts"][c]) + int(mo["lens"][c])
        text = cat[s:s + tl]
        rows.append((mo["split"][2][slot][:int(mo["clip"]["seg_req"]["pattern_len"][slot])], m.revcomp(text) if tp >> 63 else text))
    req = np.zeros(len(rows), dtype=m.REQUEST)
    pat, txt = np.zeros((len(rows), rs), dtype=np.uint8), np.zeros((len(rows), rs), dtype=np.uint8)
    for i, (p, t) in enumerate(rows):
        req[i] = (len(p), len(t), 0, i)
        pat[i, :len(p)], txt[i, :len(t)] = p, t
    cost = ef.dp_scores(req, pat, txt, mb.X, mb.O, mb.E, ends_free=(0, 0, 2 * flank, 2 * flank))
    print("ends-free costs of the planted segments", cost.tolist(), "MAX_SCORE", mb.max_score())
    assert (cost <= mb.max_score()).all() and (cost[:4] == mb.O + cg.PLANT_TAIL * mb.E).all() and (cost[4:6] == mb.O + mb.E).all() and (cost[6:] == 0).all()
    # and over the spacer, as the one-sequence mapper aligns them: the gap stays the cheaper end for 24 bases, the mismatch for one
    assert cg.PLANT_TAIL * mb.X > mb.O + cg.PLANT_TAIL * mb.E and mb.X < mb.O + mb.E
