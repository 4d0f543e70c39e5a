"""The mapper without a GPU: rule 12c's numpy model on random slot tables, every refusal of aim_mapper_device_bytes, aim_mapper_create and
aim_map_records_device by message (each condition alone, none of them needs a device), aim_amd.samout on hand-made records with the
whole text compared, the FASTA / FASTQ readers and the multi-sequence refusal of python -m aim_amd.map, the code objects of the two new
kernels, and the shared batch's premises on the chain model."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mapper_batch import REFUSALS, params_with as _params, record as _record  # noqa: E402
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
    import map_records_model as mm
    assert _define("AIM_FEATURE_MAPPER") == capi.FEATURE_MAPPER == 0x80000 and engine.features() & capi.FEATURE_MAPPER
    assert _lib().aim_abi_version() == 2 and _define("AIM_MAP_EXTEND") == capi.MAP_EXTEND and _define("AIM_MAPPER_MAX_SLOTS") == capi.MAPPER_MAX_SLOTS
    assert capi.MAP_RECORD_DTYPE == mm.RECORD_DTYPE and capi.SAM_DTYPE == mm.SAM_DTYPE and capi.SEGMENT_DTYPE == mm.SEG_DTYPE
    assert mm.RECORD_DTYPE.fields["read"][1] == 48 and mm.RECORD_DTYPE.fields["mapq"][1] == 56 and mm.RECORD_DTYPE.fields["slot"][1] == 60
    assert _lib().aim_mapper_kernel_names() == b"map_count_kernel,map_records_kernel"
    assert engine.map_records_scratch(0) == engine.map_records_scratch(1 << 20) == 8192


@pytest.mark.parametrize("K", (1, 4, 16))
def test_model_properties(K):
    import map_records_model as mm
    n = 301
    seg, sam, cls = mm.synthetic_tables(5, K, n)
    off, rec = mm.map_records(K, n, seg, sam, cls)
    mapped = mm.mapped_slots(K, n, seg, sam)
    counts = np.maximum(mapped.sum(axis=1), 1)
    assert off[0] == 0 and np.array_equal(np.diff(off.astype(np.int64)), counts) and off[n] == len(rec)
    assert not mapped[0].any() and mapped[1].all() and (K == 1 or (not mapped[2, 0] and mapped[2, K - 1]))
    assert (sam["status"][3 * K:4 * K] & mm.SAM_OVERFLOW).all() and mapped[3].all()          # an OVERFLOW row is mapped
    seen = {"unmapped": 0, "multi": 0, "ties": 0, "moved": 0}
    for r in range(n):
        g = rec[off[r]:off[r + 1]]
        assert (g["read"] == r).all() and (g["n_records"] == len(g)).all()
        if not mapped[r].any():
            seen["unmapped"] += 1
            o, row = g[0], sam[r * K]
            assert len(g) == 1 and o["sam"]["flags"] == mm.SAM_UNMAPPED and o["slot"] == r * K
            assert (o["sam"]["idx"], o["sam"]["score"], o["sam"]["status"], o["sam"]["pad"]) == (row["idx"], row["score"], row["status"], row["pad"])
            for f in ("pos", "ref_span", "nm", "n_cigar", "md_len", "cigar_offset", "md_offset"):
                assert o["sam"][f] == 0, f
            assert (o["q_begin"], o["q_end"], o["mapq"], o["seg_flags"], o["rank"]) == (0, 0, 0, 0, 0)
            continue
        assert sorted(g["rank"].tolist()) == list(range(len(g))) and g["rank"].tolist() == list(range(len(g)))     # a permutation, stored in rank order
        assert sorted(g["slot"].tolist()) == [r * K + i for i in range(K) if mapped[r, i]]
        primary = (g["sam"]["flags"] & mm.SAM_SUPPLEMENTARY) == 0
        assert primary.sum() == 1 and g["slot"][primary][0] == g["slot"].min()                 # one non-supplementary line: the lowest candidate
        keys = [(int(q), int(s)) for q, s in zip(g["q_begin"], g["slot"])]
        assert keys == sorted(keys)
        seen["multi"] += len(g) > 1
        seen["ties"] += len(set(g["q_begin"].tolist())) < len(g)
        seen["moved"] += int(g["slot"][0] != g["slot"].min())
        for o in g:
            s = int(o["slot"])
            want = sam[s].copy()
            want["flags"] = o["sam"]["flags"]
            assert o["sam"].tobytes() == want.tobytes() and (int(sam["flags"][s]) ^ int(o["sam"]["flags"])) & ~mm.SAM_SUPPLEMENTARY == 0
            assert (o["mapq"], o["q_begin"], o["q_end"], o["seg_flags"]) == (cls["mapq"][s], seg["q_begin"][s], seg["q_end"][s], seg["flags"][s])
    assert seen["unmapped"] >= 1 and (K == 1 or (seen["multi"] > 20 and seen["ties"] > 5 and seen["moved"] > 5)), seen


@pytest.mark.parametrize("case", REFUSALS, ids=lambda c: "-".join("%s=%s" % kv for kv in c[0].items()))
def test_mapper_refusals_need_no_device(case):
    """Each condition alone, from aim_mapper_device_bytes and from aim_mapper_create, under that entry point's name, before any device
    query (aim_mapper_create would answer AIM_ENODEV here otherwise)."""
    from aim_amd import capi
    lib = _lib()
    kw, text = case
    mp = _params(**kw)
    b = C.c_uint64(0)
    assert lib.aim_mapper_device_bytes(C.byref(mp), 1 << 20, C.byref(b)) == capi.AIM_EINVAL
    assert _err().startswith("aim_mapper_device_bytes: ") and text in _err(), _err()
    h = C.c_void_p()
    seq = np.zeros(16, dtype=np.uint8)
    assert lib.aim_mapper_create(C.byref(mp), 0, capi.ptr(seq), 16, C.byref(h)) == capi.AIM_EINVAL and not h.value
    assert _err().startswith("aim_mapper_create: ") and text in _err(), _err()


def test_mapper_refusals_of_the_arguments_and_an_accepted_set():
    from aim_amd import capi, engine
    lib = _lib()
    b = C.c_uint64(0)
    mp = _params()
    assert lib.aim_mapper_device_bytes(None, 0, C.byref(b)) == capi.AIM_EINVAL and _err() == "aim_mapper_device_bytes: params is NULL"
    assert lib.aim_mapper_device_bytes(C.byref(mp), 0xFE000001, C.byref(b)) == capi.AIM_EINVAL and "ref_len 4261412865 is above" in _err()
    assert lib.aim_mapper_device_bytes(C.byref(mp), 1 << 20, None) == capi.AIM_EINVAL and _err() == "aim_mapper_device_bytes: bytes is NULL"
    assert lib.aim_mapper_create(C.byref(mp), 0, None, 16, None) == capi.AIM_EINVAL and _err() == "aim_mapper_create: mapper is NULL"
    h = C.c_void_p()
    assert lib.aim_mapper_create(C.byref(mp), 0, None, 16, C.byref(h)) == capi.AIM_EINVAL and _err() == "aim_mapper_create: seq is NULL"
    # the extension's parameters are read under AIM_MAP_EXTEND alone
    off = _params(options=0, ext_band=99)
    assert lib.aim_mapper_device_bytes(C.byref(off), 1 << 20, C.byref(b)) == 0 and b.value > 0
    small, large = engine.mapper_device_bytes(_params(slots=1), 1 << 20), engine.mapper_device_bytes(_params(slots=4), 1 << 20)
    assert 0 < small < large and engine.mapper_device_bytes(_params(slots=4), 1 << 24) > large
    assert lib.aim_mapper_submit(None, 0, 0, None, None) == capi.AIM_EINVAL and lib.aim_mapper_wait(None, 0, None) == capi.AIM_EINVAL
    assert lib.aim_mapper_free(None) == 0


def test_map_records_refusals_need_no_device():
    from aim_amd import capi
    lib = _lib()
    ok = 1 << 12           # any aligned address: nothing is dereferenced before the device probe
    call = lambda K=4, n=8, seg=ok, sam=ok, cls=ok, off=ok, rec=ok, scr=ok, sb=8192: lib.aim_map_records_device(K, n, seg, sam, cls, off, rec, scr, sb, None)
    for kw, text in ((dict(K=0), "K 0 is outside 1..16"), (dict(K=17), "K 17 is outside 1..16"), (dict(K=16, n=1 << 28), "n_reads 268435456 * K 16 does not fit 32 bits"),
                     (dict(off=None), "d_rec_offsets is NULL"), (dict(off=None, n=0), "d_rec_offsets is NULL"), (dict(seg=None), "null device buffer"),
                     (dict(sam=None), "null device buffer"), (dict(cls=None), "null device buffer"), (dict(rec=None), "null device buffer"),
                     (dict(scr=None), "null device buffer"), (dict(sam=ok + 8), "d_sam and d_records must be 16-byte aligned"),
                     (dict(rec=ok + 4), "d_sam and d_records must be 16-byte aligned"), (dict(sb=8191), "scratch_bytes 8191 is below the 8192")):
        assert call(**kw) == capi.AIM_EINVAL and _err().startswith("aim_map_records_device: ") and text in _err(), (kw, _err())


def test_map_kernels_code_objects():
    """Each new kernel exists exactly once, uses no scratch and no static LDS and stays within kMapMaxVgpr."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_regs
    lib = os.path.join(ROOT, "aim_amd", "libaim_hip.so")
    if not os.path.exists(lib):
        pytest.fail("libaim_hip.so is missing: run the build")
    regs = codeobj_regs.kernel_regs(lib)
    bound = int(re.search(r"constexpr int kMapMaxVgpr = (\d+);", open(os.path.join(ROOT, "aim_amd", "csrc", "mapper.hpp")).read()).group(1))
    for name in _lib().aim_mapper_kernel_names().decode().split(","):
        found = [n for n in regs if re.search(r"\baim::%s\(" % name, n)]
        assert len(found) == 1, (name, found)
        r = regs[found[0]]
        print(name, r)
        assert r["scratch_bytes"] == 0 and r["lds_static_bytes"] == 0 and 0 < r["vgpr"] + r["agpr"] <= bound <= 512 // 8, (name, r, bound)


# ---- samout ----------------------------------------------------------------------------------------------------------------------
def test_samout_whole_text():
    """A forward read, a reverse read, an unmapped read and a two-record read (the supplementary line first in rank order, so the SA
    tags show the non-supplementary sibling first)."""
    from aim_amd import capi, samout
    M, I, D, S = 0, 1, 2, 4
    w = lambda n, op: (n << 4) | op
    cigar, md = [], []
    recs = [_record(0, 0, 1, 0, 99, 60, 1, 3, [w(8, M)], "3A4", cigar, md),
            _record(1, 0, 1, 16, 199, 37, 2, 8, [w(2, S), w(3, M), w(1, D), w(3, M)], "3^C3", cigar, md),
            _record(2, 0, 1, 4, 0, 0, 0, 77, [], "", cigar, md),
            _record(3, 0, 3, 0x800, 499, 20, 0, 0, [w(4, M), w(6, S)], "4", cigar, md),
            _record(3, 1, 3, 16, 899, 50, 1, 5, [w(4, S), w(2, M), w(1, I), w(1, M), w(2, S)], "3", cigar, md),
            _record(3, 2, 3, 0x800 | 16, 1299, 7, 0, 0, [w(8, S), w(2, M)], "2", cigar, md, status=0),
            _record(4, 0, 1, 0, 9, 11, 0, 0, [], "", cigar, md, status=capi.SAM_OVERFLOW)]
    out = {"records": np.array(recs, dtype=capi.MAP_RECORD_DTYPE), "rec_offsets": np.array([0, 1, 2, 3, 6, 7], dtype=np.uint32),
           "cigar": np.array(cigar, dtype=np.uint32), "md": np.frombuffer(bytes(md), dtype=np.uint8)}
    names = ["fwd", "rev", "none", "split", "over"]
    reads = [b"ACGTACGTNN", b"AACCGGTT", b"TTTT", b"AAAACCCCGG", b"GATTACA"]
    lens = [8, 8, 4, 10, 7]
    quals = ["IIIIHHHH", None, "!!!!", "0123456789", None]
    text = samout.header("chrT", 5000, command_line="cmd --x") + "".join(l + "\n" for l in samout.record_lines(out, names, reads, lens, "chrT", quals))
    assert text == (
        "@HD\tVN:1.6\tSO:unsorted\n@SQ\tSN:chrT\tLN:5000\n@PG\tID:aim_amd\tPN:aim_amd\tVN:1\tCL:cmd --x\n"
        "fwd\t0\tchrT\t100\t60\t8M\t*\t0\t0\tACGTACGT\tIIIIHHHH\tNM:i:1\tMD:Z:3A4\tAS:i:-3\n"
        "rev\t16\tchrT\t200\t37\t2S3M1D3M\t*\t0\t0\tAACCGGTT\t*\tNM:i:2\tMD:Z:3^C3\tAS:i:-8\n"
        "none\t4\t*\t0\t0\t*\t*\t0\t0\tTTTT\t!!!!\n"
        "split\t2048\tchrT\t500\t20\t4M6S\t*\t0\t0\tAAAACCCCGG\t0123456789\tNM:i:0\tMD:Z:4\tAS:i:0\tSA:Z:chrT,900,-,4S2M1I1M2S,50,1;chrT,1300,-,8S2M,7,0;\n"
        "split\t16\tchrT\t900\t50\t4S2M1I1M2S\t*\t0\t0\tCCGGGGTTTT\t9876543210\tNM:i:1\tMD:Z:3\tAS:i:-5\tSA:Z:chrT,500,+,4M6S,20,0;chrT,1300,-,8S2M,7,0;\n"
        "split\t2064\tchrT\t1300\t7\t8S2M\t*\t0\t0\tCCGGGGTTTT\t9876543210\tNM:i:0\tMD:Z:2\tAS:i:0\tSA:Z:chrT,900,-,4S2M1I1M2S,50,1;chrT,500,+,4M6S,20,0;\n"
        "over\t0\tchrT\t10\t11\t*\t*\t0\t0\tGATTACA\t*\tNM:i:0\tAS:i:0\n")
    assert samout.revcomp(b"ACGTNacgt") == b"acgtNACGT"


# ---- readers and the command line --------------------------------------------------------------------------------------------------
def test_fasta_and_fastq_readers(tmp_path):
    from aim_amd import map as amap
    fa = tmp_path / "r.fa"
    fa.write_bytes(b">one first sequence\nACGT\nacgtn\n\n>two\nGG\n>empty\n")
    assert amap.read_fasta(str(fa)) == [("one", b"ACGTacgtn"), ("two", b"GG"), ("empty", b"")]
    fq = tmp_path / "r.fq"
    fq.write_bytes(b"@a x/1\nACGT\n+\nIIII\n@b\nGGC\n+b\n!!#\r\n")
    assert amap.read_fastq(str(fq)) == [("a", b"ACGT", "IIII"), ("b", b"GGC", "!!#")]
    assert amap.read_reads(str(fq)) == amap.read_fastq(str(fq)) and amap.read_reads(str(fa))[0] == ("one", b"ACGTacgtn", None)
    bad = tmp_path / "bad.fq"
    bad.write_bytes(b"@a\nACGT\n+\nIII\n")
    with pytest.raises(ValueError, match="4 bases and 3 qualities"):
        amap.read_fastq(str(bad))
    bad.write_bytes(b"@a\nACGT\n+\n")
    with pytest.raises(ValueError, match="four-line"):
        amap.read_fastq(str(bad))
    bad.write_bytes(b"ACGT\n")
    with pytest.raises(ValueError, match="neither FASTA"):
        amap.read_reads(str(bad))
    with pytest.raises(ValueError, match="before the first"):
        amap.read_fasta(str(bad))
    one = tmp_path / "one.fa"
    one.write_bytes(b">chr\nacgtNN\nAC\n")
    name, ref = amap.load_reference(str(one))
    assert name == "chr" and ref.tobytes() == b"ACGTNNAC"


def test_multi_sequence_reference_is_refused(tmp_path):
    """By the reader and by the command line, which stops before it touches a device."""
    from aim_amd import map as amap
    fa = tmp_path / "two.fa"
    fa.write_bytes(b">a\nACGT\n>b\nGGCC\n")
    with pytest.raises(ValueError, match="holds 2 sequences"):
        amap.load_reference(str(fa))
    fq = tmp_path / "r.fq"
    fq.write_bytes(b"@r\nACGT\n+\nIIII\n")
    p = subprocess.run([sys.executable, "-m", "aim_amd.map", "--ref", str(fa), "--reads", str(fq), "-o", str(tmp_path / "o.sam")], cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert p.returncode == 2 and "holds 2 sequences" in p.stderr and "contig table" in p.stderr and not (tmp_path / "o.sam").exists(), p.stderr


# ---- the premises of the shared batch ----------------------------------------------------------------------------------------------
def test_batch_premises_on_the_chain_model():
    """The seed parameters give the 8 random reads no chain and every unbroken read exactly one segment."""
    import chain_class_model as ccm
    import mapper_batch as mb
    import split_model as sm
    from pipeline_batches import expected, reference
    ref = reference()
    rows, rl = mb.random_reads()
    assert (expected(ccm.CHIMERIC_ROW, rows, rl, ("mapper random", mb.RANDOM_SEED), read_size=ccm.CHIMERIC_SIZE)[3]["n_cands"] == 0).all()
    rows, rl, truth = mb.unbroken_reads(ref)
    req, tpos, votes, seeds, chains = expected(ccm.CHIMERIC_ROW, rows, rl, "mapper unbroken", read_size=ccm.CHIMERIC_SIZE)
    K, flank = ccm.CHIMERIC_ROW[7], ccm.CHIMERIC_ROW[5]
    cls = ccm.classify(K, ccm.CHIMERIC_SIZE, 128, rl, tpos, seeds, chains)
    seg = sm.segments(K, ccm.CHIMERIC_SIZE, flank, len(ref), rl, rows, req, tpos, seeds, chains, cls)[3]
    assert (((seg["flags"] & sm.VALID) != 0).reshape(-1, K).sum(axis=1) == 1).all()
    b = mb.batch()
    assert b["rows"].shape == (73, 1024) and len(b["read_len"]) == 73 and set(t[2] for t in truth) == {0, 1}
