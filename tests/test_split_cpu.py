"""Split reads without a GPU: rule 10c by hand on tests/split_model.py, the sam_split model on hand-made records, the ABI values,
symbols and struct layout, every refusal of aim_split_segments_device by message (the checks come before any device query), what the
shared batches hold, what the model gives on the chimeric reads, and the code objects of the new kernels next to the unchanged ones."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aim_hip.h")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

P, S, X = 1, 2, 4                      # aim_chain_class_t.flags: primary, secondary, supplementary
RS, FLANK, REF_LEN = 1024, 16, 100000


def _lib():
    from aim_amd import capi
    return capi.load()


def _err():
    return _lib().aim_last_error().decode()


def _define(name):
    m = re.search(r"#define\s+%s\s+(\S+)" % name, open(HEADER).read())
    return int(m.group(1).rstrip("uUlL"), 0)


def _one_read(cands, L=1000, read_size=RS, flank=FLANK, ref_len=REF_LEN, n_cands=None, row=None):
    """The model over one read whose slots are (q_lo, q_hi, strand, start, text_len, ref_span, class flags). Returns
    (requests, text_pos, patterns, segments, the read row)."""
    import chain_model as cm
    import seed_model as m
    import split_model as sm
    import chain_class_model as ccm
    K = len(cands)
    ch, tp, sd = np.zeros(K, dtype=cm.CHAIN), np.zeros(K, dtype=np.uint64), np.zeros(1, dtype=m.SEED)
    req, cls = np.zeros(K, dtype=m.REQUEST), np.zeros(K, dtype=ccm.CLASS)
    for i, (lo, hi, s, start, tlen, span, fl) in enumerate(cands):
        ch[i] = (100 - i, 5, 0, lo, hi, span)
        tp[i] = np.uint64(start | (s << 63))
        req[i] = (L, tlen, 0, 7000 + i)
        cls[i]["flags"] = fl
    sd["n_cands"] = K if n_cands is None else n_cands
    row = (np.arange(read_size) % 251 + 1).astype(np.uint8) if row is None else row
    out = sm.segments(K, read_size, flank, ref_len, np.array([L], dtype=np.int32), row[None, :], req, tp, sd, ch, cls)
    return out + (row,)


def _window(lo, hi, L, p_lo, span, flank=FLANK, read_size=RS, ref_len=REF_LEN):
    """Rule 6c for a chain (q_lo, q_hi, p_lo, span): (start, text_len)."""
    w_lo, w_hi = p_lo - lo - flank, p_lo + span + (L - hi) + flank
    start = max(w_lo, 0)
    end = max(start, min(w_hi, ref_len))
    return start, min(end - start, read_size)


def test_sole_primary_is_the_identity():
    import split_model as sm
    for s in (0, 1):
        start, tlen = _window(100, 900, 1000, 5000, 805)
        row = np.zeros(RS, dtype=np.uint8)
        row[:1000] = np.arange(1000) % 251 + 1                                 # zero behind L, as the chain tests' rows are
        req, tp, pat, seg, row = _one_read([(100, 900, s, start, tlen, 805, P), (0, 0, 0, 0, 0, 0, 0)], n_cands=1, row=row)
        assert tuple(req[0]) == (1000, tlen, 0, 7000) and int(tp[0]) == start | (s << 63) and pat[0].tobytes() == row.tobytes()
        assert tuple(seg[0]) == (0, 1000, 1000, sm.VALID | sm.LEFT_OPEN | sm.RIGHT_OPEN, 0)
        # the empty slot: rule 7's, with the whole read row
        assert tuple(req[1]) == (1000, 0, 0, 7001) and int(tp[1]) == 0 and pat[1].tobytes() == row.tobytes() and seg[1].tobytes() == bytes(8)


def test_two_primaries_same_strand():
    import split_model as sm
    L = 800
    w0, w1 = _window(0, 390, L, 5000, 392), _window(410, 800, L, 30000, 388)
    req, tp, pat, seg, row = _one_read([(0, 390, 0, w0[0], w0[1], 392, P), (410, 800, 0, w1[0], w1[1], 388, P | X)], L=L)
    # candidate 0 is left-open: from the read's start to where its chain stops; its window keeps the low flank and ends at p_hi
    assert tuple(seg[0]) == (0, 390, L, sm.VALID | sm.LEFT_OPEN, 0) and tuple(req[0]) == (390, 5392 - w0[0], 0, 7000) and int(tp[0]) == w0[0] == 5000 - FLANK
    assert pat[0, :390].tobytes() == row[:390].tobytes() and not pat[0, 390:].any()
    # candidate 1 is right-open: from where its chain starts to the read's end; its window starts at p_lo and keeps the high flank
    assert tuple(seg[1]) == (410, L, L, sm.VALID | sm.SUPPLEMENTARY | sm.RIGHT_OPEN, 1)
    assert int(tp[1]) == 30000 and tuple(req[1]) == (390, w1[0] + w1[1] - 30000, 0, 7001) and w1[0] + w1[1] == 30388 + FLANK
    assert pat[1, :390].tobytes() == row[410:800].tobytes() and not pat[1, 390:].any()


def test_two_primaries_opposite_strands():
    import split_model as sm
    L = 800
    # candidate 1 is on strand 1: its chain-query interval [0, 390) is the read's [410, 800), and the read's right side is its window's LOW side
    w0, w1 = _window(0, 390, L, 5000, 392), _window(0, 390, L, 30000, 388)
    req, tp, pat, seg, row = _one_read([(0, 390, 0, w0[0], w0[1], 392, P), (0, 390, 1, w1[0], w1[1], 388, P | X)], L=L)
    assert tuple(seg[0]) == (0, 390, L, sm.VALID | sm.LEFT_OPEN, 0)
    assert tuple(seg[1]) == (410, L, L, sm.VALID | sm.SUPPLEMENTARY | sm.RIGHT_OPEN, 1)
    # right-open on strand 1 is low-open: the window starts at the candidate's start (flank kept) and ends at p_hi
    assert int(tp[1]) == (30000 - FLANK) | (1 << 63) and tuple(req[1]) == (390, 30388 - (30000 - FLANK), 0, 7001)
    assert pat[1, :390].tobytes() == row[410:800].tobytes()             # as given: no complement
    # and the other way round: the strand-1 chain first in the read
    req, tp, pat, seg, row = _one_read([(410, 800, 1, w0[0], w0[1], 392, P), (410, 800, 0, w1[0], w1[1], 388, P | X)], L=L)
    assert tuple(seg[0]) == (0, 390, L, sm.VALID | sm.LEFT_OPEN, 0) and tuple(seg[1]) == (410, L, L, sm.VALID | sm.SUPPLEMENTARY | sm.RIGHT_OPEN, 1)


def test_three_primaries_and_a_secondary_between():
    import split_model as sm
    L = 900
    c = [(0, 290, 0, 5000, 292), (310, 590, 0, 30000, 281), (610, 900, 0, 50000, 290)]
    w = [_window(lo, hi, L, p, sp) for lo, hi, _, p, sp in c]
    # slot 1 is a secondary (a repeat copy of the middle part) between the primaries 0 and 2 in rank; rank 2 is the middle of the read
    cands = [(0, 290, 0, w[0][0], w[0][1], 292, P), (320, 580, 0, 70000, 300, 260, S), (610, 900, 0, w[2][0], w[2][1], 290, P | X),
             (310, 590, 0, w[1][0], w[1][1], 281, P | X)]
    req, tp, pat, seg, row = _one_read(cands, L=L)
    assert tuple(seg[0]) == (0, 290, L, sm.VALID | sm.LEFT_OPEN, 0) and tuple(seg[2]) == (610, L, L, sm.VALID | sm.SUPPLEMENTARY | sm.RIGHT_OPEN, 2)
    # the middle one is closed on both sides: exactly the chain, read and reference, no flank
    assert tuple(seg[3]) == (310, 590, L, sm.VALID | sm.SUPPLEMENTARY, 3) and int(tp[3]) == 30000 and tuple(req[3]) == (280, 281, 0, 7003)
    assert pat[3, :280].tobytes() == row[310:590].tobytes() and not pat[3, 280:].any()
    # the secondary is an empty slot and does not close anybody's side
    assert seg[1].tobytes() == bytes(8) and tuple(req[1]) == (L, 0, 0, 7001) and int(tp[1]) == 0 and pat[1].tobytes() == row.tobytes()


def test_window_recovery_at_the_edges():
    import split_model as sm
    L = 800
    other = (0, 390, 0, 40000, 400, 392, P)
    # start == 0 because the left clamp acted (p_lo - q_lo - flank < 0); the right side is free: p_lo comes from E
    p_lo, span = 405, 388
    st, tl = _window(410, 800, L, p_lo, span)
    assert st == 0 and tl == p_lo + span + FLANK
    req, tp, pat, seg, _ = _one_read([other, (410, 800, 0, st, tl, span, P | X)], L=L)
    assert not seg[1]["flags"] & sm.LOOSE and int(tp[1]) == p_lo and tuple(req[1])[:2] == (390, span + FLANK)
    # start == 0 and text_len == read_size: the right side may have been capped -- not recoverable
    req, tp, pat, seg, _ = _one_read([other, (410, 800, 0, 0, RS, span, P | X)], L=L)
    assert seg[1]["flags"] & sm.LOOSE and int(tp[1]) == 0 and tuple(req[1])[:2] == (390, RS)
    # start == 0 and E == ref_len (a reference shorter than the window), and text_len == 0
    req, tp, pat, seg, _ = _one_read([other, (410, 800, 0, 0, 700, span, P | X)], L=L, ref_len=700)
    assert seg[1]["flags"] & sm.LOOSE and tuple(req[1])[:2] == (390, 700)
    req, tp, pat, seg, _ = _one_read([other, (410, 800, 0, 0, 0, span, P | X)], L=L)
    assert seg[1]["flags"] & sm.LOOSE and tuple(req[1])[:2] == (390, 0)
    # E == ref_len with start > 0: recoverable from the left; the open high side keeps E, a closed one is clamped to ref_len
    ref_len = 60000
    st, tl = _window(0, 390, L, 59500, 392, ref_len=ref_len)
    assert st + tl == ref_len
    req, tp, pat, seg, _ = _one_read([(0, 390, 0, st, tl, 392, P), (410, 800, 0, 100, 500, 388, P | X)], L=L, ref_len=ref_len)
    assert not seg[0]["flags"] & sm.LOOSE and int(tp[0]) == st and tuple(req[0])[:2] == (390, 59892 - st)
    st, tl = _window(0, 390, L, 59800, 392, ref_len=ref_len)        # p_hi beyond the reference: the closed side stops at ref_len
    req, tp, pat, seg, _ = _one_read([(0, 390, 0, st, tl, 392, P), (410, 800, 0, 100, 500, 388, P | X)], L=L, ref_len=ref_len)
    assert int(tp[0]) == st and tuple(req[0])[:2] == (390, ref_len - st)
    # text_len == read_size away from the edges (start > 0): recoverable, and the segment's own text_len is capped again
    req, tp, pat, seg, _ = _one_read([(0, 100, 0, 5000, RS, 2000, P), (410, 800, 0, 100, 500, 388, P | X)], L=L)
    assert not seg[0]["flags"] & sm.LOOSE and tuple(req[0])[:2] == (100, RS)
    # a malformed chain cannot leave the read
    req, tp, pat, seg, _ = _one_read([(0, 390, 0, 5000, 400, 392, P), (900, 1000, 0, 100, 500, 388, P | X)], L=L)
    assert tuple(seg[1])[:3] == (800, 800, 800) and req[1]["pattern_len"] == 0


def _records(rows):
    from aim_amd import capi
    rec = np.zeros(len(rows), dtype=capi.SAM_DTYPE)
    words = []
    for r, (flags, w) in enumerate(rows):
        rec[r]["idx"], rec[r]["score"], rec[r]["pos"], rec[r]["ref_span"], rec[r]["nm"] = 40 + r, 9, 1000 + r, 77, 3
        rec[r]["cigar_offset"], rec[r]["n_cigar"], rec[r]["flags"], rec[r]["md_len"] = len(words), len(w), flags, 5
        words += w
    return rec, np.array(words, dtype=np.uint32)


def test_sam_split_model_by_hand():
    import split_model as sm
    cg = lambda *p: [(n << 4) | "MIDNSHP=X".index(op) for n, op in p]
    seg = np.zeros(6, dtype=sm.SEGMENT)
    seg[0] = (0, 390, 800, sm.VALID | sm.LEFT_OPEN, 0)                      # trail 410
    seg[1] = (410, 800, 800, sm.VALID | sm.SUPPLEMENTARY | sm.RIGHT_OPEN, 1)  # lead 410
    seg[2] = (410, 800, 800, sm.VALID | sm.SUPPLEMENTARY | sm.RIGHT_OPEN, 1)  # strand 1: the lead becomes the trail
    seg[3] = (100, 700, 800, sm.VALID | sm.SUPPLEMENTARY, 2)                # both clips
    seg[5] = (0, 800, 800, sm.VALID | sm.LEFT_OPEN | sm.RIGHT_OPEN, 0)      # no clip at all
    tpos = np.array([5000, 30000, 30000 | (1 << 63), 7000 | (1 << 63), 0, 9000], dtype=np.uint64)
    rec, words = _records([(0, cg((390, "M"))), (0, cg((3, "S"), (380, "M"), (2, "I"), (5, "M"))), (0x10, cg((385, "M"), (5, "S"))),
                           (0x10, cg((4, "S"), (590, "M"), (6, "S"))), (0, cg((10, "M"))), (0, cg((2, "S"), (798, "M")))])
    out, w = sm.sam_split(rec, words, seg, tpos)
    assert w[0] == cg((390, "M"), (410, "S")) and out[0]["flags"] == 0 and out[0]["n_cigar"] == 2                 # a zero lead emits no word
    assert w[1] == cg((413, "S"), (380, "M"), (2, "I"), (5, "M")) and out[1]["flags"] == 0x800 and out[1]["n_cigar"] == 4   # merged with the S
    assert w[2] == cg((385, "M"), (415, "S")) and out[2]["flags"] == 0x810 and out[2]["n_cigar"] == 2             # swapped, merged
    assert w[3] == cg((104, "S"), (590, "M"), (106, "S")) and out[3]["n_cigar"] == 3                              # strand 1: lead 100, trail 100
    assert w[4] == [] and out[4]["flags"] == 4 and (out[4]["pos"], out[4]["ref_span"], out[4]["nm"], out[4]["n_cigar"], out[4]["md_len"]) == (0, 0, 0, 0, 0)
    assert out[4]["idx"] == 44 and out[4]["score"] == 9                                                           # an unmapped row keeps the row's own
    assert w[5] == cg((2, "S"), (798, "M")) and out[5].tobytes() == rec[5].tobytes()
    for r in (0, 1, 2, 3, 5):
        assert sm.read_consumed(w[r]) == 800
        assert (out[r]["pos"], out[r]["ref_span"], out[r]["nm"], out[r]["md_len"]) == (rec[r]["pos"], rec[r]["ref_span"], rec[r]["nm"], rec[r]["md_len"])
    # a plain record that is unmapped stays as it is, and so does a row without a candidate
    rec, words = _records([(4, []), (0, cg((8, "M")))])
    out, w = sm.sam_split(rec, words, seg, tpos, sel=[1, 0xFFFFFFFF])
    assert out.tobytes() == rec.tobytes() and w == [[], cg((8, "M"))]


def test_constants_symbols_and_feature_bit(tmp_path):
    from aim_amd import capi, engine
    import split_model as sm
    assert _define("AIM_FEATURE_SPLIT") == capi.FEATURE_SPLIT == 0x20000
    assert engine.features() & capi.FEATURE_SPLIT and engine.features() & capi.FEATURE_CHAIN_CLASS
    assert _lib().aim_abi_version() == 2
    assert tuple(_define("AIM_SEG_" + n) for n in ("VALID", "SUPPLEMENTARY", "LEFT_OPEN", "RIGHT_OPEN", "LOOSE")) == \
        (capi.SEG_VALID, capi.SEG_SUPPLEMENTARY, capi.SEG_LEFT_OPEN, capi.SEG_RIGHT_OPEN, capi.SEG_LOOSE) == \
        (sm.VALID, sm.SUPPLEMENTARY, sm.LEFT_OPEN, sm.RIGHT_OPEN, sm.LOOSE) == (1, 2, 4, 8, 16)
    assert _define("AIM_SAM_SUPPLEMENTARY") == capi.SAM_SUPPLEMENTARY == sm.SAM_SUPPLEMENTARY == 0x800
    assert _define("AIM_SEED_MAX_REF_LEN") == sm.MAX_REF_LEN
    assert _lib().aim_split_kernel_names() == b"split_segments_kernel,sam_lane_split_kernel,sam_wave_split_kernel"
    assert _lib().aim_chain_class_kernel_names() == b"chain_class_kernel,read_mapq_kernel"            # the names that were there stay
    assert hasattr(_lib(), "aim_split_segments_device") and hasattr(_lib(), "aim_sam_device_split")
    assert callable(engine.split_segments_device) and callable(engine.sam_device_split) and callable(engine.split_segments)
    assert capi.SEGMENT_DTYPE == sm.SEGMENT and capi.SEGMENT_DTYPE.itemsize == 8
    src = tmp_path / "c.c"
    fields = ("q_begin", "q_end", "read_len", "flags", "cand")
    args = ", ".join(["sizeof(aim_segment_t)"] + ["offsetof(aim_segment_t, %s)" % f for f in fields])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "aim_hip.h"\nint main(void) { printf("%s\\n", %s); return 0; }\n' %
                   (" ".join(["%zu"] * (1 + len(fields))), args))
    exe = tmp_path / "c"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    assert [int(x) for x in subprocess.check_output([str(exe)], text=True).split()] == [8] + [capi.SEGMENT_DTYPE.fields[f][1] for f in fields]


def _split(K=4, read_size=128, flank=8, ref_len=65536, n_reads=4):
    """aim_split_segments_device with NULL buffers: the parameter checks come first, with or without a device."""
    return _lib().aim_split_segments_device(K, read_size, flank, ref_len, n_reads, *([None] * 12))


SPLIT_BAD = [(dict(K=0), "K 0 is outside 1..16"), (dict(K=17), "K 17 is outside 1..16"), (dict(read_size=0), "read_size 0 must be"),
             (dict(read_size=100), "read_size 100 must be"), (dict(read_size=65536), "read_size 65536 must be"),
             (dict(n_reads=1 << 30), "n_reads 1073741824 * K 4 does not fit 32 bits"), (dict(flank=-1), "flank -1 must be >= 0"),
             (dict(ref_len=0xFE000001), "ref_len 4261412865 is above 4261412864"), (dict(), "null device buffer")]


@pytest.mark.parametrize("kw,msg", SPLIT_BAD, ids=[m for _, m in SPLIT_BAD])
def test_split_refusals(kw, msg):
    from aim_amd import capi
    assert _split(**kw) == capi.AIM_EINVAL and _err().startswith("aim_split_segments_device: " + msg), _err()


def test_refusal_order_bounds_that_pass_and_the_sam_entry():
    """The null buffer is the last refusal; the largest legal values get that far; the Python layer raises with the message;
    aim_sam_device_split refuses what aim_sam_device refuses, under its own name."""
    from aim_amd import capi, engine
    assert _split(K=17, read_size=0, flank=-1) == capi.AIM_EINVAL and "K 17" in _err()
    assert _split(read_size=7, flank=-1, n_reads=1 << 30) == capi.AIM_EINVAL and "read_size 7" in _err()
    assert _split(flank=-1, n_reads=1 << 30, ref_len=1 << 32) == capi.AIM_EINVAL and "n_reads" in _err()
    assert _split(flank=-1, ref_len=1 << 32) == capi.AIM_EINVAL and "flank -1" in _err()
    assert _split(K=16, read_size=65528, flank=(1 << 31) - 1, ref_len=0xFE000000) == capi.AIM_EINVAL and _err() == "aim_split_segments_device: null device buffer"
    assert _split(K=1, read_size=8, flank=0, ref_len=0) == capi.AIM_EINVAL and "null device buffer" in _err()
    with pytest.raises(capi.AimError) as e:
        engine.split_segments_device(4, 128, -3, 1000, 4, *([None] * 11))
    assert "flank -3" in str(e.value)
    lib = _lib()
    sam = lambda fn, p, *more: getattr(lib, fn)(capi.params_ref(p), 4, *([None] * 6), 1000, 0, None, None, 16, None, 16, None, *more, None)
    for fn, more in (("aim_sam_device", ()), ("aim_sam_device_split", (None,))):
        assert sam(fn, engine.make_params("wfa", 20, 128), *more) == capi.AIM_EINVAL and _err() == fn + " needs AIM_FLAG_BACKTRACE (the records come from the ops rows)"
        assert sam(fn, engine.make_params("wfa", 20, 128, backtrace=True), *more) == capi.AIM_EINVAL and _err() == "null device buffer"


_SYN = {}


def _synthetic(K, rs):
    import split_model as sm
    if (K, rs) not in _SYN:
        d = sm.synthetic(1, 4099, K, rs)
        _SYN[(K, rs)] = (d, sm.synthetic_segments(d, K, rs))
    return _SYN[(K, rs)]


@pytest.mark.parametrize("K,rs", [(4, 104), (16, 1024)])
def test_model_properties_and_what_the_batch_holds(K, rs):
    """Per read: exactly one left-open and one right-open segment among the primaries of distinct ends, the segments lie inside the
    read, the windows inside the reference and the candidate's window. Counted on the same pass: the batch holds the cases the GPU
    test relies on."""
    import split_model as sm
    d, (req, tp, pat, seg) = _synthetic(K, rs)
    fl = seg["flags"].reshape(-1, K)
    valid = (fl & sm.VALID) != 0
    assert np.array_equal(valid, ((d["cls"]["flags"].reshape(-1, K) & P) != 0) & (np.arange(K)[None, :] < d["seed"]["n_cands"][:, None]))
    assert (((fl & sm.SUPPLEMENTARY) != 0) == (valid & (np.arange(K)[None, :] > 0))).all()
    any_valid = valid.any(axis=1)
    assert (((fl & sm.LEFT_OPEN) != 0).sum(axis=1)[any_valid] >= 1).all() and (((fl & sm.RIGHT_OPEN) != 0).sum(axis=1)[any_valid] >= 1).all()
    v = valid.reshape(-1)
    L = np.clip(d["read_len"], 0, rs).repeat(K)
    assert (seg["q_begin"][v] <= seg["q_end"][v]).all() and (seg["q_end"][v] <= L[v]).all() and (seg["read_len"][v] == L[v]).all()
    assert (req["pattern_len"][v] == seg["q_end"][v].astype(np.int64) - seg["q_begin"][v]).all() and (req["pattern_len"][~v] == L[~v]).all()
    assert (req["text_len"] >= 0).all() and (req["text_len"] <= rs).all() and (req["text_len"][~v] == 0).all() and (tp[~v] == 0).all()
    start = (tp & np.uint64(sm.MINUS - 1)).astype(np.int64)
    assert (start[v] + req["text_len"][v] <= sm.SYN_REF_LEN).all() and (req["idx"] == d["req"]["idx"]).all()
    assert (pat[~v] == d["reads"].repeat(K, axis=0)[~v]).all()
    sole = valid.sum(axis=1) == 1
    one = (valid & sole[:, None]).reshape(-1)
    assert (req[one] == d["req"][one])[L[one] == d["req"]["pattern_len"][one]].all() and (tp[one] == d["text_pos"][one]).all()      # the identity
    nprim = valid.sum(axis=1)
    count = dict(sole=int(sole.sum()), two=int((nprim == 2).sum()), three_up=int((nprim >= 3).sum()), closed_both=int((v & ((seg["flags"] & 12) == 0)).sum()),
                 loose=int(((seg["flags"] & sm.LOOSE) != 0).sum()), start0_recovered=int((v & (d["text_pos"] & np.uint64(sm.MINUS - 1) == 0) & ((seg["flags"] & sm.LOOSE) == 0)).sum()),
                 at_ref_end=int((v & (start + req["text_len"] == sm.SYN_REF_LEN)).sum()), capped=int((v & (req["text_len"] == rs)).sum()),
                 minus=int((v & (tp >> np.uint64(63) != 0)).sum()), empty=int((~v).sum()), odd_begin=int((v & (seg["q_begin"] % 4 != 0)).sum()),
                 secondary_between=int(((d["cls"]["flags"].reshape(-1, K)[:, 1:-1] & S != 0) & valid[:, 2:]).sum()) if K > 2 else 99)
    print(K, rs, count)
    assert all(c >= 20 for c in count.values()), count


def test_chimeric_reads_give_two_segments_each():
    """The model over the numpy chain model: every one of the 32 chimeric reads has exactly two AIM_SEG_VALID slots, one of them
    supplementary, one left-open and one right-open, each inside its own half (a chain's last k-mer may reach a base or two over the
    breakpoint by chance), and none is loose."""
    import chain_class_model as ccm
    import split_model as sm
    from pipeline_batches import model_chains
    rows, rl, halves = sm.chimeric()
    k, stride, w, max_occ, band, flank, min_votes, K = ccm.CHIMERIC_ROW
    req, tpos, votes, seeds, chains = model_chains("chimeric", ccm.CHIMERIC_ROW, rows, rl, ccm.CHIMERIC_SIZE)
    cls = ccm.classify(K, ccm.CHIMERIC_SIZE, 128, rl, tpos, seeds, chains)
    s_req, s_tp, s_pat, seg = sm.segments(K, ccm.CHIMERIC_SIZE, flank, m_ref_len(), rl, rows, req, tpos, seeds, chains, cls)
    fl = seg["flags"].reshape(-1, K)
    print("valid per read", ((fl & sm.VALID) != 0).sum(axis=1).tolist())
    assert (((fl & sm.VALID) != 0).sum(axis=1) == 2).all() and (((fl & sm.SUPPLEMENTARY) != 0).sum(axis=1) == 1).all()
    assert (((fl & sm.LEFT_OPEN) != 0).sum(axis=1) == 1).all() and (((fl & sm.RIGHT_OPEN) != 0).sum(axis=1) == 1).all() and not (fl & sm.LOOSE).any()
    for r in range(32):
        got = set()
        for i in np.nonzero(fl[r])[0]:
            sg = seg[r * K + i]
            hf = sm.half_of(halves[r], int(sg["q_begin"]), int(sg["q_end"]))
            got.add(hf["q_lo"])
            assert hf["q_lo"] - 8 <= int(sg["q_begin"]) and int(sg["q_end"]) <= hf["q_hi"] + 8, (r, sg, hf)
            assert hf["strand"] == int(s_tp[r * K + i]) >> 63, (r, sg, hf)
        assert len(got) == 2, r


def m_ref_len():
    import seed_model as m
    return m.REF_LEN


def test_split_kernels_code_objects():
    """Each new kernel exists exactly once per instantiation, uses no scratch and no LDS, and split_segments_kernel stays within
    kSplitMaxVgpr; the kernels that were there are still there, once each, with sam_lane_kernel and sam_wave_kernel still at eight wavefronts per
    SIMD."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_regs
    lib = os.path.join(ROOT, "aim_amd", "libaim_hip.so")
    if not os.path.exists(lib):
        pytest.fail("libaim_hip.so is missing: run the build")
    regs = codeobj_regs.kernel_regs(lib)
    names = _lib().aim_split_kernel_names().decode().split(",")
    assert names == ["split_segments_kernel", "sam_lane_split_kernel", "sam_wave_split_kernel"]
    bound = int(re.search(r"constexpr int kSplitMaxVgpr = (\d+);", open(os.path.join(ROOT, "aim_amd", "csrc", "split.hpp")).read()).group(1))
    found = [n for n in regs if re.search(r"\baim::split_segments_kernel<(16|64)>\(", n)]
    assert len(found) == 2, found
    for n in found:
        r = regs[n]
        assert r["scratch_bytes"] == 0 and r["lds_static_bytes"] == 0 and 0 < r["vgpr"] + r["agpr"] <= bound <= 512 // 8, (n, r, bound)
    for name in names[1:]:
        found = [n for n in regs if re.search(r"\baim::%s\(" % name, n)]
        assert len(found) == 1 and regs[found[0]]["scratch_bytes"] == 0 and regs[found[0]]["lds_static_bytes"] == 0, (name, found)
    for name in ("seed_candidates_kernel", "seed_minimizer_kernel", "seed_chain_kernel", "seed_chain_minimizer_kernel", "seed_chain_long_kernel",
                 "chain_class_kernel", "read_mapq_kernel", "sam_lane_kernel", "sam_wave_kernel"):
        assert len([n for n in regs if re.search(r"\baim::%s\(" % name, n)]) == 1, name
    lane = regs[[n for n in regs if re.search(r"\baim::sam_lane_kernel\(", n)][0]]
    wave = regs[[n for n in regs if re.search(r"\baim::sam_wave_kernel\(", n)][0]]
    for r in (lane, wave):                                 # (the figures themselves are in profiles/split/README.md)
        assert r["scratch_bytes"] == 0 and r["lds_static_bytes"] == 0 and 0 < r["vgpr"] + r["agpr"] <= 64, r
