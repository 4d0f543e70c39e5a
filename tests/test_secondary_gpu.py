"""Rule 16c on the GPU. The three stateless entry points on the synthetic tables of tests/secondary_model.py against the numpy model,
every output byte -- the four segment buffers after part 1, d_sec after part 2, rec_offsets, the records and aim_map_sec_t after part 3
-- for each K and batch size below, rows of 104 and 1 024, max_sec 1, 2 and 15, with and without AIM_SEC_RECORDS and a contig table, on
a grid of 8 workgroups and under the poison knobs, and the tables of K = 3 padded with empty slots to every group width
(tests/slot_padding.py). Then aim_mapper_t end to end over the three read classes of a two-copy repeat: with aim_mapper_set_secondary
against the stages driven by hand, next to a mapper without it, and over the same repeat cut into two contigs (Mapper.from_contigs).

Of the shared batch of tests/mapper_batch.py (73 reads) the reads that get a secondary row are those the models say
(reads_with_a_secondary_row below: chimeric reads whose second half lies on a planted copy); every other read gives the same records
with and without the feature."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import child  # noqa: E402
from gpu_buffers import Hip  # noqa: E402

KS = (1, 2, 3, 4, 6, 7, 8, 9, 15, 16)  # the three group widths full (4, 8, 16), one lane short, just past the width before, and 2
N_READS = (1, 65, 2100)             # one group, across a wavefront, and 2 101 scan entries: three scan parts of 1 024
GUARD = 64
SEED = 11


def guarded(arr):
    """The array's bytes with GUARD bytes of 0xEE behind them: what an in-place stage must not touch."""
    return np.concatenate([np.ascontiguousarray(arr).view(np.uint8).reshape(-1), np.full(GUARD, 0xEE, dtype=np.uint8)])


def inputs(K, n, rs):
    import secondary_model as sec
    return sec.synthetic(SEED, n, K, rs)


def run_rows(h, K, n, rs, max_sec, d):
    """aim_secondary_rows_device in place over the uploaded split outputs: the four buffers as bytes, guards included."""
    import split_model as sm
    from aim_amd import engine
    bufs = [h.up(guarded(d[k])) for k in ("seg_req", "seg_tp", "seg_pat", "seg")]
    engine.secondary_rows_device(K, rs, sm.SYN_FLANK, sm.SYN_REF_LEN, n, h.up(d["read_len"]), h.up(d["reads"], 64), h.up(d["req"]), h.up(d["text_pos"]),
                                 h.up(d["seed"]), h.up(d["chains"]), h.up(d["cls"]), *bufs, max_sec)
    return [h.down(b, len(guarded(d[k]))) for b, k in zip(bufs, ("seg_req", "seg_tp", "seg_pat", "seg"))]


def check_rows(K, n, rs, max_sec, d, got):
    import secondary_model as sec
    want = sec.synthetic_rows(d, K, rs, max_sec)
    for name, g, w in zip(("seg_requests", "seg_text_pos", "seg_patterns", "seg"), got, want[:4]):
        wb = guarded(w)
        if g.tobytes() != wb.tobytes():
            bad = np.nonzero(g != wb)[0]
            raise AssertionError((K, n, rs, max_sec, name, "first bad byte", int(bad[0]), "of", len(wb), "slots with a row", want[4][:8]))
    return want


def run_select(h, K, n, seg, sam, cls, chains):
    import secondary_model as sec
    from aim_amd import engine
    d_sec = h.filled(8 * n * K + GUARD)
    engine.secondary_select_device(K, n, h.up(seg), h.up(sam), h.up(cls), h.up(chains), sec.SYN_MAX_SCORE, sec.SYN_UNIT, d_sec)
    return h.down(d_sec, 8 * n * K + GUARD)


def check_select(K, n, seg, sam, cls, chains, got):
    import secondary_model as sec
    want = sec.select(K, n, seg, sam, cls, chains, sec.SYN_MAX_SCORE, sec.SYN_UNIT)
    g = got[:8 * n * K].view(sec.SEC_SLOT)
    if g.tobytes() != want.tobytes():
        bad = np.nonzero((g.view(np.uint8).reshape(-1, 8) != want.view(np.uint8).reshape(-1, 8)).any(axis=1))[0]
        raise AssertionError((K, n, "d_sec", bad[:8].tolist(), g[bad[0]], want[bad[0]]))
    assert (got[8 * n * K:] == 0xEE).all(), "written past d_sec"
    return want


def run_records(h, K, n, opt, seg, sam, cls, x, contig=None, starts=None):
    from aim_amd import engine
    d_off, d_rec, d_ms = h.filled(4 * (n + 1) + GUARD), h.filled(64 * n * K + GUARD), h.filled(16 * n * K + GUARD)
    sb = engine.map_records_scratch(n)
    engine.map_records_secondary_device(K, n, opt, h.up(seg), h.up(sam), h.up(cls), h.up(x), d_off, d_rec, d_ms, h.filled(sb), sb,
                                        d_contig=h.up(contig) if contig is not None else None, n_contigs=len(starts) if starts is not None else 0,
                                        d_contig_start=h.up(starts) if starts is not None else None)
    return h.down(d_off, 4 * (n + 1) + GUARD), h.down(d_rec, 64 * n * K + GUARD), h.down(d_ms, 16 * n * K + GUARD)


def check_records(K, n, opt, seg, sam, cls, x, contig, starts, got):
    import map_records_model as mm
    import secondary_model as sec
    want_off, want, want_ms = sec.records(K, n, opt, seg, sam, cls, x, contig, starts)
    off, rec, ms = got
    assert off[:4 * (n + 1)].tobytes() == want_off.tobytes(), (K, n, opt, "rec_offsets")
    assert (off[4 * (n + 1):] == 0xEE).all(), "written past rec_offsets"
    total = int(want_off[n])
    g = rec[:64 * total].view(mm.RECORD_DTYPE)
    if g.tobytes() != want.tobytes():
        bad = np.nonzero((g.view(np.uint8).reshape(total, 64) != want.view(np.uint8).reshape(total, 64)).any(axis=1))[0]
        raise AssertionError((K, n, opt, contig is not None, "records", bad[:8].tolist(), g[bad[0]], want[bad[0]]))
    gm = ms[:16 * total].view(sec.MAP_SEC)
    if gm.tobytes() != want_ms.tobytes():
        bad = np.nonzero((gm.view(np.uint8).reshape(total, 16) != want_ms.view(np.uint8).reshape(total, 16)).any(axis=1))[0]
        raise AssertionError((K, n, opt, "aim_map_sec_t", bad[:8].tolist(), gm[bad[0]], want_ms[bad[0]]))
    assert (rec[64 * total:] == 0xEE).all() and (ms[16 * total:] == 0xEE).all(), "written past the records"
    return total


def all_stages(h, K, n, rs, max_secs=(15,)):
    """The three stages over one synthetic batch, each against the model; every later stage takes the model's (= the device's) rows."""
    import secondary_model as sec
    d = inputs(K, n, rs)
    for max_sec in max_secs:
        want = check_rows(K, n, rs, max_sec, d, run_rows(h, K, n, rs, max_sec, d))
        h.free()
    seg = want[3]
    sam = sec.synthetic_sam(SEED, K, n, seg, d["cls"])
    x = check_select(K, n, seg, sam, d["cls"], d["chains"], run_select(h, K, n, seg, sam, d["cls"], d["chains"]))
    h.free()
    contig, starts = sec.synthetic_contigs(SEED, K, n)
    totals = []
    for opt, ct, st in ((0, None, None), (sec.SEC_RECORDS, None, None), (sec.SEC_RECORDS, contig, starts), (0, contig, starts)):
        totals.append(check_records(K, n, opt, seg, sam, d["cls"], x, ct, st, run_records(h, K, n, opt, seg, sam, d["cls"], x, ct, st)))
        h.free()
    return want[4], x, totals


@pytest.mark.parametrize("K", KS)
def test_stages_equal_model(K):
    """Rows of 104 at every batch size; max_sec 1, 2 and 15 at 65 reads. The synthetic inputs hold families of 0, 1 and K - 1
    secondaries, a parent extended on an inner side, a secondary whose p_lo is not recoverable, windows cut by position 0 and by ref_len,
    a winner over the cap with a mapped secondary, and score ties (tests/test_secondary_cpu.py asserts that on the model)."""
    from aim_amd import engine
    with Hip() as h:
        for n in N_READS:
            got, x, totals = all_stages(h, K, n, 104, max_secs=(1, 2, 15) if n == 65 else (15,))
            assert K == 1 or n == 1 or (len(got) > 0 and totals[1] > totals[0] >= n)
        # an empty batch: nothing is launched, rec_offsets[0] = 0 and nothing else
        engine.secondary_rows_device(K, 104, 16, 1 << 20, 0, None, None, None, None, None, None, None, None, None, None, None, 15)
        engine.secondary_select_device(K, 0, None, None, None, None, 60, 3, None)
        d_off = h.filled(8)
        engine.map_records_secondary_device(K, 0, 1, None, None, None, None, d_off, None, None, None, 0)
        assert h.down(d_off, 8).tolist() == [0, 0, 0, 0, 0xEE, 0xEE, 0xEE, 0xEE]


@pytest.mark.parametrize("K", (4, 16))
def test_rows_of_1024(K):
    """Rows of 1 024: with 4 lanes per read a row is cut into two shares, with 16 lanes it is one."""
    with Hip() as h:
        got, _, _ = all_stages(h, K, 65, 1024, max_secs=(2, 15))
        assert len(got) > 20


KNOB_CASES = ((4, 2100, 104), (16, 65, 104), (6, 2100, 104), (9, 65, 104), (4, 65, 1024))


def knob_batch():
    import secondary_model as sec
    out = {}
    with Hip() as h:
        for i, (K, n, rs) in enumerate(KNOB_CASES):
            d = inputs(K, n, rs)
            for k, v in zip(("req", "tp", "pat", "seg"), run_rows(h, K, n, rs, 15, d)):
                out["%s_%d" % (k, i)] = v
            h.free()
            seg = sec.synthetic_rows(d, K, rs, 15)[3]
            sam = sec.synthetic_sam(SEED, K, n, seg, d["cls"])
            out["sec_%d" % i] = run_select(h, K, n, seg, sam, d["cls"], d["chains"])
            x = sec.select(K, n, seg, sam, d["cls"], d["chains"], sec.SYN_MAX_SCORE, sec.SYN_UNIT)
            contig, starts = sec.synthetic_contigs(SEED, K, n)
            out["off_%d" % i], out["rec_%d" % i], out["ms_%d" % i] = run_records(h, K, n, sec.SEC_RECORDS, seg, sam, d["cls"], x, contig, starts)
            h.free()
    return out


@pytest.mark.parametrize("env", [{"AIM_CHIP_CUS": "1", "AIM_DEBUG_POISON_SCRATCH": "165", "AIM_DEBUG_POISON_OPS": "77", "AIM_DEBUG_POISON_LDS": "90"},
                                 {"AIM_CHIP_CUS": "256", "AIM_DEBUG_POISON_LDS": "255"}], ids=["cus1-poison", "cus256-lds255"])
def test_grid_and_poison_identical(tmp_path, env):
    """The same bytes -- the model's -- at AIM_CHIP_CUS 1 (8 workgroups walk the blocks of reads) and 256 and under the three
    AIM_DEBUG_POISON_* knobs."""
    import secondary_model as sec
    f = str(tmp_path / "k.npz")
    p = child.run("test_secondary_gpu", "knob_batch", npz=f, env=dict(env, AIM_PLAN_DEBUG="1"))
    cus = int(env["AIM_CHIP_CUS"])
    for K, n, rs in KNOB_CASES:
        lanes = 4 if K <= 4 else 8 if K <= 8 else 16
        parts = 2 if (rs, lanes) == (1024, 4) else 1
        g = min(8 * cus, -(-n * parts // (256 // lanes)))
        assert "[aim plan] secondary_rows_kernel grid=%d block=256 lanes=%d parts=%d reads=%d K=%d read_size=%d max_sec=15" % (g, lanes, parts, n, K, rs) in p.stderr, p.stderr
        g = min(8 * cus, -(-n // (256 // lanes)))
        assert "[aim plan] secondary_select_kernel grid=%d block=256 lanes=%d reads=%d K=%d" % (g, lanes, n, K) in p.stderr, p.stderr
        line = "[aim plan] map_count_sec_kernel grid=%d block=256 lanes=%d reads=%d K=%d options=0x1 contigs=5; scan parts=%d per_part=1024; map_records_sec_kernel grid=%d"
        assert line % (g, lanes, n, K, 3 if n == 2100 else 1, g) in p.stderr, p.stderr
    out = np.load(f)
    for i, (K, n, rs) in enumerate(KNOB_CASES):
        d = inputs(K, n, rs)
        seg = check_rows(K, n, rs, 15, d, [out["%s_%d" % (k, i)] for k in ("req", "tp", "pat", "seg")])[3]
        sam = sec.synthetic_sam(SEED, K, n, seg, d["cls"])
        x = check_select(K, n, seg, sam, d["cls"], d["chains"], out["sec_%d" % i])
        contig, starts = sec.synthetic_contigs(SEED, K, n)
        check_records(K, n, sec.SEC_RECORDS, seg, sam, d["cls"], x, contig, starts, (out["off_%d" % i], out["rec_%d" % i], out["ms_%d" % i]))


def test_empty_slots_change_nothing():
    """tests/slot_padding.py on the device: the tables of K = 3 with every read padded to 4, 8 and 16 slots -- the same reads in groups
    of 4, 8 and 16 lanes -- give, slots renamed, every byte of K = 3, which is the model's."""
    import map_records_model as mm
    import secondary_model as sec
    import slot_padding as sp
    K, n, rs = 3, 65, 104
    d = inputs(K, n, rs)
    with Hip() as h:
        want = check_rows(K, n, rs, 15, d, run_rows(h, K, n, rs, 15, d))
        seg = want[3]
        sam = sec.synthetic_sam(SEED, K, n, seg, d["cls"])
        x = check_select(K, n, seg, sam, d["cls"], d["chains"], run_select(h, K, n, seg, sam, d["cls"], d["chains"]))
        off3, rec3, ms3 = run_records(h, K, n, sec.SEC_RECORDS, seg, sam, d["cls"], x)
        total = check_records(K, n, sec.SEC_RECORDS, seg, sam, d["cls"], x, None, None, (off3, rec3, ms3))
        assert total > n
        r3 = rec3[:64 * total].view(mm.RECORD_DTYPE)
        want_ms = ms3[:16 * total].view(sec.MAP_SEC).copy()
        for K2 in (4, 8, 16):
            h.free()
            pd = dict(d, **{k: sp.pad(d[k], K, K2, n) for k in ("req", "text_pos", "chains", "cls", "seg_req", "seg_tp", "seg")})
            pd["seg_pat"] = sp.pad(d["seg_pat"].view([("row", "u1", (rs,))]).reshape(-1), K, K2, n).view(np.uint8).reshape(-1, rs)
            got = run_rows(h, K2, n, rs, 15, pd)
            for g, w, dt in zip(got, want[:4], (d["seg_req"].dtype, np.dtype("<u8"), np.dtype([("row", "u1", (rs,))]), d["seg"].dtype)):
                mine, rest = sp.unpad(g[:-GUARD].view(dt), K, K2, n)
                assert mine.tobytes() == np.ascontiguousarray(w).tobytes() and (g[-GUARD:] == 0xEE).all(), K2
            p_seg, p_sam = sp.pad(seg, K, K2, n), sp.pad(sam, K, K2, n)
            px = run_select(h, K2, n, p_seg, p_sam, pd["cls"], pd["chains"])
            assert px[:8 * n * K2].tobytes() == sp.pad(x, K, K2, n).tobytes() and (px[8 * n * K2:] == 0xEE).all(), K2
            off, rec, ms = run_records(h, K2, n, sec.SEC_RECORDS, p_seg, p_sam, pd["cls"], sp.pad(x, K, K2, n))
            assert off[:4 * (n + 1)].tobytes() == off3[:4 * (n + 1)].tobytes() and (off[4 * (n + 1):] == 0xEE).all(), K2
            assert rec[:64 * total].tobytes() == sp.records_renamed(r3, K, K2).tobytes() and (rec[64 * total:] == 0xEE).all(), K2
            want_ms["family_slot"] = sp.rename(ms3[:16 * total].view(sec.MAP_SEC)["family_slot"], r3["read"], K, K2)
            assert ms[:16 * total].tobytes() == want_ms.tobytes() and (ms[16 * total:] == 0xEE).all(), K2


# ---- the mapper end to end ---------------------------------------------------------------------------------------------------------
MAX_SEC = 2


def map_with(mp, ref, rl, rows, sc, contigs=False):
    """One batch through a mapper of its own (contigs: `ref` is a list of sequences and the mapper Mapper.from_contigs), with
    aim_mapper_set_secondary where sc is given: the result detached."""
    from aim_amd import engine
    from gpu_buffers import copy_out
    with (engine.Mapper.from_contigs(mp, ref) if contigs else engine.Mapper(mp, ref)) as m:
        if sc is not None:
            m.set_secondary(sc)
        m.submit(0, rl, rows)
        return copy_out(m.wait(0))


def by_hand(ref, rows, rl, options, contigs=None):
    """The stages driven by hand on torch buffers -- chain, classify, split, aim_secondary_rows_device, the segment alignment and
    aim_sam_device_split, aim_secondary_select_device (checked against the model over the downloaded rows) -- then the record model: a
    dict shaped like the mapper's result, with the class rows for the caller. contigs = (starts, lens): `ref` is their concatenation, and
    aim_contig_clip_device runs behind the secondary rows as it does in the mapper."""
    import chain_class_model as ccm
    import hand_stages as hs
    import mapper_batch as mb
    import secondary_model as sec
    import torch
    from aim_amd import capi, engine
    from gpu_buffers import put, zeros
    k, stride, w, max_occ, band, flank, min_votes, K = ccm.CHIMERIC_ROW
    rs, n = ccm.CHIMERIC_SIZE, len(rl)
    params = hs.wfa_params(mb.max_score(), rs, mb.X, mb.O, mb.E, 2 * flank)
    d_ref = put(ref, hs.DEV, 64)
    sp = engine.seed_params(k, rs, stride=stride, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, max_cands=K, w=w)
    out = hs.segment_rows(sp, ref, rl, rows)
    engine.secondary_rows_device(K, rs, flank, len(ref), n, *[out[x].data_ptr() for x in ("d_read_len", "d_reads", "d_req", "d_text_pos", "d_seed", "d_chains", "d_class",
                                                                                         "d_seg_req", "d_seg_text_pos", "d_seg_patterns", "d_seg")], MAX_SEC)
    torch.cuda.synchronize()
    seg = out["d_seg"].cpu().numpy().view(capi.SEGMENT_DTYPE)[:n * K].copy()
    want = sec.rows(K, rs, flank, len(ref), MAX_SEC, rl, rows, out["req"], out["text_pos"], out["seed"], out["chains"], out["class"], out["seg_req"],
                    out["seg_text_pos"], out["seg_patterns"], out["seg"])
    assert seg.tobytes() == want[3].tobytes() and out["d_seg_req"].cpu().numpy()[:16 * n * K].tobytes() == want[0].tobytes()
    assert out["d_seg_text_pos"].cpu().numpy()[:8 * n * K].tobytes() == want[1].tobytes() and out["d_seg_patterns"].cpu().numpy()[:n * K * rs].tobytes() == want[2].tobytes()
    contig = None
    if contigs is not None:
        contig = hs.clip_contigs(out, K, rs, flank, len(ref), contigs[0], contigs[1], n)[0].cpu().numpy().view(np.uint32)[:n * K].copy()
        seg = out["d_seg"].cpu().numpy().view(capi.SEGMENT_DTYPE)[:n * K].copy()
    s = hs.segment_records(params, out, n * K, d_ref, len(ref))[2]
    d_sec = zeros(8 * n * K, hs.DEV)
    engine.secondary_select_device(K, n, out["d_seg"].data_ptr(), s["d_sam"].data_ptr(), out["d_class"].data_ptr(), out["d_chains"].data_ptr(), mb.max_score(), mb.X,
                                   d_sec.data_ptr())
    torch.cuda.synchronize()
    x = d_sec.cpu().numpy()[:8 * n * K].view(sec.SEC_SLOT).copy()
    assert x.tobytes() == sec.select(K, n, seg, s["sam"], out["class"], out["chains"], mb.max_score(), mb.X).tobytes()
    off, rec, ms = sec.records(K, n, options, seg, s["sam"], out["class"], x, contig, contigs[0] if contigs is not None else None)
    return {"records": rec, "rec_offsets": off, "cigar": s["cigar"], "md": s["md"], "sec": ms, "class": out["class"], "got_rows": want[4]}


def same(got, want):
    import mapper_batch as mb
    g, w = mb.canon(got), mb.canon(want)
    assert g[1] == w[1], "rec_offsets"
    assert g[0] == w[0], ("records", np.nonzero(np.frombuffer(g[0], dtype=np.uint8) != np.frombuffer(w[0], dtype=np.uint8))[0][:8] // 64)
    assert g[2] == w[2] and g[3] == w[3], "CIGAR words or MD bytes"
    assert np.asarray(got["sec"]).tobytes() == np.asarray(want["sec"]).tobytes(), "aim_map_sec_t"


def reads_with_a_secondary_row():
    """The reads of the shared batch that rule 16c part 1 gives a row, by the chain, class, split and row models."""
    import chain_class_model as ccm
    import mapper_batch as mb
    import secondary_model as sec
    import split_model as sm
    from pipeline_batches import chimeric_expected, expected, reference
    ref = reference()
    K, flank, rs = ccm.CHIMERIC_ROW[7], ccm.CHIMERIC_ROW[5], ccm.CHIMERIC_SIZE
    rows, rl, _, (req, tpos, seeds, chains), cls, segs = chimeric_expected()
    has = [s // K for s in sec.rows(K, rs, flank, len(ref), MAX_SEC, rl, rows, req, tpos, seeds, chains, cls, *segs)[4]]
    at = len(rl)
    for key, (rows, rl) in (("mapper unbroken", mb.unbroken_reads(ref)[:2]), (("mapper random", mb.RANDOM_SEED), mb.random_reads())):
        req, tpos, votes, seeds, chains = expected(ccm.CHIMERIC_ROW, rows, rl, key, read_size=rs)
        cls = ccm.classify(K, rs, 128, rl, tpos, seeds, chains)
        segs = sm.segments(K, rs, flank, len(ref), rl, rows, req, tpos, seeds, chains, cls)
        has += [at + s // K for s in sec.rows(K, rs, flank, len(ref), MAX_SEC, rl, rows, req, tpos, seeds, chains, cls, *segs)[4]]
        at += len(rl)
    return sorted(set(has))


def end_to_end():
    """The 48 reads of the three classes (tests/secondary_model.py) through a mapper with aim_mapper_set_secondary, through the stages
    by hand, and through a mapper without it; then the shared batch of tests/mapper_batch.py with and without the feature."""
    import chain_class_model as ccm
    import mapper_batch as mb
    import secondary_model as sec
    import split_model as sm
    from aim_amd import engine
    K = ccm.CHIMERIC_ROW[7]
    classes = sec.repeat_classes()
    sc = engine.secondary_params(MAX_SEC, records=True)
    for name in ("tie", "control", "exact"):
        ref, rows, rl, truth = classes[name]
        n = len(rl)
        mp = mb.mapper_params(n, False)
        got = map_with(mp, ref, rl, rows, sc)
        want = by_hand(ref, rows, rl, sec.SEC_RECORDS)
        assert want["got_rows"] == [r * K + 1 for r in range(n)]
        same(got, want)
        dropped = map_with(mp, ref, rl, rows, engine.secondary_params(MAX_SEC, records=False))
        same(dropped, by_hand(ref, rows, rl, 0))
        plain = map_with(mp, ref, rl, rows, None)
        rec, off, ms = got["records"], got["rec_offsets"], got["sec"]
        assert np.diff(off.astype(np.int64)).tolist() == [2] * n and np.diff(dropped["rec_offsets"].astype(np.int64)).tolist() == [1] * n
        assert np.diff(plain["rec_offsets"].astype(np.int64)).tolist() == [1] * n and "sec" not in plain
        words = mb.canon(got)[2]
        for r in range(n):
            first, second, old, only = rec[off[r]], rec[off[r] + 1], plain["records"][r], dropped["records"][r]
            lo, hi, strand, n_sites = truth[r]
            inside = lambda o, a: a <= int(o["sam"]["pos"]) and int(o["sam"]["pos"]) + int(o["sam"]["ref_span"]) <= a + sec.REPEAT_LEN
            assert not int(first["sam"]["flags"]) & (sec.SAM_SECONDARY | sm.SAM_SUPPLEMENTARY | sm.SAM_UNMAPPED)
            assert int(second["sam"]["flags"]) & sec.SAM_SECONDARY and second["mapq"] == 0 and not int(second["sam"]["flags"]) & sm.SAM_SUPPLEMENTARY
            for o in (first, second, old):
                assert (int(o["sam"]["flags"]) & sm.SAM_REVERSE != 0) == bool(strand)
            assert sm.read_consumed(words[off[r]]) == sm.read_consumed(words[off[r] + 1]) == int(rl[r])
            want_only = first.copy()
            want_only["n_records"] = 1
            assert mb.canon({"records": np.array([only]), "rec_offsets": [0, 1], "cigar": dropped["cigar"], "md": dropped["md"]})[0] == \
                mb.canon({"records": np.array([want_only]), "rec_offsets": [0, 1], "cigar": got["cigar"], "md": got["md"]})[0]
            m0 = ms[off[r]]
            print(name, r, "with", int(first["sam"]["pos"]), int(first["mapq"]), int(first["sam"]["score"]), "second", int(second["sam"]["pos"]), int(m0["second_score"]),
                  "without", int(old["sam"]["pos"]), int(old["mapq"]))
            assert m0["family_slot"] == r * K and m0["n_members"] == 2 and m0["flags"] & sec.COMPLETE and ms[off[r] + 1].tobytes() == m0.tobytes()
            if name == "tie":
                # copy B, the true interval, by alignment: cheaper by one mismatch per covered site
                gap = mb.X * n_sites
                assert lo <= int(first["sam"]["pos"]) and int(first["sam"]["pos"]) + int(first["sam"]["ref_span"]) <= hi
                assert m0["flags"] & sec.SWAPPED and first["slot"] == r * K + 1 and m0["second_score"] == int(first["sam"]["score"]) + gap
                assert first["mapq"] == m0["aln_mapq"] == 6 * gap // mb.X and first["mapq"] in (24, 30) and m0["chain_mapq"] == 0 and m0["n_tied"] == 1
                assert inside(second, sec.REPEAT_A) and second["slot"] == r * K
                assert inside(old, sec.REPEAT_A) and old["mapq"] == 0 and old["slot"] == r * K          # without the feature: the wrong copy, MAPQ 0
            elif name == "control":
                assert lo <= int(first["sam"]["pos"]) and int(first["sam"]["pos"]) + int(first["sam"]["ref_span"]) <= hi
                assert not m0["flags"] & sec.SWAPPED and first["slot"] == r * K and first["mapq"] > 0 and inside(second, sec.REPEAT_A)
                assert inside(old, sec.REPEAT_B) and old["slot"] == r * K and int(old["sam"]["pos"]) == int(first["sam"]["pos"])
            else:
                assert inside(first, sec.REPEAT_A) and first["slot"] == r * K and m0["n_tied"] == 2 and first["mapq"] == 0 and not m0["flags"] & sec.SWAPPED
                assert inside(second, sec.REPEAT_B) and m0["second_score"] == int(first["sam"]["score"]) and inside(old, sec.REPEAT_A)
    # a reference of several sequences: copy A in contig 0, copy B in contig 1; the clip runs over the secondary rows too
    ref, rows, rl, truth = classes["tie"]
    cut = 8000
    seqs = [ref[:cut], ref[cut:]]
    spacer = ccm.CHIMERIC_ROW[4] + 64                  # AIM_CONTIG_SPACER(band), what the mapper uses
    cat = engine.contigs_concat(seqs, spacer)
    starts, lens = engine.contigs_layout([len(x) for x in seqs], spacer)[0], np.array([len(x) for x in seqs], dtype=np.uint32)
    got = map_with(mb.mapper_params(len(rl), False), seqs, rl, rows, sc, contigs=True)
    same(got, by_hand(cat, rows, rl, sec.SEC_RECORDS, contigs=(starts, lens)))
    off = got["rec_offsets"]
    assert np.diff(off.astype(np.int64)).tolist() == [2] * len(rl)
    for r in range(len(rl)):
        first, second = got["records"][off[r]], got["records"][off[r] + 1]
        assert first["sam"]["pad"] == 1 and truth[r][0] - cut <= int(first["sam"]["pos"]) and int(first["sam"]["pos"]) + int(first["sam"]["ref_span"]) <= truth[r][1] - cut
        assert second["sam"]["pad"] == 0 and int(second["sam"]["flags"]) & sec.SAM_SECONDARY and sec.in_copy(int(second["sam"]["pos"]), sec.REPEAT_A)
        assert first["mapq"] in (24, 30) and got["sec"][off[r]]["flags"] & sec.SWAPPED
    # the shared batch: where no read has a secondary the records are the ones the mapper always gave
    b = mb.batch()
    ref, rows, rl = b["ref"], b["rows"], b["read_len"]
    n = len(rl)
    mp = mb.mapper_params(n, True)
    got, plain = map_with(mp, ref, rl, rows, sc), map_with(mp, ref, rl, rows, None)
    ca, cb = mb.canon(got), mb.canon(plain)
    members = {r: 0 for r in range(n)}
    for o, x in zip(got["records"], got["sec"]):
        members[int(o["read"])] = max(members[int(o["read"])], int(x["n_members"]))
    has = sorted(r for r, v in members.items() if v > 1)
    print("reads with an aligned secondary:", len(has), has)
    assert has == reads_with_a_secondary_row()
    go, po = got["rec_offsets"], plain["rec_offsets"]
    for r in range(n):
        if r in has:
            continue
        a, bb = slice(int(go[r]), int(go[r + 1])), slice(int(po[r]), int(po[r + 1]))
        assert got["records"][a]["n_records"].tolist() == plain["records"][bb]["n_records"].tolist()
        assert np.frombuffer(ca[0], dtype=np.uint8).reshape(-1, 64)[a].tobytes() == np.frombuffer(cb[0], dtype=np.uint8).reshape(-1, 64)[bb].tobytes(), r
        assert ca[2][a] == cb[2][bb] and ca[3][a] == cb[3][bb], r


def test_end_to_end_equals_the_stages_by_hand():
    p = child.run("test_secondary_gpu", "end_to_end", cuda_first=True, marker="SECONDARY_END_TO_END_OK", check=False)
    print(p.stdout[-6000:])
    assert p.returncode == 0 and "SECONDARY_END_TO_END_OK" in p.stdout, p.stdout[-3000:] + p.stderr[-6000:]


def test_two_slots_reuse_empty_batch_and_refusals():
    """Two batches back to back on two slots equal the batches run alone; a reused slot returns its last batch; n_reads = 0 is a batch;
    the setter's refusals that need a mapper; pairing and secondaries refuse each other."""
    import mapper_batch as mb
    import secondary_model as sec
    from aim_amd import capi, engine
    ref, rows, rl, _ = sec.repeat_classes()["tie"]
    mp = mb.mapper_params(16, False, slots=2)
    sc = engine.secondary_params(MAX_SEC)
    A, B = slice(0, 16), slice(3, 12)
    canon = lambda o: mb.canon(o) + (np.asarray(o["sec"]).tobytes(),)
    alone = {k: canon(map_with(mp, ref, rl[s], rows[s], sc)) for k, s in (("A", A), ("B", B))}
    assert alone["A"] != alone["B"]
    with engine.Mapper(mp, ref) as m:
        with pytest.raises(capi.AimError) as e:
            m.secondary(0)
        assert e.value.code == capi.AIM_ESTATE and "aim_mapper_set_secondary was not called" in str(e.value)
        m.submit(0, rl[A], rows[A])
        with pytest.raises(capi.AimError) as e:
            m.set_secondary(sc)
        assert e.value.code == capi.AIM_EINVAL and "slot 0 is in flight" in str(e.value)
        assert "sec" not in m.wait(0)
        m.set_secondary(sc)
        with pytest.raises(capi.AimError) as e:
            m.set_secondary(sc)
        assert e.value.code == capi.AIM_EINVAL and "already set" in str(e.value)
        with pytest.raises(capi.AimError) as e:
            m.set_pairing(engine.pair_params(0, 500, rescue=False))
        assert e.value.code == capi.AIM_EINVAL and str(e.value).count("aim_mapper_set_pairing: ") == 1 and "secondaries" in str(e.value)
        with pytest.raises(capi.AimError) as e:
            m.secondary(0)
        assert e.value.code == capi.AIM_ESTATE and "no batch waited for" in str(e.value)
        m.submit(0, rl[A], rows[A])
        m.submit(1, rl[B], rows[B])
        assert canon(m.wait(0)) == alone["A"] and canon(m.wait(1)) == alone["B"]
        for s in (A, B):                                  # the longer batch first: what it left behind must not show
            m.submit(1, rl[s], rows[s])
            last = canon(m.wait(1))
        assert last == alone["B"]
        m.submit(0, rl[:0], rows[:0])
        out = m.wait(0)
        assert out["n_reads"] == 0 and len(out["records"]) == 0 and len(out["sec"]) == 0 and out["rec_offsets"].tolist() == [0]
    with engine.Mapper(mp, ref) as m:
        m.set_pairing(engine.pair_params(0, 500, rescue=False))
        with pytest.raises(capi.AimError) as e:
            m.set_secondary(sc)
        assert e.value.code == capi.AIM_EINVAL and "the mapper is paired" in str(e.value)
