"""References of several sequences on the GPU. aim_contig_clip_device on synthetic slot tables against rule 13c's numpy model, every byte
of the four buffers, for each K, batch size and contig count below, on a small and a large grid and under the poison knobs;
aim_map_records_contigs_device on the same tables, under the knobs too, and on the tables of K = 3 padded with empty slots to every group
width (tests/slot_padding.py); Mapper.from_contigs end to end on the shared batch cut into three contigs
(tests/contig_model.py) with five reads planted on the contig edges, against the stages driven by hand and against the one-sequence
mapper on the concatenation; two slots and a reused slot; and python -m aim_amd.map --contigs."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import child  # noqa: E402
import hand_stages as hs  # noqa: E402
from gpu_buffers import Hip, copy_out, put  # noqa: E402

KS = (1, 2, 3, 4, 6, 7, 8, 9, 15, 16)  # the three group widths of the record kernel full (4, 8, 16), one lane short, just past the width before, and 2
N_READS = (1, 65, 2100)
N_CONTIGS = (1, 2, 3, 1024, 1025, 5000)          # 1 024 | 1 025: the sampled table's step goes from 1 to 2; 5 000: step 8
# every contig count at 65 reads; the ends of the range at the other two sizes (one lane of work, and 33 workgroups of it)
CONTIGS_FOR = {1: (2, 5000), 65: N_CONTIGS, 2100: (3, 1025)}
GUARD = 64
SEED = 21


def run_clip(h, K, n, n_contigs, seg_flags=None, keep=False):
    """aim_contig_clip_device over uploaded tables, 64 guard bytes of 0xEE behind each of the three segment buffers and d_contig
    (itself prefilled with 0xEE): the four buffers as bytes, guards included."""
    import contig_model as cg
    from aim_amd import engine
    lens, starts, ref_len, d, want = cg.synthetic_clip(SEED, K, n, n_contigs, seg_flags)
    guard = np.full(GUARD, 0xEE, dtype=np.uint8)
    up = lambda a: h.up(np.concatenate([np.ascontiguousarray(a).view(np.uint8).reshape(-1), guard]))
    S = n * K
    d_sr, d_stp, d_sg, d_ct = up(d["seg_req"]), up(d["seg_text_pos"]), up(d["seg"]), h.filled(4 * S + GUARD)
    d_st = h.up(starts)
    engine.contig_clip_device(K, cg.SYN_READ_SIZE, cg.SYN_FLANK, ref_len, n_contigs, d_st, h.up(lens), n, h.up(d["read_len"]), h.up(d["req"]), h.up(d["text_pos"]),
                              h.up(d["chains"]), d_sr, d_stp, d_sg, d_ct)
    got = (h.down(d_sr, 16 * S + GUARD), h.down(d_stp, 8 * S + GUARD), h.down(d_sg, 8 * S + GUARD), h.down(d_ct, 4 * S + GUARD))
    return (got, (d_sg, d_ct, d_st)) if keep else got


def check_clip(K, n, n_contigs, got, seg_flags=None):
    import contig_model as cg
    want = cg.synthetic_clip(SEED, K, n, n_contigs, seg_flags)[4]
    for name, g, w in zip(("seg_req", "seg_text_pos", "seg", "contig"), got, (want["seg_req"], want["seg_text_pos"], want["seg"], want["contig"])):
        wb = w.view(np.uint8).reshape(-1)
        if g[:len(wb)].tobytes() != wb.tobytes():
            item = w.dtype.itemsize
            bad = np.nonzero((g[:len(wb)].reshape(-1, item) != wb.reshape(-1, item)).any(axis=1))[0]
            raise AssertionError((K, n, n_contigs, name, bad[:8].tolist(), g[:len(wb)].view(w.dtype)[bad[0]], w[bad[0]]))
        assert (g[len(wb):] == 0xEE).all(), "written past " + name


@pytest.mark.parametrize("K", KS)
def test_clip_equals_model(K):
    with Hip() as h:
        for n in N_READS:
            for nc in CONTIGS_FOR[n]:
                check_clip(K, n, nc, run_clip(h, K, n, nc))
                h.free()


KNOB_CASES = ((4, 2100, 5000), (16, 65, 1025), (1, 2100, 3), (4, 65, 1024), (6, 2100, 5000), (9, 65, 1025))
RECORD_KNOB_CASES = ((6, 2100, 1025), (9, 65, 3))      # the record kernel in groups of 8 lanes, and of 16 that K does not fill


def knob_batch():
    out = {}
    with Hip() as h:
        for i, (K, n, nc) in enumerate(KNOB_CASES):
            for j, g in enumerate(run_clip(h, K, n, nc)):
                out["c%d_%d" % (i, j)] = g
            h.free()
        for i, (K, n, nc) in enumerate(RECORD_KNOB_CASES):
            got = run_contig_records(h, K, n, nc)
            for j, g in enumerate(got[0]):
                out["rc%d_%d" % (i, j)] = g
            out["off_%d" % i], out["rec_%d" % i] = got[1:]
            h.free()
    return out


@pytest.mark.parametrize("env", [{"AIM_CHIP_CUS": "1", "AIM_DEBUG_POISON_SCRATCH": "165", "AIM_DEBUG_POISON_OPS": "77", "AIM_DEBUG_POISON_LDS": "90"},
                                 {"AIM_CHIP_CUS": "256", "AIM_DEBUG_POISON_LDS": "255"}], ids=["cus1-poison", "cus256-lds255"])
def test_grid_and_poison_identical(tmp_path, env):
    """The same bytes -- the model's -- at AIM_CHIP_CUS 1 (8 workgroups walk the 33 blocks of slots) and 256 and under the three
    AIM_DEBUG_POISON_* knobs; the plan line names the grid, the contigs and the step."""
    f = str(tmp_path / "k.npz")
    p = child.run("test_contigs_gpu", "knob_batch", npz=f, env=dict(env, AIM_PLAN_DEBUG="1"))
    grid = 8 if env["AIM_CHIP_CUS"] == "1" else 33
    assert "[aim plan] contig_clip_kernel grid=%d block=256 contigs=5000 step=8 slots=8400" % grid in p.stderr, p.stderr
    assert "[aim plan] contig_clip_kernel grid=5 block=256 contigs=1025 step=2 slots=1040" in p.stderr, p.stderr
    assert "block=256 contigs=3 step=1 slots=2100" in p.stderr and "[aim plan] contig_clip_kernel grid=2 block=256 contigs=1024 step=1 slots=260" in p.stderr, p.stderr
    # the record kernel in groups of 8 lanes, and of 16 with K = 9: the launcher's own rule, ceil(reads / (256 / lanes)) under the
    # resident grid of 8 workgroups per compute unit
    line = "[aim plan] map_count_kernel grid=%d block=256 lanes=%d reads=%d K=%d; scan parts=%d per_part=1024; map_records_contig_kernel grid=%d block=256"
    for lanes, n, K, parts in ((8, 2100, 6, 3), (16, 65, 9, 1)):
        g = min(8 * int(env["AIM_CHIP_CUS"]), -(-n // (256 // lanes)))
        assert line % (g, lanes, n, K, parts, g) in p.stderr, p.stderr
    assert "block=256 contigs=5000 step=8 slots=12600" in p.stderr and "contig_clip_kernel grid=3 block=256 contigs=1025 step=2 slots=585" in p.stderr, p.stderr
    out = np.load(f)
    for i, (K, n, nc) in enumerate(KNOB_CASES):
        check_clip(K, n, nc, [out["c%d_%d" % (i, j)] for j in range(4)])
    for i, (K, n, nc) in enumerate(RECORD_KNOB_CASES):
        check_contig_records(K, n, nc, [out["rc%d_%d" % (i, j)] for j in range(4)], out["off_%d" % i], out["rec_%d" % i])


def run_contig_records(h, K, n, nc):
    """The clip over map_records_model's slot tables (their aim_segment_t flags drive the clip's synthetic slots), then
    aim_map_records_contigs_device with d_contig straight from the clip on the device: (the clip's four buffers, rec_offsets, records)
    as bytes, guards included."""
    import map_records_model as mm
    from aim_amd import engine
    seg, sam, cls = mm.synthetic_tables(11, K, n)
    got, (d_sg, d_ct, d_st) = run_clip(h, K, n, nc, seg_flags=seg["flags"], keep=True)
    d_off, d_rec = h.filled(4 * (n + 1) + GUARD), h.filled(64 * n * K + GUARD)
    sb = engine.map_records_scratch(n)
    engine.map_records_contigs_device(K, n, d_sg, h.up(sam), h.up(cls), d_ct, nc, d_st, d_off, d_rec, h.filled(sb), sb)
    return got, h.down(d_off, 4 * (n + 1) + GUARD), h.down(d_rec, 64 * n * K + GUARD)


def check_records(case, n, off_b, rec_b, want_off, want):
    import map_records_model as mm
    assert off_b[:4 * (n + 1)].tobytes() == want_off.tobytes() and (off_b[4 * (n + 1):] == 0xEE).all(), case
    total = int(want_off[n])
    g = rec_b[:64 * total].view(mm.RECORD_DTYPE)
    if g.tobytes() != want.tobytes():
        bad = np.nonzero((g.view(np.uint8).reshape(total, 64) != want.view(np.uint8).reshape(total, 64)).any(axis=1))[0]
        raise AssertionError((case, bad[:8].tolist(), g[bad[0]], want[bad[0]]))
    assert (rec_b[64 * total:] == 0xEE).all(), "written past the records"


def check_contig_records(K, n, nc, clip_bytes, off_b, rec_b):
    import contig_model as cg
    import map_records_model as mm
    seg, sam, cls = mm.synthetic_tables(11, K, n)
    check_clip(K, n, nc, clip_bytes, seg_flags=seg["flags"])
    lens, starts, ref_len, d, o = cg.synthetic_clip(SEED, K, n, nc, seg["flags"])
    want_off, want = cg.records(K, n, o["seg"], sam, cls, o["contig"], starts)
    check_records((K, n, nc), n, off_b, rec_b, want_off, want)
    assert (want["sam"]["pad"] == cg.NONE).any() or n == 1


@pytest.mark.parametrize("K", KS)
def test_contig_records_equal_model(K):
    """map_records_model's slot tables, their aim_segment_t flags driving the clip's synthetic slots, d_contig straight from the clip on
    the device: offsets and records equal the model byte for byte; n_reads = 0 writes rec_offsets[0] alone."""
    from aim_amd import engine
    with Hip() as h:
        for n, nc in ((1, 1), (65, 3), (2100, 1025)):
            check_contig_records(K, n, nc, *run_contig_records(h, K, n, nc))
            h.free()
        d_off = h.filled(8)
        engine.map_records_contigs_device(K, 0, None, None, None, None, 1, None, d_off, None, None, 0)
        assert h.down(d_off, 8).tolist() == [0, 0, 0, 0, 0xEE, 0xEE, 0xEE, 0xEE]


def test_empty_slots_change_nothing_in_the_contig_records():
    """tests/slot_padding.py on the device: the clipped tables of K = 3 with every read padded to 4, 8 and 16 slots (d_contig of an empty
    slot: the read's slot 0) -- the same reads in groups of 4, 8 and 16 lanes -- give rec_offsets and, `slot` renamed, every record byte
    of K = 3, which are the model's."""
    import contig_model as cg
    import map_records_model as mm
    import slot_padding as sp
    from aim_amd import engine
    K, n, nc = 3, N_READS[1], 3
    seg, sam, cls = mm.synthetic_tables(11, K, n)
    lens, starts, ref_len, d, o = cg.synthetic_clip(SEED, K, n, nc, seg["flags"])
    want_off, want = cg.records(K, n, o["seg"], sam, cls, o["contig"], starts)
    assert (want["sam"]["pad"] == cg.NONE).any() and (want["sam"]["pad"] == 2).any() and int(want_off[n]) > n
    with Hip() as h:
        for K2 in (3, 4, 8, 16):
            d_off, d_rec = h.filled(4 * (n + 1) + GUARD), h.filled(64 * n * K2 + GUARD)
            sb = engine.map_records_scratch(n)
            engine.map_records_contigs_device(K2, n, h.up(sp.pad(o["seg"], K, K2, n)), h.up(sp.pad(sam, K, K2, n)), h.up(sp.pad(cls, K, K2, n)),
                                              h.up(sp.pad(o["contig"], K, K2, n, from_slot0=True)), nc, h.up(starts), d_off, d_rec, h.filled(sb), sb)
            off_b, rec_b = h.down(d_off, 4 * (n + 1) + GUARD), h.down(d_rec, 64 * n * K2 + GUARD)
            h.free()
            if K2 == K:
                check_records((K, n, nc), n, off_b, rec_b, want_off, want)
                off3, rec3 = off_b, rec_b[:64 * int(want_off[n])].view(mm.RECORD_DTYPE)
            assert off_b.tobytes() == off3.tobytes(), K2
            assert rec_b[:64 * len(rec3)].tobytes() == sp.records_renamed(rec3, K, K2).tobytes(), K2
            assert (rec_b[64 * len(rec3):] == 0xEE).all(), "written past the records"


# ---- the mapper end to end -----------------------------------------------------------------------------------------------------------
def whole_batch():
    """The shared 73 reads followed by the five planted ones, and the three contigs."""
    import contig_model as cg
    import mapper_batch as mb
    mo = cg.batch_models()
    return mo, cg.batch_contigs(mb.batch()["ref"])[1], mo["rows"], mo["read_len"]


def map_contigs(mp, seqs, rl, rows):
    from aim_amd import engine
    with engine.Mapper.from_contigs(mp, seqs) as m:
        m.submit(0, rl, rows)
        return copy_out(m.wait(0)), m.contigs, m.ref_len


def hand_path(extend):
    """hand_stages.single_end on the concatenation, with aim_contig_clip_device between the split (or the extension) and the
    alignment, and rule 13c's record model at the end: a dict shaped like a mapper result."""
    import chain_class_model as ccm
    import contig_model as cg
    import mapper_batch as mb
    from aim_amd import capi, engine
    mo, seqs, rows, rl = whole_batch()
    ref, starts, lens = mo["concat"], mo["starts"], mo["lens"]
    k, stride, w, max_occ, band, flank, min_votes, K = ccm.CHIMERIC_ROW
    rs, n = ccm.CHIMERIC_SIZE, len(rl)
    params = hs.wfa_params(mb.max_score(), rs, mb.X, mb.O, mb.E, 2 * flank)
    rows_n = n * K
    d_ref = put(ref, hs.DEV, 64)
    sp = engine.seed_params(k, rs, stride=stride, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, max_cands=K, w=w)
    out = hs.segment_rows(sp, ref, rl, rows, extend=(d_ref, engine.extend_params(*mb.EXTEND)) if extend else None)
    d_ct = hs.clip_contigs(out, K, rs, flank, len(ref), starts, lens, n)[0]
    seg = out["d_seg"].cpu().numpy().view(capi.SEGMENT_DTYPE)[:rows_n]
    contig = d_ct.cpu().numpy().view(np.uint32)
    s = hs.segment_records(params, out, rows_n, d_ref, len(ref))[2]
    off, rec = cg.records(K, n, seg, s["sam"], out["class"], contig, starts)
    return {"records": rec, "rec_offsets": off, "cigar": s["cigar"], "md": s["md"]}, seg, contig


def inside(rec, lens):
    """pos + ref_span <= lens[pad] for every mapped record."""
    from aim_amd import capi
    s = rec["sam"]
    mapped = (s["flags"] & capi.SAM_UNMAPPED) == 0
    return mapped, s["pos"][mapped].astype(np.int64) + s["ref_span"][mapped] <= lens[s["pad"][mapped]].astype(np.int64)


def end_to_end():
    import chain_class_model as ccm
    import contig_model as cg
    import mapper_batch as mb
    import split_model as sm
    from aim_amd import capi, engine
    mo, seqs, rows, rl = whole_batch()
    K, nb, n = mo["K"], mo["n_batch"], len(rl)
    starts, lens = mo["starts"], mo["lens"]
    for extend in (False, True):
        mp = mb.mapper_params(n, extend)
        got, layout, ref_len = map_contigs(mp, seqs, rl, rows)
        assert layout[0].tolist() == starts.tolist() and layout[1].tolist() == lens.tolist() and ref_len == mo["ref_len"]
        # ---- the stages by hand, the clip among them, and the record model ----
        want, seg, contig = hand_path(extend)
        g, w = mb.canon(got), mb.canon(want)
        assert g[1] == w[1], "rec_offsets"
        assert g[0] == w[0], ("records", np.nonzero(np.frombuffer(g[0], dtype=np.uint8) != np.frombuffer(w[0], dtype=np.uint8))[0][:8] // 64)
        assert g[2] == w[2] and g[3] == w[3], "CIGAR words or MD bytes"
        # the clip on the device did what the models said it would: nothing in the shared batch, the four single-piece planted reads
        clipped = ((seg["flags"] & cg.CLIPPED) != 0).reshape(-1, K)
        assert not clipped[:nb].any() and clipped[[nb, nb + 1, nb + 2, nb + 3, nb + 5, nb + 6]].astype(int).tolist() == [[1, 0, 0, 0]] * 6, clipped[nb:]
        assert extend or not clipped[nb + 4].any()
        if not extend:
            assert seg.tobytes() == mo["clip"]["seg"].tobytes() and contig.tobytes() == mo["clip"]["contig"].tobytes()
        # ---- the one-sequence mapper on the concatenation: the same record bytes but for pos and pad; no record of the batch is left out ----
        with engine.Mapper(mp, mo["concat"]) as m:
            m.submit(0, rl, rows)
            one = copy_out(m.wait(0))
        assert one["rec_offsets"].tobytes() == got["rec_offsets"].tobytes()
        rec, rec1 = got["records"], one["records"]
        first_planted = int(got["rec_offsets"][nb])
        a, b = rec[:first_planted].copy(), rec1[:first_planted].copy()
        mapped = (a["sam"]["flags"] & capi.SAM_UNMAPPED) == 0
        assert (b["sam"]["pad"] == 0).all() and (a["sam"]["pad"][~mapped] == cg.NONE).all()
        assert (b["sam"]["pos"][mapped] - a["sam"]["pos"][mapped] == starts[a["sam"]["pad"][mapped]]).all() and (a["sam"]["pos"][~mapped] == 0).all()
        for x in (a, b):
            for f in ("pos", "pad", "cigar_offset", "md_offset"):    # (the two offsets depend on scheduling: the words and bytes behind them are compared below)
                x["sam"][f] = 0
        assert a.tobytes() == b.tobytes(), np.nonzero(a.view(np.uint8).reshape(-1, 64) != b.view(np.uint8).reshape(-1, 64))
        o = mb.canon(one)
        assert g[2][:first_planted] == o[2][:first_planted] and g[3][:first_planted] == o[3][:first_planted]
        # every record of the shared batch sits on the contig, and at the place in it, that its truth says
        b_ = mb.batch()
        flank = ccm.CHIMERIC_ROW[5]
        for i in np.nonzero(mapped)[0]:
            r = int(a["read"][i])
            if r < mb.N_CHIMERIC:
                hf = sm.half_of(b_["halves"][r], int(a["q_begin"][i]), int(a["q_end"][i]))
                lo, hi, slack = hf["ref_lo"], hf["ref_hi"], flank + hf["edits"]
            else:
                lo, hi = b_["truth"][r - mb.N_CHIMERIC][:2]
                slack = flank + mb.UNBROKEN_EDITS
            c, local = cg.to_concat(lo)
            pos, span = int(rec["sam"]["pos"][i]), int(rec["sam"]["ref_span"][i])
            assert int(rec["sam"]["pad"][i]) == c and local - slack <= pos and pos + span <= local + (hi - lo) + slack, (r, rec[i])
        # ---- the planted reads ----
        off = got["rec_offsets"]
        counts = np.diff(off.astype(np.int64))[nb:]
        assert counts.tolist() == [1, 1, 1, 1, 2, 1, 1], counts
        words = g[2]
        for j, (contigs, strand, beyond) in enumerate(mo["what"]):
            grp = range(int(off[nb + j]), int(off[nb + j + 1]))
            assert [int(rec[i]["sam"]["pad"]) for i in grp] == list(contigs), (j, [rec[i] for i in grp])
            assert sum(int(rec[i]["sam"]["flags"]) & sm.SAM_SUPPLEMENTARY != 0 for i in grp) == len(grp) - 1
            for i in grp:
                s = rec[i]["sam"]
                assert not int(s["flags"]) & sm.SAM_UNMAPPED and (int(s["flags"]) & sm.SAM_REVERSE != 0) == bool(strand)
                if len(contigs) == 1 or not extend:         # (the extension may lean an inner side of the junction read on the spacer: the issue's note)
                    assert bool(int(rec[i]["seg_flags"]) & cg.CLIPPED) == (len(contigs) == 1)
                assert 0 <= int(s["pos"]) and int(s["pos"]) + int(s["ref_span"]) <= int(lens[int(s["pad"])]), rec[i]
                assert sm.read_consumed(words[i]) == int(rl[nb + j]), (j, words[i])
            if len(contigs) == 1:                                   # the 300 bases at the contig's edge, the others soft-clipped
                s = rec[grp[0]]["sam"]
                at_start = contigs[0] == 1
                assert int(s["ref_span"]) == cg.PLANT_PIECE and int(s["pos"]) == (0 if at_start else int(lens[0]) - cg.PLANT_PIECE) and int(s["nm"]) == 0
                clip_first = at_start                                # (the words run along the reference, whatever the read's strand)
                assert words[grp[0]] == ([(beyond << 4) | 4, cg.PLANT_PIECE << 4] if clip_first else [cg.PLANT_PIECE << 4, (beyond << 4) | 4])
        m_all, ok = inside(rec, lens)
        assert ok.all(), rec[m_all][~ok]
        # ---- and what the clip is for: the one-sequence mapper's records of the planted reads, two flags per read. bound: the record
        # as that mapper returns it (pad 0, pos in the concatenation) breaks pos + ref_span <= lens[pad]; leaves: the aligned interval
        # itself runs over an edge of the contig its pos lies in ----
        bound, leaves = [], []
        for j in range(cg.N_PLANTED):
            grp1 = rec1[int(off[nb + j]):int(off[nb + j + 1])]
            pos1 = grp1["sam"]["pos"].astype(np.int64)
            end1 = pos1 + grp1["sam"]["ref_span"]
            bound.append(int((end1 > lens[grp1["sam"]["pad"]].astype(np.int64)).any()))
            c1 = np.searchsorted(starts, pos1, side="right") - 1
            leaves.append(int(((end1 > starts[c1].astype(np.int64) + lens[c1]) | (pos1 >= starts[c1].astype(np.int64) + lens[c1])).any()))
        print("ONE_SEQUENCE extend=%d %s" % (extend, json.dumps({"bound": bound, "leaves": leaves,
                                                                  "pos_span": [(int(o["sam"]["pos"]), int(o["sam"]["ref_span"])) for o in rec1[first_planted:]]})))
        assert leaves[5:] == [1, 1], leaves                          # one base beyond the edge: a mismatch against the spacer is the cheaper end


_CHILD = {}


def end_to_end_child():
    """end_to_end() in a child process, once for the tests that read its output."""
    if "p" not in _CHILD:
        _CHILD["p"] = child.run("test_contigs_gpu", "end_to_end", cuda_first=True, marker="CONTIGS_END_TO_END_OK", check=False)
    return _CHILD["p"]


def test_end_to_end_equals_the_stages_by_hand_and_the_concatenation():
    """Mapper.from_contigs on the 73 shared reads and the seven planted ones equals the stages by hand with the clip among them plus
    the record model, with and without AIM_MAP_EXTEND, and equals the one-sequence mapper on the concatenation in every record byte of
    the shared batch but pos and pad; every planted read gives the records it was planted for, inside the contig they name; and the
    one-sequence mapper carries the two reads with one base beyond the edge out of their contig."""
    p = end_to_end_child()
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "CONTIGS_END_TO_END_OK" in p.stdout, p.stdout + p.stderr


def test_one_sequence_mapper_breaks_the_bound_on_the_planted_reads():
    """The bound every record of Mapper.from_contigs keeps, pos + ref_span <= lens[pad], put to the one-sequence mapper's records of
    the planted reads as that mapper returns them (pad 0, pos in the concatenation): it is broken, so the planted reads do exercise
    what rule 13c adds. Read by read, with and without the extension (measured on an MI355X):
      24 bases in front of contig 1, both strands   pos 20 160, ref_span 300    broken: the position is the concatenation's
      24 bases behind contig 0, both strands        pos 19 700, ref_span 300    kept: 20 000 <= lens[0] = 20 000
      the junction read                             19 700 / 20 163 (20 160)    broken by its half on contig 1
      one base in front of contig 1                 pos 20 159, ref_span 301    broken, and the interval itself starts in the spacer
      one base behind contig 0                      pos 19 700, ref_span 301    broken by the one base: 20 001
    What the 24-base reads do not do is carry an alignment over a contig's edge: 24 mismatches against the spacer's 'N' cost 72, a gap
    of 24 costs 28, so the one-sequence mapper ends them at the edge too, and the two of them that lie on contig 0 keep the bound
    even as it stands. The one-base reads (a mismatch 3, a gap 5) are there for that; the end-to-end test asserts them."""
    p = end_to_end_child()
    rows = [json.loads(l.split(" ", 2)[2]) for l in p.stdout.splitlines() if l.startswith("ONE_SEQUENCE ")]
    assert len(rows) == 2, p.stdout + p.stderr
    for row in rows:
        print(row)
        assert row["bound"] == [1, 0, 1, 0, 1, 1, 1], row
        assert row["leaves"] == [0, 0, 0, 0, 0, 1, 1], row


def test_two_slots_and_a_reused_slot():
    """Batches A and B back to back on two slots equal A and B run alone; a slot used three times returns the third batch's result; a
    mapper of one sequence next to it still gives pad 0 and global positions."""
    import mapper_batch as mb
    from aim_amd import engine
    mo, seqs, rows, rl = whole_batch()
    A, B, C3 = slice(0, 40), slice(40, 80), slice(30, 70)
    mp = mb.mapper_params(40, True, slots=2)
    alone = {k: mb.canon(map_contigs(mp, seqs, rl[s], rows[s])[0]) for k, s in (("A", A), ("B", B), ("C", C3))}
    assert alone["A"] != alone["C"] and alone["B"] != alone["C"]
    with engine.Mapper.from_contigs(mp, seqs) as m:
        assert m.contigs[0].tolist() == mo["starts"].tolist() and m.contigs[1].tolist() == mo["lens"].tolist()
        m.submit(0, rl[A], rows[A])
        m.submit(1, rl[B], rows[B])
        assert mb.canon(m.wait(0)) == alone["A"] and mb.canon(m.wait(1)) == alone["B"]
        for s in (B, A, C3):
            m.submit(1, rl[s], rows[s])
            last = mb.canon(m.wait(1))
        assert last == alone["C"]
        m.submit(0, rl[:0], rows[:0])
        out = m.wait(0)
        assert out["n_reads"] == 0 and len(out["records"]) == 0 and out["rec_offsets"].tolist() == [0]
    with engine.Mapper(mp, mo["concat"]) as m:
        assert m.contigs is None
        m.submit(0, rl[B], rows[B])
        assert (m.wait(0)["records"]["sam"]["pad"] == 0).all()


def test_command_line_with_contigs(tmp_path):
    """python -m aim_amd.map --contigs in a child process: three @SQ lines, and the body is samout over the mapper's own records."""
    import chain_class_model as ccm
    import contig_model as cg
    import mapper_batch as mb
    from aim_amd import samout
    mo, seqs, rows, rl = whole_batch()
    n = len(rl)
    k, stride, w, max_occ, band, flank, min_votes, K = ccm.CHIMERIC_ROW
    names = ["read%d" % r for r in range(n)]
    cnames = cg.batch_contigs(mb.batch()["ref"])[0]
    with open(tmp_path / "ref.fa", "wb") as f:
        for name, s in zip(cnames, seqs):
            f.write(b">%s a contig\n" % name.encode() + b"\n".join(s.tobytes()[i:i + 70] for i in range(0, len(s), 70)) + b"\n")
    with open(tmp_path / "reads.fq", "wb") as f:
        for r in range(n):
            f.write(b"@%s\n%s\n+\n%s\n" % (names[r].encode(), rows[r, :rl[r]].tobytes(), b"I" * int(rl[r])))
    cmd = [sys.executable, "-m", "aim_amd.map", "--contigs", "--ref", str(tmp_path / "ref.fa"), "--reads", str(tmp_path / "reads.fq"), "-o", str(tmp_path / "out.sam"),
           "--batch", "40", "--read-size", str(ccm.CHIMERIC_SIZE), "-k", str(k), "-w", str(w), "--max-occ", str(max_occ), "--band", str(band), "--flank", str(flank),
           "--min-votes", str(min_votes), "--max-cands", str(K), "--max-score", str(mb.max_score()), "--extend"]
    p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    text = open(tmp_path / "out.sam").read().splitlines()
    head, body = [l for l in text if l.startswith("@")], [l for l in text if not l.startswith("@")]
    assert [l[:3] for l in head] == ["@HD", "@SQ", "@SQ", "@SQ", "@PG"]
    assert head[1:4] == ["@SQ\tSN:%s\tLN:%d" % (nm, len(s)) for nm, s in zip(cnames, seqs)]
    upper = [np.frombuffer(s.tobytes().upper(), dtype=np.uint8) for s in seqs]     # the command line upper-cases the reference
    want = samout.record_lines(map_contigs(mb.mapper_params(n, True), upper, rl, rows)[0], names, rows, rl, cnames, ["I" * int(x) for x in rl])
    assert len(body) == len(want) == 2 * mb.N_CHIMERIC + mb.N_UNBROKEN + mb.N_RANDOM + cg.N_PLANTED + 1
    assert body == want
    # every line lies inside the sequence it names
    ln = dict(zip(cnames, (len(s) for s in seqs)))
    for l in body:
        f = l.split("\t")
        if f[2] != "*":
            span = sum(int(x) for x, op in re.findall(r"(\d+)([MIDNSHP=X])", f[5]) if op in "MDN=X")
            assert 1 <= int(f[3]) and int(f[3]) - 1 + span <= ln[f[2]], l
