"""Rule 14c on the GPU. aim_pair_rescue_rows_device, aim_pair_select_device (apply included) and aim_map_mates_device on synthetic slot
tables against the numpy model (tests/pair_model.py), every output byte -- the rescue rows and the pattern rows, aim_map_pair_t, the
rewritten slot arrays, aim_map_mate_t and the records -- for each K and batch size below, with and without d_contig, on a small and a
large grid and under the poison knobs, and the tables of K = 3 padded with empty slots to every group width against themselves
(tests/slot_padding.py); then aim_mapper_t with pairing on the shared paired batch (tests/pair_batch.py) against the
stages driven by hand and against the truth; and a mapper without pairing against the bytes it always gave."""
import functools
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
from gpu_buffers import Hip, copy_out, put, zeros  # noqa: E402

KS = (1, 2, 3, 4, 6, 7, 8, 9, 15, 16)  # the three group widths full (4, 8, 16), one lane short, just past the width before, and 2
N_READS = (2, 130, 4100)            # one group, across wavefronts, and more read pairs than one workgroup of any K holds
GUARD = 64
CIGAR_BASE, MD_BASE = 1000, 70000


@functools.lru_cache(maxsize=None)
def tables(K, n, contigs):
    """Built once per shape and shared: neither side writes to them."""
    import pair_model as pm
    return pm.synthetic_tables(21, K, n, contigs)


def run_stages(h, K, n, t, rescue=True):
    """The three entry points plus the record kernel over uploaded tables, as the mapper orders them: rows, select / apply, records,
    mates. Every output buffer is prefilled with 0xEE and carries a guard. Returns the downloaded bytes by name."""
    import pair_model as pm
    from aim_amd import engine
    rs, rz = pm.READ_SIZE, pm.RESCUE_SIZE
    pp = engine.pair_params(pm.MIN_SPAN, pm.MAX_SPAN, 17, rescue=rescue, rescue_size=rz)
    ee = lambda nbytes: h.filled(nbytes + GUARD)
    contigs = t["contig"] is not None
    d_rl, d_reads = h.up(t["read_len"]), h.up(t["reads"], 16)
    d_seg, d_sam, d_cls, d_res_sam = h.up(t["seg"]), h.up(t["sam"]), h.up(t["cls"]), h.up(t["res_sam"])
    d_contig = h.up(t["contig"]) if contigs else None
    d_starts, d_lens = (h.up(t["starts"]), h.up(t["lens"])) if contigs else (None, None)
    nc = len(t["starts"]) if contigs else 0
    d_req, d_tp, d_pat = ee(16 * n), ee(8 * n), ee(n * rz)
    out = {}
    if rescue:
        engine.pair_rescue_rows_device(pp, K, rs, t["ref_len"], n, d_rl, d_reads, d_seg, d_sam, d_req, d_tp, d_pat, d_contig=d_contig, n_contigs=nc,
                                       d_contig_start=d_starts, d_contig_len=d_lens)
        out["req"], out["tpos"], out["pat"] = h.down(d_req, 16 * n + GUARD), h.down(d_tp, 8 * n + GUARD), h.down(d_pat, n * rz + GUARD)
    d_pairs = ee(32 * (n // 2))
    engine.pair_select_device(pp, K, rs, n, d_rl, d_seg, d_sam, d_cls, d_res_sam if rescue else None, CIGAR_BASE, MD_BASE, d_pairs, d_contig=d_contig)
    out["pairs"] = h.down(d_pairs, 32 * (n // 2) + GUARD)
    out["seg"], out["sam"], out["cls"] = h.down(d_seg, 8 * n * K), h.down(d_sam, 48 * n * K), h.down(d_cls, 8 * n * K)
    if contigs:
        out["contig"] = h.down(d_contig, 4 * n * K)
    d_off, d_rec, d_mates = ee(4 * (n + 1)), ee(64 * n * K), ee(16 * n * K)
    sb = engine.map_records_scratch(n)
    d_scr = h.filled(sb)
    if contigs:
        engine.map_records_contigs_device(K, n, d_seg, d_sam, d_cls, d_contig, nc, d_starts, d_off, d_rec, d_scr, sb)
    else:
        engine.map_records_device(K, n, d_seg, d_sam, d_cls, d_off, d_rec, d_scr, sb)
    out["rec_before"] = h.down(d_rec, 64 * n * K)
    engine.map_mates_device(K, n, d_pairs, d_seg, d_sam, d_off, d_rec, d_mates, d_contig=d_contig, n_contigs=nc, d_contig_start=d_starts)
    out["off"], out["rec"], out["mates"] = h.down(d_off, 4 * (n + 1)), h.down(d_rec, 64 * n * K + GUARD), h.down(d_mates, 16 * n * K + GUARD)
    return out


def same(name, got, want, itemsize, case):
    got, want = np.asarray(got).view(np.uint8).reshape(-1, itemsize), np.ascontiguousarray(want).view(np.uint8).reshape(-1, itemsize)
    assert got.shape == want.shape, (case, name, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got != want).any(axis=1))[0]
        raise AssertionError((case, name, "rows", bad[:8].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist()))


def check_against_model(K, n, contigs, out, rescue=True):
    """Every byte of what run_stages brought back, and the guards and the bytes the rule leaves alone."""
    import map_records_model as mm
    import pair_model as pm
    t = tables(K, n, contigs)
    pp = pm.params(17, rescue)
    rs, rz = pm.READ_SIZE, pm.RESCUE_SIZE
    case = (K, n, contigs, rescue)
    if rescue:
        req, tpos, rows = pm.rescue_rows(pp, K, rs, t["ref_len"], n, t["read_len"], t["reads"], t["seg"], t["sam"], t["contig"], t["starts"], t["lens"])
        same("req", out["req"][:16 * n], req, 16, case)
        same("tpos", out["tpos"][:8 * n], tpos, 8, case)
        pat = np.full(n * rz + GUARD, 0xEE, dtype=np.uint8)       # a pattern row: the read's row where there is a window, nothing anywhere else
        for b, row in rows.items():
            pat[b * rz:b * rz + rs] = row
        same("pat", out["pat"], pat, 1, case)
        assert (out["req"][16 * n:] == 0xEE).all() and (out["tpos"][8 * n:] == 0xEE).all(), case
        assert ((req["text_len"] <= rz) & (req["text_len"] >= req["pattern_len"])).all()
    pairs, seg, sam, cls, contig = pm.select(pp, K, rs, n, t["read_len"], t["seg"], t["sam"], t["cls"], t["contig"], t["res_sam"], CIGAR_BASE, MD_BASE)
    same("pairs", out["pairs"][:32 * (n // 2)], pairs, 32, case)
    assert (out["pairs"][32 * (n // 2):] == 0xEE).all(), case
    same("seg", out["seg"], seg, 8, case)
    same("sam", out["sam"], sam, 48, case)
    same("cls", out["cls"], cls, 8, case)
    if contigs:
        same("contig", out["contig"], contig, 4, case)
    off, rec = mm.map_records(K, n, seg, sam, cls)
    total = int(off[n])
    if contigs:                                                    # rule 13c's two changes to a record
        for o in rec:
            if o["sam"]["flags"] & mm.SAM_UNMAPPED:
                o["sam"]["pad"] = pm.CONTIG_NONE
            else:
                c = int(contig[o["slot"]])
                o["sam"]["pos"] = (int(o["sam"]["pos"]) - (int(t["starts"][c]) if c < len(t["starts"]) else 0)) & (2 ** 64 - 1)
                o["sam"]["pad"] = c
    same("rec_before", out["rec_before"][:64 * total], rec, 64, case)
    rec2, mates = pm.mates(K, n, pairs, seg, sam, contig, t["starts"], off, rec)
    same("off", out["off"], off, 4, case)
    same("rec", out["rec"][:64 * total], rec2, 64, case)
    same("mates", out["mates"][:16 * total], mates, 16, case)
    assert (out["rec"][64 * total:64 * n * K] == out["rec_before"][64 * total:]).all() and (out["rec"][64 * n * K:] == 0xEE).all(), case
    assert (out["mates"][16 * total:] == 0xEE).all(), case
    return pairs


@pytest.mark.parametrize("contigs", (False, True), ids=("one-seq", "contigs"))
@pytest.mark.parametrize("K", KS)
def test_stages_equal_model(K, contigs):
    import pair_model as pm
    with Hip() as h:
        for n in N_READS:
            pairs = check_against_model(K, n, contigs, run_stages(h, K, n, tables(K, n, contigs)))
            h.free()
            if n >= 130:                                           # the table holds what the rule distinguishes
                f = pairs["flags"]
                assert (f & pm.PROPER).any() and (f & (pm.RESCUED_A | pm.RESCUED_B)).any() and ((f & (pm.TRIED_A | pm.TRIED_B)) != 0).sum() > \
                    ((f & (pm.RESCUED_A | pm.RESCUED_B)) != 0).sum() and (pairs["n_best"] > 1).any(), (K, n)
                assert (pairs["span"][f & pm.PROPER != 0] == pm.MIN_SPAN).any() and (pairs["span"][f & pm.PROPER != 0] == pm.MAX_SPAN).any()
        check_against_model(K, 130, contigs, run_stages(h, K, 130, tables(K, 130, contigs), rescue=False), rescue=False)
        h.free()
        from aim_amd import engine                                 # an empty batch enqueues nothing and needs no buffer
        pp = engine.pair_params(pm.MIN_SPAN, pm.MAX_SPAN, rescue_size=pm.RESCUE_SIZE)
        engine.pair_rescue_rows_device(pp, K, pm.READ_SIZE, 1000, 0, None, None, None, None, None, None, None)
        engine.pair_select_device(pp, K, pm.READ_SIZE, 0, None, None, None, None, None, 0, 0, None)
        engine.map_mates_device(K, 0, None, None, None, None, None, None)


KNOB_CASES = ((4, 4100, True), (16, 130, False), (1, 4100, False), (6, 4100, True), (9, 130, False))     # the last two: 8 lanes, and 16 that K does not fill


def knob_batch():
    out = {}
    with Hip() as h:
        for i, (K, n, contigs) in enumerate(KNOB_CASES):
            for k, v in run_stages(h, K, n, tables(K, n, contigs)).items():
                out["%s_%d" % (k, i)] = v
            h.free()
    return out


@pytest.mark.parametrize("env", [{"AIM_CHIP_CUS": "1", "AIM_DEBUG_POISON_SCRATCH": "165", "AIM_DEBUG_POISON_OPS": "77", "AIM_DEBUG_POISON_LDS": "90"},
                                 {"AIM_CHIP_CUS": "256", "AIM_DEBUG_POISON_LDS": "255"}], ids=["cus1-poison", "cus256-lds255"])
def test_grid_and_poison_identical(tmp_path, env):
    """The same bytes -- the model's -- at AIM_CHIP_CUS 1 (8 workgroups walk the 33 blocks of read pairs and the 65 blocks of records)
    and 256, and under the three AIM_DEBUG_POISON_* knobs."""
    f = str(tmp_path / "k.npz")
    p = child.run("test_pairs_gpu", "knob_batch", npz=f, env=dict(env, AIM_PLAN_DEBUG="1"))
    grid, mgrid = (8, 8) if env["AIM_CHIP_CUS"] == "1" else (33, 65)
    assert "[aim plan] pair_rescue_rows_kernel grid=%d block=256 lanes=4 reads=4100 K=4 rescue_size=512" % grid in p.stderr, p.stderr
    assert "[aim plan] pair_select_kernel grid=%d block=256 lanes=4 reads=4100 K=4 rescue=1" % grid in p.stderr, p.stderr
    assert "[aim plan] map_mates_kernel grid=%d block=256 reads=4100 K=4" % mgrid in p.stderr, p.stderr
    assert "pair_select_kernel grid=5 block=256 lanes=16 reads=130 K=16" in p.stderr, p.stderr
    # the 8-lane path ran, and a 16-lane group of 9: the launchers' own rule, ceil(read pairs / (256 / lanes)) under the resident grid
    # of 8 workgroups per compute unit (the record kernels: ceil(reads / (256 / lanes)))
    resident = 8 * int(env["AIM_CHIP_CUS"])
    for lanes, n, K, records in ((8, 4100, 6, "map_records_contig_kernel"), (16, 130, 9, "map_records_kernel")):
        g, rg = min(resident, -(-(n // 2) // (256 // lanes))), min(resident, -(-n // (256 // lanes)))
        assert "[aim plan] pair_rescue_rows_kernel grid=%d block=256 lanes=%d reads=%d K=%d rescue_size=512" % (g, lanes, n, K) in p.stderr, p.stderr
        assert "[aim plan] pair_select_kernel grid=%d block=256 lanes=%d reads=%d K=%d rescue=1" % (g, lanes, n, K) in p.stderr, p.stderr
        assert re.search(r"\[aim plan\] map_count_kernel grid=%d block=256 lanes=%d reads=%d K=%d; scan parts=\d+ per_part=\d+; %s grid=%d block=256"
                         % (rg, lanes, n, K, records, rg), p.stderr), p.stderr
    out = np.load(f)
    for i, (K, n, contigs) in enumerate(KNOB_CASES):
        check_against_model(K, n, contigs, {k[:-2]: out[k] for k in out.files if k.endswith("_%d" % i)})


def same_after_renaming(K, K2, n, t2, a, b):
    """run_stages' bytes b over the tables t2 -- those of K padded to K2 slots per read (tests/slot_padding.py) -- against a, the bytes
    over the tables themselves: what is per read is the same, slot numbers are renamed, apply leaves the empty slots as they were."""
    import pair_model as pm
    import slot_padding as sp
    case = (K, K2, n)
    for k in ("req", "tpos", "pat", "off"):                        # (the rescue rows run with rescue alone)
        if k in a:
            same(k, b[k], a[k], 1, case)
    npairs = 32 * (n // 2)
    same("pairs", b["pairs"][:npairs], sp.pairs_renamed(a["pairs"][:npairs].view(pm.PAIR_DTYPE), K, K2), 32, case)
    assert (b["pairs"][npairs:] == 0xEE).all(), case
    for k, dt in (("seg", pm.SEG_DTYPE), ("sam", pm.SAM_DTYPE), ("cls", pm.CLASS_DTYPE), ("contig", np.dtype("<u4"))):
        if k in a:
            own, rest = sp.unpad(b[k].view(dt), K, K2, n)
            same(k, own, a[k], dt.itemsize, case)
            same(k + " of the empty slots", rest, sp.unpad(t2[k], K, K2, n)[1], dt.itemsize, case)
    total = int(a["off"].view(np.uint32)[n])
    for k in ("rec_before", "rec"):
        same(k, b[k][:64 * total], sp.records_renamed(a[k][:64 * total].view(pm.RECORD_DTYPE), K, K2), 64, case)
    same("mates", b["mates"][:16 * total], a["mates"][:16 * total], 16, case)
    assert (b["rec"][64 * n * K2:] == 0xEE).all() and (b["mates"][16 * total:] == 0xEE).all(), case


@pytest.mark.parametrize("contigs", (False, True), ids=("one-seq", "contigs"))
def test_empty_slots_change_nothing(contigs):
    """tests/slot_padding.py on the device: the tables of K = 3 with every read padded to 4, 8 and 16 slots -- the same read pairs in
    groups of 4, 8 and 16 lanes -- through the rescue rows, select / apply, the records and the mates, with and without rescue: every
    byte of K = 3, slot numbers renamed. Those of K = 3 are the model's."""
    import pair_model as pm
    import slot_padding as sp
    K, n = 3, N_READS[1]
    t = tables(K, n, contigs)
    with Hip() as h:
        for rescue in (True, False):
            a = run_stages(h, K, n, t, rescue=rescue)
            h.free()
            f = check_against_model(K, n, contigs, a, rescue=rescue)["flags"]
            assert (f & pm.PROPER).any() and bool((f & (pm.RESCUED_A | pm.RESCUED_B)).any()) == rescue
            for K2 in (4, 8, 16):
                t2 = sp.pad_tables(t, K, K2, n)
                same_after_renaming(K, K2, n, t2, a, run_stages(h, K2, n, t2, rescue=rescue))
                h.free()


# ---- the mapper with pairing ---------------------------------------------------------------------------------------------------------
def make_mapper(mp, contigs):
    import pair_batch as pb
    from aim_amd import engine
    return engine.Mapper.from_contigs(mp, pb.contigs()) if contigs else engine.Mapper(mp, pb.reference())


def map_pairs(contigs, rescue, rl=None, rows=None, **caps):
    """The paired batch (or the reads given) through a mapper with pairing: (a detached result, the contig layout or None)."""
    import pair_batch as pb
    b = pb.batch()
    rl, rows = (b["read_len"], b["rows"]) if rl is None else (rl, rows)
    with make_mapper(pb.mapper_params(max(len(rl), 2)), contigs) as m:
        m.set_pairing(pb.pair_params(max(len(rl), 2), rescue, **caps))
        m.submit(0, rl, rows)
        return copy_out(m.wait(0)), m.contigs


def hand_path(contigs, rescue):
    """The stages one by one on torch buffers, one synchronize per stage: the split path to sam_device_split (with the contig clip for
    three contigs), the rescue rows through their kernel (checked against the model on the way), aim_align_device_ref and aim_sam_device
    over them behind the main CIGAR / MD regions, then the numpy model of select / apply, of the records and of the mate fields over the
    downloaded rows: a dict shaped like a mapper result."""
    import torch
    import contig_model as cg
    import map_records_model as mm
    import pair_batch as pb
    import pair_model as pm
    from aim_amd import capi, engine
    b = pb.batch()
    rows, rl = b["rows"], b["read_len"]
    K, rs, rz, flank, n = pb.K, pb.READ_SIZE, pb.RESCUE_SIZE, pb.FLANK, len(b["read_len"])
    starts = lens = None
    if contigs:
        seqs = pb.contigs()
        ref = engine.contigs_concat(seqs, capi.CONTIG_SPACER(pb.BAND))
        starts, _ = engine.contigs_layout([len(s) for s in seqs], capi.CONTIG_SPACER(pb.BAND))
        lens = np.array([len(s) for s in seqs], dtype=np.uint32)
    else:
        ref = pb.reference()
    dev = hs.DEV
    params = hs.wfa_params(pb.MAX_SCORE, rs, pb.X, pb.O, pb.E, 2 * flank)
    rparams = hs.wfa_params(pb.MAX_SCORE, rz, pb.X, pb.O, pb.E, rz)
    rows_n = n * K
    d_ref = put(ref, dev, 64)
    out = hs.segment_rows(pb.seed_params(), ref, rl, rows)
    d_ct, d_st, d_ln = hs.clip_contigs(out, K, rs, flank, len(ref), starts, lens, n) if contigs else (None, None, None)
    ptr = lambda t: None if t is None else t.data_ptr()
    ccap, mcap, rccap, rmcap = rows_n * 64, rows_n * 256, n * 64, n * 256
    d_cigar, d_md = zeros((ccap + rccap) * 4, dev), zeros(mcap + rmcap, dev)           # the rescue records go behind the main regions
    d_res, d_ops = hs.align_rows(params, rows_n, out["d_seg_req"], out["d_seg_patterns"], out["d_seg_text_pos"], d_ref, len(ref))
    last = hs.sam_rows(params, rows_n, out["d_seg_req"], out["d_seg_text_pos"], d_res, d_ops, d_ref, len(ref), (ccap, mcap), split_seg=out["d_seg"],
                       into=(d_cigar, d_md, 0, 0))
    d_sam, sam = last["d_sam"], last["sam"]
    seg = out["d_seg"].cpu().numpy().view(capi.SEGMENT_DTYPE)[:rows_n].copy()
    contig = d_ct.cpu().numpy().view(np.uint32).copy() if contigs else None
    pp = pm.Params(pb.MIN_SPAN, pb.MAX_SPAN, pb.UNPAIRED_PENALTY, pm.RESCUE if rescue else 0, rz)
    res_sam = None
    needed = [0, 0]
    if rescue:
        d_rreq, d_rtp, d_rpat = zeros(16 * n, dev), zeros(8 * n, dev), zeros(n * rz + 64, dev)
        engine.pair_rescue_rows_device(pb.pair_params(n), K, rs, len(ref), n, out["d_read_len"].data_ptr(), out["d_reads"].data_ptr(), out["d_seg"].data_ptr(),
                                       d_sam.data_ptr(), d_rreq.data_ptr(), d_rtp.data_ptr(), d_rpat.data_ptr(), d_contig=ptr(d_ct), n_contigs=len(starts) if contigs else 0,
                                       d_contig_start=ptr(d_st), d_contig_len=ptr(d_ln))
        torch.cuda.synchronize()
        want_req, want_tp, want_rows = pm.rescue_rows(pp, K, rs, len(ref), n, rl, rows, seg, sam, contig, starts, lens)
        assert d_rreq.cpu().numpy()[:16 * n].tobytes() == want_req.tobytes() and d_rtp.cpu().numpy()[:8 * n].tobytes() == want_tp.tobytes()
        d_rres, d_rops = hs.align_rows(rparams, n, d_rreq, d_rpat, d_rtp, d_ref, len(ref))
        last = hs.sam_rows(rparams, n, d_rreq, d_rtp, d_rres, d_rops, d_ref, len(ref), (rccap, rmcap), into=(d_cigar, d_md, ccap, mcap))
        res_sam, needed = last["sam"], last["cur"].tolist()
        empty = want_req["pattern_len"] == 0                      # an empty row comes back unmapped at position 0, as the rule says
        assert (res_sam["flags"][empty] == pm.SAM_UNMAPPED).all() and (res_sam["pos"][empty] == 0).all() and (res_sam["n_cigar"][empty] == 0).all()
    pairs, seg2, sam2, cls2, contig2 = pm.select(pp, K, rs, n, rl, seg, sam, out["class"], contig, res_sam, ccap, mcap)
    off, rec = cg.records(K, n, seg2, sam2, cls2, contig2, starts) if contigs else mm.map_records(K, n, seg2, sam2, cls2)
    rec2, mates = pm.mates(K, n, pairs, seg2, sam2, contig2, starts, off, rec)
    return {"records": rec2, "rec_offsets": off, "cigar": last["cigar"], "md": last["md"], "mates": mates, "pairs": pairs,
            "rescue_cigar_needed": needed[0], "rescue_md_needed": needed[1]}


def check_truth(got, layout, contigs, rescue):
    """The mapper's records against where the mates were cut from, class by class."""
    import pair_batch as pb
    import pair_model as pm
    b = pb.batch()
    rec, off, mates, pairs = got["records"], got["rec_offsets"], got["mates"], got["pairs"]
    U, R = pm.SAM_UNMAPPED, pm.SAM_REVERSE

    def primary(r):
        g = range(int(off[r]), int(off[r + 1]))
        p = [i for i in g if not int(rec["sam"]["flags"][i]) & 0x800]
        assert len(p) == 1, (r, p)
        return p[0]

    def local(tm):
        c, base = pb.contig_of(tm[0]) if contigs else (0, 0)
        return c, tm[0] - base

    def at_truth(i, tm):
        s = rec["sam"][i]
        c, lo = local(tm)
        return not s["flags"] & U and bool(s["flags"] & R) == bool(tm[2]) and int(s["pos"]) == lo and int(s["ref_span"]) == pb.L and int(s["pad"]) == c
    seen = {c: 0 for c in pb.CLASSES}
    for m, t in enumerate(b["truth"]):
        c, q, F = t["cls"], t["q"], t["span"]
        i0, i1 = primary(2 * m), primary(2 * m + 1)
        f = int(pairs["flags"][m])
        fl0, fl1 = int(rec["sam"]["flags"][i0]), int(rec["sam"]["flags"][i1])
        assert fl0 & 0x41 == 0x41 and fl1 & 0x81 == 0x81 and not fl0 & 0x80 and not fl1 & 0x40
        across = c == "g" and q >= 4
        lost = c == "b" or (c == "g" and q < 4)                    # mate 2 has no chain: only a rescue places it
        if c == "a" or (across and not contigs) or ((lost or c == "c") and rescue):
            want = pm.PROPER | ((pm.TRIED_B | pm.RESCUED_B) if lost else 0) | ((pm.TRIED_A | pm.TRIED_B | pm.RESCUED_B) if c == "c" else 0)
            assert f == want, (m, c, f, want)
            assert at_truth(i0, t["mates"][0]) and at_truth(i1, t["mates"][1]), (m, c, rec["sam"][i0], rec["sam"][i1])
            assert int(pairs["span"][m]) == F and sorted((int(mates["tlen"][i0]), int(mates["tlen"][i1]))) == [-F, F] and fl0 & 0x2 and fl1 & 0x2
            assert (int(mates["tlen"][i0]) < 0) == bool(fl0 & R) and bool(fl0 & 0x20) == bool(fl1 & R) and bool(fl1 & 0x20) == bool(fl0 & R)
            assert int(mates["mate_pos"][i0]) == int(rec["sam"]["pos"][i1]) and int(mates["mate_pos"][i1]) == int(rec["sam"]["pos"][i0])
            assert int(mates["mate_contig"][i0]) == int(rec["sam"]["pad"][i1]) and int(off[2 * m + 2]) - int(off[2 * m + 1]) == 1
            if lost or c == "c":
                assert int(rec["sam"]["cigar_offset"][i1]) >= len(b["read_len"]) * pb.K * 64 and int(rec["sam"]["score"][i1]) == (30 if lost else 0)
                assert int(pairs["slot"][m][1]) == (2 * m + 1) * pb.K + pb.K and int(rec["slot"][i1]) == (2 * m + 1) * pb.K
        else:
            assert not f & pm.PROPER and int(pairs["span"][m]) == 0 and mates["tlen"][i0] == 0 and mates["tlen"][i1] == 0 and not (fl0 | fl1) & 0x2, (m, c, f)
            if c == "c":                                           # without rescue mate 2 stays on the far copy
                far = (t["mates"][1][0] - pb.REPEAT_B + pb.REPEAT_A, 0, t["mates"][1][2])
                assert not rescue and f == 0 and at_truth(i0, t["mates"][0]) and at_truth(i1, far), (m, rec["sam"][i1])
            elif c == "d":
                assert f == ((pm.TRIED_A | pm.TRIED_B) if rescue else 0) and at_truth(i0, t["mates"][0]) and at_truth(i1, t["mates"][1])
                assert not (fl0 | fl1) & 0x8 and int(mates["mate_pos"][i0]) == int(rec["sam"]["pos"][i1]) and bool(fl0 & 0x20) == bool(fl1 & R)
            elif c == "e" or lost:
                assert f == (pm.TRIED_B if rescue else 0) and at_truth(i0, t["mates"][0]) and fl1 & U and fl0 & 0x8 and not fl1 & 0x8
                assert bool(fl1 & 0x20) == bool(fl0 & R) and int(mates["mate_pos"][i1]) == int(rec["sam"]["pos"][i0]) == int(mates["mate_pos"][i0])
                assert int(mates["mate_contig"][i1]) == int(rec["sam"]["pad"][i0]) == int(mates["mate_contig"][i0])
            elif c == "f":
                assert f == 0 and fl0 == 0x1 | 0x4 | 0x8 | 0x40 and fl1 == 0x1 | 0x4 | 0x8 | 0x80
                assert int(mates["mate_pos"][i0]) == 0 and int(mates["mate_contig"][i0]) == (pm.CONTIG_NONE if contigs else 0)
            else:                                                  # g across the cut on three contigs: both placed, each inside its contig, never proper
                assert across and contigs and f == ((pm.TRIED_A | pm.TRIED_B) if rescue else 0), (m, c, f)
                assert at_truth(i0, t["mates"][0]) and at_truth(i1, t["mates"][1]) and rec["sam"]["pad"][i0] == 0 and rec["sam"]["pad"][i1] == 1
                assert int(mates["mate_contig"][i0]) == 1 and int(mates["mate_contig"][i1]) == 0
        seen[c] += 1
    if contigs:                                                    # every mapped record lies inside its contig
        ok = (rec["sam"]["flags"] & U) == 0
        assert (rec["sam"]["pos"][ok] + rec["sam"]["ref_span"][ok] <= layout[1][rec["sam"]["pad"][ok]]).all()
    assert all(v == pb.PER_CLASS for v in seen.values())


def end_to_end():
    """The paired batch through aim_mapper_t with pairing against hand_path -- records in canon form, rec_offsets, mates and pairs, byte for
    byte -- and against the truth: one sequence and three contigs, each with and without rescue. Then a mapper on which set_pairing
    was never called against the hand-driven single-end path of tests/hand_stages.py over its batch."""
    import mapper_batch as mb
    for contigs, rescue in ((False, True), (True, True), (False, False), (True, False)):
        got, layout = map_pairs(contigs, rescue)
        want = hand_path(contigs, rescue)
        g, w = mb.canon(got), mb.canon(want)
        assert g[1] == w[1], "rec_offsets"
        assert g[0] == w[0], ("records", contigs, rescue, np.nonzero(np.frombuffer(g[0], dtype=np.uint8) != np.frombuffer(w[0], dtype=np.uint8))[0][:8] // 64)
        assert g[2] == w[2] and g[3] == w[3], "CIGAR words or MD bytes"
        assert got["mates"].tobytes() == want["mates"].tobytes() and got["pairs"].tobytes() == want["pairs"].tobytes(), (contigs, rescue)
        assert (got["rescue_cigar_needed"], got["rescue_md_needed"]) == (want["rescue_cigar_needed"], want["rescue_md_needed"])
        assert got["rescue_cigar_words"] == got["rescue_cigar_needed"] and bool(got["rescue_cigar_needed"]) == rescue
        check_truth(got, layout, contigs, rescue)
        print("contigs", contigs, "rescue", rescue, "records", len(got["records"]), "proper", int((got["pairs"]["flags"] & 1).sum()), "rescue words", got["rescue_cigar_needed"])
    b = mb.batch()
    plain = mb.map_alone(mb.mapper_params(len(b["read_len"]), False), b["ref"], b["read_len"], b["rows"])
    assert "pairs" not in plain and mb.canon(plain) == mb.canon(hs.single_end(False))


def test_mapper_with_pairing_equals_the_stages_by_hand_and_the_truth():
    p = child.run("test_pairs_gpu", "end_to_end", cuda_first=True, marker="PAIRS_END_TO_END_OK", check=False)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "PAIRS_END_TO_END_OK" in p.stdout, p.stdout + p.stderr


def canon_pairs(out):
    """mapper_batch.canon plus the mate fields, the pairs and the rescue regions' counts (a cursor left over from the slot's last batch
    would show in them)."""
    import mapper_batch as mb
    return mb.canon(out) + (out["mates"].tobytes(), out["pairs"].tobytes(), out["rescue_cigar_needed"], out["rescue_md_needed"], out["rescue_cigar_words"],
                            out["rescue_md_bytes"], len(out["rescue_cigar"]), len(out["rescue_md"]))


def test_two_slots_reuse_empty_batch_and_a_rescue_region_too_small():
    import pair_batch as pb
    import pair_model as pm
    from aim_amd import capi, engine
    b = pb.batch()
    rows, rl = b["rows"], b["read_len"]
    A, B, C3 = slice(0, 48), slice(48, 112), slice(16, 64)
    alone = {k: canon_pairs(map_pairs(False, True, rl[s], rows[s])[0]) for k, s in (("A", A), ("B", B), ("C", C3))}
    assert alone["A"] != alone["C"] and alone["B"] != alone["C"]
    with make_mapper(pb.mapper_params(64, slots=2), False) as m:
        with pytest.raises(capi.AimError) as e:
            m.pairs(0)
        assert e.value.code == capi.AIM_ESTATE and "aim_mapper_set_pairing was not called" in str(e.value)
        m.submit(0, rl[A], rows[A])
        with pytest.raises(capi.AimError) as e:                    # legal only while no slot is in flight
            m.set_pairing(pb.pair_params(64))
        assert e.value.code == capi.AIM_ESTATE and "slot 0 is in flight" in str(e.value)
        m.wait(0)
        m.set_pairing(pb.pair_params(64))
        with pytest.raises(capi.AimError) as e:
            m.set_pairing(pb.pair_params(64))
        assert e.value.code == capi.AIM_ESTATE and "already set" in str(e.value)
        with pytest.raises(capi.AimError) as e:
            m.pairs(0)
        assert e.value.code == capi.AIM_ESTATE
        with pytest.raises(capi.AimError) as e:
            m.submit(0, rl[:3], rows[:3])
        assert e.value.code == capi.AIM_EINVAL and "n_reads 3 is odd" in str(e.value)
        m.submit(0, rl[A], rows[A])
        m.submit(1, rl[B], rows[B])
        assert canon_pairs(m.wait(0)) == alone["A"] and canon_pairs(m.wait(1)) == alone["B"]
        for s in (B, A, C3):                                       # the longer batch first: what it left behind must not show
            m.submit(1, rl[s], rows[s])
            last = canon_pairs(m.wait(1))
        assert last == alone["C"]
        m.submit(0, rl[:0], rows[:0])
        out = m.wait(0)
        assert out["n_reads"] == 0 and len(out["records"]) == 0 and len(out["mates"]) == 0 and len(out["pairs"]) == 0 and out["rescue_cigar_needed"] == 0
    full, _ = map_pairs(False, True)
    need_c, need_m = full["rescue_cigar_needed"], full["rescue_md_needed"]
    assert need_c > 8 and need_m > 8
    small, _ = map_pairs(False, True, rescue_cigar_cap=need_c // 2, rescue_md_cap=need_m)
    over = (small["records"]["sam"]["status"] & pm.mm.SAM_OVERFLOW) != 0
    assert small["rescue_cigar_needed"] == need_c > small["rescue_cigar_words"] == need_c // 2 and over.any()
    assert (small["records"]["sam"]["n_cigar"][over] == 0).all() and (small["pairs"]["flags"][small["records"]["read"][over] // 2] & (pm.RESCUED_A | pm.RESCUED_B)).all()
    assert small["pairs"].tobytes() == full["pairs"].tobytes() and small["mates"].tobytes() == full["mates"].tobytes()


def test_command_line_with_reads2(tmp_path):
    """python -m aim_amd.map --reads2 over the paired batch cut into three contigs, two batches over its two slots: the lines samout
    writes for the mapper's own result of the whole batch, mate columns included."""
    import pair_batch as pb
    from aim_amd import samout
    b = pb.batch()
    rows, rl = b["rows"], b["read_len"]
    n = len(rl)
    seqs = pb.contigs()
    names = ["c%d" % i for i in range(len(seqs))]
    (tmp_path / "ref.fa").write_bytes(b"".join(b">%s\n%s\n" % (nm.encode(), s.tobytes()) for nm, s in zip(names, seqs)))
    for x in range(2):
        with open(tmp_path / ("r%d.fq" % (x + 1)), "wb") as f:
            for m in range(n // 2):
                f.write(b"@pair%d/%d\n%s\n+\n%s\n" % (m, x + 1, rows[2 * m + x, :rl[2 * m + x]].tobytes(), b"I" * int(rl[2 * m + x])))
    cmd = [sys.executable, "-m", "aim_amd.map", "--contigs", "--ref", str(tmp_path / "ref.fa"), "--reads", str(tmp_path / "r1.fq"), "--reads2", str(tmp_path / "r2.fq"),
           "-o", str(tmp_path / "out.sam"), "--batch", "64", "--read-size", str(pb.READ_SIZE), "-k", str(pb.K_MER), "-w", str(pb.W), "--max-occ", str(pb.MAX_OCC),
           "--band", str(pb.BAND), "--flank", str(pb.FLANK), "--min-votes", str(pb.MIN_VOTES), "--max-cands", str(pb.K), "--max-score", str(pb.MAX_SCORE),
           "--min-span", str(pb.MIN_SPAN), "--max-span", str(pb.MAX_SPAN), "--unpaired-penalty", str(pb.UNPAIRED_PENALTY), "--rescue-size", str(pb.RESCUE_SIZE)]
    p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    body = [l for l in open(tmp_path / "out.sam").read().splitlines() if not l.startswith("@")]
    got, _ = map_pairs(True, True)
    want = samout.record_lines(got, ["pair%d" % (r // 2) for r in range(n)], rows, rl, names, ["I" * int(x) for x in rl])
    assert body == want and len(body) == len(got["records"])
    cols = [l.split("\t") for l in body]
    assert sum(1 for c in cols if int(c[1]) & 0x2) == 2 * int((got["pairs"]["flags"] & 1).sum()) and any(c[6] == "=" and int(c[8]) < 0 for c in cols)
    assert any(int(c[1]) & 0x4 and c[2] != "*" for c in cols) and any(c[6] not in ("=", "*") for c in cols)      # placed at the mate; a mate on another contig
