"""Rule 17c on the GPU. aim_pair_rescue_rows_secondary_device, aim_pair_select_secondary_device (apply included), rule 16c's record
kernel behind them and aim_map_mates_secondary_device on synthetic slot tables (tests/pair_secondary_batch.py) against the numpy model
(tests/pair_secondary_model.py), every output byte -- the rescue rows and the pattern rows, aim_map_pair_t and aim_map_pair_mapq_t, the
rewritten slot arrays and d_sec, the records, aim_map_sec_t and aim_map_mate_t -- for each K and batch size below, with and without
d_contig, with d_est NULL and given, with AIM_SEC_RECORDS on and off, on a small and a large grid and under the poison knobs; the
tables of K = 3 padded with empty slots to every group width against themselves (tests/slot_padding.py); the cases the rule names,
found in the batches; the reduction to rule 14c's own kernels on slot arrays without a secondary row; then aim_mapper_t with
aim_mapper_set_pairing_secondary on the four truth classes of tests/pair_secondary_batch.py, against the stages driven by hand (one
sequence and three contigs, with and without a tried rescue) and against the truth, two slots, a reused slot, an empty batch, a rescue
region too small, the setters' refusals, and `python -m aim_amd.map --reads2 ... --secondary N`."""
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
N_READS = (2, 130, 4100)            # one group, across wavefronts, and more read pairs than one workgroup of any K holds
GUARD = 64
CIGAR_BASE, MD_BASE = 1000, 70000
SEED = 21


def tables(K, n, contigs, secondaries=True):
    import pair_secondary_batch as pb
    return pb.tables(SEED, K, n, contigs, secondaries)


def run_stages(h, K, n, t, rescue=True, est=None, options=1):
    """The three entry points and rule 16c's record kernel over uploaded tables, in the order of the rule: rows, select / apply, records,
    mates. Every output buffer is prefilled with 0xEE and carries a guard. Returns the downloaded bytes by name."""
    import pair_secondary_batch as pb
    from aim_amd import engine
    rs, rz = pb.READ_SIZE, pb.RESCUE_SIZE
    p = pb.params(rescue)
    pp = engine.pair_params(p.min_span, p.max_span, p.unpaired_penalty, rescue=rescue, rescue_size=rz)
    ee = lambda nbytes: h.filled(nbytes + GUARD)
    contigs = t["contig"] is not None
    d_rl, d_reads = h.up(t["read_len"]), h.up(t["reads"], 16)
    d_seg, d_sam, d_cls, d_res_sam = h.up(t["seg"]), h.up(t["sam"]), h.up(t["cls"]), h.up(t["res_sam"])
    d_sec, d_chains = h.up(t["sec"]), h.up(t["chains"])
    d_est = h.up(est) if est is not None else None
    d_contig = h.up(t["contig"]) if contigs else None
    d_starts, d_lens = (h.up(t["starts"]), h.up(t["lens"])) if contigs else (None, None)
    nc = len(t["starts"]) if contigs else 0
    d_req, d_tp, d_pat = ee(16 * n), ee(8 * n), ee(n * rz)
    out = {}
    engine.pair_rescue_rows_secondary_device(pp, K, rs, t["ref_len"], n, d_rl, d_reads, d_seg, d_sam, d_sec, d_req, d_tp, d_pat, d_est=d_est, d_contig=d_contig,
                                             n_contigs=nc, d_contig_start=d_starts, d_contig_len=d_lens)
    out["req"], out["tpos"], out["pat"] = h.down(d_req, 16 * n + GUARD), h.down(d_tp, 8 * n + GUARD), h.down(d_pat, n * rz + GUARD)
    d_pairs, d_pq = ee(32 * (n // 2)), ee(16 * (n // 2))
    engine.pair_select_secondary_device(pp, K, rs, n, d_rl, d_seg, d_sam, d_cls, d_sec, d_chains, pb.SCORE_UNIT, d_res_sam if rescue else None, CIGAR_BASE, MD_BASE,
                                        d_pairs, d_pq, d_est=d_est, d_contig=d_contig)
    out["pairs"], out["pq"] = h.down(d_pairs, 32 * (n // 2) + GUARD), h.down(d_pq, 16 * (n // 2) + GUARD)
    out["seg"], out["sam"], out["cls"], out["sec"] = h.down(d_seg, 8 * n * K), h.down(d_sam, 48 * n * K), h.down(d_cls, 8 * n * K), h.down(d_sec, 8 * n * K)
    if contigs:
        out["contig"] = h.down(d_contig, 4 * n * K)
    d_off, d_rec, d_msec, d_mates = ee(4 * (n + 1)), ee(64 * n * K), ee(16 * n * K), ee(16 * n * K)
    sb = engine.map_records_scratch(n)
    d_scr = h.filled(sb)
    engine.map_records_secondary_device(K, n, options, d_seg, d_sam, d_cls, d_sec, d_off, d_rec, d_msec, d_scr, sb, d_contig=d_contig, n_contigs=nc, d_contig_start=d_starts)
    out["rec_before"], out["msec"] = h.down(d_rec, 64 * n * K), h.down(d_msec, 16 * n * K)
    engine.map_mates_secondary_device(K, n, d_pairs, d_seg, d_sam, d_sec, d_off, d_rec, d_mates, d_contig=d_contig, n_contigs=nc, d_contig_start=d_starts)
    out["off"], out["rec"], out["mates"] = h.down(d_off, 4 * (n + 1)), h.down(d_rec, 64 * n * K + GUARD), h.down(d_mates, 16 * n * K + GUARD)
    return out


def same(name, got, want, itemsize, case):
    got, want = np.asarray(got).view(np.uint8).reshape(-1, itemsize), np.ascontiguousarray(want).view(np.uint8).reshape(-1, itemsize)
    assert got.shape == want.shape, (case, name, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got != want).any(axis=1))[0]
        raise AssertionError((case, name, "rows", bad[:8].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist()))


def check_against_model(K, n, t, out, rescue=True, est=None, options=1):
    """Every byte of what run_stages brought back, and the guards and the bytes the rule leaves alone. Returns the model's outputs."""
    import pair_secondary_batch as pb
    rs, rz = pb.READ_SIZE, pb.RESCUE_SIZE
    case = (K, n, t["contig"] is not None, rescue, est is not None, options)
    w = pb.run_model(t, K, n, rescue=rescue, est=est, options=options, cigar_base=CIGAR_BASE, md_base=MD_BASE)
    same("req", out["req"][:16 * n], w["req"], 16, case)
    same("tpos", out["tpos"][:8 * n], w["tpos"], 8, case)
    pat = np.full(n * rz + GUARD, 0xEE, dtype=np.uint8)           # a pattern row: the read's row where there is a window, nothing anywhere else
    for b, row in w["rows"].items():
        pat[b * rz:b * rz + rs] = row
    same("pat", out["pat"], pat, 1, case)
    assert (out["req"][16 * n:] == 0xEE).all() and (out["tpos"][8 * n:] == 0xEE).all(), case
    assert rescue or not w["rows"]
    same("pairs", out["pairs"][:32 * (n // 2)], w["pairs"], 32, case)
    same("pair_mapq", out["pq"][:16 * (n // 2)], w["pq"], 16, case)
    assert (out["pairs"][32 * (n // 2):] == 0xEE).all() and (out["pq"][16 * (n // 2):] == 0xEE).all(), case
    same("seg", out["seg"], w["seg"], 8, case)
    same("sam", out["sam"], w["sam"], 48, case)
    same("cls", out["cls"], w["cls"], 8, case)
    same("sec", out["sec"], w["sec"], 8, case)
    if t["contig"] is not None:
        same("contig", out["contig"], w["contig"], 4, case)
    total = int(w["off"][n])
    same("off", out["off"], w["off"], 4, case)
    same("rec_before", out["rec_before"][:64 * total], w["rec_before"], 64, case)
    same("msec", out["msec"][:16 * total], w["msec"], 16, case)
    same("rec", out["rec"][:64 * total], w["rec"], 64, case)
    same("mates", out["mates"][:16 * total], w["mates"], 16, case)
    assert (out["rec"][64 * total:64 * n * K] == out["rec_before"][64 * total:]).all() and (out["rec"][64 * n * K:] == 0xEE).all(), case
    assert (out["mates"][16 * total:] == 0xEE).all(), case
    return w


def directed_cases(K, n, t, w):
    """How often the batch holds what the rule names: ties in both reads, a chosen secondary in a supplementary family, a chosen rescue
    row next to a family with secondaries, spans at both bounds, the unpaired cost equal to the pair's cost."""
    import pair_model as pm
    p, q, sec = w["pairs"], w["pq"], t["sec"]
    taken = (p["flags"] & pm.PROPER) != 0
    c = dict(ties_both=int(((q["tied"][:, 0] > 0) & (q["tied"][:, 1] > 0)).sum()), span_min=int((p["span"][taken] == pm.MIN_SPAN).sum()),
             span_max=int((p["span"][taken] == pm.MAX_SPAN).sum()), unpaired_equal=0, promoted=0, promoted_supplementary=0, rescued_next_to_secondaries=0)
    for m in np.nonzero(taken)[0]:
        c["unpaired_equal"] += int(p["score_sum"][m] in q["alt_sum"][m].tolist() and p["n_best"][m] == 1 and (q["tied"][m] == 0).all())
        for x in (0, 1):
            r, s = 2 * m + x, int(p["slot"][m][x])
            roles, fams = sec["role"][r * K:(r + 1) * K], sec["family"][r * K:(r + 1) * K]
            if s == r * K + K:
                c["rescued_next_to_secondaries"] += int((roles == 2).any())
            elif sec["role"][s] == 2:
                c["promoted"] += 1
                c["promoted_supplementary"] += int(int(sec["family"][s]) != int(fams[roles == 1].min()))
    return c


@pytest.mark.parametrize("contigs", (False, True), ids=("one-seq", "contigs"))
@pytest.mark.parametrize("K", KS)
def test_stages_equal_model(K, contigs):
    import pair_model as pm
    import pair_secondary_batch as pb
    with Hip() as h:
        for n in N_READS:
            t = tables(K, n, contigs)
            w = check_against_model(K, n, t, run_stages(h, K, n, t))
            h.free()
            if n == 4100:                                          # the table holds what the rule distinguishes
                f = w["pairs"]["flags"]
                assert (f & pm.PROPER).any() and (f & (pm.RESCUED_A | pm.RESCUED_B)).any() and ((f & (pm.TRIED_A | pm.TRIED_B)) != 0).sum() > \
                    ((f & (pm.RESCUED_A | pm.RESCUED_B)) != 0).sum(), (K, n)
                c = directed_cases(K, n, t, w)
                print(K, contigs, c)
                assert c["span_min"] and c["span_max"] and c["unpaired_equal"], c
                if K >= 4:
                    assert c["ties_both"] and c["promoted"] and c["promoted_supplementary"] and c["rescued_next_to_secondaries"], c
        t = tables(K, 130, contigs)
        est = pb.estimate()
        check_against_model(K, 130, t, run_stages(h, K, 130, t, est=est), est=est)                       # the bounds from d_est
        h.free()
        check_against_model(K, 130, t, run_stages(h, K, 130, t, options=0), options=0)                   # without AIM_SEC_RECORDS
        h.free()
        check_against_model(K, 130, t, run_stages(h, K, 130, t, rescue=False, est=est), rescue=False, est=est)
        h.free()
        from aim_amd import engine                                 # an empty batch enqueues nothing and needs no buffer
        pp = engine.pair_params(pm.MIN_SPAN, pm.MAX_SPAN, rescue_size=pm.RESCUE_SIZE)
        engine.pair_rescue_rows_secondary_device(pp, K, pm.READ_SIZE, 1000, 0, None, None, None, None, None, None, None, None)
        engine.pair_select_secondary_device(pp, K, pm.READ_SIZE, 0, None, None, None, None, None, None, 3, None, 0, 0, None, None)
        engine.map_mates_secondary_device(K, 0, None, None, None, None, None, None, None)


@pytest.mark.parametrize("contigs", (False, True), ids=("one-seq", "contigs"))
@pytest.mark.parametrize("K", (1, 4, 9, 16))
def test_reduces_to_rule_14c_kernels(K, contigs):
    """Slot arrays in which no secondary got a row: aim_map_pair_t, the rescue rows and the slot arrays after apply equal what rule 14c's
    own kernels give on the same tables, byte for byte."""
    import pair_secondary_batch as pb
    from aim_amd import engine
    n = 130
    t = tables(K, n, contigs, secondaries=False)
    rs, rz = pb.READ_SIZE, pb.RESCUE_SIZE
    with Hip() as h:
        a = run_stages(h, K, n, t)
        h.free()
        check_against_model(K, n, t, a)
        p = pb.params()
        pp = engine.pair_params(p.min_span, p.max_span, p.unpaired_penalty, rescue=True, rescue_size=rz)
        d_rl, d_reads = h.up(t["read_len"]), h.up(t["reads"], 16)
        d_seg, d_sam, d_cls, d_res_sam = h.up(t["seg"]), h.up(t["sam"]), h.up(t["cls"]), h.up(t["res_sam"])
        d_contig = h.up(t["contig"]) if contigs else None
        d_starts, d_lens = (h.up(t["starts"]), h.up(t["lens"])) if contigs else (None, None)
        nc = len(t["starts"]) if contigs else 0
        d_req, d_tp, d_pat, d_pairs = h.filled(16 * n + GUARD), h.filled(8 * n + GUARD), h.filled(n * rz + GUARD), h.filled(32 * (n // 2) + GUARD)
        engine.pair_rescue_rows_device(pp, K, rs, t["ref_len"], n, d_rl, d_reads, d_seg, d_sam, d_req, d_tp, d_pat, d_contig=d_contig, n_contigs=nc, d_contig_start=d_starts,
                                       d_contig_len=d_lens)
        engine.pair_select_device(pp, K, rs, n, d_rl, d_seg, d_sam, d_cls, d_res_sam, CIGAR_BASE, MD_BASE, d_pairs, d_contig=d_contig)
        case = (K, contigs)
        same("req", a["req"], h.down(d_req, 16 * n + GUARD), 16, case)
        same("tpos", a["tpos"], h.down(d_tp, 8 * n + GUARD), 8, case)
        same("pat", a["pat"], h.down(d_pat, n * rz + GUARD), 1, case)
        same("pairs", a["pairs"], h.down(d_pairs, 32 * (n // 2) + GUARD), 32, case)
        same("seg", a["seg"], h.down(d_seg, 8 * n * K), 8, case)
        same("sam", a["sam"], h.down(d_sam, 48 * n * K), 48, case)
        same("cls", a["cls"], h.down(d_cls, 8 * n * K), 8, case)
        if contigs:
            same("contig", a["contig"], h.down(d_contig, 4 * n * K), 4, case)


KNOB_CASES = ((4, 4100, True), (16, 130, False), (1, 4100, False), (6, 4100, True), (9, 130, False))     # the last two: 8 lanes, and 16 that K does not fill


def knob_batch():
    import pair_secondary_batch as pb
    out = {}
    with Hip() as h:
        for i, (K, n, contigs) in enumerate(KNOB_CASES):
            for k, v in run_stages(h, K, n, tables(K, n, contigs), est=pb.estimate() if i & 1 else None).items():
                out["%s_%d" % (k, i)] = v
            h.free()
    return out


@pytest.mark.parametrize("env", [{"AIM_CHIP_CUS": "1", "AIM_DEBUG_POISON_SCRATCH": "165", "AIM_DEBUG_POISON_OPS": "77", "AIM_DEBUG_POISON_LDS": "90"},
                                 {"AIM_CHIP_CUS": "256", "AIM_DEBUG_POISON_LDS": "255"}], ids=["cus1-poison", "cus256-lds255"])
def test_grid_and_poison_identical(tmp_path, env):
    """The same bytes -- the model's -- at AIM_CHIP_CUS 1 (8 workgroups walk the 33 blocks of read pairs and the 65 blocks of records)
    and 256, and under the three AIM_DEBUG_POISON_* knobs."""
    import pair_secondary_batch as pb
    f = str(tmp_path / "k.npz")
    p = child.run("test_pair_secondary_gpu", "knob_batch", npz=f, env=dict(env, AIM_PLAN_DEBUG="1"))
    grid, mgrid = (8, 8) if env["AIM_CHIP_CUS"] == "1" else (33, 65)
    assert "[aim plan] pair_sec_rescue_rows_kernel grid=%d block=256 lanes=4 reads=4100 K=4 rescue_size=512 est=0" % grid in p.stderr, p.stderr
    assert "[aim plan] pair_sec_select_kernel grid=%d block=256 lanes=4 reads=4100 K=4 rescue=1 est=0" % grid in p.stderr, p.stderr
    assert "[aim plan] map_mates_sec_kernel grid=%d block=256 reads=4100 K=4" % mgrid in p.stderr, p.stderr
    assert "pair_sec_select_kernel grid=5 block=256 lanes=16 reads=130 K=16 rescue=1 est=1" in p.stderr, p.stderr
    resident = 8 * int(env["AIM_CHIP_CUS"])
    for lanes, n, K in ((8, 4100, 6), (16, 130, 9)):               # the 8-lane path ran, and a 16-lane group of 9
        g = min(resident, -(-(n // 2) // (256 // lanes)))
        assert "[aim plan] pair_sec_select_kernel grid=%d block=256 lanes=%d reads=%d K=%d rescue=1" % (g, lanes, n, K) in p.stderr, p.stderr
    out = np.load(f)
    for i, (K, n, contigs) in enumerate(KNOB_CASES):
        check_against_model(K, n, tables(K, n, contigs), {k[:-2]: out[k] for k in out.files if k.endswith("_%d" % i)}, est=pb.estimate() if i & 1 else None)


def pad_tables(t, K, K2, n):
    """slot_padding.pad_tables plus rule 17c's two slot arrays: d_sec and d_chains padded with zero rows."""
    import slot_padding as sp
    out = sp.pad_tables(t, K, K2, n)
    out["sec"], out["chains"] = sp.pad(t["sec"], K, K2, n), sp.pad(t["chains"], K, K2, n)
    return out


@pytest.mark.parametrize("contigs", (False, True), ids=("one-seq", "contigs"))
def test_empty_slots_change_nothing(contigs):
    """tests/slot_padding.py on the device: the tables of K = 3 with every read padded to 4, 8 and 16 slots -- the same read pairs in
    groups of 4, 8 and 16 lanes -- through the four stages: every byte of K = 3, slot numbers renamed. Those of K = 3 are the model's."""
    import pair_model as pm
    import secondary_model as scm
    import slot_padding as sp
    K, n = 3, N_READS[1]
    t = tables(K, n, contigs)
    with Hip() as h:
        a = run_stages(h, K, n, t)
        h.free()
        check_against_model(K, n, t, a)
        total = int(a["off"].view(np.uint32)[n])
        npairs = n // 2
        for K2 in (4, 8, 16):
            t2 = pad_tables(t, K, K2, n)
            b = run_stages(h, K2, n, t2)
            h.free()
            case = (K, K2, n)
            for k in ("req", "tpos", "pat", "off", "pq"):
                same(k, b[k], a[k], 1, case)
            same("pairs", b["pairs"][:32 * npairs], sp.pairs_renamed(a["pairs"][:32 * npairs].view(pm.PAIR_DTYPE), K, K2), 32, case)
            for k, dt in (("seg", pm.SEG_DTYPE), ("sam", pm.SAM_DTYPE), ("cls", pm.CLASS_DTYPE), ("sec", scm.SEC_SLOT), ("contig", np.dtype("<u4"))):
                if k in a:
                    own, rest = sp.unpad(b[k].view(dt), K, K2, n)
                    same(k, own, a[k], dt.itemsize, case)
                    same(k + " of the empty slots", rest, sp.unpad(t2[k], K, K2, n)[1], dt.itemsize, case)
            for k in ("rec_before", "rec"):
                same(k, b[k][:64 * total], sp.records_renamed(a[k][:64 * total].view(pm.RECORD_DTYPE), K, K2), 64, case)
            same("mates", b["mates"][:16 * total], a["mates"][:16 * total], 16, case)
            msec = a["msec"][:16 * total].view(scm.MAP_SEC).copy()
            msec["family_slot"] = sp.rename(msec["family_slot"], a["rec"][:64 * total].view(pm.RECORD_DTYPE)["read"], K, K2)
            same("msec", b["msec"][:16 * total], msec, 16, case)


# ---- the mapper with aim_mapper_set_pairing_secondary ------------------------------------------------------------------------------------
MAX_SEC = 2


def stages_by_hand(ref, rows, rl, pp, options, contigs=None, max_score=None, expect_rescue=False):
    """Chain, classify, split, aim_secondary_rows_device, [aim_contig_clip_device,] the segment alignment and aim_sam_device_split,
    aim_secondary_select_device on torch buffers (as tests/test_secondary_gpu.py drives them), the rescue rows through their kernel
    (against the model), aim_align_device_ref and aim_sam_device over them behind the main CIGAR / MD regions (as tests/test_pairs_gpu.py
    drives them), then the numpy model of select / apply, rule 16c's records and the mate fields over the downloaded rows: a dict
    shaped like the mapper's result. contigs = (starts, lens): `ref` is their concatenation."""
    import chain_class_model as ccm
    import hand_stages as hs
    import mapper_batch as mb
    import pair_model as pm
    import pair_secondary_model as psm
    import secondary_model as scm
    import torch
    from aim_amd import capi, engine
    from gpu_buffers import put, zeros
    k, stride, w, max_occ, band, flank, min_votes, K = ccm.CHIMERIC_ROW
    rs, n, rz = ccm.CHIMERIC_SIZE, len(rl), int(pp.rescue_size)
    ms = mb.max_score() if max_score is None else max_score
    params, rparams = hs.wfa_params(ms, rs, mb.X, mb.O, mb.E, 2 * flank), hs.wfa_params(ms, rz, mb.X, mb.O, mb.E, rz)
    dev = hs.DEV
    d_ref = put(ref, dev, 64)
    sp = engine.seed_params(k, rs, stride=stride, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, max_cands=K, w=w)
    out = hs.segment_rows(sp, ref, rl, rows)
    engine.secondary_rows_device(K, rs, flank, len(ref), n, *[out[x].data_ptr() for x in ("d_read_len", "d_reads", "d_req", "d_text_pos", "d_seed", "d_chains", "d_class",
                                                                                         "d_seg_req", "d_seg_text_pos", "d_seg_patterns", "d_seg")], MAX_SEC)
    starts, lens = contigs if contigs is not None else (None, None)
    d_ct, d_st, d_ln = hs.clip_contigs(out, K, rs, flank, len(ref), starts, lens, n) if contigs is not None else (None, None, None)
    ptr = lambda t: None if t is None else t.data_ptr()
    nc = len(starts) if contigs is not None else 0
    rows_n = n * K
    ccap, mcap, rccap, rmcap = rows_n * 64, rows_n * 256, n * 64, n * 256
    d_cigar, d_md = zeros((ccap + rccap) * 4, dev), zeros(mcap + rmcap, dev)           # the rescue records go behind the main regions
    d_res, d_ops = hs.align_rows(params, rows_n, out["d_seg_req"], out["d_seg_patterns"], out["d_seg_text_pos"], d_ref, len(ref))
    last = hs.sam_rows(params, rows_n, out["d_seg_req"], out["d_seg_text_pos"], d_res, d_ops, d_ref, len(ref), (ccap, mcap), split_seg=out["d_seg"], into=(d_cigar, d_md, 0, 0))
    d_sam, sam = last["d_sam"], last["sam"]
    seg = out["d_seg"].cpu().numpy().view(capi.SEGMENT_DTYPE)[:rows_n].copy()
    contig = d_ct.cpu().numpy().view(np.uint32)[:rows_n].copy() if contigs is not None else None
    d_sec = zeros(8 * rows_n, dev)
    engine.secondary_select_device(K, n, out["d_seg"].data_ptr(), d_sam.data_ptr(), out["d_class"].data_ptr(), out["d_chains"].data_ptr(), ms, mb.X, d_sec.data_ptr())
    d_req, d_tp, d_pat = zeros(16 * n, dev), zeros(8 * n, dev), zeros(n * rz + 64, dev)
    engine.pair_rescue_rows_secondary_device(pp, K, rs, len(ref), n, out["d_read_len"].data_ptr(), out["d_reads"].data_ptr(), out["d_seg"].data_ptr(), d_sam.data_ptr(),
                                             d_sec.data_ptr(), d_req.data_ptr(), d_tp.data_ptr(), d_pat.data_ptr(), d_contig=ptr(d_ct), n_contigs=nc, d_contig_start=ptr(d_st),
                                             d_contig_len=ptr(d_ln))
    torch.cuda.synchronize()
    x = d_sec.cpu().numpy()[:8 * rows_n].view(scm.SEC_SLOT).copy()
    assert x.tobytes() == scm.select(K, n, seg, sam, out["class"], out["chains"], ms, mb.X).tobytes()
    mpp = pm.Params(pp.min_span, pp.max_span, pp.unpaired_penalty, pp.options, rz)
    want_req, want_tp, _ = psm.rescue_rows(mpp, K, rs, len(ref), n, rl, rows, seg, sam, x, contig, starts, lens)
    assert d_req.cpu().numpy()[:16 * n].tobytes() == want_req.tobytes() and d_tp.cpu().numpy()[:8 * n].tobytes() == want_tp.tobytes()
    assert bool(want_req["pattern_len"].any()) == expect_rescue, "whether a rescue is tried"
    d_rres, d_rops = hs.align_rows(rparams, n, d_req, d_pat, d_tp, d_ref, len(ref))
    last = hs.sam_rows(rparams, n, d_req, d_tp, d_rres, d_rops, d_ref, len(ref), (rccap, rmcap), into=(d_cigar, d_md, ccap, mcap))
    res_sam, needed = last["sam"], last["cur"].tolist()
    empty = want_req["pattern_len"] == 0                          # an empty row comes back unmapped at position 0, as rule 14c says
    assert (res_sam["flags"][empty] == pm.SAM_UNMAPPED).all() and (res_sam["pos"][empty] == 0).all()
    pairs, pq, seg2, sam2, cls2, contig2, sec2 = psm.select(mpp, K, rs, n, rl, seg, sam, out["class"], contig, x, out["chains"], res_sam, mb.X, ccap, mcap)
    off, rec, msec = scm.records(K, n, options, seg2, sam2, cls2, sec2, contig2, starts)
    rec2, mates = psm.mates(K, n, pairs, sam2, sec2, contig2, starts, off, rec)
    return {"records": rec2, "rec_offsets": off, "cigar": last["cigar"], "md": last["md"], "sec": msec, "pairs": pairs, "pair_mapq": pq, "mates": mates, "sec_before": x,
            "rescue_cigar_needed": needed[0], "rescue_md_needed": needed[1], "res_sam": res_sam}


def same_result(got, want):
    import mapper_batch as mb
    g, w = mb.canon(got), mb.canon(want)
    assert g[1] == w[1], "rec_offsets"
    assert g[0] == w[0], ("records", np.nonzero(np.frombuffer(g[0], dtype=np.uint8) != np.frombuffer(w[0], dtype=np.uint8))[0][:8] // 64)
    assert g[2] == w[2] and g[3] == w[3], "CIGAR words or MD bytes"
    for k in ("pairs", "pair_mapq", "mates", "sec"):
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k


def map_combined(ref, rl, rows, pp, max_score=None, contigs=False, records=True):
    """One batch through a mapper of its own with aim_mapper_set_pairing_secondary (contigs: `ref` is a list of sequences)."""
    import chain_class_model as ccm
    import mapper_batch as mb
    from aim_amd import engine
    from gpu_buffers import copy_out
    k, stride, w, max_occ, band, flank, min_votes, K = ccm.CHIMERIC_ROW
    sp = engine.seed_params(k, ccm.CHIMERIC_SIZE, stride=stride, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, max_cands=K, w=w)
    mp = engine.mapper_params(sp, len(rl), mb.max_score() if max_score is None else max_score, mismatch=mb.X, gap_o=mb.O, gap_e=mb.E)
    with (engine.Mapper.from_contigs(mp, ref) if contigs else engine.Mapper(mp, ref)) as m:
        if pp is not None:
            m.set_pairing_secondary(pp, engine.secondary_params(MAX_SEC, records=records)) if records is not None else m.set_pairing(pp)
        m.submit(0, rl, rows)
        return copy_out(m.wait(0))


def mapper_truth_class_2():
    """The diverged repeat, the read cut from copy B, the mate next to copy A. A penalty above the score difference: copy A, an aligned
    secondary, is promoted with mapq = 6 * (penalty - difference) / 3 and copy B becomes the 0x100 line. A penalty below it: the pair is
    not taken and the records are rule 16c's with mate flags and no 0x2. Both against the stages by hand."""
    import chain_class_model as ccm
    import mapper_batch as mb
    import pair_model as pm
    import pair_secondary_batch as pb
    import secondary_model as scm
    from aim_amd import engine
    K, rs = ccm.CHIMERIC_ROW[7], ccm.CHIMERIC_SIZE
    ref, rows, rl, truth, covered = pb.truth_class2()
    n = len(rl)
    inside = lambda o, a: a <= int(o["sam"]["pos"]) and int(o["sam"]["pos"]) + int(o["sam"]["ref_span"]) <= a + scm.REPEAT_LEN
    plain = map_combined(ref, rl, rows, None)                  # no setter at all: for the positions rule 16c alone reports, see below
    with engine.Mapper(mb.mapper_params(n, False), ref) as m:
        from gpu_buffers import copy_out
        m.set_secondary(engine.secondary_params(MAX_SEC, records=True))
        m.submit(0, rl, rows)
        alone = copy_out(m.wait(0))
    assert len(plain["records"]) == n
    for penalty in pb.T2_PENALTIES:
        pp = pb.truth_params(n, rs, penalty)
        got = map_combined(ref, rl, rows, pp)
        same_result(got, stages_by_hand(ref, rows, rl, pp, scm.SEC_RECORDS))
        rec, off, pairs, pq = got["records"], got["rec_offsets"], got["pairs"], got["pair_mapq"]
        for mm in range(n // 2):
            diff = mb.X * covered[mm]
            a, b = rec[off[2 * mm]:off[2 * mm + 1]], rec[off[2 * mm + 1]:off[2 * mm + 2]]
            p, q = pairs[mm], pq[mm]
            print(penalty, mm, p, q, [(int(o["sam"]["pos"]), hex(int(o["sam"]["flags"])), int(o["mapq"]), int(o["sam"]["score"])) for o in list(a) + list(b)])
            assert len(a) == 2 and len(b) == 1 and int(a[1]["sam"]["score"]) - int(a[0]["sam"]["score"]) in (diff, -diff)
            (lo, hi, strand), (mlo, mhi, _) = truth[mm]
            assert mlo <= int(b[0]["sam"]["pos"]) < mhi
            if penalty > diff:
                assert p["flags"] == pm.PROPER and p["slot"][0] == 2 * mm * K + 1 and p["n_best"] == 1, (mm, p)
                assert inside(a[0], scm.REPEAT_A) and int(a[0]["sam"]["flags"]) & 0x2 and not int(a[0]["sam"]["flags"]) & scm.SAM_SECONDARY
                assert inside(a[1], scm.REPEAT_B) and int(a[1]["sam"]["flags"]) & scm.SAM_SECONDARY and not int(a[1]["sam"]["flags"]) & 0x2 and a[1]["mapq"] == 0
                assert a[0]["mapq"] == q["mapq"][0] == q["pair_mapq"][0] == 6 * (penalty - diff) // mb.X and q["own_mapq"][0] == 0 and q["tied"][0] == 0, (mm, q, diff)
                assert q["alt_sum"][0] == p["score_sum"] - diff + penalty and q["pair_mapq"][1] == 60 and int(b[0]["sam"]["flags"]) & 0x2
            else:
                assert p["flags"] == 0 and p["n_best"] == 0 and p["slot"].tolist() == [2 * mm * K, (2 * mm + 1) * K] and p["second_sum"] == p["score_sum"] - penalty + diff, (mm, p)
                assert q["alt_sum"].tolist() == [pm.INT_MAX] * 2 and q.tobytes()[8:] == bytes(8)
                old = alone["records"][alone["rec_offsets"][2 * mm]:alone["rec_offsets"][2 * mm + 1]]
                assert len(old) == 2
                for o, was in zip(list(a) + list(b), list(old) + [alone["records"][alone["rec_offsets"][2 * mm + 1]]]):
                    f = int(o["sam"]["flags"])
                    assert not f & 0x2 and f & 0x1 and f & ~0xEB == int(was["sam"]["flags"]) and o["mapq"] == was["mapq"] and o["sam"]["pos"] == was["sam"]["pos"]
                assert inside(a[0], scm.REPEAT_B) and inside(a[1], scm.REPEAT_A)


def mapper_truth_class_3():
    """The diverged "tie" reads, whose rule-16c winner is the secondary, copy B, each with a substituted mate next to B: the rescue is
    anchored at B -- the representative, slot 1 -- and the mate comes back inside its true interval; with set_pairing alone the anchor is
    slot 0, copy A, and it does not. The combined mapper against the stages by hand with the rescue alignment, on one sequence and on
    three contigs, and with a rescue region that is too small."""
    import chain_class_model as ccm
    import mapper_batch as mb
    import pair_model as pm
    import pair_secondary_batch as pb
    import secondary_model as scm
    from aim_amd import capi, engine
    K, rs, ms = ccm.CHIMERIC_ROW[7], ccm.CHIMERIC_SIZE, pb.T3_MAX_SCORE
    ref, rows, rl, truth = pb.truth_class3()
    n = len(rl)
    pp = pb.truth_params(n, rs)
    got = map_combined(ref, rl, rows, pp, ms)
    want = stages_by_hand(ref, rows, rl, pp, scm.SEC_RECORDS, max_score=ms, expect_rescue=True)
    same_result(got, want)
    assert got["rescue_cigar_needed"] == want["rescue_cigar_needed"] > 0 and got["rescue_md_needed"] == want["rescue_md_needed"] > 0
    old = map_combined(ref, rl, rows, pp, ms, records=None)    # set_pairing alone: the anchor is rule 12c's lowest mapped slot, copy A
    rec, off, pairs, pq = got["records"], got["rec_offsets"], got["pairs"], got["pair_mapq"]
    for mm in range(n // 2):
        (lo, hi, strand), (mlo, mhi, mstrand) = truth[mm]
        p, q = pairs[mm], pq[mm]
        a, b = rec[off[2 * mm]:off[2 * mm + 1]], rec[off[2 * mm + 1]:off[2 * mm + 2]]
        print(mm, p, q, [(int(o["sam"]["pos"]), hex(int(o["sam"]["flags"])), int(o["mapq"]), int(o["sam"]["score"])) for o in list(a) + list(b)])
        assert want["sec_before"]["role"][2 * mm * K:2 * mm * K + 2].tolist() == [2, 1]                    # rule 16c's winner is slot 1
        assert p["flags"] == pm.PROPER | pm.TRIED_B | pm.RESCUED_B and p["slot"].tolist() == [2 * mm * K + 1, (2 * mm + 1) * K + K], (mm, p)
        assert len(b) == 1 and mlo - 3 <= int(b[0]["sam"]["pos"]) and int(b[0]["sam"]["pos"]) + int(b[0]["sam"]["ref_span"]) <= mhi + 3, (mm, b, mlo)
        assert int(b[0]["sam"]["score"]) == 30 * mb.X and int(b[0]["sam"]["flags"]) & 0x2 and bool(int(b[0]["sam"]["flags"]) & 0x10) == bool(mstrand)
        assert lo <= int(a[0]["sam"]["pos"]) and int(a[0]["sam"]["pos"]) + int(a[0]["sam"]["ref_span"]) <= hi and int(a[0]["sam"]["flags"]) & 0x2
        assert len(a) == 2 and int(a[1]["sam"]["flags"]) & scm.SAM_SECONDARY and scm.in_copy(int(a[1]["sam"]["pos"]), scm.REPEAT_A)
        assert q["own_mapq"].tolist() == [int(want["sec_before"]["mapq"][2 * mm * K + 1]), 0] and b[0]["mapq"] == q["mapq"][1] == min(40, int(q["mapq"][0])) and a[0]["mapq"] == q["mapq"][0]
        assert got["sec"][off[2 * mm + 1]]["n_members"] == 1 and got["sec"][off[2 * mm + 1]]["flags"] == scm.COMPLETE
        o = old["records"][old["rec_offsets"][2 * mm + 1]]
        assert not old["pairs"][mm]["flags"] & pm.PROPER and int(o["sam"]["flags"]) & pm.SAM_UNMAPPED, (mm, old["pairs"][mm])
        assert scm.in_copy(int(old["records"][old["rec_offsets"][2 * mm]]["sam"]["pos"]), scm.REPEAT_A)
    # three contigs: copy A in contig 0, copy B and the mates in contig 1; the clip, d_contig in select / apply and in the mate fields
    cuts = (8000, 16000)
    seqs = [ref[:cuts[0]], ref[cuts[0]:cuts[1]], ref[cuts[1]:]]
    spacer = ccm.CHIMERIC_ROW[4] + 64                          # AIM_CONTIG_SPACER(band), what the mapper uses
    cat = engine.contigs_concat(seqs, spacer)
    starts, lens = engine.contigs_layout([len(x) for x in seqs], spacer)[0], np.array([len(x) for x in seqs], dtype=np.uint32)
    got3 = map_combined(seqs, rl, rows, pp, ms, contigs=True)
    same_result(got3, stages_by_hand(cat, rows, rl, pp, scm.SEC_RECORDS, contigs=(starts, lens), max_score=ms, expect_rescue=True))
    for mm in range(n // 2):
        a = got3["records"][got3["rec_offsets"][2 * mm]:got3["rec_offsets"][2 * mm + 1]]
        b = got3["records"][got3["rec_offsets"][2 * mm + 1]]
        mt = got3["mates"][got3["rec_offsets"][2 * mm]:got3["rec_offsets"][2 * mm + 1]]
        assert got3["pairs"][mm]["flags"] == pm.PROPER | pm.TRIED_B | pm.RESCUED_B
        assert [int(o["sam"]["pad"]) for o in a] == [1, 0] and b["sam"]["pad"] == 1 and truth[mm][1][0] - cuts[0] - 3 <= int(b["sam"]["pos"]) <= truth[mm][1][0] - cuts[0] + 3
        assert mt["mate_contig"].tolist() == [1, 1] and mt["mate_pos"].tolist() == [int(b["sam"]["pos"])] * 2 and mt["tlen"][1] == 0 and mt["tlen"][0] != 0
    # a rescue region too small: the rescued records carry AIM_SAM_OVERFLOW and the needed sizes, everything else stays
    small = map_combined(ref, rl, rows, pb.truth_params(n, rs, rescue_cigar_cap=3, rescue_md_cap=5), ms)
    assert small["rescue_cigar_needed"] == got["rescue_cigar_needed"] > 3 and small["rescue_md_needed"] == got["rescue_md_needed"] > 5
    assert small["rescue_cigar_words"] == 3 and small["rescue_md_bytes"] == 5 and small["pairs"].tobytes() == got["pairs"].tobytes()
    assert small["pair_mapq"].tobytes() == got["pair_mapq"].tobytes() and small["mates"].tobytes() == got["mates"].tobytes()
    over = [bool(int(o["sam"]["status"]) & capi.SAM_OVERFLOW) for o in small["records"]]
    rescued = [int(o["read"]) & 1 == 1 for o in small["records"]]
    assert sum(over) >= n // 2 - 1 and all(r or not v for v, r in zip(over, rescued)), (sum(over), n)
    keep = [i for i, v in enumerate(over) if not v]
    assert small["records"][keep]["sam"]["pos"].tolist() == got["records"][keep]["sam"]["pos"].tolist() and small["records"]["mapq"].tolist() == got["records"]["mapq"].tolist()


@pytest.mark.parametrize("fn", ("mapper_truth_class_2", "mapper_truth_class_3"))
def test_mapper_truth_classes_2_and_3(fn):
    p = child.run("test_pair_secondary_gpu", fn, cuda_first=True, marker="PAIR_SECONDARY_%s_OK" % fn, check=False)
    print(p.stdout[-6000:])
    assert p.returncode == 0 and "PAIR_SECONDARY_%s_OK" % fn in p.stdout, p.stdout[-3000:] + p.stderr[-6000:]


def mapper_end_to_end():
    """Truth class 1 (tests/pair_secondary_batch.py) through a mapper with aim_mapper_set_pairing_secondary, against the stages by hand
    and against the truth; the same reads through set_secondary alone and through set_pairing alone; then two slots, a reused slot, an
    empty batch, the views' state rules and the setters' mutual refusals."""
    import chain_class_model as ccm
    import mapper_batch as mb
    import pair_model as pm
    import pair_secondary_batch as pb
    import secondary_model as scm
    from aim_amd import capi, engine
    from gpu_buffers import copy_out
    K, rs = ccm.CHIMERIC_ROW[7], ccm.CHIMERIC_SIZE
    ref, rows, rl, truth = pb.truth_class1()
    n = len(rl)
    pp = pb.truth_pair_params(n, rs)
    sc = engine.secondary_params(MAX_SEC, records=True)
    with engine.Mapper(mb.mapper_params(n, False, slots=2), ref) as m:
        m.set_pairing_secondary(pp, sc)
        with pytest.raises(capi.AimError) as e:                # before the first wait there is no view
            m.pair_mapq(0)
        assert e.value.code == capi.AIM_ESTATE
        m.submit(0, rl, rows)
        m.submit(1, rl[:8], rows[:8])                          # a second slot in flight next to it
        got = copy_out(m.wait(0))
        part = copy_out(m.wait(1))
        m.submit(0, rl[:0], rows[:0])                          # the slot reused, with an empty batch
        empty = m.wait(0)
        assert len(empty["records"]) == 0 and len(empty["pairs"]) == 0 and len(empty["pair_mapq"]) == 0 and len(empty["sec"]) == 0
        m.submit(0, rl, rows)
        again = copy_out(m.wait(0))
        for setter, words in ((lambda: m.set_pairing(pp), "pairs over secondaries"), (lambda: m.set_secondary(sc), "already set"),
                              (lambda: m.set_pairing_secondary(pp, sc), "already set")):
            with pytest.raises(capi.AimError) as e:
                setter()
            assert words in str(e.value), str(e.value)
    for a, b in ((mb.canon(again), mb.canon(got)),):
        assert a == b
    for k in ("pairs", "pair_mapq", "mates", "sec"):
        assert again[k].tobytes() == got[k].tobytes(), k
        assert part[k].tobytes() == got[k][:len(part[k])].tobytes(), k     # a prefix of the batch is the batch of fewer pairs
    want = stages_by_hand(ref, rows, rl, pp, scm.SEC_RECORDS)
    g, w = mb.canon(got), mb.canon(want)
    assert g[1] == w[1], "rec_offsets"
    assert g[0] == w[0], ("records", np.nonzero(np.frombuffer(g[0], dtype=np.uint8) != np.frombuffer(w[0], dtype=np.uint8))[0][:8] // 64)
    assert g[2] == w[2] and g[3] == w[3], "CIGAR words or MD bytes"
    for k in ("pairs", "pair_mapq", "mates", "sec"):
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k
    # against the truth: every pair of the class
    rec, off, pairs, pq, mates = got["records"], got["rec_offsets"], got["pairs"], got["pair_mapq"], got["mates"]
    inside = lambda o, a: a <= int(o["sam"]["pos"]) and int(o["sam"]["pos"]) + int(o["sam"]["ref_span"]) <= a + scm.REPEAT_LEN
    for mm in range(n // 2):
        (lo, hi, strand), (mlo, mhi, mstrand) = truth[mm]
        p = pairs[mm]
        assert p["flags"] == pm.PROPER and p["n_best"] == 1 and p["span"] == pb.T_SPAN, (mm, p)       # proper, and no rescue was tried
        a = rec[off[2 * mm]:off[2 * mm + 1]]
        b = rec[off[2 * mm + 1]:off[2 * mm + 2]]
        assert len(a) == 2 and len(b) == 1
        first, second, mate = a[0], a[1], b[0]
        fl = int(first["sam"]["flags"])
        assert lo <= int(first["sam"]["pos"]) and int(first["sam"]["pos"]) + int(first["sam"]["ref_span"]) <= hi and inside(first, scm.REPEAT_B)
        assert fl & 0x2 and fl & 0x1 and fl & 0x40 and not fl & (scm.SAM_SECONDARY | 0x800) and bool(fl & 0x10) == bool(strand) and bool(fl & 0x20) == bool(mstrand)
        sf = int(second["sam"]["flags"])
        assert sf & scm.SAM_SECONDARY and inside(second, scm.REPEAT_A) and sf & 0x1 and sf & 0x40 and not sf & 0x2 and bool(sf & 0x20) == bool(mstrand) and second["mapq"] == 0
        ma, mb_ = mates[off[2 * mm]], mates[off[2 * mm] + 1]
        assert ma["mate_pos"] == mb_["mate_pos"] == int(mate["sam"]["pos"]) and mlo <= int(mate["sam"]["pos"]) < mhi and mb_["tlen"] == 0
        assert abs(int(ma["tlen"])) == pb.T_SPAN and int(mates[off[2 * mm + 1]]["tlen"]) == -int(ma["tlen"])
        want_q = min(60, 6 * pb.T_PENALTY // mb.X)             # own 0 (a promoted secondary), the alternative is the unpaired cost
        assert first["mapq"] == pq["mapq"][mm][0] == min(want_q, 40) and first["mapq"] >= 20 and pq["own_mapq"][mm][0] == 0 and pq["tied"][mm][0] == 0, (mm, pq[mm], first["mapq"])
        assert pq["pair_mapq"][mm][1] == 60 and mate["mapq"] == pq["mapq"][mm][1] >= pq["own_mapq"][mm][1] and int(mate["sam"]["flags"]) & 0x2
        assert got["sec"][off[2 * mm]]["flags"] & scm.SWAPPED and first["slot"] == 2 * mm * K + 1
    # set_secondary alone: copy A with MAPQ 0; set_pairing alone: copy B only with the rescue tried
    with engine.Mapper(mb.mapper_params(n, False), ref) as m:
        m.set_secondary(sc)
        m.submit(0, rl, rows)
        alone = copy_out(m.wait(0))
    with engine.Mapper(mb.mapper_params(n, False), ref) as m:
        m.set_pairing(pp)
        m.submit(0, rl, rows)
        paired = copy_out(m.wait(0))
    for mm in range(n // 2):
        o = alone["records"][alone["rec_offsets"][2 * mm]]
        assert inside(o, scm.REPEAT_A) and o["mapq"] == 0
        p = paired["pairs"][mm]
        o = paired["records"][paired["rec_offsets"][2 * mm]]
        assert p["flags"] & (pm.TRIED_A | pm.TRIED_B) and (not inside(o, scm.REPEAT_B) or p["flags"] & pm.RESCUED_A), (mm, p)
    # the setter's refusals in their order: aim_mapper_set_pairing's of pp, then ep's, then rule 16c's of sp; a refused call leaves the mapper usable
    with engine.Mapper(mb.mapper_params(n, False), ref) as m:
        bad_pp, bad_ep, bad_sc = pb.truth_pair_params(n, rs), engine.pair_estimate_params(hist_size=100), engine.secondary_params(0)
        bad_pp.unpaired_penalty = -1
        for args, words in (((bad_pp, bad_sc, bad_ep), "unpaired_penalty -1"), ((pp, bad_sc, bad_ep), "hist_size 100"), ((pp, bad_sc, None), "max_sec 0"),
                            ((pp, bad_sc, engine.pair_estimate_params()), "max_sec 0")):
            with pytest.raises(capi.AimError) as e:
                m.set_pairing_secondary(args[0], args[1], estimate=args[2])
            assert e.value.code == capi.AIM_EINVAL and "aim_mapper_set_pairing_secondary: " in str(e.value) and words in str(e.value), str(e.value)
        m.set_pairing_secondary(pp, sc, estimate=engine.pair_estimate_params(min_samples=4))      # with the estimate: the three views work
        m.submit(0, rl, rows)
        est = copy_out(m.wait(0))
        assert est["pair_estimate"]["n_samples"] >= 0 and len(est["pair_mapq"]) == n // 2 and len(est["sec"]) == len(est["records"]) == len(est["mates"])
    for first_setter in ("pairing", "secondary"):              # the new setter refuses a mapper an earlier one has touched
        with engine.Mapper(mb.mapper_params(n, False), ref) as m:
            m.set_pairing(pp) if first_setter == "pairing" else m.set_secondary(sc)
            with pytest.raises(capi.AimError) as e:
                m.set_pairing_secondary(pp, sc)
            assert e.value.code == capi.AIM_EINVAL and "no other setter has touched" in str(e.value)


def test_mapper_equals_stages_and_truth_class_1():
    p = child.run("test_pair_secondary_gpu", "mapper_end_to_end", cuda_first=True, marker="PAIR_SECONDARY_MAPPER_OK", check=False)
    print(p.stdout[-4000:])
    assert p.returncode == 0 and "PAIR_SECONDARY_MAPPER_OK" in p.stdout, p.stdout[-3000:] + p.stderr[-6000:]


def mapper_truth_class_4():
    """Both copies inside the span: the pair is proper on the copy the chains ranked first, n_best is 2 and the read's MAPQ 0; the mate's
    pair MAPQ is 60 and its MAPQ its own; the other copy is the read's one 0x100 line. The mapper against the stages by hand as well."""
    import chain_class_model as ccm
    import mapper_batch as mb
    import pair_model as pm
    import pair_secondary_batch as pb
    import secondary_model as scm
    from aim_amd import engine
    from gpu_buffers import copy_out
    rs = ccm.CHIMERIC_SIZE
    ref, rows, rl, truth, near = pb.truth_class4()
    n = len(rl)
    pp = pb.truth4_pair_params(n, rs)
    with engine.Mapper(mb.mapper_params(n, False), ref) as m:
        m.set_pairing_secondary(pp, engine.secondary_params(MAX_SEC, records=True))
        m.submit(0, rl, rows)
        got = copy_out(m.wait(0))
    want = stages_by_hand(ref, rows, rl, pp, scm.SEC_RECORDS)
    assert mb.canon(got) == mb.canon(want)
    for k in ("pairs", "pair_mapq", "mates", "sec"):
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k
    rec, off, pairs, pq = got["records"], got["rec_offsets"], got["pairs"], got["pair_mapq"]
    for mm in range(n // 2):
        p, q = pairs[mm], pq[mm]
        a, b = rec[off[2 * mm]:off[2 * mm + 1]], rec[off[2 * mm + 1]:off[2 * mm + 2]]
        print(mm, p, q, [(int(o["sam"]["pos"]), int(o["sam"]["flags"]), int(o["mapq"])) for o in list(a) + list(b)])
        assert p["flags"] == pm.PROPER and p["n_best"] == 2 and p["second_sum"] == p["score_sum"], (mm, p)
        assert q["tied"][0] == 1 and q["pair_mapq"][0] == 0 and q["mapq"][0] == 0 and a[0]["mapq"] == 0 and q["alt_sum"][0] == p["score_sum"]
        assert q["pair_mapq"][1] == 60 and q["tied"][1] == 0 and q["mapq"][1] == q["own_mapq"][1] == b[0]["mapq"], (mm, q)
        assert len(b) == 1 and len(a) == 2 and [bool(int(o["sam"]["flags"]) & scm.SAM_SECONDARY) for o in a] == [False, True]
        starts = sorted(int(o["sam"]["pos"]) // 1 for o in a)
        assert near <= starts[0] < near + scm.REPEAT_LEN and scm.REPEAT_B <= starts[1] < scm.REPEAT_B + scm.REPEAT_LEN
        assert int(a[0]["sam"]["flags"]) & 0x2 and not int(a[1]["sam"]["flags"]) & 0x2 and int(b[0]["sam"]["flags"]) & 0x2


def test_mapper_truth_class_4():
    p = child.run("test_pair_secondary_gpu", "mapper_truth_class_4", cuda_first=True, marker="PAIR_SECONDARY_CLASS4_OK", check=False)
    print(p.stdout[-4000:])
    assert p.returncode == 0 and "PAIR_SECONDARY_CLASS4_OK" in p.stdout, p.stdout[-3000:] + p.stderr[-6000:]


def test_command_line_with_reads2_and_secondary(tmp_path):
    """python -m aim_amd.map --reads2 ... --secondary N over truth class 1: paired lines with tp:A:P / tp:A:S; every repeat read has its
    line on copy B with 0x2 and one 0x100 line on copy A with mate fields, `*` for SEQ and QUAL and TLEN 0."""
    import subprocess
    import chain_class_model as ccm
    import mapper_batch as mb
    import pair_secondary_batch as pb
    import secondary_model as scm
    k, stride, w, max_occ, band, flank, min_votes, K = ccm.CHIMERIC_ROW
    ref, rows, rl, truth = pb.truth_class1()
    n = len(rl)
    (tmp_path / "ref.fa").write_bytes(b">chr\n%s\n" % ref.tobytes())
    for x in range(2):
        with open(tmp_path / ("r%d.fq" % (x + 1)), "wb") as f:
            for m in range(n // 2):
                f.write(b"@pair%d/%d\n%s\n+\n%s\n" % (m, x + 1, rows[2 * m + x, :rl[2 * m + x]].tobytes(), b"I" * int(rl[2 * m + x])))
    cmd = [sys.executable, "-m", "aim_amd.map", "--ref", str(tmp_path / "ref.fa"), "--reads", str(tmp_path / "r1.fq"), "--reads2", str(tmp_path / "r2.fq"),
           "-o", str(tmp_path / "out.sam"), "--batch", "16", "--read-size", str(ccm.CHIMERIC_SIZE), "-k", str(k), "-w", str(w), "--max-occ", str(max_occ),
           "--band", str(band), "--flank", str(flank), "--min-votes", str(min_votes), "--max-cands", str(K), "--max-score", str(mb.max_score()),
           "--min-span", str(pb.T_MIN_SPAN), "--max-span", str(pb.T_MAX_SPAN), "--unpaired-penalty", str(pb.T_PENALTY), "--secondary", str(MAX_SEC)]
    p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "not in this version" not in p.stderr, p.stdout + p.stderr
    cols = [l.split("\t") for l in open(tmp_path / "out.sam").read().splitlines() if not l.startswith("@")]
    assert len(cols) == 3 * (n // 2)
    for m in range(n // 2):
        first, second, mate = cols[3 * m:3 * m + 3]
        assert first[0] == second[0] == mate[0] == "pair%d" % m
        assert int(first[1]) & 0x43 == 0x43 and not int(first[1]) & 0x900 and scm.in_copy(int(first[3]) - 1, scm.REPEAT_B) and int(first[4]) >= 20 and "tp:A:P" in first
        assert int(second[1]) & 0x141 == 0x141 and not int(second[1]) & 0x2 and scm.in_copy(int(second[3]) - 1, scm.REPEAT_A) and second[4] == "0" and "tp:A:S" in second
        assert second[6:11] == ["=", mate[3], "0", "*", "*"] and first[6:8] == ["=", mate[3]] and abs(int(first[8])) == pb.T_SPAN
        assert int(mate[1]) & 0x83 == 0x83 and mate[7] == first[3] and int(mate[8]) == -int(first[8]) and "tp:A:P" in mate
