"""Rule 15c on the GPU. aim_pair_estimate_device and the _est twins of rule 14c's two kernels on synthetic slot tables against the Python
models (tests/pair_estimate_model.py, tests/pair_model.py), every output byte, for each K, batch size and histogram size below, with and
without d_contig, on a small and a large grid and under the poison knobs, and the tables of K = 3 padded with empty slots to every group
width against themselves (tests/slot_padding.py); then aim_mapper_t with estimation on the shared batch
(tests/pair_est_batch.py) against the stages driven by hand, against the true fragment lengths and against plain set_pairing with the
fallback bounds; and the command line's --estimate-span."""
import functools
import math
import os
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
# (hist_size, min_samples, min_mapq, min_slack): the three histogram sizes; a floor of the spread that pushes lo below 0; no fallback left
EST_SETS = ((64, 1, 20, 16), (64, 1, 0, 100), (1024, 8, 20, 16), (8192, 8, 20, 16), (1024, 10 ** 6, 20, 16))


@functools.lru_cache(maxsize=None)
def tables(K, n, contigs):
    """Built once per shape and shared: neither side writes to them."""
    import pair_estimate_model as em
    return em.synthetic_tables(21, K, n, contigs)


def run_stages(h, K, n, t, est_set):
    """aim_pair_estimate_device -- twice in a row over the same scratch, which is prefilled with 0xA5 -- then the two _est entry points
    over uploaded tables. Every output buffer is prefilled with 0xEE and carries a guard. Returns the downloaded bytes by name."""
    import pair_model as pm
    from aim_amd import engine
    rs, rz = pm.READ_SIZE, pm.RESCUE_SIZE
    pp = engine.pair_params(pm.MIN_SPAN, pm.MAX_SPAN, 17, rescue=True, rescue_size=rz)
    ep = engine.pair_estimate_params(*est_set)
    ee = lambda nbytes: h.filled(nbytes + GUARD)
    contigs = t["contig"] is not None
    d_rl, d_reads = h.up(t["read_len"]), h.up(t["reads"], 16)
    d_seg, d_sam, d_cls, d_res_sam = h.up(t["seg"]), h.up(t["sam"]), h.up(t["cls"]), h.up(t["res_sam"])
    d_contig = h.up(t["contig"]) if contigs else None
    d_starts, d_lens = (h.up(t["starts"]), h.up(t["lens"])) if contigs else (None, None)
    nc = len(t["starts"]) if contigs else 0
    sb = engine.pair_estimate_scratch(ep.hist_size)
    d_scr, d_est = h.filled(sb + GUARD, 0xA5), ee(48)
    out = {}
    for name in ("est_first", "est"):
        engine.pair_estimate_device(pp, ep, K, rs, n, d_seg, d_sam, d_cls, d_est, d_scr, sb, d_contig=d_contig)
        out[name] = h.down(d_est, 48 + GUARD)
    out["scr_guard"] = h.down(d_scr, sb + GUARD)[sb:]
    d_req, d_tp, d_pat = ee(16 * n), ee(8 * n), ee(n * rz)
    engine.pair_rescue_rows_device_est(pp, K, rs, t["ref_len"], n, d_rl, d_reads, d_seg, d_sam, d_req, d_tp, d_pat, d_est, d_contig=d_contig, n_contigs=nc,
                                       d_contig_start=d_starts, d_contig_len=d_lens)
    out["req"], out["tpos"], out["pat"] = h.down(d_req, 16 * n + GUARD), h.down(d_tp, 8 * n + GUARD), h.down(d_pat, n * rz + GUARD)
    d_pairs = ee(32 * (n // 2))
    engine.pair_select_device_est(pp, K, rs, n, d_rl, d_seg, d_sam, d_cls, d_res_sam, CIGAR_BASE, MD_BASE, d_pairs, d_est, d_contig=d_contig)
    out["pairs"] = h.down(d_pairs, 32 * (n // 2) + GUARD)
    out["seg"], out["sam"], out["cls"] = h.down(d_seg, 8 * n * K), h.down(d_sam, 48 * n * K), h.down(d_cls, 8 * n * K)
    if contigs:
        out["contig"] = h.down(d_contig, 4 * n * K)
    out["est_after"] = h.down(d_est, 48 + GUARD)                  # the _est kernels read the estimate, they never write it
    return out


def same(name, got, want, itemsize, case):
    got, want = np.asarray(got).view(np.uint8).reshape(-1, itemsize), np.ascontiguousarray(want).view(np.uint8).reshape(-1, itemsize)
    assert got.shape == want.shape, (case, name, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        bad = np.nonzero((got != want).any(axis=1))[0]
        raise AssertionError((case, name, "rows", bad[:8].tolist(), got[bad[0]].tolist(), want[bad[0]].tolist()))


def check_against_model(K, n, contigs, est_set, out):
    """d_est byte for byte, the pad words and the guard included, and the five buffers of the _est rescue rows and select / apply against
    pair_model run with the estimated bounds. Returns the model's estimate."""
    import pair_estimate_model as em
    import pair_model as pm
    t = tables(K, n, contigs)
    pp = pm.params(17, True)
    rs, rz = pm.READ_SIZE, pm.RESCUE_SIZE
    case = (K, n, contigs, est_set)
    e = em.estimate(pp, em.EstParams(*est_set), K, rs, n, t["seg"], t["sam"], t["cls"], t["contig"])
    for name in ("est_first", "est", "est_after"):
        same(name, out[name][:48], e, 48, case)
        assert (out[name][48:] == 0xEE).all(), (case, name)
    assert (out["scr_guard"] == 0xA5).all(), case
    pe = em.params_with(pp, e)
    assert 0 <= pe.min_span <= pe.max_span and pe.max_span - pe.min_span + rs <= rz, (case, pe.min_span, pe.max_span)
    req, tpos, rows = pm.rescue_rows(pe, K, rs, t["ref_len"], n, t["read_len"], t["reads"], t["seg"], t["sam"], t["contig"], t["starts"], t["lens"])
    same("req", out["req"][:16 * n], req, 16, case)
    same("tpos", out["tpos"][:8 * n], tpos, 8, case)
    pat = np.full(n * rz + GUARD, 0xEE, dtype=np.uint8)
    for b, row in rows.items():
        pat[b * rz:b * rz + rs] = row
    same("pat", out["pat"], pat, 1, case)
    assert (out["req"][16 * n:] == 0xEE).all() and (out["tpos"][8 * n:] == 0xEE).all(), case
    pairs, seg, sam, cls, contig = pm.select(pe, K, rs, n, t["read_len"], t["seg"], t["sam"], t["cls"], t["contig"], t["res_sam"], CIGAR_BASE, MD_BASE)
    same("pairs", out["pairs"][:32 * (n // 2)], pairs, 32, case)
    assert (out["pairs"][32 * (n // 2):] == 0xEE).all(), case
    same("seg", out["seg"], seg, 8, case)
    same("sam", out["sam"], sam, 48, case)
    same("cls", out["cls"], cls, 8, case)
    if contigs:
        same("contig", out["contig"], contig, 4, case)
    return e[0]


@pytest.mark.parametrize("contigs", (False, True), ids=("one-seq", "contigs"))
@pytest.mark.parametrize("K", KS)
def test_stages_equal_model(K, contigs):
    import pair_estimate_model as em
    import pair_model as pm
    from aim_amd import capi, engine
    seen = set()
    with Hip() as h:
        for n in N_READS:
            for est_set in EST_SETS:
                e = check_against_model(K, n, contigs, est_set, run_stages(h, K, n, tables(K, n, contigs), est_set))
                h.free()
                f = int(e["flags"])
                seen |= {"fallback"} if f & em.FALLBACK else set()
                seen |= {"clamped"} if f & em.CLAMPED else set()
                seen |= {"floored"} if f & em.FLOORED else set()
                seen |= {"none"} if f == 0 else set()
                seen |= {"beyond"} if e["n_beyond"] else set()
                seen |= {"empty"} if not e["n_samples"] else set()
                seen |= {"moved"} if not f & em.FALLBACK and (int(e["min_span"]), int(e["max_span"])) != (pm.MIN_SPAN, pm.MAX_SPAN) else set()
        assert seen == {"fallback", "clamped", "floored", "none", "beyond", "empty", "moved"}, (K, contigs, seen)
        # an empty batch writes the fallback estimate with every count zero, and the twins enqueue nothing
        pp = engine.pair_params(pm.MIN_SPAN, pm.MAX_SPAN, rescue_size=pm.RESCUE_SIZE)
        ep = engine.pair_estimate_params(64, 1, 0, 0)
        d_est = h.filled(48 + GUARD)
        engine.pair_estimate_device(pp, ep, K, pm.READ_SIZE, 0, None, None, None, d_est, None, 0)
        got = h.down(d_est, 48 + GUARD)
        want = np.array([(pm.MIN_SPAN, pm.MAX_SPAN, 0, 0, 0, 0, 0, em.FALLBACK, (0, 0))], dtype=capi.PAIR_ESTIMATE_DTYPE)
        assert got[:48].tobytes() == want.tobytes() and (got[48:] == 0xEE).all()
        engine.pair_estimate_device(pp, ep, K, pm.READ_SIZE, 0, None, None, None, None, None, 0)
        engine.pair_rescue_rows_device_est(pp, K, pm.READ_SIZE, 1000, 0, None, None, None, None, None, None, None, None)
        engine.pair_select_device_est(pp, K, pm.READ_SIZE, 0, None, None, None, None, None, 0, 0, None, None)


KNOB_CASES = ((4, 4100, True, EST_SETS[2]), (16, 130, False, EST_SETS[3]), (1, 4100, False, EST_SETS[0]), (4, 4100, False, EST_SETS[1]),
              (6, 4100, True, EST_SETS[2]), (9, 130, False, EST_SETS[3]))      # the last two: 8 lanes per read pair, and 16 that K does not fill


def knob_batch():
    out = {}
    with Hip() as h:
        for i, (K, n, contigs, est_set) in enumerate(KNOB_CASES):
            for k, v in run_stages(h, K, n, tables(K, n, contigs), est_set).items():
                out["%s_%d" % (k, i)] = v
            h.free()
    return out


@pytest.mark.parametrize("env", [{"AIM_CHIP_CUS": "1", "AIM_DEBUG_POISON_SCRATCH": "165", "AIM_DEBUG_POISON_OPS": "77", "AIM_DEBUG_POISON_LDS": "90"},
                                 {"AIM_CHIP_CUS": "256", "AIM_DEBUG_POISON_LDS": "255"}], ids=["cus1-poison", "cus256-lds255"])
def test_grid_and_poison_identical(tmp_path, env):
    """The same bytes -- the model's -- at AIM_CHIP_CUS 1 (8 workgroups walk the 33 blocks of read pairs) and 256 (33 workgroups, 9 for the histogram), and under the three
    AIM_DEBUG_POISON_* knobs; the scratch held 0xA5 and the estimate ran twice on it."""
    f = str(tmp_path / "k.npz")
    p = child.run("test_pair_estimate_gpu", "knob_batch", npz=f, env=dict(env, AIM_PLAN_DEBUG="1"))
    grid, hgrid = (8, 8) if env["AIM_CHIP_CUS"] == "1" else (33, 9)      # (the histogram kernel's workgroups walk four blocks at least)
    assert "[aim plan] pair_span_hist_kernel grid=%d block=256 lanes=4 reads=4100 K=4 hist_size=1024 lds=4100; pair_span_bounds_kernel grid=1 block=256" % hgrid in p.stderr, p.stderr
    assert "[aim plan] pair_rescue_rows_est_kernel grid=%d block=256 lanes=4 reads=4100 K=4 rescue_size=512" % grid in p.stderr, p.stderr
    assert "[aim plan] pair_select_est_kernel grid=%d block=256 lanes=4 reads=4100 K=4 rescue=1" % grid in p.stderr, p.stderr
    assert "pair_span_hist_kernel grid=2 block=256 lanes=16 reads=130 K=16 hist_size=8192 lds=32772" in p.stderr, p.stderr
    # the 8-lane path ran, and a 16-lane group of 9: the launchers' own rule, ceil(read pairs / (256 / lanes)) blocks under the resident
    # grid of 8 workgroups per compute unit, a workgroup of the histogram kernel walking four blocks at least
    resident = 8 * int(env["AIM_CHIP_CUS"])
    for lanes, n, K, hist_size in ((8, 4100, 6, 1024), (16, 130, 9, 8192)):
        blocks = -(-(n // 2) // (256 // lanes))
        g, hg = min(resident, blocks), min(resident, -(-blocks // 4))
        assert "[aim plan] pair_span_hist_kernel grid=%d block=256 lanes=%d reads=%d K=%d hist_size=%d lds=%d; pair_span_bounds_kernel grid=1 block=256" % (
            hg, lanes, n, K, hist_size, 4 * (hist_size + 1)) in p.stderr, p.stderr
        assert "[aim plan] pair_rescue_rows_est_kernel grid=%d block=256 lanes=%d reads=%d K=%d rescue_size=512" % (g, lanes, n, K) in p.stderr, p.stderr
        assert "[aim plan] pair_select_est_kernel grid=%d block=256 lanes=%d reads=%d K=%d rescue=1" % (g, lanes, n, K) in p.stderr, p.stderr
    out = np.load(f)
    for i, (K, n, contigs, est_set) in enumerate(KNOB_CASES):
        check_against_model(K, n, contigs, est_set, {k[:-2]: out[k] for k in out.files if k.endswith("_%d" % i)})


@pytest.mark.parametrize("contigs", (False, True), ids=("one-seq", "contigs"))
def test_empty_slots_change_nothing(contigs):
    """tests/slot_padding.py on the device: the tables of K = 3 with every read padded to 4, 8 and 16 slots -- the same read pairs in
    groups of 4, 8 and 16 lanes -- give the 48 bytes of the estimate of K = 3 under every EST_SETS row, and behind it every byte of the
    _est twins' outputs, slot numbers renamed. Those of K = 3 are the models'."""
    import pair_model as pm
    import slot_padding as sp
    K, n = 3, N_READS[1]
    t = tables(K, n, contigs)
    samples = 0
    with Hip() as h:
        for est_set in EST_SETS:
            a = run_stages(h, K, n, t, est_set)
            h.free()
            samples += int(check_against_model(K, n, contigs, est_set, a)["n_samples"])
            for K2 in (4, 8, 16):
                case = (K, K2, n, contigs, est_set)
                t2 = sp.pad_tables(t, K, K2, n)
                b = run_stages(h, K2, n, t2, est_set)
                h.free()
                for k in ("est_first", "est", "est_after", "scr_guard", "req", "tpos", "pat"):
                    same(k, b[k], a[k], 1, case)
                npairs = 32 * (n // 2)
                same("pairs", b["pairs"][:npairs], sp.pairs_renamed(a["pairs"][:npairs].view(pm.PAIR_DTYPE), K, K2), 32, case)
                assert (b["pairs"][npairs:] == 0xEE).all(), case
                for k, dt in (("seg", pm.SEG_DTYPE), ("sam", pm.SAM_DTYPE), ("cls", pm.CLASS_DTYPE), ("contig", np.dtype("<u4"))):
                    if k in a:
                        own, rest = sp.unpad(b[k].view(dt), K, K2, n)
                        same(k, own, a[k], dt.itemsize, case)
                        same(k + " of the empty slots", rest, sp.unpad(t2[k], K, K2, n)[1], dt.itemsize, case)
    assert samples


# ---- the mapper with estimation -------------------------------------------------------------------------------------------------------
def map_batch(rl, rows, estimate=True, bounds=None):
    """Reads through a mapper with pairing -- estimated, or plain set_pairing with the bounds given (default: the fallback's): a detached result."""
    import pair_est_batch as eb
    from aim_amd import engine
    n = max(len(rl), 2)
    with engine.Mapper(eb.mapper_params(n), eb.reference()) as m:
        m.set_pairing(eb.pair_params(n, *(bounds or ())), estimate=eb.est_params() if estimate else None)
        m.submit(0, rl, rows)
        return copy_out(m.wait(0))


def hand_path(rl, rows):
    """The stages one by one on torch buffers, one synchronize per stage: the split path to sam_device_split, aim_pair_estimate_device
    (checked against the model on the way), the _est rescue rows through their kernel (checked against pair_model under the estimated
    bounds), aim_align_device_ref and aim_sam_device over them behind the main CIGAR / MD regions, then the models of select / apply, of
    the records and of the mate fields over the downloaded rows: a dict shaped like a mapper result."""
    import torch
    import map_records_model as mm
    import pair_est_batch as eb
    import pair_estimate_model as em
    import pair_model as pm
    from aim_amd import capi, engine
    K, rs, rz, flank, n = eb.K, eb.READ_SIZE, eb.RESCUE_SIZE, eb.FLANK, len(rl)
    ref = eb.reference()
    dev = hs.DEV
    params = hs.wfa_params(eb.MAX_SCORE, rs, eb.X, eb.O, eb.E, 2 * flank)
    rparams = hs.wfa_params(eb.MAX_SCORE, rz, eb.X, eb.O, eb.E, rz)
    rows_n = n * K
    d_ref = put(ref, dev, 64)
    out = hs.segment_rows(eb.seed_params(), ref, rl, rows)
    ccap, mcap, rccap, rmcap = rows_n * 64, rows_n * 256, n * 64, n * 256
    d_cigar, d_md = zeros((ccap + rccap) * 4, dev), zeros(mcap + rmcap, dev)
    d_res, d_ops = hs.align_rows(params, rows_n, out["d_seg_req"], out["d_seg_patterns"], out["d_seg_text_pos"], d_ref, len(ref))
    last = hs.sam_rows(params, rows_n, out["d_seg_req"], out["d_seg_text_pos"], d_res, d_ops, d_ref, len(ref), (ccap, mcap), split_seg=out["d_seg"],
                       into=(d_cigar, d_md, 0, 0))
    d_sam, sam = last["d_sam"], last["sam"]
    seg = out["d_seg"].cpu().numpy().view(capi.SEGMENT_DTYPE)[:rows_n].copy()
    pp_c, ep_c = eb.pair_params(n), eb.est_params()
    pp = pm.Params(eb.MIN_SPAN, eb.MAX_SPAN, eb.UNPAIRED_PENALTY, pm.RESCUE, rz)
    sb = engine.pair_estimate_scratch(eb.HIST_SIZE)
    d_est, d_scr = zeros(48, dev), torch.full((sb,), 0xA5, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    engine.pair_estimate_device(pp_c, ep_c, K, rs, n, out["d_seg"].data_ptr(), d_sam.data_ptr(), out["d_class"].data_ptr(), d_est.data_ptr(), d_scr.data_ptr(), sb)
    torch.cuda.synchronize()
    est = d_est.cpu().numpy()[:48].view(capi.PAIR_ESTIMATE_DTYPE).copy()
    want_est = em.estimate(pp, em.EstParams(eb.HIST_SIZE, eb.MIN_SAMPLES, eb.MIN_MAPQ, eb.MIN_SLACK), K, rs, n, seg, sam, out["class"])
    assert est.tobytes() == want_est.tobytes(), (est, want_est)
    pe = em.params_with(pp, est)
    d_rreq, d_rtp, d_rpat = zeros(16 * n, dev), zeros(8 * n, dev), zeros(n * rz + 64, dev)
    engine.pair_rescue_rows_device_est(pp_c, K, rs, len(ref), n, out["d_read_len"].data_ptr(), out["d_reads"].data_ptr(), out["d_seg"].data_ptr(), d_sam.data_ptr(),
                                       d_rreq.data_ptr(), d_rtp.data_ptr(), d_rpat.data_ptr(), d_est.data_ptr())
    torch.cuda.synchronize()
    want_req, want_tp, _ = pm.rescue_rows(pe, K, rs, len(ref), n, rl, rows, seg, sam)
    assert d_rreq.cpu().numpy()[:16 * n].tobytes() == want_req.tobytes() and d_rtp.cpu().numpy()[:8 * n].tobytes() == want_tp.tobytes()
    d_rres, d_rops = hs.align_rows(rparams, n, d_rreq, d_rpat, d_rtp, d_ref, len(ref))
    last = hs.sam_rows(rparams, n, d_rreq, d_rtp, d_rres, d_rops, d_ref, len(ref), (rccap, rmcap), into=(d_cigar, d_md, ccap, mcap))
    res_sam, needed = last["sam"], last["cur"].tolist()
    pairs, seg2, sam2, cls2, _ = pm.select(pe, K, rs, n, rl, seg, sam, out["class"], None, res_sam, ccap, mcap)
    off, rec = mm.map_records(K, n, seg2, sam2, cls2)
    rec2, mates = pm.mates(K, n, pairs, seg2, sam2, None, None, off, rec)
    return {"records": rec2, "rec_offsets": off, "cigar": last["cigar"], "md": last["md"], "mates": mates, "pairs": pairs,
            "rescue_cigar_needed": needed[0], "rescue_md_needed": needed[1], "pair_estimate": engine.estimate_dict(est[0])}


def same_result(got, want, what):
    import mapper_batch as mb
    g, w = mb.canon(got), mb.canon(want)
    assert g[1] == w[1], (what, "rec_offsets")
    assert g[0] == w[0], (what, "records", np.nonzero(np.frombuffer(g[0], dtype=np.uint8) != np.frombuffer(w[0], dtype=np.uint8))[0][:8] // 64)
    assert g[2] == w[2] and g[3] == w[3], (what, "CIGAR words or MD bytes")
    assert got["mates"].tobytes() == want["mates"].tobytes() and got["pairs"].tobytes() == want["pairs"].tobytes(), (what, "mates or pairs")
    assert (got["rescue_cigar_needed"], got["rescue_md_needed"]) == (want["rescue_cigar_needed"], want["rescue_md_needed"]), what


def primary(out, r):
    g = range(int(out["rec_offsets"][r]), int(out["rec_offsets"][r + 1]))
    p = [i for i in g if not int(out["records"]["sam"]["flags"][i]) & 0x800]
    assert len(p) == 1, (r, p)
    return p[0]


def at_interval(out, i, tm):
    import pair_est_batch as eb
    import pair_model as pm
    s = out["records"]["sam"][i]
    return not s["flags"] & pm.SAM_UNMAPPED and bool(s["flags"] & pm.SAM_REVERSE) == bool(tm[2]) and int(s["pos"]) == tm[0] and int(s["ref_span"]) == eb.L


def end_to_end():
    """The shared batch through aim_mapper_t with estimation against hand_path -- records in canon form, rec_offsets, mates, pairs and the
    estimate -- against the true quartiles and class by class against where the mates were cut from; the same batch through plain
    set_pairing with the fallback bounds, which keeps class w on the wrong copy; a batch of classes d, r and q alone, which takes the
    fallback and gives plain set_pairing's bytes."""
    import pair_est_batch as eb
    import pair_estimate_model as em
    import pair_model as pm
    b = eb.batch()
    rl, rows, truth = b["read_len"], b["rows"], b["truth"]
    got = map_batch(rl, rows)
    want = hand_path(rl, rows)
    same_result(got, want, "estimated")
    e = got["pair_estimate"]
    assert e == want["pair_estimate"], (e, want["pair_estimate"])
    lens = sorted(t["span"] for t in truth if t["cls"] == "c")
    assert [e["p25"], e["p50"], e["p75"]] == [lens[math.ceil(q * 256 / 4) - 1] for q in (1, 2, 3)] and e["n_samples"] == 256 and e["n_beyond"] == 8 and e["flags"] == 0
    assert e["max_span"] < 600 and e["min_span"] == e["p25"] - max(3 * (e["p75"] - e["p25"]), eb.MIN_SLACK) and e["max_span"] == e["p75"] + e["p25"] - e["min_span"]
    plain = map_batch(rl, rows, estimate=False)
    assert "pair_estimate" not in plain
    rec, mates, pairs = got["records"], got["mates"], got["pairs"]
    seen = {c: 0 for c, _ in eb.COUNTS}
    for m, t in enumerate(truth):
        c, F = t["cls"], t["span"]
        i0, i1 = primary(got, 2 * m), primary(got, 2 * m + 1)
        f = int(pairs["flags"][m])
        fl0, fl1 = int(rec["sam"]["flags"][i0]), int(rec["sam"]["flags"][i1])
        if c == "c":                                               # proper, TLEN plus or minus the fragment length
            assert f == pm.PROPER and at_interval(got, i0, t["mates"][0]) and at_interval(got, i1, t["mates"][1]), (m, f)
            assert int(pairs["span"][m]) == F and sorted((int(mates["tlen"][i0]), int(mates["tlen"][i1]))) == [-F, F] and fl0 & 0x2 and fl1 & 0x2
        elif c == "w":                                             # the repeat mate comes back rescued onto its true interval, 0x2 set
            x = t["repeat"]
            ix, iu = (i0, i1) if x == 0 else (i1, i0)
            assert f == pm.PROPER | pm.TRIED_A | pm.TRIED_B | (pm.RESCUED_B if x else pm.RESCUED_A), (m, f)
            assert at_interval(got, ix, t["mates"][x]) and at_interval(got, iu, t["mates"][1 - x]) and fl0 & 0x2 and fl1 & 0x2
            assert int(pairs["span"][m]) == F and sorted((int(mates["tlen"][i0]), int(mates["tlen"][i1]))) == [-F, F]
            # ... while plain set_pairing with 0..800 returns a proper pair on the wrong copy, 300 bases further: the point of the feature
            j0, j1 = primary(plain, 2 * m), primary(plain, 2 * m + 1)
            jx = j0 if x == 0 else j1
            wrong = (t["mates"][x][0] - 300, t["mates"][x][1] - 300, t["mates"][x][2])
            assert int(plain["pairs"]["flags"][m]) == pm.PROPER and int(plain["pairs"]["span"][m]) == F + 300 and at_interval(plain, jx, wrong)
            assert int(plain["records"]["sam"]["flags"][j0]) & 0x2 and int(plain["records"]["sam"]["flags"][j1]) & 0x2
        elif c == "s":                                             # mate 2 has no chain: the rescue places it, ten substitutions
            assert f == pm.PROPER | pm.TRIED_B | pm.RESCUED_B and at_interval(got, i1, t["mates"][1]) and int(rec["sam"]["score"][i1]) == 10 * eb.X, (m, f)
            assert int(pairs["span"][m]) == F
        elif c in "dr":                                            # never proper
            assert not f & pm.PROPER and not (fl0 | fl1) & 0x2 and mates["tlen"][i0] == 0 and mates["tlen"][i1] == 0, (m, c, f)
        elif c == "l":
            assert not f & pm.PROPER and at_interval(got, i0, t["mates"][0]) and at_interval(got, i1, t["mates"][1])
        seen[c] += 1
    assert seen == dict(eb.COUNTS)
    print("estimate", e, "proper", int((pairs["flags"] & 1).sum()), "of", len(pairs), "plain proper", int((plain["pairs"]["flags"] & 1).sum()))
    # classes d, r and q alone: fewer samples than min_samples, so the fallback -- and plain set_pairing's bytes
    few_rl, few_rows = eb.subset(eb.pairs_of("drq"))
    few, few_plain = map_batch(few_rl, few_rows), map_batch(few_rl, few_rows, estimate=False)
    fe = few.pop("pair_estimate")
    assert fe["flags"] == em.FALLBACK and (fe["min_span"], fe["max_span"]) == (eb.MIN_SPAN, eb.MAX_SPAN) and fe["n_samples"] < eb.MIN_SAMPLES, fe
    same_result(few, few_plain, "fallback")


def test_mapper_with_estimation_equals_the_stages_by_hand_and_the_truth():
    p = child.run("test_pair_estimate_gpu", "end_to_end", cuda_first=True, marker="PAIR_ESTIMATE_END_TO_END_OK", check=False)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "PAIR_ESTIMATE_END_TO_END_OK" in p.stdout, p.stdout + p.stderr


def canon_est(out):
    import mapper_batch as mb
    e = out.get("pair_estimate")
    return mb.canon(out) + (out["mates"].tobytes(), out["pairs"].tobytes(), out["rescue_cigar_needed"], out["rescue_md_needed"], tuple(sorted(e.items())) if e else None)


def test_two_slots_reuse_empty_batch_and_state():
    """Two slots in flight, a reused slot (the longer batch first), an empty batch, the state rules of aim_mapper_pair_estimate, ep's
    refusals behind aim_mapper_set_pairing's, and mappers without estimation: AIM_ESTATE, and the bytes they always gave."""
    import ctypes as C
    import pair_est_batch as eb
    import pair_estimate_model as em
    from aim_amd import capi, engine
    A_rl, A_rows = eb.subset(eb.pairs_of("c")[:40] + eb.pairs_of("w"))
    B_rl, B_rows = eb.subset(eb.pairs_of("c")[100:140] + eb.pairs_of("sdl"))
    C_rl, C_rows = eb.subset(eb.pairs_of("qr"))
    alone = {k: canon_est(map_batch(rl, rows)) for k, (rl, rows) in (("A", (A_rl, A_rows)), ("B", (B_rl, B_rows)), ("C", (C_rl, C_rows)))}
    assert len({alone["A"][-1], alone["B"][-1], alone["C"][-1]}) == 3 and dict(alone["C"][-1])["flags"] == em.FALLBACK and dict(alone["A"][-1])["flags"] == 0
    n = max(len(A_rl), len(B_rl))
    with engine.Mapper(eb.mapper_params(n, slots=2), eb.reference()) as m:
        with pytest.raises(capi.AimError) as x:
            m.pair_estimate(0)
        assert x.value.code == capi.AIM_ESTATE and "aim_mapper_set_pairing_estimated was not called" in str(x.value)
        for ep, text in ((engine.pair_estimate_params(hist_size=100), "hist_size 100 must be a multiple of 64"), (engine.pair_estimate_params(min_samples=0), "min_samples must be >= 1"),
                         (engine.pair_estimate_params(min_mapq=61), "min_mapq 61 is outside 0..60")):
            with pytest.raises(capi.AimError) as x:
                m.set_pairing(eb.pair_params(n), estimate=ep)
            assert x.value.code == capi.AIM_EINVAL and "aim_mapper_set_pairing_estimated: " + text in str(x.value)
        bad = eb.pair_params(n)
        bad.options = 2
        with pytest.raises(capi.AimError) as x:                    # pp's refusals come first
            m.set_pairing(bad, estimate=engine.pair_estimate_params(hist_size=100))
        assert "aim_mapper_set_pairing_estimated: unknown options 0x2" in str(x.value)
        assert m.lib.aim_mapper_set_pairing_estimated(m.handle, C.byref(eb.pair_params(n)), None) == capi.AIM_EINVAL
        m.submit(0, A_rl, A_rows)
        with pytest.raises(capi.AimError) as x:                    # legal only while no slot is in flight
            m.set_pairing(eb.pair_params(n), estimate=eb.est_params())
        assert x.value.code == capi.AIM_ESTATE and "slot 0 is in flight" in str(x.value)
        m.wait(0)
        before = engine.mapper_pairing_device_bytes(eb.mapper_params(n, slots=2), eb.pair_params(n))
        m.set_pairing(eb.pair_params(n), estimate=eb.est_params())
        assert engine.mapper_pairing_device_bytes(eb.mapper_params(n, slots=2), eb.pair_params(n)) == before
        with pytest.raises(capi.AimError) as x:
            m.set_pairing(eb.pair_params(n), estimate=eb.est_params())
        assert x.value.code == capi.AIM_ESTATE and "already set" in str(x.value)
        with pytest.raises(capi.AimError) as x:                    # before the first wait
            m.pair_estimate(0)
        assert x.value.code == capi.AIM_ESTATE
        m.submit(0, A_rl, A_rows)
        with pytest.raises(capi.AimError) as x:                    # while the slot is in flight
            m.pair_estimate(0)
        assert x.value.code == capi.AIM_ESTATE and "slot 0 has no batch waited for" in str(x.value)
        m.submit(1, B_rl, B_rows)
        assert canon_est(m.wait(0)) == alone["A"] and canon_est(m.wait(1)) == alone["B"]
        assert tuple(sorted(m.pair_estimate(0).items())) == alone["A"][-1] and tuple(sorted(m.pair_estimate(1).items())) == alone["B"][-1]
        for k, (rl, rows) in (("B", (B_rl, B_rows)), ("A", (A_rl, A_rows)), ("C", (C_rl, C_rows))):    # a slot's result does not depend on what ran before it
            m.submit(1, rl, rows)
            assert canon_est(m.wait(1)) == alone[k]
        m.submit(0, A_rl[:0], A_rows[:0])
        out = m.wait(0)
        assert out["n_reads"] == 0 and len(out["records"]) == 0 and len(out["pairs"]) == 0
        assert out["pair_estimate"] == dict(min_span=eb.MIN_SPAN, max_span=eb.MAX_SPAN, n_samples=0, n_beyond=0, p25=0, p50=0, p75=0, flags=em.FALLBACK)
    with engine.Mapper(eb.mapper_params(len(A_rl)), eb.reference()) as m:      # plain pairing: no estimate to ask for
        m.set_pairing(eb.pair_params(len(A_rl)))
        m.submit(0, A_rl, A_rows)
        out = m.wait(0)
        assert "pair_estimate" not in out
        with pytest.raises(capi.AimError) as x:
            m.pair_estimate(0)
        assert x.value.code == capi.AIM_ESTATE and "aim_mapper_set_pairing_estimated was not called" in str(x.value)


def test_command_line_with_estimate_span(tmp_path):
    """python -m aim_amd.map --reads2 --estimate-span over a cut of the batch: the lines samout writes for the engine's own result, and one
    stderr line per batch that carries the estimate."""
    import pair_est_batch as eb
    from aim_amd import samout
    rl, rows = eb.subset(eb.pairs_of("c")[:48] + eb.pairs_of("w")[:8] + eb.pairs_of("s")[:4] + eb.pairs_of("r")[:4])
    n = len(rl)
    (tmp_path / "ref.fa").write_bytes(b">c0\n%s\n" % eb.reference().tobytes())
    for x in range(2):
        with open(tmp_path / ("r%d.fq" % (x + 1)), "wb") as f:
            for m in range(n // 2):
                f.write(b"@pair%d/%d\n%s\n+\n%s\n" % (m, x + 1, rows[2 * m + x, :rl[2 * m + x]].tobytes(), b"I" * int(rl[2 * m + x])))
    cmd = [sys.executable, "-m", "aim_amd.map", "--ref", str(tmp_path / "ref.fa"), "--reads", str(tmp_path / "r1.fq"), "--reads2", str(tmp_path / "r2.fq"),
           "-o", str(tmp_path / "out.sam"), "--batch", str(n), "--read-size", str(eb.READ_SIZE), "-k", str(eb.K_MER), "-w", str(eb.W), "--max-occ", str(eb.MAX_OCC),
           "--band", str(eb.BAND), "--flank", str(eb.FLANK), "--min-votes", str(eb.MIN_VOTES), "--max-cands", str(eb.K), "--max-score", str(eb.MAX_SCORE),
           "--min-span", str(eb.MIN_SPAN), "--max-span", str(eb.MAX_SPAN), "--unpaired-penalty", str(eb.UNPAIRED_PENALTY), "--rescue-size", str(eb.RESCUE_SIZE),
           "--estimate-span", "--est-hist-size", str(eb.HIST_SIZE), "--est-min-samples", str(eb.MIN_SAMPLES), "--est-min-mapq", str(eb.MIN_MAPQ),
           "--est-min-slack", str(eb.MIN_SLACK)]
    p = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    body = [l for l in open(tmp_path / "out.sam").read().splitlines() if not l.startswith("@")]
    got = map_batch(rl, rows)
    e = got["pair_estimate"]
    want = samout.record_lines(got, ["pair%d" % (r // 2) for r in range(n)], rows, rl, "c0", ["I" * int(x) for x in rl])
    assert body == want and len(body) == len(got["records"])
    line = "aim_amd.map: span estimate p25=%d p50=%d p75=%d bounds=%d..%d samples=%d beyond=%d flags=0x%x" % (
        e["p25"], e["p50"], e["p75"], e["min_span"], e["max_span"], e["n_samples"], e["n_beyond"], e["flags"])
    assert p.stderr.count("span estimate") == 1 and line in p.stderr, p.stderr
    assert e["n_samples"] == 48 and e["flags"] == 0 and e["max_span"] < 600
    assert sum(1 for l in body if int(l.split("\t")[1]) & 0x2) == 2 * (48 + 8 + 4)
