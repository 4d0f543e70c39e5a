"""Segment extension on the GPU. The contract is byte equality with rule 11c as tests/extend_model.py writes it down: the four in/out
buffers and d_ext (prefilled with 0xEE, 64 guard bytes behind the pattern rows) on the directed batch for every K, batch size, row size,
penalty set, band and max_ext below, the identity on the single-primary short reads, the same bytes on a small grid and under the
poison knobs, and the whole path chain -> classify -> split -> extend -> align -> SAM records on the chimeric reads against the same
path without the extension call."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import child  # noqa: E402
import hand_stages as hs  # noqa: E402
from extend_model import inner_gaps  # noqa: E402
from gpu_buffers import Hip, cached, put  # noqa: E402
from pipeline_batches import FULL, READ_SIZE, chimeric_expected, reference, short_reads  # noqa: E402

OUT = ("seg_req", "seg_text_pos", "seg_patterns", "seg", "ext")
# (K, read_size, penalty set of extend_model.PENALTIES, band, max_ext, max_cost, batch sizes): 1, 65 and 1027 reads are below, across and
# beyond a wavefront's 64 items and, at K = 4, a workgroup of the apply kernel; the largest batch runs at max_ext 32
CASES = [(4, 104, 0, 31, 64, 400, (1, 65)), (1, 104, 1, 31, 8, 400, (1, 65)), (16, 104, 2, 1, 64, 400, (65,)), (4, 1024, 0, 31, 1024, 4095, (65,)),
         (16, 1024, 1, 31, 64, 70, (65,)), (1, 1024, 2, 15, 64, 400, (65,)), (4, 104, 0, 31, 32, 400, (1027,)), (16, 1024, 2, 31, 32, 400, (1027,))]


def case_params(case):
    import extend_model as em
    K, rs, pen, band, max_ext, max_cost, ns = case
    a, x, o, e, Z = em.PENALTIES[pen]
    return em.Params(a, x, o, e, Z, max_cost, band, max_ext)


def directed(case):
    """(the reference, the directed batch of the case's largest size, the model's outputs for it)."""
    import extend_model as em

    def make():
        K, rs = case[0], case[1]
        ref = cached("directed ref", em.directed_reference)
        d = em.directed(1, max(case[6]), K, rs, ref)
        (req, tp, pat, seg), ext = em.directed_expected(case_params(case), d, K, rs, ref)
        return ref, d, (req, tp, pat, seg, ext)
    return cached(("directed",) + tuple(case[:6]) + (max(case[6]),), make)


def run_extend(h, p, K, read_size, ref, read_len, reads, seg_req, seg_tp, seg_pat, seg):
    """aim_extend_segments_device over uploaded arrays, d_ext prefilled with 0xEE and 64 guard bytes of 0xEE behind the pattern rows:
    (requests, text_pos, patterns, segments, aim_extend_t)."""
    from aim_amd import capi, engine
    n = len(read_len)
    slots = n * K
    ep = engine.extend_params(p.match, p.mismatch, p.gap_o, p.gap_e, p.xdrop, p.max_cost, p.band, p.max_ext)
    d_req, d_tp, d_seg = h.up(seg_req), h.up(seg_tp), h.up(seg)
    d_pat = h.up(np.concatenate([np.ascontiguousarray(seg_pat).reshape(-1), np.full(64, 0xEE, dtype=np.uint8)]))
    d_ext = h.filled(slots * 24)
    engine.extend_segments_device(ep, K, read_size, len(ref), n, h.up(np.ascontiguousarray(read_len, dtype=np.int32)), h.up(reads, 64), h.up(ref, 64),
                                  d_req, d_tp, d_pat, d_seg, d_ext)
    pat = h.down(d_pat, slots * read_size + 64)
    assert (pat[slots * read_size:] == 0xEE).all(), "written past the pattern rows"
    return (h.down(d_req, slots * 16).view(capi.REQUEST_DTYPE), h.down(d_tp, slots * 8).view(np.uint64), pat[:slots * read_size].reshape(slots, read_size),
            h.down(d_seg, slots * 8).view(capi.SEGMENT_DTYPE), h.down(d_ext, slots * 24).view(capi.EXTEND_DTYPE))


def same(got, want, n_slots=None):
    for name, g, w in zip(OUT, got, want):
        w = w if n_slots is None else w[:n_slots]
        if g.tobytes() != w.tobytes():
            bad = np.nonzero((g.reshape(len(w), -1).view(np.uint8) != w.reshape(len(w), -1).view(np.uint8)).any(axis=1))[0]
            raise AssertionError((name, "slots", bad[:8].tolist(), g[bad[0]], w[bad[0]]))


def run_directed(h, case, n):
    import extend_model as em
    K, rs = case[0], case[1]
    ref, d, want = directed(case)
    dd = em.directed_prefix(d, n, K)
    return run_extend(h, case_params(case), K, rs, ref, dd["read_len"], dd["reads"], dd["seg_req"], dd["seg_tp"], dd["seg_pat"], dd["seg"])


@pytest.mark.parametrize("case", CASES, ids=lambda c: "K%d-rs%d-pen%d-band%d-ext%d-cost%d" % tuple(c[:6]))
def test_directed_batch_equals_model(case):
    K = case[0]
    ref, d, want = directed(case)
    ext = want[4]
    if max(case[6]) >= 65:
        assert (ext["dq"] != 0).any() and (ext["stop"] != 0).any() and ((ext["dq"] == 0).all(axis=1) & (want[3]["flags"] != 0)).any()
    if case[5] < 100:
        assert (ext["stop"] == case[5]).any()                       # a stop by max_cost
    with Hip() as h:
        for n in case[6]:
            same(run_directed(h, case, n), want, n * K)
            h.free()


def test_single_primary_identity():
    """The short reads through the device chain, classification and split: every read with a single primary keeps every byte of all
    four buffers and gets a zero aim_extend_t; the whole output equals the model."""
    import chain_class_model as ccm
    import extend_model as em
    rows, rl = short_reads()[:2]
    case = FULL[0]
    K = case[7]
    ref = reference()
    (req, tpos, seeds, chains, cls), split = hs.chain_classify_split(case, rows, rl, READ_SIZE)
    p = em.Params(1, 3, 4, 1, 20, 400, 31, 64)
    want, want_ext = em.extend_segments(p, K, READ_SIZE, len(ref), rl, rows, ref, *split)
    with Hip() as h:
        got = run_extend(h, p, K, READ_SIZE, ref, rl, rows, *split)
    same(got, want + (want_ext,))
    prim = (cls["flags"].reshape(-1, K) & ccm.PRIMARY) != 0
    sole = np.nonzero(prim.sum(axis=1) == 1)[0]
    assert len(sole) >= 150
    for r in sole:
        sl = slice(r * K, (r + 1) * K)
        for g, s in zip(got[:4], split):
            assert g[sl].tobytes() == s[sl].tobytes(), r
        assert got[4][sl].tobytes() == bytes(24 * K), r


KNOB_CASES = (CASES[6], CASES[4])


def knob_batch():
    out = {}
    with Hip() as h:
        for i, case in enumerate(KNOB_CASES):
            for name, arr in zip(OUT, run_directed(h, case, max(case[6]))):
                out["%s_%d" % (name, i)] = arr.view(np.uint8)
            h.free()
    return out


@pytest.mark.parametrize("env", [{"AIM_CHIP_CUS": "1", "AIM_DEBUG_POISON_SCRATCH": "165", "AIM_DEBUG_POISON_OPS": "77", "AIM_DEBUG_POISON_LDS": "90"},
                                 {"AIM_CHIP_CUS": "256", "AIM_DEBUG_POISON_LDS": "255"}], ids=["cus1-poison", "cus256-lds255"])
def test_grid_and_poison_identical(tmp_path, env):
    """The same bytes -- the model's -- at AIM_CHIP_CUS 1 (32 wavefronts walk the 129 groups of items) and 256 and under the three
    AIM_DEBUG_POISON_* knobs."""
    f = str(tmp_path / "k.npz")
    p = child.run("test_extend_gpu", "knob_batch", npz=f, env=dict(env, AIM_PLAN_DEBUG="1"))
    grid = 32 if env["AIM_CHIP_CUS"] == "1" else 129
    apply_grid = 8 if env["AIM_CHIP_CUS"] == "1" else 17
    line = "[aim plan] extend_sides_kernel grid=%d block=64 lds=2656 step=1 rings=12+2*4 reads=1027 K=4 read_size=104; extend_apply_kernel grid=%d block=256"
    assert line % (grid, apply_grid) in p.stderr, p.stderr
    assert "step=1 rings=65+2*4 reads=65 K=16 read_size=1024" in p.stderr, p.stderr
    out = np.load(f)
    for i, case in enumerate(KNOB_CASES):
        want = directed(case)[2]
        for name, w in zip(OUT, want):
            assert out["%s_%d" % (name, i)].tobytes() == w.tobytes(), (name, case, env)


def test_whole_path():
    p = child.run("test_extend_gpu", "whole_path", cuda_first=True, marker="EXTEND_WHOLE_PATH_OK", check=False)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "EXTEND_WHOLE_PATH_OK" in p.stdout, p.stdout + p.stderr


def inner_clips(words, seg, text_pos, slots, halves, K):
    """The read bases of a record's own half that its CIGAR soft-clips at an inner (not open) side, summed over the records of `slots`:
    the clip at that side less the bases beyond the half's true cut (the other half of the read is clipped there whatever the
    segment does), never below zero."""
    import split_model as sm
    total = 0
    for slot in slots:
        w, sg = words[slot], seg[slot]
        lead = (w[0] >> 4) if w and w[0] & 15 == 4 else 0
        trail = (w[-1] >> 4) if len(w) > 1 and w[-1] & 15 == 4 else 0
        left, right = (trail, lead) if int(text_pos[slot]) >> 63 else (lead, trail)      # strand 1 shows the read reverse-complemented
        hf = sm.half_of(halves[slot // K], int(sg["q_begin"]), int(sg["q_end"]))
        fl = int(sg["flags"])
        if not fl & sm.LEFT_OPEN:
            total += max(left - hf["q_lo"], 0)
        if not fl & sm.RIGHT_OPEN:
            total += max(right - (int(sg["read_len"]) - hf["q_hi"]), 0)
    return total


def whole_path():
    """The chimeric reads: seed_chain_candidates, chain_classify, split_segments, then once without and once with extend_segments:
    aim_align_device_ref over all n * K segment rows (WFA (3, 4, 1), BACKTRACE | ENDSFREE | REF_TEXTS, 2 * flank of free text at both
    ends, MAX_SCORE = bound + 16 as test_split_gpu sizes it) and aim_sam_device_split. Checked with the extension: segments and d_ext
    equal the model; every read gives two mapped records, one with 0x800; the read-consuming CIGAR lengths sum to read_len; every record
    lies inside its half's true interval widened by flank + edits; every score is at most bound + x * (the overshoot of the segment's
    inner sides past the true cut); the inner clips (inner_clips: the clipped bases of a record's own half) sum to at most a quarter of
    those without the extension."""
    import torch
    import chain_class_model as ccm
    import extend_model as em
    import split_model as sm
    from aim_amd import capi, engine
    ref = reference()
    rows, rl, halves, (m_req, m_tpos, m_seeds, m_chains), m_cls, m_split = chimeric_expected()
    k, stride, w, max_occ, band, flank, min_votes, K = ccm.CHIMERIC_ROW
    rs, n = ccm.CHIMERIC_SIZE, len(rl)
    p = em.Params(1, 3, 4, 1, 20, 400, 31, 64)
    want, want_ext = em.extend_segments(p, K, rs, len(ref), rl, rows, ref, *m_split)
    x, o, e = 3, 4, 1
    bound = ccm.CHIMERIC_EDITS * max(x, o + e)
    max_score = bound + 16
    dev = torch.device("cuda:0")
    params = hs.wfa_params(max_score, rs, x, o, e, 2 * flank)
    rows_n = n * K
    d_ref = put(ref, dev, 64)
    sp = engine.seed_params(k, rs, stride=stride, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, max_cands=K, w=w)
    clips = {}
    for extend in (False, True):
        out = hs.segment_rows(sp, ref, rl, rows, extend=(d_ref, engine.extend_params(*p)) if extend else None)
        if extend:
            got = (out["seg_req"], out["seg_text_pos"], out["seg_patterns"], out["seg"], out["ext"])
            for name, g, wnt in zip(OUT, got, want + (want_ext,)):
                assert g.tobytes() == wnt.tobytes(), name
        seg = out["seg"]
        d_res, _, s = hs.segment_records(params, out, rows_n, d_ref, len(ref))
        rec, cg, cur = s["sam"], s["cigar"], s["cur"]
        assert cur[0] <= rows_n * 64 and cur[1] <= rows_n * 256 and not (rec["status"] & sm.SAM_OVERFLOW).any()
        res = d_res.cpu().numpy().view(capi.RESULT_DTYPE)
        words = [[int(v) for v in cg[int(r["cigar_offset"]):int(r["cigar_offset"]) + int(r["n_cigar"])]] for r in rec]
        mapped = (rec["flags"] & sm.SAM_UNMAPPED) == 0
        valid = (seg["flags"] & sm.VALID) != 0
        print("extend", extend, "mapped per read", mapped.reshape(n, K).sum(axis=1).tolist())
        assert np.array_equal(mapped, valid) and (mapped.reshape(n, K).sum(axis=1) == 2).all()
        assert ((mapped & (rec["flags"] & sm.SAM_SUPPLEMENTARY != 0)).reshape(n, K).sum(axis=1) == 1).all()
        over = {}
        for slot, side, g in inner_gaps(seg, halves, K):
            over[slot] = over.get(slot, 0) + max(-g, 0)
        scores = []
        for slot in np.nonzero(mapped)[0]:
            r, sg, rc_ = slot // K, seg[slot], rec[slot]
            L = int(rl[r])
            assert sm.read_consumed(words[slot]) == L == int(sg["read_len"]), (slot, words[slot])
            hf = sm.half_of(halves[r], int(sg["q_begin"]), int(sg["q_end"]))
            slack = flank + hf["edits"]
            pos, span = int(rc_["pos"]), int(rc_["ref_span"])
            assert (int(rc_["flags"]) & sm.SAM_REVERSE != 0) == bool(hf["strand"]), (slot, rc_, hf)
            assert hf["ref_lo"] - slack <= pos and pos + span <= hf["ref_hi"] + slack, (slot, rc_, hf)
            assert 0 <= int(rc_["score"]) <= bound + x * over.get(int(slot), 0) and int(res["status"][slot]) == capi.PAIR_OK, (slot, rc_, over.get(int(slot), 0))
            scores.append(int(rc_["score"]))
        clips[extend] = inner_clips(words, seg, out["seg_text_pos"], np.nonzero(mapped)[0], halves, K)
        print("scores", scores, "bound", bound, "cap", max_score)
        print("inner clips", clips[extend])
    assert 4 * clips[True] <= clips[False], clips
