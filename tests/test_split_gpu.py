"""Split reads on the GPU. The contract is byte equality with rule 10c as tests/split_model.py writes it down, over buffers prefilled
with 0xEE: split_segments_kernel on the synthetic batch for every K, batch size and row size below (both lane mappings, across and
beyond one workgroup, one read in a row of 65 528 cut into shares), on the chain kernels' own device buffers (the chimeric reads
through both chain kernels), the single-primary identity on the short reads, the same bytes on a grid of eight workgroups and under the
poison knobs, and the whole path chain -> classify -> split -> align -> SAM records with the rest of the read clipped, on both
mappings of the record kernels; aim_sam_device_split on hand-made rows and segments on both mappings: clips that merge with a peeled S,
d_sel with UINT32_MAX, valid segments on unmapped and over-cap rows, and the overflow rule with the added words."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import child  # noqa: E402
import hand_stages as hs  # noqa: E402
from gpu_buffers import Hip, cached, put  # noqa: E402
from hand_stages import chain_classify_split  # noqa: E402
from pipeline_batches import FULL, READ_SIZE, chimeric_expected, expected, reference, short_reads  # noqa: E402
from sam_model import HAND_ROWS, make_reference  # noqa: E402
from sam_rows import sam_both  # noqa: E402

KS = (1, 3, 4, 5, 8, 11, 16)       # (lanes follow the row size here, but lanes i < K carry the decision: 3, 5 and 11 leave the group of a K unfilled)
N_READS = (1, 65, 4099)             # below, across and beyond one workgroup; never a multiple of the reads per wavefront
READ_SIZES = (104, 1024)            # 16 lanes per read, 64 lanes per read
OUT = ("seg_req", "seg_text_pos", "seg_patterns", "seg")


def synthetic(K, rs, n=max(N_READS)):
    import split_model as sm

    def make():
        d = sm.synthetic(1, n, K, rs)
        return d, sm.synthetic_segments(d, K, rs)
    return cached(("syn", K, rs, n), make)


def run_split(h, K, read_size, flank, ref_len, d):
    """aim_split_segments_device over uploaded arrays, every output prefilled with 0xEE: (requests, text_pos, patterns, segments)."""
    from aim_amd import capi, engine
    n = len(d["read_len"])
    d_req, d_tp, d_pat, d_seg = h.filled(n * K * 16), h.filled(n * K * 8), h.filled(n * K * read_size + 64), h.filled(n * K * 8)
    engine.split_segments_device(K, read_size, flank, ref_len, n, h.up(np.ascontiguousarray(d["read_len"], dtype=np.int32)), h.up(d["reads"], 64),
                                 h.up(d["req"]), h.up(d["text_pos"]), h.up(d["seed"]), h.up(d["chains"]), h.up(d["cls"]), d_req, d_tp, d_pat, d_seg)
    pat = h.down(d_pat, n * K * read_size + 64)
    assert (pat[n * K * read_size:] == 0xEE).all(), "written past the pattern rows"
    return (h.down(d_req, n * K * 16).view(capi.REQUEST_DTYPE), h.down(d_tp, n * K * 8).view(np.uint64), pat[:n * K * read_size].reshape(n * K, read_size),
            h.down(d_seg, n * K * 8).view(capi.SEGMENT_DTYPE))


def same(got, want, n_slots=None):
    for name, g, w in zip(OUT, got, want):
        w = w if n_slots is None else w[:n_slots]
        if g.tobytes() != w.tobytes():
            bad = np.nonzero((g.reshape(len(w), -1).view(np.uint8) != w.reshape(len(w), -1).view(np.uint8)).any(axis=1))[0]
            raise AssertionError((name, "slots", bad[:8].tolist(), g[bad[0]], w[bad[0]]))


@pytest.mark.parametrize("rs", READ_SIZES)
@pytest.mark.parametrize("K", KS)
def test_segments_equal_model(K, rs):
    import split_model as sm
    d, want = synthetic(K, rs)
    fl = want[3]["flags"]
    assert (fl & sm.VALID).any() and (fl == 0).any() and (fl & sm.LOOSE).any() and ((fl & sm.VALID != 0) & (fl & 12 == 0)).any() == (K > 2)
    with Hip() as h:
        for n in N_READS:
            same(run_split(h, K, rs, sm.SYN_FLANK, sm.SYN_REF_LEN, sm.prefix(d, n, K)), want, n * K)
            h.free()


def test_one_read_in_a_row_of_65528():
    """The largest row: one read, K = 4, cut into shares that groups of their own walk (parts = 16 at this size)."""
    import split_model as sm
    d, want = synthetic(4, 65528, n=1)
    d2, want2 = synthetic(16, 65528, n=3)
    assert (want[3]["flags"] & sm.VALID).any() and (want2[3]["flags"] & sm.VALID).sum() >= 3
    with Hip() as h:
        same(run_split(h, 4, 65528, sm.SYN_FLANK, sm.SYN_REF_LEN, d), want)
        same(run_split(h, 16, 65528, sm.SYN_FLANK, sm.SYN_REF_LEN, d2), want2)


@pytest.mark.parametrize("max_hits", (None, 1024), ids=("seed_chain_device", "seed_chain_long_device"))
def test_chimeric_reads_on_the_device_chain(max_hits):
    import chain_class_model as ccm
    import split_model as sm
    rows, rl, halves, chain, cls, want = chimeric_expected()
    K = ccm.CHIMERIC_ROW[7]
    assert ((want[3]["flags"].reshape(-1, K) & sm.VALID != 0).sum(axis=1) == 2).all()
    got_chain, got = chain_classify_split(ccm.CHIMERIC_ROW, rows, rl, ccm.CHIMERIC_SIZE, max_hits=max_hits)
    for g, w in zip(got_chain, chain + (cls,)):
        assert g.tobytes() == w.tobytes()
    same(got, want)


def test_single_primary_identity():
    """Every short read with a single primary: the segment's request, text_pos and pattern row are the chain kernel's slot and the read
    row, byte for byte; and the whole output equals the model."""
    import chain_class_model as ccm
    import split_model as sm
    rows, rl = short_reads()[:2]
    case = FULL[0]
    K, flank = case[7], case[5]
    (req, tpos, seeds, chains, cls), got = chain_classify_split(case, rows, rl, READ_SIZE)
    want_chain = expected(case, rows, rl, "short")
    assert req.tobytes() == want_chain[0].tobytes() and chains.tobytes() == want_chain[4].tobytes()
    same(got, sm.segments(K, READ_SIZE, flank, len(reference()), rl, rows, req, tpos, seeds, chains, cls))
    prim = (cls["flags"].reshape(-1, K) & ccm.PRIMARY) != 0
    sole = np.nonzero(prim.sum(axis=1) == 1)[0]
    assert len(sole) >= 150 and (prim[sole, 0]).all()
    s_req, s_tp, s_pat, s_seg = got
    for r in sole:                                            # (short_reads() rows are zero behind read_len: the row is the segment's pattern)
        slot = r * K
        assert s_req[slot].tobytes() == req[slot].tobytes() and s_tp[slot] == tpos[slot] and s_pat[slot].tobytes() == rows[r].tobytes(), r
        assert tuple(s_seg[slot]) == (0, rl[r], rl[r], sm.VALID | sm.LEFT_OPEN | sm.RIGHT_OPEN, 0)


KNOB_CASES = ((4, 104), (16, 1024), (4, 65528))


def knob_n(rs):
    return 3 if rs == 65528 else max(N_READS)


def knob_batch():
    import split_model as sm
    out = {}
    with Hip() as h:
        for K, rs in KNOB_CASES:
            d, _ = synthetic(K, rs, n=knob_n(rs))
            for name, arr in zip(OUT, run_split(h, K, rs, sm.SYN_FLANK, sm.SYN_REF_LEN, d)):
                out["%s_%d_%d" % (name, K, rs)] = arr.view(np.uint8)
            h.free()
    return out


@pytest.mark.parametrize("env", [{"AIM_CHIP_CUS": "1", "AIM_DEBUG_POISON_SCRATCH": "165", "AIM_DEBUG_POISON_OPS": "77", "AIM_DEBUG_POISON_LDS": "90"},
                                 {"AIM_CHIP_CUS": "256", "AIM_DEBUG_POISON_LDS": "255"}], ids=["cus1-poison", "cus256-lds255"])
def test_grid_and_poison_identical(tmp_path, env):
    """The same bytes -- the model's -- at AIM_CHIP_CUS 1 (eight workgroups walk the batch) and 256 and under the three
    AIM_DEBUG_POISON_* knobs, on both lane mappings and on rows cut into shares."""
    f = str(tmp_path / "k.npz")
    p = child.run("test_split_gpu", "knob_batch", npz=f, env=dict(env, AIM_PLAN_DEBUG="1"))
    grid = 8 if env["AIM_CHIP_CUS"] == "1" else -(-4099 // 16)
    assert "[aim plan] split_segments_kernel grid=%d block=256 lanes=16 parts=1 reads=4099 K=4 read_size=104" % grid in p.stderr, p.stderr
    assert "lanes=64 parts=2 reads=4099 K=16 read_size=1024" in p.stderr and "lanes=64 parts=16 reads=3 K=4 read_size=65528" in p.stderr, p.stderr
    out = np.load(f)
    for K, rs in KNOB_CASES:
        _, want = synthetic(K, rs, n=knob_n(rs))
        for name, w in zip(OUT, want):
            assert out["%s_%d_%d" % (name, K, rs)].tobytes() == w.tobytes(), (name, K, rs, env)


@pytest.mark.parametrize("wave_min,kernel", [(None, "sam_lane_kernel"), ("0", "sam_wave_kernel")], ids=["default-row-per-lane", "row-per-wavefront"])
def test_whole_path(wave_min, kernel):
    """Once as a caller gets it (rows of 1 024 take the lane mapping) and once with AIM_SAM_WAVE_MIN = 0, so that both record calls take
    the wave mapping: sam_wave_split_kernel."""
    p = child.run("test_split_gpu", "whole_path", cuda_first=True, marker="SPLIT_WHOLE_PATH_OK", env={"AIM_SAM_WAVE_MIN": wave_min}, check=False)
    print(p.stdout[-3000:])
    assert p.returncode == 0 and "SPLIT_WHOLE_PATH_OK" in p.stdout and "record mapping %s\n" % kernel in p.stdout, p.stdout + p.stderr


def whole_path():
    """The chimeric reads: seed_chain_candidates, chain_classify, split_segments, aim_align_device_ref over all n * K segment rows (WFA
    (3, 4, 1), BACKTRACE | ENDSFREE | REF_TEXTS, 2 * flank of free text at both ends), then aim_sam_device and aim_sam_device_split on
    those rows. MAX_SCORE is sized as test_seed_chain_gpu sizes its own: each of a half's planted edits is one substitution, insertion
    or deletion, at most max(x, o + e), plus 16. Checked: the segments equal the model; the split records equal sam_split of the plain
    records; every read has exactly the model's mapped records -- two -- and exactly one of them lacks 0x800; the read-consuming CIGAR
    lengths sum to read_len; every record lies inside its half's true interval widened by flank + edits and covers the model chain's
    [p_lo, p_hi) shrunk by as much; every score is within the cost of the half's edits. For contrast the same reads through
    aim_align_device_groups at that MAX_SCORE: the count of reads that come back over the cap is printed."""
    import torch
    import chain_class_model as ccm
    import split_model as sm
    from aim_amd import capi, engine
    lib = capi.load()
    ref = reference()
    rows, rl, halves, (m_req, m_tpos, m_seeds, m_chains), m_cls, want = chimeric_expected()
    k, stride, w, max_occ, band, flank, min_votes, K = ccm.CHIMERIC_ROW
    rs, n = ccm.CHIMERIC_SIZE, len(rl)
    sp = engine.seed_params(k, rs, stride=stride, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, max_cands=K, w=w)
    out = hs.segment_rows(sp, ref, rl, rows)
    assert out["chains"].tobytes() == m_chains.tobytes() and out["class"].tobytes() == m_cls.tobytes()
    same((out["seg_req"], out["seg_text_pos"], out["seg_patterns"], out["seg"]), want)
    seg = out["seg"]
    x, o, e = 3, 4, 1
    bound = ccm.CHIMERIC_EDITS * max(x, o + e)
    max_score = bound + 16
    dev = torch.device("cuda:0")
    params = hs.wfa_params(max_score, rs, x, o, e, 2 * flank)
    rows_n = n * K
    d_ref = put(ref, dev, 64)
    ccap, mcap = rows_n * 64, rows_n * 256
    d_res, d_ops = hs.align_rows(params, rows_n, out["d_seg_req"], out["d_seg_patterns"], out["d_seg_text_pos"], d_ref, len(ref))
    print("record mapping", engine.sam_kernel_name(params))
    common = (params, rows_n, out["d_seg_req"], out["d_seg_text_pos"], d_res, d_ops, d_ref, len(ref), (ccap, mcap))
    p, s = hs.sam_rows(*common), hs.sam_rows(*common, split_seg=out["d_seg"])
    (plain, p_cg, p_md, p_cur), (split, s_cg, s_md, s_cur) = ((r["sam"], r["cigar"], r["md"], r["cur"]) for r in (p, s))
    assert p_cur[0] <= ccap and p_cur[1] <= mcap and s_cur[0] <= ccap and s_cur[1] == p_cur[1]
    want_rec, want_words = sm.sam_split(plain, p_cg, seg, out["seg_text_pos"])
    sm.check_split_records(split, s_cg, s_md, want_rec, want_words, plain, p_md)
    assert s_cur[0] == sum(len(wd) for wd in want_words)
    mapped = (split["flags"] & sm.SAM_UNMAPPED) == 0
    valid = (seg["flags"] & sm.VALID) != 0
    print("mapped per read", mapped.reshape(n, K).sum(axis=1).tolist())
    assert np.array_equal(mapped, valid) and (mapped.reshape(n, K).sum(axis=1) == 2).all()
    assert ((mapped & (split["flags"] & sm.SAM_SUPPLEMENTARY == 0)).reshape(n, K).sum(axis=1) == 1).all()
    res = d_res.cpu().numpy().view(capi.RESULT_DTYPE)
    scores, spans = [], []
    for slot in np.nonzero(mapped)[0]:
        r, sg, rec = slot // K, seg[slot], split[slot]
        L = int(rl[r])
        assert sm.read_consumed(want_words[slot]) == L == int(sg["read_len"]), (slot, want_words[slot])
        hf = sm.half_of(halves[r], int(sg["q_begin"]), int(sg["q_end"]))
        slack = flank + hf["edits"]
        pos, span = int(rec["pos"]), int(rec["ref_span"])
        assert (int(rec["flags"]) & sm.SAM_REVERSE != 0) == bool(hf["strand"]), (slot, rec, hf)
        assert hf["ref_lo"] - slack <= pos and pos + span <= hf["ref_hi"] + slack, (slot, rec, hf)
        start = int(m_tpos[slot]) & (sm.MINUS - 1)
        tl = int(m_req["text_len"][slot])
        c = m_chains[slot]
        p_lo = sm.recover_p_lo(start, tl, start + tl, int(c["q_lo"]), int(c["q_hi"]), int(c["ref_span"]), L, flank, rs, len(ref))
        assert p_lo is not None and pos <= p_lo + slack and pos + span >= p_lo + int(c["ref_span"]) - slack, (slot, rec, p_lo, c)
        assert 0 <= int(rec["score"]) <= bound and int(res["status"][slot]) == capi.PAIR_OK, (slot, rec)
        scores.append(int(rec["score"]))
        spans.append(span)
    print("scores", scores, "bound", bound)
    print("ref spans", spans)
    # for contrast: the whole read against every candidate window, one winner per read
    gparams = engine.make_params("wfa", max_score, rs, mismatch=x, gap_o=o, gap_e=e, read_groups=True, ref_texts=True, ends_free=(0, 0, 2 * flank, 2 * flank))
    d_off = put(engine.seed_groups_offsets(n, K), dev)
    d_gres = torch.zeros(n * capi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_best = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    gsb = lib.aim_scratch_bytes(capi.params_ref(gparams), rows_n)
    d_gscr = torch.zeros(max(gsb, 16), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    engine.align_device_groups(gparams, rows_n, n, out["d_req"].data_ptr(), out["d_reads"].data_ptr(), None, out["d_text_pos"].data_ptr(), d_ref.data_ptr(),
                               len(ref), d_off.data_ptr(), d_gres.data_ptr(), None, d_best.data_ptr(), d_gscr.data_ptr(), gsb)
    torch.cuda.synchronize()
    best = d_best.cpu().numpy().view(capi.BEST_DTYPE)
    print("whole reads over the cap through aim_align_device_groups: %d of %d" % (int((best["best_score"] > max_score).sum()), n))


# ---- aim_sam_device_split on hand-made rows ---------------------------------------------------------------------------------------
HAND_RS, HAND_CAP = 1024, 5000


def hand_rows():
    """sam_model's hand-made ops rows on both strands at every begin_offset mod 4, every one also as a row over the WFA cap;
    one candidate (text_pos, segment) per row plus four spare ones. The segments cycle through: clips at both ends, a lead only, a trail
    only, no clip at all, no segment (flags 0), and supplementary or not. Rows of gaps only give valid segments on unmapped rows; rows
    that begin or end with D give clips that merge with the peeled S."""
    import split_model as sm
    from aim_amd import capi
    rs = HAND_RS
    rows = [(o, strand, shift, over) for o in HAND_ROWS for strand in (0, 1) for shift in (0, 1, 2, 3) for over in ((False, True) if shift == 0 else (False,))]
    n = len(rows)
    res = np.zeros(n, dtype=capi.RESULT_DTYPE)
    ops = np.full((n, 2 * rs), ord("?"), dtype=np.uint8)
    tpos = np.zeros(n + 4, dtype=np.uint64)
    seg = np.zeros(n + 4, dtype=sm.SEGMENT)
    kinds = [(7, 9), (13, 0), (0, 21), (0, 0), None, (300, 401)]
    for i in range(n + 4):
        strand = rows[i][1] if i < n else i & 1
        tpos[i] = (100 + 37 * i) | (strand << 63)
        kind = kinds[i % len(kinds)]
        if kind is not None:
            body = 500 + i
            seg[i] = (kind[0], kind[0] + body, kind[0] + body + kind[1], sm.VALID | (sm.SUPPLEMENTARY if i % 4 < 2 else 0), i % 16)
    for i, (o, strand, shift, over) in enumerate(rows):
        b = 2 * rs - len(o) - shift
        ops[i, b:b + len(o)] = np.frombuffer(o, dtype=np.uint8)
        res["begin_offset"][i], res["end_offset"][i], res["idx"][i], res["score"][i] = b, b + len(o), i, HAND_CAP + 1 if over else i % 7
    return res, ops, tpos, seg


@pytest.mark.parametrize("wave_min", ["0", "1000000"], ids=["row-per-wavefront", "row-per-lane"])
def test_hand_made_rows_and_segments_on_both_mappings(wave_min, monkeypatch):
    """Split records equal sam_split of the plain records, with and without EQX, with d_sel NULL and with a d_sel that reverses the
    rows, points some at the spare candidates and gives every ninth row UINT32_MAX."""
    import split_model as sm
    from aim_amd import capi, engine
    monkeypatch.setenv("AIM_SAM_WAVE_MIN", wave_min)
    ref = make_reference(3, 40000)
    res, ops, tpos, seg = hand_rows()
    n = len(res)
    p = engine.make_params("wfa", HAND_CAP, HAND_RS, backtrace=True, ref_texts=True)
    assert engine.sam_kernel_name(p) == ("sam_wave_kernel" if wave_min == "0" else "sam_lane_kernel")
    sel = np.arange(n, dtype=np.uint32)[::-1].copy()
    sel[::5] = n + np.arange(len(sel[::5])) % 4
    sel[::9] = 0xFFFFFFFF
    seen = dict(merged=0, unmapped_valid=0, over_valid=0, no_segment=0, supplementary=0, both_clips=0, no_candidate=0)
    for s in (None, sel):
        for options in (0, capi.SAM_EQX):
            plain, split = sam_both(p, res, ops, tpos, ref, seg, sel=s, options=options, ccap=16 * n, mcap=64 * n + 4096)
            want, words = sm.sam_split(plain[0], plain[1], seg, tpos, sel=s)
            sm.check_split_records(split[0], split[1], split[2], want, words, plain[0], plain[2])
            assert int(split[3][0]) == sum(len(w) for w in words) and int(split[3][1]) == int(want["md_len"].sum())     # (a row without a segment needs none)
            for r in range(n):
                c = r if s is None else int(s[r])
                if c == 0xFFFFFFFF:
                    seen["no_candidate"] += 1
                    assert int(split[0]["flags"][r]) == sm.SAM_UNMAPPED and int(split[0]["pos"][r]) == 0
                    continue
                sg, pl = seg[c], plain[0][r]
                if not sg["flags"]:
                    seen["no_segment"] += 1
                    continue
                if int(pl["flags"]) & sm.SAM_UNMAPPED:
                    seen["over_valid" if int(res["score"][r]) == HAND_CAP + 1 else "unmapped_valid"] += 1
                    continue
                pw = [int(x) for x in plain[1][int(pl["cigar_offset"]):int(pl["cigar_offset"]) + int(pl["n_cigar"])]]
                clips = (int(sg["q_begin"]) > 0, int(sg["read_len"]) > int(sg["q_end"]))
                if int(tpos[c]) >> 63:
                    clips = clips[::-1]
                seen["merged"] += (clips[0] and pw[0] & 15 == 4) + (clips[1] and pw[-1] & 15 == 4)
                seen["both_clips"] += all(clips)
                seen["supplementary"] += bool(int(split[0]["flags"][r]) & sm.SAM_SUPPLEMENTARY)
    print(seen)
    assert all(v >= 8 for v in seen.values()), seen


@pytest.mark.parametrize("short", ["one word", "the plain need"])
@pytest.mark.parametrize("wave_min", ["0", "1000000"], ids=["row-per-wavefront", "row-per-lane"])
def test_cigar_capacity_below_the_need_with_the_added_words(wave_min, short, monkeypatch):
    """A cigar_cap one word below what the split records need, and one that is exactly what plain aim_sam_device needs: the cursors
    report the split need, the rows marked AIM_SAM_OVERFLOW have n_cigar = md_len = 0 and every other field right, their removal makes
    the rest fit, every other row is right and nothing is written past the capacity."""
    import split_model as sm
    from aim_amd import engine
    monkeypatch.setenv("AIM_SAM_WAVE_MIN", wave_min)
    ref = make_reference(3, 40000)
    res, ops, tpos, seg = hand_rows()
    none = seg["flags"] == 0                                    # every row gets a segment here, so that clips only add words
    seg[none] = (5, 505, 515, sm.VALID, 0)
    n = len(res)
    p = engine.make_params("wfa", HAND_CAP, HAND_RS, backtrace=True, ref_texts=True)
    mcap = 64 * n + 4096
    plain, _ = sam_both(p, res, ops, tpos, ref, seg, ccap=16 * n, mcap=mcap)
    want, words = sm.sam_split(plain[0], plain[1], seg, tpos)
    need, plain_need = sum(len(w) for w in words), int(plain[3][0])
    assert need > plain_need + 8          # (the 16 rows of MXXMIM and MMIIXM have no S of their own, and five segments in six clip)
    ccap = need - 1 if short == "one word" else plain_need
    _, (got, cg, md, cur) = sam_both(p, res, ops, tpos, ref, seg, ccap=16 * n, mcap=mcap, split_ccap=ccap)
    assert tuple(int(x) for x in cur) == (need, int(want["md_len"].sum()))
    over = [r for r in range(n) if int(got["status"][r]) & sm.SAM_OVERFLOW]
    assert over, "something has to give"
    for r in over:
        assert int(got["n_cigar"][r]) == 0 and int(got["md_len"][r]) == 0 and words[r]
        assert int(got["status"][r]) == int(want["status"][r]) | sm.SAM_OVERFLOW
        for f in ("idx", "score", "pos", "ref_span", "nm", "flags", "pad"):
            assert int(got[f][r]) == int(want[f][r]), (r, f)
    ok = [r for r in range(n) if r not in set(over)]
    assert sum(len(words[r]) for r in ok) <= ccap
    sm.check_split_records(got[ok], cg, md, want[ok], [words[r] for r in ok], plain[0][ok], plain[2])
    spans = sorted((int(got["cigar_offset"][r]), int(got["n_cigar"][r])) for r in ok if got["n_cigar"][r])
    assert all(a + l <= b for (a, l), (b, _) in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] <= ccap
