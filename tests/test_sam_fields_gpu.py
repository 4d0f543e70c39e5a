"""AIM_FLAG_SAM_FIELDS on the GPU. Every record is compared with tests/sam_model.py applied to the result rows, ops rows and text_pos of
the SAME call without the flag, and every other output of the flagged call (result rows, ops ranges, compact headers and runs, best,
mates) must equal the flag-less one. Offsets are never compared; the words and bytes they address are."""
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sam_model  # noqa: E402
from gpu_buffers import Hip  # noqa: E402,F401  (other test modules reach it as S.Hip)
from sam_model import HAND_ROWS, make_reference as reference  # noqa: E402
from sam_rows import sam_device  # noqa: E402

MINUS = 1 << 63
UINT32_MAX = 0xFFFFFFFF


def same_ranges(res, ops, res0, ops0):
    assert np.array_equal(res, res0)
    for i in range(len(res0)):
        b, e = int(res0["begin_offset"][i]), int(res0["end_offset"][i])
        assert np.array_equal(ops[i, b:e], ops0[i, b:e]), i


def same_runs(a, b):
    for k in ("idx", "score", "n_runs", "status"):
        assert np.array_equal(a["cig"][k], b["cig"][k]), k
    for i in range(len(a["cig"])):
        oa, ob, n = int(a["cig"]["run_offset"][i]), int(b["cig"]["run_offset"][i]), int(a["cig"]["n_runs"][i])
        assert np.array_equal(a["runs"][oa:oa + n], b["runs"][ob:ob + n]), i


def expected(params, res, ops, row_tpos, ref, eqx=False):
    """The model over flag-less rows; row_tpos[r] is the row's text_pos or None (no candidate)."""
    from aim_amd import capi
    wfa = params.algo == capi.ALGO_WFA
    return [sam_model.row_fields(res[i], ops[i], row_tpos[i], ref, wfa, params.max_score, eqx) for i in range(len(res))]


def need(exp):
    return sum(len(e[3]) for e in exp), sum(len(e[4]) for e in exp)


def submit(params, ref, req, pat, tpos, sam=None, chunks=1, slots=1, runs=0, packed=False, read_offsets=None, mates=None, check=True):
    """The batch in `chunks` pieces alternating over `slots` slots (a groups batch in one piece); the outputs of each piece."""
    from aim_amd import engine
    n = len(req)
    outs = []
    with engine.DeviceSet(1) as s:
        s.configure_slots(params, n, slots=slots, max_raw=n if packed else 0, max_runs=runs)
        s.set_reference(ref)
        if sam is not None:
            s.sam_capacity(max(sam[0], 1), max(sam[1], 1))
        edges = [n * c // chunks for c in range(chunks + 1)]
        pend = []
        for c in range(chunks):
            lo, hi = edges[c], edges[c + 1]
            slot = c % slots
            if len(pend) == slots:
                outs.append(s.wait(0, pend.pop(0), check=check))
            kw = dict(want_ops=True, cigar_runs_cap=runs, text_pos=tpos[lo:hi], sam=sam)
            if read_offsets is not None:
                kw.update(read_offsets=read_offsets, mates=mates)
            if packed:
                rq = req[read_offsets[:-1]] if read_offsets is not None else req[lo:hi]
                s.submit(0, slot, req[lo:hi], packed=engine.pack_batch(rq, pat if read_offsets is not None else pat[lo:hi], None), **kw)
            else:
                s.submit(0, slot, req[lo:hi], pat=pat if read_offsets is not None else pat[lo:hi], **kw)
            pend.append(slot)
        for slot in pend:
            outs.append(s.wait(0, slot, check=check))
        line = s.plan_describe(0)
    return outs, edges, line


def both(kw, ms, rs, algo, ref, req, pat, tpos, eqx=False, check=True, **sub):
    """Flag-less and flagged runs of the same call: the other outputs are equal, the records are the model's. Returns the flagged
    outputs and the expectation per piece."""
    from aim_amd import capi, engine
    p0 = engine.make_params(algo, ms, rs, backtrace=True, ref_texts=True, **kw)
    p1 = engine.make_params(algo, ms, rs, backtrace=True, ref_texts=True, sam=True, **kw)
    out0, edges, line0 = submit(p0, ref, req, pat, tpos, check=check, **sub)
    exps = []
    for c, o in enumerate(out0):
        if "read_offsets" in sub and sub["read_offsets"] is not None:
            ro = sub["read_offsets"]
            if sub.get("mates") is not None:
                sel = o["mates"]["best_pair"].reshape(-1).astype(np.int64)
            else:
                sel = o["best"]["best_pair"].astype(np.int64)
            sel = np.where(sel == UINT32_MAX, ro[:-1].astype(np.int64), sel)
            row_tpos = [tpos[int(c_)] for c_ in sel]
        else:
            row_tpos = list(tpos[edges[c]:edges[c + 1]])
        exps.append(expected(p0, o["res"], o["ops"], row_tpos, ref, eqx))
    ccap = max(max(need(e)[0] for e in exps), 1)
    mcap = max(max(need(e)[1] for e in exps), 1)
    out1, _, line1 = submit(p1, ref, req, pat, tpos, sam=(ccap, mcap, capi.SAM_EQX if eqx else 0), check=check, **sub)
    nob = lambda line: re.sub(r" budget=\d+", "", line)      # (the bound follows the device's free memory at configure time)
    assert nob(line1) == nob(line0) + " sam=1", (line0, line1)
    for o0, o1, exp in zip(out0, out1, exps):
        same_ranges(o1["res"], o1["ops"], o0["res"], o0["ops"])
        if "cig" in o0:
            same_runs(o1, o0)
        for k in ("best", "mates"):
            if k in o0:
                assert np.array_equal(o1[k], o0[k]), k
        assert np.array_equal(o1["sam"]["idx"], o0["res"]["idx"]) and np.array_equal(o1["sam"]["score"], o0["res"]["score"])
        assert np.array_equal(o1["sam"]["status"], o0["res"]["status"].astype(np.uint16))
        assert sam_model.check_records(o1["sam"], o1["sam_cigar"], o1["sam_md"], exp) == []
    return out0, out1, exps, p0


def endsfree_batch(seed, n, ref):
    """WFA (4, 6, 2), windows of l = 100 at e = 5 %, READ_SIZE 112, ends-free with a flank of 8: the read is the edited window without
    its first and last 8 bases, so the window carries the flanks."""
    from aim_amd import engine
    ms, rs = engine.launcher_sizes("wfa", 100, 0.05, mismatch=4, gap_o=6, gap_e=2)
    assert rs == 112
    req, pat, tpos, _ = engine.ref_pairs(seed, 0, n, 100, 0.05, ref, rs)
    for i in range(n):
        pl = int(req["pattern_len"][i])
        row = pat[i, 8:pl - 8].copy()
        pat[i] = 0
        pat[i, :len(row)] = row
        req["pattern_len"][i] = len(row)
    kw = dict(mismatch=4, gap_o=6, gap_e=2, ends_free=(0, 0, 8, 8))
    return kw, ms, rs, req, pat, tpos


@pytest.fixture(scope="module")
def wfa_ef():
    """The flag-less and flagged runs of the 1 000-pair ends-free batch through two slots, shared by the tests that start from it."""
    ref = reference(1)
    kw, ms, rs, req, pat, tpos = endsfree_batch(3, 1000, ref)
    out0, out1, exps, p0 = both(kw, ms, rs, "wfa", ref, req, pat, tpos, chunks=3, slots=2)
    return ref, req, pat, tpos, out0, out1, exps, p0, (kw, ms, rs)


def test_wfa_endsfree_two_slots(wfa_ef):
    ref, req, pat, tpos, out0, out1, exps, p0, _ = wfa_ef
    flat = [e for exp in exps for e in exp]
    flags = np.concatenate([o["sam"]["flags"] for o in out1])
    assert (flags == 0x10).sum() > 300 and (flags == 0).sum() > 300           # both strands
    assert sum(1 for e, t in zip(flat, tpos) if e[5] != 4 and e[0] != (int(t) & (MINUS - 1))) > 300   # the flanks move pos


def test_sam_device_equals_the_pipelined_records(wfa_ef):
    ref, req, pat, tpos, out0, out1, exps, p0, _ = wfa_ef
    res = np.concatenate([o["res"] for o in out0])
    ops = np.concatenate([o["ops"] for o in out0])
    exp = [e for x in exps for e in x]
    nc, nb = need(exp)
    sam, cg, md, cur = sam_device(p0, res, ops, tpos, ref, ccap=nc, mcap=nb, req=req)
    assert sam_model.check_records(sam, cg, md, exp) == [] and tuple(cur) == (nc, nb)
    # a selection: rows 0..9 follow sel, one of them has no candidate
    sel = np.array([5, 5, 0, UINT32_MAX, 9, 8, 7, 6, 1, 2], dtype=np.uint32)
    rows = [int(x) for x in np.where(sel == UINT32_MAX, 0, sel)]
    exp_sel = [exp[r] if s != UINT32_MAX else (0, 0, 0, [], b"", 4) for r, s in zip(rows, sel)]
    sam, cg, md, _ = sam_device(p0, res[rows], ops[rows], tpos, ref, sel=sel, ccap=nc, mcap=nb)
    assert sam_model.check_records(sam, cg, md, exp_sel) == []


@pytest.mark.parametrize("wave_min", ["0", "1000000"], ids=["row-per-wavefront", "row-per-lane"])
def test_hand_made_rows_on_both_mappings(wave_min, monkeypatch):
    """All-gap rows, rows of clips only, alternating terminal runs, soft clips at both ends, both strands, every begin_offset mod 4."""
    from aim_amd import capi, engine
    monkeypatch.setenv("AIM_SAM_WAVE_MIN", wave_min)
    ref = reference(3, 40000)
    rs = 1024
    rows = [(ops, strand, shift) for ops in HAND_ROWS for strand in (0, 1) for shift in (0, 1, 2, 3)]
    n = len(rows)
    res = np.zeros(n, dtype=capi.RESULT_DTYPE)
    ops = np.full((n, 2 * rs), ord("?"), dtype=np.uint8)
    tpos = np.zeros(n, dtype=np.uint64)
    for i, (o, strand, shift) in enumerate(rows):
        b = 2 * rs - len(o) - shift
        ops[i, b:b + len(o)] = np.frombuffer(o, dtype=np.uint8)
        res["begin_offset"][i], res["end_offset"][i], res["idx"][i], res["score"][i] = b, b + len(o), i, i % 7
        tpos[i] = (100 + 37 * i) | (strand << 63)
    p = engine.make_params("wfa", 5000, rs, backtrace=True, ref_texts=True)
    for eqx in (False, True):
        exp = expected(p, res, ops, list(tpos), ref, eqx)
        nc, nb = need(exp)
        sam, cg, md, cur = sam_device(p, res, ops, tpos, ref, options=capi.SAM_EQX if eqx else 0, ccap=nc, mcap=nb)
        assert sam_model.check_records(sam, cg, md, exp) == [] and tuple(cur) == (nc, nb)
        assert np.array_equal(sam["idx"], res["idx"]) and np.array_equal(sam["score"], res["score"])
    assert sum(1 for e in exp if e[5] == 4) == 16 and sum(1 for e in exp if e[3] and (e[3][0] & 15) == 4) >= 16


def test_one_pair():
    ref = reference(2, 40000)
    kw, ms, rs, req, pat, tpos = endsfree_batch(9, 1, ref)
    both(kw, ms, rs, "wfa", ref, req, pat, tpos)


@pytest.mark.parametrize("algo", ["nw", "swg"])
def test_global_dp(algo):
    """NW and SWG (int16 cells) at l = 100, e = 5 %, 512 pairs: global, so terminal gaps come from the alignment itself."""
    from aim_amd import engine
    ref = reference(4)
    ms, rs = engine.launcher_sizes(algo, 100, 0.05)
    req, pat, tpos, _ = engine.ref_pairs(12, 0, 512, 100, 0.05, ref, rs)
    req["text_len"][::7] += 5                                                # wider windows: terminal gap runs
    both(dict(swg_w16=True) if algo == "swg" else dict(), ms, rs, algo, ref, req, pat, tpos, check=False)


@pytest.fixture(scope="module")
def long_rows():
    """WFA at l = 2 000, e = 5 %, 64 pairs, both strands, a 70-base deletion planted in every read; the first 8 reads carry no other
    edit and their deletion sits at 1 200, which gives 4-digit MD counts."""
    from aim_amd import engine
    ref = reference(5)
    ms, rs = engine.launcher_sizes("wfa", 2000, 0.05)
    req, pat, tpos, txt = engine.ref_pairs(21, 0, 64, 2000, 0.05, ref, rs)
    for i in range(64):
        pl = int(req["pattern_len"][i])
        row, at = pat[i, :pl].copy(), 300 + 23 * i
        if i < 8:
            row, at = txt[i, :2000].copy(), 1200
        row = np.concatenate([row[:at], row[at + 70:]])
        pat[i] = 0
        pat[i, :len(row)] = row
        req["pattern_len"][i] = len(row)
    return ref, ms + 200, rs, req, pat, tpos


@pytest.mark.parametrize("wave_min", ["0", "1000000"], ids=["row-per-wavefront", "row-per-lane"])
def test_long_rows_on_both_mappings(long_rows, wave_min, monkeypatch):
    """The long rows on one row per wavefront and on one row per lane (AIM_SAM_WAVE_MIN picks; the default switches by READ_SIZE)."""
    from aim_amd import engine
    ref, ms, rs, req, pat, tpos = long_rows
    monkeypatch.setenv("AIM_SAM_WAVE_MIN", wave_min)
    assert engine.sam_kernel_name(engine.make_params("wfa", ms, rs, backtrace=True, ref_texts=True)) == ("sam_wave_kernel" if wave_min == "0" else "sam_lane_kernel")
    _, out1, exps, _ = both(dict(), ms, rs, "wfa", ref, req, pat, tpos)
    mds = [e[4] for e in exps[0]]
    long_del = [any(len(t) > 65 for t in re.findall(rb"\^[^0-9]+", m)) for m in mds]
    assert all(long_del[:8]) and sum(long_del) >= 48, "a ^ run longer than a wavefront"
    assert all(re.search(rb"\d{4}", m) for m in mds[:8]), "4-digit counts"
    assert {int(f) for f in out1[0]["sam"]["flags"]} == {0, 0x10}


def test_default_switch_takes_the_wave_mapping(monkeypatch):
    """No knob: l = 3 000 at e = 5 % has a READ_SIZE past the switch, so the rows go one per wavefront; 16 pairs, both strands, a
    planted 70-base deletion each."""
    from aim_amd import engine
    monkeypatch.delenv("AIM_SAM_WAVE_MIN", raising=False)
    ref = reference(13)
    ms, rs = engine.launcher_sizes("wfa", 3000, 0.05)
    assert engine.sam_kernel_name(engine.make_params("wfa", ms, rs, backtrace=True, ref_texts=True, sam=True)) == "sam_wave_kernel"
    req, pat, tpos, txt = engine.ref_pairs(23, 0, 16, 3000, 0.05, ref, rs)
    for i in range(16):
        pl = int(req["pattern_len"][i])
        row = np.concatenate([pat[i, :500 + 31 * i], pat[i, 570 + 31 * i:pl]])
        pat[i] = 0
        pat[i, :len(row)] = row
        req["pattern_len"][i] = len(row)
    _, out1, exps, _ = both(dict(), ms + 200, rs, "wfa", ref, req, pat, tpos)
    assert sum(any(len(t) > 65 for t in re.findall(rb"\^[^0-9]+", e[4])) for e in exps[0]) >= 12
    assert {int(f) for f in out1[0]["sam"]["flags"]} == {0, 0x10}


def test_short_rows_on_the_wave_mapping(wfa_ef, monkeypatch):
    """The 1 000 short ends-free rows through one row per wavefront (AIM_SAM_WAVE_MIN=0): the mappings agree wherever either runs."""
    ref, req, pat, tpos, out0, out1, exps, p0, _ = wfa_ef
    monkeypatch.setenv("AIM_SAM_WAVE_MIN", "0")
    res, ops, exp = out0[0]["res"], out0[0]["ops"], exps[0]
    nc, nb = need(exp)
    sam, cg, md, cur = sam_device(p0, res, ops, tpos[:len(res)], ref, ccap=nc, mcap=nb)
    assert sam_model.check_records(sam, cg, md, exp) == [] and tuple(cur) == (nc, nb)


def groups_batch(seed, n_reads, k, ref):
    from aim_amd import engine
    ms, rs = engine.launcher_sizes("wfa", 100, 0.05)
    req, rows, offs, tpos, _, _ = engine.group_pairs(seed, 0, n_reads, k, 100, 0.05, ref, rs)
    rng = np.random.default_rng(seed)
    rows[7, :100] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=100)]   # read 7: no candidate under the cap
    return ms, rs, req, rows, offs, tpos


@pytest.mark.parametrize("packed", [False, True], ids=["ascii", "packed"])
def test_read_groups(packed):
    """K = 4, 256 reads: record r follows sel[r]; read 7 has no candidate under the cap and is unmapped. Also as packed read rows."""
    ref = reference(6)
    ms, rs, req, rows, offs, tpos = groups_batch(31, 256, 4, ref)
    out0, out1, exps, _ = both(dict(read_groups=True), ms, rs, "wfa", ref, req, rows, tpos, read_offsets=offs, packed=packed)
    assert exps[0][7][5] == 4 and int(out1[0]["sam"]["flags"][7]) == 4
    assert sum(1 for e in exps[0] if e[5] != 4) > 200


def test_mate_pairs():
    """K = 4, 256 reads (128 read pairs): the records follow the paired selection."""
    from aim_amd import engine
    ms, rs = engine.launcher_sizes("wfa", 100, 0.05)
    ref, req, rows, offs, tpos, _, _, _ = engine.mate_pairs(41, 128, 100, 0.05, 400, 4, 0.3, read_size=rs)
    rows[6, :100] = rows[6, :100][::-1].copy()                               # read 6: no candidate under the cap
    out0, out1, exps, _ = both(dict(read_groups=True, mate_pairs=True), ms, rs, "wfa", ref, req, rows, tpos, read_offsets=offs, mates=(0, 1000, 12))
    ind = out0[0]["best"]["best_pair"].astype(np.int64)
    paired = out0[0]["mates"]["best_pair"].reshape(-1).astype(np.int64)
    assert (ind != paired).any(), "the paired choice differs from the independent one somewhere: the records must follow mates"


def test_bidir_above_t():
    from aim_amd import engine
    ref = reference(7)
    ms, rs = engine.launcher_sizes("wfa", 1000, 0.05)
    req, pat, tpos, _ = engine.ref_pairs(51, 0, 16, 1000, 0.05, ref, rs)
    _, _, _, _ = both(dict(bidir=True), ms + 50, rs, "wfa", ref, req, pat, tpos)


def test_escalate_with_a_tail():
    """90 % of the pairs at e = 1 %, 10 % at e = 5 %: the second stage's rows feed the same kernel."""
    from aim_amd import engine
    ref = reference(8)
    ms, rs = engine.launcher_sizes("wfa", 100, 0.05)
    req, pat, tpos, _ = engine.ref_pairs(61, 0, 1000, 100, 0.01, ref, rs)
    rq5, pt5, tp5, _ = engine.ref_pairs(62, 0, 1000, 100, 0.05, ref, rs)
    tail = np.arange(1000) % 10 == 3
    req[tail], pat[tail], tpos[tail] = rq5[tail], pt5[tail], tp5[tail]
    req["idx"] = np.arange(1000, dtype=np.uint32)
    out0, out1, exps, _ = both(dict(escalate=True), ms, rs, "wfa", ref, req, pat, tpos)
    assert "escalate=" in submit_line(dict(escalate=True), ms, rs)


def submit_line(kw, ms, rs):
    import ctypes as C
    from aim_amd import capi, engine
    b = C.create_string_buffer(2048)
    capi.check(capi.load().aim_plan_describe(capi.params_ref(engine.make_params("wfa", ms, rs, backtrace=True, ref_texts=True, sam=True, **kw)), 1000, b, 2048))
    return b.value.decode()


def test_req8_packed_runs_and_eqx():
    """AIM_FLAG_REQ8 + packed rows + compact runs requested together with the flag + AIM_SAM_EQX, WFA-adaptive at e = 1 % (the shape
    whose flag-less plan fuses the run output when nothing else is asked for)."""
    from aim_amd import engine
    ref = reference(9)
    ms, rs = engine.launcher_sizes("wfa", 100, 0.01)
    req, pat, tpos, _ = engine.ref_pairs(71, 0, 1000, 100, 0.01, ref, rs)
    out0, out1, exps, _ = both(dict(reduce=True, req8=True), ms, rs, "wfa", ref, req, pat, tpos, eqx=True, packed=True, runs=8000, chunks=2, slots=2)
    assert any((w & 15) == 8 for e in exps[0] for w in e[3]) and not any((w & 15) == 0 for e in exps[0] for w in e[3])


def test_runs_only_with_the_flag():
    """cigars without results or ops: the flag-less plan may fuse the run output; under the flag the ops rows stay on the device and
    the headers, runs and records are still right."""
    from aim_amd import capi, engine
    ref = reference(10)
    ms, rs = engine.launcher_sizes("wfa", 100, 0.01)
    req, pat, tpos, _ = engine.ref_pairs(81, 0, 777, 100, 0.01, ref, rs)
    p0 = engine.make_params("wfa", ms, rs, backtrace=True, ref_texts=True, reduce=True)
    p1 = engine.make_params("wfa", ms, rs, backtrace=True, ref_texts=True, reduce=True, sam=True)
    full, _, _ = submit(p0, ref, req, pat, tpos, packed=True)                 # result rows + ops rows, for the model
    exp = expected(p0, full[0]["res"], full[0]["ops"], list(tpos), ref)
    nc, nb = need(exp)
    outs = []
    for params, sam in ((p0, None), (p1, (nc, nb, 0))):
        with engine.DeviceSet(1) as s:
            s.configure_slots(params, 777, slots=1, max_raw=777, max_runs=8 * 777)
            s.set_reference(ref)
            if sam:
                s.sam_capacity(nc, nb)
            s.submit(0, 0, req, packed=engine.pack_batch(req, pat, None), cigar_runs_cap=8 * 777, text_pos=tpos, sam=sam, want_res=False)
            outs.append(s.wait(0, 0))
    assert "res" not in outs[1] and "ops" not in outs[1]
    same_runs(outs[1], outs[0])
    assert sam_model.check_records(outs[1]["sam"], outs[1]["sam_cigar"], outs[1]["sam_md"], exp) == []


def test_over_cap_pairs_are_unmapped(wfa_ef):
    """A cap of 8: most ends-free pairs come back over it (empty CIGAR) and give unmapped records; so do global WFA's over-cap rows."""
    from aim_amd import engine
    ref, req, pat, tpos, _, _, _, _, (kw, ms, rs) = wfa_ef
    _, out1, exps, _ = both(kw, 8, rs, "wfa", ref, req[:200], pat[:200], tpos[:200])
    un = out1[0]["sam"]["flags"] == 4
    assert un.sum() > 20 and (out1[0]["sam"]["score"][un] == 9).all()
    assert (out1[0]["sam"]["pos"][un] == (tpos[:200][un] & np.uint64(MINUS - 1))).all() and (out1[0]["sam"]["n_cigar"][un] == 0).all()
    glob = {k: v for k, v in kw.items() if k != "ends_free"}
    _, out1, _, _ = both(glob, 8, rs, "wfa", ref, req[:200], pat[:200], tpos[:200])
    assert (out1[0]["sam"]["flags"] == 4).sum() > 20


@pytest.mark.parametrize("short", ["cigar", "md"])
def test_capacity_one_below_the_need(wfa_ef, short):
    """One word (one byte) less than the batch needs: the rows marked AIM_SAM_OVERFLOW are a set whose removal makes the rest fit,
    every other row is right, nothing is written past the capacity. Through aim_sam_device and through aim_set_submit."""
    from aim_amd import engine
    ref, req, pat, tpos, out0, _, exps, p0, (kw, ms, rs) = wfa_ef
    res, ops, exp = out0[0]["res"], out0[0]["ops"], exps[0]
    n = len(res)
    nc, nb = need(exp)
    ccap, mcap = (nc - 1, nb) if short == "cigar" else (nc, nb - 1)

    def judge(sam, cg, md):
        over = sam_model.check_records(sam, cg, md, exp, skip_overflow=True)
        assert over, "something has to give"
        kept = [e for i, e in enumerate(exp) if i not in set(over)]
        assert need(kept)[0] <= ccap and need(kept)[1] <= mcap
        ok = [i for i in range(n) if i not in set(over)]
        spans = sorted((int(sam["cigar_offset"][i]), int(sam["n_cigar"][i])) for i in ok)
        assert all(a + l <= b for (a, l), (b, _) in zip(spans, spans[1:])) and (not spans or spans[-1][0] + spans[-1][1] <= ccap)
        spans = sorted((int(sam["md_offset"][i]), int(sam["md_len"][i])) for i in ok)
        assert all(a + l <= b for (a, l), (b, _) in zip(spans, spans[1:])) and spans[-1][0] + spans[-1][1] <= mcap

    sam, cg, md, cur = sam_device(p0, res, ops, tpos[:n], ref, ccap=ccap, mcap=mcap)
    assert tuple(cur) == (nc, nb)                                             # the cursors report the need
    judge(sam, cg, md)
    p1 = engine.make_params("wfa", ms, rs, backtrace=True, ref_texts=True, sam=True, **kw)
    outs, _, _ = submit(p1, ref, req[:n], pat[:n], tpos[:n], sam=(ccap, mcap, 0))
    same_ranges(outs[0]["res"], outs[0]["ops"], res, ops)
    judge(outs[0]["sam"], outs[0]["sam_cigar"], outs[0]["sam_md"])


@pytest.mark.parametrize("knob,value", [("AIM_DEBUG_POISON_SCRATCH", "171"), ("AIM_DEBUG_POISON_LDS", "171"), ("AIM_DEBUG_POISON_OPS", "171"),
                                        ("AIM_GROUP_PER_CU", "1"), ("AIM_GROUP_PER_CU", "3")])
def test_records_do_not_depend_on_the_poison_knobs(wfa_ef, knob, value, monkeypatch):
    """The same records (offsets aside, the content they address included) with scratch, LDS or the ops rows poisoned, and at two
    other grid sizes of the alignment kernel (wfa_group_kernel's residency knob; the plan line's grid= must move)."""
    from aim_amd import engine
    ref, req, pat, tpos, out0, _, exps, _, (kw, ms, rs) = wfa_ef
    n = len(out0[0]["res"])
    nc, nb = need(exps[0])
    p1 = engine.make_params("wfa", ms, rs, backtrace=True, ref_texts=True, sam=True, **kw)
    grid = lambda line: re.search(r"^(\w+) .* grid=(\d+) ", line).groups()
    base = grid(submit(p1, ref, req[:n], pat[:n], tpos[:n], sam=(nc, nb, 0))[2]) if knob == "AIM_GROUP_PER_CU" else None
    monkeypatch.setenv(knob, value)
    if base:
        monkeypatch.setenv("AIM_CHIP_CUS", "8")          # few enough compute units that the residency knob bounds the grid of a small batch
    outs, _, line = submit(p1, ref, req[:n], pat[:n], tpos[:n], sam=(nc, nb, 0))
    if base:
        assert base[0] == "wfa_group_kernel" and grid(line)[0] == base[0] and grid(line)[1] != base[1], (base, line)
    assert sam_model.check_records(outs[0]["sam"], outs[0]["sam_cigar"], outs[0]["sam_md"], exps[0]) == []


def test_state_and_argument_errors():
    from aim_amd import capi, engine
    ref = reference(2, 40000)
    kw, ms, rs, req, pat, tpos = endsfree_batch(9, 4, ref)
    p1 = engine.make_params("wfa", ms, rs, backtrace=True, ref_texts=True, sam=True, **kw)
    with engine.DeviceSet(1) as s:
        s.configure_slots(p1, 4, slots=1)
        s.set_reference(ref)
        with pytest.raises(capi.AimError) as e:
            s.submit(0, 0, req, pat=pat, text_pos=tpos, sam=(64, 64, 0))
        assert e.value.code == capi.AIM_ESTATE and "aim_set_sam_capacity" in str(e.value)
        s.sam_capacity(64, 256)
        with pytest.raises(capi.AimError) as e:
            s.submit(0, 0, req, pat=pat, text_pos=tpos)
        assert e.value.code == capi.AIM_EINVAL and "null sam" in str(e.value)
        for call in (lambda: s.push(0, req, pat, text_pos=tpos), s.launch, lambda: capi.check(s.lib.aim_set_pull(s.handle, 0, None, None))):
            with pytest.raises(capi.AimError) as e:
                call()
            assert e.value.code == capi.AIM_EINVAL and "AIM_FLAG_SAM_FIELDS is set" in str(e.value)
        s.submit(0, 0, req, pat=pat, text_pos=tpos, sam=(64, 256, 0), want_res=False)   # the records alone are an output
        out = s.wait(0, 0)
        assert len(out["sam"]) == 4 and (out["sam"]["n_cigar"] > 0).all()
        assert [c for c, _ in engine.sam_strings(out["sam"], out["sam_cigar"], out["sam_md"])] == \
            [sam_model.cigar_string(out["sam_cigar"][int(r["cigar_offset"]):int(r["cigar_offset"]) + int(r["n_cigar"])]) for r in out["sam"]]
    p0 = engine.make_params("wfa", ms, rs, backtrace=True, ref_texts=True, **kw)
    with engine.DeviceSet(1) as s:
        s.configure_slots(p0, 4, slots=1)
        with pytest.raises(capi.AimError) as e:
            s.sam_capacity(64, 64)
        assert e.value.code == capi.AIM_EINVAL
