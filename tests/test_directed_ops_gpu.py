"""The record kernels of sam_fields.hpp on the directed ops rows of directed_ops.py, through aim_sam_device and aim_sam_device_split:
every batch on both mappings (AIM_SAM_WAVE_MIN) with and without AIM_SAM_EQX against tests/sam_model.py, capacities equal to the need,
guards behind them, the cursors equal to the model's totals; the two mappings against each other; the batch cut to grid edges; a
d_sel with UINT32_MAX entries; the split kernels with segments that merge with peels longer than a tile; and the same tile edges on
rows that the alignment kernels wrote. tests/test_directed_ops_cpu.py shows what these rows can tell apart."""
import os
import re
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import directed_ops as do  # noqa: E402
import sam_model  # noqa: E402
from gpu_buffers import cached  # noqa: E402
from sam_rows import sam_both, sam_device  # noqa: E402

MAPPINGS = {"row-per-wavefront": ("0", "sam_wave_kernel"), "row-per-lane": ("1000000", "sam_lane_kernel")}
# name -> (READ_SIZE, groups, reference length); the smallest READ_SIZE that holds each group
BATCHES = {"T": (1024, ("T",), do.REF_LEN), "LDBUR": (1024, ("L", "D", "B", "U", "R"), do.REF_LEN), "LBU-64": (64, ("L", "B", "U"), do.REF_LEN),
           "long-digits": (65528, ("DL",), 300000)}
COMPARED = ("idx", "score", "pos", "ref_span", "nm", "n_cigar", "md_len", "flags", "status", "pad")


def batch(name):
    """(reference, laid batch, {eqx: expected}) of a named batch, once per process."""
    def make():
        rs, groups, ref_len = BATCHES[name]
        ref = do.reference(ref_len)
        rows = do.long_rows() if groups == ("DL",) else [r for r in do.rows_of(groups) if len(r.scn.walk) + 8 <= 2 * rs]
        b = do.lay(rows, rs, ref)
        return ref, b, {eqx: do.expected(b, ref, eqx) for eqx in (False, True)}
    return cached(("directed-ops", name), make)


def params(rs):
    from aim_amd import capi, engine
    assert do.RESULT == capi.RESULT_DTYPE
    return engine.make_params("wfa", do.MAX_SCORE, rs, backtrace=True, ref_texts=True)


def pick(mapping, rs, monkeypatch):
    from aim_amd import engine
    wave_min, kernel = MAPPINGS[mapping]
    monkeypatch.setenv("AIM_SAM_WAVE_MIN", wave_min)
    p = params(rs)
    assert engine.sam_kernel_name(p) == kernel
    return p


def judge(out, res, exp):
    """The records are the model's, the cursors its totals; idx, score and status are the rows'."""
    sam, cg, md, cur = out
    assert sam_model.check_records(sam, cg, md, exp) == []
    assert tuple(int(x) for x in cur) == do.need(exp)
    assert np.array_equal(sam["idx"], res["idx"]) and np.array_equal(sam["score"], res["score"])
    assert np.array_equal(sam["status"], res["status"].astype(np.uint16))


def content(out, r):
    sam, cg, md, _ = out
    rec = sam[r]
    co, nc, mo, ml = int(rec["cigar_offset"]), int(rec["n_cigar"]), int(rec["md_offset"]), int(rec["md_len"])
    return tuple(int(rec[f]) for f in COMPARED), cg[co:co + nc].tolist(), md[mo:mo + ml].tobytes()


@pytest.mark.parametrize("name", list(BATCHES))
def test_every_batch_on_both_mappings_and_options(name, monkeypatch):
    """Capacities are exactly the need (sam_device asserts the guard word and byte behind them), the reference is uploaded at exactly
    ref_len bytes, and the two mappings give the same records and the same addressed content row for row."""
    from aim_amd import capi
    ref, b, exps = batch(name)
    assert len(b["rows"]) <= 1000
    for eqx in (False, True):
        nc, nb = do.need(exps[eqx])
        outs = []
        for mapping in MAPPINGS:
            p = pick(mapping, b["rs"], monkeypatch)
            out = sam_device(p, b["res"], b["ops"], b["tpos"], ref, options=capi.SAM_EQX if eqx else 0, ccap=nc, mcap=nb, ref_slack=0)
            judge(out, b["res"], exps[eqx])
            outs.append(out)
        for r in range(len(b["rows"])):
            assert content(outs[0], r) == content(outs[1], r), (r, b["rows"][r].scn.name)
    un = sum(1 for e in exps[False] if e[5] == sam_model.SAM_UNMAPPED)
    assert name == "long-digits" or un >= 8 or "U" not in BATCHES[name][1]


CUTS = (1, 3, 4, 5, 63, 64, 65, 130)


@pytest.mark.parametrize("mapping", list(MAPPINGS))
def test_grid_cuts(mapping, monkeypatch):
    """n_rows at the edges of a workgroup of four wavefronts and of a wavefront of 64 lanes, over the scenario list rotated by another
    amount for every cut: each scenario meets other lanes and other wavefronts, and the last workgroup is partly empty."""
    from aim_amd import capi
    parts = [batch("T"), batch("LDBUR")]
    ref = parts[0][0]
    res, ops, tpos = (np.concatenate([p[1][k] for p in parts]) for k in ("res", "ops", "tpos"))
    p = pick(mapping, 1024, monkeypatch)
    total = len(res)
    met = set()
    for c, n in enumerate(CUTS):
        eqx = bool(c & 1)
        exp_all = parts[0][2][eqx] + parts[1][2][eqx]
        idx = (np.arange(n) * 11 + 97 * c + 13) % total               # (a stride of 11 rows: every cut draws from all groups)
        exp = [exp_all[i] for i in idx]
        nc, nb = do.need(exp)
        out = sam_device(p, res[idx], ops[idx], tpos[idx], ref, options=capi.SAM_EQX if eqx else 0, ccap=max(nc, 1), mcap=max(nb, 1), ref_slack=0)
        judge(out, res[idx], exp)
        met |= {(int(i), r % 64, (r // 64) % 4) for r, i in enumerate(idx)}
    assert len({i for i, _, _ in met}) >= 250


@pytest.mark.parametrize("mapping", list(MAPPINGS))
def test_d_sel_with_rows_without_a_candidate(mapping, monkeypatch):
    """The T and U rows under one permutation of the candidates in which every seventh row has none (UINT32_MAX): row r keeps its
    result and ops row and takes the window and strand of candidate sel[r]."""
    ref, bt, _ = batch("T")
    _, bu, _ = batch("LDBUR")
    u = [i for i, r in enumerate(bu["rows"]) if r.scn.group == "U"]
    res, ops, tpos = (np.concatenate([bt[k], bu[k][u]]) for k in ("res", "ops", "tpos"))
    n = len(res)
    stride = next(s for s in (7, 11, 13) if n % s)                          # (coprime to n: a permutation)
    sel = ((np.arange(n, dtype=np.int64) * stride + 3) % n).astype(np.uint32)
    assert len(set(sel.tolist())) == n
    sel[::7] = do.UINT32_MAX
    p = pick(mapping, 1024, monkeypatch)
    both = dict(res=res, ops=ops, tpos=tpos)
    for eqx in (False, True):
        exp = do.expected(both, ref, eqx, sel=sel)
        nc, nb = do.need(exp)
        out = sam_device(p, res, ops, tpos, ref, sel=sel, options=int(eqx), ccap=nc, mcap=nb, ref_slack=0)
        judge(out, res, exp)
        assert all(exp[r] == (0, 0, 0, [], b"", 4) for r in range(0, n, 7))
        assert sum(1 for r in range(n) if exp[r][5] != 4 and (exp[r][5] == 0x10) != bool(int(tpos[r]) >> 63)) >= 100, "the strand follows the candidate"


def long_peel(scn, end):
    """The scenario's peel at the record's first (0) or last (-1) end is longer than a tile."""
    m = re.match(r"(lead|trail)(\d+)", scn.name)
    return bool(m) and (m.group(1) == "lead") == (end == 0) and int(m.group(2)) > do.T


@pytest.mark.parametrize("mapping", list(MAPPINGS))
def test_split_records_on_the_directed_rows(mapping, monkeypatch):
    """aim_sam_device_split over the T, L and U rows. The segments cycle as in test_split_gpu.hand_rows: clips at both ends, a lead only,
    a trail only, none, no segment (flags 0), and supplementary or not. Counted: clips that merge with a peel longer than a tile at
    that end, and clips at an end without a peel, where n_cigar grows by one."""
    import split_model as sm
    from aim_amd import capi
    ref, bt, _ = batch("T")
    _, bl, _ = batch("LDBUR")
    keep = [i for i, r in enumerate(bl["rows"]) if r.scn.group in ("L", "U")]
    res, ops, tpos = (np.concatenate([bt[k], bl[k][keep]]) for k in ("res", "ops", "tpos"))
    rows = bt["rows"] + [bl["rows"][i] for i in keep]
    n = len(res)
    seg = np.zeros(n, dtype=sm.SEGMENT)
    kinds = [(7, 9), (13, 0), (0, 21), (0, 0), None, (300, 401)]
    for i in range(n):
        kind = kinds[(i + i // 8) % len(kinds)]                      # (i // 8: the eight rows of a scenario do not all meet one kind)
        if kind is not None:
            body = 500 + i % 1000
            seg[i] = (kind[0], kind[0] + body, kind[0] + body + kind[1], sm.VALID | (sm.SUPPLEMENTARY if i % 4 < 2 else 0), i % 16)
    p = pick(mapping, 1024, monkeypatch)
    both = dict(res=res, ops=ops, tpos=tpos)
    seen = dict(merged_long_peel=0, grown=0, no_segment=0, unmapped_valid=0, supplementary=0)
    for eqx in (False, True):
        exp = do.expected(both, ref, eqx)
        nc, nb = do.need(exp)
        plain, split = sam_both(p, res, ops, tpos, ref, seg, options=capi.SAM_EQX if eqx else 0, ccap=nc, mcap=nb, split_ccap=nc + 2 * n, ref_slack=0)
        judge(plain, res, exp)
        want, words = sm.sam_split(plain[0], plain[1], seg, tpos)
        sm.check_split_records(split[0], split[1], split[2], want, words, plain[0], plain[2])
        assert int(split[3][0]) == sum(len(w) for w in words) and int(split[3][1]) == int(want["md_len"].sum())
        for r in range(n):
            sg = seg[r]
            if not sg["flags"]:
                seen["no_segment"] += 1
                continue
            if exp[r][5] == sam_model.SAM_UNMAPPED:
                seen["unmapped_valid"] += 1
                continue
            clips = [int(sg["q_begin"]) > 0, int(sg["read_len"]) > int(sg["q_end"])]
            if int(tpos[r]) >> 63:
                clips = clips[::-1]
            pw = exp[r][3]
            for end, clip in ((0, clips[0]), (-1, clips[1])):
                peel = (pw[end] >> 4) if pw[end] & 15 == 4 else 0
                seen["merged_long_peel"] += bool(clip and peel and long_peel(rows[r].scn, end))
                seen["grown"] += clip and not peel
            assert len(words[r]) == len(pw) + sum(1 for end, clip in ((0, clips[0]), (-1, clips[1])) if clip and pw[end] & 15 != 4), r
            seen["supplementary"] += bool(int(split[0]["flags"][r]) & sm.SAM_SUPPLEMENTARY)
    print(seen)
    assert all(v >= 16 for v in seen.values()), seen


def planted_reads(ref, rs):
    """Reads of 600 bases cut from the reference and their intended walks: one substitution each at walk position 255, 256 and 257, a
    12-base deletion over 250 .. 261, a 70-base deletion ending at 511; each on both strands. The windows hold A C G T only and are
    chosen so that neither deletion can slide: the base in front of it differs from its last base and the base behind it from its
    first."""
    from aim_amd import capi, engine
    L = 600
    plans = [("x", 255, 1), ("x", 256, 1), ("x", 257, 1), ("del", 250, 12), ("del", 442, 70)]
    req = np.zeros(2 * len(plans), dtype=capi.REQUEST_DTYPE)
    pat = np.zeros((len(req), rs), dtype=np.uint8)
    tpos = np.zeros(len(req), dtype=np.uint64)
    walks = []
    pos = 1000
    for i in range(len(req)):
        kind, at, ln = plans[i // 2]
        minus = i & 1
        while True:
            pos += 37
            w = ref[pos:pos + L]
            if not np.isin(w, np.frombuffer(b"ACGT", dtype=np.uint8)).all():
                continue
            if kind == "del" and (w[at - 1] == w[at + ln - 1] or w[at + ln] == w[at]):
                continue
            break
        read = w.copy()
        if kind == "x":
            read[at] = ord("C") if w[at] == ord("A") else ord("A")
            walks.append(b"M" * at + b"X" + b"M" * (L - at - 1))
        else:
            read = np.concatenate([w[:at], w[at + ln:]])
            walks.append(b"M" * at + b"I" * ln + b"M" * (L - at - ln))
        row = engine.ref_window(read, 0, len(read), bool(minus))
        pat[i, :len(row)] = row
        req["pattern_len"][i], req["text_len"][i], req["idx"][i] = len(row), L, i
        tpos[i] = pos | (minus << 63)
    return req, pat, tpos, walks


@pytest.mark.parametrize("wave_min", ["0", None], ids=["row-per-wavefront", "default"])
def test_tile_edges_on_rows_the_aligner_wrote(wave_min, monkeypatch):
    """Through AIM_FLAG_SAM_FIELDS on global WFA: the flag-less ops rows are first shown to be the intended ones (the walk, reversed on
    strand 1), then the flagged call's records are the model's (test_sam_fields_gpu.both)."""
    import test_sam_fields_gpu as S
    from aim_amd import engine
    if wave_min is None:
        monkeypatch.delenv("AIM_SAM_WAVE_MIN", raising=False)
    else:
        monkeypatch.setenv("AIM_SAM_WAVE_MIN", wave_min)
    ref = do.reference()
    ms, rs = engine.launcher_sizes("wfa", 600, 0.05)
    ms += 200
    assert engine.sam_kernel_name(engine.make_params("wfa", ms, rs, backtrace=True, ref_texts=True, sam=True)) == ("sam_wave_kernel" if wave_min == "0" else "sam_lane_kernel")
    req, pat, tpos, walks = planted_reads(ref, rs)
    out0, out1, exps, _ = S.both(dict(), ms, rs, "wfa", ref, req, pat, tpos)
    res, ops = out0[0]["res"], out0[0]["ops"]
    for i, walk in enumerate(walks):
        b, e = int(res["begin_offset"][i]), int(res["end_offset"][i])
        assert ops[i, b:e].tobytes() == (walk[::-1] if i & 1 else walk), (i, ops[i, b:e].tobytes())
    cigars = [sam_model.cigar_string(e[3]) for e in exps[0]]
    assert cigars == ["600M"] * 6 + ["250M12D338M"] * 2 + ["442M70D88M"] * 2, cigars
    mds = [e[4] for e in exps[0]]
    assert [len(m) for m in mds[:6]] == [7] * 6 and mds[0][:3] == b"255" and mds[2][:3] == b"256" and mds[4][:3] == b"257" and mds[9][:4] == b"442^"
    assert {int(f) for f in out1[0]["sam"]["flags"]} == {0, 0x10}
