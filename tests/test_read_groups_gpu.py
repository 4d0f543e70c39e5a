"""Reads and their candidates in one batch (AIM_FLAG_READ_GROUPS) on the GPU. The whole contract is equality with the flag-less run
of the same candidates plus the selection model (read_groups_model.py) on the flag-less score-only results: aim_best_t, the per-read
result rows (every field), ops rows [begin_offset, end_offset), compact headers and runs -- on every algorithm and output mode, with
explicit texts and with reference windows on both strands, for groups of 1, 64, 65, 5 000 and random sizes, exact ties, a winner
whose CIGAR pass aborts, any slot count / batch split / CU count / poison knob, the stateless entry point on torch tensors, and one
4 Mi-candidate batch through two slots."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def make_reference(seed, length):
    rng = np.random.default_rng([seed, 0x67727066])
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=length)].copy()
    for _ in range(max(1, length // 20000)):          # N runs and soft-masked stretches, as in a real genome
        at = int(rng.integers(0, length - 64))
        ref[at:at + int(rng.integers(1, 40))] = ord("N")
        at = int(rng.integers(0, length - 512))
        span = slice(at, at + int(rng.integers(16, 500)))
        ref[span] = ref[span] | 0x20
    return ref


def _kw_pass1(kw):
    return {k: v for k, v in kw.items() if k not in ("backtrace", "bidir", "res8")}


def expected(algo, ms, rs, kw, req, pats, txt, offsets, runs_cap=0):
    """The flag-less runs of every candidate: (best, sel) by the model on the score-only pass, and the configured run's outputs."""
    import read_groups_model as m
    from aim_amd import engine
    p1 = engine.make_params(algo, ms, rs, **_kw_pass1(kw))
    res1, _ = engine.align(p1, req, pats, txt, check=False)
    best, sel = m.select(res1["score"], res1["status"], offsets)
    p0 = engine.make_params(algo, ms, rs, **kw)
    out = {"best": best, "sel": sel}
    with engine.DeviceSet(1) as s:
        s.configure_slots(p0, len(req), slots=1, max_runs=runs_cap)
        s.submit(0, 0, req, pat=pats, txt=txt, want_ops=bool(kw.get("backtrace")), cigar_runs_cap=runs_cap)
        out.update(s.wait(0, 0, check=False))
    return out


def run_groups(params, req, rows, offsets, txt=None, tpos=None, ref=None, runs_cap=0, slots=1, chunks=1, max_pairs=None, packed=False):
    """aim_set_submit of the groups batch, split at read boundaries into `chunks` batches over `slots` slots; outputs concatenated.
    packed: the read rows travel packed (engine.pack_batch over the reads), reads holding a byte outside A/C/G/T on the raw side list."""
    from aim_amd import engine
    n_reads = len(offsets) - 1
    read_req = req[offsets[:-1]]                 # (every candidate of a read has the read's pattern_len here)
    bounds = np.linspace(0, n_reads, chunks + 1).astype(int)
    bt = bool(params.flags & 1)
    got = []
    with engine.DeviceSet(1) as s:
        s.configure_slots(params, max_pairs or len(req), slots=slots, max_runs=runs_cap, max_raw=n_reads if packed else 0)
        if ref is not None:
            s.set_reference(ref)
        pending = []
        for c in range(chunks):
            r0, r1 = bounds[c], bounds[c + 1]
            c0, c1 = int(offsets[r0]), int(offsets[r1])
            kw = dict(want_ops=bt, cigar_runs_cap=runs_cap, read_offsets=offsets[r0:r1 + 1] - offsets[r0])
            if packed:
                kw["packed"] = engine.pack_batch(read_req[r0:r1], rows[r0:r1], None)
            else:
                kw["pat"] = rows[r0:r1]
            if tpos is not None:
                kw["text_pos"] = tpos[c0:c1]
            else:
                kw["txt"] = txt[c0:c1]
            if len(pending) == slots:
                got.append((pending.pop(0)[1], s.wait(0, (c - slots) % slots, check=False)))
            s.submit(0, c % slots, req[c0:c1], **kw)
            pending.append((c, c0))
        for k, (c, c0) in enumerate(pending):
            got.append((c0, s.wait(0, c % slots, check=False)))
        plan = s.plan_describe(0)
    out = {"plan": plan}
    for key in ("best", "res", "ops", "cig"):
        if key in got[0][1]:
            parts = []
            for c0, g in got:
                x = g[key].copy()
                if key == "best":
                    x["best_pair"] = np.where(x["n_best"] > 0, x["best_pair"] + np.uint32(c0), x["best_pair"])
                parts.append(x)
            out[key] = np.concatenate(parts)
    if "cig" in out:
        out["runs"] = np.concatenate([_runs_in_order(g["cig"], g["runs"]) for _, g in got])
    return out


def _runs_in_order(cig, runs):
    """Every row's runs, concatenated in row order (where they sit in the run buffer depends on scheduling)."""
    lens = cig["n_runs"].astype(np.int64)
    if lens.sum() == 0:
        return np.zeros(0, dtype=np.uint32)
    starts = cig["run_offset"].astype(np.int64)
    first = np.repeat(starts - np.concatenate([[0], np.cumsum(lens)[:-1]]), lens)
    return runs[first + np.arange(int(lens.sum()))]


def _hdr(cig):
    """The compact headers without run_offset (where a row's runs sit in the run buffer depends on scheduling)."""
    return np.stack([cig[k].astype(np.int64) for k in ("idx", "score", "n_runs", "status")])


def assert_groups_equal(got, exp, bt, runs):
    sel = exp["sel"]
    assert np.array_equal(got["best"], exp["best"])
    if "res" in got:
        assert np.array_equal(got["res"], exp["res"][sel])
        if bt:
            for r, i in enumerate(sel):
                b, e = int(exp["res"]["begin_offset"][i]), int(exp["res"]["end_offset"][i])
                assert np.array_equal(got["ops"][r, b:e], exp["ops"][i, b:e]), r
    if runs:
        ce = exp["cig"][sel]
        for k in ("idx", "score", "n_runs", "status"):
            assert np.array_equal(got["cig"][k], ce[k]), k
        assert np.array_equal(got["runs"], _runs_in_order(ce, exp["runs"]))


# (algo, length, error, reads, K, make_params keywords)
CASES = [
    ("nw", 100, 0.02, 300, 8, dict(backtrace=True)),
    ("swg", 100, 0.02, 300, 8, dict(backtrace=True)),
    ("swg", 100, 0.02, 300, 8, dict(backtrace=True, swg_w16=True)),
    ("swg", 100, 0.02, 300, 8, dict(res8=True)),
    ("wfa", 100, 0.01, 400, 8, dict(backtrace=True)),
    ("wfa", 100, 0.05, 400, 8, dict(reduce=True, backtrace=True, req8=True)),
    ("wfa", 100, 0.01, 400, 8, dict(reduce=True, res8=True)),
    ("wfa", 100, 0.01, 400, 8, dict(reduce=True)),
    ("wfa", 1000, 0.05, 40, 6, dict(backtrace=True)),
    ("wfa", 300, 0.03, 100, 6, dict(backtrace=True, ends_free=(0, 0, 20, 20))),
    ("wfa", 300, 0.03, 100, 6, dict(backtrace=True, gap2=(24, 1), mismatch=4, gap_o=4, gap_e=2)),
    ("wfa", 300, 0.03, 100, 6, dict(backtrace=True, linear=True, mismatch=1, gap_e=1)),
    ("wfa", 1000, 0.02, 30, 6, dict(backtrace=True, w32=True)),
    ("wfa", 1000, 0.05, 30, 6, dict(backtrace=True, bidir=True)),
    ("genasm", 1000, 0.05, 30, 4, dict(backtrace=True)),
]


def _sizes(algo, length, error, kw):
    from aim_amd import engine
    if algo == "genasm":
        return 0, engine.round_up_8(int(length * (1 + error)) + 8)
    cost = {k: kw[k] for k in ("mismatch", "gap_o", "gap_e") if k in kw}
    ms, rs = engine.launcher_sizes(algo, length, error, **cost)
    return ms, rs + (48 if "ends_free" in kw else 0)


@pytest.mark.parametrize("use_ref", [False, True], ids=["texts", "ref"])
@pytest.mark.parametrize("algo,length,error,n_reads,k,kw", CASES, ids=["%s-l%d-%s" % (c[0], c[1], "-".join(sorted(c[5]))) for c in CASES])
def test_groups_equal_flagless(algo, length, error, n_reads, k, kw, use_ref):
    from aim_amd import engine
    ref = make_reference(length, 300000)
    ms, rs = _sizes(algo, length, error, kw)
    sizes = np.random.default_rng(length).integers(1, 2 * k, size=n_reads)
    req, rows, offs, tpos, txt, pats = engine.group_pairs(length, 0, n_reads, k, length, error, ref, rs, sizes=sizes)
    bt = bool(kw.get("backtrace"))
    runs_cap = 512 * len(req) if bt else 0
    exp = expected(algo, ms, rs, kw, req, pats, txt, offs, runs_cap=runs_cap)
    pg = engine.make_params(algo, ms, rs, read_groups=True, ref_texts=use_ref, **kw)
    if use_ref:
        got = run_groups(pg, req, rows, offs, tpos=tpos, ref=ref, runs_cap=runs_cap)
    else:
        got = run_groups(pg, req, rows, offs, txt=txt, runs_cap=runs_cap)
    assert got["plan"].endswith(" groups=1")
    assert_groups_equal(got, exp, bt, bool(runs_cap))
    assert (exp["best"]["n_best"] > 0).all() or algo == "swg"


def _adaptive():
    from aim_amd import engine
    ms, rs = engine.launcher_sizes("wfa", 100, 0.02)
    return ms, rs, dict(reduce=True, backtrace=True, req8=True)


@pytest.mark.parametrize("shape", ["all1", "all64", "all65", "one5000", "random200", "ties"])
def test_group_shapes(shape):
    from aim_amd import engine
    ms, rs, kw = _adaptive()
    ref = make_reference(5, 400000)
    n_reads, sizes = {"all1": (700, [1] * 700), "all64": (40, [64] * 40), "all65": (40, [65] * 40),
                      "one5000": (5, [3, 5000, 1, 64, 7]), "random200": (60, None), "ties": (300, [8] * 300)}[shape]
    if sizes is None:
        sizes = np.random.default_rng(9).integers(1, 201, size=n_reads)
    req, rows, offs, tpos, txt, pats = engine.group_pairs(17, 0, n_reads, 8, 100, 0.02, ref, rs, sizes=sizes)
    if shape == "ties":      # duplicated windows: candidate 2j+1 repeats candidate 2j of the same read
        for r in range(n_reads):
            lo = int(offs[r])
            for j in range(0, 8, 2):
                tpos[lo + j + 1], txt[lo + j + 1] = tpos[lo + j], txt[lo + j]
    runs_cap = 16 * len(req)
    exp = expected("wfa", ms, rs, kw, req, pats, txt, offs, runs_cap=runs_cap)
    got = run_groups(engine.make_params("wfa", ms, rs, read_groups=True, ref_texts=True, **kw), req, rows, offs, tpos=tpos, ref=ref,
                     runs_cap=runs_cap)
    assert_groups_equal(got, exp, True, True)
    if shape == "all1":      # one candidate per read: the flag-less batch row for row
        assert np.array_equal(got["res"], exp["res"]) and np.array_equal(exp["sel"], np.arange(len(req)))
    if shape == "ties":
        assert (got["best"]["n_best"] >= 2).all() and (got["best"]["second_score"] == got["best"]["best_score"]).all()
        assert (got["best"]["best_pair"] % 2 == 0).all()    # the lower index of a tie wins


@pytest.mark.parametrize("algo,kw", [("wfa", dict(reduce=True, backtrace=True, req8=True)), ("wfa", dict(reduce=True, res8=True, req8=True)),
                                     ("wfa", dict(backtrace=True)), ("nw", dict(backtrace=True))],
                         ids=["adaptive-cigar", "adaptive-res8", "wfa-cigar", "nw-cigar"])
def test_packed_reads_with_reference_windows(algo, kw):
    """Packed read rows (AIM_FLAG_REF_TEXTS): reads holding N or lowercase travel on the raw side list (read indices); both strands;
    split over two slots. Every output equals the flag-less run of the explicit candidates."""
    from aim_amd import engine
    ms, rs = engine.launcher_sizes(algo, 100, 0.02)
    ref = make_reference(61, 300000)
    sizes = np.random.default_rng(61).integers(1, 24, size=400)
    req, rows, offs, tpos, txt, pats = engine.group_pairs(61, 0, 400, 8, 100, 0.02, ref, rs, sizes=sizes)
    rows[::7, 5] = ord("N")
    rows[3::11, 40] |= 0x20
    read_of = np.repeat(np.arange(400), np.diff(offs))
    pats = np.ascontiguousarray(rows[read_of])
    _, ok = engine.pack_rows(req[offs[:-1]], rows, "pattern_len")
    assert (~ok).sum() >= 80
    bt = bool(kw.get("backtrace"))
    runs_cap = 512 * len(req) if bt else 0
    exp = expected(algo, ms, rs, kw, req, pats, txt, offs, runs_cap=runs_cap)
    got = run_groups(engine.make_params(algo, ms, rs, read_groups=True, ref_texts=True, **kw), req, rows, offs, tpos=tpos, ref=ref,
                     runs_cap=runs_cap, slots=2, chunks=3, packed=True)
    assert got["plan"].endswith(" groups=1")
    assert_groups_equal(got, exp, bt, bool(runs_cap))


def test_swg_int8_winner_aborts_in_the_cigar_pass():
    """int8 SWG: the score-only pass reports OK where the CIGAR pass of the same pair stops with AIM_PAIR_SWG_NO_OP (the judge's
    swg_bt_l400_e2_int8 input, whose cells wrap); a read whose winner is such a pair reports that status, and aim_set_wait returns
    AIM_EALIGN."""
    from aim_amd import capi, engine
    ms, rs, n = 40, 416, 300
    req, pat, txt = engine.gen_pairs(713, 0, n, 400, 0.02, rs)
    kw = dict(backtrace=True)
    res0, _ = engine.align(engine.make_params("swg", ms, rs, **kw), req, pat, txt, check=False)
    abort = set(np.nonzero(res0["status"] == capi.PAIR_SWG_NO_OP)[0].tolist())
    assert abort
    # read i: its own text, plus (unless its pair aborts) the texts of pairs i + 1 and i + 2
    cand, sizes = [], []
    for i in range(n):
        own = [i] if i in abort else [i, (i + 1) % n, (i + 2) % n]
        cand += own
        sizes.append(len(own))
    cand = np.array(cand)
    read_of = np.repeat(np.arange(n), sizes)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    req2 = np.zeros(len(cand), dtype=capi.REQUEST_DTYPE)
    req2["pattern_len"], req2["text_len"], req2["idx"] = req["pattern_len"][read_of], req["text_len"][cand], np.arange(len(cand))
    txt2, pats2 = np.ascontiguousarray(txt[cand]), np.ascontiguousarray(pat[read_of])
    exp = expected("swg", ms, rs, kw, req2, pats2, txt2, offs, runs_cap=512 * len(cand))
    got = run_groups(engine.make_params("swg", ms, rs, read_groups=True, **kw), req2, pat, offs, txt=txt2, runs_cap=512 * len(cand))
    assert_groups_equal(got, exp, True, True)
    for i in abort:
        assert got["res"]["status"][i] == capi.PAIR_SWG_NO_OP and got["best"]["n_best"][i] == 1
    with engine.DeviceSet(1) as s:
        s.configure_slots(engine.make_params("swg", ms, rs, read_groups=True, **kw), len(cand), slots=1)
        s.submit(0, 0, req2, pat=pat, txt=txt2, want_ops=True, read_offsets=offs)
        with pytest.raises(capi.AimError) as e:
            s.wait(0, 0)
        assert e.value.code == capi.AIM_EALIGN


def test_slots_and_batch_split():
    from aim_amd import engine
    ms, rs, kw = _adaptive()
    ref = make_reference(31, 300000)
    sizes = np.random.default_rng(31).integers(1, 40, size=500)
    req, rows, offs, tpos, txt, pats = engine.group_pairs(31, 0, 500, 8, 100, 0.02, ref, rs, sizes=sizes)
    pg = engine.make_params("wfa", ms, rs, read_groups=True, ref_texts=True, **kw)
    a = run_groups(pg, req, rows, offs, tpos=tpos, ref=ref, runs_cap=16 * len(req))
    for slots, chunks in ((2, 3), (3, 7), (4, 4)):
        b = run_groups(pg, req, rows, offs, tpos=tpos, ref=ref, runs_cap=16 * len(req), slots=slots, chunks=chunks)
        for key in ("best", "res", "runs"):
            assert np.array_equal(a[key], b[key]), (slots, chunks, key)
        assert np.array_equal(_hdr(a["cig"]), _hdr(b["cig"]))


KNOB_CHILD = '''
import sys
import numpy as np
sys.path.insert(0, "tests")
import test_read_groups_gpu as t
from aim_amd import engine
ms, rs, kw = t._adaptive()
ref = t.make_reference(41, 200000)
req, rows, offs, tpos, txt, pats = engine.group_pairs(41, 0, 300, 8, 100, 0.02, ref, rs, sizes=np.random.default_rng(41).integers(1, 70, size=300))
g = t.run_groups(engine.make_params("wfa", ms, rs, read_groups=True, ref_texts=True, **kw), req, rows, offs, tpos=tpos, ref=ref, runs_cap=16 * len(req))
np.savez(sys.argv[1], best=g["best"], res=g["res"], cig=g["cig"], runs=g["runs"])
'''


def test_knobs_do_not_change_results(tmp_path):
    outs = []
    for i, env in enumerate(({}, {"AIM_CHIP_CUS": "40", "AIM_DEBUG_POISON_SCRATCH": "165", "AIM_DEBUG_POISON_OPS": "77",
                                  "AIM_DEBUG_POISON_LDS": "90"})):
        f = str(tmp_path / ("k%d.npz" % i))
        p = subprocess.run([sys.executable, "-c", KNOB_CHILD, f], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True,
                           timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append(np.load(f))
    for key in ("best", "res", "runs"):
        assert np.array_equal(outs[0][key], outs[1][key]), key
    assert np.array_equal(_hdr(outs[0]["cig"]), _hdr(outs[1]["cig"]))


def test_refusals_on_a_set():
    from aim_amd import capi, engine
    ms, rs, kw = _adaptive()
    ref = make_reference(3, 50000)
    req, rows, offs, tpos, txt, pats = engine.group_pairs(3, 0, 10, 4, 100, 0.02, ref, rs)
    pg = engine.make_params("wfa", ms, rs, read_groups=True, **kw)
    with engine.DeviceSet(1) as s:
        s.configure_slots(pg, 64, slots=1, max_raw=64, max_runs=1024)
        for call in (lambda: s.push(0, req, pats, txt), lambda: s.launch(), lambda: capi.check(s.lib.aim_set_pull(s.handle, 0, None, None))):
            with pytest.raises(capi.AimError) as e:
                call()
            assert e.value.code == capi.AIM_EINVAL and "aim_batch_io_groups_t" in str(e.value)
        with pytest.raises(capi.AimError) as e:
            s.submit(0, 0, req, packed=engine.pack_batch(req[offs[:-1]], rows, rows), read_offsets=offs, txt=txt, cigar_runs_cap=1024)
        assert e.value.code == capi.AIM_EINVAL and "packed batches need AIM_FLAG_REF_TEXTS" in str(e.value)
        bad = offs.copy()
        bad[4] = bad[3]
        with pytest.raises(capi.AimError) as e:
            s.submit(0, 0, req, pat=rows, txt=txt, read_offsets=bad, cigar_runs_cap=1024)
        assert e.value.code == capi.AIM_EINVAL and "read 3" in str(e.value)
        with pytest.raises(capi.AimError) as e:                  # nothing is in flight
            s.wait(0, 0)
        assert e.value.code == capi.AIM_ESTATE


ALIGN_DEVICE_GROUPS = '''
import sys
import torch
torch.cuda.init()   # (before the library: the device buffers are torch's)
sys.path.insert(0, "tests")
import test_read_groups_gpu as t
t.align_device_groups_torch()
print("ALIGN_DEVICE_GROUPS_OK")
'''


def test_align_device_groups_torch():
    p = subprocess.run([sys.executable, "-c", ALIGN_DEVICE_GROUPS], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ALIGN_DEVICE_GROUPS_OK" in p.stdout, p.stdout + p.stderr


def align_device_groups_torch():
    import torch
    from aim_amd import capi, engine
    lib = capi.load()
    dev = torch.device("cuda:0")
    ref = make_reference(19, 100000)
    ms, rs = engine.launcher_sizes("wfa", 100, 0.02)
    sizes = np.random.default_rng(19).integers(1, 30, size=200)
    req, rows, offs, tpos, txt, pats = engine.group_pairs(19, 0, 200, 8, 100, 0.02, ref, rs, sizes=sizes)
    n, nr = len(req), len(offs) - 1
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    for use_ref, kw in ((False, dict(backtrace=True)), (True, dict(backtrace=True, reduce=True)), (True, dict(reduce=True, res8=True))):
        params = engine.make_params("wfa", ms, rs, read_groups=True, ref_texts=use_ref, **kw)
        bt = bool(kw.get("backtrace"))
        d_req, d_rows, d_off = t(req), t(rows), t(offs)
        d_txt = None if use_ref else t(txt)
        d_tp = t(tpos) if use_ref else None
        d_ref = torch.zeros(len(ref) + 64, dtype=torch.uint8, device=dev)
        d_ref[: len(ref)] = torch.from_numpy(ref).to(dev)
        res_dt = capi.RESULT8_DTYPE if kw.get("res8") else capi.RESULT_DTYPE
        d_res = torch.zeros(nr * res_dt.itemsize, dtype=torch.uint8, device=dev)
        d_ops = torch.zeros(nr * 2 * rs, dtype=torch.uint8, device=dev) if bt else None
        d_best = torch.zeros(nr * 16, dtype=torch.uint8, device=dev)
        sb = lib.aim_scratch_bytes(capi.params_ref(params), n)
        assert sb > 0
        d_scr = torch.zeros(sb, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ptr = lambda x: None if x is None else x.data_ptr()
        rc = lib.aim_align_device_groups(capi.params_ref(params), n, nr, ptr(d_req), ptr(d_rows), ptr(d_txt), ptr(d_tp), ptr(d_ref), len(ref),
                                         ptr(d_off), ptr(d_res), ptr(d_ops), ptr(d_best), ptr(d_scr), sb, None)
        assert rc == 0, lib.aim_last_error()
        torch.cuda.synchronize()
        exp = expected("wfa", ms, rs, kw, req, pats, txt, offs)
        got = {"best": d_best.cpu().numpy().view(capi.BEST_DTYPE), "res": d_res.cpu().numpy().view(res_dt)}
        if bt:
            got["ops"] = d_ops.cpu().numpy().reshape(nr, 2 * rs)
        assert_groups_equal(got, exp, bt, False)


def test_four_mi_candidates_two_slots():
    """4 Mi candidates at l = 100 in groups of 8 (a 32 Ki-candidate set repeated), WFA-adaptive with compact CIGAR through two slots."""
    from aim_amd import engine
    ms, rs, kw = _adaptive()
    ref = make_reference(47, 1 << 20)
    req, rows, offs, tpos, txt, pats = engine.group_pairs(47, 0, 4096, 8, 100, 0.01, ref, rs)
    reps = 128
    n = len(req) * reps
    reqb = np.tile(req, reps)
    reqb["idx"] = np.arange(n, dtype=np.uint32)
    rowsb, tposb = np.tile(rows, (reps, 1)), np.tile(tpos, reps)
    offsb = np.arange(4096 * reps + 1, dtype=np.uint32) * 8
    pg = engine.make_params("wfa", ms, rs, read_groups=True, ref_texts=True, **kw)
    half = n // 2
    got = run_groups(pg, reqb, rowsb, offsb, tpos=tposb, ref=ref, runs_cap=8 * half, slots=2, chunks=2, max_pairs=half)
    exp = expected("wfa", ms, rs, kw, req, pats, txt, offs, runs_cap=16 * len(req))
    sel = exp["sel"]
    for rep in range(0, reps, 31):                # every 31st copy checked field by field against the flag-less run
        lo, hi = rep * 4096, (rep + 1) * 4096
        b = got["best"][lo:hi].copy()
        b["best_pair"] -= np.uint32(rep * len(req))
        assert np.array_equal(b, exp["best"])
        c = got["cig"][lo:hi]
        ce = exp["cig"][sel]
        assert np.array_equal(c["idx"] - np.uint32(rep * len(req)), ce["idx"])
        for k in ("score", "n_runs", "status"):
            assert np.array_equal(c[k], ce[k]), k
    total = got["cig"]["n_runs"].astype(np.int64)
    assert len(got["runs"]) == int(total.sum())
    assert np.array_equal(np.tile(_runs_in_order(exp["cig"][sel], exp["runs"]), reps), got["runs"])
