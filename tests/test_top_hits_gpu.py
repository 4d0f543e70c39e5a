"""The N best candidates per read (AIM_FLAG_TOP_HITS) on the GPU. The contract is equality with the flag-less run of every candidate,
indexed by the ranking model (top_hits_model.py) on the flag-less score-only results: hit_pair, the hit rows' result rows (every
field), ops rows inside [begin_offset, end_offset), compact headers and runs in row order, and aim_best_t unchanged -- on NW, SWG and
WFA in every output mode, with explicit texts and reference windows, for reads of 1 .. 5 000 candidates around the wavefront's 64-wide
chunks and 64-read blocks, exact ties, packed read rows over several slots, a hit whose CIGAR pass aborts, any CU count or poison
knob, and the stateless entry point on torch tensors."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

_EXPECTED = {}


def expected(key, algo, ms, rs, kw, req, pats, txt, offsets, runs_cap=0):
    """The flag-less runs of every candidate, computed once per `key`: the score-only rows (res1), READ_GROUPS' (best, sel) by its
    model, and the configured run's outputs."""
    if key in _EXPECTED:
        return _EXPECTED[key]
    import read_groups_model as g
    import test_read_groups_gpu as rg
    from aim_amd import engine
    res1, _ = engine.align(engine.make_params(algo, ms, rs, **rg._kw_pass1(kw)), req, pats, txt, check=False)
    best, sel = g.select(res1["score"], res1["status"], offsets)
    out = {"res1": res1, "best": best, "sel": sel}
    with engine.DeviceSet(1) as s:
        s.configure_slots(engine.make_params(algo, ms, rs, **kw), len(req), slots=1, max_runs=runs_cap)
        s.submit(0, 0, req, pat=pats, txt=txt, want_ops=bool(kw.get("backtrace")), cigar_runs_cap=runs_cap)
        out.update(s.wait(0, 0, check=False))
    _EXPECTED[key] = out
    return out


def run_hits(params, max_hits, req, rows, offsets, txt=None, tpos=None, ref=None, runs_cap=0, slots=1, chunks=1, packed=False):
    """aim_set_submit of the batch with max_hits, split at read boundaries into `chunks` batches over `slots` slots; the hit rows
    concatenated, hit_pair and best_pair as indices of the whole batch."""
    import test_read_groups_gpu as rg
    from aim_amd import engine
    n_reads = len(offsets) - 1
    read_req = req[offsets[:-1]]
    bounds = np.linspace(0, n_reads, chunks + 1).astype(int)
    bt = bool(params.flags & 1)
    got = []
    with engine.DeviceSet(1) as s:
        s.configure_slots(params, len(req), slots=slots, max_runs=runs_cap, max_raw=n_reads if packed else 0)
        if ref is not None:
            s.set_reference(ref)
        pending = []
        for c in range(chunks):
            r0, r1 = bounds[c], bounds[c + 1]
            c0, c1 = int(offsets[r0]), int(offsets[r1])
            kw = dict(want_ops=bt, cigar_runs_cap=runs_cap, read_offsets=offsets[r0:r1 + 1] - offsets[r0], max_hits=max_hits)
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
        for c, c0 in pending:
            got.append((c0, s.wait(0, c % slots, check=False)))
        plan = s.plan_describe(0)
    out = {"plan": plan}
    for key in ("best", "res", "ops", "cig", "hit_pair"):
        if key in got[0][1]:
            parts = []
            for c0, g in got:
                x = g[key].copy()
                if key == "best":
                    x["best_pair"] = np.where(x["n_best"] > 0, x["best_pair"] + np.uint32(c0), x["best_pair"])
                if key == "hit_pair":
                    x += np.uint32(c0)
                parts.append(x)
            out[key] = np.concatenate(parts)
    counts = np.concatenate([np.diff(g["hit_offsets"].astype(np.int64)) for _, g in got])
    out["hit_offsets"] = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint32)
    if "cig" in out:
        out["runs"] = np.concatenate([rg._runs_in_order(g["cig"], g["runs"]) for _, g in got])
    return out


def assert_hits_equal(got, exp, offsets, max_hits, bt, runs):
    """Every output against the flag-less runs indexed by the model's hit_pair."""
    import test_read_groups_gpu as rg
    import top_hits_model as m
    hoff, hit_pair = m.rank(exp["res1"]["score"], exp["res1"]["status"], offsets, max_hits)
    assert np.array_equal(got["hit_offsets"], hoff)
    assert np.array_equal(got["hit_pair"], hit_pair)
    assert np.array_equal(got["hit_pair"][hoff[:-1]], exp["sel"])          # rank 0 is READ_GROUPS' choice
    assert np.array_equal(got["best"], exp["best"])
    if "res" in got:
        assert len(got["res"]) == len(hit_pair)
        assert np.array_equal(got["res"], exp["res"][hit_pair])
        if bt:
            for h, i in enumerate(hit_pair):
                b, e = int(exp["res"]["begin_offset"][i]), int(exp["res"]["end_offset"][i])
                assert np.array_equal(got["ops"][h, b:e], exp["ops"][i, b:e]), h
    if runs:
        ce = exp["cig"][hit_pair]
        for k in ("idx", "score", "n_runs", "status"):
            assert np.array_equal(got["cig"][k], ce[k]), k
        assert np.array_equal(got["runs"], rg._runs_in_order(ce, exp["runs"]))
    return hoff, hit_pair


# (algo, length, error, reads, make_params keywords)
CASES = [
    ("nw", 100, 0.02, 300, dict(backtrace=True)),
    ("swg", 100, 0.02, 300, dict(backtrace=True, swg_w16=True)),
    ("wfa", 100, 0.01, 300, dict(backtrace=True)),
    ("wfa", 100, 0.01, 300, dict(reduce=True, res8=True)),
    ("wfa", 100, 0.01, 300, dict(reduce=True)),
    ("wfa", 300, 0.03, 300, dict(backtrace=True, ends_free=(0, 0, 20, 20))),
    ("wfa", 1000, 0.05, 30, dict(backtrace=True)),
]


def _case_data(algo, length, error, n_reads, kw):
    import test_read_groups_gpu as rg
    from aim_amd import engine
    ref = rg.make_reference(length, 300000)
    ms, rs = rg._sizes(algo, length, error, kw)
    sizes = np.random.default_rng(length + n_reads).integers(1, 16, size=n_reads)      # K drawn from 1..15
    req, rows, offs, tpos, txt, pats = engine.group_pairs(length, 0, n_reads, 8, length, error, ref, rs, sizes=sizes)
    runs_cap = 512 * len(req) if kw.get("backtrace") else 0
    key = ("case", algo, length, tuple(sorted(kw)))
    return ref, ms, rs, req, rows, offs, tpos, txt, runs_cap, expected(key, algo, ms, rs, kw, req, pats, txt, offs, runs_cap=runs_cap)


@pytest.mark.parametrize("use_ref", [False, True], ids=["texts", "ref"])
@pytest.mark.parametrize("algo,length,error,n_reads,kw", CASES, ids=["%s-l%d-%s" % (c[0], c[1], "-".join(sorted(c[4]))) for c in CASES])
def test_hits_equal_flagless(algo, length, error, n_reads, kw, use_ref):
    from aim_amd import engine
    ref, ms, rs, req, rows, offs, tpos, txt, runs_cap, exp = _case_data(algo, length, error, n_reads, kw)
    bt = bool(kw.get("backtrace"))
    ph = engine.make_params(algo, ms, rs, read_groups=True, top_hits=True, ref_texts=use_ref, **kw)
    for max_hits in (1, 3, 8):
        if use_ref:
            got = run_hits(ph, max_hits, req, rows, offs, tpos=tpos, ref=ref, runs_cap=runs_cap)
        else:
            got = run_hits(ph, max_hits, req, rows, offs, txt=txt, runs_cap=runs_cap)
        assert got["plan"].endswith(" groups=1 hits=1")
        hoff, _ = assert_hits_equal(got, exp, offs, max_hits, bt, bool(runs_cap))
        assert int(hoff[-1]) == int(np.minimum(np.diff(offs.astype(np.int64)), max_hits).sum())


@pytest.mark.parametrize("algo,kw", [("wfa", dict(reduce=True, backtrace=True, req8=True)), ("wfa", dict(reduce=True, res8=True)), ("nw", dict(backtrace=True))],
                         ids=["adaptive-cigar", "adaptive-res8", "nw-cigar"])
def test_one_hit_equals_read_groups(algo, kw):
    """max_hits = 1: every output equals that of the AIM_FLAG_READ_GROUPS call of the same batch, array for array."""
    import test_read_groups_gpu as rg
    from aim_amd import engine
    ms, rs = engine.launcher_sizes(algo, 100, 0.02)
    ref = rg.make_reference(23, 200000)
    sizes = np.random.default_rng(23).integers(1, 70, size=200)
    req, rows, offs, tpos, txt, pats = engine.group_pairs(23, 0, 200, 8, 100, 0.02, ref, rs, sizes=sizes)
    bt = bool(kw.get("backtrace"))
    runs_cap = 512 * len(req) if bt else 0
    a = rg.run_groups(engine.make_params(algo, ms, rs, read_groups=True, ref_texts=True, **kw), req, rows, offs, tpos=tpos, ref=ref, runs_cap=runs_cap)
    b = run_hits(engine.make_params(algo, ms, rs, read_groups=True, ref_texts=True, top_hits=True, **kw), 1, req, rows, offs, tpos=tpos, ref=ref,
                 runs_cap=runs_cap)
    strip = lambda line: re.sub(r"budget=\d+", "budget=", line)     # (the scratch bound follows the device's free memory)
    assert strip(b["plan"]) == strip(a["plan"]) + " hits=1"
    assert np.array_equal(b["hit_offsets"], np.arange(len(offs), dtype=np.uint32))
    assert np.array_equal(a["best"], b["best"]) and np.array_equal(a["res"], b["res"])
    assert np.array_equal(b["hit_pair"], np.where(a["best"]["n_best"] > 0, a["best"]["best_pair"], offs[:-1]))
    if bt:
        assert np.array_equal(rg._hdr(a["cig"]), rg._hdr(b["cig"])) and np.array_equal(a["runs"], b["runs"])
        for r in range(len(a["res"])):
            lo, hi = int(a["res"]["begin_offset"][r]), int(a["res"]["end_offset"][r])
            assert np.array_equal(a["ops"][r, lo:hi], b["ops"][r, lo:hi]), r


def _adaptive():
    from aim_amd import engine
    ms, rs = engine.launcher_sizes("wfa", 100, 0.02)
    return ms, rs, dict(reduce=True, backtrace=True, req8=True)


SHAPE_K = [1, 3, 4, 5, 63, 64, 65, 129]      # around max_hits = 4 and around the wavefront's 64-candidate chunk


@pytest.mark.parametrize("n_reads", [1, 64, 65, 130])
def test_hit_shapes(n_reads):
    """max_hits = 4 on reads of 1, 3, 4, 5, 63, 64, 65 and 129 candidates -- one of 5 000 among them at 130 reads -- for 1, 64, 65 and
    130 reads: a wavefront's reads end inside, at and past its 64-candidate chunks and its 64-read block."""
    import test_read_groups_gpu as rg
    from aim_amd import engine
    ms, rs, kw = _adaptive()
    ref = rg.make_reference(5, 400000)
    sizes = [129] if n_reads == 1 else [SHAPE_K[(r * 3 + r // 8) % 8] for r in range(n_reads)]
    if n_reads == 130:
        sizes[70] = 5000
    req, rows, offs, tpos, txt, pats = engine.group_pairs(17, 0, n_reads, 8, 100, 0.02, ref, rs, sizes=sizes)
    runs_cap = 16 * len(req)
    exp = expected(("shape", n_reads), "wfa", ms, rs, kw, req, pats, txt, offs, runs_cap=runs_cap)
    got = run_hits(engine.make_params("wfa", ms, rs, read_groups=True, ref_texts=True, top_hits=True, **kw), 4, req, rows, offs, tpos=tpos, ref=ref,
                   runs_cap=runs_cap)
    hoff, _ = assert_hits_equal(got, exp, offs, 4, True, True)
    assert np.array_equal(np.diff(hoff.astype(np.int64)), np.minimum(sizes, 4))
    assert n_reads == 1 or set(sizes) >= set(SHAPE_K)


def test_ties_come_out_in_index_order():
    """Duplicated windows (candidate 2j + 1 repeats candidate 2j of the same read): equal scores rank by batch index."""
    import test_read_groups_gpu as rg
    from aim_amd import engine
    ms, rs, kw = _adaptive()
    ref = rg.make_reference(5, 400000)
    n_reads = 300
    req, rows, offs, tpos, txt, pats = engine.group_pairs(17, 0, n_reads, 8, 100, 0.02, ref, rs, sizes=[8] * n_reads)
    for r in range(n_reads):
        lo = int(offs[r])
        for j in range(0, 8, 2):
            tpos[lo + j + 1], txt[lo + j + 1] = tpos[lo + j], txt[lo + j]
    runs_cap = 16 * len(req)
    exp = expected(("ties",), "wfa", ms, rs, kw, req, pats, txt, offs, runs_cap=runs_cap)
    ph = engine.make_params("wfa", ms, rs, read_groups=True, ref_texts=True, top_hits=True, **kw)
    for max_hits in (2, 4, 8):
        got = run_hits(ph, max_hits, req, rows, offs, tpos=tpos, ref=ref, runs_cap=runs_cap)
        hoff, hit_pair = assert_hits_equal(got, exp, offs, max_hits, True, True)
        hp, sc = hit_pair.reshape(n_reads, max_hits).astype(np.int64), got["res"]["score"].reshape(n_reads, max_hits)
        assert (np.diff(sc, axis=1) >= 0).all()                              # rank order is score order ...
        assert (hp[:, 0::2] % 2 == 0).all() and (hp[:, 1::2] == hp[:, 0::2] + 1).all() and (sc[:, 1::2] == sc[:, 0::2]).all()   # ... twins adjacent, lower index first
        tied = np.diff(sc, axis=1) == 0
        assert (np.diff(hp, axis=1)[tied] > 0).all()


def test_packed_reads_over_two_slots():
    """Packed read rows (AIM_FLAG_REF_TEXTS): reads holding N or lowercase travel on the raw side list; both strands; compact runs;
    3 chunks over 2 slots."""
    import test_read_groups_gpu as rg
    from aim_amd import engine
    ms, rs, kw = _adaptive()
    ref = rg.make_reference(61, 300000)
    sizes = np.random.default_rng(61).integers(1, 24, size=400)
    req, rows, offs, tpos, txt, pats = engine.group_pairs(61, 0, 400, 8, 100, 0.02, ref, rs, sizes=sizes)
    rows[::7, 5] = ord("N")
    rows[3::11, 40] |= 0x20
    pats = np.ascontiguousarray(rows[np.repeat(np.arange(400), np.diff(offs))])
    _, ok = engine.pack_rows(req[offs[:-1]], rows, "pattern_len")
    assert (~ok).sum() >= 80 and (tpos >> np.uint64(63)).any() and not (tpos >> np.uint64(63)).all()
    runs_cap = 512 * len(req)
    exp = expected(("packed",), "wfa", ms, rs, kw, req, pats, txt, offs, runs_cap=runs_cap)
    got = run_hits(engine.make_params("wfa", ms, rs, read_groups=True, ref_texts=True, top_hits=True, **kw), 3, req, rows, offs, tpos=tpos, ref=ref,
                   runs_cap=runs_cap, slots=2, chunks=3, packed=True)
    assert got["plan"].endswith(" groups=1 hits=1")
    assert_hits_equal(got, exp, offs, 3, True, True)


def test_swg_int8_hit_aborts_in_the_cigar_pass():
    """int8 SWG: the score-only pass reports OK where the CIGAR pass of the same pair stops with AIM_PAIR_SWG_NO_OP
    (test_swg_int8_winner_aborts_in_the_cigar_pass's input). A hit row of such a candidate carries that status, and aim_set_wait returns
    AIM_EALIGN."""
    from aim_amd import capi, engine
    ms, rs, n = 40, 416, 300
    req, pat, txt = engine.gen_pairs(713, 0, n, 400, 0.02, rs)
    kw = dict(backtrace=True)
    res0, _ = engine.align(engine.make_params("swg", ms, rs, **kw), req, pat, txt, check=False)
    abort = set(np.nonzero(res0["status"] == capi.PAIR_SWG_NO_OP)[0].tolist())
    assert abort
    cand, sizes = [], []
    for i in range(n):       # read i: its own text, plus (unless its pair aborts) the texts of pairs i + 1 and i + 2
        own = [i] if i in abort else [i, (i + 1) % n, (i + 2) % n]
        cand += own
        sizes.append(len(own))
    cand = np.array(cand)
    read_of = np.repeat(np.arange(n), sizes)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    req2 = np.zeros(len(cand), dtype=capi.REQUEST_DTYPE)
    req2["pattern_len"], req2["text_len"], req2["idx"] = req["pattern_len"][read_of], req["text_len"][cand], np.arange(len(cand))
    txt2, pats2 = np.ascontiguousarray(txt[cand]), np.ascontiguousarray(pat[read_of])
    exp = expected(("swg-abort",), "swg", ms, rs, kw, req2, pats2, txt2, offs, runs_cap=512 * len(cand))
    ph = engine.make_params("swg", ms, rs, read_groups=True, top_hits=True, **kw)
    got = run_hits(ph, 2, req2, pat, offs, txt=txt2, runs_cap=512 * len(cand))
    hoff, hit_pair = assert_hits_equal(got, exp, offs, 2, True, True)
    aborted = np.nonzero(exp["res"]["status"][hit_pair] == capi.PAIR_SWG_NO_OP)[0]
    assert len(aborted) >= len(abort) and (exp["res1"]["status"][hit_pair[aborted]] == capi.PAIR_OK).all()
    assert (got["res"]["status"][aborted] == capi.PAIR_SWG_NO_OP).all() and (got["cig"]["n_runs"][aborted] == 0).all()
    with engine.DeviceSet(1) as s:
        s.configure_slots(ph, len(cand), slots=1)
        s.submit(0, 0, req2, pat=pat, txt=txt2, want_ops=True, read_offsets=offs, max_hits=2)
        with pytest.raises(capi.AimError) as e:
            s.wait(0, 0)
        assert e.value.code == capi.AIM_EALIGN


KNOB_CHILD = '''
import sys
import numpy as np
sys.path.insert(0, "tests")
import test_top_hits_gpu as t
np.savez(sys.argv[1], **t.knob_batch())
'''


def knob_batch():
    import test_read_groups_gpu as rg
    from aim_amd import engine
    ms, rs, kw = _adaptive()
    ref = rg.make_reference(41, 200000)
    sizes = np.random.default_rng(41).integers(1, 70, size=300)
    req, rows, offs, tpos, txt, pats = engine.group_pairs(41, 0, 300, 8, 100, 0.02, ref, rs, sizes=sizes)
    g = run_hits(engine.make_params("wfa", ms, rs, read_groups=True, ref_texts=True, top_hits=True, **kw), 4, req, rows, offs, tpos=tpos, ref=ref,
                 runs_cap=16 * len(req))
    ops = g["ops"].copy()                      # (outside [begin_offset, end_offset) a row is unspecified)
    cols = np.arange(ops.shape[1])[None, :]
    ops[(cols < g["res"]["begin_offset"][:, None]) | (cols >= g["res"]["end_offset"][:, None])] = 0
    return dict(best=g["best"], res=g["res"], hdr=rg._hdr(g["cig"]), runs=g["runs"], hit_pair=g["hit_pair"], hit_offsets=g["hit_offsets"], ops=ops)


@pytest.fixture(scope="module")
def knob_baseline():
    return knob_batch()


@pytest.mark.parametrize("env", [{"AIM_CHIP_CUS": "1", "AIM_DEBUG_POISON_SCRATCH": "165", "AIM_DEBUG_POISON_OPS": "77", "AIM_DEBUG_POISON_LDS": "90"},
                                 {"AIM_CHIP_CUS": "256"}], ids=["cus1-poison", "cus256"])
def test_knobs_do_not_change_results(tmp_path, knob_baseline, env):
    f = str(tmp_path / "k.npz")
    p = subprocess.run([sys.executable, "-c", KNOB_CHILD, f], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    out = np.load(f)
    for key, want in knob_baseline.items():
        assert np.array_equal(out[key], want), key


def test_wrong_hit_offsets_are_refused_before_anything_runs():
    import test_read_groups_gpu as rg
    from aim_amd import capi, engine
    ms, rs, kw = _adaptive()
    ref = rg.make_reference(3, 50000)
    req, rows, offs, tpos, txt, pats = engine.group_pairs(3, 0, 10, 4, 100, 0.02, ref, rs, sizes=[4, 1, 6, 2, 4, 4, 9, 1, 3, 4])
    ph = engine.make_params("wfa", ms, rs, read_groups=True, top_hits=True, **kw)
    good = engine.hits_offsets(offs, 3)
    with engine.DeviceSet(1) as s:
        s.configure_slots(ph, 64, slots=1, max_runs=4096)
        assert s.plan_describe(0).endswith(" groups=1 hits=1")
        for at, read in ((4, 4), (10, 9), (0, 0)):
            bad = good.copy()
            bad[at] += 1
            with pytest.raises(capi.AimError) as e:
                s.submit(0, 0, req, pat=rows, txt=txt, read_offsets=offs, cigar_runs_cap=4096, max_hits=3, hit_offsets=bad)
            assert e.value.code == capi.AIM_EINVAL and "AIM_FLAG_TOP_HITS" in str(e.value) and "read %d " % read in str(e.value), str(e.value)
            with pytest.raises(capi.AimError) as e:                  # nothing is in flight
                s.wait(0, 0)
            assert e.value.code == capi.AIM_ESTATE
        for call in (lambda: s.push(0, req, pats, txt), lambda: s.launch()):
            with pytest.raises(capi.AimError) as e:
                call()
            assert e.value.code == capi.AIM_EINVAL and "aim_batch_io_groups_t" in str(e.value)
        s.submit(0, 0, req, pat=rows, txt=txt, read_offsets=offs, cigar_runs_cap=4096, max_hits=3, hit_offsets=good)
        out = s.wait(0, 0)
        assert len(out["cig"]) == len(out["hit_pair"]) == int(good[-1])


ALIGN_DEVICE_HITS = '''
import sys
import torch
torch.cuda.init()   # (before the library: the device buffers are torch's)
sys.path.insert(0, "tests")
import test_top_hits_gpu as t
t.align_device_hits_torch()
print("ALIGN_DEVICE_HITS_OK")
'''


def test_align_device_hits_torch():
    p = subprocess.run([sys.executable, "-c", ALIGN_DEVICE_HITS], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ALIGN_DEVICE_HITS_OK" in p.stdout, p.stdout + p.stderr


def align_device_hits_torch():
    """aim_align_device_hits on torch tensors equals the submit path (and with it the flag-less runs), with and without d_hit_pair."""
    import test_read_groups_gpu as rg
    import torch
    from aim_amd import capi, engine
    lib = capi.load()
    dev = torch.device("cuda:0")
    ref = rg.make_reference(19, 100000)
    ms, rs = engine.launcher_sizes("wfa", 100, 0.02)
    sizes = np.random.default_rng(19).integers(1, 30, size=200)
    req, rows, offs, tpos, txt, pats = engine.group_pairs(19, 0, 200, 8, 100, 0.02, ref, rs, sizes=sizes)
    n, nr, max_hits = len(req), len(offs) - 1, 3
    hoff = engine.hits_offsets(offs, max_hits)
    nh = int(hoff[-1])
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    for use_ref, kw, keep_pair in ((False, dict(backtrace=True), True), (True, dict(backtrace=True, reduce=True), False), (True, dict(reduce=True, res8=True), True)):
        params = engine.make_params("wfa", ms, rs, read_groups=True, top_hits=True, ref_texts=use_ref, **kw)
        bt = bool(kw.get("backtrace"))
        d_req, d_rows, d_off, d_hoff = t(req), t(rows), t(offs), t(hoff)
        d_txt = None if use_ref else t(txt)
        d_tp = t(tpos) if use_ref else None
        d_ref = torch.zeros(len(ref) + 64, dtype=torch.uint8, device=dev)
        d_ref[: len(ref)] = torch.from_numpy(ref).to(dev)
        res_dt = capi.RESULT8_DTYPE if kw.get("res8") else capi.RESULT_DTYPE
        d_res = torch.zeros(nh * res_dt.itemsize, dtype=torch.uint8, device=dev)
        d_ops = torch.zeros(nh * 2 * rs, dtype=torch.uint8, device=dev) if bt else None
        d_best = torch.zeros(nr * 16, dtype=torch.uint8, device=dev)
        d_pair = torch.full((nh * 4,), 0xEE, dtype=torch.uint8, device=dev) if keep_pair else None
        sb = lib.aim_scratch_bytes(capi.params_ref(params), n)
        assert sb > 0
        d_scr = torch.zeros(sb, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ptr = lambda x: None if x is None else x.data_ptr()
        engine.align_device_hits(params, n, nr, ptr(d_req), ptr(d_rows), ptr(d_txt), ptr(d_tp), ptr(d_ref), len(ref), ptr(d_off), ptr(d_res),
                                 ptr(d_ops), ptr(d_best), max_hits, ptr(d_hoff), nh, ptr(d_pair), ptr(d_scr), sb)
        torch.cuda.synchronize()
        if use_ref:
            sub = run_hits(params, max_hits, req, rows, offs, tpos=tpos, ref=ref)
        else:
            sub = run_hits(params, max_hits, req, rows, offs, txt=txt)
        assert np.array_equal(d_best.cpu().numpy().view(capi.BEST_DTYPE), sub["best"])
        res = d_res.cpu().numpy().view(res_dt)
        assert np.array_equal(res, sub["res"])
        if keep_pair:
            assert np.array_equal(d_pair.cpu().numpy().view(np.uint32), sub["hit_pair"])
        if bt:
            ops = d_ops.cpu().numpy().reshape(nh, 2 * rs)
            for h in range(nh):
                lo, hi = int(res["begin_offset"][h]), int(res["end_offset"][h])
                assert np.array_equal(ops[h, lo:hi], sub["ops"][h, lo:hi]), h
        exp = expected(("torch", tuple(sorted(kw))), "wfa", ms, rs, kw, req, pats, txt, offs)
        assert_hits_equal(dict(sub, res=res), exp, offs, max_hits, False, False)
