"""Paired-end candidate selection (AIM_FLAG_MATE_PAIRS) on the GPU. Every case compares the device's sel (through the per-read rows),
mates, best and per-read rows with two things: the model (mate_pairs_model.py) run on the flag-less per-candidate score-only results of
the same batch, and the flag-less rows of sel[r] -- every result field, ops bytes in [begin_offset, end_offset), compact headers and runs.
Batches: WFA-adaptive l = 100 e = 1 % K = 8 with and without BACKTRACE, NW l = 150, WFA with over-cap decoys, packed read rows, compact
runs; K = 1, one read pair of 3 000 x 5 candidates, zero-width windows, min_span = max_span, penalty 0 and INT32_MAX; the stateless entry
point; AIM_CHIP_CUS = 1 / 256 and the poison knobs.

A mate without an AIM_PAIR_OK candidate: no score-only pass reports another status (the plans rule AIM_PAIR_NOMEM out and the other
statuses belong to the CIGAR pass), so no batch reaches that branch through the public entry points. test_hand_made_rows_at_every_lane_count
runs group_select_kernel and mate_select_kernel themselves (tests/csrc/select_harness.hip) on hand-made result rows of every status, and
sweeps the lanes per read pair W = 1 .. 64 over the same rows."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

INT32_MAX = 2 ** 31 - 1
UINT32_MAX = 2 ** 32 - 1
MINUS = 1 << 63
REPEAT_FRAC = 0.4
SPANS = (340, 460)          # insert 400 +- 10 %, widened by the edits a window may carry


def _kw_pass1(kw):
    return {k: v for k, v in kw.items() if k not in ("backtrace", "bidir", "res8")}


def expected(algo, ms, rs, kw, req, pats, txt, offs, tpos, mates, runs_cap=0):
    """The flag-less runs of every candidate: the model on the score-only pass, and the configured run's outputs."""
    import mate_pairs_model as mm
    from aim_amd import engine
    res1, _ = engine.align(engine.make_params(algo, ms, rs, **_kw_pass1(kw)), req, pats, txt, check=False)
    sel, rows, best = mm.select(res1["score"], res1["status"], tpos, req["text_len"], offs, *mates)
    out = {"sel": sel, "mates": rows, "best": best, "res1": res1}
    with engine.DeviceSet(1) as s:
        s.configure_slots(engine.make_params(algo, ms, rs, **kw), len(req), slots=1, max_runs=runs_cap)
        s.submit(0, 0, req, pat=pats, txt=txt, want_ops=bool(kw.get("backtrace")), cigar_runs_cap=runs_cap)
        out.update(s.wait(0, 0, check=False))
    return out


def run_mates(params, req, rows, offs, tpos, ref, mates, runs_cap=0, slots=1, chunks=1, packed=False):
    """aim_set_submit of the mate-pairs batch, split at read-pair boundaries into `chunks` batches over `slots` slots; outputs
    concatenated, candidate indices made batch-wide again."""
    from aim_amd import engine
    n_reads = len(offs) - 1
    read_req = req[offs[:-1]]
    bounds = 2 * np.linspace(0, n_reads // 2, chunks + 1).astype(int)
    bt = bool(params.flags & 1)
    got, pending = [], []
    with engine.DeviceSet(1) as s:
        s.configure_slots(params, len(req), slots=slots, max_runs=runs_cap, max_raw=n_reads if packed else 0)
        s.set_reference(ref)
        for c in range(chunks):
            r0, r1 = int(bounds[c]), int(bounds[c + 1])
            c0, c1 = int(offs[r0]), int(offs[r1])
            kw = dict(want_ops=bt, cigar_runs_cap=runs_cap, read_offsets=offs[r0:r1 + 1] - offs[r0], text_pos=tpos[c0:c1], mates=mates)
            if packed:
                kw["packed"] = engine.pack_batch(read_req[r0:r1], rows[r0:r1], None)
            else:
                kw["pat"] = rows[r0:r1]
            if len(pending) == slots:
                pc, pc0 = pending.pop(0)
                got.append((pc0, s.wait(0, pc % slots, check=False)))
            s.submit(0, c % slots, req[c0:c1], **kw)
            pending.append((c, c0))
        for pc, pc0 in pending:
            got.append((pc0, s.wait(0, pc % slots, check=False)))
        plan = s.plan_describe(0)
    out = {"plan": plan}
    for key in ("best", "mates", "res", "ops", "cig"):
        if key in got[0][1]:
            parts = []
            for c0, g in got:
                x = g[key].copy()
                if key in ("best", "mates"):
                    x["best_pair"] = np.where(x["best_pair"] != UINT32_MAX, x["best_pair"] + np.uint32(c0), x["best_pair"])
                parts.append(x)
            out[key] = np.concatenate(parts)
    if "cig" in out:
        import test_read_groups_gpu as g
        out["runs"] = np.concatenate([g._runs_in_order(x["cig"], x["runs"]) for _, x in got])
    return out


def assert_mates_equal(got, exp, bt, runs):
    """mates and best against the model; the per-read rows against the flag-less rows of the model's sel (test_read_groups_gpu's
    comparison: every result field, ops[begin, end), compact headers and runs)."""
    import test_read_groups_gpu as g
    assert np.array_equal(got["mates"], exp["mates"]), np.nonzero(got["mates"] != exp["mates"])[0][:8]
    assert not got["mates"]["pad"].any()
    g.assert_groups_equal(got, exp, bt, runs)        # (exp["best"]: the independent selection; exp["sel"]: the paired one)


def _differs(exp):
    """Read pairs whose choice is proper and differs from READ_GROUPS' own selection."""
    ind = exp["best"]["best_pair"].reshape(-1, 2)
    return ((exp["mates"]["flags"] & 1) != 0) & (exp["sel"].reshape(-1, 2) != ind).any(axis=1)


# (algo, length, error, read pairs, K, make_params keywords, packed, chunks)
CASES = [
    ("wfa", 100, 0.01, 400, 8, dict(reduce=True, backtrace=True, req8=True), False, 1),
    ("wfa", 100, 0.01, 400, 8, dict(reduce=True), False, 1),
    ("wfa", 100, 0.01, 400, 8, dict(reduce=True, res8=True, req8=True), False, 1),
    ("nw", 150, 0.02, 200, 6, dict(backtrace=True), False, 1),
    ("wfa", 100, 0.01, 300, 8, dict(backtrace=True), False, 1),
    ("wfa", 100, 0.01, 400, 8, dict(reduce=True, backtrace=True, req8=True), True, 3),
    ("wfa", 100, 0.01, 300, 4, dict(backtrace=True), True, 2),
]


@pytest.mark.parametrize("algo,length,error,n_mates,k,kw,packed,chunks", CASES,
                         ids=["%s-l%d-K%d-%s%s" % (c[0], c[1], c[4], "-".join(sorted(c[5])), "-packed" if c[6] else "") for c in CASES])
def test_mates_equal_model_and_flagless(algo, length, error, n_mates, k, kw, packed, chunks):
    from aim_amd import engine
    ms, rs = engine.launcher_sizes(algo, length, error)
    ref, req, rows, offs, tpos, txt, pats, truth = engine.mate_pairs(length + k, n_mates, length, error, 400, k, REPEAT_FRAC, read_size=rs)
    if packed:                                        # reads holding N or lowercase travel on the raw side list
        rows[::7, 5] = ord("N")
        rows[3::11, 40] |= 0x20
        pats = np.ascontiguousarray(np.repeat(rows, k, axis=0))
    bt = bool(kw.get("backtrace"))
    runs_cap = 64 * len(req) if bt else 0
    mates = (SPANS[0], SPANS[1], 2 * (ms + 1) if algo == "wfa" else 40)
    exp = expected(algo, ms, rs, kw, req, pats, txt, offs, tpos, mates, runs_cap=runs_cap)
    pm = engine.make_params(algo, ms, rs, read_groups=True, ref_texts=True, mate_pairs=True, **kw)
    got = run_mates(pm, req, rows, offs, tpos, ref, mates, runs_cap=runs_cap, slots=2 if chunks > 1 else 1, chunks=chunks, packed=packed)
    assert got["plan"].endswith(" groups=1 mates=1")
    assert_mates_equal(got, exp, bt, bool(runs_cap))
    proper = (exp["mates"]["flags"] & 1) != 0
    n_diff = int(_differs(exp).sum())
    print("%d read pairs: proper %d, different from the independent winners %d, unpaired %d" % (n_mates, proper.sum(), n_diff, (~proper).sum()))
    # the repeat case: the mate changes the selection, and the rows that come back are the paired choice's, not READ_GROUPS' own
    assert n_diff >= n_mates // 10 and (~proper).any()
    ind = exp["best"]["best_pair"]
    moved = np.nonzero(exp["sel"] != ind)[0]
    if "res" in got and "idx" in got["res"].dtype.names:
        assert (got["res"]["idx"][moved] == exp["sel"][moved]).all() and (got["res"]["idx"][moved] != ind[moved]).all()
    if algo == "wfa" and not kw.get("reduce"):
        assert (exp["res1"]["score"] == ms + 1).any()          # over-cap decoys count with MAX_SCORE + 1


def _adaptive():
    from aim_amd import engine
    ms, rs = engine.launcher_sizes("wfa", 100, 0.01)
    return ms, rs, dict(reduce=True, backtrace=True, req8=True)


@pytest.mark.parametrize("mates", [(400, 400, 10), (340, 460, 0), (340, 460, INT32_MAX), (0, (1 << 62) - 1, 0), (0, 0, 3)],
                         ids=["span-exact", "penalty0", "penalty-max", "span-any", "span-zero"])
def test_pairing_parameters(mates):
    from aim_amd import engine
    ms, rs, kw = _adaptive()
    ref, req, rows, offs, tpos, txt, pats, truth = engine.mate_pairs(23, 300, 100, 0.01, 400, 8, REPEAT_FRAC, read_size=rs)
    exp = expected("wfa", ms, rs, kw, req, pats, txt, offs, tpos, mates, runs_cap=16 * len(req))
    got = run_mates(engine.make_params("wfa", ms, rs, read_groups=True, ref_texts=True, mate_pairs=True, **kw), req, rows, offs, tpos, ref, mates,
                    runs_cap=16 * len(req))
    assert_mates_equal(got, exp, True, True)
    proper = (exp["mates"]["flags"] & 1) != 0
    if mates[:2] == (400, 400):
        assert proper.any() and (~proper).sum() > 30          # only fragments of exactly 400 bases pair
    if mates[2] == INT32_MAX:
        assert (exp["mates"]["score_sum"][~proper] == INT32_MAX - 1).all() and (~proper).any()
    if mates[:2] == (0, 0):
        assert not proper.any()


def test_one_candidate_per_read():
    from aim_amd import engine
    ms, rs, kw = _adaptive()
    ref, req, rows, offs, tpos, txt, pats, truth = engine.mate_pairs(29, 500, 100, 0.01, 400, 1, REPEAT_FRAC, read_size=rs)
    mates = (SPANS[0], SPANS[1], 5)
    exp = expected("wfa", ms, rs, kw, req, pats, txt, offs, tpos, mates, runs_cap=16 * len(req))
    got = run_mates(engine.make_params("wfa", ms, rs, read_groups=True, ref_texts=True, mate_pairs=True, **kw), req, rows, offs, tpos, ref, mates,
                    runs_cap=16 * len(req))
    assert_mates_equal(got, exp, True, True)
    assert np.array_equal(exp["sel"], np.arange(len(req))) and np.array_equal(got["res"], exp["res"])
    proper = (exp["mates"]["flags"] & 1) != 0
    assert proper.any() and (~proper).any() and (exp["mates"]["n_best"][proper] == 1).all()


def _big_pair(seed, k_big, rs):
    """One read pair of k_big x 5 candidates (several chunks of combinations for any lane count) followed by ordinary read pairs of
    5 x 5: read 0 keeps its 5 generated candidates and gains seeded decoys -- copies of its true window moved by up to 40 bases, some
    on the other strand, and exact duplicates of the true window (ties)."""
    from aim_amd import capi, engine
    ref, req, rows, offs, tpos, txt, pats, truth = engine.mate_pairs(seed, 6, 100, 0.01, 400, 5, 1.0, read_size=rs)
    rng = np.random.default_rng([seed, 0x626967])
    true = int(tpos[truth["true"][0, 0]])
    pos, minus = true & (MINUS - 1), true & MINUS
    extra = np.zeros(k_big - 5, dtype=np.uint64)
    for i in range(len(extra)):
        u = rng.random()
        p = pos if u < 0.02 else min(max(pos + int(rng.integers(-40, 41)), 0), len(ref) - 100)
        extra[i] = p | (minus ^ (MINUS if 0.5 < u < 0.6 else 0))
    tpos2 = np.concatenate([tpos[:5], extra, tpos[5:]])
    n = len(tpos2)
    req2 = np.zeros(n, dtype=capi.REQUEST_DTYPE)
    req2["text_len"], req2["idx"] = 100, np.arange(n)
    offs2 = np.concatenate([[0], offs[1:].astype(np.int64) + len(extra)]).astype(np.uint32)
    read_of = np.repeat(np.arange(12), np.diff(offs2))
    req2["pattern_len"] = req["pattern_len"][offs[:-1]][read_of]
    txt2 = np.zeros((n, rs), dtype=np.uint8)
    for c in range(n):
        tp = int(tpos2[c])
        txt2[c, :100] = engine.ref_window(ref, tp & (MINUS - 1), 100, bool(tp >> 63))
    return ref, req2, rows, offs2, tpos2, txt2, np.ascontiguousarray(rows[read_of])


def test_one_read_pair_of_3000_by_5():
    from aim_amd import engine
    ms, rs, kw = _adaptive()
    ref, req, rows, offs, tpos, txt, pats = _big_pair(37, 3000, rs)
    assert offs[1] == 3000 and offs[2] == 3005
    mates = (SPANS[0], SPANS[1], 2 * (ms + 1))
    exp = expected("wfa", ms, rs, kw, req, pats, txt, offs, tpos, mates, runs_cap=16 * len(req))
    got = run_mates(engine.make_params("wfa", ms, rs, read_groups=True, ref_texts=True, mate_pairs=True, **kw), req, rows, offs, tpos, ref, mates,
                    runs_cap=16 * len(req))
    assert_mates_equal(got, exp, True, True)
    big = exp["mates"][0]
    assert big["flags"] & 1 and big["n_best"] >= 2 and big["second_sum"] == big["score_sum"]      # the duplicated true windows tie


def test_zero_width_windows():
    """text_len 0 is a valid window: it spans [start, start) and pairs by its start alone."""
    from aim_amd import engine
    ms, rs = engine.launcher_sizes("nw", 100, 0.02)
    kw = dict(backtrace=True)
    ref, req, rows, offs, tpos, txt, pats, truth = engine.mate_pairs(41, 120, 100, 0.02, 400, 4, REPEAT_FRAC, read_size=rs)
    zero = np.arange(len(req)) % 5 == 2
    req["text_len"][zero] = 0
    txt[zero] = 0
    mates = (240, 460, 10 ** 6)        # (a zero-width minus-strand window ends 100 bases early)
    exp = expected("nw", ms, rs, kw, req, pats, txt, offs, tpos, mates, runs_cap=64 * len(req))
    got = run_mates(engine.make_params("nw", ms, rs, read_groups=True, ref_texts=True, mate_pairs=True, **kw), req, rows, offs, tpos, ref, mates,
                    runs_cap=64 * len(req))
    assert_mates_equal(got, exp, True, True)
    assert zero[exp["sel"]].any() and ((exp["mates"]["flags"] & 1) != 0).any()


def test_refusals_on_a_set():
    from aim_amd import capi, engine
    ms, rs, kw = _adaptive()
    ref, req, rows, offs, tpos, txt, pats, truth = engine.mate_pairs(3, 6, 100, 0.01, 400, 4, REPEAT_FRAC, read_size=rs)
    pm = engine.make_params("wfa", ms, rs, read_groups=True, ref_texts=True, mate_pairs=True, **kw)
    with engine.DeviceSet(1) as s:
        for flags in (0x2000, 0x2000 | 0x800, 0x2000 | 0x400):
            bad = capi.Params(capi.ALGO_WFA, 0, 3, 4, 1, 4, 4, ms, rs, flags)
            with pytest.raises(capi.AimError) as e:
                s.configure_slots(bad, 64, slots=1)
            assert e.value.code == capi.AIM_EINVAL and "AIM_FLAG_MATE_PAIRS needs AIM_FLAG_" in str(e.value)
        s.configure_slots(pm, 64, slots=1, max_runs=1024)
        s.set_reference(ref)
        with pytest.raises(capi.AimError) as e:                  # (aim_set_push refuses AIM_FLAG_REF_TEXTS before it looks further)
            s.push(0, req, pats, txt)
        assert e.value.code == capi.AIM_EINVAL and "aim_set_push_ref" in str(e.value)
        for call in (lambda: s.push(0, req, pats, text_pos=tpos), lambda: s.launch(), lambda: capi.check(s.lib.aim_set_pull(s.handle, 0, None, None))):
            with pytest.raises(capi.AimError) as e:
                call()
            assert e.value.code == capi.AIM_EINVAL and "aim_batch_io_groups_t" in str(e.value)
        for sub, words in ((dict(read_offsets=offs[:-1], n=int(offs[-2])), "is odd"), (dict(mates=(10, 9, 0)), "bad span [10, 9]"),
                           (dict(mates=(0, 1 << 62, 0)), "bad span"), (dict(mates=(0, 500, -1)), "unpaired_penalty -1 is negative")):
            n = sub.pop("n", len(req))
            args = dict(read_offsets=offs, mates=(340, 460, 5))
            args.update(sub)
            with pytest.raises(capi.AimError) as e:
                s.submit(0, 0, req[:n], pat=rows[:len(args["read_offsets"]) - 1], text_pos=tpos[:n], cigar_runs_cap=1024, **args)
            assert e.value.code == capi.AIM_EINVAL and words in str(e.value), str(e.value)
        with pytest.raises(capi.AimError) as e:                  # nothing is in flight after the refusals
            s.wait(0, 0)
        assert e.value.code == capi.AIM_ESTATE
        s.submit(0, 0, req, pat=rows, text_pos=tpos, cigar_runs_cap=1024, read_offsets=offs, mates=(340, 460, 5))
        out = s.wait(0, 0)
        assert len(out["mates"]) == 6 and len(out["best"]) == 12


def _hand_made_rows(seed):
    """151 read pairs of K = 1 .. 9 candidates (read pair 0: 200 x 3, several chunks at every W) with scores 0 .. 5 (ties), a few near
    INT32_MAX (clamped sums), every status, both strands, starts within 400 bases and text_len 0 / 90 / 100 / 110. Every 7th read, both
    reads of read pair 10 and whichever short read the draw leaves so have no OK candidate."""
    from aim_amd import capi
    rng = np.random.default_rng([seed, 0x68616e64])
    ks = rng.integers(1, 10, size=302)
    ks[0], ks[1] = 200, 3
    offs = np.concatenate([[0], np.cumsum(ks)]).astype(np.uint32)
    n, nr = int(offs[-1]), len(ks)
    read_of = np.repeat(np.arange(nr), ks)
    dead = np.zeros(nr, dtype=bool)
    dead[5::7] = True
    dead[20] = dead[21] = True
    res = np.zeros(n, dtype=capi.RESULT_DTYPE)
    res["score"] = rng.integers(0, 6, size=n)
    res["score"][rng.random(n) < 0.02] = INT32_MAX - 2
    res["status"] = np.where(rng.random(n) < 0.7, capi.PAIR_OK, rng.integers(1, 4, size=n))
    res["status"][dead[read_of] & (res["status"] == capi.PAIR_OK)] = capi.PAIR_NOMEM
    res["idx"] = np.arange(n)
    req = np.zeros(n, dtype=capi.REQUEST_DTYPE)
    req["pattern_len"], req["idx"] = 100, np.arange(n)
    req["text_len"] = rng.choice([0, 90, 100, 110], size=n)
    tpos = rng.integers(1000, 1400, size=n).astype(np.uint64) | np.where(rng.random(n) < 0.5, np.uint64(MINUS), np.uint64(0))
    return res, req, tpos, offs


def _select_harness():
    from aim_amd import build
    path = build.test_helper("select_harness")
    if not os.path.exists(path):
        pytest.fail("%s is missing: run the build" % path)
    fn = C.CDLL(path).select_harness_run
    fn.restype = C.c_int
    fn.argtypes = [C.c_uint32, C.c_uint32] + [C.c_void_p] * 4 + [C.c_int64, C.c_int64, C.c_int32, C.c_uint32] + [C.c_void_p] * 3
    return fn


def test_hand_made_rows_at_every_lane_count():
    """The selection kernels on rows no score-only pass produces, against the model; the rows do not depend on W. A mate without an OK
    candidate: best_pair UINT32_MAX, score_sum INT32_MAX, flags 0, sel = read_offsets[r]; the other mate keeps its independent winner."""
    import mate_pairs_model as mm
    from aim_amd import capi
    run = _select_harness()
    res, req, tpos, offs = _hand_made_rows(47)
    n, nr = len(res), len(offs) - 1
    mates = (80, 300, 4)
    sel, rows, best = mm.select(res["score"], res["status"], tpos, req["text_len"], offs, *mates)
    # what the batch holds: every outcome, ties, a clamped sum, and the reads without an OK candidate
    proper = (rows["flags"] & 1) != 0
    dead = best["n_best"] == 0
    none = dead.reshape(-1, 2)
    assert none.all(axis=1).any() and (none[:, 0] & ~none[:, 1]).any() and (~none[:, 0] & none[:, 1]).any()
    assert proper.any() and (~proper & ~none.any(axis=1)).any() and (rows["n_best"] > 1).any() and (rows["score_sum"] == INT32_MAX - 1).any()
    assert (proper & (sel.reshape(-1, 2) != best["best_pair"].reshape(-1, 2)).any(axis=1)).any()
    for m in np.nonzero(none.any(axis=1))[0]:
        assert rows["score_sum"][m] == INT32_MAX and rows["second_sum"][m] == INT32_MAX and rows["flags"][m] == 0 and rows["n_best"][m] == 0
        for r in (2 * m, 2 * m + 1):
            assert rows["best_pair"][m][r & 1] == (UINT32_MAX if dead[r] else best["best_pair"][r])
            assert sel[r] == (offs[r] if dead[r] else best["best_pair"][r])
    for lanes in (1, 2, 4, 8, 16, 32, 64):
        g_best, g_sel, g_rows = np.zeros(nr, dtype=capi.BEST_DTYPE), np.zeros(nr, dtype=np.uint32), np.zeros(nr // 2, dtype=capi.MATE_DTYPE)
        rc = run(n, nr, capi.ptr(res), capi.ptr(req), capi.ptr(tpos), capi.ptr(offs), *mates, lanes, capi.ptr(g_best), capi.ptr(g_sel), capi.ptr(g_rows))
        assert rc == 0, (lanes, rc)
        assert np.array_equal(g_best, best), lanes
        assert np.array_equal(g_rows, rows), (lanes, np.nonzero(g_rows != rows)[0][:8])
        assert np.array_equal(g_sel, sel), (lanes, np.nonzero(g_sel != sel)[0][:8])


KNOB_CHILD = '''
import sys
import numpy as np
sys.path.insert(0, "tests")
import test_mate_pairs_gpu as t
from aim_amd import engine
ms, rs, kw = t._adaptive()
ref, req, rows, offs, tpos, txt, pats = t._big_pair(43, 700, rs)
more = engine.mate_pairs(43, 200, 100, 0.01, 400, 8, t.REPEAT_FRAC, read_size=rs)
pm = engine.make_params("wfa", ms, rs, read_groups=True, ref_texts=True, mate_pairs=True, **kw)
a = t.run_mates(pm, req, rows, offs, tpos, ref, (340, 460, 12), runs_cap=16 * len(req))
b = t.run_mates(pm, more[1], more[2], more[3], more[4], more[0], (340, 460, 12), runs_cap=16 * len(more[1]), slots=2, chunks=3)
np.savez(sys.argv[1], **{k + "_a": a[k] for k in ("best", "mates", "res", "cig", "runs")}, **{k + "_b": b[k] for k in ("best", "mates", "res", "cig", "runs")})
'''


def test_knobs_do_not_change_results(tmp_path):
    import test_read_groups_gpu as g
    outs = []
    for i, env in enumerate(({}, {"AIM_CHIP_CUS": "1"}, {"AIM_CHIP_CUS": "256", "AIM_DEBUG_POISON_SCRATCH": "165", "AIM_DEBUG_POISON_OPS": "77",
                                                        "AIM_DEBUG_POISON_LDS": "90"})):
        f = str(tmp_path / ("k%d.npz" % i))
        p = subprocess.run([sys.executable, "-c", KNOB_CHILD, f], cwd=ROOT, env=dict(os.environ, **env), capture_output=True, text=True,
                           timeout=300)
        assert p.returncode == 0, p.stdout + p.stderr
        outs.append(np.load(f))
    for o in outs[1:]:
        for key in ("best_a", "mates_a", "res_a", "runs_a", "best_b", "mates_b", "res_b", "runs_b"):
            assert np.array_equal(outs[0][key], o[key]), key
        for key in ("cig_a", "cig_b"):
            assert np.array_equal(g._hdr(outs[0][key]), g._hdr(o[key]))
    assert (outs[0]["mates_b"]["flags"] & 1).any() and not (outs[0]["mates_b"]["flags"] & 1).all()


ALIGN_DEVICE_MATES = '''
import sys
import torch
torch.cuda.init()   # (before the library: the device buffers are torch's)
sys.path.insert(0, "tests")
import test_mate_pairs_gpu as t
t.align_device_mates_torch()
print("ALIGN_DEVICE_MATES_OK")
'''


def test_align_device_mates_agrees_with_submit():
    p = subprocess.run([sys.executable, "-c", ALIGN_DEVICE_MATES], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "ALIGN_DEVICE_MATES_OK" in p.stdout, p.stdout + p.stderr


def align_device_mates_torch():
    import torch
    from aim_amd import capi, engine
    lib = capi.load()
    dev = torch.device("cuda:0")
    ms, rs = engine.launcher_sizes("wfa", 100, 0.01)
    ref, req, rows, offs, tpos, txt, pats, truth = engine.mate_pairs(19, 200, 100, 0.01, 400, 8, REPEAT_FRAC, read_size=rs)
    n, nr = len(req), len(offs) - 1
    mates = (SPANS[0], SPANS[1], 2 * (ms + 1))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    for kw, keep_best in ((dict(backtrace=True, reduce=True), True), (dict(backtrace=True), False), (dict(reduce=True, res8=True), False)):
        params = engine.make_params("wfa", ms, rs, read_groups=True, ref_texts=True, mate_pairs=True, **kw)
        bt = bool(kw.get("backtrace"))
        d_req, d_rows, d_off, d_tp = t(req), t(rows), t(offs), t(tpos)
        d_ref = torch.zeros(len(ref) + 64, dtype=torch.uint8, device=dev)
        d_ref[: len(ref)] = torch.from_numpy(ref).to(dev)
        res_dt = capi.RESULT8_DTYPE if kw.get("res8") else capi.RESULT_DTYPE
        d_res = torch.zeros(nr * res_dt.itemsize, dtype=torch.uint8, device=dev)
        d_ops = torch.zeros(nr * 2 * rs, dtype=torch.uint8, device=dev) if bt else None
        d_best = torch.zeros(nr * 16, dtype=torch.uint8, device=dev) if keep_best else None     # NULL: the library keeps a scratch copy
        d_mates = torch.zeros((nr // 2) * 32, dtype=torch.uint8, device=dev)
        sb = lib.aim_scratch_bytes(capi.params_ref(params), n)
        assert sb > 0
        d_scr = torch.full((sb,), 0xA5, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        ptr = lambda x: None if x is None else x.data_ptr()
        engine.align_device_mates(params, n, nr, ptr(d_req), ptr(d_rows), ptr(d_tp), ptr(d_ref), len(ref), ptr(d_off), ptr(d_res), ptr(d_ops),
                                  ptr(d_best), mates, ptr(d_mates), ptr(d_scr), sb)
        torch.cuda.synchronize()
        exp = expected("wfa", ms, rs, kw, req, pats, txt, offs, tpos, mates)
        got = {"mates": d_mates.cpu().numpy().view(capi.MATE_DTYPE), "res": d_res.cpu().numpy().view(res_dt),
               "best": d_best.cpu().numpy().view(capi.BEST_DTYPE) if keep_best else exp["best"]}
        if bt:
            got["ops"] = d_ops.cpu().numpy().reshape(nr, 2 * rs)
        assert_mates_equal(got, exp, bt, False)
        sub = run_mates(params, req, rows, offs, tpos, ref, mates)          # ... and the same rows as aim_set_submit gives
        assert np.array_equal(sub["mates"], got["mates"]) and np.array_equal(sub["res"], got["res"])
        if keep_best:
            assert np.array_equal(sub["best"], got["best"])
        assert _differs(exp).any()
