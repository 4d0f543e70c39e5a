"""Low-complexity inputs (tests/low_complexity.py) on the GPU: homopolymers, tandem repeats, two-letter sequence and runs of 'N' on
every kernel shape of the full-row table and on the MAX_SCORE 10 lane rows, against the oracle pair by pair; the flagged WFA modes
against their models; the packed / compact transports, SAM_FIELDS and the planner's other routes, which must change nothing.
tests/test_low_complexity_cpu.py holds the oracle to independent models on the same batches first, and shows that they tell the
traceback tie orders apart. One process; knobs are set around each DeviceSet."""
import numpy as np
import pytest

import full_rows as F
import low_complexity as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(built):
    import ctypes as C
    from aim_amd import capi
    lib = capi.load()
    n = C.c_int()
    assert lib.aim_device_count(C.byref(n)) == 0 and n.value >= 1, lib.aim_last_error()
    return lib


def _row_against_the_oracle(fam, rs, pad):
    from aim_amd import capi
    req = L.row_batch(fam, rs, pad)[0]
    res, ops, line, todo = L.align_row(fam, rs, pad)
    print("%s/%d %s: %s; to-do list %d of %d pairs" % (fam, rs, pad, line, todo, len(req)))
    assert F.plan_matches(line, L.expected_plan(fam, rs)), line
    ores, oops = L.oracle_row(fam, rs, pad)
    F.compare(res, ops, ores, oops, req, bool(L.row_params(fam, rs).flags & capi.FLAG_BACKTRACE))


@pytest.mark.parametrize("fam,rs", L.ROWS, ids=lambda v: str(v))
def test_low_complexity_rows_match_the_oracle(gpu, fam, rs):
    """Every pair of the row's low-complexity batch, the ones over the cap included: score, max_operations, end_offset and
    status, and with CIGAR begin_offset and the ops bytes of [begin_offset, end_offset); the plan line names the row's kernel
    and shape. The to-do list's count is printed, not pinned: these batches send more walks off the register kernels' band
    than random data does."""
    _row_against_the_oracle(fam, rs, "zero")


def _first_rows_by_kernel():
    first = {}
    for fam, rs in L.ROWS:
        first.setdefault(L.expected_plan(fam, rs).split()[0], (fam, rs))
    return first


NOISE_ROWS = _first_rows_by_kernel()


def test_noise_rows_cover_every_kernel_a_row_reaches():
    """wfa_bidir_kernel is reached through its flag only: the BIDIR feature rows below run it."""
    assert set(NOISE_ROWS) == set(F.KERNEL_NAMES) - {"wfa_bidir_kernel"}


@pytest.mark.parametrize("fam,rs", sorted(NOISE_ROWS.values()), ids=lambda v: str(v))
def test_low_complexity_rows_with_noise_padding(gpu, fam, rs):
    """The first row of each kernel with seeded A/C/G/T/N behind every length instead of zeros."""
    _row_against_the_oracle(fam, rs, "noise")


# ------------------------------------------------------------------ feature rows
def _cigars(req, pat, txt, res, ops, rescore, check_cigar):
    for i in range(len(req)):
        p, t = bytes(pat[i, :req["pattern_len"][i]]), bytes(txt[i, :req["text_len"][i]])
        s = bytes(ops[i, int(res["begin_offset"][i]):int(res["end_offset"][i])]).decode()
        assert res["max_operations"][i] == len(p) + len(t)
        assert check_cigar(s, p, t) is None, (i, s)
        assert rescore(s, len(p), len(t)) == res["score"][i], (i, s)


def _inner_patterns(req, pat, cut):
    """Every pattern without its first and last `cut` bases (where it is long enough): the text then carries flanks that continue
    the pattern's own repeat, so under free text ends every placement of the pattern along the repeat is a tie."""
    req, out = req.copy(), np.zeros_like(pat)
    for i in range(len(req)):
        pl = int(req["pattern_len"][i])
        c = cut if pl > 4 * cut else 0
        out[i, :pl - 2 * c] = pat[i, c:pl - c]
        req["pattern_len"][i] = pl - 2 * c
    return req, out


FEATURE_ROWS = [(f, rs) for f in F.FEATURES for rs in (112, 1024)]      # (full_rows.FEATURE_ROWS plus WFA_W32 at READ_SIZE 112)


@pytest.mark.parametrize("feature,rs", FEATURE_ROWS, ids=lambda v: str(v))
def test_feature_rows_match_their_models(gpu, feature, rs):
    """ENDSFREE, AFFINE2P, LINEAR and WFA_BIDIR on one light and one heavy pair of each class, every pair under the cap: scores
    equal the flag's own model and the CIGARs re-score to them. WFA_W32 gives the flag-less bytes, WFA_BIDIR the flag-less
    score, status, max_operations and end_offset."""
    import affine2p_model, endsfree_model, linear_model
    from aim_amd import engine
    req, pat, txt, cls, light = L.one_of_each(rs, L.SEED)
    assert len(req) == 18 and light.sum() == 9
    if feature == "endsfree":
        req, pat = _inner_patterns(req, pat, 8)
    params = F.feature_params(feature, rs)
    res, ops = engine.align(params, req, pat, txt)
    sres, _ = engine.align(F.feature_params(feature, rs, backtrace=feature == "bidir"), req, pat, txt)
    assert (res["status"] == 0).all() and np.array_equal(sres["score"], res["score"])
    if feature == "endsfree":
        ef = F.FEATURES["endsfree"]["ends_free"]
        want = endsfree_model.dp_scores(req, pat, txt, ends_free=ef)
        assert np.array_equal(res["score"], want)
        assert (want[light] <= 5).all() and (want == 0).sum() >= 4          # a placement along the repeat costs nothing
        _cigars(req, pat, txt, res, ops, lambda s, pl, tl: endsfree_model.rescore(s, pl, tl, ends_free=ef), endsfree_model.check_cigar)
    elif feature == "affine2p":
        assert np.array_equal(res["score"], affine2p_model.dp_scores(req, pat, txt, o2=24, e2=1))
        _cigars(req, pat, txt, res, ops, lambda s, pl, tl: affine2p_model.rescore(s, o2=24, e2=1), affine2p_model.check_cigar)
    elif feature == "linear":
        assert np.array_equal(res["score"], linear_model.dp_scores(req, pat, txt, x=2, g=3))
        assert np.array_equal(res["score"], F.nw_model(req, pat, txt, 2, 3, 3))
        _cigars(req, pat, txt, res, ops, lambda s, pl, tl: linear_model.rescore(s, x=2, g=3), linear_model.check_cigar)
    else:
        plain = engine.make_params("wfa", params.max_score, rs, backtrace=True)
        bres, bops = engine.align(plain, req, pat, txt)
        ores, oops, _ = L.oracle_of(plain, "wfa", req, pat, txt)
        F.compare(bres, bops, ores, oops, req, True)
        assert np.array_equal(res["score"], F.affine_model(req, pat, txt))
        if feature == "w32":
            F.compare(res, ops, ores, oops, req, True)
        else:
            for f in ("score", "status", "max_operations", "end_offset"):
                assert np.array_equal(res[f], bres[f]), f
            _cigars(req, pat, txt, res, ops, lambda s, pl, tl: endsfree_model.rescore(s, pl, tl), endsfree_model.check_cigar)


# ------------------------------------------------------------------ transports
TRANSPORT = [("wfa5_bt", 112), ("wfa10_bt", 136), ("wfa2_red_bt", 320), ("nw_bt", 176), ("swg16_bt", 1024), ("wfa18_254_bt", 112)]


@pytest.mark.parametrize("fam,rs", TRANSPORT, ids=lambda v: str(v))
def test_packed_input_and_compact_runs(gpu, fam, rs):
    """aim_set_submit with 2-bit packed rows (every n_run pair travels raw) and device-side run lists: results equal the
    oracle's, and the run lists print the CIGAR the ops rows print."""
    from aim_amd import engine
    req, pat, txt, cls, _ = L.row_batch(fam, rs, "noise")
    n = len(req)
    params = L.row_params(fam, rs)
    ores, oops = L.oracle_row(fam, rs, "noise")
    packed = engine.pack_batch(req, pat, txt)
    assert packed[2].tolist() == np.nonzero(cls == L.CLASSES.index("n_run"))[0].tolist()
    with engine.DeviceSet(1) as s:
        s.configure_slots(params, n, slots=2, max_raw=n, max_runs=n * 2 * rs)
        s.submit(0, 0, req, packed=packed, want_ops=True)
        out = s.wait(0, 0, check=False)
        F.compare(out["res"], out["ops"], ores, oops, req, True)
        want = engine.format_output(out["res"], out["ops"], True)
        for slot, pk in ((1, None), (0, packed)):
            if pk is None:
                s.submit(0, slot, req, pat, txt, cigar_runs_cap=n * 2 * rs, want_ops=True)
            else:
                s.submit(0, slot, req, packed=pk, cigar_runs_cap=n * 2 * rs, want_ops=True)
            out = s.wait(0, slot, check=False)
            F.compare(out["res"], out["ops"], ores, oops, req, True)
            assert np.array_equal(out["cig"]["score"], ores["score"]) and np.array_equal(out["cig"]["idx"], req["idx"])
            assert np.array_equal(out["cig"]["status"], ores["status"].astype(np.uint16))
            assert (ores["status"] == 0).all()
            assert engine.format_output_runs(out["cig"], out["runs"]) == want


def test_fuzz_fused_seed_77_case(gpu):
    """The first case of `tools/fuzz_parity.py --focus fused --seed 77`, which reported "CIGAR text differs": 5000 low-complexity
    pairs (batch seed 601167582) at READ_SIZE 112, MAX_SCORE 18, mismatch 2 / gap 5 + 4, reduction and CIGAR, REQ8 requests,
    packed rows in and run lists out of wfa_group_kernel. The kernel was right: the fuzzer printed the oracle's text with the
    oracle's own row numbers 0, 1, ... against the device's text with the requests' idx, which gen_pairs starts at 0 and these
    batches at 7000. Here the ops rows, the run lists' headers and the printed CIGARs are all held to the oracle."""
    from aim_amd import engine
    from oracle import oracle
    rs, ms, n = 112, 18, 5000
    req, pat, txt, _, _ = L.low_complexity_batch(rs, n, 601167582, ms)
    params = engine.make_params("wfa", ms, rs, backtrace=True, reduce=True, req8=True, mismatch=2, gap_o=5, gap_e=4)
    ores, oops, _ = L.oracle_of(params, "wfa", req, pat, txt)
    assert (ores["status"] == 0).all() and (ores["score"] <= ms).mean() > 0.5 and (ores["score"] > ms).sum() > 100
    ores["idx"] = req["idx"]
    cap = n * (2 * min(ms, 100 + 8) + 12) + 64          # the fuzzer's run cap
    with engine.DeviceSet(1) as s:
        s.configure_slots(params, n, slots=1, max_raw=n, max_runs=cap)
        s.submit(0, 0, req, packed=engine.pack_batch(req, pat, txt), cigar_runs_cap=cap, want_ops=True)
        out = s.wait(0, 0, check=False)
        assert s.plan_describe(0).split()[0] == "wfa_group_kernel"
    F.compare(out["res"], out["ops"], ores, oops, req, True)
    assert np.array_equal(out["cig"]["score"], ores["score"]) and np.array_equal(out["cig"]["idx"], req["idx"])
    assert engine.format_output_runs(out["cig"], out["runs"]) == oracle.format_output(ores, oops, True)


# ------------------------------------------------------------------ SAM fields
def _assembled_reference(req, txt):
    """(reference, text_pos): the texts laid end to end, every other one reverse-complemented, so that pair i's text is the
    window of text_len bases at text_pos[i] on its strand."""
    from aim_amd import engine
    parts, tpos, at = [], np.zeros(len(req), dtype=np.uint64), 0
    for i in range(len(req)):
        t = txt[i, :req["text_len"][i]]
        minus = i % 2 == 1
        parts.append(engine.ref_window(t, 0, len(t), minus))
        tpos[i] = at | ((1 << 63) if minus else 0)
        at += len(t)
    ref = np.concatenate(parts)
    for i in (0, 1, len(req) - 1):
        assert np.array_equal(engine.ref_window(ref, int(tpos[i]) & ((1 << 63) - 1), int(req["text_len"][i]), i % 2 == 1), txt[i, :req["text_len"][i]])
    return ref, tpos


@pytest.mark.parametrize("wave_min", ["0", "1000000"], ids=["wave", "lane"])
@pytest.mark.parametrize("algo,kw", [("nw", dict(mismatch=7, gap_i=3, gap_d=3)), ("wfa", {})], ids=["nw733", "wfa"])
def test_sam_fields(gpu, monkeypatch, algo, kw, wave_min):
    """AIM_FLAG_SAM_FIELDS on the READ_SIZE 112 batch as REF_TEXTS windows of a reference assembled from its texts, on both
    strands: aim_sam_t, CIGAR words and MD of every finished row equal tests/sam_model.py on the flag-less rows (a deletion
    inside a run of equal bases, 'N' in the reference), on both mappings (AIM_SAM_WAVE_MIN); the flag-less rows are the
    oracle's. NW with mismatch 7 / gaps 3 + 3 writes a foreign base as a deletion next to an insertion."""
    import test_sam_fields_gpu as S
    monkeypatch.setenv("AIM_SAM_WAVE_MIN", wave_min)
    rs = 112
    ms = F.launcher_score(rs, 0.02, 4 if algo == "nw" else 5)
    req, pat, txt, _, _ = L.low_complexity_batch(rs, F.pairs_for(rs), L.SEED, ms)
    ref, tpos = _assembled_reference(req, txt)
    out0, out1, exps, p0 = S.both(kw, ms, rs, algo, ref, req, pat, tpos, check=False)
    ores, oops, _ = L.oracle_of(p0, algo, req, pat, txt)
    F.compare(out1[0]["res"], out1[0]["ops"], ores, oops, req, True)
    assert len(exps[0]) == len(req) and sum(len(e[3]) for e in exps[0]) > len(req)


# ------------------------------------------------------------------ planner routes
ROUTE_ROWS = [(fam, rs) for fam in ("wfa2_red_bt", "nw_bt", "swg16_bt") for rs in (112, 1024)]


@pytest.mark.parametrize("fam,rs", ROUTE_ROWS, ids=lambda v: str(v))
def test_planner_routes_change_nothing(gpu, monkeypatch, fam, rs):
    """The family's batch under every setting of reference_rows.KNOBS that gives it another plan than the default: results and
    the ops bytes inside [begin_offset, end_offset) are byte-equal to the default route's, which are the oracle's."""
    import reference_rows as R
    from aim_amd import engine
    f = L.FAMILIES[fam]
    params = engine.make_params(f["algo"], f["ms"](rs), rs, **f["kw"])
    req, pat, txt, _, _ = L.low_complexity_batch(rs, F.pairs_for(rs), L.SEED, f["ms"](rs))
    ores, oops, _ = L.oracle_of(params, f["algo"], req, pat, txt)
    plans = {}
    for name, env in R.KNOBS:
        R.apply_env(monkeypatch, R.knob_env(env))
        rc, line = R.plan_line(params, len(req))
        if rc == 0:
            plans.setdefault(R.plan_key(line), (name, env))
    assert len(plans) >= 2, plans
    base = None
    for key, (name, env) in plans.items():
        R.apply_env(monkeypatch, R.knob_env(env))
        with engine.DeviceSet(1) as s:
            res, ops = s.align(params, req, pat, txt, check=False)
            line = s.plan_describe(0)
        assert R.plan_key(line) == key, (name, line, key)
        inside = (np.arange(ops.shape[1])[None, :] >= res["begin_offset"][:, None]) & (np.arange(ops.shape[1])[None, :] < res["end_offset"][:, None])
        got = (res.tobytes(), np.where(inside, ops, 0).tobytes())
        if base is None:
            assert name == "default"
            F.compare(res, ops, ores, oops, req, True)
            base = got
        assert got == base, (name, line)
    print("%s/%d: %d routes: %s" % (fam, rs, len(plans), [n for n, _ in plans.values()]))
