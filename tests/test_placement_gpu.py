"""A pair's result does not depend on its place in the batch (tests/placement.py), on the GPU: every row of the full-row table runs
its batch rotated, reversed, cut to ragged prefixes, as single pairs, with a hostile pair in every other place and as one pair
repeated, all on ONE device set configured once -- so that the per-batch re-plan and the reuse of scratch, to-do counters and
history regions from launch to launch are under test too -- and, up to READ_SIZE 320, eight times over on a one-CU chip, where a
workgroup has many units. The expected rows are a gather of the oracle's rows of the table batch
(tests/test_placement_cpu.py shows that the oracle is per pair, and that this set sees fake devices the table batch cannot)."""
import re

import numpy as np
import pytest

import full_rows as F
import placement as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(built):
    import ctypes as C
    from aim_amd import capi
    lib = capi.load()
    n = C.c_int()
    assert lib.aim_device_count(C.byref(n)) == 0 and n.value >= 1, lib.aim_last_error()
    return lib


def _launch(s, batch):
    req, pat, txt = batch
    s.push(0, req, pat, txt)
    s.launch()
    res, ops = s.pull(0, check=False)
    return res, ops, s.plan_describe(0), s.fallback_pairs(0)


def _token(line, name):
    m = re.search(r" %s=(\d+)" % name, line)
    return int(m.group(1)) if m else None


@pytest.mark.parametrize("fam,rs", F.ROWS, ids=lambda v: str(v))
def test_placement_matches_the_oracle(gpu, monkeypatch, fam, rs):
    """Every arrangement of the row, launch after launch on one set: score, max_operations, end_offset, status and idx of every pair,
    with CIGAR also begin_offset and the ops bytes of [begin_offset, end_offset), equal the oracle's row of that pair. The
    permutations run on the row's own kernel and shape and leave the row's own number of pairs on the to-do list."""
    from aim_amd import capi, engine
    B = F.row_batch(rs, "zero")
    n0 = len(B[0])
    params = F.row_params(fam, rs)
    bt = bool(params.flags & capi.FLAG_BACKTRACE)
    ores, oops = F.oracle_row(fam, rs, "zero")
    u = P.unit_of(F.expected_plan(fam, rs))
    for k, v in F.FAMILIES[fam]["env"].items():          # (full_rows._with_env, put back when the test ends)
        monkeypatch.setenv(k, v)
    with engine.DeviceSet(1) as s:
        s.configure(params, n0)
        for name, sel in P.arrangements(rs, n0, u, short=(fam, rs) in P.SLOW_ROWS):
            batch = P.arranged(B, sel)
            res, ops, line, todo = _launch(s, batch)
            print("%s/%d %s n=%d: %s; to-do list %d" % (fam, rs, name, len(sel), line, todo))
            try:
                F.compare(res, ops, *P.expected(ores, oops, sel), batch[0], bt)
            except AssertionError as e:
                raise AssertionError("%s (n = %d, %s): %s" % (name, len(sel), line, e)) from None
            assert _token(line, "n") == len(sel), line
            if P.is_permutation(sel, n0):
                assert F.plan_matches(line, F.expected_plan(fam, rs)) and P.unit_of(line) == u, (name, line)
                assert todo == F.expected_todo(fam, rs), (name, todo, F.expected_todo(fam, rs))
    if rs <= P.TILED_MAX_RS:
        monkeypatch.setenv("AIM_CHIP_CUS", "1")
        name, sel = P.tiled(n0)
        batch = P.arranged(B, sel)
        with engine.DeviceSet(1) as s:
            s.configure(params, len(sel))
            res, ops, line, todo = _launch(s, batch)
        print("%s/%d %s n=%d, one CU: %s; to-do list %d" % (fam, rs, name, len(sel), line, todo))
        F.compare(res, ops, *P.expected(ores, oops, sel), batch[0], bt)
        assert F.plan_matches(line, F.expected_plan(fam, rs)), line
        waves = _token(line, "grid") * (_token(line, "block") // 64) // (_token(line, "wavefronts_per_pair") or 1)
        units = -(-len(sel) // P.unit_of(line))
        assert waves < units, (line, waves, units)          # fewer wavefronts than units: the persistent loops go round
        assert todo == P.TILED_COPIES * F.expected_todo(fam, rs), (todo, F.expected_todo(fam, rs))    # (a per-pair property)


# ------------------------------------------------------------------ feature rows
HEAD_EXTRA = (F.IDENTICAL, F.TWIN_A, F.TWIN_B, F.N_LAST, F.MIN_PAIRS - 1)          # the head batch of test_full_rows_gpu._head
HEAD_N = F.HEAD + len(HEAD_EXTRA)
_MODEL = {}


def _head_and_model(feature, rs):
    """The head batch and its model scores, computed once per (feature, READ_SIZE)."""
    import affine2p_model, endsfree_model, linear_model
    import test_full_rows_gpu as G
    if (feature, rs) not in _MODEL:
        req, pat, txt = G._head(rs, "zero")
        if feature == "endsfree":
            want = endsfree_model.dp_scores(req, pat, txt, ends_free=F.FEATURES["endsfree"]["ends_free"])
        elif feature == "affine2p":
            want = affine2p_model.dp_scores(req, pat, txt, o2=24, e2=1)
        elif feature == "linear":
            want = linear_model.dp_scores(req, pat, txt, x=2, g=3)
        else:
            want = F.affine_model(req, pat, txt)
        want = np.asarray(want).copy()
        want.flags.writeable = False
        _MODEL[(feature, rs)] = ((req, pat, txt), want)
    return _MODEL[(feature, rs)]


def _rescore_of(feature):
    import affine2p_model, endsfree_model, linear_model
    if feature == "endsfree":
        ef = F.FEATURES["endsfree"]["ends_free"]
        return lambda s, pl, tl: endsfree_model.rescore(s, pl, tl, ends_free=ef)
    if feature == "affine2p":
        return lambda s, pl, tl: affine2p_model.rescore(s, o2=24, e2=1)
    if feature == "linear":
        return lambda s, pl, tl: linear_model.rescore(s, x=2, g=3)
    return lambda s, pl, tl: endsfree_model.rescore(s, pl, tl)


def head_arrangements():
    """`reversed`, rotation 1, the singletons the head batch has (no A_VS_C there) and its last pair, full against full, 64 times."""
    at = {p: i for i, p in enumerate(list(range(F.HEAD)) + list(HEAD_EXTRA))}
    singles = [("single_" + name, np.array([at[p]])) for name, p in P.SINGLETONS if p in at]
    assert len(singles) == len(P.SINGLETONS) - 1
    large = [("reversed", P.reversed_sel(HEAD_N)), ("rot1", P.rotation(HEAD_N, 1)), ("last_pair_64_times", np.full(64, HEAD_N - 1))]
    out = []
    for i in range(len(singles)):
        out += large[i:i + 1] + singles[i:i + 1]
    return out


@pytest.mark.parametrize("feature,rs", F.FEATURE_ROWS, ids=lambda v: str(v))
def test_placement_feature_rows(gpu, feature, rs):
    """ENDSFREE, AFFINE2P, LINEAR, WFA_W32 and WFA_BIDIR on arrangements of their head batch, one set per row: scores equal the
    gathered model scores, every CIGAR uses up both sequences and re-scores to its score, and W32 and BIDIR give the flag-less
    run's score, status, max_operations and end_offset on the same arrangement."""
    import test_full_rows_gpu as G
    from aim_amd import engine
    B, want = _head_and_model(feature, rs)
    assert len(B[0]) == HEAD_N and B[0]["text_len"][P.EMPTY_TEXT] == 0 and B[0]["pattern_len"][P.EMPTY_PATTERN] == 0
    params = F.feature_params(feature, rs)
    plain = engine.make_params("wfa", params.max_score, rs, backtrace=True) if feature in ("w32", "bidir") else None
    with engine.DeviceSet(1) as s, engine.DeviceSet(1) as s0:
        s.configure(params, 64)
        if plain is not None:
            s0.configure(plain, 64)
        for name, sel in head_arrangements():
            req, pat, txt = batch = P.arranged(B, sel)
            res, ops, line, _ = _launch(s, batch)
            print("%s/%d %s n=%d: %s" % (feature, rs, name, len(sel), line))
            assert np.array_equal(res["idx"], req["idx"]) and (res["status"] == 0).all(), name
            assert np.array_equal(res["score"], want[sel]), (name, res["score"].tolist(), want[sel].tolist())
            G._cigars(req, pat, txt, res, ops, _rescore_of(feature))
            if plain is not None:
                bres, _, _, _ = _launch(s0, batch)
                for f in ("score", "status", "max_operations", "end_offset", "idx"):
                    assert np.array_equal(res[f], bres[f]), (name, f)


# ------------------------------------------------------------------ packed input and run lists
_TRANSPORT_ORACLE = {}


def _transport_oracle(fam, rs):
    import test_full_rows_gpu as G
    if (fam, rs) not in _TRANSPORT_ORACLE:
        algo, mk = G._transport_row(fam, rs)
        B = F.row_batch(rs, "noise")
        ores, oops, _ = G._oracle_of(mk(), *B, algo)
        ores.flags.writeable = oops.flags.writeable = False
        _TRANSPORT_ORACLE[(fam, rs)] = (B, mk(), ores, oops)
    return _TRANSPORT_ORACLE[(fam, rs)]


def _transport_rows():
    import test_full_rows_gpu as G
    return G.TRANSPORT


@pytest.mark.parametrize("fam,rs", _transport_rows(), ids=lambda v: str(v))
def test_placement_packed_input_and_run_lists(gpu, fam, rs):
    """`reversed`, a hostile arrangement, the duplicates and the prefix n0 - 1 through aim_set_submit with packed rows and
    device-side run lists, two batches in flight on alternating slots: results and ops equal the gather, and the run lists print
    the CIGARs the gathered ops rows print. Where in the run buffer a pair's runs land follows the order in which the kernel's
    lanes bump the cursor; what its header points to does not."""
    from aim_amd import engine
    B, params, ores, oops = _transport_oracle(fam, rs)
    n0 = len(B[0])
    cap = n0 * 2 * rs
    todo = [("reversed", P.reversed_sel(n0)), P.hostiles(n0)[0]] + P.duplicates(n0) + [P.prefixes(n0, 64)[-1]]
    assert [n for n, _ in todo] == ["reversed", "hostile_a_vs_c", "all_twin_a", "all_after_twins", "prefix%d" % (n0 - 1)]
    batches = [P.arranged(B, sel) for _, sel in todo]

    def check(k, out):
        name, sel = todo[k]
        req = batches[k][0]
        eres, eops = P.expected(ores, oops, sel)
        try:
            F.compare(out["res"], out["ops"], eres, eops, req, True)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (name, e)) from None
        cig = out["cig"]
        assert np.array_equal(cig["idx"], req["idx"]) and np.array_equal(cig["score"], eres["score"]), name
        assert np.array_equal(cig["status"], eres["status"].astype(np.uint16)), name
        assert (eres["status"] == 0).all()
        numbered = eres.copy()
        numbered["idx"] = req["idx"]
        assert engine.format_output_runs(cig, out["runs"]) == engine.format_output(numbered, eops, True), name

    with engine.DeviceSet(1) as s:
        s.configure_slots(params, n0, slots=2, max_raw=n0, max_runs=cap)
        for k, (req, pat, txt) in enumerate(batches):
            s.submit(0, k % 2, req, packed=engine.pack_batch(req, pat, txt), cigar_runs_cap=cap, want_ops=True)
            if k:
                check(k - 1, s.wait(0, (k - 1) % 2, check=False))
        check(len(batches) - 1, s.wait(0, (len(batches) - 1) % 2, check=False))
