"""Sequences that fill READ_SIZE on every kernel shape (tests/full_rows.py), on the GPU: every table row, zero- and noise-padded,
against the oracle pair by pair; the flagged WFA modes against their models; the packed / compact, REQ8 / RES8, REF_TEXTS and
SAM_FIELDS transports; device arrays with exactly the documented tail slack; and the planner and poison knobs, which must change
nothing. tests/test_full_rows_cpu.py shows that the oracle ignores the bytes behind a length, that the table reaches the shapes it names and that the comparison used here fails on
a kernel that is wrong at these edges."""
import os
import subprocess
import sys

import numpy as np
import pytest

import full_rows as F
from conftest import ROOT

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(built):
    import ctypes as C
    from aim_amd import capi
    lib = capi.load()
    n = C.c_int()
    assert lib.aim_device_count(C.byref(n)) == 0 and n.value >= 1, lib.aim_last_error()
    return lib


@pytest.mark.parametrize("pad", ["zero", "noise"])
@pytest.mark.parametrize("fam,rs", F.ROWS, ids=lambda v: str(v))
def test_full_rows_match_the_oracle(gpu, fam, rs, pad):
    """Every pair of the row's batch: score, max_operations, end_offset and status, and with CIGAR begin_offset and the ops bytes
    of [begin_offset, end_offset); the plan line names the row's kernel and shape, and the to-do list holds the row's pinned
    number of pairs (full_rows.expected_todo), the same under both paddings."""
    from aim_amd import capi
    req, _, _ = F.row_batch(rs, pad)
    res, ops, line, todo = F.align_row(fam, rs, pad)
    print("%s/%d %s: %s; to-do list %d of %d pairs" % (fam, rs, pad, line, todo, len(req)))
    assert F.plan_matches(line, F.expected_plan(fam, rs)), line
    ores, oops = F.oracle_row(fam, rs, pad)
    F.compare(res, ops, ores, oops, req, bool(F.row_params(fam, rs).flags & capi.FLAG_BACKTRACE))
    assert todo == F.expected_todo(fam, rs), (todo, F.expected_todo(fam, rs))


# ------------------------------------------------------------------ feature rows
def _head(rs, pad):
    return F.head_only(*F.full_row_batch(rs, F.MIN_PAIRS, F.SEED, pad), extra=(F.IDENTICAL, F.TWIN_A, F.TWIN_B, F.N_LAST, F.MIN_PAIRS - 1))


def _cigars(req, pat, txt, res, ops, rescore):
    """Every CIGAR uses up both sequences, tells matches from mismatches truthfully and re-scores to the reported score."""
    from endsfree_model import check_cigar
    for i in range(len(req)):
        p, t = bytes(pat[i, :req["pattern_len"][i]]), bytes(txt[i, :req["text_len"][i]])
        s = bytes(ops[i, int(res["begin_offset"][i]):int(res["end_offset"][i])]).decode()
        assert res["max_operations"][i] == len(p) + len(t)
        assert check_cigar(s, p, t) is None, (i, s)
        assert rescore(s, len(p), len(t)) == res["score"][i], (i, s)


@pytest.mark.parametrize("pad", ["zero", "noise"])
@pytest.mark.parametrize("feature,rs", F.FEATURE_ROWS, ids=lambda v: str(v))
def test_feature_rows_match_their_models(gpu, feature, rs, pad):
    """ENDSFREE, AFFINE2P, LINEAR and WFA_BIDIR on the head pairs (and five more full pairs), every pair under the cap: scores
    equal the flag's own model and the CIGARs re-score to them. WFA_W32 (READ_SIZE 1024: below 32 760) gives the flag-less bytes."""
    import affine2p_model, endsfree_model, linear_model
    from aim_amd import engine
    req, pat, txt = _head(rs, pad)
    params = F.feature_params(feature, rs)
    res, ops = engine.align(params, req, pat, txt)
    sres, _ = engine.align(F.feature_params(feature, rs, backtrace=feature == "bidir"), req, pat, txt)
    assert (res["status"] == 0).all() and np.array_equal(sres["score"], res["score"])
    if feature == "endsfree":
        ef = F.FEATURES["endsfree"]["ends_free"]
        assert np.array_equal(res["score"], endsfree_model.dp_scores(req, pat, txt, ends_free=ef))
        _cigars(req, pat, txt, res, ops, lambda s, pl, tl: endsfree_model.rescore(s, pl, tl, ends_free=ef))
    elif feature == "affine2p":
        assert np.array_equal(res["score"], affine2p_model.dp_scores(req, pat, txt, o2=24, e2=1))
        _cigars(req, pat, txt, res, ops, lambda s, pl, tl: affine2p_model.rescore(s, o2=24, e2=1))
    elif feature == "linear":
        assert np.array_equal(res["score"], linear_model.dp_scores(req, pat, txt, x=2, g=3))
        assert np.array_equal(res["score"], F.nw_model(req, pat, txt, 2, 3, 3))
        _cigars(req, pat, txt, res, ops, lambda s, pl, tl: linear_model.rescore(s, x=2, g=3))
    else:
        plain = engine.make_params("wfa", params.max_score, rs, backtrace=True)
        bres, bops = engine.align(plain, req, pat, txt)
        ores, oops, _ = _oracle_of(plain, req, pat, txt)
        F.compare(bres, bops, ores, oops, req, True)
        assert np.array_equal(res["score"], F.affine_model(req, pat, txt))
        if feature == "w32":
            F.compare(res, ops, ores, oops, req, True)
        else:
            for f in ("score", "status", "max_operations", "end_offset"):
                assert np.array_equal(res[f], bres[f]), f
            _cigars(req, pat, txt, res, ops, lambda s, pl, tl: endsfree_model.rescore(s, pl, tl))


def _oracle_of(params, req, pat, txt, algo="wfa"):
    from oracle import oracle
    return oracle.align_batch(F.oracle_params(params, algo), req["pattern_len"], req["text_len"], pat, txt, nthreads=8)


# ------------------------------------------------------------------ transport rows
TRANSPORT = [("wfa2_red_bt", 112), ("nw_bt", 176), ("swg16_bt", 1024), ("wfa2_bt", 1024)]


def _transport_row(fam, rs):
    """The family's params at a READ_SIZE of the transport rows (the planner picks the kernel; nothing here depends on which)."""
    from aim_amd import engine
    f = F.FAMILIES[fam]
    return f["algo"], lambda **kw: engine.make_params(f["algo"], f["ms"](rs), rs, **dict(f["kw"], **kw))


@pytest.mark.parametrize("fam,rs", TRANSPORT, ids=lambda v: str(v))
def test_packed_input_and_compact_runs_on_full_rows(gpu, fam, rs):
    """aim_set_submit with rows packed to the last 2-bit slot (the N pair travels raw) and device-side run lists: results equal the
    oracle's, and the run lists print the CIGAR the ops rows print."""
    from aim_amd import engine
    algo, mk = _transport_row(fam, rs)
    req, pat, txt = F.row_batch(rs, "noise")
    n = len(req)
    params = mk()
    ores, oops, _ = _oracle_of(params, req, pat, txt, algo)
    packed = engine.pack_batch(req, pat, txt)
    assert F.N_LAST in packed[2].tolist() and len(packed[2]) < n // 2 and packed[0].shape[1] * 16 == rs
    assert packed[0][F.IDENTICAL, -1] >> 30 == engine._CODE[pat[F.IDENTICAL, rs - 1]]          # the last slot holds the last base
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
            if (ores["status"] == 0).all():
                assert engine.format_output_runs(out["cig"], out["runs"]) == want


@pytest.mark.parametrize("fam,rs", [("wfa2_red", 112), ("nw", 176), ("swg16", 1024), ("wfa2", 1024)], ids=lambda v: str(v))
def test_req8_res8_on_full_rows(gpu, fam, rs):
    from aim_amd import engine
    algo, mk = _transport_row(fam, rs)
    req, pat, txt = F.row_batch(rs, "noise")
    ores, _, _ = _oracle_of(mk(), req, pat, txt, algo)
    for req8, res8 in ((True, True), (True, False), (False, True)):
        res, _ = engine.align(mk(req8=req8, res8=res8), req, pat, txt, check=False)
        assert np.array_equal(res["idx"], req["idx"])
        if res8:
            ok = ores["status"] == 0
            assert np.array_equal(res["score"][ok], ores["score"][ok])
        else:
            F.compare(res, None, ores, None, req, False)
    bres, bops = engine.align(mk(req8=True, backtrace=True), req, pat, txt, check=False)
    ores, oops, _ = _oracle_of(mk(backtrace=True), req, pat, txt, algo)
    F.compare(bres, bops, ores, oops, req, True)


def _ref_batch(rs, n=24):
    """(reference, requests, patterns, text_pos, texts): windows of length READ_SIZE on both strands -- pairs 0 / 1 start at
    position 0, pairs 2 / 3 end at ref_len exactly -- against patterns that fill their rows (every third one base short, noise
    behind it); the last pair is 'A' * rs against a run of 'C' * rs in the reference."""
    from aim_amd import engine
    rng = np.random.default_rng([rs, 0x72656677])
    ref = F.ACGT[rng.integers(0, 4, size=6 * rs + 5)]
    ref[3 * rs:4 * rs] = ord("C")
    ref_len = len(ref)
    pos = rng.integers(0, ref_len - rs + 1, size=n)
    pos[:4] = (0, 0, ref_len - rs, ref_len - rs)
    pos[n - 1] = 3 * rs
    minus = np.arange(n) % 2 == 1
    minus[n - 1] = False
    tpos = pos.astype(np.uint64) | (minus.astype(np.uint64) << np.uint64(63))
    req = np.zeros(n, dtype=engine.REQUEST_DTYPE)
    pat = F.ACGTN[rng.integers(0, 5, size=(n, rs))]
    txt = np.zeros((n, rs), dtype=np.uint8)
    for i in range(n):
        txt[i] = engine.ref_window(ref, int(pos[i]), rs, bool(minus[i]))
        pl = rs - (i % 3 == 2)
        pat[i, :pl] = F._derived_text(rng, txt[i], pl)
        req[i] = (pl, rs, 0, 900 + i)
    pat[n - 1] = ord("A")
    req["pattern_len"][n - 1] = rs
    return ref, req, pat, tpos, txt


@pytest.mark.parametrize("fam,rs", TRANSPORT, ids=lambda v: str(v))
def test_ref_texts_windows_of_read_size(gpu, fam, rs):
    """Texts named as windows of length READ_SIZE of a resident reference, on both strands, one at position 0 and one that ends
    at ref_len exactly, against patterns that fill their rows: every output equals the explicit-text batch's and the oracle's."""
    from aim_amd import engine
    algo, mk = _transport_row(fam, rs)
    ref, req, pat, tpos, txt = _ref_batch(rs)
    ores, oops, _ = _oracle_of(mk(), req, pat, txt, algo)
    res0, ops0 = engine.align(mk(), req, pat, txt, check=False)
    F.compare(res0, ops0, ores, oops, req, True)
    res, ops = engine.align(mk(ref_texts=True), req, pat, None, check=False, reference=ref, text_pos=tpos)
    F.compare(res, ops, ores, oops, req, True)
    assert res.tobytes() == res0.tobytes()


@pytest.mark.parametrize("wave_min", ["0", "1000000"], ids=["wave", "lane"])
@pytest.mark.parametrize("rs", [112, 1024])
def test_sam_fields_of_full_rows(gpu, monkeypatch, rs, wave_min):
    """AIM_FLAG_SAM_FIELDS on the REF_TEXTS batch, NW with mismatch 7 / gaps 3 + 3: pos, ref_span, nm, CIGAR words and MD of
    every row equal tests/sam_model.py on the flag-less rows, on both mappings (AIM_SAM_WAVE_MIN), the 2 * rs-operation row (all
    deletions and insertions) included, whatever the flag's rule makes of it."""
    import test_sam_fields_gpu as S
    monkeypatch.setenv("AIM_SAM_WAVE_MIN", wave_min)
    ref, req, pat, tpos, txt = _ref_batch(rs)
    kw = dict(mismatch=7, gap_i=3, gap_d=3)
    out0, out1, exps, p0 = S.both(kw, F.launcher_score(rs, 0.02, 4), rs, "nw", ref, req, pat, tpos)
    r = out0[0]["res"][len(req) - 1]
    assert r["status"] == 0 and r["begin_offset"] == 0 and r["end_offset"] == 2 * rs
    ores, oops, _ = _oracle_of(p0, req, pat, txt, "nw")
    F.compare(out1[0]["res"], out1[0]["ops"], ores, oops, req, True)
    assert len(exps[0]) == len(req) and sum(len(e[3]) for e in exps[0]) > len(req)


# ------------------------------------------------------------------ device arrays with the documented slack
@pytest.mark.parametrize("fam,rs", [("nw", 120), ("nw_bt", 104), ("nw_bt", 184), ("swg16_bt", 136), ("wfa2_bt", 88), ("wfa5_bt", 72), ("nw_bt", 1288)],
                         ids=lambda v: str(v))
def test_align_device_with_exactly_the_documented_slack(gpu, fam, rs):
    """aim_align_device on device arrays of n * READ_SIZE + 16 bytes (the READ_SIZE % 16 == 8 rows are the ones whose 16-byte
    staging loads reach 8 bytes past the last row), the 16 slack bytes noise: the results are the oracle's, so they depend neither
    on the slack's contents nor on anything behind it."""
    import ctypes as C
    import test_sam_fields_gpu as S
    from aim_amd import capi
    req, pat, txt = F.row_batch(rs, "noise")
    n = len(req)
    params = F.row_params(fam, rs)
    bt = bool(params.flags & capi.FLAG_BACKTRACE)
    slack = F.ACGTN[np.random.default_rng(rs).integers(0, 5, size=(2, 16))]
    h = S.Hip()
    try:
        d_pat = h.up(np.concatenate([pat.reshape(-1), slack[0]]))
        d_txt = h.up(np.concatenate([txt.reshape(-1), slack[1]]))
        d_req, d_res = h.up(req), h.up(np.zeros(n * capi.RESULT_DTYPE.itemsize, dtype=np.uint8))
        d_ops = h.up(np.zeros(n * 2 * rs if bt else 16, dtype=np.uint8))
        sb = int(gpu.aim_scratch_bytes(capi.params_ref(params), n))
        d_scr = h.up(np.full(max(sb, 256), 0xA5, dtype=np.uint8))
        rc = gpu.aim_align_device(capi.params_ref(params), n, d_req, d_pat, d_txt, d_res, d_ops if bt else None, d_scr, sb, None)
        assert rc == 0, gpu.aim_last_error()
        res = h.down(d_res, n * capi.RESULT_DTYPE.itemsize).view(capi.RESULT_DTYPE)
        ops = h.down(d_ops, n * 2 * rs).reshape(n, 2 * rs) if bt else None
    finally:
        h.free()
    ores, oops = F.oracle_row(fam, rs, "noise")
    F.compare(res, ops, ores, oops, req, bt)


# ------------------------------------------------------------------ knobs
KNOB_ROWS = ["nw/192", "nw_bt/192", "swg16_bt/192", "nw/1024", "nw_bt/1024", "swg16_bt/1024", "nw_bt/2048", "swg16_bt/2048", "nw_bt_733/2048"]


def _align_in_a_process(tmp_path, name, env):
    e = {k: v for k, v in os.environ.items() if not k.startswith("AIM_") or k == "AIM_LIB"}
    e.update(env)
    out = str(tmp_path / (name + ".npz"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "full_rows.py"), "--align", out] + KNOB_ROWS, env=e, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-1000:] + r.stderr[-2000:]
    return np.load(out)


@pytest.fixture(scope="module")
def default_knobs(gpu, tmp_path_factory):
    return _align_in_a_process(tmp_path_factory.mktemp("knobs"), "default", {})


@pytest.mark.parametrize("env", [{"AIM_CHIP_CUS": "2"}, {"AIM_DEBUG_POISON_SCRATCH": "165"}, {"AIM_DEBUG_POISON_OPS": "90"},
                                 {"AIM_DEBUG_POISON_LDS": "255"}], ids=lambda e: "+".join(e))
def test_knobs_change_nothing(gpu, default_knobs, tmp_path, env):
    """The READ_SIZE 192, 1024 and 2048 rows in a process of their own under a two-CU chip and each poison knob: results and the
    ops bytes inside [begin_offset, end_offset) are byte-equal to the default process's."""
    got = _align_in_a_process(tmp_path, "knob", env)
    assert sorted(got.files) == sorted(default_knobs.files) and len(got.files) >= len(KNOB_ROWS)
    for k in got.files:
        assert got[k].tobytes() == default_knobs[k].tobytes(), k
