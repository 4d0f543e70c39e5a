"""wfa_lane_kernel's refill schedule (AIM_LANE_INTERLEAVE == 2, wfa_lane.hpp): the next group's LDS-DMA pieces are issued
between the pack steps, after the diagonal construction and after the cells of the score loop, and whatever the score loop
had not issued when it left early goes out in one unrolled run behind it. A piece issued too early overwrites rows that are
still being read, one never issued leaves the previous group's rows in LDS; both show as results of the wrong pair. Every
case is compared field by field with the CPU oracle.

Several iterations per wavefront come from AIM_CHIP_CUS=4 (a grid of 32 single-wave workgroups, asserted on the plan line)
with 12 325 pairs: 193 groups, six or seven per wavefront, the batch's last one partial (37 pairs)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_MULTI = 3 * 64 * 64 + 37      # 193 groups of 64 pairs, the last one partial
GRID = 32                       # AIM_CHIP_CUS=4 x 8 workgroups per CU
LENGTH = {112: 100, 80: 70}     # read length whose launcher READ_SIZE is the key


@pytest.fixture(scope="module")
def gpu(built):
    from aim_amd import capi
    lib = capi.load()
    n = C.c_int()
    assert lib.aim_device_count(C.byref(n)) == 0 and n.value >= 1, "no HIP device visible"
    return lib


def _second_groups(n_pairs):
    """The group every wavefront of the GRID-workgroup grid works on in its second iteration (xcd_unit, aim_device.hpp)."""
    n_groups = (n_pairs + 63) // 64
    per_xcd, bpx = (n_groups + 7) // 8, GRID // 8
    out = []
    for xcd in range(8):
        for j in range(bpx):
            local = j + bpx
            if local < per_xcd and xcd * per_xcd + local < n_groups:
                out.append(xcd * per_xcd + local)
    return out


_BATCHES = {}


def _batch(rs, err, variant):
    """Seeded batch (shared by the tests, never modified after it is made). Every variant carries four groups of exact
    matches, the only groups on which the score loop's early exit fires at the first score.
      plain      nothing else
      non_acgt   one 'N' inside one pattern of every wavefront's second group: the raw-byte path in the middle of the refills
      short      one group holds a pair whose sequences are shorter than all but the last 16-base step: the masked pack"""
    key = (rs, err, variant)
    if key not in _BATCHES:
        from aim_amd import engine
        req, pat, txt = engine.gen_pairs(20240 + rs, 0, N_MULTI, LENGTH[rs], err, rs)
        for g in (2, 77, 150, 191):   # exact matches: the whole wavefront is done at score 0
            lo, hi = g * 64, g * 64 + 64
            txt[lo:hi] = pat[lo:hi]
            req["text_len"][lo:hi] = req["pattern_len"][lo:hi]
        if variant == "non_acgt":
            for k, g in enumerate(_second_groups(N_MULTI)):
                p = g * 64 + (7 * k) % 64
                pat[p, (11 * k) % int(req["pattern_len"][p])] = ord("N")
        elif variant == "short":
            p = 100 * 64 + 5
            cut = 16 * (rs // 16 - 1) - 6           # 90 at READ_SIZE 112, 58 at 80: below 16 * (NP - 1)
            req["pattern_len"][p] = cut
            req["text_len"][p] = cut + 1
        _BATCHES[key] = (req, pat, txt)
    return _BATCHES[key]


_ORACLE = {}


def _oracle(key, req, pat, txt, ms, rs, backtrace):
    if key not in _ORACLE:
        from oracle import oracle
        op = oracle.params("wfa", ms, rs, backtrace=backtrace, reduce=True)
        ores, oops, _ = oracle.align_batch(op, req["pattern_len"], req["text_len"], pat, txt, nthreads=8)
        _ORACLE[key] = (ores, oops)
    return _ORACLE[key]


def _check(gpu, key, req, pat, txt, ms, rs, backtrace=False, req8=False, res8=False, grid=None):
    from aim_amd import engine
    params = engine.make_params("wfa", ms, rs, reduce=True, backtrace=backtrace, req8=req8, res8=res8)
    assert gpu.aim_kernel_name(C.byref(params)) == b"wfa_lane_kernel"
    with engine.DeviceSet(1) as s:
        res, ops = s.align(params, req, pat, txt, check=False)
        plan = s.plan_describe(0)
    assert plan.startswith("wfa_lane_kernel"), plan
    if grid is not None:
        assert " grid=%d " % grid in plan, plan
    ores, oops = _oracle(key + (ms, backtrace), req, pat, txt, ms, rs, backtrace)
    # every field the layout carries ({idx, score} with RES8; begin_offset is defined with CIGAR only)
    fields = ("score",) if res8 else ("score", "max_operations", "end_offset", "status") + (("begin_offset",) if backtrace else ())
    for f in ("idx",) + fields:
        exp = req["idx"] if f == "idx" else ores[f]
        bad = np.nonzero(res[f] != exp)[0]
        assert bad.size == 0, "%s differs at pair %d (group %d): hip %d oracle %d" % (f, bad[0], bad[0] // 64, res[f][bad[0]], exp[bad[0]])
    if backtrace:
        assert (res["status"] == 0).all()
        b, e = res["begin_offset"].astype(np.int64), res["end_offset"].astype(np.int64)
        col = np.arange(ops.shape[1])[None, :]
        inside = (col >= b[:, None]) & (col < e[:, None])
        bad = np.nonzero(((ops != oops) & inside).any(axis=1))[0]
        assert bad.size == 0, "ops differ at pair %d: hip %r oracle %r" % (
            bad[0], ops[bad[0], b[bad[0]]:e[bad[0]]].tobytes(), oops[bad[0], b[bad[0]]:e[bad[0]]].tobytes())
    return res


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_no_next_group_or_a_partial_one(gpu, n):
    """One or two groups per wavefront at most: there is no next group, or it is the batch's partial last one (burst path)."""
    from aim_amd import engine
    req, pat, txt = engine.gen_pairs(515, 0, n, 100, 0.01, 112)
    _check(gpu, ("small", n), req, pat, txt, 5, 112)
    _check(gpu, ("small", n), req, pat, txt, 5, 112, req8=True, res8=True)


@pytest.mark.parametrize("variant", ["plain", "non_acgt", "short"])
@pytest.mark.parametrize("compact", [False, True], ids=["default_io", "req8_res8"])
@pytest.mark.parametrize("rs", [112, 80])
def test_refilled_buffers_over_many_iterations(gpu, monkeypatch, rs, compact, variant):
    """Score-only, static shape: every wavefront consumes a buffer it refilled itself five or six times."""
    from aim_amd import engine
    monkeypatch.setenv("AIM_CHIP_CUS", "4")
    ms, got_rs = engine.launcher_sizes("wfa", LENGTH[rs], 0.01)
    assert got_rs == rs
    req, pat, txt = _batch(rs, 0.01, variant)
    res = _check(gpu, (rs, 0.01, variant), req, pat, txt, ms, rs, req8=compact, res8=compact, grid=GRID)
    assert (res["score"][2 * 64:3 * 64] == 0).all()


@pytest.mark.parametrize("variant", ["plain", "non_acgt", "short"])
def test_dynamic_bounds_shape(gpu, monkeypatch, variant):
    """MAX_SCORE 10 at e = 2 %: the score loop of wfa_scores_dynamic hands the pieces out."""
    from aim_amd import engine
    monkeypatch.setenv("AIM_CHIP_CUS", "4")
    ms, rs = engine.launcher_sizes("wfa", 100, 0.02)
    assert (ms, rs) == (10, 112)
    req, pat, txt = _batch(112, 0.02, variant)
    _check(gpu, (112, 0.02, variant), req, pat, txt, ms, rs, grid=GRID)
    _check(gpu, (112, 0.02, variant), req, pat, txt, ms, rs, req8=True, res8=True, grid=GRID)


@pytest.mark.parametrize("variant", ["plain", "non_acgt"])
@pytest.mark.parametrize("rs", [112, 80])
def test_cigar_instantiation(gpu, monkeypatch, rs, variant):
    """With CIGAR: the operations inside [begin_offset, end_offset) are compared as well."""
    from aim_amd import engine
    monkeypatch.setenv("AIM_CHIP_CUS", "4")
    ms, _ = engine.launcher_sizes("wfa", LENGTH[rs], 0.01)
    req, pat, txt = _batch(rs, 0.01, variant)
    _check(gpu, (rs, 0.01, variant), req, pat, txt, ms, rs, backtrace=True, grid=GRID)


@pytest.mark.parametrize("ms", [2, 4])
def test_run_time_max_score_below_the_shape(gpu, monkeypatch, ms):
    """A run-time MAX_SCORE below the template's 5: wavefronts past the cap are computed and ignored, pairs past it report
    MAX_SCORE + 1; the refill must not depend on where a pair stopped."""
    monkeypatch.setenv("AIM_CHIP_CUS", "4")
    req, pat, txt = _batch(112, 0.01, "plain")
    res = _check(gpu, (112, 0.01, "plain"), req, pat, txt, ms, 112, grid=GRID)
    assert (res["score"] == ms + 1).any()
    _check(gpu, (112, 0.01, "plain"), req, pat, txt, ms, 112, backtrace=True, grid=GRID)


@pytest.mark.parametrize("rs", [112, 80])
def test_poisoned_lds(gpu, monkeypatch, rs):
    """AIM_DEBUG_POISON_LDS fills the workgroup's LDS at kernel entry (honoured by the production build): a row or request
    piece of the first refill that is never issued reads 0xff bytes instead of a plausible stale row."""
    from aim_amd import engine
    monkeypatch.setenv("AIM_CHIP_CUS", "4")
    monkeypatch.setenv("AIM_DEBUG_POISON_LDS", "255")
    ms, _ = engine.launcher_sizes("wfa", LENGTH[rs], 0.01)
    req, pat, txt = _batch(rs, 0.01, "non_acgt")
    _check(gpu, (rs, 0.01, "non_acgt"), req, pat, txt, ms, rs, req8=True, res8=True, grid=GRID)
    _check(gpu, (rs, 0.01, "non_acgt"), req, pat, txt, ms, rs, grid=GRID)
