"""wfa_lane_kernel's result ring on the plan line (no GPU): the score-only {idx, score} lane plan carries 512 B of LDS per ring
slot behind the request slots and still fits 8 workgroups on a CU; the plans without a ring -- with CIGAR, and the default
result layout -- are the lines of the library before the ring existed."""
import ctypes as C

import pytest

RING_SLOTS = 8                       # AIM_LANE_RES_RING of the shipped build (wfa_lane.hpp)
BASE_LDS = {112: 15360, 80: 11264}   # 2 x 64 rows + 64 request slots of 16 B
LENGTH = {112: 100, 80: 70}

# AIM_SCRATCH_GB=16, AIM_CHIP_CUS=256, 2 048 pairs: the lines of the library before the ring
BEFORE = {
    (112, "cigar"): "wfa_lane_kernel n=2048 grid=32 block=64 lds=16896 scratch=256 budget=17179869184",
    (112, "default"): "wfa_lane_kernel n=2048 grid=32 block=64 lds=15360 scratch=256 budget=17179869184",
    (80, "cigar"): "wfa_lane_kernel n=2048 grid=32 block=64 lds=12800 scratch=256 budget=17179869184",
    (80, "default"): "wfa_lane_kernel n=2048 grid=32 block=64 lds=11264 scratch=256 budget=17179869184",
}


@pytest.fixture(scope="module")
def lib(built):
    from aim_amd import capi
    return capi.load()


def _describe(lib, params, n=2048):
    from aim_amd import capi
    buf = C.create_string_buffer(512)
    assert lib.aim_plan_describe(capi.params_ref(params), n, buf, len(buf)) == 0, lib.aim_last_error().decode()
    return buf.value.decode()


def _params(rs, **kw):
    from aim_amd import engine
    ms, got = engine.launcher_sizes("wfa", LENGTH[rs], 0.01)
    assert got == rs
    return engine.make_params("wfa", ms, rs, reduce=True, **kw)


@pytest.fixture(autouse=True)
def _env(monkeypatch):
    monkeypatch.setenv("AIM_SCRATCH_GB", "16")
    monkeypatch.setenv("AIM_CHIP_CUS", "256")


@pytest.mark.parametrize("rs", [112, 80])
def test_ring_lds_on_the_score_only_res8_plan(lib, rs):
    line = _describe(lib, _params(rs, req8=True, res8=True))
    assert line == "wfa_lane_kernel n=2048 grid=32 block=64 lds=%d scratch=256 budget=17179869184" % (BASE_LDS[rs] + 512 * RING_SLOTS), line
    # the dynamic-bounds shape (MAX_SCORE 10) shares the code and the ring
    if rs == 112:
        from aim_amd import engine
        dyn = _describe(lib, engine.make_params("wfa", 10, 112, reduce=True, req8=True, res8=True))
        assert " lds=%d " % (BASE_LDS[112] + 512 * RING_SLOTS) in dyn, dyn


@pytest.mark.parametrize("rs", [112, 80])
def test_eight_workgroups_still_fit_a_cu(lib, rs):
    """LDS is handed out in granules of 1 280 B; the persistent grid is 8 workgroups per CU."""
    line = _describe(lib, _params(rs, req8=True, res8=True))
    lds = int(line.split(" lds=")[1].split()[0])
    assert (160 * 1024) // ((lds + 1279) // 1280 * 1280) >= 8, line
    assert RING_SLOTS <= 10


@pytest.mark.parametrize("rs", [112, 80])
def test_plans_without_a_ring_are_unchanged(lib, rs):
    assert _describe(lib, _params(rs, backtrace=True)) == BEFORE[(rs, "cigar")]
    assert _describe(lib, _params(rs)) == BEFORE[(rs, "default")]
