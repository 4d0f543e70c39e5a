"""wfa_lane_kernel's result ring (AIM_LANE_RES_RING = K, wfa_lane.hpp): score-only {idx, score} results of K full groups
collect in LDS and leave as 16-B stores at the top of the following iteration; what is left leaves behind the loop, and the
batch's partial last group is stored directly. A slot flushed twice, never, to another group's place or before it was written
shows as idx / score of the wrong pair; a 16-B store past the array's end shows in the guard words. Every case compares idx
and score of every pair with the CPU oracle, with the compact layouts (the ring) and the default ones (the direct store).

A small grid comes from AIM_CHIP_CUS=1: 8 single-wave workgroups (asserted on the plan line), n_groups / 8 iterations each.
K is read off the plan line (512 B of LDS per slot); the shapes below follow it, and are the issue's at K = 8."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_HEAD = 152 * 64 + 37          # 153 groups: seven waves do 20 iterations, the eighth 13 and the partial last group (37 pairs)
GRID = 8                        # AIM_CHIP_CUS=1 x 8 workgroups per CU
LENGTH = {112: 100, 80: 70}
BASE_LDS = {112: 15360, 80: 11264}   # rows + request slots, without a ring


@pytest.fixture(scope="module")
def gpu(built):
    from aim_amd import capi
    lib = capi.load()
    n = C.c_int()
    assert lib.aim_device_count(C.byref(n)) == 0 and n.value >= 1, "no HIP device visible"
    return lib


@pytest.fixture(scope="module")
def ring_k(gpu):
    """Slots of the ring the library was built with (0: no ring); the boundary shapes are the issue's (K = 8) when there is none."""
    from aim_amd import capi, engine
    buf = C.create_string_buffer(512)
    assert gpu.aim_plan_describe(capi.params_ref(engine.make_params("wfa", 5, 112, reduce=True, req8=True, res8=True)), 2048, buf, len(buf)) == 0
    lds = int(buf.value.decode().split(" lds=")[1].split()[0])
    assert (lds - BASE_LDS[112]) % 512 == 0
    return (lds - BASE_LDS[112]) // 512


_BATCHES, _ORACLE = {}, {}


def _batch(rs, err, variant="plain"):
    """Seeded batch of N_HEAD pairs, shared and never modified once made; smaller cases are prefixes of it (a pair's result does
    not depend on the batch around it). non_acgt: an 'N' in one pattern of group 10 -- with 8 workgroups the second iteration
    of its wave, in the middle of the first ring."""
    key = (rs, err, variant)
    if key not in _BATCHES:
        from aim_amd import engine
        req, pat, txt = engine.gen_pairs(7310 + rs, 0, N_HEAD, LENGTH[rs], err, rs)
        if variant == "non_acgt":
            p = 10 * 64 + 21
            pat[p, int(req["pattern_len"][p]) // 2] = ord("N")
        _BATCHES[key] = (req, pat, txt)
    return _BATCHES[key]


def _oracle(key, ms, rs):
    if key + (ms,) not in _ORACLE:
        from oracle import oracle
        req, pat, txt = _batch(*key)
        ores, _, _ = oracle.align_batch(oracle.params("wfa", ms, rs, backtrace=False, reduce=True), req["pattern_len"], req["text_len"], pat, txt, nthreads=8)
        _ORACLE[key + (ms,)] = ores
    return _ORACLE[key + (ms,)]


def _compare(res, req, ores, n, what):
    for f in ("idx", "score"):
        exp = (req["idx"] if f == "idx" else ores[f])[:n]
        bad = np.nonzero(res[f][:n] != exp)[0]
        assert bad.size == 0, "%s: %s differs at pair %d (group %d) of %d: hip %d oracle %d (%d pairs differ)" % (
            what, f, bad[0], bad[0] // 64, n, res[f][bad[0]], exp[bad[0]], bad.size)


def _check(gpu, key, ms, rs, n=N_HEAD, compact=True, grid=None):
    from aim_amd import engine
    req, pat, txt = _batch(*key)
    params = engine.make_params("wfa", ms, rs, reduce=True, req8=compact, res8=compact)
    assert gpu.aim_kernel_name(C.byref(params)) == b"wfa_lane_kernel"
    with engine.DeviceSet(1) as s:
        res, _ = s.align(params, req[:n], pat[:n], txt[:n], check=False)
        plan = s.plan_describe(0)
    assert plan.startswith("wfa_lane_kernel"), plan
    if grid is not None:
        assert " grid=%d " % grid in plan, plan
    _compare(res, req, _oracle(key, ms, rs), n, "%s n=%d %s" % (key, n, "req8/res8" if compact else "default"))
    return res


LAYOUTS = pytest.mark.parametrize("compact", [True, False], ids=["req8_res8", "default_io"])


@LAYOUTS
def test_headline_shape(gpu, monkeypatch, compact):
    """READ_SIZE 112, MAX_SCORE 5: at K = 8 two full flushes and a 4-slot remainder in seven waves; one flush, a remainder and
    the partial last group in the eighth."""
    monkeypatch.setenv("AIM_CHIP_CUS", "1")
    _check(gpu, (112, 0.01), 5, 112, compact=compact, grid=GRID)


@LAYOUTS
def test_read_size_80(gpu, monkeypatch, compact):
    from aim_amd import engine
    monkeypatch.setenv("AIM_CHIP_CUS", "1")
    ms, rs = engine.launcher_sizes("wfa", 70, 0.01)
    assert rs == 80
    _check(gpu, (80, 0.01), ms, 80, compact=compact, grid=GRID)


@LAYOUTS
def test_dynamic_bounds_shape(gpu, monkeypatch, compact):
    from aim_amd import engine
    monkeypatch.setenv("AIM_CHIP_CUS", "1")
    assert engine.launcher_sizes("wfa", 100, 0.02) == (10, 112)
    _check(gpu, (112, 0.02), 10, 112, compact=compact, grid=GRID)


@LAYOUTS
@pytest.mark.parametrize("extra", [0, 1], ids=["full_groups", "plus_one_pair"])
@pytest.mark.parametrize("which", ["8K-1", "8K", "8K+1", "16K"])
def test_boundary_group_counts(gpu, monkeypatch, ring_k, which, extra, compact):
    """Per wave: a ring one short of full, exactly full at loop exit, one past, and two full rounds; with and without a partial
    group of one pair behind them."""
    monkeypatch.setenv("AIM_CHIP_CUS", "1")
    k = ring_k or 8
    groups = {"8K-1": 8 * k - 1, "8K": 8 * k, "8K+1": 8 * k + 1, "16K": 16 * k}[which]
    n = groups * 64 + extra
    assert n <= N_HEAD
    _check(gpu, (112, 0.01), 5, 112, n=n, compact=compact, grid=GRID)


@LAYOUTS
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_short_batches(gpu, n, compact):
    """Default grid: the ring is never filled, there is only the flush behind the loop."""
    _check(gpu, (112, 0.01), 5, 112, n=n, compact=compact)


GUARDED_CHILD = '''
import sys
import torch
torch.cuda.init()   # (before the library: the device buffers are torch's)
sys.path.insert(0, "tests")
import test_lane_result_ring_gpu as t
t.guarded_result_arrays()
print("GUARDED_OK")
'''


def test_guarded_result_array(gpu):
    """aim_align_device on torch buffers, as bench.py calls it (in a child process that brings up torch before the library): the
    result array is pre-filled with a sentinel and followed by guard words. No 16-B store may reach the guard, and every pair
    below n is written (the sentinel is no pair's idx). n odd, and n = 63 (mod 64); both layouts."""
    env = dict(os.environ, AIM_CHIP_CUS="1")
    p = subprocess.run([sys.executable, "-c", GUARDED_CHILD], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0 and "GUARDED_OK" in p.stdout, p.stdout + p.stderr


def guarded_result_arrays():
    import torch
    from aim_amd import capi, engine
    lib = capi.load()
    req, pat, txt = _batch(112, 0.01)
    ores = _oracle((112, 0.01), 5, 112)
    assert (req["idx"] != 0xA5A5A5A5).all()
    dev = torch.device("cuda", 0)

    def to_dev(a, pad=64):
        t = torch.zeros(a.nbytes + pad, dtype=torch.uint8, device=dev)
        t[:a.nbytes].copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)))
        return t

    guard = 256
    for n in (N_HEAD, 40 * 64 + 63):
        assert n % 2 == 1
        for compact in (True, False):
            params = engine.make_params("wfa", 5, 112, reduce=True, req8=compact, res8=compact)
            res_dtype = capi.RESULT8_DTYPE if compact else capi.RESULT_DTYPE
            d_req = to_dev(engine.to_request8(req[:n]) if compact else req[:n])
            d_pat, d_txt = to_dev(pat[:n]), to_dev(txt[:n])
            d_res = torch.full((n * res_dtype.itemsize + guard,), 0xA5, dtype=torch.uint8, device=dev)
            sb = lib.aim_scratch_bytes(C.byref(params), n)
            d_scr = torch.zeros(max(sb, 256), dtype=torch.uint8, device=dev)
            torch.cuda.synchronize(dev)
            capi.check(lib.aim_align_device(C.byref(params), n, d_req.data_ptr(), d_pat.data_ptr(), d_txt.data_ptr(), d_res.data_ptr(), None,
                                            d_scr.data_ptr(), d_scr.numel(), None))
            torch.cuda.synchronize(dev)
            out = d_res.cpu().numpy()
            tail = out[n * res_dtype.itemsize:]
            assert (tail == 0xA5).all(), "n=%d compact=%s: guard overwritten at byte %d behind the array" % (n, compact, int(np.nonzero(tail != 0xA5)[0][0]))
            _compare(out[:n * res_dtype.itemsize].view(res_dtype), req, ores, n, "guarded n=%d %s" % (n, "req8/res8" if compact else "default"))


@LAYOUTS
def test_poisoned_lds(gpu, monkeypatch, compact):
    """LDS filled with 0xff at kernel entry: a slot flushed before it was written shows as 0xffffffff results."""
    monkeypatch.setenv("AIM_CHIP_CUS", "1")
    monkeypatch.setenv("AIM_DEBUG_POISON_LDS", "255")
    _check(gpu, (112, 0.01), 5, 112, compact=compact, grid=GRID)


@LAYOUTS
def test_non_acgt_group_in_mid_ring(gpu, monkeypatch, compact):
    """A group that takes the raw-byte path lands in its slot like any other."""
    monkeypatch.setenv("AIM_CHIP_CUS", "1")
    res = _check(gpu, (112, 0.01, "non_acgt"), 5, 112, compact=compact, grid=GRID)
    assert res["idx"][10 * 64 + 21] == _batch(112, 0.01, "non_acgt")[0]["idx"][10 * 64 + 21]


@LAYOUTS
def test_run_time_max_score_below_the_shape(gpu, monkeypatch, compact):
    """MAX_SCORE 2 on the MAX_SCORE 5 shape: scores of MAX_SCORE + 1 go through the ring."""
    monkeypatch.setenv("AIM_CHIP_CUS", "1")
    res = _check(gpu, (112, 0.01), 2, 112, compact=compact, grid=GRID)
    assert (res["score"] == 3).any()
