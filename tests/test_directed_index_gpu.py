"""The five seeding kernels on hand-built indexes (tests/directed_index.py): every batch of the table through every kernel it names,
over buffers prefilled with 0xEE, each output array compared byte for byte with the model -- hits at positions up to
AIM_SEED_MAX_REF_LEN, a case on each side of every threshold of the rule, K from 1 to 16, and the raw arrays of E4, whose entries point
outside what aim_index_sizes describes (and never outside the allocations: tests/test_directed_index_cpu.py). The chaining kernels run
with d_chains given and NULL; seed_chain_long_kernel at H = 1024 and read_size <= 4096 also equals seed_chain_minimizer_kernel on the
same buffers. What each scenario is, and that the model shows it, is the CPU module's part."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import child  # noqa: E402
import directed_index as d  # noqa: E402
from gpu_buffers import Hip  # noqa: E402

NAMES = ("requests", "text_pos", "votes", "seed", "chains")
RUNS = sorted({(name, kernel, H) for name, kernel, H, _ in d.runs()})
_STATE = {"failed": False}


def launch(h, kernel, b, K, H, d_in, chains=True):
    """One launch of `kernel` over the uploaded batch d_in = (d_rl, d_rows, d_bucket, d_pos), every output prefilled with 0xEE: four
    arrays for the voting kernels, five for the chaining ones (four with chains=False, which passes d_chains = NULL). Once a step
    has failed, no later one starts."""
    if _STATE["failed"]:
        pytest.fail("an earlier GPU step of this module failed: nothing more is started")
    _STATE["failed"] = True
    from aim_amd import capi, engine
    p, n = b["params"], len(b["rl"])
    voting = kernel in d.VOTING
    sp = engine.seed_params(p["k"], p["read_size"], stride=1, max_occ=p["max_occ"], band=p["band"], flank=p["flank"], min_votes=p["min_votes"], max_cands=K,
                            w=None if d.MODE[kernel] == "stride" else d.W, long_reads=kernel == "long")
    out = [h.filled(n * K * 16), h.filled(n * K * 8), h.filled(n * K * 4), h.filled(n * 16)]
    if voting:
        engine.seed_device(sp, n, *d_in, p["ref_len"], *out)
    else:
        out.append(h.filled(n * K * 16) if chains else None)
        if kernel == "long":
            engine.seed_chain_long_device(sp, H, n, *d_in, p["ref_len"], *out)
        else:
            engine.seed_chain_device(sp, n, *d_in, p["ref_len"], *out)
    got = [h.down(out[0], n * K * 16).view(capi.REQUEST_DTYPE), h.down(out[1], n * K * 8).view(np.uint64), h.down(out[2], n * K * 4).view(np.uint32),
           h.down(out[3], n * 16).view(capi.SEED_DTYPE)]
    if not voting and chains:
        got.append(h.down(out[4], n * K * 16).view(capi.CHAIN_DTYPE))
    _STATE["failed"] = False
    return got


def upload(h, b):
    """(d_rl, d_rows, d_bucket, d_pos): the raw arrays as they are; d_pos is the batch's dev_pos, for E4 the padded allocation."""
    return (h.up(np.ascontiguousarray(b["rl"], dtype=np.int32)), h.up(np.ascontiguousarray(b["rows"]), 64), h.up(b["raw"][0]), h.up(b["dev_pos"]))


def assert_equal(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert g.tobytes() == w.tobytes(), (what, name, np.nonzero(g.view(np.uint8) != w.view(np.uint8))[0][:8] // g.dtype.itemsize)


@pytest.mark.parametrize("name,kernel,H", RUNS, ids=["%s-%s-H%d" % r for r in RUNS])
def test_equals_model(name, kernel, H):
    from aim_amd import capi, engine
    assert engine.features() & capi.FEATURE_SEED_CHAIN_LONG and engine.features() & capi.FEATURE_MINIMIZERS
    b = d.batch(name, d.MODE[kernel], H)
    p = b["params"]
    if name == "e4":
        assert int(b["raw"][0].max()) <= d.E4_POS_ALLOC == len(b["dev_pos"]) and len(d.e4_affected(b["raw"][0]))
    else:
        assert int(b["raw"][0][-1]) == len(b["dev_pos"]) and p["ref_len"] == d.REF_LEN
    with Hip() as h:
        d_in = upload(h, b)
        for K in (p["K"] if isinstance(p["K"], tuple) else (p["K"],)):
            want = d.expected(name, kernel, H, K)
            got = launch(h, kernel, b, K, H, d_in)
            assert_equal(got, want, (name, kernel, H, K))
            if kernel in d.VOTING:
                continue
            assert_equal(launch(h, kernel, b, K, H, d_in, chains=False), want[:4], (name, kernel, H, K, "d_chains NULL"))
            if kernel == "long" and H == 1024 and p["read_size"] <= 4096:      # the header's identity
                assert_equal(launch(h, "chain_min", b, K, H, d_in), got, (name, "long == chain_min", K))


# ---- any CU count and poison knob: the two largest batches in a child process ---------------------------------------------------------
def knob_batch():
    out = {}
    for name in d.LARGEST:
        for kernel in d.TABLE[name][0]["kernels"]:
            b = d.batch(name, d.MODE[kernel])
            with Hip() as h:
                got = launch(h, kernel, b, b["params"]["K"], 1024, upload(h, b))
            for n, arr in zip(NAMES, got):
                out["%s-%s-%s" % (name, kernel, n)] = arr.view(np.uint8)
    return out


@pytest.mark.parametrize("env", [{"AIM_CHIP_CUS": "1", "AIM_DEBUG_POISON_SCRATCH": "165", "AIM_DEBUG_POISON_OPS": "77", "AIM_DEBUG_POISON_LDS": "90"},
                                 {"AIM_CHIP_CUS": "256", "AIM_DEBUG_POISON_LDS": "255"}], ids=["cus1-poison", "cus256-lds255"])
def test_grid_and_poison_identical(tmp_path, env):
    """The same bytes -- the model's -- at AIM_CHIP_CUS 1 and 256 and under the three AIM_DEBUG_POISON_* knobs."""
    if _STATE["failed"]:
        pytest.fail("an earlier GPU step of this module failed: nothing more is started")
    f = str(tmp_path / "k.npz")
    p = child.run("test_directed_index_gpu", "knob_batch", npz=f, env=env, check=False)
    if p.returncode != 0:
        _STATE["failed"] = True
    assert p.returncode == 0, p.stdout + p.stderr
    out = np.load(f)
    for name in d.LARGEST:
        assert isinstance(d.TABLE[name][0]["K"], int)
        for kernel in d.TABLE[name][0]["kernels"]:
            for n, want in zip(NAMES, d.expected(name, kernel, 1024, d.TABLE[name][0]["K"])):
                assert out["%s-%s-%s" % (name, kernel, n)].tobytes() == want.tobytes(), (name, kernel, n, env)
