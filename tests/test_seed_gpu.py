"""Device-side seeding on the GPU. The contract is byte equality with the rule as tests/seed_model.py writes it down: every request,
text_pos, vote and aim_seed_t, the empty slots included -- over short, full-row and empty reads, both strands, edits and N, a strand
that overflows AIM_SEED_MAX_HITS, windows clamped at both ends of the reference, any CU count and poison knob -- and the chain:
the kernel's device buffers go straight into aim_align_device_groups."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import child  # noqa: E402
from gpu_buffers import Hip  # noqa: E402
from pipeline_batches import edge_reads  # noqa: E402

READ_SIZE = 128
# (k, stride, max_occ, band, flank, min_votes, K)
CASES = [(11, 1, 8, 8, 8, 2, 4), (11, 4, 2, 0, 0, 1, 1), (8, 1, 64, 4, 16, 3, 16), (14, 3, 1, 16, 8, 1, 8)]

_DATA = {}


def data():
    """The reference, its model indexes and the 256 reads, made once."""
    if not _DATA:
        import seed_model as m
        ref = m.make_reference()
        rows, rl, true_pos, strand, plain = m.make_reads(ref, 256, READ_SIZE)
        _DATA.update(ref=ref, rows=rows, rl=rl, true_pos=true_pos, strand=strand, plain=plain, index={}, expected={})
    return _DATA


def model_index(k):
    import seed_model as m
    d = data()
    if k not in d["index"]:
        d["index"][k] = m.build_index(d["ref"], k)
    return d["index"][k]


def expected(case, rows=None, rl=None, key=None, idx_base=0):
    """The model's output for a parameter row, computed once per (case, key)."""
    import seed_model as m
    d = data()
    k, stride, max_occ, band, flank, min_votes, K = case
    ck = (case, key, idx_base)
    if ck not in d["expected"]:
        d["expected"][ck] = m.seed(d["rows"] if rows is None else rows, d["rl"] if rl is None else rl, model_index(k), len(d["ref"]), k, stride,
                                   max_occ, band, flank, min_votes, K, READ_SIZE, idx_base=idx_base)
    return d["expected"][ck]


def run_seed(case, rows, rl, idx_base=0):
    """aim_seed_device over buffers uploaded through the HIP runtime the library loaded; the index is the library's own build."""
    from aim_amd import capi, engine
    d = data()
    k, stride, max_occ, band, flank, min_votes, K = case
    sp = engine.seed_params(k, READ_SIZE, stride=stride, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, max_cands=K, idx_base=idx_base)
    bucket, pos = engine.build_index(d["ref"], k, threads=4)
    n = len(rl)
    with Hip() as h:
        d_b, d_p = h.up(bucket), h.up(pos)
        d_rl, d_rows = h.up(np.ascontiguousarray(rl, dtype=np.int32)), h.up(rows, 64)
        d_req, d_tp, d_v, d_s = h.filled(n * K * 16), h.filled(n * K * 8), h.filled(n * K * 4), h.filled(n * 16)
        engine.seed_device(sp, n, d_rl, d_rows, d_b, d_p, len(d["ref"]), d_req, d_tp, d_v, d_s)
        return (h.down(d_req, n * K * 16).view(capi.REQUEST_DTYPE), h.down(d_tp, n * K * 8).view(np.uint64),
                h.down(d_v, n * K * 4).view(np.uint32), h.down(d_s, n * 16).view(capi.SEED_DTYPE))


def assert_equal(got, want):
    for name, g, w in zip(("requests", "text_pos", "votes", "seed"), got, want):
        assert g.tobytes() == w.tobytes(), (name, np.nonzero(g != w)[0][:8])


@pytest.mark.parametrize("case", CASES, ids=["k%d-s%d-occ%d-b%d-f%d-v%d-K%d" % c for c in CASES])
def test_equals_model(case):
    import seed_model as m
    d = data()
    want = expected(case)
    assert set(d["rl"].tolist()) >= {0, 5, 8, 11, 14, 100, READ_SIZE} and set(d["strand"].tolist()) == {0, 1}
    assert (d["rows"] == ord("N")).any()
    if case[0] == 8:        # the reads from inside the tandem repeat: ~93 seeds of 24 positions each overflow the 1 024 kept hits
        assert (want[3]["flags"] & m.TRUNCATED).any() and (want[3]["n_hits"] == m.MAX_HITS).any()
    assert (want[3]["n_cands"] < case[6]).any()                 # empty slots exist ...
    assert (want[3]["n_cands"] > 0).any() and (want[0]["text_len"] > 0).any()
    assert_equal(run_seed(case, d["rows"], d["rl"]), want)


def test_idx_base_and_wraparound():
    """requests[].idx = idx_base + slot, modulo 2^32."""
    d = data()
    case = CASES[0]
    base = 0xFFFFFFF0
    want = expected(case, rows=d["rows"][:32], rl=d["rl"][:32], key="idx", idx_base=base)
    assert want[0]["idx"][0] == base and want[0]["idx"][-1] == (base + 32 * case[6] - 1) % (1 << 32) < base
    assert_equal(run_seed(case, d["rows"][:32], d["rl"][:32], idx_base=base), want)


def test_window_edges():
    """flank 25 reaches past both ends of the reference: start is clamped at 0 and end at ref_len exactly as the model says, and
    aim_ref_windows_check accepts every slot (the empty ones too)."""
    from aim_amd import capi, engine
    ref = data()["ref"]
    rows, rl, starts = edge_reads()
    flank = 25
    case = (11, 1, 8, 8, flank, 2, 4)
    want = expected(case, rows=rows, rl=rl, key="edges")
    req, tpos, votes, seed = want
    first = tpos[0::4] & np.uint64((1 << 63) - 1)
    assert (seed["n_cands"] >= 1).all() and (votes[0::4] >= 90).all()
    assert (first[starts < flank] == 0).all()                                         # clamped at the left edge
    right = starts + 100 + flank > len(ref)
    assert right.any() and (first[right] + req["text_len"][0::4][right].astype(np.uint64) <= len(ref)).all()
    assert (req["text_len"][0::4][right] < 100 + 2 * flank).all() and (req["text_len"][0::4][right] < READ_SIZE).any()   # ... and cut short at the right one
    got = run_seed(case, rows, rl)
    assert_equal(got, want)
    p = engine.make_params("wfa", 20, READ_SIZE, ref_texts=True)
    bad = C.c_uint32(0xFFFFFFFF)
    rc = capi.load().aim_ref_windows_check(capi.params_ref(p), len(got[0]), capi.ptr(got[0]), capi.ptr(got[1]), len(ref), C.byref(bad))
    assert rc == capi.AIM_OK, capi.load().aim_last_error()


def knob_batch():
    d = data()
    out = {}
    for i in (0, 2):           # the default row and the one that overflows
        req, tpos, votes, seed = run_seed(CASES[i], d["rows"], d["rl"])
        out.update({"req%d" % i: req.view(np.uint8), "tpos%d" % i: tpos, "votes%d" % i: votes, "seed%d" % i: seed.view(np.uint8)})
    return out


@pytest.mark.parametrize("env", [{"AIM_CHIP_CUS": "1", "AIM_DEBUG_POISON_SCRATCH": "165", "AIM_DEBUG_POISON_OPS": "77", "AIM_DEBUG_POISON_LDS": "90"},
                                 {"AIM_CHIP_CUS": "256", "AIM_DEBUG_POISON_LDS": "255"}], ids=["cus1-poison", "cus256-lds255"])
def test_grid_and_poison_identical(tmp_path, env):
    """The same bytes -- the model's -- at AIM_CHIP_CUS 1 and 256 and under the three AIM_DEBUG_POISON_* knobs."""
    f = str(tmp_path / "k.npz")
    child.run("test_seed_gpu", "knob_batch", npz=f, env=env)
    out = np.load(f)
    for i in (0, 2):
        req, tpos, votes, seed = expected(CASES[i])
        for key, want in (("req%d" % i, req), ("tpos%d" % i, tpos), ("votes%d" % i, votes), ("seed%d" % i, seed)):
            assert out[key].tobytes() == want.tobytes(), (key, env)


def test_chain_on_device():
    p = child.run("test_seed_gpu", "chain_on_device", cuda_first=True, marker="CHAIN_ON_DEVICE_OK")
    assert "CHAIN_ON_DEVICE_OK" in p.stdout, p.stdout + p.stderr


def chain_on_device():
    """seed_candidates, then aim_align_device_groups (REF_TEXTS | READ_GROUPS | ENDSFREE) on the device tensors it returned: no
    candidate array visits the host in between. The group rows equal those of the same candidates submitted from the host, and every
    error-free read drawn clear of the repeat maps to its slot 0 with score 0."""
    import torch
    from aim_amd import capi, engine
    lib = capi.load()
    d = data()
    ref, n = d["ref"], 64
    rows, rl = np.ascontiguousarray(d["rows"][:n]), d["rl"][:n]
    case = CASES[0]
    k, stride, max_occ, band, flank, min_votes, K = case
    sp = engine.seed_params(k, READ_SIZE, stride=stride, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, max_cands=K)
    out = engine.seed_candidates(sp, engine.build_index(ref, k), len(ref), rl, rows)
    assert_equal((out["req"], out["text_pos"], out["votes"], out["seed"]), expected(case, rows=rows, rl=rl, key="chain"))
    dev = torch.device("cuda:0")
    params = engine.make_params("wfa", 20, READ_SIZE, read_groups=True, ref_texts=True, ends_free=(0, 0, 2 * flank, 2 * flank))
    offs = engine.seed_groups_offsets(n, K)
    d_off = torch.from_numpy(offs.view(np.uint8).copy()).to(dev)
    d_ref = torch.zeros(len(ref) + 64, dtype=torch.uint8, device=dev)
    d_ref[:len(ref)] = torch.from_numpy(ref).to(dev)
    d_res = torch.zeros(n * capi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_best = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    sb = lib.aim_scratch_bytes(capi.params_ref(params), n * K)
    assert sb > 0
    d_scr = torch.zeros(sb, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    engine.align_device_groups(params, n * K, n, out["d_req"].data_ptr(), out["d_reads"].data_ptr(), None, out["d_text_pos"].data_ptr(),
                               d_ref.data_ptr(), len(ref), d_off.data_ptr(), d_res.data_ptr(), None, d_best.data_ptr(), d_scr.data_ptr(), sb)
    torch.cuda.synchronize()
    res, best = d_res.cpu().numpy().view(capi.RESULT_DTYPE), d_best.cpu().numpy().view(capi.BEST_DTYPE)
    with engine.DeviceSet(1) as s:                    # the same candidates, sent from the host
        s.configure_slots(params, n * K, slots=1)
        s.set_reference(ref)
        s.submit(0, 0, out["req"], pat=rows, text_pos=out["text_pos"], read_offsets=offs)
        host = s.wait(0, 0, check=False)
    assert np.array_equal(res, host["res"]) and np.array_equal(best, host["best"])
    plain = np.nonzero(d["plain"][:n])[0]
    assert len(plain) >= 4 and set(d["strand"][plain].tolist()) == {0, 1}
    assert np.array_equal(best["best_pair"][plain], plain.astype(np.uint32) * K) and (best["best_score"][plain] == 0).all()
    assert (res["score"][plain] == 0).all() and (res["status"][plain] == capi.PAIR_OK).all()
