"""aim_seed_chain_long_device on the GPU. The contract is byte equality with the rule as tests/chain_long_model.py writes it down:
every request, text_pos, vote, aim_seed_t and aim_chain_t, the empty slots included, over buffers prefilled with 0xEE. The batches
(tests/chain_long_batches.py) are the places where the kernel's widths and its tiled hit phase can go wrong: the old kernel's own
batch (A: the same bytes as aim_seed_chain_device), more than 1 024 anchors and query offsets beyond 12 bits (B), chain scores beyond
13 and 14 bits (C, D), the largest cap, a truncated strand and the largest read_size (D), repeats that truncate at a small cap (E),
w = 1 (F), read lengths around the tile seams with N runs across them (G), d_chains = NULL, an idx_base that wraps and windows clamped
at both ends of the reference (H), any CU count and poison knob (I), and the chain on the device into aim_align_device_groups (J)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import child  # noqa: E402
from gpu_buffers import Hip  # noqa: E402

NAMES = ("requests", "text_pos", "votes", "seed", "chains")
_STATE = {"failed": False}


@pytest.fixture(autouse=True)
def _feature():
    """A library without AIM_FEATURE_SEED_CHAIN_LONG fails every test here."""
    from aim_amd import capi, engine
    assert engine.features() & capi.FEATURE_SEED_CHAIN_LONG and hasattr(capi.load(), "aim_seed_chain_long_device")


def run_long(case, rows, rl, ref, idx_base=0, chains=True, old=False):
    """aim_seed_chain_long_device over buffers uploaded through the HIP runtime the library loaded, every output prefilled with 0xEE;
    the index is the library's own host build. chains=False passes d_chains = NULL and returns four arrays. old=True also runs
    aim_seed_chain_device over the same input buffers into outputs of its own and returns (long, old). Once a step has failed, no
    later one starts."""
    if _STATE["failed"]:
        pytest.fail("an earlier GPU step of this module failed: nothing more is started")
    _STATE["failed"] = True
    from aim_amd import capi, engine
    k, w, max_occ, band, flank, min_votes, K, H, read_size = case
    sp = engine.seed_params(k, read_size, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, max_cands=K, idx_base=idx_base, w=w,
                            long_reads=True)
    bucket, pos = engine.index_build_minimizers(ref, k, w, threads=4)
    n = len(rl)
    with Hip() as h:
        d_b, d_p = h.up(bucket), h.up(pos)
        d_rl, d_rows = h.up(np.ascontiguousarray(rl, dtype=np.int32)), h.up(np.ascontiguousarray(rows), 64)

        def outputs():
            return [h.filled(n * K * 16), h.filled(n * K * 8), h.filled(n * K * 4), h.filled(n * 16), h.filled(n * K * 16) if chains else None]

        def down(d):
            out = (h.down(d[0], n * K * 16).view(capi.REQUEST_DTYPE), h.down(d[1], n * K * 8).view(np.uint64),
                   h.down(d[2], n * K * 4).view(np.uint32), h.down(d[3], n * 16).view(capi.SEED_DTYPE))
            return out + ((h.down(d[4], n * K * 16).view(capi.CHAIN_DTYPE),) if chains else ())
        d = outputs()
        engine.seed_chain_long_device(sp, H, n, d_rl, d_rows, d_b, d_p, len(ref), *d)
        got = down(d)
        if old:
            d2 = outputs()
            engine.seed_chain_device(sp, n, d_rl, d_rows, d_b, d_p, len(ref), *d2)
            got = (got, down(d2))
        _STATE["failed"] = False
        return got


def assert_equal(got, want):
    for name, g, w in zip(NAMES, got, want):
        assert g.tobytes() == w.tobytes(), (name, np.nonzero(g.view(np.uint8) != w.view(np.uint8))[0][:8] // g.dtype.itemsize)


def check(case, b, key, tandem=False):
    import chain_long_batches as lb
    want = lb.expected(case, b, key, tandem=tandem)
    assert_equal(run_long(case, b["rows"], b["rl"], lb.reference(tandem)), want)
    return want


# ---- A: the same bytes as the old kernel ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("row", [0, 1])
def test_a_same_bytes_as_seed_chain_device(row):
    import chain_long_model as clm
    import minimizer_model as mm
    import seed_model as m
    import pipeline_batches as old
    k, stride, w, max_occ, band, flank, min_votes, K = old.MINIMIZER[row]
    ref = old.reference()
    rows, rl = old.short_reads()[:2]
    assert len(rl) == 256 and rows.shape[1] == 128
    want = clm.seed_chain_long(rows, rl, mm.build_index(ref, k, w), len(ref), k, w, max_occ, band, flank, min_votes, K, 128, 1024)
    assert (want[3]["n_cands"] > 0).any() and (want[3]["n_cands"] < K).any() and (want[4]["n_anchors"] > 1).any()
    got, got_old = run_long((k, w, max_occ, band, flank, min_votes, K, 1024, 128), rows, rl, ref, old=True)
    assert_equal(got, want)
    assert_equal(got, got_old)


# ---- B .. F ---------------------------------------------------------------------------------------------------------------------
def test_b_more_than_1024_anchors_offsets_beyond_12_bits():
    import chain_long_batches as lb
    want = check(lb.CASE_B, lb.batch_b(), "B")
    assert (want[3]["n_hits"].max(axis=1) > 1024).all() and not want[3]["flags"].any() and (want[4]["q_hi"][0::4] > 4096).all()


def test_c_large_chain_scores():
    import chain_long_batches as lb
    want = check(lb.CASE_C, lb.batch_c(), "C")
    assert want[4]["score"].max() > 8191 and want[4]["n_anchors"].max() > 2048


def test_d_limits_three_long_reads():
    import chain_long_batches as lb
    want = check(lb.CASE_D1, lb.batch_d1(), "D1")
    assert (want[3]["n_hits"].max(axis=1) > 4096).all() and want[4]["score"].max() > 16383 and want[4]["q_hi"].max() > 65000


def test_d_limits_truncated_at_8192():
    import chain_long_batches as lb
    want = check(lb.CASE_D2, lb.batch_d2(), "D2")
    assert (want[3]["n_hits"].max(axis=1) == 8192).all() and (want[3]["flags"] == 1).all()


def test_d_limits_read_size_65528():
    import chain_long_batches as lb
    b = lb.batch_d3()
    want = check(lb.CASE_D3, b, "D3")
    assert b["rl"][0] == 65528 == lb.CASE_D3[8] and want[3]["n_cands"][0] >= 1 and want[4]["q_hi"][0] > 65000


def test_e_repeats_truncate_at_a_small_cap():
    import chain_long_batches as lb
    want = check(lb.CASE_E, lb.batch_e(), "E", tandem=True)
    assert (want[3]["flags"][1::2] == 1).all() and not want[3]["flags"][0::2].any()


def test_f_every_kmer_is_a_seed():
    import chain_long_batches as lb
    want = check(lb.CASE_F, lb.batch_f(), "F")
    assert (want[3]["n_hits"].max(axis=1) > 3000).all() and not want[3]["flags"].any()


# ---- G: tile seams --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [32, 2])
def test_g_tile_seams(w):
    import chain_long_batches as lb
    b = lb.batch_g()
    T = lb.tile()
    assert set(range(T - 40, T + 41)) | set(range(2 * T - 40, 2 * T + 41)) | {0, 10, 11, 3 * T} == set(b["rl"].tolist())
    want = check(lb.case_g(w), b, "G%d" % w)
    assert (want[3]["n_cands"] >= 1).sum() >= len(b["rl"]) - 4


# ---- H: d_chains, idx_base, window edges ----------------------------------------------------------------------------------------
def test_h_without_chains():
    import chain_long_batches as lb
    b = lb.batch_b()
    got = run_long(lb.CASE_B, b["rows"], b["rl"], lb.reference(), chains=False)
    assert len(got) == 4
    assert_equal(got, lb.expected(lb.CASE_B, b, "B")[:4])


def test_h_idx_base_wraps():
    import chain_long_batches as lb
    b = lb.batch_b()
    base = 0xFFFFFFF0
    want = lb.expected(lb.CASE_B, b, "B", idx_base=base)
    assert want[0]["idx"][0] == base and want[0]["idx"][-1] == (base + 8 * 4 - 1) % (1 << 32) < base
    assert_equal(run_long(lb.CASE_B, b["rows"], b["rl"], lb.reference(), idx_base=base), want)


def test_h_window_edges():
    """flank 150 reaches past both ends of the reference: start is clamped at 0 and end at ref_len exactly as the model says."""
    import chain_long_batches as lb
    b = lb.batch_h()
    want = check(lb.CASE_H, b, "H")
    req, tpos = want[0], want[1]
    start = (tpos[0::4] & np.uint64((1 << 63) - 1)).astype(np.int64)
    assert (want[3]["n_cands"] >= 1).all() and (start[:2] == 0).all()
    assert (start[2:] + req["text_len"][0::4][2:] <= lb.REF_LEN).all() and start[2] + req["text_len"][0::4][2] == lb.REF_LEN


# ---- I: grid and poison ---------------------------------------------------------------------------------------------------------
def knob_batch():
    import chain_long_batches as lb
    out = {}
    for i, (case, b, tandem) in enumerate(((lb.CASE_B, lb.batch_b(), False), (lb.CASE_E, lb.batch_e(), True))):
        for name, arr in zip(NAMES, run_long(case, b["rows"], b["rl"], lb.reference(tandem))):
            out["%s%d" % (name, i)] = arr.view(np.uint8)
    return out


@pytest.mark.parametrize("env", [{"AIM_CHIP_CUS": "1", "AIM_DEBUG_POISON_SCRATCH": "165", "AIM_DEBUG_POISON_OPS": "77", "AIM_DEBUG_POISON_LDS": "90"},
                                 {"AIM_CHIP_CUS": "256", "AIM_DEBUG_POISON_LDS": "255"}], ids=["cus1-poison", "cus256-lds255"])
def test_i_grid_and_poison_identical(tmp_path, env):
    """The same bytes -- the model's -- at AIM_CHIP_CUS 1 and 256 and under the three AIM_DEBUG_POISON_* knobs."""
    import chain_long_batches as lb
    if _STATE["failed"]:
        pytest.fail("an earlier GPU step of this module failed: nothing more is started")
    f = str(tmp_path / "k.npz")
    p = child.run("test_seed_chain_long_gpu", "knob_batch", npz=f, env=env, check=False)
    if p.returncode != 0:
        _STATE["failed"] = True
    assert p.returncode == 0, p.stdout + p.stderr
    out = np.load(f)
    for i, (case, b, key, tandem) in enumerate(((lb.CASE_B, lb.batch_b(), "B", False), (lb.CASE_E, lb.batch_e(), "E", True))):
        for name, want in zip(NAMES, lb.expected(case, b, key, tandem=tandem)):
            assert out["%s%d" % (name, i)].tobytes() == want.tobytes(), (name, case, env)


# ---- J: the chain on the device -------------------------------------------------------------------------------------------------
def test_j_chain_on_device():
    if _STATE["failed"]:
        pytest.fail("an earlier GPU step of this module failed: nothing more is started")
    p = child.run("test_seed_chain_long_gpu", "chain_on_device", cuda_first=True, marker="SEED_CHAIN_LONG_ON_DEVICE_OK", check=False)
    if p.returncode != 0:
        _STATE["failed"] = True
    assert p.returncode == 0 and "SEED_CHAIN_LONG_ON_DEVICE_OK" in p.stdout, p.stdout + p.stderr


def chain_on_device():
    """seed_chain_long_candidates over batch B, then aim_align_device_groups (REF_TEXTS | READ_GROUPS | ENDSFREE with 2 * flank of free
    text at both ends) on the device tensors it returned. The rows equal those of the same candidates submitted from the host, and
    every well-placed read maps to its slot 0 within the cost of the alignment its edits define: each of the 80 sequential edits is one
    substitution, insertion or deletion, at most max(x, o + e), plus o + 200 e for the planted deletion."""
    import torch
    import chain_long_batches as lb
    from aim_amd import capi, engine
    lib = capi.load()
    ref, b = lb.reference(), lb.batch_b()
    rows, rl, strand, deleted = b["rows"], b["rl"], b["strand"], b["deleted"]
    k, w, max_occ, band, flank, min_votes, K, H, read_size = lb.CASE_B
    n = len(rl)
    sp = engine.seed_params(k, read_size, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, max_cands=K, w=w, long_reads=True)
    out = engine.seed_chain_long_candidates(sp, H, engine.index_build_minimizers(ref, k, w), len(ref), rl, rows)
    assert_equal((out["req"], out["text_pos"], out["votes"], out["seed"], out["chains"]), lb.expected(lb.CASE_B, b, "B"))
    x, o, e = 3, 4, 1
    bound = lb.B_EDITS * max(x, o + e) + np.where(deleted, o + lb.B_DEL * e, 0)
    dev = torch.device("cuda:0")
    params = engine.make_params("wfa", int(bound.max()) + 16, read_size, mismatch=x, gap_o=o, gap_e=e, read_groups=True, ref_texts=True,
                                ends_free=(0, 0, 2 * flank, 2 * flank))
    offs = engine.seed_groups_offsets(n, K)
    d_off = torch.from_numpy(offs.view(np.uint8).copy()).to(dev)
    d_ref = torch.zeros(len(ref) + 64, dtype=torch.uint8, device=dev)
    d_ref[:len(ref)] = torch.from_numpy(ref).to(dev)
    d_res = torch.zeros(n * capi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_best = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    sb = lib.aim_scratch_bytes(capi.params_ref(params), n * K)
    d_scr = torch.zeros(max(sb, 16), dtype=torch.uint8, device=dev)
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
    good = np.nonzero(lb.well_placed(lb.CASE_B, b, "B"))[0]
    assert len(good) >= 7 and set(strand[good].tolist()) == {0, 1} and deleted[good].any() and (~deleted[good]).any()
    print("scores", best["best_score"][good].tolist(), "bounds", bound[good].tolist())
    assert np.array_equal(best["best_pair"][good], good.astype(np.uint32) * K)
    assert (best["best_score"][good] <= bound[good]).all() and (best["best_score"][good] >= 0).all()
    assert (res["status"][good] == capi.PAIR_OK).all()
