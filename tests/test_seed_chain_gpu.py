"""Colinear chaining of the seed hits on the GPU. The contract is byte equality with the rule as tests/chain_model.py writes it down:
every request, text_pos, vote, aim_seed_t and aim_chain_t, the empty slots included, over buffers prefilled with 0xEE -- the parameter
rows of both seed sources at read_size 128, long reads with a 60-base deletion at read_size 1 024, rows of 4 096, d_chains = NULL, an
idx_base that wraps, windows clamped at both ends of the reference, any CU count and poison knob -- and the chain on the device: the
kernel's buffers go straight into aim_align_device_groups, and the chained window is the one the read aligns to within the cost of
its edits."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import child  # noqa: E402
from gpu_buffers import Hip  # noqa: E402
from pipeline_batches import (FULL, LONG, LONG_DEL, LONG_EDITS, LONG_SIZE, MINIMIZER, READ_SIZE, case_id, edge_reads, expected, long_reads,  # noqa: E402
                              reference, short_reads)

NAMES = ("requests", "text_pos", "votes", "seed", "chains")


def run_chain(case, rows, rl, read_size=READ_SIZE, idx_base=0, ref=None, chains=True):
    """aim_seed_chain_device over buffers uploaded through the HIP runtime the library loaded, every output prefilled with 0xEE; the
    index is the library's own host build. chains=False passes d_chains = NULL and returns four arrays."""
    from aim_amd import capi, engine
    k, stride, w, max_occ, band, flank, min_votes, K = case
    ref = reference() if ref is None else ref
    sp = engine.seed_params(k, read_size, stride=stride, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, max_cands=K, idx_base=idx_base, w=w)
    bucket, pos = engine.build_index(ref, k, threads=4) if w is None else engine.index_build_minimizers(ref, k, w, threads=4)
    n = len(rl)
    with Hip() as h:
        d_b, d_p = h.up(bucket), h.up(pos)
        d_rl, d_rows = h.up(np.ascontiguousarray(rl, dtype=np.int32)), h.up(np.ascontiguousarray(rows), 64)
        d_req, d_tp, d_v, d_s = h.filled(n * K * 16), h.filled(n * K * 8), h.filled(n * K * 4), h.filled(n * 16)
        d_c = h.filled(n * K * 16) if chains else None
        engine.seed_chain_device(sp, n, d_rl, d_rows, d_b, d_p, len(ref), d_req, d_tp, d_v, d_s, d_c)
        out = (h.down(d_req, n * K * 16).view(capi.REQUEST_DTYPE), h.down(d_tp, n * K * 8).view(np.uint64),
               h.down(d_v, n * K * 4).view(np.uint32), h.down(d_s, n * 16).view(capi.SEED_DTYPE))
        return out + ((h.down(d_c, n * K * 16).view(capi.CHAIN_DTYPE),) if chains else ())


def assert_equal(got, want):
    for name, g, w in zip(NAMES, got, want):
        assert g.tobytes() == w.tobytes(), (name, np.nonzero(g.view(np.uint8) != w.view(np.uint8))[0][:8] // g.dtype.itemsize)


@pytest.mark.parametrize("case", FULL + MINIMIZER, ids=[case_id(c) for c in FULL + MINIMIZER])
def test_equals_model(case):
    import seed_model as m
    rows, rl, _, strand, _ = short_reads()
    want = expected(case, rows, rl, "short")
    K = case[7]
    assert set(rl.tolist()) >= {0, 5, 8, 11, 14, 100, READ_SIZE} and set(strand.tolist()) == {0, 1} and (rows == ord("N")).any()
    if case[0] == 8:        # the reads from inside the tandem repeat overflow the 1 024 kept hits
        assert (want[3]["flags"] & m.TRUNCATED).any() and (want[3]["n_hits"] == m.MAX_HITS).any()
    assert (want[3]["n_cands"] > 0).any() and (want[0]["text_len"] > 0).any() and (want[1] >> np.uint64(63)).any()
    assert (want[3]["n_cands"] < K).any() or K == 1                                       # empty slots exist
    assert (want[4]["n_anchors"] > 1).any() and (want[4]["score"] > case[0]).any()
    assert_equal(run_chain(case, rows, rl), want)


def test_long_reads_equal_model():
    rows, rl, pos, span, strand, clear, deleted = long_reads()
    want = expected(LONG, rows, rl, "long", read_size=LONG_SIZE)
    assert deleted.sum() == 32 and set(strand.tolist()) == {0, 1} and (want[3]["n_hits"].max(axis=1) >= 32).all()
    assert (want[4]["ref_span"][0::4] > want[4]["q_hi"][0::4].astype(np.int64) - want[4]["q_lo"][0::4] + 40)[deleted].sum() >= 24    # chains across the deletion
    assert_equal(run_chain(LONG, rows, rl, read_size=LONG_SIZE), want)


def test_read_size_4096():
    """Rows of 4 096 over the full index and over minimizers: full rows, a long and a short read, both strands, one with N runs."""
    import minimizer_model as mm
    import seed_model as m
    rs = 4096
    rng = np.random.default_rng(6)
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, 40000)].copy()
    rows = np.zeros((6, rs), dtype=np.uint8)
    rl = np.zeros(6, dtype=np.int32)
    for r, L in enumerate((rs, rs, 3001, 40, rs, 11)):
        p = int(rng.integers(0, len(ref) - L))
        read = m.edit(rng, ref[p:p + L], L // 50)[:rs] if r in (1, 2) else ref[p:p + L].copy()
        if r == 4:
            read[100:130] = ord("N")
            read[2000] = ord("N")
        read = m.revcomp(read) if r % 2 else read
        rows[r, :len(read)] = read
        rl[r] = len(read)
    for case in ((11, 4, None, 8, 64, 8, 2, 4), (11, 1, 16, 8, 64, 8, 2, 4)):
        k, w = case[0], case[2]
        index = m.build_index(ref, k) if w is None else mm.build_index(ref, k, w)
        want = expected(case, rows, rl, "rs4096", read_size=rs, ref=ref, index=index)
        assert (want[3]["n_cands"][:5] >= 1).all() and want[3]["n_hits"].max() > 300 and (want[0]["text_len"] == rs).any()
        assert want[4]["q_hi"].max() > 4000 and want[4]["n_anchors"].max() > 300
        assert_equal(run_chain(case, rows, rl, read_size=rs, ref=ref), want)


def test_without_chains():
    """d_chains = NULL: the same requests, text_pos, votes and aim_seed_t."""
    rows, rl = short_reads()[:2]
    for case in (FULL[0], MINIMIZER[0]):
        got = run_chain(case, rows[:96], rl[:96], chains=False)
        assert len(got) == 4
        assert_equal(got, expected(case, rows[:96], rl[:96], "short96")[:4])


def test_idx_base_and_wraparound():
    """requests[].idx = idx_base + slot, modulo 2^32."""
    rows, rl = short_reads()[:2]
    case = FULL[0]
    base = 0xFFFFFFF0
    want = expected(case, rows[:32], rl[:32], "idx", idx_base=base)
    assert want[0]["idx"][0] == base and want[0]["idx"][-1] == (base + 32 * case[7] - 1) % (1 << 32) < base
    assert_equal(run_chain(case, rows[:32], rl[:32], idx_base=base), want)


def test_window_edges():
    """flank 25 reaches past both ends of the reference: start is clamped at 0 and end at ref_len exactly as the model says."""
    ref = reference()
    rows, rl, starts = edge_reads()
    flank = 25
    case = (11, 1, None, 8, 8, flank, 2, 4)
    want = expected(case, rows, rl, "edges")
    req, tpos, votes, seed, chains = want
    first = tpos[0::4] & np.uint64((1 << 63) - 1)
    assert (seed["n_cands"] >= 1).all() and (chains["n_anchors"][0::4] >= 90).all() and (votes[0::4] >= 100).all()
    assert (first[starts < flank] == 0).all()                                         # clamped at the left edge
    right = starts + 100 + flank > len(ref)
    assert right.any() and (first[right] + req["text_len"][0::4][right].astype(np.uint64) <= len(ref)).all()
    assert (req["text_len"][0::4][right] < 100 + 2 * flank).all() and (req["text_len"][0::4][right] < READ_SIZE).any()   # ... and cut short at the right one
    left = starts < flank                      # an error-free read: itself plus what is there of the flanks, capped at the row
    assert (req["text_len"][0::4][left] == np.minimum(starts[left] + 100 + flank, READ_SIZE)).all()
    assert_equal(run_chain(case, rows, rl), want)


KNOB_CASES = (FULL[0], FULL[1], MINIMIZER[0])


def knob_batch():
    rows, rl = short_reads()[:2]
    out = {}
    for i, case in enumerate(KNOB_CASES):          # the default row, the one that overflows and a minimizer row
        for name, arr in zip(NAMES, run_chain(case, rows, rl)):
            out["%s%d" % (name, i)] = arr.view(np.uint8)
    return out


@pytest.mark.parametrize("env", [{"AIM_CHIP_CUS": "1", "AIM_DEBUG_POISON_SCRATCH": "165", "AIM_DEBUG_POISON_OPS": "77", "AIM_DEBUG_POISON_LDS": "90"},
                                 {"AIM_CHIP_CUS": "256", "AIM_DEBUG_POISON_LDS": "255"}], ids=["cus1-poison", "cus256-lds255"])
def test_grid_and_poison_identical(tmp_path, env):
    """The same bytes -- the model's -- at AIM_CHIP_CUS 1 and 256 and under the three AIM_DEBUG_POISON_* knobs."""
    rows, rl = short_reads()[:2]
    f = str(tmp_path / "k.npz")
    child.run("test_seed_chain_gpu", "knob_batch", npz=f, env=env)
    out = np.load(f)
    for i, case in enumerate(KNOB_CASES):
        for name, want in zip(NAMES, expected(case, rows, rl, "short")):
            assert out["%s%d" % (name, i)].tobytes() == want.tobytes(), (name, case, env)


def well_placed():
    """The long reads drawn clear of the planted repeats whose model rank 0 covers their true span: right strand, start at or before
    the first reference base of the read, end at or after its last."""
    rows, rl, pos, span, strand, clear, deleted = long_reads()
    req, tpos, votes, seed, chains = expected(LONG, rows, rl, "long", read_size=LONG_SIZE)
    start = (tpos[0::4] & np.uint64((1 << 63) - 1)).astype(np.int64)
    minus = (tpos[0::4] >> np.uint64(63)).astype(np.int64)
    end = start + req["text_len"][0::4]
    return clear & (seed["n_cands"] >= 1) & (minus == strand) & (start <= pos) & (end >= pos + span)


def test_long_reads_are_well_placed_by_the_model():
    """On the CPU, from the model alone: at least 56 of the 64 long reads are in the set test_chain_on_device checks."""
    assert well_placed().sum() >= 56


def test_chain_on_device():
    p = child.run("test_seed_chain_gpu", "chain_on_device", cuda_first=True, marker="SEED_CHAIN_ON_DEVICE_OK")
    assert "SEED_CHAIN_ON_DEVICE_OK" in p.stdout, p.stdout + p.stderr


def chain_on_device():
    """seed_chain_candidates over the long reads, then aim_align_device_groups (REF_TEXTS | READ_GROUPS | ENDSFREE with 2 * flank of
    free text at both ends) on the device tensors it returned. The rows equal those of the same candidates submitted from the host,
    and every well-placed read maps to its slot 0 within the cost of the alignment its edits define: each of the n_edits sequential
    edits is one substitution, insertion or deletion, at most max(x, o + e), plus o + 60 e for the planted deletion."""
    import torch
    from aim_amd import capi, engine
    lib = capi.load()
    ref, n = reference(), 64
    rows, rl, pos, span, strand, clear, deleted = long_reads()
    k, stride, w, max_occ, band, flank, min_votes, K = LONG
    sp = engine.seed_params(k, LONG_SIZE, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, max_cands=K, w=w)
    out = engine.seed_chain_candidates(sp, engine.index_build_minimizers(ref, k, w), len(ref), rl, rows)
    assert_equal((out["req"], out["text_pos"], out["votes"], out["seed"], out["chains"]), expected(LONG, rows, rl, "long", read_size=LONG_SIZE))
    x, o, e = 3, 4, 1
    bound = LONG_EDITS * max(x, o + e) + np.where(deleted, o + LONG_DEL * e, 0)
    dev = torch.device("cuda:0")
    params = engine.make_params("wfa", int(bound.max()) + 16, LONG_SIZE, mismatch=x, gap_o=o, gap_e=e, read_groups=True, ref_texts=True,
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
    good = np.nonzero(well_placed())[0]
    assert len(good) >= 56 and set(strand[good].tolist()) == {0, 1} and deleted[good].any() and (~deleted[good]).any()
    print("scores", best["best_score"][good].tolist(), "bounds", bound[good].tolist())
    assert np.array_equal(best["best_pair"][good], good.astype(np.uint32) * K)
    assert (best["best_score"][good] <= bound[good]).all() and (best["best_score"][good] >= 0).all()
    assert (res["status"][good] == capi.PAIR_OK).all()
