"""Primary / secondary chains and MAPQ on the GPU. The contract is byte equality with rules 8c and 9c as tests/chain_class_model.py
writes them down, over buffers prefilled with 0xEE: chain_class_kernel on the synthetic batch for every group width, mask level and
batch size below, across and beyond one workgroup; read_mapq_kernel on the synthetic selections with and without mates; both on a
grid of eight workgroups and on wider groups than K needs; the classification of the chain kernels' own device buffers (three
short-read rows, the chimeric reads through both chain kernels); and the whole path chain -> classify -> align -> MAPQ."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import child  # noqa: E402
from gpu_buffers import Hip, cached  # noqa: E402
from hand_stages import chain_then_classify  # noqa: E402
from pipeline_batches import READ_SIZE, expected, reference, short_reads  # noqa: E402

KS = (1, 2, 3, 4, 5, 7, 8, 9, 15, 16)  # 7, 9, 15: a group of 8 one lane short, just past it, and a group of 16 one lane short
MASKS = (1, 128, 256)
N_READS = (1, 5, 67, 4099)          # below, across and beyond one workgroup; never a multiple of the reads per wavefront
SHORT_ROWS = [(11, 1, None, 8, 8, 8, 2, 4), (11, 1, 5, 8, 32, 8, 2, 4), (13, 1, 10, 8, 32, 8, 2, 4)]


def synthetic(K):
    import chain_class_model as ccm
    return cached(("syn", K), lambda: ccm.synthetic(1, max(N_READS), K))


def expected_class(K, mask_q8):
    import chain_class_model as ccm
    return cached(("class", K, mask_q8), lambda: ccm.classify(K, ccm.SYN_READ_SIZE, mask_q8, **synthetic(K)))


def prefix(d, n, K):
    return dict(read_len=d["read_len"][:n], text_pos=d["text_pos"][:n * K], seed=d["seed"][:n], chains=d["chains"][:n * K])


def run_classify(h, K, read_size, mask_q8, d):
    """aim_chain_classify_device over uploaded arrays, d_class prefilled with 0xEE."""
    from aim_amd import capi, engine
    n = len(d["read_len"])
    d_cls = h.filled(n * K * 8)
    engine.chain_classify_device(K, read_size, mask_q8, n, h.up(d["read_len"]), h.up(d["text_pos"]), h.up(d["seed"]), h.up(d["chains"]), d_cls)
    return h.down(d_cls, n * K * 8).view(capi.CHAIN_CLASS_DTYPE)


def run_mapq(h, K, score_unit, best, mates, cls):
    from aim_amd import capi, engine
    n = len(best)
    d_out = h.filled(n * 8)
    engine.read_mapq_device(K, n, score_unit, h.up(best), None if mates is None else h.up(mates), h.up(cls), d_out)
    return h.down(d_out, n * 8).view(capi.READ_MAPQ_DTYPE)


def same(got, want):
    assert got.tobytes() == want.tobytes(), np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0][:8]


@pytest.mark.parametrize("mask_q8", MASKS)
@pytest.mark.parametrize("K", KS)
def test_classification_equals_model(K, mask_q8):
    import chain_class_model as ccm
    d, want = synthetic(K), expected_class(K, mask_q8)
    assert (want["flags"] & ccm.SECONDARY).any() or K == 1
    assert (want["flags"] == 0).any() and (want["mapq"] > 0).any()
    with Hip() as h:
        for n in N_READS:
            same(run_classify(h, K, ccm.SYN_READ_SIZE, mask_q8, prefix(d, n, K)), want[:n * K])


def mapq_batch(K, n):
    """(class rows of a synthetic batch, aim_best_t, aim_mate_t) for n reads."""
    import chain_class_model as ccm

    def make():
        cls = ccm.classify(K, ccm.SYN_READ_SIZE, 128, **ccm.synthetic(2, n, K))
        return (cls,) + ccm.synthetic_best(3, n, K)
    return cached(("mapq", K, n), make)


@pytest.mark.parametrize("with_mates", (False, True), ids=("reads", "mates"))
@pytest.mark.parametrize("score_unit", (1, 3, 4))
@pytest.mark.parametrize("K", (1, 2, 4, 7, 8, 9, 16))
def test_read_mapq_equals_model(K, score_unit, with_mates):
    import chain_class_model as ccm
    with Hip() as h:
        for n in (2, 300, 1000):                      # below, across and beyond one workgroup
            cls, best, mates = mapq_batch(K, n)
            want = ccm.read_mapq(K, score_unit, best, mates if with_mates else None, cls)
            if n == 1000:
                assert (want["flags"] & ccm.UNMAPPED).sum() >= 20 and (want["mapq"] > 0).sum() >= 20 and len(set(want["aln_mapq"].tolist())) >= 8
                assert with_mates == bool((want["flags"] & ccm.PROPER).any())
            same(run_mapq(h, K, score_unit, best, mates if with_mates else None, cls), want)


def knob_batch():
    import chain_class_model as ccm
    out = {}
    with Hip() as h:
        for K in (4, 16):
            out["class%d" % K] = run_classify(h, K, ccm.SYN_READ_SIZE, 128, synthetic(K)).view(np.uint8)
        cls, best, mates = mapq_batch(4, 4098)
        out["mapq"] = run_mapq(h, 4, 3, best, mates, cls).view(np.uint8)
    return out


@pytest.mark.parametrize("env", [{"AIM_CHIP_CUS": "1"}, {"AIM_CHIP_CUS": "1", "AIM_CLASS_G": "16"}, {"AIM_CLASS_G": "8"}], ids=["cus1", "cus1-g16", "g8"])
def test_grid_and_group_width_identical(tmp_path, env):
    """The same bytes -- the model's -- when eight workgroups walk the batch (AIM_CHIP_CUS = 1) and when a read of K = 4 gets 8 or 16
    lanes (AIM_CLASS_G)."""
    import chain_class_model as ccm
    f = str(tmp_path / "k.npz")
    p = child.run("test_chain_class_gpu", "knob_batch", npz=f, env=dict(env, AIM_PLAN_DEBUG="1"))
    lanes = int(env.get("AIM_CLASS_G", "4"))
    grids = (8, 8) if "AIM_CHIP_CUS" in env else (-(-4099 // (256 // lanes)), -(-4098 // 256))     # eight workgroups, or one pass
    assert "[aim plan] chain_class_kernel grid=%d block=256 lanes=%d reads=4099 K=4" % (grids[0], lanes) in p.stderr, p.stderr
    assert "[aim plan] read_mapq_kernel grid=%d block=256 reads=4098 K=4 score_unit=3 mates=1" % grids[1] in p.stderr, p.stderr
    out = np.load(f)
    for K in (4, 16):
        assert out["class%d" % K].tobytes() == expected_class(K, 128).tobytes(), (K, env)
    cls, best, mates = mapq_batch(4, 4098)
    assert out["mapq"].tobytes() == ccm.read_mapq(4, 3, best, mates, cls).tobytes(), env


@pytest.mark.parametrize("row", SHORT_ROWS, ids=[str(r) for r in SHORT_ROWS])
def test_short_reads_on_the_device_chain(row):
    import chain_class_model as ccm
    rows, rl = short_reads()[:2]
    req, tpos, votes, seeds, chains = expected(row, rows, rl, "short")
    K = row[7]
    want = ccm.classify(K, READ_SIZE, 128, rl, tpos, seeds, chains)
    assert (want["flags"] & ccm.SECONDARY).sum() >= 10 and (want["flags"] == 0).any()      # (reads of 100 bases have no second part)
    got = chain_then_classify(row, rows, rl, READ_SIZE)
    assert got[1].tobytes() == tpos.tobytes() and got[2].tobytes() == seeds.tobytes() and got[3].tobytes() == chains.tobytes()
    same(got[4], want)


@pytest.mark.parametrize("max_hits", (None, 1024), ids=("seed_chain_device", "seed_chain_long_device"))
def test_chimeric_reads_on_the_device_chain(max_hits):
    import chain_class_model as ccm
    rows, rl = cached("chimeric reads", lambda: ccm.chimeric_reads(reference()))
    K = ccm.CHIMERIC_ROW[7]
    req, tpos, votes, seeds, chains = expected(ccm.CHIMERIC_ROW, rows, rl, "chimeric", read_size=ccm.CHIMERIC_SIZE)
    want = ccm.classify(K, ccm.CHIMERIC_SIZE, 128, rl, tpos, seeds, chains)
    fl = want["flags"].reshape(-1, K)
    assert (((fl & ccm.PRIMARY) != 0).sum(axis=1) >= 2).all() and (((fl & ccm.SECONDARY) != 0) & (want["parent"].reshape(-1, K) != 0)).any()
    got = chain_then_classify(ccm.CHIMERIC_ROW, rows, rl, ccm.CHIMERIC_SIZE, max_hits=max_hits)
    assert got[1].tobytes() == tpos.tobytes() and got[2].tobytes() == seeds.tobytes() and got[3].tobytes() == chains.tobytes()
    same(got[4], want)


def test_whole_path():
    p = child.run("test_chain_class_gpu", "whole_path", cuda_first=True, marker="CHAIN_CLASS_WHOLE_PATH_OK")
    assert "CHAIN_CLASS_WHOLE_PATH_OK" in p.stdout, p.stdout + p.stderr


def whole_path():
    """The reads from inside the planted copies plus the plain reads: seed_chain_candidates, chain_classify, aim_align_device_groups
    with test_seed_chain_gpu's alignment parameters, read_mapq_device. All these reads are error-free (bound 0), and MAX_SCORE is
    10 mismatches + 16: a candidate over the cap counts with MAX_SCORE + 1, which is only a lower bound of its cost, so aln_mapq can
    reach 60 only where the cap lies 10 score units above the winner. The classes equal the model over the chain model, the MAPQ rows
    equal the model over the downloaded aim_best_t; a planted read is ambiguous three ways (MAPQ 0) and a plain read is not
    (MAPQ >= 51, the least chain MAPQ counted on the model)."""
    import torch
    import chain_class_model as ccm
    import seed_model as m
    from aim_amd import capi, engine
    ref = reference()
    srows, srl, _, _, plain = short_reads()
    prows, prl = ccm.planted_reads(ref)
    rows = np.concatenate([prows, srows[plain]])
    rl = np.concatenate([prl, srl[plain]])
    n, n_planted = len(rl), len(prl)
    assert ccm.PLANTED_SIZE == READ_SIZE and n - n_planted >= 20
    row = SHORT_ROWS[0]
    k, stride, w, max_occ, band, flank, min_votes, K = row
    sp = engine.seed_params(k, READ_SIZE, stride=stride, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, max_cands=K)
    out = engine.chain_classify(sp, engine.seed_chain_candidates(sp, engine.build_index(ref, k, threads=4), len(ref), rl, rows))
    req, tpos, votes, seeds, chains = expected(row, rows, rl, "planted+plain")
    assert out["chains"].tobytes() == chains.tobytes() and out["text_pos"].tobytes() == tpos.tobytes()
    want_cls = ccm.classify(K, READ_SIZE, capi.CHAIN_MASK_DEFAULT, rl, tpos, seeds, chains)
    same(out["class"], want_cls)
    x, o, e = 3, 4, 1
    dev = torch.device("cuda:0")
    params = engine.make_params("wfa", 10 * x + 16, READ_SIZE, mismatch=x, gap_o=o, gap_e=e, read_groups=True, ref_texts=True, ends_free=(0, 0, 2 * flank, 2 * flank))
    d_off = torch.from_numpy(engine.seed_groups_offsets(n, K).view(np.uint8).copy()).to(dev)
    d_ref = torch.zeros(len(ref) + 64, dtype=torch.uint8, device=dev)
    d_ref[:len(ref)] = torch.from_numpy(ref).to(dev)
    d_res = torch.zeros(n * capi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
    d_best = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
    d_mapq = torch.full((n * 8,), 0xEE, dtype=torch.uint8, device=dev)
    sb = capi.load().aim_scratch_bytes(capi.params_ref(params), n * K)
    d_scr = torch.zeros(max(sb, 16), dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    engine.align_device_groups(params, n * K, n, out["d_req"].data_ptr(), out["d_reads"].data_ptr(), None, out["d_text_pos"].data_ptr(),
                               d_ref.data_ptr(), len(ref), d_off.data_ptr(), d_res.data_ptr(), None, d_best.data_ptr(), d_scr.data_ptr(), sb)
    engine.read_mapq_device(K, n, x, d_best.data_ptr(), None, out["d_class"].data_ptr(), d_mapq.data_ptr())
    torch.cuda.synchronize()
    best = d_best.cpu().numpy().view(capi.BEST_DTYPE)
    got = d_mapq.cpu().numpy().view(capi.READ_MAPQ_DTYPE)
    print("best", best[:n_planted + 4].tolist())
    print("mapq", got.tolist())
    same(got, ccm.read_mapq(K, x, best, None, want_cls))
    assert (best["best_score"] == 0).all() and (best["n_best"][:n_planted] == 3).all()
    assert (got["flags"] & ~np.uint8(ccm.MAPQ_SECONDARY) == 0).all()            # all mapped; verification may prefer a secondary copy
    assert (got["mapq"][:n_planted] == 0).all() and (got["chain_mapq"][:n_planted] == 0).all() and (got["aln_mapq"][:n_planted] == 0).all()
    assert (got["mapq"][n_planted:] >= 51).all() and (got["slot"][n_planted:] == np.arange(n_planted, n, dtype=np.uint32) * K).all()
