"""The batch-I/O and read-groups launchers (batch_io.hpp, groups.hpp, hits.hpp, mates.hpp) own their grid, block and store-width
arithmetic. Each path that goes through one runs here through the public C ABI at 1, 63, 65 and 257 rows -- the edges of the 64- and
256-thread workgroups -- and at two READ_SIZEs, 112 (a multiple of 16: 16-byte stores in the row gathers) and 120 (a multiple of 8
only: 8-byte stores). The plain batches are compared with the oracle; the groups batches with the comparison of their own GPU tests
(the flag-less run of every candidate, itself an oracle-checked path, indexed by the host model of the selection). For the mate-pairs
batch the sizes count read pairs (a batch of an odd number of reads is refused)."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

SIZES = [1, 63, 65, 257]
READ_SIZES = [112, 120]
L, ERR = 100, 0.01


def _oracle_text(algo, params, req, pat, txt):
    import test_gpu_parity as gp
    return gp._oracle_text(algo, params, req, pat, txt)


def _wfa(rs, **kw):
    from aim_amd import engine
    return engine.make_params("wfa", engine.launcher_sizes("wfa", L, ERR)[0], rs, **kw)


@pytest.mark.parametrize("rs", READ_SIZES)
@pytest.mark.parametrize("n", SIZES)
def test_ascii_batch_with_the_compact_cigar(n, rs):
    """cigar_rle_kernel behind the alignment of ASCII rows."""
    from aim_amd import engine
    req, pat, txt = engine.gen_pairs(41, 0, n, L, ERR, rs)
    params = _wfa(rs, backtrace=True)
    ores, want = _oracle_text("wfa", params, req, pat, txt)
    with engine.DeviceSet(1) as s:
        s.configure_slots(params, n, slots=1, max_runs=2 * rs * n)
        s.submit(0, 0, req, pat, txt, cigar_runs_cap=2 * rs * n)
        out = s.wait(0, 0, check=False)
    assert np.array_equal(out["cig"]["score"], ores["score"])
    assert int(out["cig"]["n_runs"].sum()) == len(out["runs"])
    assert engine.format_output_runs(out["cig"], out["runs"]) == want


@pytest.mark.parametrize("rs", READ_SIZES)
@pytest.mark.parametrize("n", SIZES)
def test_packed_batch_expanded_with_one_raw_pair(n, rs):
    """unpack_rows_kernel and scatter_raw_rows_kernel: NW has no kernel that reads packed rows, so the batch is expanded first."""
    from aim_amd import engine
    req, pat, txt = engine.gen_pairs(42, 0, n, L, 0.02, rs)
    pat[n // 2, 3] = ord("N")
    params = engine.make_params("nw", engine.launcher_sizes("nw", L, 0.02)[0], rs, backtrace=True)
    ores, want = _oracle_text("nw", params, req, pat, txt)
    packed = engine.pack_batch(req, pat, txt)
    assert packed[2].tolist() == [n // 2]
    with engine.DeviceSet(1) as s:
        s.configure_slots(params, n, slots=1, max_raw=n)
        s.submit(0, 0, req, packed=packed, want_ops=True)
        out = s.wait(0, 0, check=False)
    assert np.array_equal(out["res"]["score"], ores["score"])
    assert engine.format_output(out["res"], out["ops"], True) == want


@pytest.mark.parametrize("rs", READ_SIZES)
@pytest.mark.parametrize("n", SIZES)
def test_packed_batch_on_the_fused_kernel_with_the_raw_side_pass(n, rs):
    """gather_elems_kernel and scatter_elems_kernel (and cigar_rle_kernel over the side list): a packed batch whose kernel reads the
    packed rows itself, one raw pair, compact CIGAR and result rows + ops rows out of the same submit."""
    from aim_amd import engine
    req, pat, txt = engine.gen_pairs(43, 0, n, L, ERR, rs)
    pat[n // 2, 5] = ord("N")
    params = _wfa(rs, backtrace=True)
    ores, want = _oracle_text("wfa", params, req, pat, txt)
    packed = engine.pack_batch(req, pat, txt)
    with engine.DeviceSet(1) as s:
        s.configure_slots(params, n, slots=1, max_raw=n, max_runs=2 * rs * n)
        s.submit(0, 0, req, packed=packed, cigar_runs_cap=2 * rs * n, want_ops=True)
        out = s.wait(0, 0, check=False)
        plan = s.plan_describe(0)
    print(plan)
    assert np.array_equal(out["res"]["score"], ores["score"]) and np.array_equal(out["cig"]["score"], ores["score"])
    assert engine.format_output(out["res"], out["ops"], True) == want
    assert engine.format_output_runs(out["cig"], out["runs"]) == want


@pytest.mark.parametrize("rs", READ_SIZES)
@pytest.mark.parametrize("n", SIZES)
def test_packed_ref_texts_batch_with_an_n_window(n, rs):
    """gather_text_packed_kernel, gather_todo_rows_kernel and cigar_rle_todo_kernel (READ_SIZE 112: the fused lane kernel keeps the
    batch), or gather_text_rows_kernel behind unpack_rows_kernel where the planner has no packed kernel for the READ_SIZE. One
    window holds an N; with more than one pair, one pattern does too and travels on the raw side list (gather_text_rows_kernel over
    the side list)."""
    import test_ref_texts_gpu as rt
    from aim_amd import engine
    ref = rt.make_reference(44, 100000, specials=False)
    req, pat, tpos, txt = engine.ref_pairs(44, 0, n, L, ERR, ref, rs, minus_fraction=0.5)
    p0 = int(tpos[0]) & ((1 << 63) - 1)
    ref[p0 + 9] = ord("N")
    txt = rt.texts_of(ref, req, tpos, rs)
    assert ord("N") in txt[0, :int(req["text_len"][0])]
    if n > 1:
        pat[n - 1, 5] = ord("N")
    params = _wfa(rs, backtrace=True, ref_texts=True)
    ores, want = _oracle_text("wfa", _wfa(rs, backtrace=True), req, pat, txt)
    with engine.DeviceSet(1) as s:
        s.configure_slots(params, n, slots=1, max_raw=n, max_runs=2 * rs * n)
        s.set_reference(ref)
        s.submit(0, 0, req, packed=engine.pack_batch(req, pat, None), cigar_runs_cap=2 * rs * n, text_pos=tpos)
        out = s.wait(0, 0, check=False)
        plan = s.plan_describe(0)
    print(plan)
    if rs == 112:
        assert plan.startswith("wfa_lane_packed_kernel"), plan
    assert np.array_equal(out["cig"]["score"], ores["score"])
    assert engine.format_output_runs(out["cig"], out["runs"]) == want


@pytest.mark.parametrize("rs", READ_SIZES)
@pytest.mark.parametrize("n", SIZES)
def test_ref_texts_rows_gathered_for_an_ascii_batch(n, rs):
    """gather_text_rows_kernel at both store widths, both strands."""
    import test_ref_texts_gpu as rt
    from aim_amd import engine
    ref = rt.make_reference(45, 100000)
    req, pat, tpos, txt = engine.ref_pairs(45, 0, n, L, ERR, ref, rs, minus_fraction=0.5)
    params = _wfa(rs, backtrace=True, ref_texts=True)
    ores, want = _oracle_text("wfa", _wfa(rs, backtrace=True), req, pat, txt)
    res, ops = engine.align(params, req, pat, None, check=False, reference=ref, text_pos=tpos)
    assert engine.format_output(res, ops, True) == want


@pytest.mark.parametrize("rs", READ_SIZES)
@pytest.mark.parametrize("n_mates", SIZES)
def test_groups_batch_with_backtrace_and_mates(n_mates, rs):
    """group_map, group_rows (read -> candidates, winners -> pass 2), group_select, mate_select, gather_elems, cigar_rle."""
    import test_mate_pairs_gpu as tm
    from aim_amd import engine
    ms = engine.launcher_sizes("wfa", L, ERR)[0]
    kw = dict(backtrace=True)
    ref, req, rows, offs, tpos, txt, pats, truth = engine.mate_pairs(46, n_mates, L, ERR, 400, 4, tm.REPEAT_FRAC, read_size=rs)
    runs_cap = 64 * len(req)
    mates = (tm.SPANS[0], tm.SPANS[1], 2 * (ms + 1))
    exp = tm.expected("wfa", ms, rs, kw, req, pats, txt, offs, tpos, mates, runs_cap=runs_cap)
    got = tm.run_mates(engine.make_params("wfa", ms, rs, read_groups=True, ref_texts=True, mate_pairs=True, **kw), req, rows, offs, tpos, ref, mates,
                       runs_cap=runs_cap)
    assert got["plan"].endswith(" groups=1 mates=1")
    tm.assert_mates_equal(got, exp, True, True)


@pytest.mark.parametrize("rs", READ_SIZES)
@pytest.mark.parametrize("n_reads", SIZES)
def test_groups_batch_with_backtrace_and_hits(n_reads, rs):
    """... and hit_select_kernel, whose grid is group_select_kernel's; the rows behind the selection are hits."""
    import test_read_groups_gpu as rg
    import test_top_hits_gpu as th
    from aim_amd import engine
    ms = engine.launcher_sizes("wfa", L, 0.02)[0]
    kw = dict(backtrace=True)
    ref = rg.make_reference(47, 200000)
    sizes = np.random.default_rng(47 + n_reads).integers(1, 9, size=n_reads)
    req, rows, offs, tpos, txt, pats = engine.group_pairs(47, 0, n_reads, 8, L, 0.02, ref, rs, sizes=sizes)
    runs_cap = 64 * len(req)
    exp = th.expected(("launchers", n_reads, rs), "wfa", ms, rs, kw, req, pats, txt, offs, runs_cap=runs_cap)
    got = th.run_hits(engine.make_params("wfa", ms, rs, read_groups=True, top_hits=True, ref_texts=True, **kw), 3, req, rows, offs, tpos=tpos, ref=ref,
                      runs_cap=runs_cap)
    assert got["plan"].endswith(" groups=1 hits=1")
    th.assert_hits_equal(got, exp, offs, 3, True, True)


@pytest.mark.parametrize("rs", READ_SIZES)
@pytest.mark.parametrize("n", SIZES)
def test_escalate_batch_reaches_its_second_stage(n, rs):
    """escalate_select_kernel and escalate_list_kernel: every pair is a tail pair, so the list holds the pairs over the first cap."""
    from aim_amd import engine
    from oracle import oracle
    ms = 25
    req, pat, txt, tail = engine.mixed_pairs(48, n, L, 0.01, 0.05, 1.0, rs)
    res, ops = engine.align(engine.make_params("wfa", ms, rs, escalate=True, backtrace=True), req, pat, txt)
    ores, oops, worst = oracle.align_batch(oracle.params("wfa", ms, rs, backtrace=True), req["pattern_len"], req["text_len"], pat, txt, nthreads=4)
    assert worst == 0
    assert np.array_equal(res["score"], ores["score"])
    assert (ores["score"] > 10).any()          # the first stage's cap (test_escalate_gpu: escalate=10 at these penalties) left work for the second
    assert engine.format_output(res, ops, True) == oracle.format_output(ores, oops, True)
