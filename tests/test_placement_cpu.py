"""Arrangements of the full-row batches (tests/placement.py), without a device: the index arrays put the hard pairs into the
slots and 16-lane rows they are meant to reach, the oracle is per pair (which is what entitles tests/test_placement_gpu.py to
gather the oracle's rows of the table batch instead of running it again), fake devices that are wrong in a way the table's own
batch cannot see fail on the arrangement set (and where the table batch does see one, a test says where), and every arrangement
runs on the kernel and shape of its table row."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import full_rows as F
import placement as P
from conftest import GOLDEN, ROOT

N0 = 130
PER_PAIR_ROWS = [("wfa2_red_bt", 88), ("nw_bt", 184), ("swg16_bt", 136), ("wfa5_bt", 72), ("genasm_bt", 64)]


# ------------------------------------------------------------------ the index arrays
def _where(sel, pair):
    at = np.nonzero(sel == pair)[0]
    assert at.size == 1
    return int(at[0])


def test_families_are_what_they_say():
    for n0 in (130, 40, 20):
        rev = P.reversed_sel(n0)
        assert P.is_permutation(rev, n0) and rev[-2:].tolist() == [P.EMPTY_TEXT, P.EMPTY_PATTERN]
        assert set(rev[-F.N_SPECIAL:].tolist()) == set(range(F.N_SPECIAL)) and rev[0] == n0 - 1
        rots = P.rotations(n0)
        assert len({name for name, _ in rots}) == len(rots) and all(P.is_permutation(sel, n0) for _, sel in rots)
        assert rots[0][0] == "rot1" and rots[0][1][:3].tolist() == [n0 - 1, 0, 1]
        for (_, sel), (_, h) in zip(P.hostiles(n0), P.HOSTS):
            assert len(sel) == n0 and (sel[0::2] == h).all() and (sel[1::2] >= F.N_SPECIAL).all() and sel[1] == F.N_SPECIAL
        for (_, sel), (_, p) in zip(P.duplicates(n0), P.DUPLICATES):
            assert len(sel) == n0 and (sel == p).all()
        name, sel = P.tiled(n0)
        assert len(sel) == 8 * n0 and all(P.is_permutation(sel[c * n0:(c + 1) * n0], n0) for c in range(8))
        assert sel[n0 + 11] == 0 and sel[0] == 0
        for u in P.UNITS + (3, 10):
            sizes = P.prefix_sizes(n0, u)
            assert sizes == sorted(set(sizes)) and all(2 <= n < n0 for n in sizes) and {2, n0 - 1} <= set(sizes)
            if u > 1 and u + 1 < n0:
                assert any(n % u == 1 for n in sizes), (n0, u)          # a last unit that holds exactly one pair
            for (name, s), n in zip(P.prefixes(n0, u), sizes):
                assert np.array_equal(s, rev[:n])
    assert [int(s[0]) for _, s in P.singletons()] == [0, 9, 10, F.A_VS_C, F.N_LAST, F.TWIN_A]


def test_arrangement_lists(built):
    """Large and small batches alternate; rows beyond READ_SIZE 2048 take the short list; the list depends on (rs, n0, u) alone."""
    full = P.arrangements(184, 130, 10)
    names = [n for n, _ in full]
    assert names[:4] == ["full", "single_empty_text", "reversed", "single_empty_pattern"] and len(set(names)) == len(names)
    for (_, before), (name, sel) in zip(full, full[1:]):       # a row left unwritten would not hold the right bytes from the launch before
        assert len(sel) > 1 or before[0] != sel[0], name
    assert {"reversed", "hostile_a_vs_c", "hostile_empty_text", "hostile_n_last", "all_twin_a", "all_after_twins", "prefix129", "prefix11",
            "prefix21"} <= set(names)
    assert sum(n.startswith("rot") for n in names) == len(P.ROTATIONS) and sum(n.startswith("single_") for n in names) == 6
    sizes = [len(s) for _, s in full]
    assert all(a == 130 or b == 130 for a, b in zip(sizes, sizes[1:]))
    short = [n for n, _ in P.arrangements(3848, 20, 1)]
    assert sorted(short) == sorted(["full", "reversed", "rot1", "prefix2", "prefix19"] + [n for n, _ in P.singletons()])
    slow = [n for n, _ in P.arrangements(1544, 40, 1, short=True)]
    assert slow == ["full", "prefix2", "reversed", "prefix3", "rot1", "prefix39", "hostile_empty_text", "all_twin_a", "all_after_twins"]
    assert all(row in F.ROWS for row in P.SLOW_ROWS)
    again = P.arrangements(184, 130, 10)
    assert all(a[0] == b[0] and np.array_equal(a[1], b[1]) for a, b in zip(full, again))
    b = F.row_batch(40, "zero")
    req, pat, txt = P.arranged(b, P.reversed_sel(130))
    assert req["idx"].tolist() == list(range(7000, 7130)) and np.array_equal(pat[-1], b[1][P.EMPTY_PATTERN])
    assert req["text_len"][-2] == 0 and req["pattern_len"][-1] == 0 and np.array_equal(txt[0], b[2][129])


@pytest.mark.parametrize("u", P.UNITS)
def test_hosts_reach_both_ends_of_a_unit_and_every_lane_row(u):
    """Over `reversed` and the rotations of a 130-pair batch, by position mod 64: rs/0, 0/rs, A_VS_C and N_LAST each stand in slot 0
    and in slot u - 1 of a unit of u pairs, and in each of the four 16-lane rows of a wavefront."""
    arrs = [("reversed", P.reversed_sel(N0))] + P.rotations(N0)
    for h in P.COVERED:
        lane = np.array([_where(sel, h) for _, sel in arrs]) % 64
        assert {0, u - 1} <= set((lane % u).tolist()), (h, sorted(set((lane % u).tolist())))
        assert set((lane // 16).tolist()) == {0, 1, 2, 3}, h


@pytest.mark.parametrize("n0", [40, 20])
def test_hosts_in_the_smaller_batches(n0):
    """40 and 20 pairs do not fill a wavefront of 64: the hosts still reach every 16-lane row that exists and both ends of every
    unit of up to 8 (40 pairs) or 4 (20 pairs) pairs -- the kernels of these READ_SIZEs have units of 1 to 4."""
    arrs = [("reversed", P.reversed_sel(n0))] + P.rotations(n0)
    for h in P.COVERED:
        lane = np.array([_where(sel, h) for _, sel in arrs])
        assert set((lane // 16).tolist()) == set(range((n0 + 15) // 16)), h
        for u in (1, 2, 3, 4) + ((8,) if n0 == 40 else ()):
            assert {0, u - 1} <= set((lane % u).tolist()), (h, u)


def test_unit_of():
    assert P.unit_of("wfa_group_kernel n=130 grid=72 block=64 G=32 hist=0") == 2
    assert P.unit_of("wfa_group_kernel n=130 G=1 hist=0") == 64 and P.unit_of("wfa_group_kernel n=1 G=64") == 1
    assert P.unit_of("dp_group_kernel n=130 grid=16 lanes_per_pair=6 fb_grid=8") == 10
    assert P.unit_of("dp_group_kernel n=130 lanes_per_pair=45") == 1
    for k in ("nw_reg_kernel", "swg_reg_kernel", "wfa_lane_kernel", "wfa_lane_packed_kernel pack_first=1", "nw_lane_kernel seq_lds=1",
              "swg_lane_kernel seq_lds=0"):
        assert P.unit_of(k + " n=5") == 64
    for k in ("wfa_wave_kernel seq_lds=1", "wfa_bidir_kernel", "dp_wave_kernel wavefronts_per_pair=2", "genasm_wave_kernel",
              "dp_strip_kernel wavefronts_per_pair=2 cells_per_lane=20"):
        assert P.unit_of(k) == 1
    assert set(F.KERNEL_NAMES) == {"wfa_wave_kernel", "wfa_bidir_kernel", "dp_wave_kernel", "dp_strip_kernel", "genasm_wave_kernel",
                                   "wfa_lane_kernel", "wfa_lane_packed_kernel", "nw_lane_kernel", "swg_lane_kernel", "nw_reg_kernel",
                                   "swg_reg_kernel", "wfa_group_kernel", "dp_group_kernel"}


# ------------------------------------------------------------------ the oracle is per pair
def _some(n0, u):
    return [("reversed", P.reversed_sel(n0)), P.rotations(n0)[3], P.hostiles(n0)[0], P.prefixes(n0, u)[-1], P.duplicates(n0)[0],
            P.singletons()[1]]


@pytest.mark.parametrize("fam,rs", PER_PAIR_ROWS, ids=lambda v: str(v))
def test_oracle_is_per_pair(built, fam, rs):
    """The oracle run on an arranged batch gives the gather of its rows of the table batch: `reversed`, a rotation, a hostile
    arrangement, the prefix n0 - 1 (and a duplicate batch and a singleton)."""
    from oracle import oracle
    B = F.row_batch(rs, "zero")
    ores, oops = F.oracle_row(fam, rs, "zero")
    op = F.oracle_params(F.row_params(fam, rs), F.FAMILIES[fam]["algo"])
    for name, sel in _some(len(B[0]), 64):
        req, pat, txt = P.arranged(B, sel)
        res, ops, _ = oracle.align_batch(op, req["pattern_len"], req["text_len"], pat, txt, nthreads=8)
        want = P.expected(ores, oops, sel)
        assert len(res) == len(sel)
        F.compare(res, ops, want[0], want[1], req, oops is not None, idx=False)
        assert np.array_equal(res["begin_offset"], want[0]["begin_offset"]), name


# ------------------------------------------------------------------ fake devices the table batch cannot see
def _empty(req):
    return (req["pattern_len"] == 0) | (req["text_len"] == 0)


def _over_the_cap(fam, rs, res):
    if F.FAMILIES[fam]["algo"] != "wfa":
        return np.zeros(len(res), dtype=bool)
    return res["score"] > F.row_params(fam, rs).max_score


def _with_n(batch):
    req, pat, txt = batch
    col = np.arange(pat.shape[1])[None, :]
    return (((pat == ord("N")) & (col < req["pattern_len"][:, None])) | ((txt == ord("N")) & (col < req["text_len"][:, None]))).any(axis=1)


def _neighbour_takes_the_score(hard, res):
    score = res["score"].copy()
    for p in range(1, len(res)):
        if p % 64 >= 32 and hard[p]:
            res["score"][p - 1] = score[p]


def neighbour_takes_the_score(fam, rs, batch, res, ops):
    """Mutant 1: in the upper half of a wavefront, the pair in front of an empty or over-the-cap pair takes that pair's score."""
    _neighbour_takes_the_score(_empty(batch[0]) | _over_the_cap(fam, rs, res), res)


def neighbour_of_a_todo_pair_takes_the_score(fam, rs, batch, res, ops):
    """Mutant 1 for the pairs a kernel hands to its to-do list whatever the cap: an empty sequence, or a base outside ACGT."""
    _neighbour_takes_the_score(_empty(batch[0]) | _with_n(batch), res)


def single_last_pair_is_not_written(fam, rs, batch, res, ops):
    """Mutant 2: a last unit of 64 that holds exactly one pair leaves its row unwritten."""
    if len(batch[0]) % 64 == 1:
        res[-1] = np.zeros(1, dtype=res.dtype)[0]
        if ops is not None:
            ops[-1] = 0


def _same(req, pat, txt, p, q):
    return np.array_equal(pat[p], pat[q]) and np.array_equal(txt[p], txt[q]) and req["pattern_len"][p] == req["pattern_len"][q] and \
        req["text_len"][p] == req["text_len"][q]


def _swapper(first_lane):
    def mutant(fam, rs, batch, res, ops):
        req = batch[0]
        for p in range(0, len(req) - 1, 2):
            if p % 64 >= first_lane and _same(req, batch[1], batch[2], p, p + 1):
                res[[p, p + 1]] = res[[p + 1, p]]
                if ops is not None:
                    ops[[p, p + 1]] = ops[[p + 1, p]]
    return mutant


# Mutant 3: the rows of positions p and p ^ 1 are swapped when both hold the same sequences. As stated the table batch does see
# it, through idx and at one place only: TWIN_A and TWIN_B stand at 12 and 13 (see test_the_twins_...). Behind the first
# 16-lane row it sees nothing.
twins_are_swapped = _swapper(0)
twins_are_swapped_behind_the_first_lane_row = _swapper(16)
twins_are_swapped_behind_the_first_lane_row.__name__ = "twins_are_swapped_behind_the_first_lane_row"


def _device(fam, rs, sel, mutant):
    """(req, res, ops, expected res, expected ops) of a fake device: the oracle's rows, gathered, numbered like the requests,
    then mutated."""
    B = F.row_batch(rs, "zero")
    ores, oops = F.oracle_row(fam, rs, "zero")
    batch = P.arranged(B, sel) if sel is not None else B
    sel = np.arange(len(B[0])) if sel is None else sel
    eres, eops = P.expected(ores, oops, sel)
    res, ops = eres.copy(), None if eops is None else eops.copy()
    res["idx"] = batch[0]["idx"]
    if mutant is not None:
        mutant(fam, rs, batch, res, ops)
    return batch[0], res, ops, eres, eops


def _caught_by(fam, rs, mutant):
    """Names of the row's arrangements (the GPU module's list) on which compare() fails for the mutant."""
    n0 = F.pairs_for(rs)
    out = []
    for name, sel in P.arrangements(rs, n0, 64):
        req, res, ops, eres, eops = _device(fam, rs, sel, mutant)
        try:
            F.compare(res, ops, eres, eops, req, eops is not None)
        except AssertionError:
            out.append(name)
    return out


MUTANTS = [neighbour_takes_the_score, neighbour_of_a_todo_pair_takes_the_score, single_last_pair_is_not_written,
           twins_are_swapped_behind_the_first_lane_row]
# Where the table batch does see a mutant: at MAX_SCORE 9 and 5 the 2 % body itself has pairs over the cap in the upper half of
# a wavefront, next to pairs under it, so the WFA rows see mutant 1 there (and only there: see the test below).
SEEN_BY_THE_TABLE_BATCH = {(neighbour_takes_the_score, "wfa2_red_bt", 88), (neighbour_takes_the_score, "wfa5_bt", 72)}


@pytest.mark.parametrize("fam,rs", PER_PAIR_ROWS, ids=lambda v: str(v))
def test_the_unmutated_fake_device_passes_everywhere(built, fam, rs):
    assert _caught_by(fam, rs, None) == []
    req, res, ops, eres, eops = _device(fam, rs, None, None)
    assert req["idx"][0] == 5000
    F.compare(res, ops, eres, eops, req, eops is not None)


@pytest.mark.parametrize("mutant,fam,rs", [(m, fam, rs) for fam, rs in PER_PAIR_ROWS for m in MUTANTS if (m, fam, rs) not in SEEN_BY_THE_TABLE_BATCH],
                         ids=lambda v: getattr(v, "__name__", str(v)))
def test_mutants_pass_the_table_batch_and_fail_the_arrangements(built, mutant, fam, rs):
    """Both directions: the fake device passes compare() on the table's own batch -- that is the gap -- and fails it on at least one
    arrangement of the row's list."""
    req, res, ops, eres, eops = _device(fam, rs, None, mutant)
    F.compare(res, ops, eres, eops, req, eops is not None)
    caught = _caught_by(fam, rs, mutant)
    print(fam, rs, mutant.__name__, "caught by", caught)
    assert caught, "the set does not see " + mutant.__name__
    if mutant in (neighbour_takes_the_score, neighbour_of_a_todo_pair_takes_the_score):
        assert any(n.startswith("hostile_") for n in caught)
        # (on the WFA rows the head pairs in front of rs/0, 0/rs and N_LAST are over the cap themselves and have the same score)
        assert F.FAMILIES[fam]["algo"] == "wfa" or any(n.startswith("rot") for n in caught)
    elif mutant is single_last_pair_is_not_written:
        assert {"prefix65", "prefix129"} <= set(caught) and sum(n.startswith("single_") for n in caught) == 6
    else:
        assert {"all_twin_a", "all_after_twins"} <= set(caught)


@pytest.mark.parametrize("mutant,fam,rs", sorted(SEEN_BY_THE_TABLE_BATCH, key=lambda c: c[1]), ids=lambda v: getattr(v, "__name__", str(v)))
def test_where_the_table_batch_sees_mutant_1(built, mutant, fam, rs):
    """On the two WFA rows the table batch fails the mutant, at body pairs alone: every pair whose score it has changed stands in
    front of a body pair over the cap. No constructed pair -- A_VS_C, the empty sequences, N_LAST -- ever stands in the upper half
    of a wavefront there, and the arrangements see the mutant at those too."""
    req, res, ops, eres, eops = _device(fam, rs, None, mutant)
    with pytest.raises(AssertionError, match="score differs"):
        F.compare(res, ops, eres, eops, req, eops is not None)
    changed = np.nonzero(res["score"] != eres["score"])[0]
    assert changed.size and (changed + 1 >= F.N_SPECIAL).all() and ((changed + 1) % 64 >= 32).all()
    caught = _caught_by(fam, rs, mutant)
    assert {"hostile_a_vs_c", "hostile_empty_text"} <= set(caught), caught
    for name, sel in P.arrangements(rs, len(req), 64):
        if name in ("hostile_a_vs_c", "hostile_empty_text"):     # (here every changed pair stands in front of the host)
            areq, ares, _, aeres, _ = _device(fam, rs, sel, mutant)
            at = np.nonzero(ares["score"] != aeres["score"])[0]
            assert at.size and (at % 2 == 1).all() and (at % 64 >= 31).all(), name


@pytest.mark.parametrize("fam,rs", PER_PAIR_ROWS, ids=lambda v: str(v))
def test_the_twins_of_the_table_batch_show_a_swap_by_idx_alone(built, fam, rs):
    """Mutant 3 as stated, from lane 0 on: the table batch sees it at TWIN_A / TWIN_B (positions 12 and 13, one 16-lane row of the
    first unit) and through nothing but idx; the arrangements see it at every position."""
    req, res, ops, eres, eops = _device(fam, rs, None, twins_are_swapped)
    assert np.nonzero(res["idx"] != req["idx"])[0].tolist() == [F.TWIN_A, F.TWIN_B]
    F.compare(res, ops, eres, eops, req, eops is not None, idx=False)
    with pytest.raises(AssertionError, match="idx differs"):
        F.compare(res, ops, eres, eops, req, eops is not None)
    assert {"all_twin_a", "all_after_twins"} <= set(_caught_by(fam, rs, twins_are_swapped))


# ------------------------------------------------------------------ plans
@pytest.fixture(scope="module")
def plans(built):
    env = {k: v for k, v in os.environ.items() if not k.startswith("AIM_") or k == "AIM_LIB"}
    env.update(AIM_SCRATCH_GB="16", AIM_CHIP_CUS="256")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "placement.py"), "--plans"], env=env, capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout)


def test_every_permutation_runs_on_the_rows_own_shape(plans):
    """aim_plan_describe at n0 still names the kernel and shape of the table row, so every arrangement of n0 pairs runs there."""
    assert len(plans) == len(F.ROWS)
    for fam, rs in F.ROWS:
        line = plans["%s/%d" % (fam, rs)][str(F.pairs_for(rs))]
        assert F.plan_matches(line, F.expected_plan(fam, rs)), (fam, rs, line)


def test_the_prefix_sizes_reach_every_kernel(plans):
    names = {line.split()[0] for row in plans.values() for line in row.values()}
    assert names == set(F.KERNEL_NAMES) - {"wfa_bidir_kernel"}, sorted(names)
    for key, row in plans.items():
        assert {"1", "2", str(F.pairs_for(int(key.split("/")[1])) - 1)} <= set(row), key


def test_plans_equal_the_golden(plans):
    """(row, n) -> kernel and shape, as tests/golden/make_placement_plans.py wrote them: a planner change that moves a prefix size
    or a singleton to another kernel shows up here as a diff."""
    want = json.load(open(os.path.join(GOLDEN, "placement_plans.json")))
    moved = ["%s n=%s: golden %r, the planner says %r" % (k, n, want.get(k, {}).get(n), line)
             for k, row in plans.items() for n, line in row.items() if want.get(k, {}).get(n) != line]
    assert not moved, "\n".join(moved[:40])
    assert {k: sorted(v) for k, v in want.items()} == {k: sorted(v) for k, v in plans.items()}
