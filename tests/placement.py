"""Arrangements of a full-row batch (tests/full_rows.py): the same pairs in other places. Plain numpy, no device.

Every alignment entry point promises that a result row depends on its own pair alone, while the kernels put 64 / G, 64 / lanes or
64 pairs into a wavefront, reduce across lanes, reuse LDS slots and scratch from unit to unit and re-plan every batch at its own
pair count. The row batches keep their hard pairs at positions 0 .. 16, so every row of the table sees them in the same lanes of
the first unit. An arrangement is (name, sel): `sel` holds positions into a table row's batch B = full_rows.row_batch(rs, pad), and
since the oracle is per pair (tests/test_placement_cpu.py shows it) the expected rows are the same gather of the oracle's rows of
B. Nothing here makes a new input: every pair is one the table already runs."""
import re

import numpy as np

import full_rows as F

# 1 .. 59 move the head through the four 16-lane rows of a wavefront; 47, 49, 53 and 54 are there so that, together with
# `reversed`, each of COVERED stands once in the first and once in the last lane of a wavefront (positions 0 and 63 mod 64), which
# is slot 0 and slot u - 1 of a unit for every unit size u (tests/test_placement_cpu.py checks it)
ROTATIONS = (1, 5, 16, 27, 32, 48, 59, 47, 49, 53, 54)
EMPTY_TEXT, EMPTY_PATTERN = 9, 10                                  # head pairs rs/0 and 0/rs
SINGLETONS = (("rs_rs", 0), ("empty_text", EMPTY_TEXT), ("empty_pattern", EMPTY_PATTERN), ("a_vs_c", F.A_VS_C), ("n_last", F.N_LAST),
              ("twin_a", F.TWIN_A))
# the hosts of the hostile-neighbour arrangements: over the cap on WFA and all mismatches elsewhere; an empty text (dp_group's
# to-do list); non-ACGT (the WFA kernels' to-do list)
HOSTS = (("a_vs_c", F.A_VS_C), ("empty_text", EMPTY_TEXT), ("n_last", F.N_LAST))
COVERED = (EMPTY_TEXT, EMPTY_PATTERN, F.A_VS_C, F.N_LAST)          # the pairs test_placement_cpu.py follows through slots and rows
DUPLICATES = (("twin_a", F.TWIN_A), ("after_twins", F.AFTER_TWINS))
UNITS = (1, 2, 4, 8, 16, 32, 64)
TILED_MAX_RS = 320
TILED_COPIES = 8
LONG_RS = 2048                                                    # above it a row takes the short list
FIRST_IDX = 7000


def arranged(B, sel):
    """(req[sel], pat[sel], txt[sel]) with idx = 7000 + position: a row that lands in another pair's place shows even where the
    two pairs are duplicates."""
    req, pat, txt = B
    sel = np.asarray(sel, dtype=np.int64)
    r = req[sel].copy()
    r["idx"] = FIRST_IDX + np.arange(len(sel), dtype=np.uint32)
    return r, np.ascontiguousarray(pat[sel]), np.ascontiguousarray(txt[sel])


def expected(ores, oops, sel):
    """The oracle's rows of B, gathered the same way."""
    sel = np.asarray(sel, dtype=np.int64)
    return ores[sel], None if oops is None else oops[sel]


def unit_of(plan_line):
    """Pairs per wavefront of the kernel a plan line names."""
    kernel = plan_line.split()[0]
    for token in ("G", "lanes_per_pair"):
        m = re.search(r" %s=(\d+)" % token, plan_line)
        if m:
            return 64 // int(m.group(1))
    if kernel in ("wfa_wave_kernel", "wfa_bidir_kernel", "dp_wave_kernel", "dp_strip_kernel", "genasm_wave_kernel"):
        return 1
    assert kernel in ("wfa_lane_kernel", "wfa_lane_packed_kernel", "nw_lane_kernel", "swg_lane_kernel", "nw_reg_kernel",
                      "swg_reg_kernel"), plan_line
    return 64


def rotation(n0, k):
    """B rotated by k: pair p stands at position (p + k) mod n0."""
    return (np.arange(n0) - k) % n0


def rotations(n0):
    seen, out = set(), []
    for k in ROTATIONS:
        if k % n0 and k % n0 not in seen:
            seen.add(k % n0)
            out.append(("rot%d" % (k % n0), rotation(n0, k % n0)))
    return out


def reversed_sel(n0):
    """B backwards, the two empty-sequence pairs moved behind everything else: the body first, the hard pairs last, and the batch
    ends on rs/0 and 0/rs."""
    back = [p for p in range(n0 - 1, -1, -1) if p not in (EMPTY_TEXT, EMPTY_PATTERN)]
    return np.array(back + [EMPTY_TEXT, EMPTY_PATTERN])


def singletons():
    return [("single_" + name, np.array([p])) for name, p in SINGLETONS]


def _run_order(singles):
    """rs/rs last: behind `full` it would stand where the launch before had the same pair with the same idx, and a row the kernel
    never wrote would still hold the right bytes."""
    return singles[1:] + singles[:1]


def prefix_sizes(n0, u):
    return sorted({n for n in (2, u - 1, u, u + 1, 2 * u + 1, 63, 64, 65, n0 - 1) if 2 <= n < n0})


def prefixes(n0, u, sizes=None):
    """The first n pairs of the reversed batch. The small ones end on body pairs; n0 - 1 ends on the hard pairs, rs/0 last."""
    rev = reversed_sel(n0)
    return [("prefix%d" % n, rev[:n]) for n in (prefix_sizes(n0, u) if sizes is None else sizes)]


def hostile(n0, host):
    """[h, b0, h, b1, ...]: the host at every even position, the body (from N_SPECIAL on) at the odd ones."""
    sel = np.empty(n0, dtype=np.int64)
    sel[0::2] = host
    k = len(sel[1::2])
    sel[1::2] = F.N_SPECIAL + np.arange(k) % (n0 - F.N_SPECIAL)
    return sel


def hostiles(n0):
    return [("hostile_" + name, hostile(n0, h)) for name, h in HOSTS]


def duplicates(n0):
    return [("all_" + name, np.full(n0, p)) for name, p in DUPLICATES]


def tiled(n0):
    """B eight times over, copy c rotated by 11 * c: for one-CU runs, where a workgroup then has many units."""
    return ("tiled", np.concatenate([rotation(n0, (11 * c) % n0) for c in range(TILED_COPIES)]))


# Rows whose launch takes some 0.2 to 0.4 s on an MI355X whatever the pair count (int8 SWG with CIGAR, one pair per lane or one
# workgroup per pair at READ_SIZE 1192 to 1544: the full list took 3.6, 6.0 and 10.1 s there). They run the short form of the list.
SLOW_ROWS = (("swg8_bt", 1192), ("swg8_bt", 1200), ("swg8_bt", 1544))


def arrangements(rs, n0, u, short=False):
    """The arrangements of one table row (without `tiled`), deterministic from (rs, n0, u), in the order they are run: large and
    small batches alternate -- full, singleton, rotation, prefix, and so on. short: without the singletons, with one rotation and
    one hostile arrangement."""
    if rs > LONG_RS:
        large = [("reversed", reversed_sel(n0)), rotations(n0)[0]]
        small = _run_order(singletons()) + prefixes(n0, u, sizes=sorted({2, n0 - 1}))
    elif short:
        large = [("reversed", reversed_sel(n0)), rotations(n0)[0], hostiles(n0)[1]] + duplicates(n0)
        small = prefixes(n0, u)
    else:
        large = [("reversed", reversed_sel(n0))] + rotations(n0) + hostiles(n0) + duplicates(n0)
        small = _run_order(singletons()) + prefixes(n0, u)
    out = [("full", np.arange(n0))]
    for i in range(max(len(large), len(small))):
        out += small[i:i + 1] + large[i:i + 1]
    return out


def is_permutation(sel, n0):
    return len(sel) == n0 and np.array_equal(np.sort(sel), np.arange(n0))


# ------------------------------------------------------------------ plans of the prefix sizes
def plan_table():
    """{"family/READ_SIZE": {n: kernel-and-shape words of aim_plan_describe}} at n0 and at every prefix size of the row, under each
    row's own knobs (the caller sets the planning environment: 16 GB, 256 CUs)."""
    out = {}
    for fam, rs in F.ROWS:
        env = F.FAMILIES[fam]["env"]
        F._with_env(env)
        try:
            params, n0 = F.row_params(fam, rs), F.pairs_for(rs)
            full = F.plan_line(params, n0)
            lines = {n0: full}
            for n in [1] + (prefix_sizes(n0, unit_of(full)) if rs <= LONG_RS else sorted({2, n0 - 1})):
                lines[n] = F.plan_line(params, n)
            out["%s/%d" % (fam, rs)] = {str(n): shape_words(line) for n, line in sorted(lines.items())}
        finally:
            F._without_env(env)
    return out


SHAPE_TOKENS = ("lanes_per_pair=", "wavefronts_per_pair=", "cells_per_lane=", "G=", "seq_lds=", "pack_first=")


def shape_words(line):
    """The kernel name and the shape tokens of a plan line (grid and scratch sizes follow the pair count and stay out)."""
    words = line.split()
    return " ".join(words[:1] + [w for w in words[1:] if w.startswith(SHAPE_TOKENS)])


if __name__ == "__main__":
    import json
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1] == "--plans":
        json.dump(plan_table(), sys.stdout)
