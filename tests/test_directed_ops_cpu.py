"""The directed ops rows of directed_ops.py, judged on the CPU: every scenario's claim holds on sam_model; the tile restatement of the
two record kernels (sam_tile_model.py) equals sam_model on every directed row and on 2 000 seeded random rows; every mutant of the
restatement is told from the model by named directed rows; the model's records rebuild the reference from a consistent read; and the
rows cover what they promise. No kernel can be mutated on the GPU, so this is the evidence that the rows would catch a subtly wrong
one."""
import collections
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import directed_ops as do  # noqa: E402
import sam_model  # noqa: E402
import sam_tile_model as tm  # noqa: E402

SHORT_GROUPS = tuple(g for g in do.GROUPS if g != "DL")
LONG_RS, LONG_REF = 65528, 300000


@pytest.fixture(scope="module")
def short():
    ref = do.reference()
    batch = do.lay(do.rows_of(SHORT_GROUPS), 1024, ref)
    return ref, batch, {eqx: do.expected(batch, ref, eqx) for eqx in (False, True)}


@pytest.fixture(scope="module")
def long():
    ref = do.reference(LONG_REF)
    batch = do.lay(do.long_rows(), LONG_RS, ref)
    return ref, batch, {eqx: do.expected(batch, ref, eqx) for eqx in (False, True)}


def label(r):
    return "%s/%s strand %d shift %d %s filler %02x %s" % (r.scn.group, r.scn.name, r.strand, r.shift, r.end, r.filler, r.kind)


def restated(mapping, batch, ref, i, eqx, mutate=None):
    return tm.fields(mapping, batch["res"][i], batch["ops"][i], batch["tpos"][i], ref, True, do.MAX_SCORE, eqx=eqx, mutate=mutate,
                     filler=batch["rows"][i].filler)


def test_every_claim_holds_on_the_model(short, long):
    n = 0
    for ref, batch, exps in (short, long):
        for i, (r, e) in enumerate(zip(batch["rows"], exps[False])):
            if r.kind == "ok":
                assert do.claim_holds(r.scn, e), (label(r), sam_model.cigar_string(e[3])[:80], e[4][:80])
                n += 1
            else:
                assert e[5] == sam_model.SAM_UNMAPPED and e[0] == int(batch["tpos"][i]) & (do.MINUS - 1), label(r)
    assert n >= 1500
    # the same ops with AIM_SAM_EQX: '=' and 'X' runs whose lengths sum to the M runs', the MD and every other field unchanged
    for ref, batch, exps in (short, long):
        for r, e0, e1 in zip(batch["rows"], exps[False], exps[True]):
            assert e0[:3] == e1[:3] and e0[4:] == e1[4:], label(r)
            merged = []
            for w in e1[3]:
                op = 0 if w & 15 in (7, 8) else w & 15
                if merged and merged[-1][0] == op:
                    merged[-1][1] += w >> 4
                else:
                    merged.append([op, w >> 4])
            assert [(n_ << 4) | op for op, n_ in merged] == e0[3], label(r)
            assert sum(w >> 4 for w in e1[3] if w & 15 == 8) == r.scn.walk.count(b"X") * (e1[5] != sam_model.SAM_UNMAPPED), label(r)


@pytest.mark.parametrize("mapping", ["lane", "wave"])
def test_restatement_equals_the_model_on_every_directed_row(short, long, mapping):
    for ref, batch, exps in (short, long):
        for eqx in (False, True):
            for i, r in enumerate(batch["rows"]):
                assert restated(mapping, batch, ref, i, eqx) == exps[eqx][i], (mapping, eqx, label(r))


def random_rows(seed, n, rs=1024):
    """Edge-heavy random rows: run lengths drawn around 1, 4, 10, 100 and 256, runs of M X I D and now and then another byte, on both
    strands, at every shift, at either end of the row, with every filler."""
    rng = np.random.default_rng([seed, 0x6F7073])
    rows = []
    for i in range(n):
        budget = int(rng.integers(1, 2 * rs - 16))
        walk = bytearray()
        while len(walk) < budget:
            centre = (1, 4, 10, 100, 256)[int(rng.integers(0, 5))]
            ln = max(1, centre + int(rng.integers(-2, 3)))
            op = b"MMMXID"[int(rng.integers(0, 6))] if rng.random() < 0.97 else int(rng.integers(0, 256))
            walk += bytes([op]) * min(ln, 3 if op != ord("M") and centre > 10 and rng.random() < 0.5 else ln)
        walk = bytes(walk[:budget])
        s = do.Scenario("random", "r%d" % i, walk, None, None, True, None)
        rows.append(do.Row(s, i & 1, (i >> 1) & 3, "lo" if (i >> 3) & 1 else "hi", do.FILLERS[i % len(do.FILLERS)], "ok"))
    return rows


def test_restatement_equals_the_model_on_random_rows():
    ref = do.reference()
    rows = random_rows(1, 2000)
    batch = do.lay(rows, 1024, ref)
    seen = collections.Counter()
    for i, r in enumerate(rows):
        eqx = bool((i // 5) & 1)
        want = sam_model.row_fields(batch["res"][i], batch["ops"][i], batch["tpos"][i], ref, True, do.MAX_SCORE, eqx)
        for mapping in ("lane", "wave"):
            assert restated(mapping, batch, ref, i, eqx) == want, (mapping, eqx, i, r.scn.walk)
        seen[("strand", r.strand)] += 1
        seen[("shift", r.shift)] += 1
        seen[("filler", r.filler)] += 1
        seen[("eqx", eqx)] += 1
        seen["mapped"] += want[5] != sam_model.SAM_UNMAPPED
        seen["tiles>1"] += len(r.scn.walk) > tm.TILE
    assert all(seen[("strand", s)] >= 900 for s in (0, 1)) and all(seen[("shift", s)] >= 400 for s in range(4)), seen
    assert all(seen[("filler", f)] >= 300 for f in do.FILLERS) and seen[("eqx", True)] >= 900 and seen["mapped"] >= 1800 and seen["tiles>1"] >= 1000, seen


def mutant_mappings(mutant):
    return ("wave",) if mutant in tm.WAVE_MUTANTS else ("lane",) if mutant in tm.LANE_MUTANTS else ("lane", "wave")


@pytest.mark.parametrize("mutant", [m for m in tm.MUTANTS if m not in tm.OUTPUT_EQUIVALENT])
def test_every_mutant_is_killed_by_directed_rows(short, mutant, capsys):
    """Each mutant over the short directed rows (the long-digit rows stay out: the restatement walks them once per mapping, above) until
    four rows of two different scenarios have told it from the model; the rows are named."""
    ref, batch, exps = short
    for mapping in mutant_mappings(mutant):
        killers = []
        for eqx in (False, True):
            for i, r in enumerate(batch["rows"]):
                if restated(mapping, batch, ref, i, eqx, mutant) != exps[eqx][i]:
                    killers.append((label(r), "eqx" if eqx else "plain"))
                    if len(killers) >= 4 and len({k[0].split(" ")[0] for k in killers}) >= 2:
                        break
            if len(killers) >= 4:
                break
        with capsys.disabled():
            shown = killers if len(killers) <= 3 else killers[:2] + killers[-1:]       # (the last one is of another scenario)
            print("\n  %s on %s: killed by %s" % (mutant, mapping, "; ".join("%s (%s)" % k for k in shown)))
        assert killers, "no directed row tells %s on the %s mapping from the model: a scenario is missing" % (mutant, mapping)


@pytest.mark.parametrize("mutant", tm.OUTPUT_EQUIVALENT)
def test_two_guards_cannot_show_in_the_output(short, mutant):
    """sam_walk4's `valid` mask and its `w0 >= 0` guard. Every consumer of the four ops tests k + j < n (or kk <= last < n) itself, the
    byte that prev_q hands on lies below `last`, and a word below the row holds only bytes past n: no row can make these two mutants
    print another record, and no scenario can be added that does. What the guard prevents is a load in front of the row, which a record
    cannot show. Asserted over every directed row with every filler -- strand-1 rows at begin_offset 0 .. 3 among them -- so that a
    later change that makes either guard matter to the output fails here and gets its scenario then."""
    ref, batch, exps = short
    below = 0
    for i, r in enumerate(batch["rows"]):
        eqx = bool(i & 1)
        assert restated("wave", batch, ref, i, eqx, mutant) == exps[eqx][i], (mutant, label(r))
        below += r.strand == 1 and r.kind == "ok" and int(batch["res"]["begin_offset"][i]) < 4 and len(r.scn.walk) % 4 != 0
    assert below >= 100, "strand-1 rows whose last quad starts below row byte 0"


def test_the_model_rebuilds_the_reference(short, long):
    """The round trip: a read consistent with the ops and the reference, then reference[pos : pos + ref_span] back from that read, the
    CIGAR words and the MD; the read-consuming CIGAR lengths sum to the read's length."""
    done = 0
    for ref, batch, exps in (short, long):
        for eqx in (False, True):
            for i, r in enumerate(batch["rows"]):
                pos, span, nm, words, md, flags = exps[eqx][i]
                if flags == sam_model.SAM_UNMAPPED:
                    continue
                ws = int(batch["tpos"][i]) & (do.MINUS - 1)
                read = do.build_read(r.scn.walk, ref[ws:ws + do.ref_consumed(r.scn.walk)].tobytes())
                back, used = sam_model.rebuild_reference(read, words, md, strict=True)
                assert back == ref[pos:pos + span].tobytes() and used == len(read), label(r)
                assert sum(w >> 4 for w in words if w & 15 in (0, 1, 4, 7, 8)) == len(read), label(r)
                assert nm == sum(w >> 4 for w in words if w & 15 in (1, 2)) + r.scn.walk.count(b"X"), label(r)
                done += 1
    assert done >= 3000


def test_coverage(short, long):
    seen = collections.Counter()
    digits = set()
    for ref, batch, exps in (short, long):
        for i, r in enumerate(batch["rows"]):
            g = "D" if r.scn.group == "DL" else r.scn.group
            seen[(g, "strand", r.strand)] += 1
            seen[(g, "shift", int(batch["res"]["begin_offset"][i]) % 4 if r.kind != "inverted" else r.shift)] += 1
            seen[(g, "filler", r.filler)] += 1
            if r.strand == 1 and r.kind == "ok":
                seen[("strand1-begin", int(batch["res"]["begin_offset"][i]))] += 1
            digits |= {len(t) for t in re.findall(rb"\d+", exps[False][i][4])}
            walk = r.scn.walk
            core = [k for k in range(len(walk)) if walk[k:k + 1] in (b"M", b"X")]
            for eqx in (False, True):
                cls = [tm.bam_op(tm.sam_class(c), eqx) for c in walk]
                if any(cls[k] != cls[k - 1] for k in range(tm.TILE, len(walk), tm.TILE) if core and core[0] < k <= core[-1]):
                    seen[("boundary-at-tile", eqx)] += 1
            seen[("kind", r.kind)] += 1
    for g in SHORT_GROUPS:
        assert all(seen[(g, "strand", s)] for s in (0, 1)) and all(seen[(g, "shift", s)] for s in range(4)), (g, seen)
        assert all(seen[(g, "filler", f)] for f in do.FILLERS), (g, seen)
        assert sum(1 for s in do.SCENARIOS if s.group == g and s.fill) >= 4, g
    assert all(s.fill for s in do.SCENARIOS if s.group != "DL" and (s.walk[-1:] == b"M" or s.walk[:1] == b"M"))
    assert all(seen[("strand1-begin", b)] >= 10 for b in range(4)), seen
    assert digits >= {1, 2, 3, 4, 5, 6}, digits
    assert seen[("boundary-at-tile", False)] >= 8 and seen[("boundary-at-tile", True)] >= 8, seen
    assert all(seen[("kind", k)] >= 4 for k in ("empty", "inverted", "status", "overcap")), seen
