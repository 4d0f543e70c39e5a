"""The oracle against the live reference: the unmodified reference programs, compiled for the CPU under oracle/upmem_shim by
__graft_entry__.build() (oracle/ref_build.py), run on the recorded rows, on the suite's own batches and on fresh inputs. No GPU, and
nothing is compiled here: a missing binary is a failure that names build().

Every reference and oracle run of this module is made once, on a pool of threads, by the `live` fixture; the tests assert its
results. Measured wall times are in DESIGN.md "Oracle"."""
import gzip
import json
import os

import numpy as np
import pytest

import reference_live as L
import reference_rows as R
from conftest import GOLDEN, judge_case_input, judge_dataset_cases, md5

TABLE_CASES = L.table_cases()
FRESH_CASES = [(e, bt) for e in L.FRESH for bt in (False, True)]
RECORDED = ([("row", c["name"], c) for c in R.all_reference_rows()] + [("dataset", c["name"], c) for c in judge_dataset_cases()]
            + [("sample", k, k) for k in L.SAMPLE_ROWS])


def _recorded_job(kind, case):
    from oracle import ref_run
    if kind == "sample":
        with gzip.open(os.path.join(GOLDEN, "sample-l100-e1-40K.gz"), "rb") as f:
            data = f.read()
        return ref_run.run(L.sample_config(case)[0], data, L.SAMPLE_N)
    if kind == "dataset":
        return ref_run.run(L.case_config(case)[0], L.dataset_bytes(case), case["n"])
    return ref_run.run(L.case_config(case)[0], judge_case_input(case), case["gen"]["n"])


def _table_job(source, key):
    from aim_amd import capi
    _, params, name, op, (req, pat, txt, lost), refit = L.case_batch(source, key)
    r = L.compare_batch(name, op, bool(params.flags & capi.FLAG_BACKTRACE), req, pat, txt)
    r["lost"], r["fitted"] = lost, refit
    return r


def _fresh_job(entry, bt):
    from aim_amd import engine
    from oracle import ref_run
    params = L.fresh_params(entry, bt)
    name, _, op = L.params_config(params, entry[1])
    out = []
    for label, data, n in L.fresh_inputs(entry, params.read_size):
        req, pat, txt = engine.parse_pairs(data, params.read_size)
        out.append((label, L.compare_batch(name, op, bt, req, pat, txt)))
    return out


@pytest.fixture(scope="module")
def live(built):
    from oracle import ref_build
    missing = [n for n in ref_build.table() if not os.path.exists(ref_build.host_path(n))]
    assert not missing, ("%d of %d reference binaries are missing under oracle/_ref (first: %s): __graft_entry__.build() compiles them "
                         "from oracle/ref_configs.json where the reference tree is present" % (len(missing), len(ref_build.table()), missing[0]))
    jobs = {("recorded", name): (lambda k=kind, c=case: _recorded_job(k, c)) for kind, name, case in RECORDED}
    jobs.update({("table", cid): (lambda s=source, k=key: _table_job(s, k)) for cid, source, key in TABLE_CASES})
    jobs.update({("fresh", L.fresh_id(e, bt)): (lambda e=e, bt=bt: _fresh_job(e, bt)) for e, bt in FRESH_CASES})
    return L.run_pool(jobs)


def _result(live, key):
    r = live[key]
    if isinstance(r, Exception):
        raise r
    return r


# ------------------------------------------------------------------ the table of configurations
def test_config_table_is_current():
    """oracle/ref_configs.json is what oracle/make_ref_configs.py writes from the tests' tables: every binary a test asks for is
    named there, so build() makes it."""
    import importlib.util
    from oracle import ref_build
    spec = importlib.util.spec_from_file_location("make_ref_configs", os.path.join(ref_build.HERE, "make_ref_configs.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert open(ref_build.TABLE).read() == mod.render(), "run oracle/make_ref_configs.py"


def test_config_table_entries():
    from oracle import ref_build
    for name, e in ref_build.table().items():
        assert e["nr_tasklets"] == 1 and e["variant"] in sum(ref_build.VARIANTS.values(), ()), name
        assert all(f.startswith("-D") for f in e["flags"]), name
        assert [f.split("=")[0] for f in e["flags"][:5]] == ["-DMAX_SCORE", "-DREAD_SIZE", "-DWRAM_SEGMENT", "-DMATCH", "-DMISMATCH"], name
        segment = int(e["flags"][2].split("=")[1])
        assert e["variant"] == "WFA/DPU-WRAM" or segment < 62000, name          # */dpu/dpu_allocator_wram.c's init check


# ------------------------------------------------------------------ the domain predicate against the code's own indexing
def _last_cell(plen, tlen):
    """The largest flat index nw.c:112-145 / swg.c:124-162 touch: rows 0..tlen of stride tlen + 1, columns 0..plen."""
    cols = tlen + 1
    idx = [v for v in range(plen + 1)] + [cols * h for h in range(tlen + 1)]
    idx += [cols * h + v for h in range(1, tlen + 1) for v in range(1, plen + 1)]
    return max(idx)


@pytest.mark.parametrize("rs", [8, 16])
@pytest.mark.parametrize("algo,variant", [("nw", "NW/DPU-WRAM"), ("swg", "SWG/DPU-WRAM"), ("nw", "NW/DPU-MRAM"), ("swg", "SWG/DPU-MRAM")])
def test_domain_is_the_table_bound(algo, variant, rs):
    for pl in range(rs + 2):
        for tl in range(rs + 2):
            want = pl <= rs and tl <= rs and _last_cell(pl, tl) < rs * rs
            assert bool(L.in_reference_domain(algo, variant, True, rs, pl, tl)) == want, (pl, tl)


def test_domain_edges():
    rs = 112
    nw = lambda pl, tl: bool(L.in_reference_domain("nw", "NW/DPU-WRAM", True, rs, pl, tl))
    assert not nw(rs, rs) and not nw(1, rs) and not nw(0, rs)          # a full text never fits
    assert not nw(rs, rs - 1) and nw(rs - 1, rs - 1) and nw(rs, rs - 2) and nw(rs, 0)
    wfa = lambda pl, tl, **kw: bool(L.in_reference_domain("wfa", kw.pop("variant", "WFA/DPU-MRAM"), True, rs, pl, tl, **kw))
    assert wfa(rs, rs) and wfa(0, rs) and wfa(rs, 0) and not wfa(rs + 1, 1) and not wfa(1, rs + 1)
    assert wfa(rs, rs, variant="WFA/DPU-WRAM") and not wfa(rs, rs, variant="WFA/DPU-WRAM", overflows=True)
    assert bool(L.in_reference_domain("wfa", "WFA/DPU-WRAM", False, rs, rs, rs, overflows=True))          # score only: no backtrace to run
    got = L.in_reference_domain("swg", "SWG/DPU-WRAM", False, rs, np.array([rs, 5, rs]), np.array([rs, 5, rs - 2]))
    assert got.tolist() == [False, True, True]
    with pytest.raises(AssertionError):
        L.in_reference_domain("nw", "NW/DPU-WRAM", False, 110, 1, 1)


def test_domain_batch_ends_in_the_sentinel():
    import full_rows as F
    req, pat, txt = F.row_batch(104, "zero")
    oreq, opat, otxt, lost = L.domain_batch("nw", "NW/DPU-WRAM", True, req, pat, txt)
    assert len(oreq) == len(req) - lost + 1 and lost == 13
    assert opat[-1, :oreq["pattern_len"][-1]].tobytes() == L.SENTINEL[0] and otxt[-1, :oreq["text_len"][-1]].tobytes() == L.SENTINEL[1]
    assert oreq["idx"].tolist() == list(range(len(oreq)))
    assert L.in_reference_domain("nw", "NW/DPU-WRAM", True, 104, oreq["pattern_len"], oreq["text_len"]).all()
    wreq, _, _, wlost = L.domain_batch("wfa", "WFA/DPU-MRAM", True, req, pat, txt)
    assert wlost == 0 and len(wreq) == len(req) + 1          # WFA takes every full row


# ------------------------------------------------------------------ a. the stand-in SDK reproduces every recorded row
def test_recorded_rows_are_all_there():
    """Every recorded reference result of tests/golden: judge_r01..r06 (120 digests, 4 aborts), r03's 4 dataset rows at NR_DPUS 4
    and the 6 digests of reference_digests.json."""
    assert len(RECORDED) == 134 and len({n for _, n, _ in RECORDED}) == 134
    assert sum("abort" in c for k, _, c in RECORDED if k == "row") == 4
    assert all(c["nr_dpus"] == 4 for k, _, c in RECORDED if k == "dataset")


@pytest.mark.parametrize("kind,name,case", RECORDED, ids=[n for _, n, _ in RECORDED])
def test_recorded_row(live, kind, name, case):
    rc, out, log = _result(live, ("recorded", name))
    if kind == "row" and "abort" in case:
        assert rc != 0 and case["abort"].encode() in log, (rc, log[-300:])
        return
    want = json.load(open(os.path.join(GOLDEN, "reference_digests.json")))[case] if kind == "sample" else case["output_md5"]
    assert rc == 0, (rc, log[-300:])
    assert md5(out) == want


# ------------------------------------------------------------------ b. the oracle on the suite's own batches
@pytest.mark.parametrize("cid,source,key", TABLE_CASES, ids=[c[0] for c in TABLE_CASES])
def test_oracle_equals_reference_on_table_batch(live, cid, source, key):
    r = _result(live, ("table", cid))
    pairs, lost, fitted = L.excluded_counts()[cid]
    assert (r["n"] - 1 + r["lost"], r["lost"], int(r["fitted"])) == (pairs, lost, fitted), "tests/golden/reference_live_excluded.json"
    L.check_compared(r, cid)


def test_excluded_table():
    """One entry per table case, none above the cap of a quarter of the row's pairs; a fitted batch loses nothing."""
    table = L.excluded_counts()
    assert sorted(table) == sorted(c[0] for c in TABLE_CASES)
    for cid, (pairs, lost, fitted) in table.items():
        assert lost <= L.MAX_LOST * pairs, cid
        assert not (fitted and lost), cid
    assert any(lost for _, lost, _ in table.values()) and any(f for _, _, f in table.values())


def test_table_cases_cover_the_tables():
    import low_complexity as LC
    import penalty_rows as P
    ids = {c[0] for c in TABLE_CASES}
    for fam in ("nw", "nw_bt", "swg16_bt", "swg8_bt", "wfa5_bt", "wfa2", "wfa2_red_bt", "wfa_wave", "wfa10_bt"):
        for rs, _ in LC.TABLE[fam]:
            assert "low-%s-%d" % (fam, rs) in ids
    assert not any(c[2][0].startswith(("genasm",)) for c in TABLE_CASES if c[1] in ("low", "full"))
    pens = {r["pen"] for r in P.ROWS.values() if "w32" not in r["kw"]}
    assert {P.ROWS[c[2][0]]["pen"] for c in TABLE_CASES if c[1] == "penalty"} == pens
    for name, _ in L._penalty_sets():
        flags = {(c[2][2], c[2][3]) for c in TABLE_CASES if c[1] == "penalty" and c[2][0] == name}
        assert flags == set(P.ALL4), name


# ------------------------------------------------------------------ c. fresh inputs
def test_fresh_entries_are_fresh():
    used = L.recorded_costs()
    kinds = {}
    for kind, algo, l, e, n, seed, costs in L.FRESH:
        kinds[kind] = kinds.get(kind, 0) + 1
        g = costs.get("gap", 4)
        c = (costs["mismatch"], g, g) if algo == "nw" else (costs["mismatch"], costs["gap_o"], costs["gap_e"])
        assert c not in used[algo], (kind, c)
    assert kinds == {"nw": 4, "swg8": 4, "swg16": 4, "wfa": 4, "wfa_red": 4}


@pytest.mark.parametrize("entry,bt", FRESH_CASES, ids=[L.fresh_id(e, bt) for e, bt in FRESH_CASES])
def test_oracle_equals_reference_on_fresh_input(live, entry, bt):
    for label, r in _result(live, ("fresh", L.fresh_id(entry, bt))):
        L.check_compared(r, "%s on %s" % (L.fresh_id(entry, bt), label))
