"""The live reference (oracle/ref_build.py, oracle/ref_run.py) as the tests use it: which binary a recorded row, a table row or a
fresh entry runs on, which pairs the reference can take at all, and the batches both live-reference test modules compare on.
No device. oracle/make_ref_configs.py writes oracle/ref_configs.json from all_configs()."""
import gzip
import json
import os

import numpy as np

from conftest import GOLDEN, judge_costs, judge_dataset_cases

SAMPLE_N = 20000          # reference_digests.json: Datasets/sample-l100-e1-40K, n = 20000, NR_DPUS 1
SAMPLE_ROWS = {           # digest key -> (algo, variant, MAX_SCORE, make-config keywords)
    "wfa_backtrace": ("wfa", "WFA/DPU-WRAM", 5, dict(backtrace=True)),
    "wfa_reduce_backtrace": ("wfa", "WFA/DPU-WRAM", 5, dict(backtrace=True, reduce=True)),
    "swg_w8_backtrace": ("swg", "SWG/DPU-WRAM", 5, dict(backtrace=True)),
    "swg_w16_backtrace": ("swg", "SWG/DPU-MRAM", 5, dict(backtrace=True)),
    "nw_backtrace": ("nw", "NW/DPU-WRAM", 4, dict(backtrace=True)),
    "wfa_score_only": ("wfa", "WFA/DPU-WRAM", 5, dict()),
}
SAMPLE_READ_SIZE = 112


def _ref_build():
    from oracle import ref_build
    return ref_build


# ------------------------------------------------------------------ recorded rows -> binaries
def case_config(case):
    """(name, table entry) of the binary a recorded row (judge_r0?_cases.json: `cases` and `dataset_cases`) was made with. A
    row's `variant` may carry a remark behind the tree's name; an NW row gives `gap` or `gap_i` / `gap_d`; an SWG row without
    `variant` ran on the tree whose cell width is its `swg_cell_bytes` (ref_build.swg_variant)."""
    rb = _ref_build()
    algo, ms = case["algo"], case["max_score"]
    costs = judge_costs(case)
    if "gap" in costs:
        costs["gap_i"] = costs["gap_d"] = costs.pop("gap")
    if "variant" in case:
        variant = case["variant"].split(" ")[0]
    elif algo == "swg":
        variant = rb.swg_variant(ms, case.get("swg_cell_bytes", 0))
    else:
        variant = rb.VARIANTS[algo][0]
    return rb.config(algo, variant, ms, case["read_size"], backtrace=case["backtrace"], reduce=bool(case.get("reduce", False)),
                     nr_dpus=case.get("nr_dpus", 1), **costs)


def sample_config(key):
    algo, variant, ms, kw = SAMPLE_ROWS[key]
    return _ref_build().config(algo, variant, ms, SAMPLE_READ_SIZE, **kw)


def dataset_bytes(case):
    with gzip.open(os.path.join(GOLDEN, case["dataset"] + ".gz"), "rb") as f:
        return f.read()


def recorded_configs():
    import reference_rows as R
    out = dict(case_config(c) for c in R.all_reference_rows() + judge_dataset_cases())
    out.update(sample_config(k) for k in SAMPLE_ROWS)
    return out


# ------------------------------------------------------------------ the reference's domain
def in_reference_domain(algo, variant, backtrace, read_size, plen, tlen, overflows=False):
    """Whether the reference program `variant` takes a pair of these lengths without undefined behaviour; plen / tlen may be
    arrays. Read off the reference's own lines (the WRAM trees; the MRAM trees' lines where they differ):

    * host.c:119-123 -- a sequence longer than READ_SIZE ends the host. A sequence of exactly READ_SIZE bases is legal in every
      row but a DPU's last: strcpy (host.c:126-127) puts its NUL into the first byte of the next row of the same buffer, which
      the next strcpy overwrites; behind the last row it would land past the malloc of host.c:204-205. The batches therefore end
      in SENTINEL, so no full row is ever last, and this predicate has nothing to add for it.
    * The DPU reads ROUND_UP_MULTIPLE_8(len) bytes of a row (wfa.c:421-423, nw.c:203-205, swg.c:218-220) into a buffer of
      ROUND_UP_MULTIPLE_8(len) (wfa.c:417-418) or ROUND_UP_MULTIPLE_8(READ_SIZE) bytes (nw.c:183-184, swg.c:207-208); the source
      runs on into the next row or region of MRAM, never past it. With READ_SIZE a multiple of 8 (the launchers' rule,
      run-*-pim-*.py `read_length = ceil(.../8)*8`; host.c:232 asserts it of the whole buffer) no length adds a condition.
    * The ops row holds 2 * READ_SIZE bytes (wfa.c:463, nw.c:190, swg.c:205) and a traceback writes plen + tlen of them at most
      (max_operations, wfa.c:63); the host copies ROUND_UP_MULTIPLE_8(max_operations) <= 2 * READ_SIZE (host.c:347-348).
    * NW and SWG keep one flat table of READ_SIZE * READ_SIZE cells (nw.c:187; NW/DPU-MRAM nw.c:265; SWG/DPU-MRAM swg.c:246-253)
      or ROUND_UP_MULTIPLE_8(READ_SIZE) * READ_SIZE (swg.c:196) and address cell (h, v) as (tlen + 1) * h + v for h <= tlen,
      v <= plen (nw.c:112-145, swg.c:124-162): the last cell written is (tlen + 1) * tlen + plen, which must lie inside the
      table. So tlen == READ_SIZE is always outside, and tlen == READ_SIZE - 1 is inside only below plen == READ_SIZE. (A pattern
      longer than the text makes rows alias inside the table, which is defined and which the oracle restates.) What lies behind
      the table is the ops row (nw.c:190) or the request, result and cigar structs (swg.c:198-205).
    * WFA has no table. WFA/DPU-WRAM with BACKTRACE indexes wavefronts[MAX_SCORE + 1] of a MAX_SCORE + 1 entry array once a
      pair's score passes MAX_SCORE (wfa.c:345, 369-373), so there a pair is inside only if it does not overflow (`overflows`,
      which is not a function of the lengths; the tests run WFA with BACKTRACE on WFA/DPU-MRAM, which returns before the
      backtrace, WFA/DPU-MRAM wfa.c:400-404).
    * The WRAM arena check (dpu_allocator_wram.c:17-23) ends the program with `out of memory`: defined, and a property of
      WRAM_SEGMENT, not of a pair. oracle/ref_build.py sizes WRAM_SEGMENT so that it cannot trigger (wfa_wram_segment)."""
    plen, tlen = np.asarray(plen, dtype=np.int64), np.asarray(tlen, dtype=np.int64)
    assert read_size % 8 == 0, "the launchers round READ_SIZE up to a multiple of 8"
    ok = (plen >= 0) & (tlen >= 0) & (plen <= read_size) & (tlen <= read_size)
    if algo in ("nw", "swg"):
        cells = read_size * read_size          # (swg.c:196's ROUND_UP_MULTIPLE_8(READ_SIZE) equals READ_SIZE here)
        ok &= (tlen + 1) * tlen + plen < cells
    elif algo == "wfa":
        if variant == "WFA/DPU-WRAM" and backtrace:
            ok &= ~np.asarray(overflows, dtype=bool)
    else:
        raise ValueError("the reference has no " + algo)
    return ok


SENTINEL = (b"ACGTACGT", b"ACGAACGT")          # the short last pair of every batch: the host's last row is never full


def live_variant(algo, max_score, backtrace, swg_cell_bytes):
    """The tree a table row or fresh entry runs on: the WRAM tree, but WFA with BACKTRACE on WFA/DPU-MRAM (in_reference_domain)
    and int16 SWG below MAX_SCORE 127 on SWG/DPU-MRAM (the only int16 build there)."""
    rb = _ref_build()
    if algo == "wfa":
        return rb.VARIANTS["wfa"][1 if backtrace else 0]
    if algo == "swg":
        return rb.swg_variant(max_score, swg_cell_bytes)
    return rb.VARIANTS[algo][0]


def params_config(params, algo):
    """(name, table entry, oracle parameters) of an aim_params_t of a family the reference can express."""
    from aim_amd import capi
    import full_rows as F
    bt, red = bool(params.flags & capi.FLAG_BACKTRACE), bool(params.flags & capi.FLAG_REDUCE)
    cell = 2 if (params.flags & capi.FLAG_SWG_W16) else 0
    variant = live_variant(algo, params.max_score, bt, cell)
    name, entry = _ref_build().config(algo, variant, params.max_score, params.read_size, match=params.match, mismatch=params.mismatch,
                                      gap_o=params.gap_o, gap_e=params.gap_e, gap_i=params.gap_i, gap_d=params.gap_d, backtrace=bt,
                                      reduce=red)
    return name, entry, F.oracle_params(params, algo)


def domain_batch(algo, variant, backtrace, req, pat, txt):
    """(requests, patterns, texts, pairs left out): the pairs inside the reference's domain, numbered from 0, then SENTINEL."""
    from aim_amd import capi
    rs = pat.shape[1]
    keep = np.nonzero(in_reference_domain(algo, variant, backtrace, rs, req["pattern_len"], req["text_len"]))[0]
    n = len(keep) + 1
    oreq = np.zeros(n, dtype=capi.REQUEST_DTYPE)
    opat = np.zeros((n, rs), dtype=np.uint8)
    otxt = np.zeros((n, rs), dtype=np.uint8)
    oreq["pattern_len"][:-1], oreq["text_len"][:-1] = req["pattern_len"][keep], req["text_len"][keep]
    opat[:-1], otxt[:-1] = pat[keep], txt[keep]
    p, t = SENTINEL
    opat[-1, :len(p)], otxt[-1, :len(t)] = np.frombuffer(p, np.uint8), np.frombuffer(t, np.uint8)
    oreq["pattern_len"][-1], oreq["text_len"][-1] = len(p), len(t)
    oreq["idx"] = np.arange(n, dtype=np.uint32)
    return oreq, opat, otxt, len(req) - len(keep)


MAX_LOST = 0.25          # of a row's pairs


# ------------------------------------------------------------------ table rows the reference can express
def expressible(fam):
    """full_rows / low_complexity family names: NW, SWG and global WFA; an env-only family shares its base family's binary."""
    return fam.startswith(("nw", "swg16", "swg8", "wfa5", "wfa2", "wfa_wave", "wfa10", "wfa18"))


def _penalty_sets():
    """[(name of the first penalty_rows row with the set, (x, o, e))] of the global-WFA sets (W32 rows: a source edit in the
    reference, left out)."""
    import penalty_rows as P
    seen, out = set(), []
    for name, r in P.ROWS.items():
        if "w32" in r["kw"] or r["pen"] in seen:
            continue
        seen.add(r["pen"])
        out.append((name, r["pen"]))
    return out


def table_cases():
    """[(case id, source, key)]: every comparison of oracle and live reference on the tests' own batches. source "low" / "full":
    key (family, READ_SIZE) of low_complexity.ROWS / full_rows.ROWS; "bonus": of match_bonus.ROWS; "penalty": (row name, MAX_SCORE,
    BACKTRACE, REDUCE) for every penalty set of penalty_rows.ROWS at the row's caps under all four flag sets."""
    import full_rows as F
    import low_complexity as LC
    import match_bonus as MB
    import penalty_rows as P
    out = [("low-%s-%d" % k, "low", k) for k in LC.ROWS if expressible(k[0])]
    out += [("full-%s-%d" % k, "full", k) for k in F.ROWS if expressible(k[0])]
    out += [("bonus-%s-%d" % k, "bonus", k) for k in MB.ROWS]
    for name, _ in _penalty_sets():
        for ms in P.caps_of(name):
            for bt, red in P.ALL4:
                out.append(("penalty-" + P.case_id((name, ms, bt, red)), "penalty", (name, ms, bt, red)))
    return out


def table_case(source, key):
    """(algo, aim_params_t, (requests, patterns, texts)) of a table case, before the domain filter."""
    import full_rows as F
    import low_complexity as LC
    import match_bonus as MB
    import penalty_rows as P
    if source == "low":
        return LC.FAMILIES[key[0]]["algo"], LC.row_params(*key), LC.row_batch(*key)[:3]
    if source == "full":
        return F.FAMILIES[key[0]]["algo"], F.row_params(*key), F.row_batch(key[1], "zero")
    if source == "bonus":
        return "swg", MB.row_params(*key), F.row_batch(key[1], "zero")
    if source == "penalty":
        name, ms, bt, red = key
        from aim_amd import engine
        x, o, e = P.ROWS[name]["pen"]
        return "wfa", engine.make_params("wfa", ms, P.RS, mismatch=x, gap_o=o, gap_e=e, backtrace=bt, reduce=red), P.batch()
    raise ValueError(source)


def fitted(make, rs):
    """A batch of the generator `make(length)` in rows of READ_SIZE rs, at the length a launcher would have given that READ_SIZE
    (l + edits + 1 <= READ_SIZE: the l of full_rows' own body pairs)."""
    l = max(1, (rs - 8) * 100 // 104)
    req, pat, txt = make(l)[:3]
    wide = [np.zeros((len(req), rs), dtype=np.uint8) for _ in range(2)]
    wide[0][:, :l], wide[1][:, :l] = pat, txt
    return req.copy(), wide[0], wide[1]


def case_batch(source, key):
    """(algo, aim_params_t, table entry name, oracle parameters, (requests, patterns, texts, pairs left out), fitted) of a table
    case, ready for both sides. Where a full_rows batch would lose more than MAX_LOST of its pairs (the batches of 40 and 20 pairs
    above READ_SIZE 1024 lose their 13 full-length pairs), the generator is called at the launcher's length for that READ_SIZE
    instead, and every pair is inside."""
    from aim_amd import capi
    import full_rows as F
    algo, params, batch = table_case(source, key)
    name, entry, op = params_config(params, algo)
    bt = bool(params.flags & capi.FLAG_BACKTRACE)
    out = domain_batch(algo, entry["variant"], bt, *batch)
    refit = out[3] > MAX_LOST * len(batch[0]) and source in ("full", "bonus")
    if refit:
        rs = params.read_size
        out = domain_batch(algo, entry["variant"], bt, *fitted(lambda l: F.full_row_batch(l, F.pairs_for(rs), F.SEED), rs))
    return algo, params, name, op, out, refit


def compare_batch(name, op, backtrace, req, pat, txt):
    """Both sides on one batch: dict(rc, out, log) of the live reference, `want` the oracle's output file and `worst` its worst
    status. Where the oracle says the reference stops (worst != 0: int8 SWG's `No backtrace operation found`), also `rest`: the
    same comparison without the pairs the oracle stops on."""
    from aim_amd import engine
    from oracle import oracle, ref_run
    ores, oops, worst = oracle.align_batch(op, req["pattern_len"], req["text_len"], pat, txt, nthreads=1)
    rc, out, log = ref_run.run(name, engine.pairs_to_text(req, pat, txt), len(req))
    r = dict(rc=rc, out=out, log=log, worst=worst, want=oracle.format_output(ores, oops, backtrace), n=len(req))
    if worst != 0:
        keep = np.nonzero(ores["status"] == 0)[0]
        r["rest"] = compare_batch(name, op, backtrace, req[keep], np.ascontiguousarray(pat[keep]), np.ascontiguousarray(txt[keep]))
        r["stopped"] = len(req) - len(keep)
    return r


ABORT_SWG = b"SWG backtrace. No backtrace operation found"


def check_compared(r, label):
    """Assert one compare_batch result: byte-equal output files, or -- where the oracle says the reference stops -- the
    reference's own stop, and byte-equal files on the pairs the oracle finishes."""
    if r["worst"] == 0:
        assert r["rc"] == 0, "%s: the reference ended with %d: %r" % (label, r["rc"], r["log"][-300:])
        if r["out"] != r["want"]:
            a, b = r["out"].split(b"\n"), r["want"].split(b"\n")
            at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
            raise AssertionError("%s: output differs at line %d: reference %r, oracle %r" % (label, at, a[at:at + 2], b[at:at + 2]))
    else:
        assert r["rc"] == 1 and ABORT_SWG in r["log"], "%s: the oracle stops (status %d), the reference ended with %d: %r" % (
            label, r["worst"], r["rc"], r["log"][-300:])
        assert 0 < r["stopped"] < r["n"]
        check_compared(r["rest"], label + " without the %d pairs the oracle stops on" % r["stopped"])


def run_pool(jobs, workers=None):
    """{key: result or the exception} of {key: zero-argument function}, on up to 16 threads (the work is in child processes and
    in the oracle's C code)."""
    import concurrent.futures

    def call(f):
        try:
            return f()
        except Exception as e:          # noqa: BLE001 -- handed to the test that asked for this key
            return e
    workers = workers or max(1, min(16, os.cpu_count() or 1))
    keys = list(jobs)
    with concurrent.futures.ThreadPoolExecutor(max_workers=workers) as pool:
        return dict(zip(keys, pool.map(call, [jobs[k] for k in keys])))


# ------------------------------------------------------------------ fresh inputs: penalties no recorded row uses, launcher sizes
# (kind, algo, l, e, n, seed, costs): MAX_SCORE and READ_SIZE are the launcher's (engine.launcher_sizes) for l, e and the costs;
# every entry runs without and with BACKTRACE, on engine.gen_pairs' file and on conftest.tails_v1 of it.
FRESH = [
    ("nw", "nw", 100, 0.05, 300, 2101, dict(mismatch=4, gap=6)),
    ("nw", "nw", 150, 0.03, 300, 2102, dict(mismatch=1, gap=3)),
    ("nw", "nw", 70, 0.10, 300, 2103, dict(mismatch=6, gap=2)),
    ("nw", "nw", 250, 0.04, 200, 2104, dict(mismatch=5, gap=8)),
    ("swg8", "swg", 100, 0.02, 300, 2111, dict(mismatch=4, gap_o=5, gap_e=1)),
    ("swg8", "swg", 100, 0.05, 300, 2112, dict(mismatch=2, gap_o=2, gap_e=1)),
    ("swg8", "swg", 70, 0.03, 300, 2113, dict(mismatch=6, gap_o=1, gap_e=1)),
    ("swg8", "swg", 90, 0.04, 300, 2114, dict(mismatch=1, gap_o=6, gap_e=1)),
    ("swg16", "swg", 150, 0.05, 300, 2121, dict(mismatch=4, gap_o=5, gap_e=2)),
    ("swg16", "swg", 100, 0.10, 300, 2122, dict(mismatch=2, gap_o=2, gap_e=2)),
    ("swg16", "swg", 300, 0.10, 150, 2123, dict(mismatch=6, gap_o=1, gap_e=1)),
    ("swg16", "swg", 200, 0.15, 200, 2124, dict(mismatch=1, gap_o=6, gap_e=3)),
    ("wfa", "wfa", 100, 0.05, 300, 2131, dict(mismatch=5, gap_o=3, gap_e=1)),
    ("wfa", "wfa", 150, 0.02, 300, 2132, dict(mismatch=2, gap_o=6, gap_e=1)),
    ("wfa", "wfa", 70, 0.08, 300, 2133, dict(mismatch=7, gap_o=2, gap_e=3)),
    ("wfa", "wfa", 300, 0.04, 200, 2134, dict(mismatch=4, gap_o=4, gap_e=2)),
    ("wfa_red", "wfa", 100, 0.05, 300, 2141, dict(mismatch=3, gap_o=2, gap_e=1)),
    ("wfa_red", "wfa", 150, 0.02, 300, 2142, dict(mismatch=6, gap_o=6, gap_e=1)),
    ("wfa_red", "wfa", 1000, 0.05, 60, 2143, dict(mismatch=2, gap_o=4, gap_e=2)),
    ("wfa_red", "wfa", 300, 0.10, 200, 2144, dict(mismatch=5, gap_o=5, gap_e=5)),
]


def fresh_id(entry, backtrace):
    kind, _, l, e, _, _, costs = entry
    return "%s-l%d-e%g-%s%s" % (kind, l, e, "_".join(str(v) for v in costs.values()), "-bt" if backtrace else "")


def fresh_params(entry, backtrace):
    from aim_amd import engine
    kind, algo, l, e, _, _, costs = entry
    ms, rs = engine.launcher_sizes(algo, l, e, **costs)
    if kind == "swg8":
        assert ms < 127, (entry, ms)
    return engine.make_params(algo, ms, rs, backtrace=backtrace, reduce=kind == "wfa_red", swg_w16=kind == "swg16", **costs)


def fresh_inputs(entry, read_size):
    """[(label, input file bytes, pairs)] of an entry."""
    from aim_amd import engine
    from conftest import tails_v1
    _, _, l, e, n, seed, _ = entry
    data = engine.pairs_to_text(*engine.gen_pairs(seed, 0, n, l, e, read_size))
    return [("gen_pairs", data, n), ("tails_v1", tails_v1(data), n)]


def recorded_costs():
    """{algo: set of cost tuples} of every recorded row: (x, o, e) for WFA and SWG, (x, gap_i, gap_d) for NW."""
    import reference_rows as R
    out = {"wfa": {(3, 4, 1)}, "swg": {(3, 4, 1)}, "nw": {(3, 4, 4)}}
    for c in R.all_reference_rows() + judge_dataset_cases():
        k = judge_costs(c)
        if c["algo"] == "nw":
            g = k.get("gap", 4)
            out["nw"].add((k.get("mismatch", 3), k.get("gap_i", g), k.get("gap_d", g)))
        else:
            out[c["algo"]].add((k.get("mismatch", 3), k.get("gap_o", 4), k.get("gap_e", 1)))
    return out


# ------------------------------------------------------------------ the GPU module's cases
def gpu_cases():
    """[(kernel family, with CIGAR, table family, READ_SIZE)]: per family of reference_rows.FAMILIES and per score-only / CIGAR, the
    smallest READ_SIZE of low_complexity.TABLE (full_rows.TABLE and the wfa10 rows) whose pinned plan names a kernel of that family, among
    the table families the reference can express. A family that never plans with (or without) CIGAR has no such case."""
    import low_complexity as LC
    import reference_rows as R
    best = {}
    for fam, rows in LC.TABLE.items():
        if not expressible(fam):
            continue
        bt = bool(LC.FAMILIES[fam]["kw"].get("backtrace", False))
        for rs, plan in rows:
            k = (plan.split()[0][:-len("_kernel")], bt)
            if k[0] in R.FAMILIES and (k not in best or rs < best[k][1]):
                best[k] = (fam, rs)
    return [(k[0], k[1]) + best[k] for k in sorted(best)]


GPU_PAIRS = 288          # 32 rounds of the nine low-complexity classes


def gpu_batch(fam, rs):
    """(algo, aim_params_t, variant, (requests, patterns, texts, pairs left out)) of a GPU case."""
    import low_complexity as LC
    algo, params = LC.FAMILIES[fam]["algo"], LC.row_params(fam, rs)
    name, _, _ = params_config(params, algo)
    from aim_amd import capi
    bt = bool(params.flags & capi.FLAG_BACKTRACE)
    variant = live_variant(algo, params.max_score, bt, 2 if (params.flags & capi.FLAG_SWG_W16) else 0)
    req, pat, txt, _, _ = LC.low_complexity_batch(rs, GPU_PAIRS, LC.SEED + 1, params.max_score)
    return algo, params, name, domain_batch(algo, variant, bt, req, pat, txt)


# ------------------------------------------------------------------ every configuration
EXCLUDED_FILE = os.path.join(GOLDEN, "reference_live_excluded.json")


def excluded_counts():
    """{table case id: [pairs, pairs outside the reference's domain, fitted]} as committed (measure_excluded)."""
    with open(EXCLUDED_FILE) as f:
        return json.load(f)


def measure_excluded():
    """{case id: [pairs of the batch, pairs outside the domain, 1 where the batch is the fitted one]}."""
    out = {}
    for cid, source, key in table_cases():
        batch, refit = case_batch(source, key)[4:]
        out[cid] = [len(batch[0]) - 1 + batch[3], int(batch[3]), int(refit)]
    return out


def all_configs():
    out = recorded_configs()
    for _, source, key in table_cases():
        algo, params, _ = table_case(source, key)
        out.update([params_config(params, algo)[:2]])
    for entry in FRESH:
        for bt in (False, True):
            out.update([params_config(fresh_params(entry, bt), entry[1])[:2]])
    return out          # (the GPU module's cases are rows of low_complexity.ROWS)


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1] == "--excluded":          # rewrite the committed table of pairs outside the domain
        with open(EXCLUDED_FILE, "w") as f:
            json.dump(measure_excluded(), f, indent=0, sort_keys=True)
            f.write("\n")
