"""WFA across penalty sets: the batch, the table of rows and the comparison that tests/test_penalty_rows_cpu.py and
tests/test_penalty_rows_gpu.py use. Plain numpy; the library is asked for plans and (by the GPU module and the --run worker) for
alignments.

Two properties of the WFA kernels depend on the penalties alone. The ring depths: wfa_group_kernel keeps max(x, o + e) + 1 rows of
M and the next power of two above e rows of I / D and refuses more than 32 / 16; wfa_wave_kernel keeps the last 64 score
descriptors in LDS and gives up its live-window ring when (R + 1) rows no longer fit. And the reference's -10
(tests/sentinel_model.py): a cell no present source covers holds -10 instead of NULL, which changes scores as soon as
(10 + k) * x < o + k * e for a gap length k that occurs (sentinel_model.visible). On such a set global WFA returns the reference's
score, which can lie below the cost of the CIGAR it prints, and the kernels must return those bytes.

Every row runs one batch (batch()): READ_SIZE 112, 130 pairs, patterns of 96 bases."""
import os

import numpy as np

import full_rows as F

RS, N, PLEN = 112, 130, 96
SEED = F.SEED
GAPS = (1, 2, 3, 5, 8, 12)
PLACES = ("begin", "mid", "end")
N_CONSTRUCTED = 2 * len(GAPS) * len(PLACES) * 2
PLAN_ENV = {"AIM_SCRATCH_GB": "16", "AIM_CHIP_CUS": "256"}


def _other(rng, base):
    return F.ACGT[(int(np.searchsorted(F.ACGT, base)) + 1 + int(rng.integers(0, 3))) % 4]


def constructed_pairs(rng):
    """[(pattern, text, (kind, k, place, mismatch))]: one insertion (the text has k bases more) or deletion (k bases fewer) of
    k = 1, 2, 3, 5, 8, 12 bases at offset 0, at mid-read and at the end, without and with one mismatch a quarter into the read."""
    out = []
    for kind in ("ins", "del"):
        for k in GAPS:
            for place in PLACES:
                for mism in (False, True):
                    p = F.ACGT[rng.integers(0, 4, size=PLEN)]
                    at = {"begin": 0, "mid": PLEN // 2, "end": PLEN if kind == "ins" else PLEN - k}[place]
                    if kind == "ins":
                        t = np.concatenate([p[:at], F.ACGT[rng.integers(0, 4, size=k)], p[at:]])
                    else:
                        t = np.concatenate([p[:at], p[at + k:]])
                    if mism:
                        q = PLEN // 4 + (k if place == "begin" and kind == "ins" else 0) - (k if place == "begin" and kind == "del" else 0)
                        t[q] = _other(rng, t[q])
                    out.append((p, t, (kind, k, place, mism)))
    return out


def _random_pair(rng, edits):
    p = F.ACGT[rng.integers(0, 4, size=PLEN)]
    t = p.copy()
    for _ in range(edits):
        at = int(rng.integers(0, len(t)))
        what = int(rng.integers(0, 3))
        if what == 0:
            t[at] = _other(rng, t[at])
        elif what == 1:
            t = np.insert(t, at, F.ACGT[rng.integers(0, 4)])
        else:
            t = np.delete(t, at)
    return p, t


# places of the specials behind the constructed pairs; the pairs between them and the last are random
IDENTICAL, WITH_N, EMPTY_PATTERN, EMPTY_TEXT = N_CONSTRUCTED, N_CONSTRUCTED + 1, N_CONSTRUCTED + 2, N_CONSTRUCTED + 3
FIRST_LEAD8 = N_CONSTRUCTED + 4
N_LEAD8 = 16
FIRST_RANDOM = FIRST_LEAD8 + N_LEAD8
LEAD14, LEAD32 = N - 3, N - 2          # leading deletions longer than any constructed gap
FULL_ROW = N - 1
_BATCH = {}


def batch(pad="zero", rs=RS, n=N):
    """(requests, patterns[n][rs], texts[n][rs]) in the wire layout, the same for every row. Pairs 0 .. 71: constructed_pairs().
    IDENTICAL: a pattern against itself. WITH_N: an 'N' in each sequence, at different places. EMPTY_PATTERN, EMPTY_TEXT: plen = 0
    against 3 bases, 2 bases against tlen = 0 (short, so that MAX_SCORE stays the single gaps'). FIRST_LEAD8 ..: 16 pairs whose
    text lacks the pattern's first 8 bases and differs in 0 .. 3 more: a leading deletion of exactly 8 bases is the only gap on
    which (2, 5, 4) shows the -10 (sentinel_model.visible), so this set too has its 16 pairs below the optimum. Then random pairs
    of 0 .. 4 edits (substitution, insertion or deletion of one base each). LEAD14, LEAD32: texts that lack the pattern's first
    14 and 32 bases: the edge diagonal of such a gap is born at a score where the gap sources are present and out of range, so
    the reference reads NULL there and a kernel that read -10 would score these pairs lower (on the shorter gaps every set of
    the table reads -10 either way). FULL_ROW last: rs bases against rs bases, three edits, so the batch ends at the arrays' last
    byte. pad as in full_rows.full_row_batch. Built once per process and never changed afterwards."""
    key = (pad, rs, n)
    if key in _BATCH:
        return _BATCH[key]
    from aim_amd import capi
    rng = np.random.default_rng([SEED, rs, 0x70656E])
    req = np.zeros(n, dtype=capi.REQUEST_DTYPE)
    pat = np.zeros((n, rs), dtype=np.uint8)
    txt = np.zeros((n, rs), dtype=np.uint8)

    def put(i, p, t):
        pat[i, :len(p)], txt[i, :len(t)] = p, t
        req["pattern_len"][i], req["text_len"][i] = len(p), len(t)

    for i, (p, t, _) in enumerate(constructed_pairs(rng)):
        put(i, p, t)
    p = F.ACGT[rng.integers(0, 4, size=PLEN)]
    put(IDENTICAL, p, p)
    p, t = _random_pair(rng, 2)
    p[PLEN // 3] = ord("N")
    t[2 * PLEN // 3] = ord("N")
    put(WITH_N, p, t)
    put(EMPTY_PATTERN, p[:0], F.ACGT[rng.integers(0, 4, size=3)])
    put(EMPTY_TEXT, F.ACGT[rng.integers(0, 4, size=2)], p[:0])
    for i in range(FIRST_LEAD8, FIRST_RANDOM):
        p = F.ACGT[rng.integers(0, 4, size=PLEN)]
        t = p[8:].copy()
        for at in rng.choice(np.arange(16, PLEN - 8), size=(i - FIRST_LEAD8) % 4, replace=False):
            t[at] = _other(rng, t[at])
        put(i, p, t)
    for i in range(FIRST_RANDOM, n - 3):
        put(i, *_random_pair(rng, (i - FIRST_RANDOM) % 5))
    for i, k in ((LEAD14, 14), (LEAD32, 32)):
        p = F.ACGT[rng.integers(0, 4, size=PLEN)]
        put(i, p, p[k:])
    p = F.ACGT[rng.integers(0, 4, size=rs)]
    t = p.copy()
    t[rs // 5] = _other(rng, t[rs // 5])
    t = np.insert(np.delete(t, rs // 2), 3 * rs // 4, F.ACGT[rng.integers(0, 4)])
    put(n - 1, p, t)
    req["idx"] = 7000 + np.arange(n, dtype=np.uint32)
    if pad == "noise":
        nrng = np.random.default_rng([SEED, rs, 0x6E6F6973])
        col = np.arange(rs)[None, :]
        for rows, k in ((pat, "pattern_len"), (txt, "text_len")):
            noise = F.ACGTN[nrng.integers(0, 5, size=rows.shape)]
            behind = col >= req[k].astype(np.int64)[:, None]
            rows[behind] = noise[behind]
    for a in (req, pat, txt):
        a.flags.writeable = False
    _BATCH[key] = (req, pat, txt)
    return _BATCH[key]


# ------------------------------------------------------------------ the table
ALL4 = ((False, False), (True, False), (False, True), (True, True))          # (BACKTRACE, REDUCE)
SCORE_ONLY = ((False, False),)


def _row(pen, what, visible=False, flagsets=ALL4, extra_caps=(), env=None, **kw):
    return dict(pen=pen, what=what, visible=visible, flagsets=flagsets, extra_caps=tuple(extra_caps), env=env or {}, kw=kw)


# name -> the penalty set (x, o, e), the quantity the row is there for, and how it runs. Every row runs at the oracle's largest
# score of the batch, at its median (so that about half the pairs come back at MAX_SCORE + 1), where the set's unit
# gcd(x, o + e, e) is above 1 also at the median plus 1 (no multiple of the unit), and at its extra caps.
ROWS = {
    # the -10 is invisible: e <= x and o + e <= 11 x; the oracle equals the gap-affine optimum
    "15_16_15": _row((15, 16, 15), "ring_m=32 and ring_e=16 on wfa_group_kernel (at the median cap, and under REDUCE at the largest)"),
    "8_4_8": _row((8, 4, 8), "ring_e=16 and unit=4"),
    "31_28_3": _row((31, 28, 3), "ring_m=32 by the mismatch penalty, wfa_group_kernel at every cap"),
    "32_28_3": _row((32, 28, 3), "ring_m would be 33: wfa_wave_kernel, ring=33x"),
    "16_15_16": _row((16, 15, 16), "ring_e would be 32: wfa_wave_kernel"),
    "63_40_3": _row((63, 40, 3), "s - x is the oldest of wfa_wave_kernel's 64 descriptors in LDS: ring=64x"),
    "64_40_3": _row((64, 40, 3), "s - x is read through gmeta[]: ring=65x"),
    "70_40_3": _row((70, 40, 3), "s - x and s - (o + e) = 43 apart from the LDS descriptors: ring=71x"),
    "255_200_55": _row((255, 200, 55), "the deepest live-window ring of 16-bit offsets: ring=256x16", flagsets=SCORE_ONLY),
    "256_200_56": _row((256, 200, 56), "one row more: ring=0x0", flagsets=SCORE_ONLY),
    "127_100_27_w32": _row((127, 100, 27), "the deepest live-window ring of 32-bit offsets: ring=128x16", flagsets=SCORE_ONLY, w32=True),
    "128_100_28_w32": _row((128, 100, 28), "ring=0x0 under W32, at half the depth", flagsets=SCORE_ONLY, w32=True),
    "6_9_3": _row((6, 9, 3), "unit=3"),
    "10_15_5": _row((10, 15, 5), "unit=5 and ring_e=8"),
    "3_4_2": _row((3, 4, 2), "one step from the lane cost set (3,4,1): not a lane kernel at MAX_SCORE 5", extra_caps=(5,)),
    "3_5_1": _row((3, 5, 1), "one step from the lane cost set (3,4,1): not a lane kernel at MAX_SCORE 5", extra_caps=(5,)),
    "4_4_1": _row((4, 4, 1), "one step from the lane cost set (3,4,1): not a lane kernel at MAX_SCORE 5", extra_caps=(5,)),
    # the -10 is visible: byte for byte against the oracle
    "1_12_1": _row((1, 12, 1), "o + e > 11 x on the default plan; wfa_group_kernel G=64 at MAX_SCORE 620", True, extra_caps=(620,)),
    "1_12_1_wave": _row((1, 12, 1), "the same on wfa_wave_kernel", True, env={"AIM_FORCE_WAVE": "1"}),
    "1_12_1_w32": _row((1, 12, 1), "the same with 32-bit offsets: every byte equal to the flag-less run", True, w32=True),
    "1_30_1": _row((1, 30, 1), "ring_m=32 with the -10 visible; at MAX_SCORE 124 both row layouts (G=64 one home per diagonal, G=32 wlds=128)", True,
                   extra_caps=(124,)),
    # (width 4 is not feasible here: 16 pairs of 32 ring rows are more LDS than a workgroup has, and the planner keeps its own width)
    "1_30_1_G8": _row((1, 30, 1), "the same at width 8, the narrowest that fits 32 ring rows: reached at the median cap only -- at the largest score the rows are wider, the planner overrides the knob and the cases repeat 1_30_1's at G=32", True, env={"AIM_GROUP_G": "8"}),
    "1_30_1_G16": _row((1, 30, 1), "the same at width 16", True, env={"AIM_GROUP_G": "16"}),
    "1_31_1": _row((1, 31, 1), "ring_m would be 33: wfa_wave_kernel, ring=33x", True),
    "2_24_2": _row((2, 24, 2), "unit=2", True),
    "2_24_2_unit1": _row((2, 24, 2), "the same set without the unit", True, env={"AIM_GROUP_UNIT1": "1"}),
    "1_9_2": _row((1, 9, 2), "visible through e > x", True),
    "2_5_4": _row((2, 5, 4), "visible only on a leading deletion of 8 bases", True),
}
VISIBLE = [k for k, r in ROWS.items() if r["visible"]]
INVISIBLE = [k for k, r in ROWS.items() if not r["visible"]]
MODEL_INVISIBLE = ("15_16_15", "6_9_3", "3_5_1")         # the invisible rows the sentinel model is run on


def unit_of(pen):
    x, o, e = pen
    return int(np.gcd.reduce([x, o + e, e]))


def oracle_run(pen, ms, bt=False, red=False, pad="zero"):
    """(results, ops) of the oracle's global WFA on the batch; once per process, never changed afterwards."""
    key = (pen, ms, bt, red, pad)
    if key not in _ORACLE:
        from oracle import oracle
        req, pat, txt = batch(pad)
        x, o, e = pen
        op = oracle.params("wfa", ms, RS, mismatch=x, gap_o=o, gap_e=e, backtrace=bt, reduce=red)
        res, ops, worst = oracle.align_batch(op, req["pattern_len"], req["text_len"], pat, txt, nthreads=8)
        res.flags.writeable = False
        if ops is not None:
            ops.flags.writeable = False
        _ORACLE[key] = (res, ops, worst)
    return _ORACLE[key][:2]


_ORACLE = {}
UNCAPPED = 4000        # over every score of the batch under every set of the table


def oracle_scores(pen):
    return oracle_run(pen, UNCAPPED)[0]["score"]


def gotoh_scores(pen):
    """The gap-affine optimum of every pair of the batch (tests/endsfree_model.dp_scores, no free end); once per process."""
    if pen not in _GOTOH:
        from endsfree_model import dp_scores
        x, o, e = pen
        g = dp_scores(*batch(), x=x, o=o, e=e, ends_free=(0, 0, 0, 0))
        g.flags.writeable = False
        _GOTOH[pen] = g
    return _GOTOH[pen]


_GOTOH = {}


def caps_of(name):
    """The row's MAX_SCOREs: the oracle's largest score, its median, the median plus 1 where the unit is above 1, the extras."""
    r = ROWS[name]
    sc = np.sort(oracle_scores(r["pen"]))
    caps = [int(sc[-1]), int(sc[len(sc) // 2])]
    if unit_of(r["pen"]) > 1:
        caps.append(caps[1] + 1)
    return caps + [c for c in r["extra_caps"] if c not in caps]


def cases_of(name):
    return [(name, ms, bt, red) for ms in caps_of(name) for bt, red in ROWS[name]["flagsets"]]


def case_params(case):
    from aim_amd import engine
    name, ms, bt, red = case
    x, o, e = ROWS[name]["pen"]
    return engine.make_params("wfa", ms, RS, mismatch=x, gap_o=o, gap_e=e, backtrace=bt, reduce=red, **ROWS[name]["kw"])


def case_id(case):
    return "%s-ms%d%s%s" % (case[0], case[1], "-bt" if case[2] else "", "-reduce" if case[3] else "")


# ------------------------------------------------------------------ plans
PLANS_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "penalty_rows_plans.json")
PLAN_TOKENS = ("G", "ring", "bidir", "endsfree", "affine2p")   # of aim_plan_describe's line, next to the kernel name and a final " w32"
DEBUG_TOKENS = ("ring_m", "ring_e", "wlds", "unit")      # of AIM_PLAN_DEBUG's wfa_group line


def plan_env(env):
    from wfa_group_rows import plan_env as pe
    return pe(dict(PLAN_ENV, **env))


def run_env(env):
    from wfa_group_rows import run_env as re_
    return re_(env)


def plan_tokens(line, debug):
    """What the table pins of a case's plan: 'kernel G=.. ring=.. [w32]' and, for wfa_group_kernel, 'ring_m=.. ring_e=.. wlds=..
    unit=..' of the debug line."""
    w = line.split()
    want = [w[0]] + [t for t in w[1:] if t.split("=")[0] in PLAN_TOKENS] + (["w32"] if "w32" in w[1:] else [])
    d = [t for t in debug.split() if t.split("=")[0] in DEBUG_TOKENS]
    return " ".join(want), " ".join(d)


def _describe(params, n):
    """(aim_plan_describe's line, the last wfa_group line AIM_PLAN_DEBUG printed for it); AIM_PLAN_DEBUG is set by the caller."""
    import sys
    import tempfile
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile() as f:
        os.dup2(f.fileno(), 2)
        try:
            line = F.plan_line(params, n)
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        f.seek(0)
        dbg = [l for l in f.read().decode(errors="replace").splitlines() if l.startswith("[aim plan] wfa_group G=")]
    return line, (dbg[-1] if dbg and line.startswith("wfa_group_kernel") else "")


def describe_rows(names):
    """{case id: [plan tokens, debug tokens, aim_scratch_bytes, aim_kernel_name]} of every case of the rows, under the
    environment as it is."""
    from aim_amd import capi
    lib = capi.load()
    out = {}
    for name in names:
        for case in cases_of(name):
            p = case_params(case)
            toks, dbg = plan_tokens(*_describe(p, N))
            out[case_id(case)] = [toks, dbg, int(lib.aim_scratch_bytes(capi.params_ref(p), N)), lib.aim_kernel_name(capi.params_ref(p)).decode()]
    return out


def pinned_plans():
    import json
    with open(PLANS_FILE) as f:
        return json.load(f)


def expected_plan(case):
    """(plan tokens, debug tokens) the case ran under when the table was made."""
    return tuple(pinned_plans()[case_id(case)])


# ------------------------------------------------------------------ the flags that promise a minimum cost, on deep invisible sets
# Ends-free WFA (free lengths 3, 0, 16, 5) and dual-cost WFA on penalty sets that need the deepest rings and on which the -10 cannot
# show (the only ones these flags accept), against their DP models. The second piece (30, 1) has o2 + e2 = 31, a 32-row M ring,
# and is the cheaper one from gaps of 12 bases on. Each runs at its model's largest score and at its median.
FLAG_ENDS_FREE = (3, 0, 16, 5)
FLAG_GAP2 = (30, 1)
FLAG_ROWS = {"endsfree_15_16_15": ("endsfree", (15, 16, 15)), "endsfree_31_28_3": ("endsfree", (31, 28, 3)),
             "affine2p_4_8_3": ("affine2p", (4, 8, 3))}
_FLAG_MODEL = {}


def flag_scores(name):
    """The flag's DP model on the batch; once per process."""
    if name not in _FLAG_MODEL:
        from wfa_group_rows import variant_scores
        kind, (x, o, e) = FLAG_ROWS[name]
        want = variant_scores(kind, *batch(), dict(mismatch=x, gap_o=o, gap_e=e), ends_free=FLAG_ENDS_FREE, gap2=FLAG_GAP2)
        want.flags.writeable = False
        _FLAG_MODEL[name] = want
    return _FLAG_MODEL[name]


def flag_cases(name):
    want = flag_scores(name)
    return [(name, ms, bt) for ms in (int(want.max()), int(np.sort(want)[len(want) // 2])) for bt in (False, True)]


def flag_case_id(case):
    return "flag-%s-ms%d%s" % (case[0], case[1], "-bt" if case[2] else "")


def flag_params(case):
    from aim_amd import engine
    name, ms, bt = case
    kind, (x, o, e) = FLAG_ROWS[name]
    kw = dict(ends_free=FLAG_ENDS_FREE) if kind == "endsfree" else dict(gap2=FLAG_GAP2)
    return engine.make_params("wfa", ms, RS, mismatch=x, gap_o=o, gap_e=e, backtrace=bt, **kw)


def describe_flag_rows():
    """{flag case id: [plan tokens, debug tokens]} under the environment as it is."""
    return {flag_case_id(c): list(plan_tokens(*_describe(flag_params(c), N))) for name in FLAG_ROWS for c in flag_cases(name)}


# ------------------------------------------------------------------ running (in this process, or as a worker under the row's knobs)
def align(params, req, pat, txt):
    """(results, ops, plan line, fallback pairs): configure, push, launch, pull on one device."""
    from aim_amd import engine
    with engine.DeviceSet(1) as s:
        s.configure(params, len(req))
        s.push(0, req, pat, txt)
        s.launch()
        res, ops = s.pull(0, check=False)
        return res, ops, s.plan_describe(0), s.fallback_pairs(0)


def run_rows(names, pad="zero", bt=None):
    """{case id + "/res" | "/ops" | "/line" | "/todo": ...} of every case of the rows (bt: of those with or without BACKTRACE) on
    the device, under the environment as it is."""
    out = {}
    req, pat, txt = batch(pad)
    for name in names:
        for case in cases_of(name):
            if bt is not None and case[2] != bt:
                continue
            res, ops, line, todo = align(case_params(case), req, pat, txt)
            k = case_id(case)
            out[k + "/res"], out[k + "/line"], out[k + "/todo"] = res, line, todo
            if ops is not None:
                out[k + "/ops"] = ops
    return out


def check_case(case, out, pad="zero", pinned=True):
    """The GPU module's comparison of one case: the plan line it ran under (the kernel and shape tokens of the table; the debug
    tokens are checked without a device), every per-pair output against the oracle, and the to-do list's length."""
    k = case_id(case)
    name, ms, bt, red = case
    line, todo = str(out[k + "/line"]), int(out[k + "/todo"])
    want = expected_plan(case)[0]
    print("%s: %s; to-do list %d" % (k, line, todo))
    if pinned:
        assert F.plan_matches(line, want), "ran under %r, the table says %r" % (line, want)
    else:          # (a run under knobs that change the shape: the kernel only)
        assert line.split()[0] == want.split()[0], (line, want)
    req, _, _ = batch(pad)
    ores, oops = oracle_run(ROWS[name]["pen"], ms, bt, red, pad)
    F.compare(out[k + "/res"], out.get(k + "/ops"), ores, oops, req, bt)
    if line.startswith("wfa_group_kernel"):
        # the kernel's to-do list: the pair with 'N' bytes, which cannot be packed into 2-bit rows (what every wfa_group row of
        # tests/wfa_group_rows.py and full_rows.py hands on), and nothing else
        assert todo == 1, "%d pairs on the to-do list" % todo
    else:
        assert todo == 0, todo


if __name__ == "__main__":
    import json
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import penalty_rows as P          # (one copy of the caches and tables, whatever this file was started as)
    if sys.argv[1] == "--plans":         # --plans ROW ...: describe_rows under the environment as it is, as JSON
        json.dump(P.describe_rows(sys.argv[2:]), sys.stdout)
    elif sys.argv[1] == "--flag-plans":
        json.dump(P.describe_flag_rows(), sys.stdout)
    elif sys.argv[1] == "--run":         # --run OUT.npz PAD score|cigar ROW ...
        np.savez(sys.argv[2], **P.run_rows(sys.argv[5:], sys.argv[3], sys.argv[4] == "cigar"))
