"""Every width G of wfa_group_kernel under each WFA variant (AIM_FLAG_ENDSFREE, AIM_FLAG_AFFINE2P, AIM_FLAG_LINEAR) and as the
second stage of AIM_FLAG_WFA_ESCALATE: the table of rows that reach each instantiation, the batches, the models' scores and the
comparison both test modules use (tests/test_wfa_group_rows_cpu.py, tests/test_wfa_group_rows_gpu.py). Plain numpy; the library is
asked for gen_pairs rows, for plans and (by the GPU module and the --run worker) for alignments.

tests/full_rows.py walks READ_SIZE through G = 1 .. 64 for the global kernels only. Here the key of a row is (kind, G, backtrace)
for the three variants and (kind, G, backtrace, reduce) for the escalation pass. How the rows are chosen (make_table()):

  * default plan first: the first READ_SIZE (a multiple of 8) at which the plan under no AIM_GROUP_* variable gives that G, with
    full_rows.pairs_for(READ_SIZE) pairs and MAX_SCORE by the launchers' rule at 2 % (10 % where the 2 % rule reaches the width
    only beyond READ_SIZE 2048: the models would then run 3000-base pairs);
  * forced second: a (kind, G) the default planner never gives over READ_SIZE 8 .. 4096 is forced with AIM_GROUP_G at the
    smallest READ_SIZE at which the forced plan is feasible;
  * escalate: READ_SIZE over the lane kernels' range, MAX_SCORE in {11, 25, 50, 100}; the widths no default plan gives are forced.
    The second stage's modulo-row kernels (rows of 96 entries, G = 16 and 8) are no default plan's -- they need 2 * MAX_SCORE + 3
    >= 192 and 4 * MAX_SCORE <= READ_SIZE, beyond the lane kernels' READ_SIZE -- but AIM_GROUP_WLDS=96 reaches them: kind
    "escalate_modrows".

The G = 4 and G = 32 rows of every variant run the second penalty set (mismatch 4, gap_o 6, gap_e 2; gap-linear 2 / 3): one width
that stages its rows in LDS and one that reduces over two DPP rows. full_row_batch() builds every READ_SIZE from 8 up (its head
pairs shrink with READ_SIZE), so the smallest rows need no other constructions; what changes in a row's batch is its gen_pairs
body only (row_batch(): the escalation rows, and CLEAN_BODY)."""
import contextlib
import os
import re

import numpy as np

import full_rows as F

WIDTHS = (1, 2, 4, 8, 16, 32, 64)
VARIANTS = ("endsfree", "affine2p", "linear")
ESC_SCORES = (11, 25, 50, 100)
ENDS_FREE = (3, 0, 16, 5)        # asymmetric: a mix-up of the four lengths or of begin and end changes scores
GAP2 = (24, 1)
ALT_WIDTHS = (4, 32)             # the rows on the second penalty set
PENALTIES = {                    # kind -> (default, second set): make_params keywords
    "endsfree": (dict(mismatch=3, gap_o=4, gap_e=1), dict(mismatch=4, gap_o=6, gap_e=2)),
    "affine2p": (dict(mismatch=3, gap_o=4, gap_e=1), dict(mismatch=4, gap_o=6, gap_e=2)),
    "linear": (dict(mismatch=3, gap_e=1), dict(mismatch=2, gap_e=3)),
}
RATES = (0.01, 0.02, 0.05, 0.10)
PLAN_ENV = {"AIM_SCRATCH_GB": "16", "AIM_CHIP_CUS": "256"}       # what test_full_rows_cpu.py plans under
SEED = F.SEED

# An instantiation no knob setting reaches: (key, why). Every one of wfa_group_kernel's variant and to-do-input instantiations is
# reached by a row below; tests/test_wfa_group_rows_cpu.py checks that no swept plan lands here.
UNREACHED = []


def score_rule(kind, rs, rate, pen):
    """MAX_SCORE of a read that fills READ_SIZE at the error rate: full_rows.launcher_score with the variant's cost per edit
    (a gap base at gap_o + gap_e), linear_model.max_score_rule for gap-linear."""
    if kind == "linear":
        from linear_model import max_score_rule
        return max(1, max_score_rule(rs / (1.0 + rate), rate, pen["mismatch"], pen["gap_e"]))
    return F.launcher_score(rs, rate, pen["gap_o"] + pen["gap_e"])


def pen_of(kind, G):
    return PENALTIES[kind][1 if G in ALT_WIDTHS else 0]


# key -> (READ_SIZE, MAX_SCORE, penalties, environment); made by make_table() (python tests/wfa_group_rows.py --make-table) and
# checked against the planner by tests/test_wfa_group_rows_cpu.py: when a planner change moves an edge, that test prints the new
# line and the row takes the new first READ_SIZE of its width. A row with AIM_GROUP_* in its environment is a forced one.
TABLE = {
    ('endsfree', 1, False): (8, 1, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_G': '1'}),
    ('endsfree', 1, True): (8, 1, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_G': '1'}),
    ('endsfree', 2, False): (8, 1, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_G': '2'}),
    ('endsfree', 2, True): (8, 1, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_G': '2'}),
    ('endsfree', 4, False): (8, 2, {'mismatch': 4, 'gap_o': 6, 'gap_e': 2}, {}),
    ('endsfree', 4, True): (8, 2, {'mismatch': 4, 'gap_o': 6, 'gap_e': 2}, {}),
    ('endsfree', 8, False): (56, 6, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('endsfree', 8, True): (56, 6, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('endsfree', 16, False): (232, 23, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('endsfree', 16, True): (232, 23, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('endsfree', 32, False): (200, 32, {'mismatch': 4, 'gap_o': 6, 'gap_e': 2}, {}),
    ('endsfree', 32, True): (200, 32, {'mismatch': 4, 'gap_o': 6, 'gap_e': 2}, {}),
    ('endsfree', 64, False): (696, 317, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('endsfree', 64, True): (696, 317, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('affine2p', 1, False): (8, 1, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_G': '1'}),
    ('affine2p', 1, True): (8, 1, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_G': '1'}),
    ('affine2p', 2, False): (8, 1, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_G': '2'}),
    ('affine2p', 2, True): (8, 1, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_G': '2'}),
    ('affine2p', 4, False): (8, 2, {'mismatch': 4, 'gap_o': 6, 'gap_e': 2}, {}),
    ('affine2p', 4, True): (8, 2, {'mismatch': 4, 'gap_o': 6, 'gap_e': 2}, {}),
    ('affine2p', 8, False): (24, 3, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('affine2p', 8, True): (24, 3, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('affine2p', 16, False): (72, 8, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('affine2p', 16, True): (72, 8, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('affine2p', 32, False): (104, 17, {'mismatch': 4, 'gap_o': 6, 'gap_e': 2}, {}),
    ('affine2p', 32, True): (104, 17, {'mismatch': 4, 'gap_o': 6, 'gap_e': 2}, {}),
    ('affine2p', 64, False): (944, 93, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('affine2p', 64, True): (944, 93, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('linear', 1, False): (8, 2, {'mismatch': 3, 'gap_e': 1}, {}),
    ('linear', 1, True): (8, 2, {'mismatch': 3, 'gap_e': 1}, {}),
    ('linear', 2, False): (104, 6, {'mismatch': 3, 'gap_e': 1}, {}),
    ('linear', 2, True): (104, 6, {'mismatch': 3, 'gap_e': 1}, {}),
    ('linear', 4, False): (208, 15, {'mismatch': 2, 'gap_e': 3}, {}),
    ('linear', 4, True): (208, 15, {'mismatch': 2, 'gap_e': 3}, {}),
    ('linear', 8, False): (616, 26, {'mismatch': 3, 'gap_e': 1}, {}),
    ('linear', 8, True): (616, 26, {'mismatch': 3, 'gap_e': 1}, {}),
    ('linear', 16, False): (1280, 52, {'mismatch': 3, 'gap_e': 1}, {}),
    ('linear', 16, True): (1280, 52, {'mismatch': 3, 'gap_e': 1}, {}),
    ('linear', 32, False): (624, 171, {'mismatch': 2, 'gap_e': 3}, {}),
    ('linear', 32, True): (624, 171, {'mismatch': 2, 'gap_e': 3}, {}),
    ('linear', 64, False): (248, 10, {'mismatch': 3, 'gap_e': 1}, {}),
    ('linear', 64, True): (248, 10, {'mismatch': 3, 'gap_e': 1}, {}),
    ('escalate', 1, False, False): (72, 11, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_G': '1'}),
    ('escalate', 1, False, True): (72, 11, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_G': '1'}),
    ('escalate', 1, True, False): (72, 11, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_G': '1'}),
    ('escalate', 1, True, True): (72, 11, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_G': '1'}),
    ('escalate', 2, False, False): (72, 11, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_G': '2'}),
    ('escalate', 2, False, True): (72, 11, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_G': '2'}),
    ('escalate', 2, True, False): (72, 11, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_G': '2'}),
    ('escalate', 2, True, True): (72, 11, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_G': '2'}),
    ('escalate', 4, False, False): (72, 11, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('escalate', 4, False, True): (72, 11, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('escalate', 4, True, False): (72, 11, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('escalate', 4, True, True): (72, 11, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('escalate', 8, False, False): (72, 25, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('escalate', 8, False, True): (72, 25, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('escalate', 8, True, False): (72, 25, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('escalate', 8, True, True): (72, 25, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('escalate', 16, False, False): (72, 50, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('escalate', 16, False, True): (72, 50, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('escalate', 16, True, False): (72, 50, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('escalate', 16, True, True): (72, 50, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('escalate', 32, False, False): (72, 100, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('escalate', 32, False, True): (72, 50, {'mismatch': 4, 'gap_o': 6, 'gap_e': 2}, {}),
    ('escalate', 32, True, False): (72, 100, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {}),
    ('escalate', 32, True, True): (72, 50, {'mismatch': 4, 'gap_o': 6, 'gap_e': 2}, {}),
    ('escalate', 64, False, False): (72, 11, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_G': '64'}),
    ('escalate', 64, False, True): (72, 11, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_G': '64'}),
    ('escalate', 64, True, False): (72, 11, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_G': '64'}),
    ('escalate', 64, True, True): (72, 11, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_G': '64'}),
    ('escalate_modrows', 16, False, True): (72, 50, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_WLDS': '96'}),
    ('escalate_modrows', 16, True, True): (72, 50, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_WLDS': '96'}),
    ('escalate_modrows', 8, False, True): (72, 50, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_WLDS': '96', 'AIM_GROUP_G': '8'}),
    ('escalate_modrows', 8, True, True): (72, 50, {'mismatch': 3, 'gap_o': 4, 'gap_e': 1}, {'AIM_GROUP_WLDS': '96', 'AIM_GROUP_G': '8'}),
}

# Pairs on the to-do list (aim_set_fallback_pairs) per variant row and padding, as first measured on an MI355X: every row hands on
# the one pair with 'N' in its last column and nothing else; a row that measures otherwise gets its own entry here.
_TODO_N_LAST = 1
_TODO = {}


def expected_todo(key, pad):
    return _TODO.get((key, pad), _TODO_N_LAST)


def is_forced(key):
    return any(k.startswith("AIM_GROUP_") for k in TABLE[key][3])


def row_id(key):
    return "-".join([key[0], "G%d" % key[1], "bt" if key[2] else "score"] + (["reduce"] if len(key) > 3 and key[3] else []))


VARIANT_ROWS = [k for k in TABLE if k[0] in VARIANTS]
ESCALATE_ROWS = [k for k in TABLE if k[0].startswith("escalate")]


def row_kwargs(key):
    """make_params keywords of a row, without max_score / read_size."""
    kind, bt = key[0], key[2]
    rs, ms, pen, env = TABLE[key]
    kw = dict(pen, backtrace=bt)
    if kind == "endsfree":
        kw["ends_free"] = ENDS_FREE
    elif kind == "affine2p":
        kw["gap2"] = GAP2
    elif kind == "linear":
        kw["linear"] = True
    else:
        kw.update(reduce=key[3], escalate=True)
    return kw


def row_params(key, **over):
    from aim_amd import engine
    rs, ms, pen, env = TABLE[key]
    return engine.make_params("wfa", ms, rs, **dict(row_kwargs(key), **over))


def row_token(key):
    """The variant's own token of the plan line."""
    return {"endsfree": " endsfree=%d,%d,%d,%d" % ENDS_FREE, "affine2p": " affine2p=%d,%d" % GAP2, "linear": " linear"}.get(key[0], " escalate=")


def group_line(key, line):
    """The wfa_group_kernel stage of a row's plan line: the line itself, the second stage under escalation. None when the
    plan is another."""
    if key[0].startswith("escalate"):
        if " | " not in line:
            return None
        line = line.split(" | ")[1]
    return line if line.startswith("wfa_group_kernel ") else None


def line_width(key, line):
    g = group_line(key, line)
    m = re.search(r" G=(\d+) ", g) if g else None
    return int(m.group(1)) if m else None


def escalate_cap(line):
    m = re.search(r" escalate=(\d+)$", line)
    return int(m.group(1)) if m else None


def plan_env(env):
    """The environment a row is planned under without a device: every AIM_* variable but AIM_LIB cleared, the chip fixed."""
    from reference_rows import knob_env
    return knob_env(dict(PLAN_ENV, **env))


def run_env(env):
    """... and run under on the device: the chip is the real one."""
    out = {k: v for k, v in os.environ.items() if not k.startswith("AIM_") or k == "AIM_LIB"}
    out.update(env)
    return out


# ------------------------------------------------------------------ batches and models
# Variant rows whose READ_SIZE is so small that gen_pairs' one edit per pair (its least) puts nearly every pair over MAX_SCORE:
# every other pair of their body comes from gen_pairs at error rate 0, so that a third of the batch stays under the cap.
CLEAN_BODY = {("affine2p", 1), ("affine2p", 2), ("affine2p", 4), ("affine2p", 8)}


def _put_body(req, pat, txt, sel, body, pad, salt):
    """Pairs `sel` of the batch become the gen_pairs rows `body` (at the same places); behind their lengths the batch's padding."""
    breq, bpat, btxt = body
    rs = pat.shape[1]
    nrng = np.random.default_rng([SEED, rs, salt])
    for rows, brows, key in ((pat, bpat, "pattern_len"), (txt, btxt, "text_len")):
        new = brows[sel - F.N_SPECIAL]
        if pad == "noise":
            noise = F.ACGTN[nrng.integers(0, 5, size=new.shape)]
            new = np.where(np.arange(rs)[None, :] >= breq[key][sel - F.N_SPECIAL].astype(np.int64)[:, None], noise, new)
        rows[sel] = new
        req[key][sel] = breq[key][sel - F.N_SPECIAL]


def row_batch(key, pad="zero"):
    """full_rows.full_row_batch at the row's READ_SIZE. The escalation rows carry gen_pairs rows at 5 % in place of the 2 % body:
    the pairs the first stage leaves then lie all over the batch, not at its front. CLEAN_BODY rows: see there."""
    from aim_amd import engine
    rs = TABLE[key][0]
    n = F.pairs_for(rs)
    req, pat, txt = F.full_row_batch(rs, n, SEED, pad)
    body = n - F.N_SPECIAL - 1
    if key[0].startswith("escalate"):
        l = max(1, (rs - 8) * 100 // 105)
        _put_body(req, pat, txt, F.N_SPECIAL + np.arange(body), engine.gen_pairs(SEED, 0, body, l, 0.05, rs), pad, 0x657363)
    elif (key[0], key[1]) in CLEAN_BODY:
        l = max(1, (rs - 8) * 100 // 104)
        _put_body(req, pat, txt, F.N_SPECIAL + np.arange(0, body, 2), engine.gen_pairs(SEED + 1, 0, body, l, 0.0, rs), pad, 0x636C65)
    return req, pat, txt


def variant_scores(kind, req, pat, txt, pen, ends_free=ENDS_FREE, gap2=GAP2):
    """The variant's optimum per pair by its DP model (tests/endsfree_model.py, affine2p_model.py, linear_model.py)."""
    if kind == "endsfree":
        from endsfree_model import dp_scores
        return dp_scores(req, pat, txt, x=pen["mismatch"], o=pen["gap_o"], e=pen["gap_e"], ends_free=ends_free)
    if kind == "affine2p":
        from affine2p_model import dp_scores
        return dp_scores(req, pat, txt, x=pen["mismatch"], o1=pen["gap_o"], e1=pen["gap_e"], o2=gap2[0], e2=gap2[1])
    from linear_model import dp_scores
    return dp_scores(req, pat, txt, x=pen["mismatch"], g=pen["gap_e"])


def cheapest_edit(kind, pen):
    """The least cost a single edit adds to an alignment."""
    if kind == "linear":
        return min(pen["mismatch"], pen["gap_e"])
    return min(pen["mismatch"], pen["gap_o"] + pen["gap_e"])


_MODEL, _ORACLE = {}, {}


def model_row(key):
    """Model scores of a variant row's batch (the sequences are the same under both paddings and with and without BACKTRACE);
    computed once per process and never changed afterwards."""
    rs, ms, pen, env = TABLE[key]
    k = (key[0], rs, tuple(sorted(pen.items())), (key[0], key[1]) in CLEAN_BODY)
    if k not in _MODEL:
        want = variant_scores(key[0], *row_batch(key), pen)
        want.flags.writeable = False
        _MODEL[k] = want
    return _MODEL[k]


def oracle_of(req, pat, txt, ms, rs, pen, bt, reduce=False):
    from oracle import oracle
    op = oracle.params("wfa", ms, rs, backtrace=bt, reduce=reduce, **pen)
    res, ops, _ = oracle.align_batch(op, req["pattern_len"], req["text_len"], pat, txt, nthreads=8)
    return res, ops


def oracle_row(key, pad="zero"):
    """The oracle's global WFA on the row's batch at the row's MAX_SCORE, penalties and BACKTRACE / REDUCE; once per process."""
    rs, ms, pen, env = TABLE[key]
    red = len(key) > 3 and key[3]
    k = (key[0].startswith("escalate"), (key[0], key[1]) in CLEAN_BODY, rs, ms, tuple(sorted(pen.items())), key[2], red, pad)
    if k not in _ORACLE:
        res, ops = oracle_of(*row_batch(key, pad), ms, rs, pen, key[2], red)
        res.flags.writeable = False
        if ops is not None:
            ops.flags.writeable = False
        _ORACLE[k] = (res, ops)
    return _ORACLE[k]


# ------------------------------------------------------------------ the comparison
def check_variant(kind, pen, ms, req, pat, txt, res, ops, bt, want, ends_free=ENDS_FREE, gap2=GAP2):
    """Part 2's comparison of a variant run with the variant's model: every score equals the model's, capped (over MAX_SCORE:
    MAX_SCORE + 1), every status is AIM_PAIR_OK; with BACKTRACE an over-cap pair has the ops range the header documents for the
    flag (ends-free: empty; affine2p and gap-linear: global WFA's one byte), and every other pair's CIGAR uses up both sequences,
    tells 'M' from 'X' truthfully and re-scores to the reported score. Raises AssertionError naming the first pair that differs."""
    import affine2p_model
    import endsfree_model
    import linear_model
    assert len(res) == len(req) == len(want)
    assert np.array_equal(res["idx"], req["idx"]), "idx differs"
    capped = np.where(want <= ms, want, ms + 1)
    bad = np.nonzero(res["score"] != capped)[0]
    assert bad.size == 0, "score differs at pair %d: got %d, model %d (plen %d tlen %d; %d pairs differ)" % (
        bad[0], res["score"][bad[0]], capped[bad[0]], req["pattern_len"][bad[0]], req["text_len"][bad[0]], bad.size)
    bad = np.nonzero(res["status"] != 0)[0]
    assert bad.size == 0, "status %d at pair %d" % (res["status"][bad[0]] if bad.size else 0, bad[0] if bad.size else -1)
    if not bt:
        return
    x = pen["mismatch"]
    for i in range(len(req)):
        r = res[i]
        plen, tlen = int(req["pattern_len"][i]), int(req["text_len"][i])
        b, e = int(r["begin_offset"]), int(r["end_offset"])
        if want[i] > ms:
            if kind == "endsfree":
                assert b == e, "over-cap pair %d: ops range [%d, %d) is not empty" % (i, b, e)
            else:
                assert r["max_operations"] == plen + tlen and e == plen + tlen and b == e - 1, "over-cap pair %d: ops range [%d, %d)" % (i, b, e)
            continue
        assert r["max_operations"] == plen + tlen, "max_operations differs at pair %d" % i
        assert 0 <= b <= e <= ops.shape[1], "ops range [%d, %d) at pair %d" % (b, e, i)
        s = bytes(ops[i, b:e]).decode("latin-1")
        p, t = bytes(pat[i, :plen]), bytes(txt[i, :tlen])
        err = endsfree_model.check_cigar(s, p, t)
        assert err is None, "CIGAR of pair %d: %s (%s)" % (i, err, s[-60:])
        if kind == "endsfree":
            cost = endsfree_model.rescore(s, plen, tlen, x=x, o=pen["gap_o"], e=pen["gap_e"], ends_free=ends_free)
        elif kind == "affine2p":
            cost = affine2p_model.rescore(s, x=x, o1=pen["gap_o"], e1=pen["gap_e"], o2=gap2[0], e2=gap2[1])
        else:
            cost = linear_model.rescore(s, x=x, g=pen["gap_e"])
        assert cost == r["score"], "CIGAR of pair %d re-scores to %d, reported %d (%s)" % (i, cost, r["score"], s[-60:])


def same_bytes(a, b):
    """Two runs gave the same result rows and the same ops[begin_offset, end_offset) bytes."""
    (res0, ops0), (res1, ops1) = a, b
    bad = np.nonzero(res0 != res1)[0]
    assert bad.size == 0, "result row differs at pair %d: %r / %r" % (bad[0], res0[bad[0]], res1[bad[0]])
    if ops0 is not None:
        for i in range(len(res0)):
            lo, hi = int(res0["begin_offset"][i]), int(res0["end_offset"][i])
            assert bytes(ops0[i, lo:hi]) == bytes(ops1[i, lo:hi]), "ops differ at pair %d: %r / %r" % (
                i, bytes(ops0[i, lo:hi])[-60:], bytes(ops1[i, lo:hi])[-60:])


def degenerate_runs(key):
    """[(name, make_params keywords)] of the parameter settings under which the row's variant must reproduce global WFA."""
    rs, ms, pen, env = TABLE[key]
    if key[0] == "endsfree":
        return [("free0", dict(pen, ends_free=(0, 0, 0, 0)))]
    if key[0] == "affine2p":
        return [("same", dict(pen, gap2=(pen["gap_o"], pen["gap_e"]))), ("never", dict(pen, gap2=(ms, 1)))]
    return []


def check_row(key, pad, out):
    """Every check of part 2 on what run_row() returned for a row (in this process or in a worker)."""
    rs, ms, pen, env = TABLE[key]
    bt = key[2]
    req, pat, txt = row_batch(key, pad)
    n = len(req)
    ops = out.get("ops")
    line, todo = str(out["line"]), int(out["todo"])
    print("%s %s: %s; to-do list %d of %d pairs" % (row_id(key), pad, line, todo, n))
    assert line_width(key, line) == key[1] and row_token(key) in line, line
    if key[0] in VARIANTS:
        check_variant(key[0], pen, ms, req, pat, txt, out["res"], ops, bt, model_row(key))
        wline = str(out["wave_line"])
        assert wline.startswith("wfa_wave_kernel "), wline
        same_bytes((out["res"], ops), (out["wave_res"], out.get("wave_ops")))
        for name, kw in degenerate_runs(key):
            if name + "_res" not in out:
                continue
            dline = str(out[name + "_line"])
            print("  %s: %s" % (name, dline))
            # (a second piece of MAX_SCORE + 1 needs a ring that deep: beyond 31 rows the plan is wfa_wave_kernel's)
            assert line_width(key, dline) == key[1] or (name == "never" and ms + 1 > 31 and dline.startswith("wfa_wave_kernel ")), dline
            ores, oops = oracle_row(key, pad)
            if key[0] == "endsfree" and bt:
                ores = empty_over_cap(ores, ms)
            F.compare(out[name + "_res"], out.get(name + "_ops"), ores, oops, req, bt)
        assert 4 * todo <= n, "%d of %d pairs left for wfa_wave_kernel" % (todo, n)
        assert todo == expected_todo(key, pad), (todo, expected_todo(key, pad))
    else:
        c = escalate_cap(line)
        assert c is not None and 0 < c < ms, line
        ores, oops = oracle_row(key, pad)
        F.compare(out["res"], ops, ores, oops, req, bt)
        over = escalated(ores, c)
        assert over.size >= 10 and over[0] // 64 != over[-1] // 64, over


def empty_over_cap(ores, ms):
    """Global WFA's result rows as ends-free WFA with no free end gives them: the same but for a pair over MAX_SCORE, whose ops
    range the flag documents as empty (begin_offset == end_offset) where global WFA's holds one byte."""
    out = ores.copy()
    over = out["score"] > ms
    out["begin_offset"][over] = out["end_offset"][over]
    return out


def escalated(ores, c):
    """Indices of the pairs the first stage leaves for the second: the oracle's score (at MAX_SCORE) is over the first cap."""
    return np.nonzero(ores["score"] > c)[0]


# ------------------------------------------------------------------ running a row (in this process, or as a worker under the row's knobs)
def _align(params, req, pat, txt):
    from aim_amd import engine
    with engine.DeviceSet(1) as s:
        s.configure(params, len(req))
        s.push(0, req, pat, txt)
        s.launch()
        res, ops = s.pull(0, check=False)
        return res, ops, s.plan_describe(0), s.fallback_pairs(0)


@contextlib.contextmanager
def _env(**env):
    """The variables set for the block, then as they were (the library reads them at every plan)."""
    was = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in was.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def run_row(key, pad):
    """The row's batch on the device under the environment as it is (the caller has set the row's knobs): the row's own params;
    for a variant row also the same params on wfa_wave_kernel (AIM_FORCE_WAVE=1) and, zero-padded, the degenerate settings at the
    row's own width (AIM_GROUP_G)."""
    req, pat, txt = row_batch(key, pad)
    out = {}
    res, ops, out["line"], out["todo"] = _align(row_params(key), req, pat, txt)
    out["res"] = res
    if ops is not None:
        out["ops"] = ops
    if key[0] in VARIANTS:
        with _env(AIM_FORCE_WAVE="1"):
            res, ops, out["wave_line"], _ = _align(row_params(key), req, pat, txt)
        out["wave_res"] = res
        if ops is not None:
            out["wave_ops"] = ops
        if pad == "zero":
            from aim_amd import engine
            rs, ms = TABLE[key][:2]
            for name, kw in degenerate_runs(key):      # (their rows and rings are smaller: held to the row's width)
                with _env(AIM_GROUP_G=str(key[1])):
                    res, ops, out[name + "_line"], _ = _align(engine.make_params("wfa", ms, rs, backtrace=key[2], **kw), req, pat, txt)
                out[name + "_res"] = res
                if ops is not None:
                    out[name + "_ops"] = ops
    return out


def plan_of(key, **over):
    return F.plan_line(row_params(key, **over), F.pairs_for(TABLE[key][0]))


# ------------------------------------------------------------------ making the table
def _plan_width(kind, rs, ms, pen, bt, red=False):
    from aim_amd import engine
    kw = dict(pen, backtrace=bt)
    if kind == "endsfree":
        kw["ends_free"] = ENDS_FREE
    elif kind == "affine2p":
        kw["gap2"] = GAP2
    elif kind == "linear":
        kw["linear"] = True
    else:
        kw.update(reduce=red, escalate=True)
    line = F.plan_line(engine.make_params("wfa", ms, rs, **kw), F.pairs_for(rs))
    key = (kind, 0, bt, red) if kind.startswith("escalate") else (kind, 0, bt)
    return line_width(key, line), line


LANE_READ_SIZES = range(72, 177, 8)      # the READ_SIZEs wfa_lane_kernel / wfa_lane_packed_kernel take (5 .. 11 dwords per packed row)
ESC_PEN = dict(mismatch=3, gap_o=4, gap_e=1)
ESC_PENS = (ESC_PEN, dict(mismatch=4, gap_o=6, gap_e=2), dict(mismatch=2, gap_o=3, gap_e=1), dict(mismatch=5, gap_o=4, gap_e=2))   # the lane kernels' penalty sets


def make_table():
    """The table by the module's rules, under the current planner. The caller has set PLAN_ENV."""
    table = {}
    for kind in VARIANTS:
        for G in WIDTHS:
            pen = pen_of(kind, G)
            for bt in (False, True):
                found = None
                for rate, top in ((0.02, 2048), (0.10, 4096)):
                    for rs in range(8, top + 1, 8):
                        ms = score_rule(kind, rs, rate, pen)
                        if _plan_width(kind, rs, ms, pen, bt)[0] == G:
                            found = (rs, ms, pen, {})
                            break
                    if found:
                        break
                if not found:
                    env = {"AIM_GROUP_G": str(G)}
                    F._with_env(env)
                    for rs in range(8, 4097, 8):
                        ms = score_rule(kind, rs, 0.02, pen)
                        if _plan_width(kind, rs, ms, pen, bt)[0] == G:
                            found = (rs, ms, pen, env)
                            break
                    F._without_env(env)
                if found:
                    table[(kind, G, bt)] = found
    for G in WIDTHS:
        for bt in (False, True):
            for red in (False, True):
                found = None
                for env in ({}, {"AIM_GROUP_G": str(G)}):
                    F._with_env(env)
                    for pen in ESC_PENS:
                        for rs in LANE_READ_SIZES:
                            for ms in ESC_SCORES:
                                if not found and _plan_width("escalate", rs, ms, pen, bt, red)[0] == G:
                                    found = (rs, ms, pen, env)
                    F._without_env(env)
                    if found:
                        break
                if found:
                    table[("escalate", G, bt, red)] = found
    for G, env in ((16, {"AIM_GROUP_WLDS": "96"}), (8, {"AIM_GROUP_WLDS": "96", "AIM_GROUP_G": "8"})):
        for bt in (False, True):
            F._with_env(env)
            found = None
            for rs in LANE_READ_SIZES:
                for ms in ESC_SCORES:
                    if not found and 2 * ms + 3 > 96 and _plan_width("escalate", rs, ms, ESC_PEN, bt, True)[0] == G:
                        found = (rs, ms, ESC_PEN, env)
            F._without_env(env)
            if found:
                table[("escalate_modrows", G, bt, True)] = found
    return table


if __name__ == "__main__":
    import ast
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import wfa_group_rows as W          # (one copy of the caches and tables, whatever this file was started as)
    if sys.argv[1] == "--make-table":
        F._with_env(PLAN_ENV)
        for k, v in W.make_table().items():
            print("    %r: %r," % (k, v))
    elif sys.argv[1] == "--plan":        # --plan ROW: the row's plan line under the environment as it is
        print(W.plan_of(ast.literal_eval(sys.argv[2])))
    elif sys.argv[1] == "--run":         # --run OUT.npz PAD ROW ...: run_row of every row under the environment as it is
        out = {}
        for i, key in enumerate(sys.argv[4:]):
            for name, v in W.run_row(ast.literal_eval(key), sys.argv[3]).items():
                out["%d/%s" % (i, name)] = v
        np.savez(sys.argv[2], **out)
