"""Low-complexity inputs for the alignment kernels: homopolymers, dinucleotide and tandem repeats, two-letter sequence and runs of
'N', in the wire layout and on the kernel-shape table of tests/full_rows.py. Plain numpy; no device.

engine.gen_pairs and full_rows.full_row_batch draw uniform random A/C/G/T, where an optimal path is nearly unique and only the
alignment's own diagonal matches for long. In a repeat an indel can sit anywhere inside a run at equal cost, so the traceback's
choice among diagonal, insertion and deletion decides the CIGAR, and every diagonal inside the band extends to the end of the row.

Every class has a LIGHT form (the class's pattern; the text differs by one substitution, one 1-base deletion, one 1-base insertion
or nothing: 0, 3 or 5 at mismatch 3 / gap 4 + 1) and a HEAVY form (the table in CLASSES_DOC). Pairs come in rounds of nine, one of
each class; every fourth round fills READ_SIZE, the others use l = (READ_SIZE - 8) * 100 // 104 like the body of a full-row batch."""
import numpy as np

import full_rows as F

CLASSES = ("homo_len", "homo_foreign", "dinuc", "tandem_copy", "tandem_rot", "tandem_sub", "homo_island", "two_letter", "n_run")
CLASSES_DOC = {
    "homo_len": "one base repeated; the text is 0..3 bases shorter or longer",
    "homo_foreign": "one base repeated, with one foreign base at independent places in pattern and text",
    "dinuc": "a 2-base unit; 1..3 bases inserted or deleted",
    "tandem_copy": "a random unit of 3/5/7/13/17/31/33 bases in tandem; one whole copy more or less",
    "tandem_rot": "the same pattern rotated by 1..3 bases",
    "tandem_sub": "a unit of 3/4/6/11/16/32 bases; 1 % substitutions, at least one",
    "homo_island": "random sequence with a run of 12..40 equal bases whose length changes by 1..3, plus 1 % substitutions",
    "two_letter": "85 % A / 15 % T; 1 % substitutions and one indel",
    "n_run": "random sequence with a run of 4..19 'N'; one 'N' more or less",
}
LIGHT_KINDS = ("sub", "del", "ins", "sub", "del", "ins", "sub", "none")      # of pair (round r, class c): entry (r + c) % 8 ...
LIGHT_PLACES = ("any", "first", "last")                                       # ... at place (r + 2 * c) % 3: the edges of a row get edits too
SEED = 20262
N, A, T = ord("N"), ord("A"), ord("T")


def _other(rng, b, alphabet=F.ACGT):
    """A base of the alphabet that is not b."""
    rest = alphabet[alphabet != b]
    return rest[rng.integers(0, len(rest))]


def _tandem(unit, length):
    return np.tile(unit, length // len(unit) + 1)[:length].copy()


def _unit(rng, k):
    """k random bases, at least two of them different (k >= 2)."""
    while True:
        u = F.ACGT[rng.integers(0, 4, size=k)]
        if k < 2 or (u != u[0]).any():
            return u


def _subs(rng, s, k, alphabet=F.ACGT):
    s = s.copy()
    if len(s) and k > 0:
        for at in rng.choice(len(s), size=min(k, len(s)), replace=False):
            s[at] = _other(rng, s[at], alphabet)
    return s


def _run_len(rng, lo, hi, L):
    """A run length drawn from lo..hi, never above L // 2 (and at least 1)."""
    return max(1, min(int(rng.integers(lo, hi + 1)), L // 2))


def _with_run(rng, L, run, base):
    """(random sequence of L bases with `run` copies of `base` inside it, the run's first position)."""
    s = F.ACGT[rng.integers(0, 4, size=L)]
    at = int(rng.integers(0, L - run + 1))
    s[at:at + run] = base
    return s, at


UNIT_SIZES = {"tandem_copy": (3, 5, 7, 13, 17, 31, 33), "tandem_rot": (3, 5, 7, 13, 17, 31, 33), "tandem_sub": (3, 4, 6, 11, 16, 32)}


def _unit_len(rng, cls, L):
    """A unit length of the class, never above L // 3 (and at least 1)."""
    sizes = UNIT_SIZES[cls]
    return max(1, min(int(sizes[rng.integers(0, len(sizes))]), L // 3))


def _base_pattern(rng, cls, L):
    """The class's own pattern of L bases (what the light form aligns), and the alphabet its substitutions draw from."""
    if cls in ("homo_len", "homo_foreign"):
        return np.full(L, F.ACGT[rng.integers(0, 4)], dtype=np.uint8), F.ACGT
    if cls == "dinuc":
        return _tandem(_unit(rng, 2), L), F.ACGT
    if cls in ("tandem_copy", "tandem_rot", "tandem_sub"):
        return _tandem(_unit(rng, _unit_len(rng, cls, L)), L), F.ACGT
    if cls == "homo_island":
        return _with_run(rng, L, _run_len(rng, 12, 40, L), F.ACGT[rng.integers(0, 4)])[0], F.ACGT
    if cls == "two_letter":
        return np.where(rng.random(L) < 0.85, A, T).astype(np.uint8), np.array([A, T], dtype=np.uint8)
    if cls == "n_run":
        return _with_run(rng, L, _run_len(rng, 4, 19, L), N)[0], F.ACGT
    raise ValueError(cls)


def _place(rng, place, n):
    """An index into n positions: 'first', 'last' or anywhere."""
    return 0 if place == "first" else (n - 1 if place == "last" else int(rng.integers(0, n)))


def _light(rng, cls, L, kind, place):
    """max(plen, tlen) == L; the text is the pattern after one edit of `kind` at `place`."""
    if kind == "ins" and L > 1:
        p, alphabet = _base_pattern(rng, cls, L - 1)
        return p, np.insert(p, _place(rng, place, L), alphabet[rng.integers(0, len(alphabet))])
    p, alphabet = _base_pattern(rng, cls, L)
    if kind == "sub":
        t = p.copy()
        at = _place(rng, place, L)
        t[at] = _other(rng, t[at], F.ACGT if cls in ("homo_len", "homo_foreign", "n_run") else alphabet)
        return p, t
    if kind == "del" and L > 1:
        return p, np.delete(p, _place(rng, place, L))
    return p, p.copy()


def _longer_shorter(rng, longer, shorter):
    """The text is the longer or the shorter one with equal probability."""
    return (shorter, longer) if rng.integers(0, 2) else (longer, shorter)


def _heavy(rng, cls, L):
    """max(plen, tlen) == L; CLASSES_DOC[cls]."""
    if cls == "homo_len":
        p, _ = _base_pattern(rng, cls, L)
        return _longer_shorter(rng, p, p[:max(1, L - int(rng.integers(0, 4)))].copy())
    if cls == "homo_foreign":
        p, _ = _base_pattern(rng, cls, L)
        return _subs(rng, p, 1), _subs(rng, p, 1)
    if cls == "dinuc":
        p, _ = _base_pattern(rng, cls, L)
        k = min(int(rng.integers(1, 4)), L - 1)
        at = int(rng.integers(0, L - k + 1))
        return _longer_shorter(rng, p, np.delete(p, slice(at, at + k)))
    if cls == "tandem_copy":
        k = _unit_len(rng, cls, L)           # (drawn here, not in _base_pattern: the copy that goes is one unit long)
        p = _tandem(_unit(rng, k), L)
        return _longer_shorter(rng, p, p[:max(1, L - k)].copy())
    if cls == "tandem_rot":
        p, _ = _base_pattern(rng, cls, L)
        return p, np.roll(p, -int(rng.integers(1, 4)))
    if cls == "tandem_sub":
        p, _ = _base_pattern(rng, cls, L)
        return p, _subs(rng, p, max(1, L // 100))
    if cls in ("homo_island", "n_run"):
        island = cls == "homo_island"
        run = _run_len(rng, 12, 40, L) if island else _run_len(rng, 4, 19, L)
        k = min(int(rng.integers(1, 4)) if island else 1, max(run - 1, 0))
        longer, at = _with_run(rng, L, run, F.ACGT[rng.integers(0, 4)] if island else N)
        shorter = np.delete(longer, slice(at, at + k))
        p, t = _longer_shorter(rng, longer, shorter)
        if island and L // 100:
            t = _subs(rng, t, L // 100)
        return p, t
    if cls == "two_letter":
        p, alphabet = _base_pattern(rng, cls, L)
        shorter = np.delete(p, int(rng.integers(0, L))) if L > 1 else p.copy()
        p, t = _longer_shorter(rng, p, shorter)
        return p, _subs(rng, t, L // 100, alphabet)
    raise ValueError(cls)


def round_is_full(r):
    return r % 4 == 3


def round_is_light(r, max_score):
    """Three rounds of every four where max_score <= 10, two of four otherwise; the phase moves by one every four rounds, so the
    rounds that fill READ_SIZE come in both forms."""
    return (r + r // 4) % 4 != 3 if max_score <= 10 else (r + r // 4) % 4 in (0, 2)


def low_complexity_batch(rs, n, seed, max_score, pad="zero"):
    """(requests, patterns[n][rs], texts[n][rs], cls, light): pair i has class CLASSES[i % 9] (cls[i] is its index) and the light
    form where light[i]. Every pair is drawn from a generator of its own seeded by (seed, rs, i), so a pair's bytes depend on
    max_score through its form only. pad as in full_rows.full_row_batch."""
    from aim_amd import capi
    if pad not in ("zero", "noise"):
        raise ValueError("pad is 'zero' or 'noise'")
    req = np.zeros(n, dtype=capi.REQUEST_DTYPE)
    pat = np.zeros((n, rs), dtype=np.uint8)
    txt = np.zeros((n, rs), dtype=np.uint8)
    cls = np.arange(n) % len(CLASSES)
    light = np.zeros(n, dtype=bool)
    l = max(1, (rs - 8) * 100 // 104)
    for i in range(n):
        r = i // len(CLASSES)
        light[i] = round_is_light(r, max_score)
        rng = np.random.default_rng([int(seed), int(rs), i, int(light[i]), 0x6C6F7763])
        L = rs if round_is_full(r) else l
        if light[i]:
            c = int(cls[i])
            p, t = _light(rng, CLASSES[c], L, LIGHT_KINDS[(r + c) % len(LIGHT_KINDS)], LIGHT_PLACES[(r + 2 * c) % len(LIGHT_PLACES)])
        else:
            p, t = _heavy(rng, CLASSES[cls[i]], L)
        assert max(len(p), len(t)) == L, (CLASSES[cls[i]], len(p), len(t), L)
        pat[i, :len(p)], txt[i, :len(t)] = p, t
        req["pattern_len"][i], req["text_len"][i] = len(p), len(t)
    req["idx"] = 7000 + np.arange(n, dtype=np.uint32)
    if pad == "noise":
        nrng = np.random.default_rng([int(seed), int(rs), 0x6E6F6973])
        col = np.arange(rs)[None, :]
        for rows, key in ((pat, "pattern_len"), (txt, "text_len")):
            noise = F.ACGTN[nrng.integers(0, 5, size=rows.shape)]
            behind = col >= req[key].astype(np.int64)[:, None]
            rows[behind] = noise[behind]
    return req, pat, txt, cls, light


def one_of_each(rs, seed, max_score=1 << 20, pad="zero"):
    """18 pairs: the light and the heavy form of every class, the second nine filling READ_SIZE. (Rounds 0 and 3 of a batch at
    a large max_score are light / heavy.)"""
    req, pat, txt, cls, light = low_complexity_batch(rs, 4 * len(CLASSES), seed, max_score, pad)
    sel = np.r_[0:9, 27:36]
    assert light[:9].all() and not light[27:36].any()
    return req[sel].copy(), np.ascontiguousarray(pat[sel]), np.ascontiguousarray(txt[sel]), cls[sel], light[sel]


# ------------------------------------------------------------------ the table: full_rows' rows plus the dynamic-bounds lane shape
# MAX_SCORE 10 with the reduction: a 2-base gap (6), two mismatches (6) and mismatch + gap (8) fit the cap, and the lane kernels
# run with per-score bounds instead of the static ones of MAX_SCORE <= 5. Kept here so full_rows.TABLE and its measured to-do
# counts stay what they are. tests/test_low_complexity_cpu.py checks the tokens against the planner.
FAMILIES = dict(F.FAMILIES,
                wfa10=F._fam("wfa", lambda rs: 10, reduce=True),
                wfa10_bt=F._fam("wfa", lambda rs: 10, reduce=True, backtrace=True),
                # other costs on the run-list path (no table row: the planner picks the kernel, wfa_group at READ_SIZE 112)
                wfa18_254_bt=F._fam("wfa", lambda rs: 18, reduce=True, backtrace=True, mismatch=2, gap_o=5, gap_e=4))
_PK = "wfa_lane_packed_kernel pack_first=1"
TABLE = dict(F.TABLE, wfa10=[(80, "wfa_lane_kernel"), (112, "wfa_lane_kernel"), (136, _PK), (176, _PK)],
             wfa10_bt=[(80, _PK), (112, _PK), (136, _PK), (176, _PK)])      # (with CIGAR every READ_SIZE plans on the packed kernel)
WFA10_ROWS = [(fam, rs) for fam in ("wfa10", "wfa10_bt") for rs, _ in TABLE[fam]]
ROWS = F.ROWS + WFA10_ROWS


def expected_plan(fam, rs):
    return dict(TABLE[fam])[rs]


def row_params(fam, rs):
    from aim_amd import engine
    if fam in F.FAMILIES:
        return F.row_params(fam, rs)
    f = FAMILIES[fam]
    return engine.make_params(f["algo"], f["ms"](rs), rs, **f["kw"])


def row_batch(fam, rs, pad="zero"):
    return low_complexity_batch(rs, F.pairs_for(rs), SEED, FAMILIES[fam]["ms"](rs), pad)


_ORACLE = {}


def oracle_of(params, algo, req, pat, txt):
    from oracle import oracle
    return oracle.align_batch(F.oracle_params(params, algo), req["pattern_len"], req["text_len"], pat, txt, nthreads=8)


def oracle_row(fam, rs, pad="zero"):
    """(results, ops) of the oracle on a row's low-complexity batch; computed once per session and never changed afterwards.
    Rows that differ only in a knob share one run."""
    f = FAMILIES[fam]
    key = (f["algo"], f["ms"](rs), tuple(sorted(f["kw"].items())), rs, pad)
    if key not in _ORACLE:
        req, pat, txt, _, _ = row_batch(fam, rs, pad)
        res, ops, _ = oracle_of(row_params(fam, rs), f["algo"], req, pat, txt)
        res.flags.writeable = False
        if ops is not None:
            ops.flags.writeable = False
        _ORACLE[key] = (res, ops)
    return _ORACLE[key]


def plan_lines():
    """{"family/READ_SIZE": aim_plan_describe's line} of the wfa10 rows."""
    return {"%s/%d" % (fam, rs): F.plan_line(row_params(fam, rs), F.pairs_for(rs)) for fam, rs in WFA10_ROWS}


def align_row(fam, rs, pad="zero", batch=None):
    """(results, ops, plan line, fallback pairs) of a row's low-complexity batch on the device, under the row's own knobs."""
    from aim_amd import engine
    req, pat, txt = (batch or row_batch(fam, rs, pad))[:3]
    params = row_params(fam, rs)
    env = FAMILIES[fam]["env"]
    F._with_env(env)
    try:
        with engine.DeviceSet(1) as s:
            s.configure(params, len(req))
            s.push(0, req, pat, txt)
            s.launch()
            res, ops = s.pull(0, check=False)
            return res, ops, s.plan_describe(0), s.fallback_pairs(0)
    finally:
        F._without_env(env)


# ------------------------------------------------------------------ NW traceback with the tie order as a parameter
ORDERS = ("DIM", "DMI", "IDM", "IMD", "MDI", "MID")      # 'D' deletion (v - 1), 'I' insertion (h - 1), 'M' the diagonal
ORACLE_ORDER = "DIM"                                        # aim_oracle.c nw_pair: deletion, then insertion, else the diagonal


def nw_table(p, t, x=3, gi=4, gd=4):
    """dp[h][v]: the plain NW table, text along h, pattern along v."""
    dp = np.zeros((len(t) + 1, len(p) + 1), dtype=np.int64)
    v = np.arange(len(p) + 1, dtype=np.int64)
    dp[0] = v * gd
    pp = np.asarray(p, dtype=np.int64)
    for h in range(1, len(t) + 1):
        best = np.empty(len(p) + 1, dtype=np.int64)
        best[0] = h * gi
        best[1:] = np.minimum(dp[h - 1, :-1] + np.where(pp == t[h - 1], 0, x), dp[h - 1, 1:] + gi)
        dp[h] = np.minimum.accumulate(best - v * gd) + v * gd
    return dp


def nw_traceback(p, t, order, x=3, gi=4, gd=4, dp=None):
    """The ops (bytes, first operation first) of the walk from (tlen, plen) that takes the first move of `order` whose
    predecessor explains the cell; rows and columns 0 are all insertions / deletions."""
    dp = nw_table(p, t, x, gi, gd) if dp is None else dp
    h, v = len(t), len(p)
    out = bytearray()
    while h > 0 and v > 0:
        sub = 0 if p[v - 1] == t[h - 1] else x
        for mv in order:
            if mv == "D" and dp[h, v] == dp[h, v - 1] + gd:
                out.append(ord("D"))
                v -= 1
                break
            if mv == "I" and dp[h, v] == dp[h - 1, v] + gi:
                out.append(ord("I"))
                h -= 1
                break
            if mv == "M" and dp[h, v] == dp[h - 1, v - 1] + sub:
                out.append(ord("X") if sub else ord("M"))
                h -= 1
                v -= 1
                break
        else:
            raise AssertionError("no move explains cell (%d, %d)" % (h, v))
    out += b"I" * h + b"D" * v
    return bytes(out[::-1])


if __name__ == "__main__":
    import json
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if sys.argv[1] == "--plans":
        json.dump(plan_lines(), sys.stdout)
