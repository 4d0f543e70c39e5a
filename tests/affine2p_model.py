"""Independent checkers for dual-cost gap-affine WFA (AIM_FLAG_AFFINE2P): a five-state Gotoh DP vectorised over pairs, a
memoised brute-force recursion for tiny pairs, and a CIGAR cost function. No GPU, no library: plain numpy / Python.

Costs: match 0, mismatch x, a maximal run of L insertions or of L deletions costs min(o1 + L*e1, o2 + L*e2). The score is the
minimum cost of a global alignment."""
import functools

import numpy as np

INF = 1 << 28


def gap_cost(L, o1, e1, o2, e2):
    return min(o1 + L * e1, o2 + L * e2)


def dp_scores(req, pat, txt, x=3, o1=4, e1=1, o2=24, e2=1):
    """Dual-affine optimum of every pair (one DP row per pattern base for all pairs at once).

    Row i: D1 / D2 (deletion, consumes pattern) from row i-1; M' = min(diagonal, D1, D2); then both insertion states of the whole
    row at once, I[j] = o + e*j + min_{k<j} (M'[k] - e*k) per piece -- a run never needs to restart inside a run of its own kind
    (two adjacent runs never cost less than one), so M' is enough."""
    plen = np.asarray(req["pattern_len"], dtype=np.int64)
    tlen = np.asarray(req["text_len"], dtype=np.int64)
    n = len(plen)
    W = int(tlen.max()) + 1 if n else 1
    H = int(plen.max()) if n else 0
    j = np.arange(W, dtype=np.int64)[None, :]

    def with_ins(mp):
        out = mp
        for o, e in ((o1, e1), (o2, e2)):
            pm = mp - e * j
            pref = np.minimum.accumulate(pm, axis=1)
            ins = np.full_like(mp, INF)
            ins[:, 1:] = o + e * j[:, 1:] + pref[:, :-1]
            out = np.minimum(out, ins)
        return np.minimum(out, INF)

    first = np.full((n, W), INF, dtype=np.int64)
    first[:, 0] = 0
    M = with_ins(first)
    D1 = np.full((n, W), INF, dtype=np.int64)
    D2 = np.full((n, W), INF, dtype=np.int64)
    best = np.where(plen == 0, M[np.arange(n), tlen], INF)
    txt_i = np.asarray(txt[:, :W - 1], dtype=np.int64)
    for i in range(1, H + 1):
        D1 = np.minimum(np.minimum(M + o1 + e1, D1 + e1), INF)
        D2 = np.minimum(np.minimum(M + o2 + e2, D2 + e2), INF)
        diag = np.full((n, W), INF, dtype=np.int64)
        if W > 1:
            pc = np.asarray(pat[:, i - 1], dtype=np.int64)[:, None]
            diag[:, 1:] = M[:, :-1] + np.where(txt_i == pc, 0, x)
        M = with_ins(np.minimum(np.minimum(diag, D1), D2))
        best = np.where(plen == i, M[np.arange(n), tlen], best)
    return best


def brute_score(p, t, x=3, o1=4, e1=1, o2=24, e2=1):
    """Minimum over every alignment, straight from the definition: a sequence of match / mismatch steps and maximal gap runs,
    each run charged min(o1 + L*e1, o2 + L*e2) (tiny inputs)."""
    P, T = len(p), len(t)

    @functools.lru_cache(maxsize=None)
    def go(i, j, last):   # last: 0 after a match / mismatch (or at the start), 1 after an insertion run, 2 after a deletion run
        if i == P and j == T:
            return 0
        best = INF
        if i < P and j < T:
            best = min(best, (0 if p[i] == t[j] else x) + go(i + 1, j + 1, 0))
        if last != 1:
            for L in range(1, T - j + 1):
                best = min(best, gap_cost(L, o1, e1, o2, e2) + go(i, j + L, 1))
        if last != 2:
            for L in range(1, P - i + 1):
                best = min(best, gap_cost(L, o1, e1, o2, e2) + go(i + L, j, 2))
        return best

    return go(0, 0, 0)


def single_affine_scores(req, pat, txt, x=3, o=4, e=1):
    """Piece 1 alone (global WFA's cost): the dual model with a piece 2 that never pays off."""
    return dp_scores(req, pat, txt, x, o, e, o, e)


def runs_of(cigar):
    """[(op, length)] of an op string."""
    out = []
    for c in cigar:
        if out and out[-1][0] == c:
            out[-1][1] += 1
        else:
            out.append([c, 1])
    return [(c, k) for c, k in out]


def check_cigar(ops, p, t):
    """The ops use up exactly len(p) and len(t), 'M' only on equal bases, 'X' only on different ones. Returns an error or None."""
    v = h = 0
    for c in ops:
        if c in "MX":
            if v >= len(p) or h >= len(t):
                return "M/X past an end at (%d, %d)" % (v, h)
            if (c == "M") != (p[v] == t[h]):
                return "%s on %s/%s at (%d, %d)" % (c, chr(p[v]), chr(t[h]), v, h)
            v += 1
            h += 1
        elif c == "I":
            h += 1
        elif c == "D":
            v += 1
        else:
            return "op %r" % c
    if (v, h) != (len(p), len(t)):
        return "uses (%d, %d) of (%d, %d)" % (v, h, len(p), len(t))
    return None


def rescore(ops, x=3, o1=4, e1=1, o2=24, e2=1):
    """Dual-affine cost of an op string: every maximal 'I' or 'D' run charged min(o1 + L*e1, o2 + L*e2)."""
    cost = 0
    for c, k in runs_of(ops):
        if c == "X":
            cost += x * k
        elif c in "ID":
            cost += gap_cost(k, o1, e1, o2, e2)
    return cost
