"""Independent checkers for ends-free (semi-global) WFA (AIM_FLAG_ENDSFREE): a gap-affine DP model vectorised over pairs,
a memoised brute-force recursion for tiny pairs, and CIGAR checks. No GPU, no library: plain numpy / Python.

Costs are WFA's: match 0, mismatch x, a gap of length L costs o + L*e. Leading and trailing gaps inside the free lengths cost 0;
the alignment starts at (0, h <= TB) or (v <= PB, 0) and ends at (plen, h >= tlen - TE) or (v >= plen - PE, tlen). Each free
length is clamped to the pair's length."""
import functools

import numpy as np

INF = 1 << 28


def dp_scores(req, pat, txt, x=3, o=4, e=1, ends_free=(0, 0, 0, 0)):
    """Ends-free gap-affine optimum of every pair (Gotoh, one DP row per step for all pairs at once).

    Row i: F (deletion, consumes pattern) from row i-1; M' = min(diagonal, F); then the insertion state of the whole row at
    once, E[j] = o + e*j + min_{k<j} (M'[k] - e*k) -- an insertion run never starts from an insertion, so M' is enough."""
    plen = np.asarray(req["pattern_len"], dtype=np.int64)
    tlen = np.asarray(req["text_len"], dtype=np.int64)
    n = len(plen)
    PB, PE, TB, TE = (np.minimum(int(f), lens) for f, lens in zip(ends_free, (plen, plen, tlen, tlen)))
    W = int(tlen.max()) + 1 if n else 1
    H = int(plen.max()) if n else 0
    j = np.arange(W, dtype=np.int64)[None, :]
    ej = e * j

    def with_ins(mp):
        pm = mp - ej
        pref = np.minimum.accumulate(pm, axis=1)
        E = np.full_like(mp, INF)
        E[:, 1:] = o + ej[:, 1:] + pref[:, :-1]
        return np.minimum(mp, np.minimum(E, INF))

    M = with_ins(np.where(j <= TB[:, None], 0, INF))
    F = np.full((n, W), INF, dtype=np.int64)
    best = np.full(n, INF, dtype=np.int64)
    txt_i = np.asarray(txt[:, :W - 1], dtype=np.int64)

    def take_end(i, M):
        nonlocal best
        # right border (v >= plen - PE, tlen) in row i
        on = (i >= plen - PE) & (i <= plen)
        v = M[np.arange(n), tlen]
        best = np.where(on, np.minimum(best, v), best)
        # bottom border (plen, h >= tlen - TE)
        last = i == plen
        if last.any():
            masked = np.where(j >= (tlen - TE)[:, None], M, INF)
            masked = np.where(j <= tlen[:, None], masked, INF)
            best = np.where(last, np.minimum(best, masked.min(axis=1)), best)

    take_end(0, M)
    for i in range(1, H + 1):
        F = np.minimum(M + o + e, F + e)
        diag = np.full((n, W), INF, dtype=np.int64)
        if W > 1:
            pc = np.asarray(pat[:, i - 1], dtype=np.int64)[:, None]
            diag[:, 1:] = M[:, :-1] + np.where(txt_i == pc, 0, x)
        mp = np.minimum(diag, F)
        mp[:, 0] = np.where(i <= PB, 0, mp[:, 0])
        M = np.minimum(with_ins(np.minimum(mp, INF)), INF)
        F = np.minimum(F, INF)
        take_end(i, M)
    return best


def brute_score(p, t, x=3, o=4, e=1, ends_free=(0, 0, 0, 0)):
    """Minimum over every alignment of the whole of p against the whole of t, straight from the definition (tiny inputs)."""
    P, T = len(p), len(t)
    PB, PE, TB, TE = min(ends_free[0], P), min(ends_free[1], P), min(ends_free[2], T), min(ends_free[3], T)

    @functools.lru_cache(maxsize=None)
    def go(i, j, st):   # st: 0 after a match / mismatch (or at the start), 1 inside an insertion run, 2 inside a deletion run
        best = INF
        if (i == P and j >= T - TE) or (j == T and i >= P - PE):
            best = 0
        if i < P and j < T:
            best = min(best, (0 if p[i] == t[j] else x) + go(i + 1, j + 1, 0))
        if j < T:
            best = min(best, (e if st == 1 else o + e) + go(i, j + 1, 1))
        if i < P:
            best = min(best, (e if st == 2 else o + e) + go(i + 1, j, 2))
        return best

    starts = [(0, h) for h in range(TB + 1)] + [(v, 0) for v in range(1, PB + 1)]
    return min(go(v, h, 0) for v, h in starts)


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


def rescore(ops, plen, tlen, x=3, o=4, e=1, ends_free=(0, 0, 0, 0)):
    """Cost of an op string with its leading and trailing gap runs free up to the free lengths."""
    PB, PE, TB, TE = min(ends_free[0], plen), min(ends_free[1], plen), min(ends_free[2], tlen), min(ends_free[3], tlen)
    runs = [list(r) for r in runs_of(ops)]
    if runs and runs[0][0] in "ID":
        runs[0][1] -= min(runs[0][1], TB if runs[0][0] == "I" else PB)
    if runs and runs[-1][0] in "ID":
        runs[-1][1] -= min(runs[-1][1], TE if runs[-1][0] == "I" else PE)
    cost = 0
    for c, k in runs:
        if k == 0 or c == "M":
            continue
        cost += x * k if c == "X" else o + e * k
    return cost
