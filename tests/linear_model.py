"""Independent checkers for gap-linear WFA (AIM_FLAG_LINEAR): a DP vectorised over pairs, a memoised brute-force recursion for tiny
pairs, and a CIGAR checker. No GPU, no library: plain numpy / Python.

Costs: match 0, mismatch x, every inserted or deleted base g. The score is the minimum cost of a global alignment; x = g = 1 is the
edit distance."""
import functools

import numpy as np

INF = 1 << 40


def dp_scores(req, pat, txt, x=1, g=1):
    """Gap-linear optimum of every pair (one DP row per pattern base for all pairs at once).

    Row i: C[j] = min(H[i-1][j] + g, H[i-1][j-1] + (x if p[i-1] != t[j-1] else 0)); then the insertions of the whole row at once,
    H[i][j] = min_{k <= j} (C[k] + g*(j-k)) = g*j + prefix-min(C[k] - g*k)."""
    plen = np.asarray(req["pattern_len"], dtype=np.int64)
    tlen = np.asarray(req["text_len"], dtype=np.int64)
    n = len(plen)
    out = np.zeros(n, dtype=np.int64)
    if n == 0:
        return out
    W = int(tlen.max()) + 1
    j = np.arange(W, dtype=np.int64)[None, :]
    T = np.asarray(txt, dtype=np.uint8)[:, :W - 1]
    if T.shape[1] < W - 1:
        T = np.pad(T, ((0, 0), (0, W - 1 - T.shape[1])))
    P = np.asarray(pat, dtype=np.uint8)
    rows = np.arange(n)
    h = np.broadcast_to(g * j, (n, W)).copy()   # row 0: j insertions
    done = plen == 0
    out[done] = h[rows[done], tlen[done]]
    for i in range(1, int(plen.max()) + 1):
        c = h + g
        c[:, 1:] = np.minimum(c[:, 1:], h[:, :-1] + x * (P[:, i - 1:i] != T))
        h = g * j + np.minimum.accumulate(c - g * j, axis=1)
        at = plen == i
        out[at] = h[rows[at], tlen[at]]
    return out


def brute_score(p, t, x=1, g=1):
    """The same optimum by plain recursion over (i, j) (tiny pairs only)."""
    @functools.lru_cache(maxsize=None)
    def go(i, j):
        if i == len(p):
            return (len(t) - j) * g
        if j == len(t):
            return (len(p) - i) * g
        return min(go(i + 1, j + 1) + (0 if p[i] == t[j] else x), go(i + 1, j) + g, go(i, j + 1) + g)
    return go(0, 0)


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


def rescore(ops, x=1, g=1):
    """Gap-linear cost of a CIGAR string."""
    return ops.count("X") * x + (ops.count("I") + ops.count("D")) * g


def max_score_rule(length, error, x, g):
    """MAX_SCORE for generated pairs: ceil(l*e) edits, each costing at most max(min(x, 2g), g)."""
    edits = int(np.ceil(length * error - 1e-9))
    return edits * max(min(x, 2 * g), g)
