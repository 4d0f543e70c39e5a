"""Banded checker for WFA beyond READ_SIZE 32 760 (AIM_FLAG_WFA_W32): one Gotoh DP for the global gap-affine, dual-cost gap-affine
(affine2p), gap-linear and ends-free scores, vectorised over pairs and restricted to a band of diagonals. No GPU, no library:
plain numpy.

The full-width models (endsfree_model, affine2p_model, linear_model) keep a whole DP row of every pair; at l = 40 000 that is out of
reach. Here row i holds only the diagonals d = h - v of the band, so a pair costs O(plen * band) and l = 40 000 takes seconds.

The band. Every gap base costs at least emin (the smallest gap-extend cost; gap-linear: g), so an alignment of cost <= MAX_SCORE
holds at most B = MAX_SCORE // emin gap bases. Starting on diagonal 0 and ending on diagonal tlen - plen, it never leaves the
diagonals within B of both. With ends-free the start lies on [-PB, TB] and the end on [ak - TE, ak + PE] (ak = tlen - plen), so
the band widens by the free lengths. Every alignment of cost <= MAX_SCORE lies inside the band: below the cap the banded optimum is
the exact optimum. Above the cap it is the cost of the best alignment inside the band, which is >= the exact optimum > MAX_SCORE.

Costs: match 0, mismatch x; a maximal run of L insertions or of L deletions costs min over the gap pieces of o + L*e (one piece
(o, e) for gap-affine, two for affine2p, (0, g) for gap-linear)."""
import numpy as np

INF = 1 << 40


def band(plen, tlen, max_score, emin, ends_free=(0, 0, 0, 0)):
    """(lo, hi) diagonals of every pair's band, as int64 arrays (see the module docstring)."""
    plen = np.asarray(plen, dtype=np.int64)
    tlen = np.asarray(tlen, dtype=np.int64)
    PB, PE, TB, TE = (np.minimum(int(f), lens) for f, lens in zip(ends_free, (plen, plen, tlen, tlen)))
    B = int(max_score) // int(emin)
    ak = tlen - plen
    lo = np.maximum(np.maximum(-PB - B, ak - TE - B), -plen)
    hi = np.minimum(np.minimum(TB + B, ak + PE + B), tlen)
    return lo, hi


def dp_scores(req, pat, txt, max_score, x=3, o=4, e=1, gap2=None, linear=False, ends_free=(0, 0, 0, 0)):
    """Banded optimum of every pair: exact where it is <= max_score, > max_score elsewhere.

    gap2=(o2, e2): dual-cost gap-affine (a run costs min(o + L*e, o2 + L*e2)). linear=True: gap-linear, every gap base costs e (o is
    ignored). ends_free=(PB, PE, TB, TE): leading / trailing gaps inside the free lengths cost 0 (each clamped to the pair's length).

    Row i (pattern bases consumed), column c = d - lo of the pair's band (text position h = i + lo + c). Per gap piece: D (deletion,
    consumes pattern) comes from row i - 1 at column c + 1; M' = min(diagonal, every D); the insertion state of the whole row at
    once, I[c] = o + e*c + min_{c' < c} (M'[c'] - e*c') -- a run never needs to restart inside a run of its own kind (two adjacent
    runs never cost less than one), so M' is enough (as in affine2p_model)."""
    plen = np.asarray(req["pattern_len"], dtype=np.int64)
    tlen = np.asarray(req["text_len"], dtype=np.int64)
    n = len(plen)
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    pieces = [(0, e)] if linear else [(o, e)] + ([tuple(int(v) for v in gap2)] if gap2 is not None else [])
    emin = min(pe for _, pe in pieces)
    PB, PE, TB, TE = (np.minimum(int(f), lens) for f, lens in zip(ends_free, (plen, plen, tlen, tlen)))
    lo, hi = band(plen, tlen, max_score, emin, ends_free)
    W = max(int((hi - lo).max()) + 1, 1)
    H = int(plen.max())
    c = np.arange(W, dtype=np.int64)[None, :]
    rows = np.arange(n)[:, None]
    rs = txt.shape[1]
    in_band = c <= (hi - lo)[:, None]
    pat = np.asarray(pat)
    txt = np.asarray(txt)

    def columns(i):
        h = i + lo[:, None] + c                       # text position of every column
        ok = in_band & (h >= 0) & (h <= tlen[:, None])
        return h, ok

    def with_ins(mp, ok):
        mp = np.where(ok, mp, INF)
        out = mp
        for po, pe in pieces:
            pref = np.minimum.accumulate(mp - pe * c, axis=1)
            ins = np.full_like(mp, INF)
            ins[:, 1:] = po + pe * c[:, 1:] + pref[:, :-1]
            out = np.minimum(out, ins)
        return np.where(ok, np.minimum(out, INF), INF)

    best = np.full(n, INF, dtype=np.int64)
    ef = any(ends_free)

    def take_end(i, M, h):
        nonlocal best
        if not ef:
            at = i == plen
            if at.any():
                cc = np.clip(tlen - plen - lo, 0, W - 1)
                v = np.where((tlen - plen >= lo) & (tlen - plen <= hi), M[np.arange(n), cc], INF)
                best = np.where(at, v, best)
            return
        # right border (v >= plen - PE, tlen) in row i
        on = (i >= plen - PE) & (i <= plen)
        cc = tlen - i - lo
        inb = (cc >= 0) & (cc < W)
        v = np.where(inb, M[np.arange(n), np.clip(cc, 0, W - 1)], INF)
        best = np.where(on, np.minimum(best, v), best)
        # bottom border (plen, h >= tlen - TE)
        last = i == plen
        if last.any():
            masked = np.where((h >= (tlen - TE)[:, None]) & (h <= tlen[:, None]), M, INF)
            best = np.where(last, np.minimum(best, masked.min(axis=1)), best)

    h, ok = columns(0)
    start = np.where((h == 0) | (ef & (h >= 0) & (h <= TB[:, None])), 0, INF)
    M = with_ins(start, ok)
    Ds = [np.full((n, W), INF, dtype=np.int64) for _ in pieces]
    take_end(0, M, h)
    for i in range(1, H + 1):
        h, ok = columns(i)
        up = np.full((n, W), INF, dtype=np.int64)       # row i - 1 at column c + 1: the same text position
        up[:, :-1] = M[:, 1:]
        mp = np.full((n, W), INF, dtype=np.int64)
        for k, (po, pe) in enumerate(pieces):
            Dup = np.full((n, W), INF, dtype=np.int64)
            Dup[:, :-1] = Ds[k][:, 1:]
            Ds[k] = np.where(ok, np.minimum(np.minimum(up + po + pe, Dup + pe), INF), INF)
            mp = np.minimum(mp, Ds[k])
        pc = pat[:, min(i - 1, pat.shape[1] - 1)].astype(np.int64)[:, None]
        tc = txt[rows, np.clip(h - 1, 0, rs - 1)].astype(np.int64)
        diag = np.where(h >= 1, M + np.where(tc == pc, 0, x), INF)
        mp = np.minimum(mp, diag)
        if ef:
            mp = np.where((h == 0) & (i <= PB[:, None]), 0, mp)
        M = with_ins(mp, ok)
        take_end(i, M, h)
    return best
