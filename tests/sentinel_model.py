"""A second, independent statement of the reference's WFA recurrence with its -10: plain Python, score only, written from the
rule as WFA/DPU-*/dpu/wfa.c states it and not from oracle/aim_oracle.c. No GPU, no library.

The rule (affine_wfa_compute_next / affine_wfa_compute_offsets). The wavefront of score s reads three sources: M of s - x (sub),
M of s - (o + e) (gap open) and I / D of s - e (gap extend). A source is ABSENT when its score is negative, when no wavefront
exists at that score, or (I / D) when that wavefront was made without gap components. When all are absent there is no wavefront at
s. Otherwise the wavefront spans [min lo - 1, max hi + 1] over the sources present (an absent one counts as lo = 1, hi = -1), and
on every diagonal k of it

    ins = -10 when gap open and I are both absent; else both fetched at k - 1: NULL when both fetches are NULL, max + 1 otherwise
    del = -10 when gap open and D are both absent; else the maximum of both fetched at k + 1
    sub = -10 when sub is absent; else M[s - x][k] + 1
    M   = max(sub, ins, del)

where a fetch from an absent source, or from a present one outside its [lo, hi], gives NULL (INT16_MIN / 2). So a cell that no
present source covers holds -10, not NULL, and ten mismatch steps later (sub adds 1 per step) it holds 0: a real offset that
nothing paid a gap for. Extension (affine_wfa_extend) happens only from offsets >= 0 with v = offset - k >= 0; the loop ends
when M[tlen - plen] >= tlen, and a score over MAX_SCORE reports MAX_SCORE + 1. REDUCE is not modelled.

On the penalty sets where (10 + k) * x >= o + k * e for every gap length k that occurs, the -10 can never win and the score is
the gap-affine optimum; visible() names the others."""

NULL = -(1 << 15) // 2
ABSENT = -10


def can_be_visible(x, o, e):
    """The necessary condition, whatever the gap lengths: (10 + k) * x < o + k * e for some k >= 1, which is o + e > 11 * x or
    e > x. Where it is false no input shows the -10 (over x 1 .. 6, o 1 .. 70, e 1 .. 6 the oracle then equals the gap-affine
    optimum on every single-gap pair)."""
    return o + e > 11 * x or e > x


def gap_components(x, o, e, top):
    """has[s]: the wavefront of score s exists and has I / D components (a gap opened at s - (o + e), or one extended from
    s - e), for s = 0 .. top. A function of the penalties alone."""
    exists, has = [False] * (top + 1), [False] * (top + 1)
    exists[0] = True
    for s in range(1, top + 1):
        has[s] = (s >= o + e and exists[s - o - e]) or (s >= e and has[s - e])
        exists[s] = has[s] or (s >= x and exists[s - x])
    return has


def visible(x, o, e, kmax, gaps=None):
    """True when the -10 changes the score of a pair with one leading gap of k bases, for some 1 <= k <= kmax (or some k in
    `gaps`). The inequality (10 + k) * x < o + k * e alone is necessary and not sufficient: the -10 cell must also be born. The
    edge diagonal +-j first exists at score j * x, and holds -10 there only when that wavefront has no I / D components
    (gap_components); otherwise its gap fetches are out of range and the cell is NULL. A -10 born on diagonal j is a real offset
    at (10 + j) * x on its own diagonal, and on a diagonal k > j after a gap of k - j bases opened from it, at
    (10 + j) * x + o + (k - j) * e; the true gap costs o + k * e. (Checked against the oracle over x 1 .. 6, o 1 .. 70,
    e 1 .. 6 by tests/test_penalty_rows_cpu.py: exact on all 2 520 sets; the inequality alone is wrong on 59, all with e > x
    and o + e <= 11 * x.)"""
    ks = list(gaps) if gaps is not None else list(range(1, kmax + 1))
    has = gap_components(x, o, e, max(ks) * x)
    for k in ks:
        for j in range(1, k + 1):
            if not has[j * x] and (10 + j) * x + (0 if j == k else o + (k - j) * e) < o + k * e:
                return True
    return False


class _WF:
    __slots__ = ("lo", "hi", "M", "I", "D")

    def __init__(self, lo, hi, has_i, has_d):
        self.lo, self.hi = lo, hi
        self.M = {}
        self.I = {} if has_i else None
        self.D = {} if has_d else None


def _fetch(rows, lo, hi, k, out_of_range):
    """AFFINE_WAVEFRONT_COND_FETCH: rows is None for an absent source."""
    if rows is None:
        return NULL
    return rows[k] if lo <= k <= hi else out_of_range


def _next(wfs, s, x, o, e, absent, out_of_range):
    def at(score):
        return wfs.get(score) if score >= 0 else None
    m_sub, m_o, w_e = at(s - x), at(s - o - e), at(s - e)
    sub_rows = m_sub.M if m_sub is not None else None
    o_rows = m_o.M if m_o is not None else None
    i_rows = w_e.I if w_e is not None else None
    d_rows = w_e.D if w_e is not None else None
    has_i = o_rows is not None or i_rows is not None
    has_d = o_rows is not None or d_rows is not None
    if sub_rows is None and not has_i and not has_d:
        return None
    sub_lo, sub_hi = (m_sub.lo, m_sub.hi) if sub_rows is not None else (1, -1)
    o_lo, o_hi = (m_o.lo, m_o.hi) if o_rows is not None else (1, -1)
    e_lo, e_hi = (w_e.lo, w_e.hi) if (i_rows is not None or d_rows is not None) else (1, -1)
    lo = min(sub_lo, o_lo, e_lo) - 1
    hi = max(sub_hi, o_hi, e_hi) + 1
    w = _WF(lo, hi, has_i, has_d)
    for k in range(lo, hi + 1):
        ins = absent
        if has_i:
            g = _fetch(o_rows, o_lo, o_hi, k - 1, out_of_range)
            i = _fetch(i_rows, e_lo, e_hi, k - 1, out_of_range)
            ins = NULL if (g == NULL and i == NULL) else max(g, i) + 1
            w.I[k] = ins
        dele = absent
        if has_d:
            dele = max(_fetch(o_rows, o_lo, o_hi, k + 1, out_of_range), _fetch(d_rows, e_lo, e_hi, k + 1, out_of_range))
            w.D[k] = dele
        sub = absent
        if sub_rows is not None:
            sub = sub_rows[k] + 1 if sub_lo <= k <= sub_hi else out_of_range
        w.M[k] = max(sub, ins, dele)
    return w


def wfa_score(p, t, x, o, e, max_score, absent=ABSENT, out_of_range=NULL):
    """Score of one pair (bytes-like p, t). absent / out_of_range: what an absent source and an out-of-range fetch contribute;
    other values than the defaults are the mutations tests/test_penalty_rows_cpu.py uses."""
    plen, tlen = len(p), len(t)
    ak = tlen - plen
    w = _WF(0, 0, False, False)
    w.M[0] = 0
    wfs = {0: w}
    s = 0
    while True:
        if w is not None:
            M = w.M
            for k in range(w.lo, w.hi + 1):
                h = M[k]
                if h < 0:
                    continue
                v = h - k
                if v < 0:
                    continue
                while v < plen and h < tlen and p[v] == t[h]:
                    v += 1
                    h += 1
                M[k] = h
            if w.lo <= ak <= w.hi and M[ak] >= tlen:
                return s
        s += 1
        if s > max_score:
            return s
        w = _next(wfs, s, x, o, e, absent, out_of_range)
        if w is not None:
            wfs[s] = w


def scores(req, pat, txt, x, o, e, max_score, **kw):
    """wfa_score of every pair of a batch in the wire layout."""
    import numpy as np
    out = np.zeros(len(req), dtype=np.int64)
    for i in range(len(req)):
        out[i] = wfa_score(bytes(pat[i, :int(req["pattern_len"][i])]), bytes(txt[i, :int(req["text_len"][i])]), x, o, e, max_score, **kw)
    return out
