"""Bidirectional gap-affine WFA (AIM_FLAG_WFA_BIDIR) in plain Python: the model wfa_bidir_kernel follows step by step.

Costs: match 0, mismatch x, a maximal run of L insertions or deletions o + L*e. Offsets are the reference's (h along the text,
diagonal k = h - v), but every wavefront is clipped to the matrix: a cell with v > plen or h > tlen is NULL, so the forward and
the reverse wavefronts only ever hold in-matrix cells and their overlap is a point of a real alignment.

- wf_align(): forward WFA from (0, 0) starting in component `cs` to (plen, tlen) ending in component `ce`, with a history and the
  walk of the reference (W7 order: deletion extend, deletion open, insertion extend, insertion open, mismatch). Starting in I or
  D means the gap that crosses the start is already open: score 0 has that component at offset 0 next to M.
- breakpoint(): forward and reverse score-only WFA until they provably met, as in Marco-Sola et al. 2023 (the scope of
  max(x, o + e) + 1 scores, the collision phase on anti-diagonals, then the overlap phase with its stop rule).
- align(): the explicit stack of sub-problems, right half first, base case wf_align() at a score bound <= T or a short side.

Component ids: 0 M, 1 I, 2 D."""
M, I, D = 0, 1, 2
NULL = None


def _clip(off, k, plen, tlen):
    if off is None:
        return None
    if off > tlen or off - k > plen or off < 0 or off - k < 0:
        return None
    return off


def _max(a, b):
    return b if a is None else a if b is None else max(a, b)


def _extend(P, T, off, k):
    v, h = off - k, off
    while v < len(P) and h < len(T) and P[v] == T[h]:
        v += 1
        h += 1
    return h


class Wfa:
    """One direction's wavefronts: wf[s] = [M, I, D], each a dict k -> offset (h), NULL cells absent; None for a NULL score."""

    def __init__(self, P, T, x, o, e, cs, open_first=False):
        self.P, self.T, self.x, self.o, self.e = P, T, x, o, e
        self.plen, self.tlen = len(P), len(T)
        if open_first and cs != M:
            # the reverse direction of a sub-problem that ends inside a gap: its first op is that gap, opened here (the sub-problem
            # pays the open; the one after it continues the gap for free), so the first wavefront is the open at score o + e
            k, off = (1, 1) if cs == I else (-1, 0)
            ok = _clip(off, k, self.plen, self.tlen) is not None
            w = [{k: _extend(P, T, off, k)}, {k: off}, {}] if cs == I else [{k: _extend(P, T, off, k)}, {}, {k: off}]
            self.wf = [None] * (o + e) + [w if ok else None]
            return
        # the forward direction of a sub-problem that starts inside a gap: the gap is open already (score 0 holds it next to M)
        w0 = [{0: _extend(P, T, 0, 0)}, {}, {}]
        if cs != M:
            w0[cs][0] = 0
        self.wf = [w0]

    def get(self, s, c, k):
        if s < 0 or s >= len(self.wf) or self.wf[s] is None:
            return None
        return self.wf[s][c].get(k)

    def step(self):
        """Compute and extend the next score's wavefront."""
        s = len(self.wf)
        x, oe, e = self.x, self.o + self.e, self.e
        ks = set()
        for src in (s - x, s - oe, s - e):
            if 0 <= src < s and self.wf[src] is not None:
                for c in range(3):
                    ks.update(self.wf[src][c].keys())
        if not ks:
            self.wf.append(None)
            return
        lo, hi = min(ks) - 1, max(ks) + 1
        nm, ni, nd = {}, {}, {}
        for k in range(lo, hi + 1):
            # every candidate clipped on its own (the walk tests them one by one): a diagonal's in-matrix offsets are an interval
            a, b = self.get(s - oe, M, k - 1), self.get(s - e, I, k - 1)
            ins = _max(_clip(None if a is None else a + 1, k, self.plen, self.tlen), _clip(None if b is None else b + 1, k, self.plen, self.tlen))
            a, b = self.get(s - oe, M, k + 1), self.get(s - e, D, k + 1)
            dele = _max(_clip(a, k, self.plen, self.tlen), _clip(b, k, self.plen, self.tlen))
            a = self.get(s - x, M, k)
            sub = _clip(None if a is None else a + 1, k, self.plen, self.tlen)
            if ins is not None:
                ni[k] = ins
            if dele is not None:
                nd[k] = dele
            cand = [t for t in (ins, dele, sub) if t is not None]
            if cand:
                nm[k] = _extend(self.P, self.T, max(cand), k)
        self.wf.append([nm, ni, nd] if (nm or ni or nd) else None)

    def max_antidiag(self, s):
        if s >= len(self.wf) or self.wf[s] is None or not self.wf[s][M]:
            return -1
        return max(2 * off - k for k, off in self.wf[s][M].items())


def wf_align(P, T, x, o, e, cs=M, ce=M, max_s=1 << 30):
    """(score, ops) of the optimal global alignment that starts in component cs and ends in ce; (None, None) over max_s."""
    w = Wfa(P, T, x, o, e, cs)
    kend = len(T) - len(P)
    s = 0
    while w.get(s, ce, kend) != len(T):
        if s >= max_s:
            return None, None
        w.step()
        s += 1
    return s, walk(w, s, ce, cs)


def walk(w, s, ce, cs):
    """The reference's walk (wfa_wave.hpp), clipped, from component ce at (plen, tlen) back to component cs at (0, 0)."""
    x, oe, e = w.x, w.o + w.e, w.e
    k = w.tlen - w.plen
    off = w.tlen
    bt = ce
    ops = []
    while True:
        if s == 0:
            if bt == M:
                assert k == 0
                ops.extend("M" * off)
            else:
                assert bt == cs and k == 0 and off == 0
            break
        cl = lambda t, kk: _clip(t, kk, w.plen, w.tlen)
        del_ext = del_open = ins_ext = ins_open = mis = None
        if bt != I:
            del_ext = cl(w.get(s - e, D, k + 1), k)
            del_open = cl(w.get(s - oe, M, k + 1), k)
        if bt != D:
            t = w.get(s - e, I, k - 1)
            ins_ext = cl(None if t is None else t + 1, k)
            t = w.get(s - oe, M, k - 1)
            ins_open = cl(None if t is None else t + 1, k)
        if bt == M:
            t = w.get(s - x, M, k)
            mis = cl(None if t is None else t + 1, k)
        cand = [t for t in (del_ext, del_open, ins_ext, ins_open, mis) if t is not None]
        best = max(cand)
        if bt == M:
            assert best <= off
            ops.extend("M" * (off - best))
            off = best
        else:
            assert best == off
        if best == del_ext:
            ops.append("D"); s -= e; k += 1; bt = D
        elif best == del_open:
            ops.append("D"); s -= oe; k += 1; bt = M
        elif best == ins_ext:
            ops.append("I"); s -= e; k -= 1; off -= 1; bt = I
        elif best == ins_open:
            ops.append("I"); s -= oe; k -= 1; off -= 1; bt = M
        else:
            ops.append("X"); s -= x; off -= 1
    return "".join(reversed(ops))


class Breakpoint:
    def __init__(self, score):
        self.score = score          # best combined score found (initially the bound + 1: "none")
        self.v = self.h = None      # the forward cell (sub-problem coordinates)
        self.comp = M
        self.sf = self.sr = None    # the two halves' scores


def _overlap(new, old, s_new, s_old, new_is_fwd, scope, o, bp, plen, tlen):
    """The new wavefront (score s_new) against the other direction's last `scope` scores. Order: older score offset i = 0 ..
    scope - 1, then M, I, D, then diagonals upward (of the forward wavefront); the first strictly better candidate wins."""
    for i in range(scope):
        so = s_old - i
        if so < 0:
            break
        for c in (M, I, D):
            cand = s_new + so - (o if c != M else 0)
            if cand >= bp.score:
                continue
            fw, sfw, rv, srv = (new, s_new, old, so) if new_is_fwd else (old, so, new, s_new)
            if fw.wf[sfw] is None or rv.wf[srv] is None:
                continue
            hit = None
            for kf in sorted(fw.wf[sfw][c]):
                kr = (tlen - plen) - kf
                of, orr = fw.wf[sfw][c][kf], rv.wf[srv][c].get(kr)
                if orr is not None and of + orr >= tlen:
                    hit = (kf, of)
                    break
            if hit is not None:
                kf, of = hit
                bp.score, bp.comp = cand, c
                bp.v, bp.h = of - kf, of
                bp.sf = sfw
                bp.sr = srv - (o if c != M else 0)


def breakpoint(P, T, x, o, e, cs, ce, bound):
    """The breakpoint of an optimal alignment of score <= bound, or a Breakpoint whose score is bound + 1 (over the bound)."""
    plen, tlen = len(P), len(T)
    fw = Wfa(P, T, x, o, e, cs)
    rv = Wfa(P[::-1], T[::-1], x, o, e, ce, True)
    scope = max(x, o + e) + 1
    max_ad = plen + tlen - 1
    sf, sr = len(fw.wf) - 1, len(rv.wf) - 1
    fmax, rmax = fw.max_antidiag(sf), rv.max_antidiag(sr)
    bp = Breakpoint(bound + 1)
    last_fwd = False
    # collision phase: no cell of one direction can reach the other's yet
    while fmax + rmax < max_ad:
        if sf + max(sr - scope + 1, 0) - o > bound + scope:
            return bp
        sf += 1
        fw.step()
        fmax = max(fmax, fw.max_antidiag(sf))
        last_fwd = True
        if fmax + rmax >= max_ad:
            break
        sr += 1
        rv.step()
        rmax = max(rmax, rv.max_antidiag(sr))
        last_fwd = False
    # overlap phase (the paper's stop rule: no later overlap can beat the best one found)
    while True:
        if last_fwd:
            if sf + max(sr - (scope - 1), 0) - o >= bp.score:
                break
            _overlap(fw, rv, sf, sr, True, scope, o, bp, plen, tlen)
            sr += 1
            rv.step()
        if max(sf - (scope - 1), 0) + sr - o >= bp.score:
            break
        _overlap(rv, fw, sr, sf, False, scope, o, bp, plen, tlen)
        sf += 1
        fw.step()
        last_fwd = True
    return bp


def threshold(x, o, e, base_t=250):
    """The base-case score bound T the plan prints: at least base_t, and at least 2 * (max(x, o + e) + 1) + o."""
    return max(base_t, 2 * (max(x, o + e) + 1) + o)


def align(P, T, x=3, o=4, e=1, max_score=1 << 30, base_t=250, short=8, stats=None):
    """(score, ops) of BiWFA with the explicit stack; (max_score + 1, None) over the cap. `stats` collects breakpoint components."""
    # a breakpoint of a sub-problem of score > 2 * scope + o has both halves of score > 0 (the two directions' scores differ by
    # less than a scope): both are strictly smaller, so the recursion ends
    base_t = threshold(x, o, e, base_t)
    # whole pair: the base case up to T (the kernel runs the reference's own WFA and walk here: the flag-less bytes)
    s, ops = wf_align(P, T, x, o, e, M, M, min(base_t, max_score))
    if s is not None:
        return s, ops
    if max_score <= base_t:
        return max_score + 1, None
    bp = breakpoint(P, T, x, o, e, M, M, max_score)
    if bp.score > max_score:
        return max_score + 1, None
    total = bp.score
    out = []   # pieces, right to left
    # (v0, v1, h0, h1, start component, end component, score estimate, breakpoint already found). The estimate is the
    # breakpoint's split (sf, sr); a half's true score may differ from it (the forward cell lies on an optimal path, but the
    # overlap's scores need not split there), so the estimate only picks the first try, and no sub-problem is bounded by it.
    stack = [(0, len(P), 0, len(T), M, M, total, bp)]
    while stack:
        v0, v1, h0, h1, cs, ce, est, pre = stack.pop()
        p, t = P[v0:v1], T[h0:h1]
        if not p or not t:   # one gap run (or nothing): its ops need no WFA (and its two ends may share one open gap)
            out.append("I" * len(t) + "D" * len(p))
            continue
        if pre is None and (est <= base_t or min(len(p), len(t)) <= short):
            s, ops = wf_align(p, t, x, o, e, cs, ce, base_t)
            if s is not None:
                out.append(ops)
                continue
        b = pre if pre is not None else breakpoint(p, t, x, o, e, cs, ce, total)
        assert b.score <= total, (b.score, total)
        if b.score <= base_t:
            s, ops = wf_align(p, t, x, o, e, cs, ce, base_t)
            assert s == b.score
            out.append(ops)
            continue
        assert (b.v, b.h) not in ((0, 0), (len(p), len(t))), "no progress"
        if stats is not None:
            stats.append(b.comp)
        # right half first (it is popped first: the ops row is written from its end)
        stack.append((v0, v0 + b.v, h0, h0 + b.h, cs, b.comp, b.sf, None))
        stack.append((v0 + b.v, v1, h0 + b.h, h1, b.comp, ce, b.sr, None))
    return total, "".join(reversed(out))


def gotoh(P, T, x=3, o=4, e=1):
    """Brute-force in-matrix Gotoh DP score."""
    INF = 1 << 40
    n, m = len(P), len(T)
    Mx = [[INF] * (m + 1) for _ in range(n + 1)]
    Ix = [[INF] * (m + 1) for _ in range(n + 1)]
    Dx = [[INF] * (m + 1) for _ in range(n + 1)]
    Mx[0][0] = 0
    for i in range(n + 1):
        for j in range(m + 1):
            if i > 0:
                Dx[i][j] = min(Mx[i - 1][j] + o + e, Dx[i - 1][j] + e)
            if j > 0:
                Ix[i][j] = min(Mx[i][j - 1] + o + e, Ix[i][j - 1] + e)
            if i > 0 and j > 0:
                Mx[i][j] = Mx[i - 1][j - 1] + (0 if P[i - 1] == T[j - 1] else x)
            if i or j:
                Mx[i][j] = min(Mx[i][j], Ix[i][j], Dx[i][j])
    return Mx[n][m]
