"""Hand-built seed indexes: for the five seeding kernels the index is an input, so a test can write the occurrence list of every k-mer
of a read and put each hit exactly where the rule (include/aim_hip.h, AIM_FEATURE_SEED .. AIM_FEATURE_SEED_CHAIN_LONG) has an edge,
at positions up to AIM_SEED_MAX_REF_LEN. This file holds the builder (index_from, distinct_read, Query), the scenarios, one function
each, and the table that groups them into batches: the scenarios of a batch share the parameters and read_size and go through a kernel
in one launch. The expectation is always one of the numpy models (seed_model, minimizer_model, chain_model, chain_long_model); this
file is plain numpy and shares no code with the library.

A scenario is written against the offsets a kernel looks up on each strand (Query.js): every offset under stride 1, the query's own
(W, k) minimizers for seed_minimizer_kernel, seed_chain_minimizer_kernel and seed_chain_long_kernel. A scenario that needs offsets a
read does not offer raises Unfit and the batch takes the next read of its pool; a batch that runs out of reads is an error."""
import numpy as np

import chain_long_model as clm
import chain_model as cm
import minimizer_model as mm
import seed_model as m

REF_LEN = 0xFE000000                    # AIM_SEED_MAX_REF_LEN
W = 4                                   # the minimizer window of the three minimizer kernels' runs
K_LIST = (1, 2, 3, 5, 7, 9, 10, 11, 15, 16)
KERNELS = ("cand", "min", "chain", "chain_min", "long")
VOTING = ("cand", "min")
MODE = {"cand": "stride", "chain": "stride", "min": "min", "chain_min": "min", "long": "min"}
LETTER = np.frombuffer(b"ACTG", dtype=np.uint8)          # by code: (ascii >> 1) & 3
E4_REF_LEN = 5000
E4_POS_ALLOC = 8192                     # entries of the device allocation of d_pos in E4, prefilled with 0xEE


class Unfit(Exception):
    """The read does not offer the offsets the scenario needs."""


# ---- the builder --------------------------------------------------------------------------------------------------------------------
def index_from(k, occ):
    """(bucket[4^k + 1] uint32, pos uint32) as INDEX lays them out: bucket by prefix sum of the run lengths, pos the runs in code order,
    each in the order given."""
    bucket = np.zeros(4 ** k + 1, dtype=np.uint32)
    codes = sorted(c for c in occ if len(occ[c]))
    for c in codes:
        bucket[c + 1] = len(occ[c])
    np.cumsum(bucket, out=bucket)
    pos = np.array([p for c in codes for p in occ[c]], dtype=np.uint32)
    return bucket, pos


def distinct_read(rng, L, k):
    """L bases of A C G T whose k-mer codes on both strands are pairwise distinct (no k-mer is its own reverse complement either), so
    every hit list is independently assignable. Greedy: a base that would repeat a code is replaced by the next one, and where none
    of the four fits the last 2 k bases are drawn again."""
    mask = (1 << (2 * k)) - 1
    used, seq, fr = set(), np.zeros(L, dtype=np.int64), [(0, 0)] * (L + 1)      # fr[i]: the two codes that end before base i
    first = rng.integers(0, 4, size=L)
    i = 0
    while i < L:
        f, r = fr[i]
        for t in range(4):
            b = (int(first[i]) + t) & 3
            nf = (f >> 2) | (b << (2 * (k - 1)))        # the forward k-mer that ends here
            nr = ((r << 2) & mask) | (b ^ 2)            # ... and its reverse complement
            if i < k - 1 or not (nf in used or nr in used or nf == nr):
                break
        else:
            back = max(i - 2 * k, 0)
            for x in range(max(back, k - 1), i):
                used.difference_update(fr[x + 1])
            first[back:i + 1] = rng.integers(0, 4, size=i + 1 - back)
            i = back
            continue
        if i >= k - 1:
            used.update((nf, nr))
        seq[i], fr[i + 1] = b, (nf, nr)
        i += 1
    return LETTER[seq]


class Query:
    """A read as a kernel sees it: code[s][j] of each strand's query and js[s], the offsets it looks up, ascending. w = None: every
    offset (stride 1); otherwise the query's own (w, k) minimizers -- minimizer_model.selected on each strand's query."""

    def __init__(self, read, k, w):
        self.read, self.k, self.L, self.w = read, k, len(read), w
        q = (read, m.revcomp(read))
        self.code = [m.kmer_codes(q[0], k), m.kmer_codes(q[1], k)]
        if w is None:
            self.js = [list(range(self.L - k + 1))] * 2
        else:
            self.js = [[int(j) for j in np.nonzero(mm.selected(q[s], k, w))[0]] for s in (0, 1)]

    def looked_up(self):
        return {int(self.code[s][j]) for s in (0, 1) for j in self.js[s]}


class Occ(dict):
    """occ under construction: {code: positions}, every code assigned once."""

    def __init__(self, q):
        super().__init__()
        self.q = q

    def put(self, s, j, positions):
        if j not in self.q.js[s]:
            raise Unfit
        c = int(self.q.code[s][j])
        assert c not in self and all(0 <= p <= REF_LEN - self.q.k for p in positions)
        self[c] = [int(p) for p in positions]


def top(k):
    """Hits sit in the top 2^20 positions below ref_len - k unless a scenario says otherwise."""
    return REF_LEN - k - (1 << 20)


def spaced(a, gap, start=0):
    """The greedy subsequence of the offsets a, from a[start] on, whose consecutive members are at least `gap` apart."""
    out = []
    for j in a[start:]:
        if not out or j - out[-1] >= gap:
            out.append(j)
    return out


def first_at_least(a, j):
    for x in a:
        if x >= j:
            return x
    raise Unfit


# ---- rules 2-3: hits ----------------------------------------------------------------------------------------------------------------
def h1(q, P, s=0, extra=False):
    """Exactly cap hits on strand s and none on the other; extra: one more hit at the strand's last seed."""
    a, cap, occ = q.js[s], P["cap"], Occ(q)
    n = len(a) - 1
    if n < 1 or n * P["max_occ"] < cap:
        raise Unfit
    per, left = -(-cap // n), cap
    for i in range(n):
        c = min(per, left)
        if c:
            occ.put(s, a[i], [top(q.k) + 4096 * i + 3 * t for t in range(c)])
        left -= c
    if extra:
        occ.put(s, a[-1], [top(q.k) + 4096 * n])
    return occ


def h2(q, P):
    """Strand 0 passes the cap within its seeds below offset 64; strand 1's only hits come from seeds beyond offset 64."""
    occ = Occ(q)
    low = [j for j in q.js[0] if j < 64]
    if len(low) * P["max_occ"] <= P["cap"]:
        raise Unfit
    for i, j in enumerate(low):
        occ.put(0, j, [top(q.k) + 4096 * i + 3 * t for t in range(P["max_occ"])])
    late = [j for j in q.js[1] if j >= 64][-3:]
    if len(late) < 3:
        raise Unfit
    for i, j in enumerate(late):
        occ.put(1, j, [top(q.k) + 700000 + j, top(q.k) + 700001 + j])
    return occ


def h3(q, P):
    """One code with n == max_occ (kept) and one with n == max_occ + 1 (skipped)."""
    occ = Occ(q)
    occ.put(0, q.js[0][0], [top(q.k) + 1000 * t for t in range(P["max_occ"])])
    occ.put(0, q.js[0][1], [top(q.k) + 500 + 1000 * t for t in range(P["max_occ"] + 1)])
    return occ


def h4(q, P):
    """One code with 3000 positions under max_occ = 5000: the run is cut at the cap inside a single seed."""
    occ = Occ(q)
    occ.put(0, q.js[0][0], [top(q.k) + 300 * t for t in range(3000)])
    return occ


def h5(q, P, last=False, p=0):
    """The only hit sits at the first seed (j = 0) or the last (j = L - k, L = read_size), at position 0 or ref_len - k."""
    occ = Occ(q)
    occ.put(0, q.L - q.k if last else 0, [p])
    return occ


# ---- rules 4-6: voting --------------------------------------------------------------------------------------------------------------
def v1(q, P, delta=0):
    """Two hits whose keys differ by exactly delta."""
    occ, (j1, j2) = Occ(q), q.js[0][:2]
    occ.put(0, j1, [top(q.k) + 5000])
    occ.put(0, j2, [top(q.k) + 5000 + delta + (j2 - j1)])
    return occ


def v2(q, P):
    """Two pairs, each exactly band apart: one with keys near read_size (p near 0), one with keys near ref_len."""
    occ, band = Occ(q), P["band"]
    j1, j2, j3, j4 = q.js[0][:4]
    occ.put(0, j1, [0])
    occ.put(0, j2, [band + (j2 - j1)])
    occ.put(0, j4, [REF_LEN - q.k])
    occ.put(0, j3, [REF_LEN - q.k - band - (j4 - j3)])
    return occ


def v3(q, P):
    """1024 hits spread over the whole position range."""
    occ, a, per = Occ(q), q.js[0], P["max_occ"]
    if len(a) * per < 1024:
        raise Unfit
    step = (REF_LEN - q.k) // 1023
    for i in range(1024 // per):
        occ.put(0, a[i], [step * t for t in range(i * per, (i + 1) * per)])
    return occ


def v4(q, P):
    """A cluster of min_votes - 1 hits and one of min_votes, each on one diagonal."""
    occ, a, mv = Occ(q), q.js[0], P["min_votes"]
    if len(a) < 2 * mv - 1:
        raise Unfit
    for i, j in enumerate(a[:2 * mv - 1]):
        occ.put(0, j, [top(q.k) + (0 if i < mv - 1 else 100000) + j])
    return occ


def v5(q, P):
    """10 clusters of 2 votes on each strand, their a_lo in scrambled order, and one cluster of 3 on strand 1."""
    occ = Occ(q)
    for s in (0, 1):
        a = q.js[s]
        if len(a) < 23:
            raise Unfit
        for c in range(10):
            for j in a[2 * c:2 * c + 2]:
                occ.put(s, j, [top(q.k) + 20000 * ((7 * c + 3) % 10) + j])
        if s:
            for j in a[20:23]:
                occ.put(s, j, [top(q.k) + 500000 + j])
    return occ


def v6(q, P, kind="lo"):
    """Windows under a large flank. lo: a_lo such that lo < 0; hi: a_hi such that hi > ref_len; span: a_hi - a_lo > read_size;
    s1: a start with bit 31 set on strand 1."""
    occ, a = Occ(q), q.js[0]
    if kind == "lo":
        for j in a[:2]:
            occ.put(0, j, [5 + j])
    elif kind == "hi":
        for j in a[-2:]:
            occ.put(0, j, [REF_LEN - q.k - a[-1] + j])
    elif kind == "span":
        if len(a) < 20:
            raise Unfit
        for i, j in enumerate(a[:20]):
            occ.put(0, j, [top(q.k) + 8 * i + (j - a[0])])
    else:
        for j in q.js[1][:2]:
            occ.put(1, j, [0x90000000 + j])
    return occ


# ---- rules 4c-6c: chaining ----------------------------------------------------------------------------------------------------------
def link_score(f, dp, dq, k):
    """f + gain - cost of rule 4c, for placing anchors; what a scenario claims is asserted on the models, not on this."""
    g = abs(dp - dq)
    return f + min(dp, dq, k) - (((g * k) >> 7) + (g.bit_length() >> 1))


def c1(q, P, fillers=63, prefix=0):
    """Anchor A, `fillers` anchors that sort between A and B and are admissible neither from A (g > band) nor to B (dq < 0), then B
    with A as its only admissible predecessor; `prefix` unrelated anchors sort in front of A."""
    occ, a, band = Occ(q), q.js[0], P["band"]
    jA = a[0]
    jB = first_at_least(a, jA + 66)
    jF = first_at_least(a, max(jB + 1, jA + 64 + band + 1))
    P0 = top(q.k) + 600000
    occ.put(0, jA, [P0])
    occ.put(0, jB, [P0 + (jB - jA)])
    occ.put(0, jF, [P0 + 1 + i for i in range(fillers)])
    if prefix:
        if a[-1] <= jF:
            raise Unfit
        occ.put(0, a[-1], [P0 - 500000 + 3 * t for t in range(prefix)])
    return occ


def c2(q, P, g=0, pre=1):
    """`pre` colinear anchors at least k apart, then one anchor whose gap to the last of them is exactly g."""
    occ = Occ(q)
    sp = spaced(q.js[0], q.k)
    if len(sp) < pre + 1:
        raise Unfit
    P0 = top(q.k) + 1000
    for j in sp[:pre]:
        occ.put(0, j, [P0 + j])
    jA, jB = sp[pre - 1], (sp[pre] if pre == 1 else q.js[0][-1])
    if jB - jA < q.k:
        raise Unfit
    occ.put(0, jB, [P0 + jB + g])
    return occ


def c3(q, P, over=0):
    """Two anchors; the best (only) candidate score of the second is exactly k + over."""
    occ, a, k = Occ(q), q.js[0], q.k
    for jA in a:
        for jB in a:
            for dp in range(1, 2 * k + P["band"]):
                dq = jB - jA
                if dq > 0 and abs(dp - dq) <= P["band"] and link_score(k, dp, dq, k) == k + over:
                    occ.put(0, jA, [top(k) + 2000])
                    occ.put(0, jB, [top(k) + 2000 + dp])
                    return occ
    raise Unfit


def c4(q, P, apart=1):
    """Two roots P1 < P2 that offer B the same score, `apart` sorted indexes from each other: B takes P2, the nearer."""
    occ, a, k = Occ(q), q.js[0], q.k
    x = 1 if apart == 1 else 32
    if x > P["band"]:
        raise Unfit
    j1 = a[0]
    jB = first_at_least(a, j1 + k + 2 * x)
    dq, P0 = jB - j1, top(k) + 3000
    occ.put(0, j1, [P0, P0 + 2 * x])
    occ.put(0, jB, [P0 + dq + x])
    if apart > 1:
        jF = first_at_least(a, max(jB + 1, j1 + 2 * x + P["band"] + 1))
        occ.put(0, jF, [P0 + 1 + i for i in range(apart - 1)])
    return occ


def c5(q, P, kind="tie"):
    """tie: a root with two children of equal f, so the tree has two anchors of equal greatest f. tail: root -> X -> Z with
    k < f(Z) < f(X), so the tree's end is not its last anchor."""
    occ, a, k = Occ(q), q.js[0], q.k
    P0 = top(k) + 4000
    if kind == "tie":
        j0 = a[0]
        jX = first_at_least(a, j0 + k)
        occ.put(0, j0, [P0])
        occ.put(0, jX, [P0 + (jX - j0), P0 + (jX - j0) + 1])
        return occ
    for j0 in a:
        jX = first_at_least(a, j0 + k)
        for jZ in a:
            for dp in range(1, 2 * k + P["band"]):
                dq = jZ - jX
                if dq > 0 and abs(dp - dq) <= P["band"] and k < link_score(2 * k, dp, dq, k) < 2 * k:
                    occ.put(0, j0, [P0])
                    occ.put(0, jX, [P0 + (jX - j0)])
                    occ.put(0, jZ, [P0 + (jX - j0) + dp])
                    return occ
    raise Unfit


def c6(q, P, kind="p"):
    """p: two anchors of equal p; j: two of equal j; far: p near 0 and p near ref_len - k with j increasing (dp above 2^31)."""
    occ, (j1, j2) = Occ(q), q.js[0][:2]
    if kind == "p":
        occ.put(0, j1, [top(q.k) + 6000])
        occ.put(0, j2, [top(q.k) + 6000])
    elif kind == "j":
        occ.put(0, j1, [top(q.k) + 6000, top(q.k) + 6000 + min(P["band"], 3) + 1])
    else:
        occ.put(0, j1, [3])
        occ.put(0, j2, [REF_LEN - q.k])
    return occ


def c7(q, P):
    """A colinear chain of min_votes - 1 anchors and, far from it, one of min_votes."""
    occ, mv = Occ(q), P["min_votes"]
    sp = spaced(q.js[0], q.k)
    if len(sp) < 2 * mv - 1:
        raise Unfit
    for i, j in enumerate(sp[:2 * mv - 1]):
        occ.put(0, j, [top(q.k) + (0 if i < mv - 1 else 100000) + j])
    return occ


def c8(q, P):
    """More than 16 single-anchor chains of score k per strand, p_lo scrambled, two of them with equal p_lo and different q_lo, and
    one two-anchor chain on strand 1."""
    occ = Occ(q)
    for s in (0, 1):
        a = q.js[s]
        if len(a) < 24:
            raise Unfit
        for i, j in enumerate(a[:18]):
            occ.put(s, j, [top(q.k) + 10000 + 1000 * ((7 * i + 5) % 18)])
        for j in a[18:20]:
            occ.put(s, j, [top(q.k) + 100])                # the smallest p_lo of the strand: q_lo decides between the two
        if s:
            jX = first_at_least(a[21:], a[20] + q.k)
            occ.put(s, a[20], [top(q.k) + 950000 + a[20]])
            occ.put(s, jX, [top(q.k) + 950000 + jX])
    return occ


def c9(q, P, kind="lo"):
    """Windows 6c under a large flank. lo: clamped at 0; hi: a chain that ends at p = ref_len - k and j = L - k, so q_hi == L ==
    read_size and the window is clamped at ref_len; s1: a chain on strand 1 (bit 31 of the position and bit 63 of text_pos)."""
    occ, s = Occ(q), int(kind == "s1")
    sp = spaced(q.js[s], q.k)
    if kind == "hi":
        sp = [j for j in q.js[0] if j <= q.L - 2 * q.k][-1:] + [q.L - q.k]
    if len(sp) < 2:
        raise Unfit
    base = {"lo": 5, "hi": REF_LEN - q.L, "s1": top(q.k)}[kind]
    for j in sp[:2]:
        occ.put(s, j, [base + j])
    return occ


# ---- the table ----------------------------------------------------------------------------------------------------------------------
def S(name, fn, high=True, **kw):
    return dict(name=name, fn=fn, kw=kw, high=high)


def P(k, read_size, max_occ, band, flank, min_votes, K=4, kernels=KERNELS, H=(1024,), ref_len=REF_LEN):
    return dict(k=k, read_size=read_size, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, K=K, kernels=kernels, H=H, ref_len=ref_len)


H1 = [S("H1.cap.s0", h1), S("H1.cap+1.s0", h1, extra=True), S("H1.cap.s1", h1, s=1), S("H1.cap+1.s1", h1, s=1, extra=True)]
TABLE = {
    # name: (parameters, scenarios). `cap` (the hit cap the H scenarios aim at) is filled in per run: 1024, or H for the long kernel.
    "a": (P(8, 128, 64, 8, 8, 2), H1 + [
        S("H2", h2), S("V1.band8.at", v1, delta=8), S("V1.band8.over", v1, delta=9), S("V2.band8", v2), S("V4.min2", v4),
        S("C2.band8.at", c2, g=8), S("C2.band8.over", c2, g=9), S("C4.1", c4, apart=1),
        S("C5.tie", c5, kind="tie"), S("C5.tail", c5, kind="tail"), S("C6.p", c6, kind="p"), S("C6.j", c6, kind="j"), S("C6.far", c6, kind="far"),
        S("C7.min2", c7)]),
    "a2048": (P(8, 128, 64, 8, 8, 2, kernels=("long",), H=(2048,)), H1),
    "b": (P(8, 128, 1, 0, 8, 1), [
        S("H3.occ1", h3), S("H5.first.0", h5, high=False), S("H5.first.top", h5, p=REF_LEN - 8), S("H5.last.0", h5, high=False, last=True),
        S("H5.last.top", h5, last=True, p=REF_LEN - 8), S("V1.band0.at", v1, delta=0), S("V1.band0.over", v1, delta=1), S("V2.band0", v2),
        S("C2.band0.at", c2, g=0), S("C2.band0.over", c2, g=1)]),
    "c": (P(8, 128, 16, 8, 8, 5), [S("H3.occ16", h3), S("V4.min5", v4), S("C7.min5", c7)]),
    "h4": (P(8, 128, 5000, 8, 8, 2, H=(1024, 2048)), [S("H4", h4)]),
    "v3": (P(8, 128, 64, (1 << 31) - 1, 8, 2, kernels=VOTING), [S("V3", v3)]),
    "v4c": (P(8, 128, 64, (1 << 31) - 1, 8, 1025, kernels=VOTING), [S("V4.min1025", v3)]),
    "v5": (P(8, 128, 64, 8, 8, 2, K=K_LIST), [S("V5", v5), S("V5.few", v1, delta=8)]),      # (.few: one candidate, so every K > 1 has empty slots)
    "c8": (P(8, 128, 64, 8, 8, 1, K=K_LIST), [S("C8", c8), S("C8.few", c2, g=0)]),
    "f": (P(8, 128, 64, 8, 10 ** 6, 1), [
        S("V6.lo", v6, high=False, kind="lo"), S("V6.hi", v6, kind="hi"), S("V6.span", v6, kind="span"), S("V6.s1", v6, kind="s1"),
        S("C9.lo", c9, high=False, kind="lo"), S("C9.hi", c9, kind="hi"), S("C9.s1", c9, kind="s1"),
        # (min_votes 1: a root at score k leaves two chains, a link one -- under min_votes 2 both leave none)
        S("C3.k", c3, over=0), S("C3.k+1", c3, over=1)]),
    "c1": (P(11, 1024, 128, 64, 8, 1), [
        S("C1.63.at0", c1, fillers=63), S("C1.64.at0", c1, fillers=64), S("C1.63.at81", c1, fillers=63, prefix=81),
        S("C1.64.at81", c1, fillers=64, prefix=81), S("C4.63", c4, apart=63)]),
    "c2": (P(11, 4096, 16, 4096, 8, 1), [S("C2.band4096.at", c2, g=4096, pre=40), S("C2.band4096.over", c2, g=4097, pre=40)]),
    "c2long": (P(11, 65528, 16, 4096, 8, 1, kernels=("long",)), [S("C2.long.at", c2, g=4096, pre=40), S("C2.long.over", c2, g=4097, pre=40)]),
    "e4": (P(8, 128, 16, 8, 8, 1, ref_len=E4_REF_LEN), [S("E4", None, high=False)]),
}
LARGEST = ("a", "c1")                   # the two batches with the most reads and anchors: the child-process runs
_POOL, _BATCH, _EXPECTED = {}, {}, {}


def pool(k, read_size):
    """The reads a batch draws from: one distinct_read cut into rows of read_size, so the codes of all of them are pairwise distinct.
    The seed is fixed per (k, read_size)."""
    if (k, read_size) not in _POOL:
        n = {128: 64, 1024: 12, 4096: 4, 65528: 3}[read_size]
        seq = distinct_read(np.random.default_rng(1000 * k + read_size), n * read_size, k)
        _POOL[k, read_size] = seq.reshape(n, read_size)
    return _POOL[k, read_size]


def e4_read(mode):
    """A 128-base read with distinct 8-mer codes that holds both A.X and C.X for one 7-mer X -- codes c and c + 1 -- and looks both up."""
    for seed in range(4000):
        rng = np.random.default_rng(77000 + seed)
        read = LETTER[rng.integers(0, 4, size=128)]
        read[70:78] = read[20:28]
        read[20], read[70] = ord("A"), ord("C")
        q = Query(read, 8, None if mode == "stride" else W)
        codes = np.concatenate(q.code)
        if len(set(codes.tolist())) == len(codes) and 20 in q.js[0] and 70 in q.js[0] and int(q.code[0][20]) + 1 == int(q.code[0][70]):
            return q
    raise RuntimeError("no E4 read")


def e4_batch(mode):
    """E4's arrays: a clean index (every code the read looks up gets two positions, c_a three, and one code it does not look up a long
    run that brings the total to pos_capacity - 3), then (a) bucket[c_a + 1] lowered below bucket[c_a] and (b) the entries behind the
    third-last looked-up code raised by 2, so that its run straddles pos_capacity and the last two runs lie beyond it."""
    k = 8
    q = e4_read(mode)
    cap = E4_REF_LEN - k + 1
    c_a = int(q.code[0][20])
    looked = sorted(q.looked_up())
    occ, t = {}, 0
    for c in looked:
        occ[c] = sorted((37 * (t + i)) % cap for i in range(3 if c == c_a else 2))
        t += 3
    pad = looked[-3] - 1
    assert pad not in set(np.concatenate(q.code).tolist()) and looked[0] < c_a and c_a + 1 < pad
    tail2 = len(occ[looked[-2]]) + len(occ[looked[-1]])
    occ[pad] = list(range(cap - 1 - sum(len(v) for v in occ.values())))       # the clean index holds cap - 1 positions
    clean = index_from(k, occ)
    assert int(clean[0][-1]) == cap - 1 and int(clean[0][looked[-3] + 1]) == cap - 1 - tail2
    bucket, pos = clean[0].copy(), clean[1]
    bucket[c_a + 1] = bucket[c_a] - 1                          # (a)
    bucket[looked[-3] + 1:] += np.uint32(tail2 + 2)            # (b): the run of looked[-3] now ends at cap + 1
    return q, clean, (bucket, pos), dict(c_a=c_a, last=looked[-3:], looked=looked)


def e4_affected(bucket, k=8):
    """The codes whose (b0, b1) fails b0 <= b1 <= pos_capacity, from the raw bucket array."""
    b0, b1 = bucket[:-1].astype(np.int64), bucket[1:].astype(np.int64)
    return np.nonzero(~((b0 <= b1) & (b1 <= E4_REF_LEN - k + 1)))[0]


def e4_model_index(raw, k=8):
    """What the tolerance sentence makes of the raw arrays: an affected code is absent, every other code has the run pos[b0, b1) the
    raw bucket gives it -- for the code behind the lowered entry that is a wrong run inside the array, in the array's order."""
    bucket, pos = raw
    bad = set(e4_affected(bucket, k).tolist())
    b = bucket.astype(np.int64)
    occ = {int(c): pos[b[c]:b[c + 1]].tolist() for c in np.nonzero(b[1:] != b[:-1])[0] if int(c) not in bad}
    return index_from(k, occ)


def batch(name, mode, H=1024):
    """The batch `name` for the kernels of `mode` ("stride" or "min") and the hit cap H: dict(params, rows, rl, scen [(scenario, row)],
    queries, index (the model's), raw (the arrays the kernel is given), dev_pos (the d_pos allocation's content))."""
    key = (name, mode, H)
    if key in _BATCH:
        return _BATCH[key]
    params, scen = TABLE[name]
    k, rs = params["k"], params["read_size"]
    PP = dict(params, cap=H if (mode == "min" and "long" in params["kernels"] and H != 1024) else 1024)
    if name == "e4":
        q, clean, raw, info = e4_batch(mode)
        index = e4_model_index(raw)
        dev_pos = np.full(E4_POS_ALLOC, 0xEEEEEEEE, dtype=np.uint32)
        dev_pos[:len(raw[1])] = raw[1]
        out = dict(params=params, rows=q.read.reshape(1, rs).copy(), rl=np.array([rs], dtype=np.int32), scen=[(scen[0], 0)], queries=[q],
                   index=index, raw=raw, dev_pos=dev_pos, clean=clean, info=info)
        _BATCH[key] = out
        return out
    reads, free = pool(k, rs), list(range(len(pool(k, rs))))
    occ, rows, queries, made = {}, [], [], {}
    for sc in scen:
        for at in free:
            if at not in made:
                made[at] = Query(reads[at], k, None if mode == "stride" else W)
            q = made[at]
            try:
                o = sc["fn"](q, PP, **sc["kw"])
            except Unfit:
                continue
            free.remove(at)
            break
        else:
            raise RuntimeError("no read of the pool fits %s (%s)" % (sc["name"], mode))
        assert not set(o) & set(occ)
        occ.update(o)
        rows.append(reads[at])
        queries.append(q)
    index = index_from(k, occ)
    out = dict(params=params, rows=np.array(rows, dtype=np.uint8), rl=np.full(len(rows), rs, dtype=np.int32), scen=[(sc, i) for i, sc in enumerate(scen)],
               queries=queries, index=index, raw=index, dev_pos=index[1])
    _BATCH[key] = out
    return out


def runs():
    """Every (batch name, kernel, H, K) the table asks for."""
    out = []
    for name, (params, _) in TABLE.items():
        for kernel in params["kernels"]:
            for H in (params["H"] if kernel == "long" else (1024,)):
                for K in (params["K"] if isinstance(params["K"], tuple) else (params["K"],)):
                    out.append((name, kernel, H, K))
    return out


def model(kernel, b, K, H=1024, index=None, detail=None, mods=None):
    """The model of `kernel` over batch b: the arrays as the kernel writes them (four for the voting kernels, five for the chaining).
    mods: other modules in the place of seed_model / minimizer_model / chain_model / chain_long_model, by those names."""
    mods = mods or {}
    sm, mn, ch, lg = (mods.get(n, d) for n, d in (("seed_model", m), ("minimizer_model", mm), ("chain_model", cm), ("chain_long_model", clm)))
    p = b["params"]
    args = (b["rows"], b["rl"], index or b["index"], p["ref_len"], p["k"])
    tail = (p["max_occ"], p["band"], p["flank"], p["min_votes"], K, p["read_size"])
    if kernel == "cand":
        return sm.seed(*args, 1, *tail)
    if kernel == "min":
        return mn.seed(*args, W, *tail)
    if kernel == "chain":
        return ch.seed_chain(*args, 1, None, *tail, detail=detail)
    if kernel == "chain_min":
        return ch.seed_chain(*args, 1, W, *tail, detail=detail)
    return lg.seed_chain_long(*args, W, *tail, H, detail=detail)


def expected(name, kernel, H, K):
    """model() for one run of the table, computed once."""
    key = (name, kernel, H, K)
    if key not in _EXPECTED:
        _EXPECTED[key] = model(kernel, batch(name, MODE[kernel], H), K, H)
    return _EXPECTED[key]
