"""Rule 15c (include/aim_hip.h, AIM_FEATURE_PAIR_ESTIMATE) in plain Python integers, written from the text of the rule: the sample rule, the
histogram, the quartiles by the cum definition, the bounds and the flags. One read pair at a time, no vectorising. estimate() returns the
48 bytes of aim_pair_estimate_t; params_with() turns them into the pair_model.Params that pair_model.rescue_rows and pair_model.select
take unchanged. synthetic_tables() is pair_model's, extended with what the sample rule distinguishes."""
import numpy as np

import map_records_model as mm
import pair_model as pm

ESTIMATE_DTYPE = np.dtype([("min_span", "<i8"), ("max_span", "<i8"), ("n_samples", "<u4"), ("n_beyond", "<u4"), ("p25", "<u4"), ("p50", "<u4"), ("p75", "<u4"),
                           ("flags", "<u4"), ("pad", "<u4", (2,))])
assert ESTIMATE_DTYPE.itemsize == 48
FALLBACK, CLAMPED, FLOORED = 0x1, 0x2, 0x4
MAX_HIST = 8192


class EstParams:
    """aim_pair_est_params_t as the model reads it."""

    def __init__(self, hist_size=2048, min_samples=64, min_mapq=20, min_slack=16):
        self.hist_size, self.min_samples, self.min_mapq, self.min_slack = hist_size, min_samples, min_mapq, min_slack


def sample(ep, K, m, mapped, sam, cls, contig):
    """The span of read pair m when it is a sample, else None."""
    slots = []
    for r in (2 * m, 2 * m + 1):
        own = [i for i in range(K) if mapped[r, i]]
        if len(own) != 1:                                  # unmapped, or split
            return None
        slots.append(r * K + own[0])
    x, y = slots
    if int(cls["mapq"][x]) < ep.min_mapq or int(cls["mapq"][y]) < ep.min_mapq:
        return None
    if contig is not None and int(contig[x]) != int(contig[y]):
        return None
    x_rev, y_rev = bool(sam["flags"][x] & pm.SAM_REVERSE), bool(sam["flags"][y] & pm.SAM_REVERSE)
    if x_rev == y_rev:
        return None
    f, r = (y, x) if x_rev else (x, y)
    pos_f, pos_r = int(sam["pos"][f]), int(sam["pos"][r])
    if pos_f > pos_r:
        return None
    return pos_r + int(sam["ref_span"][r]) - pos_f


def samples(ep, K, n_reads, seg, sam, cls, contig=None, order=None):
    """[(m, span)] over the read pairs that are samples, in the order given (the result of the rule does not depend on it)."""
    mapped = mm.mapped_slots(K, n_reads, seg, sam)
    out = []
    for m in (range(n_reads // 2) if order is None else order):
        s = sample(ep, K, int(m), mapped, sam, cls, contig)
        if s is not None:
            out.append((int(m), s))
    return out


def quartiles(hist, n):
    """(p25, p50, p75): p_q is the smallest s with 4 * cum(s) >= q * n; all 0 when n == 0."""
    if n == 0:
        return 0, 0, 0
    out = []
    for q in (1, 2, 3):
        cum = 0
        for s, c in enumerate(hist):
            cum += c
            if 4 * cum >= q * n:
                out.append(s)
                break
    return tuple(out)


def bounds(pp, ep, read_size, n_samples, p25, p50, p75):
    """(lo, hi, flags) by the bounds rule."""
    if n_samples < ep.min_samples:
        return pp.min_span, pp.max_span, FALLBACK
    flags = 0
    slack = max(3 * (p75 - p25), ep.min_slack)
    lo = p25 - slack
    if lo < 0:
        lo, flags = 0, flags | FLOORED
    hi = p75 + slack
    if pp.options & pm.RESCUE:
        W = pp.rescue_size - read_size
        if hi - lo > W:
            lo = max(p50 - W // 2, 0)
            hi = lo + W
            flags |= CLAMPED
    return lo, hi, flags


def estimate_from_spans(pp, ep, read_size, spans):
    """aim_pair_estimate_t (one item of ESTIMATE_DTYPE) from the samples' spans."""
    hist = [0] * ep.hist_size
    n = beyond = 0
    for s in spans:
        if s < ep.hist_size:
            hist[s] += 1
            n += 1
        else:
            beyond += 1
    p25, p50, p75 = quartiles(hist, n)
    lo, hi, flags = bounds(pp, ep, read_size, n, p25, p50, p75)
    out = np.zeros(1, dtype=ESTIMATE_DTYPE)
    out[0] = (lo, hi, n, beyond, p25, p50, p75, flags, (0, 0))
    return out


def estimate(pp, ep, K, read_size, n_reads, seg, sam, cls, contig=None, order=None):
    return estimate_from_spans(pp, ep, read_size, [s for _, s in samples(ep, K, n_reads, seg, sam, cls, contig, order)])


def params_with(pp, est):
    """pp with the estimated bounds: what pair_model.rescue_rows and pair_model.select run with under rule 15c."""
    return pm.Params(int(np.ravel(est["min_span"])[0]), int(np.ravel(est["max_span"])[0]), pp.unpaired_penalty, pp.options, pp.rescue_size)


def synthetic_tables(seed, K, n_reads, contigs):
    """pair_model.synthetic_tables with mapq bytes drawn on both sides of 20 (and the two edges 19 and 20 themselves), and with a share of
    the read pairs made single-slot -- every slot but one of either read loses AIM_SEG_VALID -- so that samples are common, while other
    reads keep a second mapped slot. The planted partners of pair_model give spans of 299..501; a few pairs get spans of 40..70 and of
    900..1100, so small and large histograms both see samples below and beyond hist_size."""
    t = pm.synthetic_tables(seed, K, n_reads, contigs)
    rng = np.random.default_rng([int(seed), K, n_reads, int(contigs), 0x657374])
    seg, sam, cls = t["seg"], t["sam"], t["cls"]
    cls["mapq"] = rng.choice(np.array([0, 3, 19, 20, 20, 37, 60, 60], dtype=np.uint8), size=len(cls))
    starts, lens = t["starts"], t["lens"]
    for m in range(n_reads // 2):
        u = rng.random()
        if u < 0.55:                                       # a single-slot pair at a chosen span: slot i of read 2m, slot j of read 2m + 1
            i, j = int(rng.integers(0, K)), int(rng.integers(0, K))
            kind = rng.random()
            span = int(rng.integers(40, 71)) if kind < 0.15 else int(rng.integers(900, 1101)) if kind < 0.3 else int(rng.integers(330, 471))
            c = int(rng.integers(0, 3))
            pos_f = int(starts[c]) + int(rng.integers(0, int(lens[c]) - 1200))
            span_r = min(int(rng.integers(30, 111)), span)
            rows = [(2 * m * K + i, pos_f, 0, int(rng.integers(90, 111))), ((2 * m + 1) * K + j, pos_f + span - span_r, pm.SAM_REVERSE, span_r)]
            if rng.random() < 0.5:                         # read 2m is the reverse one
                rows = [(2 * m * K + i, rows[1][1], rows[1][2], rows[1][3]), ((2 * m + 1) * K + j, rows[0][1], rows[0][2], rows[0][3])]
            for r, (slot, pos, rev, rspan) in zip((2 * m, 2 * m + 1), rows):
                seg["flags"][r * K:(r + 1) * K] &= ~np.uint8(pm.SEG_VALID)
                seg["flags"][slot] |= pm.SEG_VALID
                sam["pos"][slot], sam["ref_span"][slot] = pos, rspan
                sam["flags"][slot] = (int(sam["flags"][slot]) & mm.SAM_SUPPLEMENTARY) | rev
                if t["contig"] is not None:
                    t["contig"][slot] = c if rng.random() < 0.9 else (c + 1) % 3
            if rng.random() < 0.1 and K > 1:               # ... and a second mapped slot for read 2m: split, no sample
                extra = 2 * m * K + (i + 1) % K
                seg["flags"][extra] |= pm.SEG_VALID
                sam["flags"][extra] = int(sam["flags"][extra]) & ~pm.SAM_UNMAPPED
            if rng.random() < 0.1:                         # same strand: no sample
                sam["flags"][rows[1][0]] = (int(sam["flags"][rows[1][0]]) & ~pm.SAM_REVERSE) | (int(sam["flags"][rows[0][0]]) & pm.SAM_REVERSE)
    return t
