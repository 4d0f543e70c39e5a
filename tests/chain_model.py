"""Colinear chaining of the seed hits (include/aim_hip.h, AIM_FEATURE_SEED_CHAIN) in plain numpy, written from the rule's text: the
anchors, the DP with its 64-wide lookback, the trees and their chains, the ranking, the windows and the aim_chain_t rows. Rules 1-3
(queries, seeds, kept hits) come from tests/seed_model.py and tests/minimizer_model.py. It shares no code with the library.

The DP is sequential over the sorted anchors of a strand and vectorised two ways: over the 64 candidate predecessors of a step and
over all the strands of a batch at once, so a 256-read batch takes a second or two."""
import numpy as np

import minimizer_model as mm
import seed_model as m

LOOKBACK = 64
MAX_BAND = 4096
CHAIN = np.dtype([("score", "<u4"), ("n_anchors", "<u2"), ("reserved", "<u2"), ("q_lo", "<u2"), ("q_hi", "<u2"), ("ref_span", "<u4")])
_BITS = np.array([g.bit_length() for g in range(1 << 14)], dtype=np.int64)      # floor(log2 g) + 1, 0 for g = 0


def cost(g, k):
    """cost(0) = 0; cost(g) = ((g * k) >> 7) + ((floor(log2 g) + 1) >> 1). g: an int or an int64 array below 2^14."""
    g = np.asarray(g, dtype=np.int64)
    return np.where(g > 0, ((g * k) >> 7) + (_BITS[np.minimum(g, len(_BITS) - 1)] >> 1), 0)


def anchors(query, bucket, pos, k, stride, w, max_occ):
    """Rules 2 and 3 for one query: (the kept hits [(p, j)] in (j, p) order, truncated). w = None: the seeds sit at every stride-th
    offset; otherwise they are the query's (w, k) minimizers."""
    code = m.kmer_codes(query, k)
    if w is None:
        seeds = range(0, len(query) - k + 1, stride)
    else:
        seeds = np.nonzero(mm.selected(query, k, w))[0] if len(code) else []
    out = []
    for j in seeds:
        c = int(code[j])
        if c < 0:
            continue
        lo, hi = int(bucket[c]), int(bucket[c + 1])
        if hi - lo == 0 or hi - lo > max_occ:
            continue
        out += [(int(p), int(j)) for p in pos[lo:hi]]
    return out[:m.MAX_HITS], len(out) > m.MAX_HITS


def dp(strands, k, band):
    """The DP for a list of strands, each a list of anchors sorted by (p, j): per strand (f[n], pred[n]), pred -1 at a root."""
    B = len(strands)
    n = np.array([len(a) for a in strands], dtype=np.int64)
    N = int(n.max()) if B else 0
    # column LOOKBACK + i holds anchor i; the LOOKBACK columns in front are "no anchor" (f = 0)
    P = np.zeros((B, LOOKBACK + N), dtype=np.int64)
    J = np.zeros((B, LOOKBACK + N), dtype=np.int64)
    F = np.zeros((B, LOOKBACK + N), dtype=np.int64)
    for b, a in enumerate(strands):
        if a:
            P[b, LOOKBACK:LOOKBACK + len(a)] = [x[0] for x in a]
            J[b, LOOKBACK:LOOKBACK + len(a)] = [x[1] for x in a]
    pred = np.full((B, N), -1, dtype=np.int64)
    for i in range(N):
        live = i < n
        win = slice(i, i + LOOKBACK)                          # anchors i - 64 .. i - 1
        d_p = P[:, LOOKBACK + i, None] - P[:, win]
        d_q = J[:, LOOKBACK + i, None] - J[:, win]
        g = np.abs(d_p - d_q)
        ok = (F[:, win] > 0) & (d_p > 0) & (d_q > 0) & (g <= band)
        gain = np.minimum(np.minimum(d_p, d_q), k)
        score = np.where(ok, F[:, win] + gain - cost(np.where(ok, g, 0), k), -1)
        best = score.max(axis=1)
        nearest = LOOKBACK - 1 - np.argmax(score[:, ::-1], axis=1)      # the largest index among equal best scores
        take = live & (best > k)
        F[:, LOOKBACK + i] = np.where(live, np.where(take, best, k), 0)
        pred[:, i] = np.where(take, i - LOOKBACK + nearest, -1)
    return [(F[b, LOOKBACK:LOOKBACK + n[b]].copy(), pred[b, :n[b]].copy()) for b in range(B)]


def trees(f, pred):
    """(root[n], depth[n], ends {root: end}): every anchor's root and the length of its path to it, and each tree's end -- the anchor
    of greatest f, the lowest index on a tie."""
    n = len(f)
    root, depth, ends = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), {}
    for i in range(n):
        j = int(pred[i])
        root[i], depth[i] = (i, 1) if j < 0 else (root[j], depth[j] + 1)
        t = int(root[i])
        if t not in ends or f[i] > f[ends[t]]:
            ends[t] = i
    return root, depth, ends


def chains(a, f, pred, k, min_votes):
    """[(score, n_anchors, p_lo, q_lo, p_hi, q_hi)] of a strand's sorted anchors, the chains below min_votes dropped."""
    root, depth, ends = trees(f, pred)
    out = []
    for t, e in ends.items():
        if depth[e] >= min_votes:
            out.append((int(f[e]), int(depth[e]), a[t][0], a[t][1], a[e][0] + k, a[e][1] + k))
    return out


def path(pred, end):
    """The chain that ends at `end`, from its root on."""
    out = [end]
    while pred[out[-1]] >= 0:
        out.append(int(pred[out[-1]]))
    return out[::-1]


def strand_anchors(reads, read_len, index, k, stride, w, max_occ):
    """Per read and strand: (sorted anchors, number kept, truncated)."""
    bucket, pos = index
    out = []
    for r in range(len(read_len)):
        read = np.asarray(reads[r][:int(read_len[r])], dtype=np.uint8)
        for s in (0, 1):
            a, trunc = anchors(read if s == 0 else m.revcomp(read), bucket, pos, k, stride, w, max_occ)
            out.append((sorted(a), len(a), trunc))
    return out


def seed_chain(reads, read_len, index, ref_len, k, stride, w, max_occ, band, flank, min_votes, K, read_size, idx_base=0, detail=None):
    """The whole batch: (requests[n * K], text_pos[n * K], votes[n * K], seed rows[n], chains[n * K]) as the kernels write them.
    detail: a list that receives (anchors, f, pred) per read and strand."""
    assert 0 <= band <= MAX_BAND
    n = len(read_len)
    sa = strand_anchors(reads, read_len, index, k, stride, w, max_occ)
    fp = dp([a for a, _, _ in sa], k, band)
    if detail is not None:
        detail += [(a, f, p) for (a, _, _), (f, p) in zip(sa, fp)]
    req = np.zeros(n * K, dtype=m.REQUEST)
    tpos = np.zeros(n * K, dtype=np.uint64)
    votes = np.zeros(n * K, dtype=np.uint32)
    rows = np.zeros(n, dtype=m.SEED)
    ch = np.zeros(n * K, dtype=CHAIN)
    for r in range(n):
        L = int(read_len[r])
        found, flags = [], 0
        for s in (0, 1):
            a, kept, trunc = sa[2 * r + s]
            flags |= m.TRUNCATED if trunc else 0
            found += [(c[0], s) + c[1:] for c in chains(a, *fp[2 * r + s], k, min_votes)]
        found.sort(key=lambda c: (-c[0], c[1], c[3], c[4]))
        found = found[:K]
        rows[r] = (len(found), [sa[2 * r][1], sa[2 * r + 1][1]], flags)
        for i in range(K):
            slot = r * K + i
            req[slot] = (L, 0, 0, (idx_base + slot) & 0xFFFFFFFF)
            if i < len(found):
                score, s, n_anchors, p_lo, q_lo, p_hi, q_hi = found[i]
                lo = p_lo - q_lo - flank
                hi = p_hi + (L - q_hi) + flank
                start = max(lo, 0)
                end = max(start, min(hi, ref_len))
                req["text_len"][slot] = min(end - start, read_size)
                tpos[slot] = np.uint64(start | (s << 63))
                votes[slot] = score
                ch[slot] = (score, n_anchors, 0, q_lo, q_hi, p_hi - p_lo)
    return req, tpos, votes, rows, ch


# ---- what a strand's chains hold: counted by the tests that have to show their batches contain the cases ----------------------------
def branching(pred):
    """Anchors chosen as the predecessor of two or more successors."""
    return int((np.bincount(pred[pred >= 0]) >= 2).sum()) if (pred >= 0).any() else 0


def tied(a, f, pred, k, band):
    """Anchors whose best candidate score is reached by more than one admissible predecessor."""
    n_tied = 0
    for i in np.nonzero(pred >= 0)[0]:
        hits = 0
        for j in range(max(0, i - LOOKBACK), i):
            d_p, d_q = a[i][0] - a[j][0], a[i][1] - a[j][1]
            if d_p > 0 and d_q > 0 and abs(d_p - d_q) <= band and f[j] + min(d_p, d_q, k) - int(cost(abs(d_p - d_q), k)) == f[i]:
                hits += 1
        n_tied += hits > 1
    return n_tied


def strand_stats(d, k, band, with_ties):
    """What one strand's (anchors, f, pred) holds: branching anchors, links with g > 0, trees whose end is not their last anchor, and
    (where asked: the count is quadratic) anchors with tied best predecessors."""
    a, f, pred = d
    diag = np.array([p - j for p, j in a], dtype=np.int64)
    linked = np.nonzero(pred >= 0)[0]
    root, depth, ends = trees(f, pred)
    return dict(branching=branching(pred), gap_links=int((diag[linked] != diag[pred[linked]]).sum()),
                end_not_last=sum(1 for t, e in ends.items() if e != np.nonzero(root == t)[0].max()), ties=tied(a, f, pred, k, band) if with_ties else 0)
