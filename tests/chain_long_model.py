"""Chaining for long reads (include/aim_hip.h, AIM_FEATURE_SEED_CHAIN_LONG) in plain numpy, written from the rule's text: it is
aim_seed_chain_device's rule over minimizer seeds with the hit cap H in the place of AIM_SEED_MAX_HITS and read_size up to 65 528.
The parts of the rule that section leaves as they were -- the DP, the trees and their chains -- are tests/chain_model.py's, the
queries, codes and the minimizer selection tests/seed_model.py's and tests/minimizer_model.py's; the anchor collection with its cap,
the ranking, the windows and the rows are written here. It shares no code with the library and assigns to no other model's
constants."""
import numpy as np

import chain_model as cm
import minimizer_model as mm
import seed_model as m

MAX_READ_SIZE = 65528
MAX_HITS = 8192
MIN_HITS = 1024


def anchors(query, bucket, pos, k, w, max_occ, H):
    """Rules 2 and 3 for one query with the cap H: (the kept hits [(p, j)] in (j, p) order, truncated). The seeds are the query's
    (w, k) minimizers; w = 1 selects every valid k-mer."""
    code = m.kmer_codes(query, k)
    seeds = np.nonzero(mm.selected(query, k, w))[0] if len(code) else []
    out = []
    for j in seeds:
        c = int(code[j])
        lo, hi = int(bucket[c]), int(bucket[c + 1])
        if hi - lo == 0 or hi - lo > max_occ:
            continue
        out += [(int(p), int(j)) for p in pos[lo:hi]]
    return out[:H], len(out) > H


def strand_anchors(reads, read_len, index, k, w, max_occ, H):
    """Per read and strand: (anchors sorted by (p, j), number kept, truncated)."""
    bucket, pos = index
    out = []
    for r in range(len(read_len)):
        read = np.asarray(reads[r][:int(read_len[r])], dtype=np.uint8)
        for s in (0, 1):
            a, trunc = anchors(read if s == 0 else m.revcomp(read), bucket, pos, k, w, max_occ, H)
            out.append((sorted(a), len(a), trunc))
    return out


def seed_chain_long(reads, read_len, index, ref_len, k, w, max_occ, band, flank, min_votes, K, read_size, H, idx_base=0, detail=None):
    """The whole batch: (requests[n * K], text_pos[n * K], votes[n * K], seed rows[n], chains[n * K]) as the kernel writes them.
    detail: a list that receives (anchors, f, pred) per read and strand."""
    assert 0 <= band <= cm.MAX_BAND and 1 <= w <= mm.MAX_W
    assert MIN_HITS <= H <= MAX_HITS and H & (H - 1) == 0
    assert 0 < read_size <= MAX_READ_SIZE and read_size % 8 == 0
    n = len(read_len)
    sa = strand_anchors(reads, read_len, index, k, w, max_occ, H)
    fp = cm.dp([a for a, _, _ in sa], k, band)
    if detail is not None:
        detail += [(a, f, p) for (a, _, _), (f, p) in zip(sa, fp)]
    req = np.zeros(n * K, dtype=m.REQUEST)
    tpos = np.zeros(n * K, dtype=np.uint64)
    votes = np.zeros(n * K, dtype=np.uint32)
    rows = np.zeros(n, dtype=m.SEED)
    ch = np.zeros(n * K, dtype=cm.CHAIN)
    for r in range(n):
        L = int(read_len[r])
        found, flags = [], 0
        for s in (0, 1):
            a, kept, trunc = sa[2 * r + s]
            flags |= m.TRUNCATED if trunc else 0
            f, pred = fp[2 * r + s]
            assert not len(f) or (k <= f.min() and f.max() <= H * 14)
            found += [(c[0], s) + c[1:] for c in cm.chains(a, f, pred, k, min_votes)]
        found.sort(key=lambda c: (-c[0], c[1], c[3], c[4]))         # (score descending, strand, p_lo, q_lo)
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
