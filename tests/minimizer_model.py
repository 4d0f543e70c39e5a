"""The (w, k) minimizer rule (include/aim_hip.h, AIM_FEATURE_MINIMIZERS) in plain Python / numpy, by its window definition: the order,
the windows, the selection, the index over the selected positions and a strand's seeds. Everything the rule leaves as it was -- codes,
clusters, ranking, slots -- is tests/seed_model.py's. It shares no code with the library."""
import numpy as np

import seed_model as m

MAX_W = 32
INVALID = 1 << 32                    # above every key, 0xFFFFFFFF included


def h(c):
    """The order key of the codes c: uint32 arithmetic throughout."""
    x = np.asarray(c, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    mask = np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x85EBCA6B)) & mask
    x ^= x >> np.uint64(13)
    x = (x * np.uint64(0xC2B2AE35)) & mask
    x ^= x >> np.uint64(16)
    return x


def keys(seq, k):
    """key[p] for p = 0 .. len - k (int64): h(code), or INVALID where the k-mer covers a byte other than A C G T."""
    code = m.kmer_codes(seq, k)
    key = h(np.maximum(code, 0)).astype(np.int64)
    key[code < 0] = INVALID
    return key


def windows(n, w):
    """The windows [lo, hi) over n positions."""
    if n <= 0:
        return []
    if n < w:
        return [(0, n)]
    return [(s, s + w) for s in range(n - w + 1)]


def selected(seq, k, w):
    """bool[n]: the positions that are the minimizer -- the leftmost position of smallest key -- of at least one window."""
    key = keys(seq, k)
    sel = np.zeros(len(key), dtype=bool)
    for lo, hi in windows(len(key), w):
        at = lo + int(np.argmin(key[lo:hi]))          # (argmin: the first of equal minima)
        if key[at] != INVALID:
            sel[at] = True
    return sel


def selected_local(seq, k, w):
    """The same set by the local test: a valid i with L + R + 1 >= min(w, n), L the run of strictly greater keys immediately to its
    left and R the run of greater-or-equal keys immediately to its right, both capped at w - 1."""
    key = keys(seq, k)
    n = len(key)
    sel = np.zeros(n, dtype=bool)
    for i in range(n):
        if key[i] == INVALID:
            continue
        L = R = 0
        while L < w - 1 and i - L - 1 >= 0 and key[i - L - 1] > key[i]:
            L += 1
        while R < w - 1 and i + R + 1 < n and key[i + R + 1] >= key[i]:
            R += 1
        sel[i] = L + R + 1 >= min(w, n)
    return sel


def build_index(ref, k, w):
    """seed_model.build_index over the selected positions alone."""
    code = m.kmer_codes(ref, k)
    p = np.nonzero(selected(ref, k, w))[0] if len(code) else np.zeros(0, dtype=np.int64)
    order = np.argsort(code[p], kind="stable")
    bucket = np.zeros(4 ** k + 1, dtype=np.uint32)
    np.add.at(bucket, code[p] + 1, 1)
    np.cumsum(bucket, out=bucket)
    return bucket, p[order].astype(np.uint32)


def strand_hits(query, bucket, pos, k, w, max_occ, read_size):
    """Rule 2 with minimizers and rule 3 for one query: (kept keys in (j, p) order, truncated, number of seeds)."""
    code = m.kmer_codes(query, k)
    out = []
    seeds = np.nonzero(selected(query, k, w))[0] if len(code) else []
    for j in seeds:
        c = int(code[j])
        lo, hi = int(bucket[c]), int(bucket[c + 1])
        if hi - lo == 0 or hi - lo > max_occ:
            continue
        out += [int(p) + read_size - int(j) for p in pos[lo:hi]]
    return out[:m.MAX_HITS], len(out) > m.MAX_HITS, len(seeds)


def seed_read(read, bucket, pos, ref_len, k, w, max_occ, band, flank, min_votes, K, read_size):
    """seed_model.seed_read with the minimizer seeds: ([(start, strand, text_len, votes)], n_hits[2], flags)."""
    L = len(read)
    cl, n_hits, flags = [], [0, 0], 0
    for s in (0, 1):
        hits, trunc, _ = strand_hits(read if s == 0 else m.revcomp(read), bucket, pos, k, w, max_occ, read_size)
        n_hits[s] = len(hits)
        flags |= m.TRUNCATED if trunc else 0
        cl += [(v, s, lo, hi) for v, lo, hi in m.clusters(hits, band) if v >= min_votes]
    cl.sort(key=lambda c: (-c[0], c[1], c[2]))
    cands = []
    for v, s, a_lo, a_hi in cl[:K]:
        lo = a_lo - read_size - flank
        hi = lo + L + 2 * flank + min(a_hi - a_lo, read_size)
        start = max(lo, 0)
        end = max(start, min(hi, ref_len))
        cands.append((start, s, min(end - start, read_size), v))
    return cands, n_hits, flags


def seed(reads, read_len, index, ref_len, k, w, max_occ, band, flank, min_votes, K, read_size, idx_base=0):
    """The whole batch in seed_model.seed's form: (requests[n * K], text_pos[n * K], votes[n * K], seed rows[n])."""
    bucket, pos = index
    n = len(read_len)
    req = np.zeros(n * K, dtype=m.REQUEST)
    tpos = np.zeros(n * K, dtype=np.uint64)
    votes = np.zeros(n * K, dtype=np.uint32)
    rows = np.zeros(n, dtype=m.SEED)
    for r in range(n):
        L = int(read_len[r])
        cands, n_hits, flags = seed_read(np.asarray(reads[r][:L], dtype=np.uint8), bucket, pos, ref_len, k, w, max_occ, band, flank, min_votes, K, read_size)
        rows[r] = (len(cands), n_hits, flags)
        for i in range(K):
            slot = r * K + i
            req[slot] = (L, 0, 0, (idx_base + slot) & 0xFFFFFFFF)
            if i < len(cands):
                start, s, tlen, v = cands[i]
                req["text_len"][slot] = tlen
                tpos[slot] = np.uint64(start | (s << 63))
                votes[slot] = v
    return req, tpos, votes, rows
