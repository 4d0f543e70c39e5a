"""Device-side seeding (include/aim_hip.h, AIM_FEATURE_SEED) in plain Python / numpy: the index, the hits, the clusters, the ranking
and the slots, written from the rule's text. It shares no code with the library."""
import numpy as np

MAX_HITS = 1024
TRUNCATED = 1
CODE = {65: 0, 67: 1, 84: 2, 71: 3}            # A C T G: (ascii >> 1) & 3
COMP = {65: 84, 84: 65, 67: 71, 71: 67}        # only A C G T are complemented

REQUEST = np.dtype([("pattern_len", "<i4"), ("text_len", "<i4"), ("padding", "<i4"), ("idx", "<u4")])
SEED = np.dtype([("n_cands", "<u4"), ("n_hits", "<u4", (2,)), ("flags", "<u4")])


def kmer_codes(seq, k):
    """code[p] of the k-mer seq[p, p + k) for p = 0 .. len - k, or -1 where it covers a byte other than A C G T."""
    seq = np.asarray(seq, dtype=np.uint8)
    n = len(seq) - k + 1
    if n <= 0:
        return np.zeros(0, dtype=np.int64)
    base = np.full(256, -1, dtype=np.int64)
    for c, v in CODE.items():
        base[c] = v
    b = base[seq]
    code = np.zeros(n, dtype=np.int64)
    bad = np.zeros(n, dtype=bool)
    for i in range(k):
        code |= np.maximum(b[i:i + n], 0) << (2 * i)
        bad |= b[i:i + n] < 0
    code[bad] = -1
    return code


def build_index(ref, k):
    """(bucket[4^k + 1], pos[n_pos]): bucket is the exclusive prefix sum of the codes' counts, pos the positions by (code, position)."""
    code = kmer_codes(ref, k)
    p = np.nonzero(code >= 0)[0]
    order = np.argsort(code[p], kind="stable")
    bucket = np.zeros(4 ** k + 1, dtype=np.uint32)        # (uint32 throughout: 1 GiB at k = 14)
    np.add.at(bucket, code[p] + 1, 1)
    np.cumsum(bucket, out=bucket)
    return bucket, p[order].astype(np.uint32)


def revcomp(read):
    return np.array([COMP.get(int(c), int(c)) for c in read[::-1]], dtype=np.uint8)


def strand_hits(query, bucket, pos, k, stride, max_occ, read_size):
    """Rules 2 and 3 for one query: (kept keys in (j, p) order, truncated)."""
    code = kmer_codes(query, k)
    keys = []
    for j in range(0, len(query) - k + 1, stride):
        c = int(code[j])
        if c < 0:
            continue
        lo, hi = int(bucket[c]), int(bucket[c + 1])
        if hi - lo == 0 or hi - lo > max_occ:
            continue
        keys += [int(p) + read_size - j for p in pos[lo:hi]]
    return keys[:MAX_HITS], len(keys) > MAX_HITS


def clusters(keys, band):
    """Rule 4: [(votes, a_lo, a_hi)] of the sorted keys' maximal runs with consecutive differences <= band."""
    out = []
    for a in sorted(keys):
        if out and a - out[-1][2] <= band:
            out[-1] = (out[-1][0] + 1, out[-1][1], a)
        else:
            out.append((1, a, a))
    return out


def seed_read(read, bucket, pos, ref_len, k, stride, max_occ, band, flank, min_votes, K, read_size):
    """One read: ([(start, strand, text_len, votes)] for the candidates, n_hits[2], flags)."""
    L = len(read)
    cl, n_hits, flags = [], [0, 0], 0
    for s in (0, 1):
        keys, trunc = strand_hits(read if s == 0 else revcomp(read), bucket, pos, k, stride, max_occ, read_size)
        n_hits[s] = len(keys)
        flags |= TRUNCATED if trunc else 0
        cl += [(v, s, lo, hi) for v, lo, hi in clusters(keys, band) if v >= min_votes]
    cl.sort(key=lambda c: (-c[0], c[1], c[2]))
    cands = []
    for v, s, a_lo, a_hi in cl[:K]:
        lo = a_lo - read_size - flank
        hi = lo + L + 2 * flank + min(a_hi - a_lo, read_size)
        start = max(lo, 0)
        end = max(start, min(hi, ref_len))
        cands.append((start, s, min(end - start, read_size), v))
    return cands, n_hits, flags


def seed(reads, read_len, index, ref_len, k, stride, max_occ, band, flank, min_votes, K, read_size, idx_base=0):
    """The whole batch: (requests[n * K], text_pos[n * K], votes[n * K], seed rows[n]) as the kernel writes them."""
    bucket, pos = index
    n = len(read_len)
    req = np.zeros(n * K, dtype=REQUEST)
    tpos = np.zeros(n * K, dtype=np.uint64)
    votes = np.zeros(n * K, dtype=np.uint32)
    rows = np.zeros(n, dtype=SEED)
    for r in range(n):
        L = int(read_len[r])
        cands, n_hits, flags = seed_read(np.asarray(reads[r][:L], dtype=np.uint8), bucket, pos, ref_len, k, stride, max_occ, band, flank, min_votes, K,
                                         read_size)
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


# ---- the test data of tests/test_seed_cpu.py and tests/test_seed_gpu.py ---------------------------------------------------------
REF_LEN = 65536
PLANT_LEN, PLANT_AT = 300, (5000, 22000, 47000)
N_RUN = (30000, 50)              # a run of 50 'N'
LOWER = (40000, 200)             # 200 lower-case bases
TANDEM = (12000, 40, 24)         # a 40-base unit, 24 copies in tandem: every 8-mer of it occurs 24 times


def make_reference(seed=1234):
    """64 KiB of seeded random A C G T with a 300-base segment planted three times, a run of 50 N, lower-case bases and a tandem
    repeat. The tandem repeat is what lets a read overflow MAX_HITS: in random sequence an 8-mer occurs about once per 64 KiB, so a
    read's ~100 seeds find a few hundred hits at most; inside the repeat each finds 24."""
    rng = np.random.default_rng(seed)
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=REF_LEN)].copy()
    seg = ref[PLANT_AT[0]:PLANT_AT[0] + PLANT_LEN].copy()
    for at in PLANT_AT[1:]:
        ref[at:at + PLANT_LEN] = seg
    at, unit, copies = TANDEM
    ref[at:at + unit * copies] = np.tile(ref[at:at + unit], copies)
    ref[N_RUN[0]:N_RUN[0] + N_RUN[1]] = ord("N")
    ref[LOWER[0]:LOWER[0] + LOWER[1]] |= 0x20
    return ref


def clean_position(rng, L):
    """A start whose window [p, p + L) stays clear of the planted copies, the N run, the lower-case bases and the tandem repeat."""
    special = [(at, PLANT_LEN) for at in PLANT_AT] + [N_RUN, LOWER, (TANDEM[0], TANDEM[1] * TANDEM[2])]
    while True:
        p = int(rng.integers(0, REF_LEN - L))
        if all(p + L <= at or p >= at + n for at, n in special):
            return p


def edit(rng, seq, n_edits):
    """n_edits sequential uniform substitutions, insertions and deletions (gen_pairs' scheme)."""
    s = list(seq)
    for _ in range(n_edits):
        op, at = int(rng.integers(0, 3)), int(rng.integers(0, max(len(s), 1)))
        c = int(b"ACGT"[int(rng.integers(0, 4))])
        if op == 0 and s:
            s[at] = c
        elif op == 1:
            s.insert(at, c)
        elif s:
            del s[at]
    return np.array(s, dtype=np.uint8)


def make_reads(ref, n, read_size, seed=99):
    """n reads in rows of read_size: lengths 100 (about that after edits) and a few of exactly 0, 5, 8, 11, 14 and read_size; both
    strands; 0 / 2 / 5 % edits; some with an N; every 32nd from inside the tandem repeat. Returns (rows, read_len, true_pos, strand, plain): plain marks the error-free reads of length 100 without an N that
    were drawn clear of the planted copies, the N run, the lower-case bases and the tandem repeat."""
    rng = np.random.default_rng(seed)
    rows = np.zeros((n, read_size), dtype=np.uint8)
    rl = np.zeros(n, dtype=np.int32)
    true_pos, strand, plain = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=bool)
    odd = [0, 5, 8, 11, 14, read_size]
    for r in range(n):
        L = odd[(r // 16) % len(odd)] if r % 16 == 7 else 100
        p = int(rng.integers(0, len(ref) - read_size)) if r % 5 else clean_position(rng, max(L, 1))
        if r % 32 == 9:
            p = TANDEM[0] + int(rng.integers(0, TANDEM[1] * TANDEM[2] - read_size))
        e = 0 if r % 16 == 7 else (0, 0, 2, 5)[r % 4]
        read = ref[p:p + L].copy()
        read = edit(rng, read, -(-L * e // 100))[:read_size] if e else read
        if r % 3 == 1:
            read = revcomp(read)
        with_n = r % 11 == 3 and len(read) > 40
        if with_n:
            read[int(rng.integers(0, len(read)))] = ord("N")
        rows[r, :len(read)] = read
        rl[r], true_pos[r], strand[r] = len(read), p, int(r % 3 == 1)
        plain[r] = r % 5 == 0 and r % 32 != 9 and e == 0 and L == 100 and not with_n
    return rows, rl, true_pos, strand, plain
