"""The test batches of aim_seed_chain_long_device, shared by tests/test_seed_chain_long_cpu.py (what the batches hold, from the model
alone) and tests/test_seed_chain_long_gpu.py (the kernel's bytes against the model's). Every batch, index and model output is made
once per process. A case is (k, w, max_occ, band, flank, min_votes, K, H, read_size)."""
import os
import re

import numpy as np

from gpu_buffers import cached

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_LEN = 1 << 18
TANDEM = (100000, 300, 40)          # batch E's reference: a 300-base unit, 40 copies in tandem

CASE_B = (11, 10, 8, 256, 16, 2, 4, 2048, 8232)
CASE_C = (11, 10, 8, 512, 16, 2, 4, 4096, 20608)
CASE_D1 = (11, 19, 8, 256, 16, 2, 4, 8192, 65464)
CASE_D2 = (11, 10, 8, 256, 16, 2, 4, 8192, 65464)
CASE_D3 = (11, 19, 8, 256, 16, 2, 4, 8192, 65528)
CASE_E = (11, 5, 64, 64, 16, 2, 4, 2048, 6144)
CASE_F = (11, 1, 8, 128, 16, 2, 4, 4096, 4136)
CASE_H = CASE_B[:4] + (150,) + CASE_B[5:]
B_EDITS, B_DEL = 80, 200
DUP = 40                            # bases of a tandem duplication in a read (batch E)


def tile():
    """kSeedLongTile, read from the kernel's header."""
    text = open(os.path.join(ROOT, "aim_amd", "csrc", "seed_chain_long.hpp")).read()
    return int(re.search(r"constexpr uint32_t kSeedLongTile = (\d+);", text).group(1))


def reference(tandem=False):
    """2^18 seeded random bases; tandem=True: the same with TANDEM planted."""
    def make():
        ref = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(4242).integers(0, 4, size=REF_LEN)].copy()
        if tandem:
            at, unit, copies = TANDEM
            ref[at:at + unit * copies] = np.tile(ref[at:at + unit], copies)
        return ref
    return cached(("chain long ref", tandem), make)


def model_index(k, w, tandem=False):
    import minimizer_model as mm
    return cached(("chain long index", k, w, tandem), lambda: mm.build_index(reference(tandem), k, w))


def draw(ref, seed, n, L, edits, read_size, deletion=0, every_del=2, starts=None, dups=0):
    """n reads of L reference bases with `edits` sequential edits in rows of read_size: read r lies across a deletion of `deletion`
    reference bases in its middle when r % every_del == 1, and is reverse-complemented when r % 3 == 1. dups: that many evenly spaced
    tandem duplications of DUP bases are among the read's L bases (it then covers L - dups * DUP reference bases): the first anchor of
    the second copy and the next anchor of the first both take the last anchor in front of the duplication as their predecessor, which
    is how a tree branches when the band is narrower than every repeat of the reference. Returns a dict: rows, rl, pos, span
    (reference bases covered), strand, deleted."""
    import seed_model as m
    rng = np.random.default_rng(seed)
    rows, rl = np.zeros((n, read_size), dtype=np.uint8), np.zeros(n, dtype=np.int32)
    pos, span, strand = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    deleted = np.zeros(n, dtype=bool)
    for r in range(n):
        deleted[r], strand[r] = deletion > 0 and r % every_del == 1, r % 3 == 1
        span[r] = L - dups * DUP + (deletion if deleted[r] else 0)
        p = int(rng.integers(0, len(ref) - span[r])) if starts is None else int(starts[r])
        h = L // 2
        base = np.concatenate([ref[p:p + h], ref[p + h + deletion:p + span[r]]]) if deleted[r] else ref[p:p + span[r]]
        for c in range(dups, 0, -1):                      # (from the far end, so the cut points stay where they were)
            at = c * len(base) // (dups + 1)
            base = np.concatenate([base[:at], base[at - DUP:at], base[at:]])
        read = (m.edit(rng, base, edits) if edits else base.copy())[:read_size]
        read = m.revcomp(read) if strand[r] else read
        rows[r, :len(read)], rl[r], pos[r] = read, len(read), p
    return dict(rows=rows, rl=rl, pos=pos, span=span, strand=strand, deleted=deleted)


def batch_b():
    """8 reads of 8 000 bases, 80 edits each, every second across a 200-base deletion, every third on the minus strand."""
    return cached("chain long B", lambda: draw(reference(), 1, 8, 8000, B_EDITS, CASE_B[8], deletion=B_DEL))


def batch_c():
    """4 reads of 20 000 bases with 3 % edits, every second across a 500-base deletion."""
    return cached("chain long C", lambda: draw(reference(), 2, 4, 20000, 600, CASE_C[8], deletion=500))


def batch_d1():
    """3 reads of 65 400 bases with 1 % edits, one on the minus strand."""
    return cached("chain long D1", lambda: draw(reference(), 3, 3, 65400, 654, CASE_D1[8]))


def batch_d2():
    """2 reads of 65 400 bases, one on each strand: at w = 10 the true strand holds more than 8 192 hits."""
    return cached("chain long D2", lambda: draw(reference(), 4, 2, 65400, 654, CASE_D2[8]))


def batch_d3():
    """One error-free read that fills a row of 65 528."""
    return cached("chain long D3", lambda: draw(reference(), 5, 1, 65528, 0, CASE_D3[8]))


def batch_e():
    """6 reads of 6 000 bases -- five tandem duplications of 40 bases among them -- with 1 % edits over the reference with the tandem
    repeat, the odd ones from inside the repeat."""
    def make():
        ref = reference(True)
        rng = np.random.default_rng(6)
        at, unit, copies = TANDEM
        starts = [at + int(rng.integers(0, unit * copies - 6000)) if r % 2 else int(rng.integers(0, at - 6000)) for r in range(6)]
        return draw(ref, 7, 6, 6000, 60, CASE_E[8], starts=starts, dups=5)
    return cached("chain long E", make)


def batch_f():
    """6 reads of 4 000 bases with 2 % edits, every second across a 100-base deletion (w = 1: every valid k-mer is a seed)."""
    return cached("chain long F", lambda: draw(reference(), 8, 6, 4000, 80, CASE_F[8], deletion=100))


def batch_h():
    """Reads of batch B's kind from the first and the last 100 reference bases."""
    span = 8000 + B_DEL
    starts = [0, 37, REF_LEN - 8000, REF_LEN - span - 41]       # (reads 1 and 3 lie across the deletion)
    return cached("chain long H", lambda: draw(reference(), 9, 4, 8000, B_EDITS, CASE_H[8], deletion=B_DEL, starts=starts))


def case_g(w):
    T = tile()
    return (11, w, 8, 64, 8, 2, 4, 1024, 3 * T + 64)


def batch_g():
    """Tile seams: every read length in [tile - 40, tile + 40] and [2 tile - 40, 2 tile + 40] and the lengths 0, k - 1, k and 3 tile,
    1 % substitutions, every third read on the minus strand; every fourth has a run of 30 N across a tile boundary of one strand's walk (from
    the read's start for strand 0, from its end for strand 1), and read 93 has a lower-case base at the boundary."""
    def make():
        import seed_model as m
        T, k = tile(), 11
        ref = reference()
        rs = 3 * T + 64
        lengths = list(range(T - 40, T + 41)) + list(range(2 * T - 40, 2 * T + 41)) + [0, k - 1, k, 3 * T]
        rng = np.random.default_rng(10)
        n = len(lengths)
        rows, rl, strand = np.zeros((n, rs), dtype=np.uint8), np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64)
        for r, L in enumerate(lengths):
            p = int(rng.integers(0, len(ref) - L - 1))
            read = ref[p:p + L].copy()
            for at in rng.integers(0, max(L, 1), size=L // 100):      # substitutions only: the lengths are the point
                read[at] = b"ACGT"[int(rng.integers(0, 4))]
            if r % 3 == 1:
                read, strand[r] = m.revcomp(read), 1
            n_len = len(read)
            if r % 4 == 0 and n_len > 100:
                at = T - 15 if r % 8 == 0 else n_len - T - 15        # across position T of the walk from the start / from the end
                at = max(min(at, n_len - 30), 0)                     # (a read below the tile has no seam: the run sits at its end)
                read[at:at + 30] = ord("N")
            if r == 93:
                read[T - 1] |= 0x20
            rows[r, :n_len], rl[r] = read, n_len
        return dict(rows=rows, rl=rl, strand=strand, lengths=np.array(lengths))
    return cached("chain long G", make)


def expected(case, b, key, tandem=False, idx_base=0, detail=None):
    """The model's output for a case over a batch, once per (case, key, idx_base)."""
    import chain_long_model as clm
    k, w, max_occ, band, flank, min_votes, K, H, read_size = case

    def make():
        d = []
        out = clm.seed_chain_long(b["rows"], b["rl"], model_index(k, w, tandem), REF_LEN, k, w, max_occ, band, flank, min_votes, K, read_size, H,
                                  idx_base=idx_base, detail=d)
        return out, d
    out, d = cached(("chain long expected", case, key, idx_base), make)
    if detail is not None:
        detail += d
    return out


def well_placed(case, b, key):
    """Per read: the model's rank 0 is on the read's strand and its window covers the read's true span."""
    K = case[6]
    req, tpos, votes, seed, chains = expected(case, b, key)
    start = (tpos[0::K] & np.uint64((1 << 63) - 1)).astype(np.int64)
    minus = (tpos[0::K] >> np.uint64(63)).astype(np.int64)
    end = start + req["text_len"][0::K]
    return (seed["n_cands"] >= 1) & (minus == b["strand"]) & (start <= b["pos"]) & (end >= b["pos"] + b["span"])
