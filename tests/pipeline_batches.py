"""The batches the seed-chain family of tests shares, over seed_model's reference: the parameter rows, the short, long, edge and
chimeric reads, and the chain model's output for a row over a batch, each made once per process (gpu_buffers.cached)."""
import os
import re

import numpy as np

from gpu_buffers import cached

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

READ_SIZE = 128
# (k, stride, w, max_occ, band, flank, min_votes, K); w = None: the full index at that stride
FULL = [(11, 1, None, 8, 8, 8, 2, 4), (8, 1, None, 64, 48, 16, 3, 16), (14, 3, None, 1, 16, 8, 1, 8), (11, 4, None, 2, 0, 0, 1, 1)]
MINIMIZER = [(11, 1, 5, 8, 32, 8, 2, 4), (13, 1, 10, 8, 32, 8, 2, 4),
             (8, 1, 2, 64, 48, 16, 3, 16)]   # minimizer strands that overflow the 1 024 kept hits (the reads from inside the tandem repeat)
LONG = (11, 1, 10, 8, 96, 16, 2, 4)          # the long reads' row, at read_size 1 024
LONG_SIZE, LONG_L, LONG_DEL, LONG_EDITS = 1024, 800, 60, 80


def index_tile():
    """kIndexTile, read from the index kernels' header."""
    return int(re.search(r"constexpr uint32_t kIndexTile = (\d+);", open(os.path.join(ROOT, "aim_amd", "csrc", "index.hpp")).read()).group(1))


def case_id(c):
    return "k%d-s%d-w%s-occ%d-b%d-f%d-v%d-K%d" % c


def reference():
    import seed_model as m
    return cached("ref", m.make_reference)


def short_reads():
    """seed_model's 256 reads in rows of 128."""
    import seed_model as m
    return cached("short", lambda: m.make_reads(reference(), 256, READ_SIZE))


def model_index(k, w):
    import minimizer_model as mm
    import seed_model as m
    return cached(("model index", k, w), lambda: m.build_index(reference(), k) if w is None else mm.build_index(reference(), k, w))


def expected(case, rows, rl, key, read_size=READ_SIZE, idx_base=0, ref=None, index=None):
    """The model's output for a parameter row over the batch `key`, computed once."""
    import chain_model as cm
    k, stride, w, max_occ, band, flank, min_votes, K = case
    ref = reference() if ref is None else ref
    return cached(("expected", case, key, read_size, idx_base),
                  lambda: cm.seed_chain(rows, rl, index or model_index(k, w), len(ref), k, stride, w, max_occ, band, flank, min_votes, K, read_size,
                                        idx_base=idx_base))


def model_chains(key, row, rows, rl, read_size):
    """expected() in the argument order of the CPU tests of the later stages."""
    return expected(row, rows, rl, key, read_size=read_size)


def long_reads():
    """64 reads of about 800 bases in rows of 1 024: 80 edits each, every second one with 60 reference bases deleted in the middle,
    every third from the minus strand; all but every 16th drawn clear of the planted copies, the N run, the lower-case bases and
    the tandem repeat. Returns (rows, read_len, true_pos, true_span, strand, clear, with_deletion)."""
    def make():
        import seed_model as m
        ref = reference()
        rng = np.random.default_rng(2024)
        n = 64
        rows, rl = np.zeros((n, LONG_SIZE), dtype=np.uint8), np.zeros(n, dtype=np.int32)
        pos, span, strand = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        clear, deleted = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
        for r in range(n):
            deleted[r], clear[r], strand[r] = r % 2 == 1, r % 16 != 5, r % 3 == 1
            span[r] = LONG_L + (LONG_DEL if deleted[r] else 0)
            p = m.clean_position(rng, int(span[r])) if clear[r] else int(rng.integers(0, len(ref) - span[r]))
            h = LONG_L // 2
            base = np.concatenate([ref[p:p + h], ref[p + h + LONG_DEL:p + span[r]]]) if deleted[r] else ref[p:p + LONG_L]
            read = m.edit(rng, base, LONG_EDITS)[:LONG_SIZE]
            read = m.revcomp(read) if strand[r] else read
            rows[r, :len(read)], rl[r], pos[r] = read, len(read), p
        return rows, rl, pos, span, strand, clear, deleted
    return cached("long", make)


def edge_reads():
    """Reads of 100 bases from the first and last 20 positions of the reference, both strands."""
    import seed_model as m
    ref = reference()
    starts = list(range(0, 20)) + list(range(len(ref) - 100 - 19, len(ref) - 100 + 1))
    rows = np.zeros((2 * len(starts), READ_SIZE), dtype=np.uint8)
    for i, p in enumerate(starts):
        rows[2 * i, :100] = ref[p:p + 100]
        rows[2 * i + 1, :100] = m.revcomp(ref[p:p + 100])
    return rows, np.full(len(rows), 100, dtype=np.int32), np.repeat(starts, 2)


def chimeric_expected():
    """(rows, read_len, halves, the chain model's outputs, the class model's rows, the split model's outputs) for the chimeric reads."""
    import chain_class_model as ccm
    import split_model as sm

    def make():
        ref = reference()
        rows, rl, halves = sm.chimeric(ref)
        K, flank = ccm.CHIMERIC_ROW[7], ccm.CHIMERIC_ROW[5]
        req, tpos, votes, seeds, chains = expected(ccm.CHIMERIC_ROW, rows, rl, "chimeric", read_size=ccm.CHIMERIC_SIZE)
        cls = ccm.classify(K, ccm.CHIMERIC_SIZE, 128, rl, tpos, seeds, chains)
        segs = sm.segments(K, ccm.CHIMERIC_SIZE, flank, len(ref), rl, rows, req, tpos, seeds, chains, cls)
        return rows, rl, halves, (req, tpos, seeds, chains), cls, segs
    return cached("chimeric expected", make)
