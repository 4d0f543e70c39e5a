"""The paired-end batch the rule-15c tests share, over a seeded reference of its own: 40 000 random bases with one 150-base segment planted
twice 300 bases apart (NEAR_A, NEAR_B) and a second one planted twice 20 000 bases apart (FAR_A, FAR_B). Mates are 100 bases at
read_size 104, K = 4, pair_batch's seeding parameters; the fallback bounds are 0..800 at rescue_size 904. Reads 2m and 2m + 1 are mates:
  c  256 concordant, error-free pairs; the fragment length is 400 plus a seeded integer draw of standard deviation ~25, clipped to 300..500
  w   16 pairs with the forward mate inside the SECOND copy of the near repeat and the reverse mate unique to the right of it, at a true
      span of 380..420. The chain model ranks the first copy -- 300 bases further from the mate -- first, and under 0..800 that copy
      still gives a proper pair, at a span of about 700. The two copies and the unique mate do not overlap.
  s   16 pairs, mate 2 with pair_batch.substituted: no chain, a rescue candidate (fragments 350..450)
  d   16 discordant pairs: eight on one strand, eight with the forward mate 5 000 bases to the RIGHT of the reverse one
  q   16 pairs with one mate inside the far repeat: its chain MAPQ is 0
  r    8 pairs, mate 2 random
  l    8 concordant pairs with fragments of 3 000 bases: samples beyond hist_size
tests/test_pair_estimate_cpu.py checks on the chain model and the ends-free DP model that the seeds below give the premises the GPU
expectations rest on; if one fails for a seed, another seed is picked, never a looser test."""
import numpy as np

import pair_batch as pb

REF_LEN, REF_SEED, READ_SEED = 40000, 2203, 91
NEAR_A, NEAR_B, FAR_A, FAR_B, REPEAT_LEN = 10000, 10300, 17000, 37000, 150
L, READ_SIZE, K = pb.L, pb.READ_SIZE, pb.K
K_MER, W, MAX_OCC, BAND, FLANK, MIN_VOTES = pb.K_MER, pb.W, pb.MAX_OCC, pb.BAND, pb.FLANK, pb.MIN_VOTES
X, O, E, MAX_SCORE = pb.X, pb.O, pb.E, pb.MAX_SCORE
MIN_SPAN, MAX_SPAN, RESCUE_SIZE, UNPAIRED_PENALTY = 0, 800, 904, 17
HIST_SIZE, MIN_SAMPLES, MIN_MAPQ, MIN_SLACK = 2048, 32, 20, 16
COUNTS = (("c", 256), ("w", 16), ("s", 16), ("d", 16), ("q", 16), ("r", 8), ("l", 8))
N_PAIRS = sum(n for _, n in COUNTS)
ZONES = ((600, 8800), (11600, 16000), (18200, 32000))      # away from the repeats and the ends by more than a window of the fallback

_CACHE = {}
revcomp, substituted = pb.revcomp, pb.substituted


def reference():
    if "ref" not in _CACHE:
        ref = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(REF_SEED).integers(0, 4, size=REF_LEN)].copy()
        ref[NEAR_B:NEAR_B + REPEAT_LEN] = ref[NEAR_A:NEAR_A + REPEAT_LEN]
        ref[FAR_B:FAR_B + REPEAT_LEN] = ref[FAR_A:FAR_A + REPEAT_LEN]
        _CACHE["ref"] = ref
    return _CACHE["ref"]


def batch():
    """dict(rows uint8[2 * N_PAIRS][READ_SIZE], read_len, truth): truth[m] = dict(cls, q, span, mates, repeat) with mates[x] = (lo, hi,
    strand) in the reference, or None for a random read; strand 1: the read is the reverse complement of ref[lo:hi]. span is the
    fragment length; repeat is the index (0 / 1) of the mate inside a repeat, for classes w and q."""
    if "batch" in _CACHE:
        return _CACHE["batch"]
    ref = reference()
    rng = np.random.default_rng(READ_SEED)
    rows = np.zeros((2 * N_PAIRS, READ_SIZE), dtype=np.uint8)
    truth = []

    def place(room):
        lo, hi = ZONES[int(rng.integers(0, len(ZONES)))]
        return int(rng.integers(lo, hi - room))

    def cut(lo, strand, mutate=False):
        seq = ref[lo:lo + L]
        seq = substituted(seq) if mutate else seq
        return (revcomp(seq) if strand else seq), (lo, lo + L, strand)

    def rand():
        return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=L)], None
    for cls, count in COUNTS:
        for q in range(count):
            flip = q % 2 == 1                                   # every other pair: read 2m is the reverse mate
            repeat = None
            if cls == "c":
                F = min(max(400 + int(round(float(rng.normal(0.0, 25.0)))), 300), 500)
                p = place(F)
            elif cls == "w":                                    # forward mate inside the second copy, the reverse mate ends F bases on
                F = int(rng.integers(380, 421))
                p = NEAR_B + 3 * q
                repeat = 1 if flip else 0
            elif cls == "s":
                F = int(rng.integers(350, 451))
                p = place(F)
            elif cls == "d":
                F = int(rng.integers(350, 451))
                lo, hi = ZONES[2]
                p = int(rng.integers(lo, hi - 6000))
            elif cls == "q":                                    # forward mate inside the far repeat's first or second copy
                F = int(rng.integers(380, 421))
                p = (FAR_A if q < 8 else FAR_B) + 3 * q
                repeat = 1 if flip else 0
            elif cls == "l":
                F = 3000
                lo, hi = ZONES[2]
                p = int(rng.integers(lo, hi - F))
            else:
                F = int(rng.integers(350, 451))
                p = place(F)
            left, right = (p, 0), (p + F - L, 1)                # (position, strand) of the forward and of the reverse mate
            if cls == "d":
                if q < 8:
                    right = (right[0], 0)                       # both on the forward strand
                else:
                    left = (p + 5000, 0)                        # everted: the forward mate lies to the right of the reverse one
            first, second = (right, left) if flip else (left, right)
            m1, t1 = cut(*first)
            m2, t2 = rand() if cls == "r" else cut(*second, mutate=cls == "s")
            rows[2 * len(truth), :L], rows[2 * len(truth) + 1, :L] = m1, m2
            truth.append(dict(cls=cls, q=q, span=F, mates=(t1, t2), repeat=repeat))
    _CACHE["batch"] = dict(rows=rows, read_len=np.full(2 * N_PAIRS, L, dtype=np.int32), truth=truth)
    return _CACHE["batch"]


def pairs_of(classes):
    """The indices m of the read pairs of the given classes."""
    return [m for m, t in enumerate(batch()["truth"]) if t["cls"] in classes]


def subset(ms):
    """(read_len, rows) of the read pairs ms, in that order."""
    b = batch()
    idx = np.array([r for m in ms for r in (2 * m, 2 * m + 1)], dtype=np.int64)
    return b["read_len"][idx].copy(), b["rows"][idx].copy()


def seed_params():
    return pb.seed_params()


def mapper_params(max_reads, slots=1):
    return pb.mapper_params(max_reads, slots=slots)


def pair_params(max_reads, min_span=MIN_SPAN, max_span=MAX_SPAN):
    from aim_amd import engine
    return engine.pair_params(min_span, max_span, UNPAIRED_PENALTY, rescue=True, rescue_size=RESCUE_SIZE, rescue_cigar_cap=max_reads * 64, rescue_md_cap=max_reads * 256)


def est_params():
    from aim_amd import engine
    return engine.pair_estimate_params(HIST_SIZE, MIN_SAMPLES, MIN_MAPQ, MIN_SLACK)
