"""The paired-end batch the rule-14c tests share, over a seeded reference of its own: 40 000 random bases with one 150-base segment
planted twice (REPEAT_A, REPEAT_B), also cut into three contigs at CUTS. Mates are 100 bases at read_size 104, fragments 300..500 bases,
reads 2m and 2m + 1 mates, eight pairs per class:
  a  concordant                                        b  mate 2 with a substitution every 10th base (10 mismatches, no intact 11-mer)
  c  mate 2 inside the second copy of the repeat, mate 1 unique beside it
  d  discordant: both mates on one strand (four pairs), or 5 000 bases apart (four pairs)
  e  mate 2 random                                     f  both mates random
  g  four fragments that end 10..40 bases in front of the first cut, mate 2 as in b (the rescue window is clipped by the contig's end),
     and four fragments that span the first cut (proper in one sequence, on two contigs in three)
tests/test_pairs_cpu.py checks on the chain model and the ends-free DP model that the seeds below give the premises the GPU expectations
rest on; if one fails for a seed, another seed is picked, never a looser test."""
import numpy as np

REF_LEN, REF_SEED, READ_SEED = 40000, 1405, 77
REPEAT_A, REPEAT_B, REPEAT_LEN = 10000, 30000, 150
CUTS = (13000, 27000)
L, READ_SIZE, RESCUE_SIZE = 100, 104, 512
MIN_SPAN, MAX_SPAN, UNPAIRED_PENALTY = 300, 500, 17
K_MER, W, MAX_OCC, BAND, FLANK, MIN_VOTES, K = 11, 5, 8, 16, 2, 3, 4      # (a window of L + 2 * FLANK fits READ_SIZE)
X, O, E, MAX_SCORE = 3, 4, 1, 40
CLASSES = "abcdefg"
PER_CLASS = 8
N_PAIRS = PER_CLASS * len(CLASSES)
ZONES = ((500, 9000), (14000, 26000), (31000, 39000))      # away from the repeat, the cuts and the ends by more than a window

_CACHE = {}
_COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    _COMP[_a] = _b


def revcomp(seq):
    return _COMP[np.asarray(seq, dtype=np.uint8)][::-1]


def reference():
    if "ref" not in _CACHE:
        ref = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(REF_SEED).integers(0, 4, size=REF_LEN)].copy()
        ref[REPEAT_B:REPEAT_B + REPEAT_LEN] = ref[REPEAT_A:REPEAT_A + REPEAT_LEN]
        _CACHE["ref"] = ref
    return _CACHE["ref"]


def contigs():
    """The reference cut at CUTS: a list of three uint8 arrays."""
    ref = reference()
    edges = (0,) + CUTS + (REF_LEN,)
    return [ref[a:b].copy() for a, b in zip(edges, edges[1:])]


def contig_of(pos):
    """(contig, offset of the contig in the uncut reference) of a position."""
    c = sum(pos >= cut for cut in CUTS)
    return c, ((0,) + CUTS)[c]


def substituted(seq):
    """A substitution at every 10th base, from index 5: ten mismatches, no run of 11 intact bases."""
    out = np.array(seq, dtype=np.uint8)
    for i in range(5, len(out), 10):
        out[i] = {ord("A"): ord("C"), ord("C"): ord("G"), ord("G"): ord("T"), ord("T"): ord("A")}[int(out[i])]
    return out


def batch():
    """dict(rows uint8[2 * N_PAIRS][READ_SIZE], read_len, truth): truth[m] = dict(cls, mates) with mates[x] = (lo, hi, strand) in the
    uncut reference, or None for a random read; strand 1: the read is the reverse complement of ref[lo:hi]."""
    if "batch" in _CACHE:
        return _CACHE["batch"]
    ref = reference()
    rng = np.random.default_rng(READ_SEED)
    rows = np.zeros((2 * N_PAIRS, READ_SIZE), dtype=np.uint8)
    truth = []

    def place():
        lo, hi = ZONES[int(rng.integers(0, len(ZONES)))]
        return int(rng.integers(lo, hi - MAX_SPAN))

    def cut(lo, strand, mutate=False):
        seq = ref[lo:lo + L]
        seq = substituted(seq) if mutate else seq
        return (revcomp(seq) if strand else seq), (lo, lo + L, strand)

    def rand():
        return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=L)], None
    for ci, cls in enumerate(CLASSES):
        for q in range(PER_CLASS):
            F = int(rng.integers(MIN_SPAN, MAX_SPAN + 1))
            flip = q % 2 == 1                                   # every other pair: read 2m is the reverse mate
            p = place()
            if cls == "c":                                      # mate 2 inside the second copy, mate 1 unique on its side of it
                at = REPEAT_B + 10 + 4 * q
                p = at + L - F if not flip else at
            elif cls == "d" and q >= 4:
                p = int(rng.integers(14000, 20000))
            elif cls == "g":
                p = CUTS[0] - F - 10 * (q + 1) if q < 4 else CUTS[0] - F + L + 20 * (q - 3)
                flip = False
            left, right = (p, 0), (p + F - L, 1)                # (position, strand) of the forward and of the reverse mate
            if cls == "g" or not flip:
                first, second = left, right
            else:
                first, second = right, left
            if cls == "d":
                second = (second[0], first[1]) if q < 4 else (second[0] + 5000, second[1])
            m1, t1 = cut(*first) if cls != "f" else rand()
            m2, t2 = cut(*second, mutate=cls == "b" or (cls == "g" and q < 4)) if cls not in "ef" else rand()
            rows[2 * len(truth), :L], rows[2 * len(truth) + 1, :L] = m1, m2
            truth.append(dict(cls=cls, q=q, span=F, mates=(t1, t2)))
    _CACHE["batch"] = dict(rows=rows, read_len=np.full(2 * N_PAIRS, L, dtype=np.int32), truth=truth)
    return _CACHE["batch"]


def seed_params():
    from aim_amd import engine
    return engine.seed_params(K_MER, READ_SIZE, stride=1, max_occ=MAX_OCC, band=BAND, flank=FLANK, min_votes=MIN_VOTES, max_cands=K, w=W)


def mapper_params(max_reads, slots=1, cigar_cap=None, md_cap=None):
    from aim_amd import engine
    return engine.mapper_params(seed_params(), max_reads, MAX_SCORE, mismatch=X, gap_o=O, gap_e=E, slots=slots, cigar_cap=cigar_cap, md_cap=md_cap)


def pair_params(max_reads, rescue=True, rescue_cigar_cap=None, rescue_md_cap=None):
    from aim_amd import engine
    return engine.pair_params(MIN_SPAN, MAX_SPAN, UNPAIRED_PENALTY, rescue=rescue, rescue_size=RESCUE_SIZE,
                              rescue_cigar_cap=max_reads * 64 if rescue_cigar_cap is None else rescue_cigar_cap,
                              rescue_md_cap=max_reads * 256 if rescue_md_cap is None else rescue_md_cap)
