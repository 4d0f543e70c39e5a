"""The synthetic slot tables the CPU and GPU tests of rule 17c share: secondary_model.synthetic's chains, classes and segments with
the rows of part 1 (or without: the reduction to rule 14c), secondary_model.synthetic_sam's records with d_sec from the part 2 model,
and on top of them what pairing needs -- positions and strands inside pair_model's three-contig layout, partners planted at spans of
every kind against primaries and secondaries alike so that ties occur in both reads, a contig per slot, and rescue records placed
against the mate's representative. Plain numpy, no device."""
import functools

import numpy as np

import pair_model as pm
import pair_secondary_model as psm
import secondary_model as scm

READ_SIZE, RESCUE_SIZE = pm.READ_SIZE, pm.RESCUE_SIZE
PENALTY = 6                     # a multiple of the score unit, so "the unpaired cost equals the pair's cost" occurs
SCORE_UNIT = scm.SYN_UNIT


def params(rescue=True, penalty=PENALTY):
    return pm.Params(pm.MIN_SPAN, pm.MAX_SPAN, penalty, pm.RESCUE if rescue else 0, RESCUE_SIZE)


def estimate(min_span=pm.MIN_SPAN + 20, max_span=pm.MAX_SPAN - 30):
    """An aim_pair_estimate_t whose bounds differ from params()': what d_est hands to the kernels."""
    from aim_amd import capi
    e = np.zeros(1, dtype=capi.PAIR_ESTIMATE_DTYPE)
    e["min_span"], e["max_span"], e["n_samples"], e["p25"], e["p50"], e["p75"] = min_span, max_span, 100, 380, 400, 420
    return e


@functools.lru_cache(maxsize=None)
def tables(seed, K, n_reads, contigs, secondaries=True):
    """A dict with seg, sam, cls, chains, sec, contig (None without contigs), res_sam, read_len, reads, starts, lens, ref_len. Built once
    per shape and shared: nobody writes to it."""
    rng = np.random.default_rng([int(seed), K, n_reads, int(contigs), int(secondaries), 0x31376330])
    starts, lens, ref_len = pm.layout()
    d = scm.synthetic(seed, n_reads, K, READ_SIZE)
    seg = scm.synthetic_rows(d, K, READ_SIZE, scm.SEC_MAX)[3] if secondaries else d["seg"]
    cls, chains = d["cls"], d["chains"]
    sam = scm.synthetic_sam(seed, K, n_reads, seg, cls)
    sec = scm.select(K, n_reads, seg, sam, cls, chains, scm.SYN_MAX_SCORE, SCORE_UNIT)
    part = psm.taking_part(K, n_reads, seg, sam, sec)
    S = n_reads * K

    def place(row, pos, rev, span=None):
        row["pos"] = min(max(int(pos), 0), ref_len - 1)
        row["ref_span"] = int(rng.integers(90, 111)) if span is None else span
        row["flags"] = (int(row["flags"]) & (pm.SAM_UNMAPPED | 0x800)) | (pm.SAM_REVERSE if rev else 0)   # the bits the split path sets

    def partner(row, other, kind):
        """`row` becomes the mate record of `other` at a span of the given kind."""
        span = {0: pm.MIN_SPAN - 1, 1: pm.MIN_SPAN, 2: int(rng.integers(pm.MIN_SPAN, pm.MAX_SPAN + 1)), 3: pm.MAX_SPAN, 4: pm.MAX_SPAN + 1}[kind]
        if other["flags"] & pm.SAM_REVERSE:       # row is the forward one: pos_f = pos_r + ref_span_r - span
            place(row, int(other["pos"]) + int(other["ref_span"]) - span, False)
        else:
            rs = int(rng.integers(90, 111))
            place(row, int(other["pos"]) + span - rs, True, span=rs)

    edges = [0, 3, ref_len - 1, ref_len - 120, int(starts[1]), int(starts[1]) + 40, int(starts[1] - pm.SPACER - 100), int(starts[2]) + 7, int(starts[0] + lens[0]) - 30]
    for s in range(S):
        place(sam[s], int(rng.choice(edges)) if rng.random() < 0.15 else int(rng.integers(200, ref_len - 700)), rng.random() < 0.5)
    for m in range(n_reads // 2):
        ia, ib = np.nonzero(part[2 * m])[0], np.nonzero(part[2 * m + 1])[0]
        if not len(ia) or not len(ib) or rng.random() < 0.35:
            continue
        i = int(rng.choice(ia))
        anchor = sam[2 * m * K + i]
        for i2 in ia:                                  # other slots of read 2m next to it: the same strand, the same place
            if i2 != i and rng.random() < 0.4:
                place(sam[2 * m * K + i2], int(anchor["pos"]) + int(rng.integers(0, 3)), bool(anchor["flags"] & pm.SAM_REVERSE), span=int(anchor["ref_span"]))
        for j in ib:                                   # slots of read 2m + 1 at spans of every kind
            if rng.random() < 0.6:
                partner(sam[(2 * m + 1) * K + j], anchor, int(rng.integers(0, 5)))
    contig_of = lambda pos: int(np.searchsorted(starts, pos, side="right") - 1)
    contig = np.zeros(S, dtype=np.uint32)
    for s in range(S):
        contig[s] = contig_of(int(sam["pos"][s])) if rng.random() < 0.93 else int(rng.integers(0, 3))
    res_sam = rng.integers(0, 256, size=n_reads * pm.SAM_DTYPE.itemsize, dtype=np.uint8).view(pm.SAM_DTYPE).copy()
    for b in range(n_reads):                           # the rescue records, placed against their anchor: the mate's representative
        res_sam["score"][b] = int(rng.integers(0, 8)) * SCORE_UNIT
        res_sam["flags"][b] = (int(res_sam["flags"][b]) & ~(pm.SAM_UNMAPPED | scm.SAM_SECONDARY)) | (pm.SAM_UNMAPPED if rng.random() < 0.25 else 0)
        res_sam["cigar_offset"][b], res_sam["md_offset"][b] = int(rng.integers(0, 1 << 20)), int(rng.integers(0, 1 << 20))
        place(res_sam[b], int(rng.integers(0, ref_len)), rng.random() < 0.5)
        rep = psm.representative(K, b ^ 1, part, sec)
        if rep is not None and rng.random() < 0.75:
            partner(res_sam[b], sam[(b ^ 1) * K + rep], int(rng.integers(0, 5)))
    return {"seg": seg, "sam": sam, "cls": cls, "chains": chains, "sec": sec, "contig": contig if contigs else None, "res_sam": res_sam,
            "read_len": d["read_len"], "reads": d["reads"], "starts": starts, "lens": lens, "ref_len": ref_len}


def run_model(t, K, n, rescue=True, est=None, options=scm.SEC_RECORDS, cigar_base=0, md_base=0, penalty=PENALTY):
    """The three stages of rule 17c and rule 16c's record list between them, by the models: a dict of everything a device run gives."""
    pp = params(rescue, penalty)
    e = None if est is None else est[0]
    out = {}
    out["req"], out["tpos"], out["rows"] = psm.rescue_rows(pp, K, READ_SIZE, t["ref_len"], n, t["read_len"], t["reads"], t["seg"], t["sam"], t["sec"], t["contig"],
                                                           t["starts"], t["lens"], est=e)
    out["pairs"], out["pq"], out["seg"], out["sam"], out["cls"], out["contig"], out["sec"] = psm.select(
        pp, K, READ_SIZE, n, t["read_len"], t["seg"], t["sam"], t["cls"], t["contig"], t["sec"], t["chains"], t["res_sam"], SCORE_UNIT, cigar_base, md_base, est=e)
    out["off"], out["rec_before"], out["msec"] = scm.records(K, n, options, out["seg"], out["sam"], out["cls"], out["sec"], out["contig"], t["starts"])
    out["rec"], out["mates"] = psm.mates(K, n, out["pairs"], out["sam"], out["sec"], out["contig"], t["starts"], out["off"], out["rec_before"])
    return out


# ---- truth class 1: an exact repeat, the read in copy B, a unique mate at a proper span beyond B ------------------------------------
T_MIN_SPAN, T_MAX_SPAN, T_SPAN, T_PENALTY = 800, 1200, 1000, 17


def truth_class1():
    """(ref, rows, read_len, truth): secondary_model's 16 error-free reads from copy B of the exact two-copy repeat as reads 2m, each
    with a mate 2m + 1 of 300 bases cut from the unique sequence at span T_SPAN -- behind B for a forward read, in front of it for a
    reverse one; copy A lies 8 000 bases away, outside any proper span. truth[m] = (lo, hi, strand) of the repeat read and of its mate."""
    import chain_class_model as ccm
    import seed_model as m
    ref, rows, rl, truth = scm.repeat_classes()["exact"]
    n, L = len(rl), scm.REPEAT_READ_LEN
    out = np.zeros((2 * n, ccm.CHIMERIC_SIZE), dtype=np.uint8)
    places = []
    for r in range(n):
        lo, hi, strand, _ = truth[r]
        mlo = hi - T_SPAN if strand else lo + T_SPAN - L
        assert not (mlo < scm.REPEAT_B + scm.REPEAT_LEN and mlo + L > scm.REPEAT_B) and not (mlo < scm.REPEAT_A + scm.REPEAT_LEN and mlo + L > scm.REPEAT_A)
        mate = ref[mlo:mlo + L]
        out[2 * r] = rows[r]
        out[2 * r + 1, :L] = mate if strand else m.revcomp(mate)
        places.append(((lo, hi, strand), (mlo, mlo + L, 1 - strand)))
    return ref, out, np.full(2 * n, L, dtype=np.int32), places


def truth_pair_params(max_reads, read_size):
    from aim_amd import engine
    return engine.pair_params(T_MIN_SPAN, T_MAX_SPAN, T_PENALTY, rescue=True, rescue_size=engine.round_up_8(T_MAX_SPAN - T_MIN_SPAN + read_size),
                              rescue_cigar_cap=max_reads * 64, rescue_md_cap=max_reads * 256)


# ---- truth class 4: both copies inside the span ------------------------------------------------------------------------------------------
T4_MIN_SPAN, T4_MAX_SPAN, T4_SPAN, T4_GAP = 600, 2600, 1600, 300


def truth_class4():
    """truth_class1's reads over a second fixture: the other copy of the repeat lies T4_GAP bases in front of copy B instead of 8 000,
    and the mates are cut at span T4_SPAN, clear of both copies, so the read pairs with its mate from either copy inside
    T4_MIN_SPAN..T4_MAX_SPAN. Returns (ref, rows, read_len, truth, start of the near copy)."""
    import chain_class_model as ccm
    import seed_model as m
    rng = np.random.default_rng(5)
    bases = np.frombuffer(b"ACGT", dtype=np.uint8)
    ref = bases[rng.integers(0, 4, size=scm.REPEAT_REF_LEN)].copy()
    near = scm.REPEAT_B - scm.REPEAT_LEN - T4_GAP
    ref[near:near + scm.REPEAT_LEN] = ref[scm.REPEAT_B:scm.REPEAT_B + scm.REPEAT_LEN]
    rows, rl, truth = scm.repeat_reads(ref, ())
    n, L = len(rl), scm.REPEAT_READ_LEN
    out = np.zeros((2 * n, ccm.CHIMERIC_SIZE), dtype=np.uint8)
    places = []
    for r in range(n):
        lo, hi, strand, _ = truth[r]
        mlo = hi - T4_SPAN if strand else lo + T4_SPAN - L
        assert mlo + L <= near or mlo >= scm.REPEAT_B + scm.REPEAT_LEN
        mate = ref[mlo:mlo + L]
        out[2 * r] = rows[r]
        out[2 * r + 1, :L] = mate if strand else m.revcomp(mate)
        places.append(((lo, hi, strand), (mlo, mlo + L, 1 - strand)))
    return ref, out, np.full(2 * n, L, dtype=np.int32), places, near


def truth4_pair_params(max_reads, read_size):
    from aim_amd import engine
    return engine.pair_params(T4_MIN_SPAN, T4_MAX_SPAN, T_PENALTY, rescue=True, rescue_size=engine.round_up_8(T4_MAX_SPAN - T4_MIN_SPAN + read_size),
                              rescue_cigar_cap=max_reads * 64, rescue_md_cap=max_reads * 256)


# ---- truth classes 2 and 3 ------------------------------------------------------------------------------------------------------------------
T2_PENALTIES = (17, 9)          # above and below the score difference between the copies, 3 per covered site: 12 or 15
T3_MAX_SCORE = 96               # the substituted mate costs 30 mismatches of 3


def _with_mates(ref, rows, rl, truth, mate_place, mutate=False):
    import chain_class_model as ccm
    import pair_batch as pb14
    import seed_model as m
    n, L = len(rl), scm.REPEAT_READ_LEN
    out = np.zeros((2 * n, ccm.CHIMERIC_SIZE), dtype=np.uint8)
    places = []
    for r in range(n):
        lo, hi, strand, _ = truth[r]
        mlo = mate_place(lo, hi, strand)
        for a in (scm.REPEAT_A, scm.REPEAT_B):
            assert mlo + L <= a or mlo >= a + scm.REPEAT_LEN
        mate = pb14.substituted(ref[mlo:mlo + L]) if mutate else ref[mlo:mlo + L]
        out[2 * r] = rows[r]
        out[2 * r + 1, :L] = mate if strand else m.revcomp(mate)
        places.append(((lo, hi, strand), (mlo, mlo + L, 1 - strand)))
    return ref, out, np.full(2 * n, L, dtype=np.int32), places


def truth_class2():
    """The diverged repeat, secondary_model's "control" reads cut from copy B (the chains and the alignment both prefer B), each with an
    exact mate at span T_SPAN from where the read would lie in copy A: only the combination with copy A -- an aligned secondary that
    costs 3 more per covered site -- is proper. truth[m] = ((lo, hi, strand) in copy B, the mate's); covered[m] = the sites the read covers."""
    ref, rows, rl, truth = scm.repeat_classes()["control"]
    d = scm.REPEAT_B - scm.REPEAT_A
    out = _with_mates(ref, rows, rl, truth, lambda lo, hi, strand: (hi - d) - T_SPAN if strand else (lo - d) + T_SPAN - scm.REPEAT_READ_LEN)
    return out + ([t[3] for t in truth],)


def truth_class3():
    """The diverged repeat, secondary_model's "tie" reads (the chains tie and rank copy A first; rule 16c's winner is the secondary, copy
    B), each with a mate next to copy B at span T_SPAN that carries a substitution at every 10th base: no chain, so only a rescue
    places it -- anchored at the representative, copy B. Anchored at slot 0, copy A, the window lies 8 000 bases away."""
    ref, rows, rl, truth = scm.repeat_classes()["tie"]
    return _with_mates(ref, rows, rl, truth, lambda lo, hi, strand: hi - T_SPAN if strand else lo + T_SPAN - scm.REPEAT_READ_LEN, mutate=True)


def truth_params(max_reads, read_size, penalty=T_PENALTY, rescue_cigar_cap=None, rescue_md_cap=None):
    from aim_amd import engine
    return engine.pair_params(T_MIN_SPAN, T_MAX_SPAN, penalty, rescue=True, rescue_size=engine.round_up_8(T_MAX_SPAN - T_MIN_SPAN + read_size),
                              rescue_cigar_cap=max_reads * 64 if rescue_cigar_cap is None else rescue_cigar_cap,
                              rescue_md_cap=max_reads * 256 if rescue_md_cap is None else rescue_md_cap)
