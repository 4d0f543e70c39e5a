"""The batch the mapper tests share, over seed_model's reference at read_size 1 024 with CHIMERIC_ROW's seed parameters: the 32 chimeric
reads of test_split_gpu.chimeric_expected(), 33 unbroken reads cut from the same reference with a few edits, and 8 random reads that the
chain model gives no chain (RANDOM_SEED was picked for that; tests/test_mapper_cpu.py checks it on the model)."""
import numpy as np

N_CHIMERIC, N_UNBROKEN, N_RANDOM = 32, 33, 8
UNBROKEN_EDITS, UNBROKEN_SEED = 6, 4242
RANDOM_LEN, RANDOM_SEED = 400, 7
# whole_path's penalties and cap (tests/test_extend_gpu.py): WFA (3, 4, 1), MAX_SCORE = CHIMERIC_EDITS * max(x, o + e) + 16
X, O, E = 3, 4, 1
EXTEND = (1, 3, 4, 1, 20, 400, 31, 64)

_CACHE = {}


def max_score():
    import chain_class_model as ccm
    return ccm.CHIMERIC_EDITS * max(X, O + E) + 16


def unbroken_reads(ref):
    """(rows, read_len, truth): reads of 250..600 bases from clean positions, UNBROKEN_EDITS edits each, every third from the minus
    strand; truth[r] = (ref_lo, ref_hi, strand)."""
    import chain_class_model as ccm
    import seed_model as m
    rng = np.random.default_rng(UNBROKEN_SEED)
    rows, rl, truth = np.zeros((N_UNBROKEN, ccm.CHIMERIC_SIZE), dtype=np.uint8), np.zeros(N_UNBROKEN, dtype=np.int32), []
    for r in range(N_UNBROKEN):
        L = int(rng.integers(250, 601))
        p = m.clean_position(rng, L)
        read = m.edit(rng, ref[p:p + L], UNBROKEN_EDITS)
        strand = int(r % 3 == 2)
        if strand:
            read = m.revcomp(read)
        rows[r, :len(read)], rl[r] = read, len(read)
        truth.append((p, p + L, strand))
    return rows, rl, truth


def random_reads(seed=RANDOM_SEED):
    import chain_class_model as ccm
    rng = np.random.default_rng(seed)
    rows = np.zeros((N_RANDOM, ccm.CHIMERIC_SIZE), dtype=np.uint8)
    rows[:, :RANDOM_LEN] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(N_RANDOM, RANDOM_LEN))]
    return rows, np.full(N_RANDOM, RANDOM_LEN, dtype=np.int32)


def batch():
    """dict(ref, rows, read_len, halves (of the chimeric reads), truth (of the unbroken reads)); reads [0, 32) are chimeric, [32, 65)
    unbroken, [65, 73) random."""
    if "batch" not in _CACHE:
        from test_seed_chain_gpu import reference
        from test_split_gpu import chimeric_expected
        ref = reference()
        c_rows, c_rl, halves = chimeric_expected()[:3]
        u_rows, u_rl, truth = unbroken_reads(ref)
        r_rows, r_rl = random_reads()
        _CACHE["batch"] = dict(ref=ref, rows=np.ascontiguousarray(np.concatenate([c_rows, u_rows, r_rows])),
                               read_len=np.concatenate([c_rl, u_rl, r_rl]).astype(np.int32), halves=halves, truth=truth)
    return _CACHE["batch"]


def mapper_params(max_reads, extend, slots=1, cigar_cap=None, md_cap=None):
    import chain_class_model as ccm
    from aim_amd import engine
    k, stride, w, max_occ, band, flank, min_votes, K = ccm.CHIMERIC_ROW
    sp = engine.seed_params(k, ccm.CHIMERIC_SIZE, stride=stride, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, max_cands=K, w=w)
    return engine.mapper_params(sp, max_reads, max_score(), mismatch=X, gap_o=O, gap_e=E, extend=engine.extend_params(*EXTEND) if extend else None,
                                slots=slots, cigar_cap=cigar_cap, md_cap=md_cap)


def canon(out):
    """A mapper result (or the hand-driven one) in a form two runs can be compared in: the records with cigar_offset / md_offset
    zeroed, the rec_offsets, and per record the CIGAR words and MD bytes the offsets address."""
    rec = np.array(out["records"], copy=True)
    words = [out["cigar"][int(s["cigar_offset"]):int(s["cigar_offset"]) + int(s["n_cigar"])].tolist() for s in rec["sam"]]
    md = [bytes(np.asarray(out["md"][int(s["md_offset"]):int(s["md_offset"]) + int(s["md_len"])], dtype=np.uint8).tobytes()) for s in rec["sam"]]
    rec["sam"]["cigar_offset"] = 0
    rec["sam"]["md_offset"] = 0
    return rec.tobytes(), np.asarray(out["rec_offsets"], dtype=np.uint32).tobytes(), words, md
