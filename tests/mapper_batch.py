"""The batch the mapper tests share, over seed_model's reference at read_size 1 024 with CHIMERIC_ROW's seed parameters: the 32 chimeric
reads of pipeline_batches.chimeric_expected(), 33 unbroken reads cut from the same reference with a few edits, and 8 random reads that the
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
        from pipeline_batches import chimeric_expected, reference
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


def map_alone(mp, ref, rl, rows):
    """One batch through a mapper of its own: the result detached from the slot's pinned buffers."""
    from aim_amd import engine
    from gpu_buffers import copy_out
    with engine.Mapper(mp, ref) as m:
        m.submit(0, rl, rows)
        return copy_out(m.wait(0))


def canon(out):
    """A mapper result (or the hand-driven one) in a form two runs can be compared in: the records with cigar_offset / md_offset
    zeroed, the rec_offsets, and per record the CIGAR words and MD bytes the offsets address."""
    rec = np.array(out["records"], copy=True)
    words = [out["cigar"][int(s["cigar_offset"]):int(s["cigar_offset"]) + int(s["n_cigar"])].tolist() for s in rec["sam"]]
    md = [bytes(np.asarray(out["md"][int(s["md_offset"]):int(s["md_offset"]) + int(s["md_len"])], dtype=np.uint8).tobytes()) for s in rec["sam"]]
    rec["sam"]["cigar_offset"] = 0
    rec["sam"]["md_offset"] = 0
    return rec.tobytes(), np.asarray(out["rec_offsets"], dtype=np.uint32).tobytes(), words, md


# ---- what the CPU tests of the mapper family share --------------------------------------------------------------------------------
def params_with(**kw):
    """aim_mapper_params_t that every check accepts, then the overrides: seed_<field>, ext_<field> or a field of the struct itself."""
    from aim_amd import engine
    sp = engine.seed_params(11, 1024, max_occ=8, band=96, flank=16, min_votes=2, max_cands=4, w=10)
    mp = engine.mapper_params(sp, 64, 76, extend=engine.extend_params(), slots=2)
    for name, v in kw.items():
        if name.startswith("seed_"):
            setattr(mp.seed, name[5:], v)
        elif name.startswith("ext_"):
            setattr(mp.extend, name[4:], v)
        else:
            setattr(mp, name, v)
    return mp


REFUSALS = [
    (dict(seed_k=15), "k 15 is outside 8..14"),
    (dict(seed_options=0), "options 0x0 must be AIM_SEED_OPT_MINIMIZERS(w)"),
    (dict(seed_options=(10 << 8) | 1), "unknown options"),
    (dict(seed_stride=2), "stride 2 must be 1 with AIM_SEED_OPT_MINIMIZERS"),
    (dict(seed_max_occ=0), "max_occ 0 must be >= 1"),
    (dict(seed_band=4097), "band 4097 is above 4096"),
    (dict(seed_flank=-1), "flank -1 must be >= 0"),
    (dict(seed_min_votes=0), "min_votes 0 must be >= 1"),
    (dict(seed_max_cands=17), "max_cands 17 is outside 1..16"),
    (dict(seed_read_size=4104), "read_size 4104 must be a positive multiple of 8, at most 4096 (aim_seed_chain_device)"),
    (dict(seed_read_size=1020), "read_size 1020 must be a positive multiple of 8"),
    (dict(max_hits=1000), "max_hits 1000 must be a power of two in 1024..8192"),
    (dict(max_hits=1024, seed_read_size=65536), "at most 65528 (aim_seed_chain_long_device)"),
    (dict(max_hits=1024, seed_options=0), "takes minimizer seeds only"),
    (dict(mask_q8=0), "mask_q8 0 is outside 1..256"),
    (dict(mask_q8=257), "mask_q8 257 is outside 1..256"),
    (dict(max_reads=1 << 30), "n_reads 1073741824 * max_cands 4 does not fit 32 bits"),
    (dict(ext_match=0), "match 0 must be >= 1"),
    (dict(ext_band=32), "band 32 is outside 1..31"),
    (dict(ext_max_ext=7), "max_ext 7 is outside 8..1024"),
    (dict(ext_max_cost=4096), "max_cost 4096 is outside 1..4095"),
    (dict(ext_mismatch=40), "is above 64"),
    (dict(gap_o=0), "penalties must be"),
    (dict(match=1), "penalties must be"),
    (dict(gap_e=4), "AIM_FLAG_ENDSFREE needs gap_o + gap_e <= 11 * mismatch and gap_e <= mismatch"),
    (dict(gap_o=40), "AIM_FLAG_ENDSFREE needs gap_o + gap_e <= 11 * mismatch"),
    (dict(max_score=-1), "max_score must be >= 0"),
    (dict(sam_options=2), "unknown sam_options 0x2"),
    (dict(max_reads=1 << 18), "max_reads * K * (4 * read_size + 10) must stay below 2^32"),
    (dict(options=2), "unknown options 0x2"),
    (dict(max_reads=0), "max_reads must be >= 1"),
    (dict(slots=0), "slots 0 is outside 1..4"),
    (dict(slots=5), "slots 5 is outside 1..4"),
]


def record(read, rank, n, flags, pos, mapq, nm, score, words, md, cigar, mdbuf, status=0):
    from aim_amd import capi
    rec = np.zeros(1, dtype=capi.MAP_RECORD_DTYPE)[0]
    rec["read"], rec["rank"], rec["n_records"], rec["mapq"] = read, rank, n, mapq
    s = rec["sam"]
    s["flags"], s["pos"], s["nm"], s["score"], s["status"] = flags, pos, nm, score, status
    s["cigar_offset"], s["n_cigar"], s["md_offset"], s["md_len"] = len(cigar), len(words), len(mdbuf), len(md)
    cigar.extend(words)
    mdbuf.extend(md.encode())
    return rec
