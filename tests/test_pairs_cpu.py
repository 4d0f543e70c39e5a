"""Rule 14c without a GPU: the struct sizes and the feature bit, every refusal of the three stateless entry points and of
aim_mapper_pairing_device_bytes / aim_mapper_set_pairing by message (each condition alone, none of them needs a device), properties of
the numpy model on synthetic slot tables, and the code objects of the three new kernels."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aim_hip.h")


def _lib():
    from aim_amd import capi
    return capi.load()


def _err():
    return _lib().aim_last_error().decode()


def _define(name):
    m = re.search(r"#define\s+%s\s+(\S+)" % name, open(HEADER).read())
    return int(m.group(1).rstrip("uUlL"), 0)


def test_feature_bit_and_layouts():
    import pair_model as pm
    from aim_amd import capi, engine
    assert _define("AIM_FEATURE_PAIRED") == capi.FEATURE_PAIRED == 0x200000 and engine.features() & capi.FEATURE_PAIRED
    assert _lib().aim_abi_version() == 2
    assert capi.MAP_PAIR_DTYPE == pm.PAIR_DTYPE and capi.MAP_MATE_DTYPE == pm.MATE_DTYPE and capi.MAP_PAIR_DTYPE.itemsize == 32 and capi.MAP_MATE_DTYPE.itemsize == 16
    assert C.sizeof(capi.MapPairParams) == 40 and capi.MapPairParams.rescue_size.offset == 24 and capi.MapPairParams.options.offset == 20
    assert pm.PAIR_DTYPE.fields["span"][1] == 24 and pm.MATE_DTYPE.fields["tlen"][1] == 8
    assert (_define("AIM_PAIR_RESCUE"), _define("AIM_PAIR_PROPER"), _define("AIM_PAIR_RESCUE_TRIED_A"), _define("AIM_PAIR_RESCUE_TRIED_B"), _define("AIM_PAIR_RESCUED_A"),
            _define("AIM_PAIR_RESCUED_B")) == (capi.PAIR_RESCUE, capi.PAIR_PROPER, capi.PAIR_RESCUE_TRIED_A, capi.PAIR_RESCUE_TRIED_B, capi.PAIR_RESCUED_A,
                                               capi.PAIR_RESCUED_B) == (pm.RESCUE, pm.PROPER, pm.TRIED_A, pm.TRIED_B, pm.RESCUED_A, pm.RESCUED_B)
    assert _lib().aim_pair_kernel_names() == b"pair_rescue_rows_kernel,pair_select_kernel,map_mates_kernel"
    # the structs the issue leaves alone
    assert C.sizeof(capi.MapperParams) == 124 and C.sizeof(capi.MapperOut) == 56 and capi.MAP_RECORD_DTYPE.itemsize == 64


OK = 1 << 12               # any aligned address: nothing is dereferenced before the device probe


def _pp(**kw):
    from aim_amd import engine
    args = dict(min_span=300, max_span=500, unpaired_penalty=17, rescue=True, rescue_size=512)
    opts = kw.pop("options", None)
    args.update(kw)
    pp = engine.pair_params(**args)
    if opts is not None:
        pp.options = opts
    return pp


def _rows(pp=None, K=4, rs=104, ref_len=40000, nc=0, st=None, ln=None, n=8, rl=OK, reads=OK, seg=OK, sam=OK, contig=None, req=OK, tp=OK, pat=OK, null_pp=False):
    pp = pp or _pp()
    return _lib().aim_pair_rescue_rows_device(None if null_pp else C.byref(pp), K, rs, ref_len, nc, st, ln, n, rl, reads, seg, sam, contig, req, tp, pat, None)


def _select(pp=None, K=4, rs=104, n=8, rl=OK, seg=OK, sam=OK, cls=OK, contig=None, res=OK, pairs=OK, null_pp=False):
    pp = pp or _pp()
    return _lib().aim_pair_select_device(None if null_pp else C.byref(pp), K, rs, n, rl, seg, sam, cls, contig, res, 0, 0, pairs, None)


def _mates(K=4, n=8, pairs=OK, seg=OK, sam=OK, contig=None, nc=0, st=None, off=OK, rec=OK, mates=OK):
    return _lib().aim_map_mates_device(K, n, pairs, seg, sam, contig, nc, st, off, rec, mates, None)


SHARED = [  # refusals of aim_map_pair_params_t and the batch's shape: the same from the two entry points that take the struct
    (dict(null_pp=True), "aim_map_pair_params_t is NULL"),
    (dict(pp=dict(options=3)), "unknown options 0x3"),
    (dict(n=7), "n_reads 7 is odd"),
    (dict(K=0), "K 0 is outside 1..16"),
    (dict(K=17), "K 17 is outside 1..16"),
    (dict(K=16, n=1 << 28), "n_reads 268435456 * (K 16 + 1) does not fit 32 bits"),
    (dict(pp=dict(min_span=-1)), "0 <= min_span <= max_span < 2^62 (min_span -1"),
    (dict(pp=dict(max_span=299)), "0 <= min_span <= max_span < 2^62 (min_span 300, max_span 299)"),
    (dict(pp=dict(max_span=1 << 62, rescue_size=1 << 20)), "max_span < 2^62"),
    (dict(pp=dict(unpaired_penalty=-1)), "unpaired_penalty -1 must be >= 0"),
    (dict(rs=100), "read_size 100 must be a positive multiple of 8"),
    (dict(pp=dict(rescue_size=508)), "rescue_size 508 must be a multiple of 8"),
    (dict(pp=dict(rescue_size=96, max_span=300)), "rescue_size 96 is below read_size 104"),
    (dict(pp=dict(rescue_size=296)), "max_span 500 - min_span 300 + read_size 104 exceeds rescue_size 296"),
]


@pytest.mark.parametrize("case", SHARED, ids=lambda c: c[1][:28].replace(" ", "_"))
def test_shared_refusals_need_no_device(case):
    from aim_amd import capi
    kw, text = dict(case[0]), case[1]
    if "pp" in kw:
        kw["pp"] = _pp(**kw["pp"])
    for fn, call in (("aim_pair_rescue_rows_device", _rows), ("aim_pair_select_device", _select)):
        assert call(**kw) == capi.AIM_EINVAL and _err().startswith(fn + ": ") and text in _err(), (fn, kw, _err())


def test_entry_point_refusals_need_no_device():
    from aim_amd import capi
    E = capi.AIM_EINVAL
    for kw, text in ((dict(ref_len=0), "ref_len must be >= 1"), (dict(ref_len=0xFE000001), "ref_len 4261412865 is above"),
                     (dict(contig=OK, nc=0, st=OK, ln=OK), "n_contigs 0 is outside 1.."), (dict(contig=OK, nc=3, st=None, ln=OK), "without its contig table"),
                     (dict(contig=OK, nc=3, st=OK, ln=None), "without its contig table"), (dict(rl=None), "null device buffer"), (dict(reads=None), "null device buffer"),
                     (dict(seg=None), "null device buffer"), (dict(sam=None), "null device buffer"), (dict(req=None), "null device buffer"),
                     (dict(tp=None), "null device buffer"), (dict(pat=None), "null device buffer"), (dict(sam=OK + 8), "d_sam must be 16-byte aligned"),
                     (dict(req=OK + 8), "d_res_requests must be 16-byte aligned"), (dict(reads=OK + 4), "d_reads must be 8-byte aligned"),
                     (dict(pat=OK + 4), "d_res_patterns must be 8-byte aligned"), (dict(seg=OK + 4), "d_seg must be 8-byte aligned"),
                     (dict(tp=OK + 4), "d_res_text_pos must be 8-byte aligned")):
        assert _rows(**kw) == E and _err().startswith("aim_pair_rescue_rows_device: ") and text in _err(), (kw, _err())
    # without AIM_PAIR_RESCUE the rows entry point still wants its rescue_size; the choice does not read it and needs no d_res_sam
    off = _pp(rescue=False, rescue_size=0)
    assert _rows(pp=off) == E and "rescue_size 0 is below read_size 104" in _err()
    assert _select(pp=off, res=None, pairs=OK + 8) == E and "d_pairs must be 16-byte aligned" in _err()      # (the NULL d_res_sam passed)
    for kw, text in ((dict(rl=None), "null device buffer"), (dict(seg=None), "null device buffer"), (dict(sam=None), "null device buffer"),
                     (dict(cls=None), "null device buffer"), (dict(pairs=None), "null device buffer"), (dict(res=None), "null device buffer"),
                     (dict(sam=OK + 8), "d_sam must be 16-byte aligned"), (dict(res=OK + 8), "d_res_sam must be 16-byte aligned"),
                     (dict(pairs=OK + 8), "d_pairs must be 16-byte aligned"), (dict(seg=OK + 4), "d_seg must be 8-byte aligned"),
                     (dict(cls=OK + 4), "d_class must be 8-byte aligned")):
        assert _select(**kw) == E and _err().startswith("aim_pair_select_device: ") and text in _err(), (kw, _err())
    for kw, text in ((dict(n=7), "n_reads 7 is odd"), (dict(K=0), "K 0 is outside 1..16"), (dict(K=17), "K 17 is outside 1..16"),
                     (dict(K=16, n=1 << 28), "(K 16 + 1) does not fit 32 bits"), (dict(contig=OK, nc=0, st=OK), "n_contigs 0 is outside 1.."),
                     (dict(contig=OK, nc=2, st=None), "without its contig table"), (dict(pairs=None), "null device buffer"), (dict(seg=None), "null device buffer"),
                     (dict(sam=None), "null device buffer"), (dict(off=None), "null device buffer"), (dict(rec=None), "null device buffer"),
                     (dict(mates=None), "null device buffer"), (dict(sam=OK + 8), "d_sam must be 16-byte aligned"), (dict(pairs=OK + 8), "d_pairs must be 16-byte aligned"),
                     (dict(rec=OK + 8), "d_records must be 16-byte aligned"), (dict(mates=OK + 8), "d_mates must be 16-byte aligned"),
                     (dict(seg=OK + 4), "d_seg must be 8-byte aligned")):
        assert _mates(**kw) == E and _err().startswith("aim_map_mates_device: ") and text in _err(), (kw, _err())


def _mapper_params(**kw):
    from aim_amd import engine
    sp = engine.seed_params(11, 104, max_occ=8, band=96, flank=16, min_votes=2, max_cands=4, w=5)
    mp = engine.mapper_params(sp, 64, 40, slots=2)
    for name, v in kw.items():
        setattr(mp, name, v)
    return mp


def test_mapper_pairing_refusals_and_bytes():
    """aim_mapper_pairing_device_bytes answers without a device; aim_mapper_set_pairing, aim_mapper_pairs and their NULL arguments."""
    from aim_amd import capi, engine
    lib = _lib()
    b = C.c_uint64(0)
    mp = _mapper_params()
    fn = "aim_mapper_pairing_device_bytes: "
    for pp, text in ((_pp(options=2), "unknown options 0x2"), (_pp(min_span=-5), "0 <= min_span"), (_pp(rescue_size=100), "rescue_size 100 must be a multiple of 8"),
                     (_pp(rescue_size=104, max_span=300), None), (_pp(rescue_size=296), "exceeds rescue_size 296"),
                     (_pp(rescue_cigar_cap=0xFFFFFFFF), "cigar_cap + rescue_cigar_cap"), (_pp(rescue_md_cap=0xFFFFFFFF), "md_cap + rescue_md_cap")):
        rc = lib.aim_mapper_pairing_device_bytes(C.byref(mp), C.byref(pp), C.byref(b))
        assert (rc == 0 and b.value > 0) if text is None else (rc == capi.AIM_EINVAL and _err().startswith(fn) and text in _err()), (text, _err())
    assert lib.aim_mapper_pairing_device_bytes(None, C.byref(_pp()), C.byref(b)) == capi.AIM_EINVAL and _err() == fn + "params is NULL"
    assert lib.aim_mapper_pairing_device_bytes(C.byref(mp), None, C.byref(b)) == capi.AIM_EINVAL and "aim_map_pair_params_t is NULL" in _err()
    assert lib.aim_mapper_pairing_device_bytes(C.byref(mp), C.byref(_pp()), None) == capi.AIM_EINVAL and _err() == fn + "bytes is NULL"
    assert lib.aim_mapper_pairing_device_bytes(C.byref(_mapper_params(slots=9)), C.byref(_pp()), C.byref(b)) == capi.AIM_EINVAL and "slots 9 is outside" in _err()
    with_rescue = engine.mapper_pairing_device_bytes(mp, _pp(rescue_cigar_cap=4096, rescue_md_cap=8192))
    without = engine.mapper_pairing_device_bytes(mp, _pp(rescue=False, rescue_size=0))
    assert 0 < without < with_rescue and engine.mapper_pairing_device_bytes(_mapper_params(slots=1), _pp()) * 2 == engine.mapper_pairing_device_bytes(mp, _pp())
    assert with_rescue >= 2 * (4 * 4096 + 8192 + 64 * (2 * 512 + 512))      # the regions and the rescue rows of both slots at least
    assert lib.aim_mapper_set_pairing(None, C.byref(_pp())) == capi.AIM_EINVAL and _err() == "aim_mapper_set_pairing: mapper is NULL"
    assert lib.aim_mapper_pairs(None, 0, None) == capi.AIM_EINVAL and _err() == "aim_mapper_pairs: mapper is NULL"


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def _run_model(K, n, contigs, t=None, pp=None):
    import pair_model as pm
    t = t or pm.synthetic_tables(5, K, n, contigs)
    pp = pp or pm.params()
    rows = pm.rescue_rows(pp, K, pm.READ_SIZE, t["ref_len"], n, t["read_len"], t["reads"], t["seg"], t["sam"], t["contig"], t["starts"], t["lens"])
    sel = pm.select(pp, K, pm.READ_SIZE, n, t["read_len"], t["seg"], t["sam"], t["cls"], t["contig"], t["res_sam"], 1000, 2000)
    return t, rows, sel


@pytest.mark.parametrize("contigs", (False, True), ids=("one-seq", "contigs"))
@pytest.mark.parametrize("K", (1, 4, 16))
def test_model_properties(K, contigs):
    import map_records_model as mm
    import pair_model as pm
    n = 300
    t, (req, tpos, rows), (pairs, seg, sam, cls, contig) = _run_model(K, n, contigs)
    mapped0 = mm.mapped_slots(K, n, t["seg"], t["sam"])
    f = pairs["flags"]
    # the fixed cases of synthetic_tables
    assert f[0] == 0 and pairs["slot"][0].tolist() == [pm.NONE, pm.NONE] and pairs["score_sum"][0] == pm.INT_MAX
    assert f[1] == pm.PROPER | pm.TRIED_B | pm.RESCUED_B and pairs["slot"][1].tolist() == [2 * K, 3 * K + K] and pairs["span"][1] == 350
    assert (pairs["span"][3], pairs["span"][4]) == (pm.MIN_SPAN, pm.MAX_SPAN) and f[3] == f[4] == pm.PROPER
    assert f[5] == pm.PROPER | pm.TRIED_A | pm.TRIED_B | pm.RESCUED_B                 # read 10's rescue row came back unmapped, read 11's is proper
    assert f[6] == pm.PROPER | pm.TRIED_A | pm.TRIED_B | pm.RESCUED_B and pairs["n_best"][6] == 2 and pairs["second_sum"][6] == pairs["score_sum"][6]
    assert f[11] == pm.TRIED_A | pm.TRIED_B and pairs["span"][11] == 0
    assert bool(f[12] & pm.PROPER) == (not contigs)                                   # never proper across contigs
    if K > 1:
        assert f[2] == pm.PROPER and pairs["n_best"][2] == 4 and pairs["slot"][2].tolist() == [4 * K, 5 * K] and pairs["second_sum"][2] == pairs["score_sum"][2]
        assert f[7] == 0 and pairs["score_sum"][7] == 17 and pairs["second_sum"][7] == 60 and pairs["slot"][7].tolist() == [14 * K, 15 * K]
    assert not (f[12] & pm.TRIED_A) and t["read_len"][24] == 0                        # a read of length 0 is not rescued
    # windows: inside the contig (the reference), at most rescue_size, at least the read; cut on either side somewhere
    cut_lo = cut_hi = empty = 0
    for b in range(n):
        L, tl = int(req["pattern_len"][b]), int(req["text_len"][b])
        assert req["idx"][b] == b and req["padding"][b] == 0
        if not L:
            assert tl == 0 and tpos[b] == 0 and b not in rows
            empty += 1
            continue
        lo = int(tpos[b]) & ~pm.MINUS_STRAND
        a = b ^ 1
        rep = a * K + int(np.nonzero(mapped0[a])[0][0])
        c = int(t["contig"][rep]) if contigs else 0
        c_lo, c_hi = (int(t["starts"][c]), int(t["starts"][c]) + int(t["lens"][c])) if contigs else (0, t["ref_len"])
        assert L <= tl <= pm.RESCUE_SIZE and c_lo <= lo and lo + tl <= c_hi and L == min(max(int(t["read_len"][b]), 0), pm.READ_SIZE)
        assert bool(int(tpos[b]) & pm.MINUS_STRAND) == (not t["sam"]["flags"][rep] & pm.SAM_REVERSE)   # the mate is looked for on the other strand
        cut_lo += lo == c_lo
        cut_hi += lo + tl == c_hi
    assert cut_lo >= 1 and cut_hi >= 1 and empty >= 1, (cut_lo, cut_hi, empty)
    # apply: exactly one non-supplementary line per mapped read, a rescued read has exactly one record, in slot 0
    off, rec = mm.map_records(K, n, seg, sam, cls)
    mapped1 = mm.mapped_slots(K, n, seg, sam)
    for r in range(n):
        g = rec[off[r]:off[r + 1]]
        assert ((g["sam"]["flags"] & (mm.SAM_SUPPLEMENTARY | mm.SAM_UNMAPPED)) == 0).sum() == (1 if mapped1[r].any() else 0)
        if f[r >> 1] & (pm.RESCUED_B if r & 1 else pm.RESCUED_A):
            assert len(g) == 1 and g["slot"][0] == r * K and mapped1[r].tolist() == [True] + [False] * (K - 1)
            assert g["sam"]["cigar_offset"][0] == t["res_sam"]["cigar_offset"][r] + 1000 and g["sam"]["md_offset"][0] == t["res_sam"]["md_offset"][r] + 2000
            assert cls["mapq"][r * K] == t["cls"]["mapq"][(r ^ 1) * K + int(np.nonzero(mapped0[r ^ 1])[0][0])]
        else:
            assert mapped1[r].tolist() == mapped0[r].tolist() and seg[r * K:(r + 1) * K].tobytes() == t["seg"][r * K:(r + 1) * K].tobytes()
    # the mate fields: tlen signs and the flag bits
    rec2, mt = pm.mates(K, n, pairs, seg, sam, contig, t["starts"], off, rec)
    fl = rec2["sam"]["flags"].astype(np.int64)
    assert (fl & 0x1).all() and (((fl & 0x40) != 0) == (rec2["read"] % 2 == 0)).all() and (((fl & 0x80) != 0) == (rec2["read"] % 2 == 1)).all()
    assert ((rec2["sam"]["flags"] ^ rec["sam"]["flags"]) & ~np.uint16(0xEB) == 0).all()
    for m in range(n // 2):
        g = np.arange(off[2 * m], off[2 * m + 2])
        chosen = g[(fl[g] & 0x2) != 0]
        if f[m] & pm.PROPER:
            assert len(chosen) == 2 and sorted(mt["tlen"][chosen].tolist()) == [-pairs["span"][m], pairs["span"][m]]
            assert all((mt["tlen"][i] < 0) == bool(fl[i] & 0x10) for i in chosen) and (mt["tlen"][np.setdiff1d(g, chosen)] == 0).all()
            assert rec2["read"][chosen].tolist() == [2 * m, 2 * m + 1]
        else:
            assert len(chosen) == 0 and (mt["tlen"][g] == 0).all()
    both_unmapped = [t_ for t_ in range(len(rec2)) if fl[t_] & 0x4 and fl[t_] & 0x8]
    assert both_unmapped and all(mt["mate_pos"][i] == 0 and mt["mate_contig"][i] == (pm.CONTIG_NONE if contigs else 0) for i in both_unmapped)


@pytest.mark.parametrize("K", (4, 16))
def test_choice_is_invariant_under_permuting_lanes_and_subsets(K):
    """What a read pair's lanes do: each holds the result of a subset of the combinations, and the parts are combined pairwise. Any
    order of the combinations and any split into subsets gives the answer of the rule's own statement (best_of): the chosen (i, j), the
    cost, the count of ties, the runner-up and the span."""
    import functools
    import map_records_model as mm
    import pair_model as pm
    n = 200
    t = pm.synthetic_tables(5, K, n, True)
    pp = pm.params()
    mapped = mm.mapped_slots(K, n, t["seg"], t["sam"])
    rng = np.random.default_rng(9)
    seen = ties = 0
    for m in range(n // 2):
        ca, cb = pm.read_cands(K, 2 * m, mapped, t["sam"], t["contig"]), pm.read_cands(K, 2 * m + 1, mapped, t["sam"], t["contig"])
        for x in list(ca.values()) + list(cb.values()):        # many proper combinations: one contig, and every candidate near its mate's
            x["contig"] = 0
        for j, y in cb.items():
            y["rev"], y["pos"] = True, 5000 + 10 * j
        for i, x in ca.items():
            x["rev"], x["pos"] = False, 5000 + 400 + 10 * i - 100 - pm.MAX_SPAN + 150
        ca[K] = dict(pm.cand(t["res_sam"][2 * m], 0), rev=False, pos=4700)
        cb[K] = dict(pm.cand(t["res_sam"][2 * m + 1], 0), rev=True, pos=5050)
        want = pm.best_of(pp, ca, cb, K)
        combos = pm.proper_combos(pp, ca, cb, K)
        assert (want is None) == (not combos) and not any(c[1] == K and c[2] == K for c in combos)
        if not combos:
            continue
        seen += 1
        ties += want[3] > 1
        for _ in range(4):
            order = [combos[i] for i in rng.permutation(len(combos))]
            assert functools.reduce(pm.combine, order, None) == want                      # one lane sees them all, in any order
            cuts = sorted(rng.integers(0, len(order) + 1, size=3).tolist())
            parts = [functools.reduce(pm.combine, order[a:b], None) for a, b in zip([0] + cuts, cuts + [len(order)])]   # four lanes, some of them empty
            assert pm.combine(pm.combine(parts[0], parts[1]), pm.combine(parts[2], parts[3])) == want
            assert pm.combine(pm.combine(parts[3], parts[0]), pm.combine(parts[1], parts[2])) == want
    assert seen > 50 and ties > 5, (seen, ties)


def test_pair_kernels_code_objects():
    """Each new kernel exists exactly once, uses no scratch and no static LDS and stays within kPairMaxVgpr: the bound of the map kernels."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_regs
    lib = os.path.join(ROOT, "aim_amd", "libaim_hip.so")
    if not os.path.exists(lib):
        pytest.fail("libaim_hip.so is missing: run the build")
    regs = codeobj_regs.kernel_regs(lib)
    src = lambda f: open(os.path.join(ROOT, "aim_amd", "csrc", f)).read()
    bound = int(re.search(r"constexpr int kPairMaxVgpr = (\d+);", src("pair.hpp")).group(1))
    assert bound == int(re.search(r"constexpr int kMapMaxVgpr = (\d+);", src("mapper.hpp")).group(1))
    for name in _lib().aim_pair_kernel_names().decode().split(","):
        found = [n for n in regs if re.search(r"\baim::%s\(" % name, n)]
        assert len(found) == 1, (name, found)
        r = regs[found[0]]
        print(name, r)
        assert r["scratch_bytes"] == 0 and r["lds_static_bytes"] == 0 and 0 < r["vgpr"] + r["agpr"] <= bound <= 512 // 8, (name, r, bound)


# ---- the premises of the shared paired batch -------------------------------------------------------------------------------------------
def _batch_chains():
    import chain_class_model as ccm
    import chain_model as cm
    import minimizer_model as mnm
    import pair_batch as pb
    b = pb.batch()
    ref = pb.reference()
    req, tpos, votes, seeds, chains = cm.seed_chain(b["rows"], b["read_len"], mnm.build_index(ref, pb.K_MER, pb.W), len(ref), pb.K_MER, 1, pb.W, pb.MAX_OCC, pb.BAND,
                                                    pb.FLANK, pb.MIN_VOTES, pb.K, pb.READ_SIZE)
    cls = ccm.classify(pb.K, pb.READ_SIZE, 128, b["read_len"], tpos, seeds, chains)
    return b, req, tpos, seeds, chains, cls


def test_batch_premises_on_the_chain_model():
    """What makes the GPU expectations exact: an exact mate has a chain at its true place; a substituted mate and a random read have no
    chain at all; in class c the repeat's far copy is mate 2's candidate 0 and the near copy a secondary, which is never aligned."""
    import chain_class_model as ccm
    import pair_batch as pb
    b, req, tpos, seeds, chains, cls = _batch_chains()
    K = pb.K
    assert len(b["truth"]) == pb.N_PAIRS == 56 and b["rows"].shape == (112, pb.READ_SIZE)
    for m, t in enumerate(b["truth"]):
        for x in range(2):
            r, tm = 2 * m + x, t["mates"][x]
            n = int(seeds["n_cands"][r])
            substituted = x == 1 and (t["cls"] == "b" or (t["cls"] == "g" and t["q"] < 4))
            if tm is None or substituted:
                assert n == 0, (m, x, t["cls"], n)
                continue
            assert n >= 1, (m, x, t["cls"])
            starts = [int(tpos[r * K + i]) & ~(1 << 63) for i in range(n)]
            if t["cls"] == "c" and x == 1:
                assert n >= 2 and abs(starts[0] - (tm[0] - pb.REPEAT_B + pb.REPEAT_A)) <= pb.FLANK + pb.BAND and abs(starts[1] - tm[0]) <= pb.FLANK + pb.BAND, (m, starts, tm)
                assert cls["flags"][r * K] & ccm.PRIMARY and cls["flags"][r * K + 1] == ccm.SECONDARY
            else:
                assert abs(starts[0] - tm[0]) <= pb.FLANK + pb.BAND and (int(tpos[r * K]) >> 63) == tm[2], (m, x, t["cls"], starts, tm)


def test_batch_premises_on_the_ends_free_model():
    """The rescue rows of rule 14c over the true placements, scored by the ends-free DP model: at most MAX_SCORE at the true window of
    classes b, c and the clipped half of g, above it for every window tried in d, e and f (where none is tried)."""
    import endsfree_model as efm
    import pair_batch as pb
    import pair_model as pm
    b = pb.batch()
    ref = pb.reference()
    n, K = 2 * pb.N_PAIRS, 1
    seg, sam = np.zeros(n, dtype=pm.SEG_DTYPE), np.zeros(n, dtype=pm.SAM_DTYPE)
    contig = np.zeros(n, dtype=np.uint32)
    lens = np.diff(np.array((0,) + pb.CUTS + (pb.REF_LEN,))).astype(np.uint32)
    starts = np.array((0,) + pb.CUTS, dtype=np.uint32)
    for m, t in enumerate(b["truth"]):
        for x in range(2):
            r, tm = 2 * m + x, t["mates"][x]
            far = t["cls"] == "c" and x == 1                       # mapped to the repeat's far copy, as the chain model says
            lost = tm is None or (x == 1 and (t["cls"] == "b" or (t["cls"] == "g" and t["q"] < 4)))
            sam["flags"][r] = pm.SAM_UNMAPPED
            if not lost:
                lo = tm[0] - pb.REPEAT_B + pb.REPEAT_A if far else tm[0]
                seg["flags"][r], sam["pos"][r], sam["ref_span"][r], sam["flags"][r] = pm.SEG_VALID, lo, pb.L, pm.SAM_REVERSE if tm[2] else 0
                contig[r] = pb.contig_of(lo)[0]
    pp = pm.Params(pb.MIN_SPAN, pb.MAX_SPAN, pb.UNPAIRED_PENALTY, pm.RESCUE, pb.RESCUE_SIZE)
    for cut in (False, True):                                      # one sequence; three contigs laid end to end (no spacer: the model's layout is the test's)
        req, tpos, rows = pm.rescue_rows(pp, K, pb.READ_SIZE, len(ref), n, b["read_len"], b["rows"], seg, sam, contig if cut else None, starts, lens)
        tried = [r for r in range(n) if req["pattern_len"][r]]
        txt = np.zeros((len(tried), pb.RESCUE_SIZE), dtype=np.uint8)
        for i, r in enumerate(tried):
            lo, tl = int(tpos[r]) & ~pm.MINUS_STRAND, int(req["text_len"][r])
            w = ref[lo:lo + tl]
            txt[i, :tl] = pb.revcomp(w) if int(tpos[r]) >> 63 else w
        pat = np.zeros((len(tried), pb.RESCUE_SIZE), dtype=np.uint8)
        pat[:, :pb.READ_SIZE] = b["rows"][tried]
        score = dict(zip(tried, efm.dp_scores(req[tried], pat, txt, pb.X, pb.O, pb.E, ends_free=(0, 0, pb.RESCUE_SIZE, pb.RESCUE_SIZE)).tolist()))
        seen = {c: 0 for c in pb.CLASSES}
        for m, t in enumerate(b["truth"]):
            c, q = t["cls"], t["q"]
            got = {r: score[r] for r in (2 * m, 2 * m + 1) if r in score}
            seen[c] += len(got)
            if c == "a" or (c == "g" and q >= 4 and not cut):
                assert not got, (m, c)                             # proper as mapped: no rescue
            elif c == "b" or (c == "g" and q < 4):
                assert got == {2 * m + 1: 10 * pb.X}, (m, c, got)  # the ten substitutions and nothing else, also in the clipped window
            elif c == "c":
                assert set(got) == {2 * m, 2 * m + 1} and got[2 * m + 1] == 0 and got[2 * m] > pb.MAX_SCORE, (m, got)
            elif c in "de":
                assert len(got) == (2 if c == "d" else 1) and min(got.values()) > pb.MAX_SCORE, (m, c, got)
            elif c == "f":
                assert not got
            else:                                                  # g across the cut, three contigs: the windows are cut away or hold no mate
                assert all(v > pb.MAX_SCORE for v in got.values()), (m, got)
        assert seen["b"] == 8 and seen["c"] == 16 and seen["d"] == 16 and seen["e"] == 8 and seen["g"] >= 4, seen


# ---- samout and the command line's readers -----------------------------------------------------------------------------------------
def test_samout_paired_whole_text():
    """A proper pair on one contig, a pair on two contigs, a mapped read with an unmapped mate (written at its mate's place) and a
    pair of unmapped reads; the second read of the first pair has a supplementary record, whose line carries the same mate fields."""
    from aim_amd import capi, samout
    from mapper_batch import record as _record
    w = lambda n, op: (n << 4) | op
    cigar, md = [], []
    recs = [_record(0, 0, 1, 0x1 | 0x2 | 0x20 | 0x40, 99, 60, 0, 0, [w(8, 0)], "8", cigar, md),
            _record(1, 0, 2, 0x1 | 0x2 | 0x10 | 0x80, 391, 60, 1, 3, [w(6, 0), w(2, 4)], "2A3", cigar, md),
            _record(1, 1, 2, 0x1 | 0x10 | 0x80 | 0x800, 4999, 9, 0, 0, [w(6, 4), w(2, 0)], "2", cigar, md),
            _record(2, 0, 1, 0x1 | 0x40, 9, 30, 0, 0, [w(4, 0)], "4", cigar, md),
            _record(3, 0, 1, 0x1 | 0x10 | 0x20 | 0x80, 19, 31, 0, 0, [w(4, 0)], "4", cigar, md),
            _record(4, 0, 1, 0x1 | 0x8 | 0x10 | 0x40, 699, 22, 0, 0, [w(4, 0)], "4", cigar, md),
            _record(5, 0, 1, 0x1 | 0x4 | 0x20 | 0x80, 0, 0, 0, 5, [], "", cigar, md),
            _record(6, 0, 1, 0x1 | 0x4 | 0x8 | 0x40, 0, 0, 0, 0, [], "", cigar, md),
            _record(7, 0, 1, 0x1 | 0x4 | 0x8 | 0x80, 0, 0, 0, 0, [], "", cigar, md)]
    recs[3]["sam"]["pad"], recs[4]["sam"]["pad"], recs[5]["sam"]["pad"] = 0, 1, 1
    recs[3]["sam"]["flags"] |= 0x20
    mates = np.array([(391, 300, 0), (99, -300, 0), (99, 0, 0), (19, 0, 1), (9, 0, 0), (699, 0, 1), (699, 0, 1), (0, 0, 0xFFFFFFFF), (0, 0, 0xFFFFFFFF)],
                     dtype=capi.MAP_MATE_DTYPE)
    out = {"records": np.array(recs, dtype=capi.MAP_RECORD_DTYPE), "rec_offsets": np.array([0, 1, 3, 4, 5, 6, 7, 8, 9], dtype=np.uint32),
           "cigar": np.array(cigar, dtype=np.uint32), "md": np.frombuffer(bytes(md), dtype=np.uint8), "mates": mates}
    names = ["p", "p", "q", "q", "u", "u", "z", "z"]
    reads = [b"ACGTACGT", b"AACCGGTT", b"ACGT", b"GGCC", b"AAAA", b"CCCC", b"GG", b"TT"]
    lens = [8, 8, 4, 4, 4, 4, 2, 2]
    text = "".join(l + "\n" for l in samout.record_lines(out, names, reads, lens, ["c0", "c1"]))
    assert text == (
        "p\t99\tc0\t100\t60\t8M\t=\t392\t300\tACGTACGT\t*\tNM:i:0\tMD:Z:8\tAS:i:0\n"
        "p\t147\tc0\t392\t60\t6M2S\t=\t100\t-300\tAACCGGTT\t*\tNM:i:1\tMD:Z:2A3\tAS:i:-3\tSA:Z:c0,5000,-,6S2M,9,0;\n"
        "p\t2193\tc0\t5000\t9\t6S2M\t=\t100\t0\tAACCGGTT\t*\tNM:i:0\tMD:Z:2\tAS:i:0\tSA:Z:c0,392,-,6M2S,60,1;\n"
        "q\t97\tc0\t10\t30\t4M\tc1\t20\t0\tACGT\t*\tNM:i:0\tMD:Z:4\tAS:i:0\n"
        "q\t177\tc1\t20\t31\t4M\tc0\t10\t0\tGGCC\t*\tNM:i:0\tMD:Z:4\tAS:i:0\n"
        "u\t89\tc1\t700\t22\t4M\t=\t700\t0\tTTTT\t*\tNM:i:0\tMD:Z:4\tAS:i:0\n"
        "u\t165\tc1\t700\t0\t*\t=\t700\t0\tCCCC\t*\n"
        "z\t77\t*\t0\t0\t*\t*\t0\t0\tGG\t*\n"
        "z\t141\t*\t0\t0\t*\t*\t0\t0\tTT\t*\n")
    single = dict(out)
    del single["mates"]                                   # without the mate fields: the single-end text, FLAG as it stands
    assert samout.record_lines(single, names, reads, lens, ["c0", "c1"])[0].split("\t")[6:9] == ["*", "0", "0"]


def test_reads2_reader(tmp_path):
    from aim_amd import map as amap
    a = [("r1/1", b"ACGT", "IIII"), ("r2", b"GG", None)]
    b = [("r1/2", b"TTTT", "JJJJ"), ("r2", b"CC", None)]
    assert amap.pair_reads(a, b) == [("r1", b"ACGT", "IIII"), ("r1", b"TTTT", "JJJJ"), ("r2", b"GG", None), ("r2", b"CC", None)]
    assert amap.mate_name("x/1") == "x" and amap.mate_name("x/3") == "x/3" and amap.mate_name("/2") == ""
    with pytest.raises(ValueError, match="names differ: 'r2' and 'r3/2'"):
        amap.pair_reads(a, [b[0], ("r3/2", b"CC", None)])
    with pytest.raises(ValueError, match="holds 2 reads and --reads2 1"):
        amap.pair_reads(a, b[:1])
    fa = tmp_path / "ref.fa"
    fa.write_bytes(b">c\nACGTACGTACGTACGTACGT\n")
    f1, f2 = tmp_path / "a.fq", tmp_path / "b.fq"
    f1.write_bytes(b"@r/1\nACGT\n+\nIIII\n")
    f2.write_bytes(b"@s/2\nACGT\n+\nIIII\n")
    import subprocess
    run = lambda *more: subprocess.run([sys.executable, "-m", "aim_amd.map", "--ref", str(fa), "--reads", str(f1), "--reads2", str(f2), "-o", str(tmp_path / "o.sam")] +
                                       list(more), cwd=ROOT, capture_output=True, text=True, timeout=120)
    p = run()
    assert p.returncode == 2 and "names differ" in p.stderr and not (tmp_path / "o.sam").exists(), p.stderr
    f2.write_bytes(b"@r/2\nACGT\n+\nIIII\n")
    p = run("--batch", "7")
    assert p.returncode == 2 and "--batch 7 must be even" in p.stderr, p.stderr
