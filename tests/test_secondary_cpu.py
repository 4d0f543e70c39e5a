"""Rule 16c without a GPU: the feature bit, the struct layouts, the kernel names and every refusal by message (none needs a device); the
numpy model of the three parts on synthetic tables, its properties, and the same tables padded with empty slots; part 1's identity on
the chain model's own output; the MAPQ of a locus without secondaries against rule 12c's byte; the code objects of the four kernels;
aim_amd.samout on a hand-made result with the whole text compared; and the premises of the three read classes on the chain model."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from mapper_batch import params_with as _params, record as _record  # noqa: E402
HEADER = os.path.join(ROOT, "include", "aim_hip.h")
RS = 104


def _lib():
    from aim_amd import capi
    return capi.load()


def _err():
    return _lib().aim_last_error().decode()


def _define(name):
    m = re.search(r"#define\s+%s\s+(\S+)" % name, open(HEADER).read())
    return int(m.group(1).rstrip("uUlL"), 0)


def test_feature_bit_layouts_and_kernel_names():
    from aim_amd import capi, engine
    import secondary_model as sec
    assert _define("AIM_FEATURE_SECONDARY") == capi.FEATURE_SECONDARY == 0x800000 and engine.features() & capi.FEATURE_SECONDARY
    assert _define("AIM_SEC_MAX") == capi.SEC_MAX == sec.SEC_MAX == 15 and _define("AIM_SEC_RECORDS") == capi.SEC_RECORDS == sec.SEC_RECORDS
    assert _define("AIM_SAM_SECONDARY") == capi.SAM_SECONDARY == sec.SAM_SECONDARY == 0x100
    assert (_define("AIM_SEC_SWAPPED"), _define("AIM_SEC_COMPLETE")) == (capi.SEC_SWAPPED, capi.SEC_COMPLETE) == (sec.SWAPPED, sec.COMPLETE)
    assert capi.SEC_SLOT_DTYPE == sec.SEC_SLOT and capi.MAP_SEC_DTYPE == sec.MAP_SEC and sec.SEC_SLOT.itemsize == 8 and sec.MAP_SEC.itemsize == 16
    assert sec.SEC_SLOT.fields["gap"][1] == 6 and sec.MAP_SEC.fields["second_score"][1] == 4 and sec.MAP_SEC.fields["flags"][1] == 12
    assert _lib().aim_secondary_kernel_names() == b"secondary_rows_kernel,secondary_select_kernel,map_count_sec_kernel,map_records_sec_kernel"
    assert _lib().aim_abi_version() == 2
    p = engine.secondary_params(3, records=False)
    assert (p.max_sec, p.options) == (3, 0) and engine.secondary_params().options == capi.SEC_RECORDS


# ---- refusals --------------------------------------------------------------------------------------------------------------------
OK = 1 << 12           # any aligned address: nothing is dereferenced before the device probe


def test_secondary_rows_refusals_need_no_device():
    from aim_amd import capi
    lib = _lib()
    names = ("rl", "reads", "req", "tp", "seed", "chains", "cls", "sreq", "stp", "spat", "seg")

    def call(K=4, rs=1024, flank=16, ref_len=1 << 20, n=8, max_sec=2, **bufs):
        b = [bufs.get(x, OK) for x in names]
        return lib.aim_secondary_rows_device(K, rs, flank, ref_len, n, *b, max_sec, None)
    cases = [(dict(K=0), "K 0 is outside 1..16"), (dict(K=17), "K 17 is outside 1..16"), (dict(rs=0), "read_size 0 must be a positive multiple of 8"),
             (dict(rs=100), "read_size 100 must be a positive multiple of 8"), (dict(rs=65536), "at most 65528"),
             (dict(K=16, n=1 << 28), "n_reads 268435456 * K 16 does not fit 32 bits"), (dict(flank=-1), "flank -1 must be >= 0"),
             (dict(ref_len=0xFE000001), "ref_len 4261412865 is above"), (dict(max_sec=0), "max_sec 0 is outside 1..15"),
             (dict(max_sec=16), "max_sec 16 is outside 1..15"), (dict(max_sec=16, seg=None), "max_sec 16 is outside 1..15")]
    cases += [({x: None}, "null device buffer") for x in names]
    for kw, text in cases:
        assert call(**kw) == capi.AIM_EINVAL and _err().startswith("aim_secondary_rows_device: ") and text in _err(), (kw, _err())


def test_secondary_select_refusals_need_no_device():
    from aim_amd import capi
    lib = _lib()
    call = lambda K=4, n=8, seg=OK, sam=OK, cls=OK, chains=OK, ms=60, unit=3, sec=OK: lib.aim_secondary_select_device(K, n, seg, sam, cls, chains, ms, unit, sec, None)
    for kw, text in ((dict(K=0), "K 0 is outside 1..16"), (dict(K=17), "K 17 is outside 1..16"), (dict(K=16, n=1 << 28), "does not fit 32 bits"),
                     (dict(ms=-1), "max_score -1 is outside 0..2147483646"), (dict(ms=0x7FFFFFFF), "max_score 2147483647 is outside"),
                     (dict(unit=0), "score_unit 0 must be >= 1"), (dict(seg=None), "null device buffer"), (dict(sam=None), "null device buffer"),
                     (dict(cls=None), "null device buffer"), (dict(chains=None), "null device buffer"), (dict(sec=None), "null device buffer")):
        assert call(**kw) == capi.AIM_EINVAL and _err().startswith("aim_secondary_select_device: ") and text in _err(), (kw, _err())


def test_map_records_secondary_refusals_need_no_device():
    from aim_amd import capi
    lib = _lib()

    def call(K=4, n=8, opt=1, seg=OK, sam=OK, cls=OK, sec=OK, ct=None, nc=0, cs=None, off=OK, rec=OK, srec=OK, scr=OK, sb=8192):
        return lib.aim_map_records_secondary_device(K, n, opt, seg, sam, cls, sec, ct, nc, cs, off, rec, srec, scr, sb, None)
    for kw, text in ((dict(K=0), "K 0 is outside 1..16"), (dict(K=17), "K 17 is outside 1..16"), (dict(K=16, n=1 << 28), "does not fit 32 bits"),
                     (dict(off=None), "d_rec_offsets is NULL"), (dict(off=None, n=0), "d_rec_offsets is NULL"), (dict(opt=2), "unknown options 0x2"),
                     (dict(ct=OK, nc=0, cs=OK), "n_contigs 0 is outside 1..1048576"), (dict(ct=OK, nc=(1 << 20) + 1, cs=OK), "n_contigs 1048577 is outside"),
                     (dict(ct=OK, nc=3), "d_contig_start is NULL"), (dict(seg=None), "null device buffer"), (dict(sam=None), "null device buffer"),
                     (dict(cls=None), "null device buffer"), (dict(sec=None), "null device buffer"), (dict(rec=None), "null device buffer"),
                     (dict(srec=None), "null device buffer"), (dict(scr=None), "null device buffer"), (dict(sam=OK + 8), "must be 16-byte aligned"),
                     (dict(rec=OK + 4), "must be 16-byte aligned"), (dict(srec=OK + 8), "must be 16-byte aligned"), (dict(sb=8191), "scratch_bytes 8191 is below the 8192")):
        assert call(**kw) == capi.AIM_EINVAL and _err().startswith("aim_map_records_secondary_device: ") and text in _err(), (kw, _err())


def test_mapper_secondary_refusals_need_no_device():
    """The parameter refusals come before the mapper is looked at, so they need neither a mapper nor a device."""
    from aim_amd import capi, engine
    lib = _lib()
    mp, b = _params(), C.c_uint64(0)
    for fn, call in (("aim_mapper_secondary_device_bytes", lambda sc: lib.aim_mapper_secondary_device_bytes(C.byref(mp), sc, C.byref(b))),
                     ("aim_mapper_set_secondary", lambda sc: lib.aim_mapper_set_secondary(None, sc))):
        for sc, text in ((None, "params is NULL"), (capi.MapSecParams(0, 0), "max_sec 0 is outside 1..15"), (capi.MapSecParams(16, 1), "max_sec 16 is outside 1..15"),
                         (capi.MapSecParams(2, 2), "unknown options 0x2")):
            assert call(C.byref(sc) if sc is not None else None) == capi.AIM_EINVAL and _err().startswith(fn + ": ") and text in _err(), (fn, _err())
    ok = capi.MapSecParams(2, 1)
    assert lib.aim_mapper_set_secondary(None, C.byref(ok)) == capi.AIM_EINVAL and _err() == "aim_mapper_set_secondary: mapper is NULL"
    assert lib.aim_mapper_secondary_device_bytes(None, C.byref(ok), C.byref(b)) == capi.AIM_EINVAL and _err() == "aim_mapper_secondary_device_bytes: params is NULL"
    assert lib.aim_mapper_secondary_device_bytes(C.byref(mp), C.byref(ok), None) == capi.AIM_EINVAL and _err() == "aim_mapper_secondary_device_bytes: bytes is NULL"
    bad = _params(mask_q8=0)
    assert lib.aim_mapper_secondary_device_bytes(C.byref(bad), C.byref(ok), C.byref(b)) == capi.AIM_EINVAL and "mask_q8 0 is outside 1..256" in _err()
    so = capi.MapperSecondaryOut()
    assert lib.aim_mapper_secondary(None, 0, C.byref(so)) == capi.AIM_EINVAL and _err() == "aim_mapper_secondary: mapper is NULL"
    # 8 + 16 bytes per slot row, rounded up to 256 per buffer, per mapper slot
    want = mp.slots * (((8 * 64 * 4 + 255) & ~255) + ((16 * 64 * 4 + 255) & ~255))
    assert engine.mapper_secondary_device_bytes(mp, ok) == want


# ---- the model -------------------------------------------------------------------------------------------------------------------
def _tables(K, n, max_sec=15, rs=RS, seed=3):
    import secondary_model as sec
    d = sec.synthetic(seed, n, K, rs)
    s_req, s_tp, s_pat, s_seg, got = sec.synthetic_rows(d, K, rs, max_sec)
    sam = sec.synthetic_sam(seed, K, n, s_seg, d["cls"])
    return d, (s_req, s_tp, s_pat, s_seg, got), sam


@pytest.mark.parametrize("K", (1, 2, 4, 7, 16))
def test_rows_model_properties(K):
    import chain_class_model as ccm
    import secondary_model as sec
    import split_model as sm
    n = 120
    d, (s_req, s_tp, s_pat, s_seg, got), _ = _tables(K, n)
    cls, seg0 = d["cls"], d["seg"]
    touched = np.zeros(n * K, dtype=bool)
    touched[got] = True
    # every other slot keeps every byte
    for a, b in ((s_req, d["seg_req"]), (s_tp, d["seg_tp"]), (s_seg, seg0)):
        assert a[~touched].tobytes() == b[~touched].tobytes()
    assert s_pat[~touched].tobytes() == d["seg_pat"][~touched].tobytes()
    for slot in got:
        r, i = divmod(slot, K)
        j = int(cls["parent"][slot])
        ps = seg0[r * K + j]
        assert cls["flags"][slot] == ccm.SECONDARY and cls["flags"][r * K + j] & ccm.PRIMARY and ps["flags"] & sm.VALID
        g = s_seg[slot]
        assert (g["q_begin"], g["q_end"], g["read_len"], g["cand"]) == (ps["q_begin"], ps["q_end"], ps["read_len"], i) and g["flags"] == ps["flags"] & sec.KEPT
        L, w = int(g["q_end"]) - int(g["q_begin"]), s_req[slot]
        assert w["pattern_len"] == L and 0 <= w["text_len"] <= RS and w["idx"] == d["req"]["idx"][slot] and w["padding"] == 0
        assert int(s_tp[slot]) >> 63 == int(d["text_pos"][slot]) >> 63 and (int(s_tp[slot]) & (sm.MINUS - 1)) + int(w["text_len"]) <= sm.SYN_REF_LEN
        assert s_pat[slot, :L].tobytes() == d["reads"][r, int(g["q_begin"]):int(g["q_end"])].tobytes() and not s_pat[slot, L:].any()
    if K >= 4:
        # the planted reads: K - 1 secondaries under an extended parent; one not recoverable; windows cut by 0 and by ref_len
        assert [s for s in got if s < K] == list(range(1, K)) and (s_seg["q_begin"][1], s_seg["q_end"][1]) == (24, RS - 40)
        assert K + 1 not in got and K + 2 in got and int(s_tp[K + 2]) & (sm.MINUS - 1) == 0
        ends = [int(s_tp[2 * K + i] & np.uint64(sm.MINUS - 1)) + int(s_req["text_len"][2 * K + i]) for i in range(1, K)]
        assert ends[0] == sm.SYN_REF_LEN and all(e == sm.SYN_REF_LEN or s_req["text_len"][2 * K + 1 + i] == RS for i, e in enumerate(ends))
        assert not [s for s in got if 3 * K <= s < 4 * K]
        # max_sec cuts a family in candidate order
        got1 = _tables(K, n, max_sec=1)[1][4]
        assert [s for s in got1 if s < K] == [1] and set(got1) < set(got)
    n_sec = int(((cls["flags"] & 3) == ccm.SECONDARY).sum())
    assert (K == 1 and not got) or (len(got) > (n // 4 if K >= 4 else 4) and n_sec > len(got)), (len(got), n_sec)


@pytest.mark.parametrize("K", (1, 2, 4, 7, 16))
def test_select_and_records_model_properties(K):
    import chain_class_model as ccm
    import map_records_model as mm
    import secondary_model as sec
    import split_model as sm
    n = 200
    d, (_, _, _, seg, _), sam = _tables(K, n)
    cls, chains = d["cls"], d["chains"]
    x = sec.select(K, n, seg, sam, cls, chains, sec.SYN_MAX_SCORE, sec.SYN_UNIT)
    mapped = mm.mapped_slots(K, n, seg, sam)
    seen = {"swapped": 0, "tied": 0, "incomplete": 0, "single": 0, "runner_over_cap": 0}
    for r in range(n):
        for j in range(K):
            slot = r * K + j
            if sec.kind(cls, slot) != ccm.PRIMARY:
                continue
            fam = [i for i in range(K) if x["role"][r * K + i] and x["family"][r * K + i] == j]
            wins = [i for i in fam if x["role"][r * K + i] == 1]
            members = [j] + [i for i in range(K) if sec.kind(cls, r * K + i) == ccm.SECONDARY and cls["parent"][r * K + i] == j and seg["flags"][r * K + i] & sm.VALID]
            assert sorted(fam) == sorted(i for i in members if mapped[r, i]) and len(wins) == (1 if fam else 0)
            if not fam:
                continue
            w = wins[0]
            assert all(sam["score"][r * K + w] <= sam["score"][r * K + i] for i in fam)
            s = x[r * K + w]
            assert s["mapq"] <= min(s["aln_mapq"], 6 * min(int(chains["n_anchors"][r * K + w]), 10)) and (s["flags"] >> 4) + 1 == len(members)
            assert bool(s["flags"] & sec.SWAPPED) == (w != j) and (s["n_tied"] > 1) <= (s["aln_mapq"] == 0)
            seen["swapped"] += w != j
            seen["tied"] += s["n_tied"] > 1
            seen["incomplete"] += not s["flags"] & sec.COMPLETE
            seen["runner_over_cap"] += len(members) > len(fam) and s["gap"] != 65535
            if len(members) == 1:                     # a primary alone: exactly rule 12c's byte, the chain MAPQ of rule 8c
                assert cls["n_sub"][slot] > 0 or (s["mapq"] == cls["mapq"][slot] and s["gap"] == 65535 and s["aln_mapq"] == 60 and s["flags"] == sec.COMPLETE)
                seen["single"] += cls["n_sub"][slot] == 0
    assert seen["single"] > 10 and (K == 1 or all(v > 0 for v in seen.values())), seen
    if K >= 2:
        assert x["role"][0] == 0 and (x["role"][1:K] == 1).sum() == 1 and (x["flags"][1:K] & sec.SWAPPED).all()    # the primary over the cap, a mapped secondary wins
        t = 2 * K                                     # equal scores: the lowest candidate, MAPQ 0
        assert x["n_tied"][t] == K and x["aln_mapq"][t] == 0 and x["mapq"][t] == 0 and x["role"][t] == 1 and (x["role"][t + 1:t + K] == 2).all()
    for opt in (0, sec.SEC_RECORDS):
        off, rec, ms = sec.records(K, n, opt, seg, sam, cls, x)
        assert off[0] == 0 and off[n] == len(rec) == len(ms)
        for r in range(n):
            g, gs = rec[off[r]:off[r + 1]], ms[off[r]:off[r + 1]]
            roles = x["role"][r * K:(r + 1) * K]
            n1, n2 = int((roles == 1).sum()), int((roles == 2).sum()) if opt else 0
            assert len(g) == max(n1 + n2, 1) and (g["read"] == r).all() and (g["n_records"] == len(g)).all()
            if not n1:
                assert g[0]["sam"]["flags"] == sm.SAM_UNMAPPED and tuple(gs[0]) == (r * K, sec.INT32_MAX, 0, 0, 0, 0, 0)
                continue
            assert g["rank"].tolist() == list(range(len(g)))
            is2 = (g["sam"]["flags"] & sec.SAM_SECONDARY) != 0
            assert not is2[:n1].any() and is2[n1:].all() and (g["mapq"][n1:] == 0).all() and not (g["sam"]["flags"][n1:] & sm.SAM_SUPPLEMENTARY).any()
            assert ((g["sam"]["flags"][:n1] & sm.SAM_SUPPLEMENTARY) == 0).sum() == 1
            keys = [(int(q), int(f)) for q, f in zip(g["q_begin"][:n1], gs["family_slot"][:n1])]
            assert keys == sorted(keys) and sorted(g["slot"].tolist()) == sorted(r * K + i for i in range(K) if roles[i] == 1 or (opt and roles[i] == 2))
    # a batch without secondaries: rule 12c's records byte for byte
    none = np.array([not any(sec.kind(cls, r * K + i) == ccm.SECONDARY for i in range(K)) and
                     all(cls["n_sub"][r * K + i] == 0 and (chains["score"][r * K + i] > 0 or not mapped[r, i]) for i in range(K)) for r in range(n)])
    assert none.sum() > 10
    off, rec, _ = sec.records(K, n, sec.SEC_RECORDS, seg, sam, cls, x)
    off12, rec12 = mm.map_records(K, n, seg, sam, cls)
    for r in np.nonzero(none)[0]:
        assert rec[off[r]:off[r + 1]].tobytes() == rec12[off12[r]:off12[r + 1]].tobytes(), r


def test_contigs_in_the_record_model():
    import secondary_model as sec
    import split_model as sm
    K, n = 4, 60
    d, (_, _, _, seg, _), sam = _tables(K, n)
    x = sec.select(K, n, seg, sam, d["cls"], d["chains"], sec.SYN_MAX_SCORE, sec.SYN_UNIT)
    contig, starts = sec.synthetic_contigs(3, K, n)
    off, rec, ms = sec.records(K, n, sec.SEC_RECORDS, seg, sam, d["cls"], x)
    off2, rec2, ms2 = sec.records(K, n, sec.SEC_RECORDS, seg, sam, d["cls"], x, contig, starts)
    assert off.tobytes() == off2.tobytes() and ms.tobytes() == ms2.tobytes()
    outside = 0
    for a, b in zip(rec, rec2):
        if a["sam"]["flags"] & sm.SAM_UNMAPPED:
            assert b["sam"]["pad"] == sec.CONTIG_NONE and b["sam"]["pos"] == 0
            continue
        c = int(contig[a["slot"]])
        outside += c >= len(starts)
        assert b["sam"]["pad"] == c and int(b["sam"]["pos"]) == int(a["sam"]["pos"]) - (int(starts[c]) if c < len(starts) else 0)
    assert outside > 0


@pytest.mark.parametrize("K,K2", ((3, 4), (3, 8), (3, 16), (6, 8), (9, 16)))
def test_model_under_slot_padding(K, K2):
    """A read's K slots followed by empty ones are the same read: every part's output over the padded tables is the output over the
    tables themselves, slots renamed."""
    import secondary_model as sec
    import slot_padding as sp
    import split_model as sm
    n = 80
    d, (s_req, s_tp, s_pat, s_seg, got), sam = _tables(K, n)
    pd = dict(d, **{k: sp.pad(d[k], K, K2, n) for k in ("req", "text_pos", "chains", "cls", "seg_req", "seg_tp", "seg")})
    pd["seg_pat"] = sp.pad(d["seg_pat"].view([("row", "u1", (RS,))]).reshape(-1), K, K2, n).view(np.uint8).reshape(-1, RS)
    p_req, p_tp, p_pat, p_seg, p_got = sec.synthetic_rows(pd, K2, RS, 15)
    assert [divmod(s, K2) for s in p_got] == [divmod(s, K) for s in got]
    assert sp.unpad(p_req, K, K2, n)[0].tobytes() == s_req.tobytes() and sp.unpad(p_tp, K, K2, n)[0].tobytes() == s_tp.tobytes()
    assert sp.unpad(p_seg, K, K2, n)[0].tobytes() == s_seg.tobytes() and not sp.unpad(p_seg, K, K2, n)[1].view(np.uint8).any()
    x = sec.select(K, n, s_seg, sam, d["cls"], d["chains"], sec.SYN_MAX_SCORE, sec.SYN_UNIT)
    px = sec.select(K2, n, p_seg, sp.pad(sam, K, K2, n), pd["cls"], pd["chains"], sec.SYN_MAX_SCORE, sec.SYN_UNIT)
    assert px.tobytes() == sp.pad(x, K, K2, n).tobytes()
    off, rec, ms = sec.records(K, n, sec.SEC_RECORDS, s_seg, sam, d["cls"], x)
    poff, prec, pms = sec.records(K2, n, sec.SEC_RECORDS, p_seg, sp.pad(sam, K, K2, n), pd["cls"], px)
    want_ms = ms.copy()
    want_ms["family_slot"] = sp.rename(ms["family_slot"], rec["read"], K, K2)
    assert poff.tobytes() == off.tobytes() and prec.tobytes() == sp.records_renamed(rec, K, K2).tobytes() and pms.tobytes() == want_ms.tobytes()
    assert len(rec) > n and (rec["sam"]["flags"] & sec.SAM_SECONDARY).any() and (rec["sam"]["flags"] & sm.SAM_SUPPLEMENTARY).any()


# ---- the three read classes on the CPU models --------------------------------------------------------------------------------------
def _class_chains(name):
    import chain_class_model as ccm
    import chain_model as cm
    import minimizer_model as mz
    import secondary_model as sec
    from gpu_buffers import cached

    def make():
        ref, rows, rl, truth = sec.repeat_classes()[name]
        k, stride, w, max_occ, band, flank, min_votes, K = ccm.CHIMERIC_ROW
        req, tpos, votes, seeds, chains = cm.seed_chain(rows, rl, mz.build_index(ref, k, w), len(ref), k, stride, w, max_occ, band, flank, min_votes, K, ccm.CHIMERIC_SIZE)
        cls = ccm.classify(K, ccm.CHIMERIC_SIZE, ccm.MASK_DEFAULT, rl, tpos, seeds, chains)
        return ref, rows, rl, truth, req, tpos, seeds, chains, cls
    return cached(("secondary class", name), make)


@pytest.mark.parametrize("name", ("tie", "control", "exact"))
def test_class_premises_on_the_chain_model(name):
    """Asserted on the models, so that a change to hashing or chaining cannot silently empty the end-to-end test."""
    import chain_class_model as ccm
    import secondary_model as sec
    ref, rows, rl, truth, req, tpos, seeds, chains, cls = _class_chains(name)
    K = ccm.CHIMERIC_ROW[7]
    assert len(rl) == 16 and (seeds["n_cands"] == 2).all()
    for r in range(16):
        c0, c1 = r * K, r * K + 1
        at = [int(tpos[c]) & ((1 << 63) - 1) for c in (c0, c1)]
        assert [int(cls["flags"][c]) for c in (c0, c1)] == [ccm.PRIMARY, ccm.SECONDARY] and int(cls["parent"][c1]) == 0
        assert int(tpos[c0]) >> 63 == int(tpos[c1]) >> 63 == truth[r][2] and truth[r][3] in (4, 5)
        if name == "control":                         # the chains already prefer copy B
            assert sec.in_copy(at[0], sec.REPEAT_B) and sec.in_copy(at[1], sec.REPEAT_A) and chains["score"][c0] > chains["score"][c1] and 13 <= cls["mapq"][c0] <= 16
        else:                                         # equal chain scores: the copy of lowest position is the primary, chain MAPQ 0
            assert sec.in_copy(at[0], sec.REPEAT_A) and sec.in_copy(at[1], sec.REPEAT_B) and chains["score"][c0] == chains["score"][c1] and cls["mapq"][c0] == 0
        assert chains["n_anchors"][c0] >= 10 and chains["n_anchors"][c1] >= 10
    if name == "tie":
        assert 145 <= chains["score"].reshape(-1, K)[:, 0].min() and chains["score"].max() <= 170


@pytest.mark.parametrize("name", ("tie", "control", "exact"))
def test_identity_of_part_1(name):
    """One primary, no extension: the secondary's request and text_pos equal the chain kernel's own slot byte for byte, and its pattern
    row is the read row (which is zero behind L)."""
    import chain_class_model as ccm
    import secondary_model as sec
    import split_model as sm
    ref, rows, rl, truth, req, tpos, seeds, chains, cls = _class_chains(name)
    K, flank, rs = ccm.CHIMERIC_ROW[7], ccm.CHIMERIC_ROW[5], ccm.CHIMERIC_SIZE
    segs = sm.segments(K, rs, flank, len(ref), rl, rows, req, tpos, seeds, chains, cls)
    o_req, o_tp, o_pat, o_seg, got = sec.rows(K, rs, flank, len(ref), 15, rl, rows, req, tpos, seeds, chains, cls, *segs)
    assert got == [r * K + 1 for r in range(16)]
    for slot in got:
        r = slot // K
        assert o_req[slot].tobytes() == req[slot].tobytes() and o_tp[slot] == tpos[slot] and o_pat[slot].tobytes() == rows[r].tobytes()
        assert tuple(o_seg[slot]) == (0, rl[r], rl[r], sm.VALID | sm.LEFT_OPEN | sm.RIGHT_OPEN, 1)
        assert o_req[K * r].tobytes() == segs[0][K * r].tobytes() and o_seg[K * r].tobytes() == segs[3][K * r].tobytes()


# ---- the code objects ------------------------------------------------------------------------------------------------------------
def test_secondary_kernels_code_objects():
    """Each new kernel exists exactly once, uses no scratch and no static LDS and stays within kSecMaxVgpr (40, 34, 12 and 56 VGPRs at
    the time of writing)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_regs
    lib = os.path.join(ROOT, "aim_amd", "libaim_hip.so")
    if not os.path.exists(lib):
        pytest.fail("libaim_hip.so is missing: run the build")
    regs = codeobj_regs.kernel_regs(lib)
    bound = int(re.search(r"constexpr int kSecMaxVgpr = (\d+);", open(os.path.join(ROOT, "aim_amd", "csrc", "secondary.hpp")).read()).group(1))
    for name in _lib().aim_secondary_kernel_names().decode().split(","):
        found = [n for n in regs if re.search(r"\baim::%s\(" % name, n)]
        assert len(found) == 1, (name, found)
        r = regs[found[0]]
        print(name, r)
        assert r["scratch_bytes"] == 0 and r["lds_static_bytes"] == 0 and 0 < r["vgpr"] + r["agpr"] <= bound <= 512 // 8, (name, r, bound)


# ---- samout ----------------------------------------------------------------------------------------------------------------------
def test_samout_whole_text_with_secondaries():
    """A swapped locus with its losing copy as a 0x100 line, a split read whose second locus has a secondary, and an unmapped read;
    the same records without "sec" and without 0x100 lines give the text samout always gave."""
    from aim_amd import capi, samout
    M, S = 0, 4
    w = lambda n, op: (n << 4) | op
    cigar, md = [], []
    recs = [_record(0, 0, 2, 0, 12019, 24, 4, 12, [w(8, M)], "8", cigar, md),
            _record(0, 1, 2, 0x100, 4019, 0, 8, 24, [w(8, M)], "3A4", cigar, md),
            _record(1, 0, 3, 16, 199, 60, 0, 0, [w(4, M), w(4, S)], "4", cigar, md),
            _record(1, 1, 3, 0x800, 899, 30, 1, 3, [w(4, S), w(4, M)], "1C2", cigar, md),
            _record(1, 2, 3, 0x100 | 16, 2899, 0, 2, 6, [w(4, S), w(4, M)], "4", cigar, md),
            _record(2, 0, 1, 4, 0, 0, 0, 77, [], "", cigar, md)]
    out = {"records": np.array(recs, dtype=capi.MAP_RECORD_DTYPE), "rec_offsets": np.array([0, 2, 5, 6], dtype=np.uint32),
           "cigar": np.array(cigar, dtype=np.uint32), "md": np.frombuffer(bytes(md), dtype=np.uint8), "sec": np.zeros(6, dtype=capi.MAP_SEC_DTYPE)}
    names, reads, lens, quals = ["rep", "split", "none"], [b"ACGTACGT", b"AACCGGTT", b"TTTT"], [8, 8, 4], ["IIIIHHHH", None, "!!!!"]
    text = "".join(l + "\n" for l in samout.record_lines(out, names, reads, lens, "chrT", quals))
    assert text == (
        "rep\t0\tchrT\t12020\t24\t8M\t*\t0\t0\tACGTACGT\tIIIIHHHH\tNM:i:4\tMD:Z:8\tAS:i:-12\ttp:A:P\n"
        "rep\t256\tchrT\t4020\t0\t8M\t*\t0\t0\t*\t*\tNM:i:8\tMD:Z:3A4\tAS:i:-24\ttp:A:S\n"
        "split\t16\tchrT\t200\t60\t4M4S\t*\t0\t0\tAACCGGTT\t*\tNM:i:0\tMD:Z:4\tAS:i:0\ttp:A:P\tSA:Z:chrT,900,+,4S4M,30,1;\n"
        "split\t2048\tchrT\t900\t30\t4S4M\t*\t0\t0\tAACCGGTT\t*\tNM:i:1\tMD:Z:1C2\tAS:i:-3\ttp:A:P\tSA:Z:chrT,200,-,4M4S,60,0;\n"
        "split\t272\tchrT\t2900\t0\t4S4M\t*\t0\t0\t*\t*\tNM:i:2\tMD:Z:4\tAS:i:-6\ttp:A:S\n"
        "none\t4\t*\t0\t0\t*\t*\t0\t0\tTTTT\t!!!!\n")
    keep = [0, 2, 3, 5]
    plain = [recs[i].copy() for i in keep]
    for rec, n in zip(plain, (1, 2, 2, 1)):
        rec["n_records"] = n
    plain[2]["rank"] = 1
    without = {"records": np.array(plain, dtype=capi.MAP_RECORD_DTYPE), "rec_offsets": np.array([0, 1, 3, 4], dtype=np.uint32), "cigar": out["cigar"], "md": out["md"]}
    lines = text.splitlines()
    assert samout.record_lines(without, names, reads, lens, "chrT", quals) == [lines[i].replace("\ttp:A:P", "") for i in keep]
