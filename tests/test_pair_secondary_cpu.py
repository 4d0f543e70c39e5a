"""Rule 17c without a GPU: the struct size and the feature bit, every refusal of the three stateless entry points by message (each
condition alone, none of them needs a device), the numpy model (tests/pair_secondary_model.py) against a second, plain-loop
enumeration of all (K + 1)^2 combinations, its reduction to rule 14c on slot arrays without a secondary row, the invariance of what
the lanes of a read pair reduce, the code objects of the three new kernels, the mapper's refusals that need no device, the premises
of the four GPU truth classes on the chain model and the ends-free model, and a whole-text samout case."""
import ctypes as C
import functools
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aim_hip.h")
OK = 1 << 12               # any aligned address: nothing is dereferenced before the device probe


def _lib():
    from aim_amd import capi
    return capi.load()


def _err():
    return _lib().aim_last_error().decode()


def _define(name):
    m = re.search(r"#define\s+%s\s+(\S+)" % name, open(HEADER).read())
    return int(m.group(1).rstrip("uUlL"), 0)


def test_feature_bit_and_layouts():
    import pair_secondary_model as psm
    from aim_amd import capi, engine
    assert _define("AIM_FEATURE_PAIR_SECONDARY") == capi.FEATURE_PAIR_SECONDARY == 0x1000000 == 2 * _define("AIM_FEATURE_SECONDARY")
    assert engine.features() & capi.FEATURE_PAIR_SECONDARY and _lib().aim_abi_version() == 2
    assert capi.MAP_PAIR_MAPQ_DTYPE == psm.PAIR_MAPQ_DTYPE and capi.MAP_PAIR_MAPQ_DTYPE.itemsize == 16
    f = psm.PAIR_MAPQ_DTYPE.fields
    assert [f[k][1] for k in ("alt_sum", "mapq", "pair_mapq", "own_mapq", "tied")] == [0, 8, 10, 12, 14]
    assert re.search(r"int32_t alt_sum\[2\];.*\n\s*uint8_t mapq\[2\];.*\n\s*uint8_t pair_mapq\[2\];.*\n\s*uint8_t own_mapq\[2\];.*\n\s*uint8_t tied\[2\];", open(HEADER).read())
    assert _lib().aim_pair_secondary_kernel_names() == b"pair_sec_rescue_rows_kernel,pair_sec_select_kernel,map_mates_sec_kernel"
    # the structs the rule leaves alone
    assert capi.MAP_PAIR_DTYPE.itemsize == 32 and capi.MAP_MATE_DTYPE.itemsize == 16 and capi.SEC_SLOT_DTYPE.itemsize == 8 and C.sizeof(capi.MapPairParams) == 40


def _pp(**kw):
    from aim_amd import engine
    args = dict(min_span=300, max_span=500, unpaired_penalty=17, rescue=True, rescue_size=512)
    opts = kw.pop("options", None)
    args.update(kw)
    pp = engine.pair_params(**args)
    if opts is not None:
        pp.options = opts
    return pp


def _rows(pp=None, K=4, rs=104, ref_len=40000, nc=0, st=None, ln=None, n=8, rl=OK, reads=OK, seg=OK, sam=OK, contig=None, sec=OK, req=OK, tp=OK, pat=OK, est=None,
          null_pp=False):
    pp = pp or _pp()
    return _lib().aim_pair_rescue_rows_secondary_device(None if null_pp else C.byref(pp), K, rs, ref_len, nc, st, ln, n, rl, reads, seg, sam, contig, sec, req, tp, pat, est,
                                                        None)


def _select(pp=None, K=4, rs=104, n=8, rl=OK, seg=OK, sam=OK, cls=OK, contig=None, sec=OK, chains=OK, unit=3, res=OK, pairs=OK, pq=OK, est=None, null_pp=False):
    pp = pp or _pp()
    return _lib().aim_pair_select_secondary_device(None if null_pp else C.byref(pp), K, rs, n, rl, seg, sam, cls, contig, sec, chains, unit, res, 0, 0, pairs, pq, est, None)


def _mates(K=4, n=8, pairs=OK, seg=OK, sam=OK, sec=OK, contig=None, nc=0, st=None, off=OK, rec=OK, mates=OK):
    return _lib().aim_map_mates_secondary_device(K, n, pairs, seg, sam, sec, contig, nc, st, off, rec, mates, None)


SHARED = [  # rule 14c's refusals of aim_map_pair_params_t and of the batch's shape, in its order, from both entry points that take the struct
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
    for fn, call in (("aim_pair_rescue_rows_secondary_device", _rows), ("aim_pair_select_secondary_device", _select)):
        assert call(**kw) == capi.AIM_EINVAL and _err().startswith(fn + ": ") and text in _err(), (fn, kw, _err())


def test_refusals_keep_their_order():
    """A call that breaks several rules is refused for the first of them: the struct's before the entry point's own, score_unit before
    the buffers, a NULL buffer before an alignment."""
    from aim_amd import capi
    E = capi.AIM_EINVAL
    assert _rows(pp=_pp(options=3), n=7, ref_len=0, sec=None) == E and "unknown options 0x3" in _err()
    assert _rows(n=7, ref_len=0, sec=None) == E and "n_reads 7 is odd" in _err()
    assert _rows(ref_len=0, contig=OK, nc=0, sec=None) == E and "ref_len must be >= 1" in _err()
    assert _rows(contig=OK, nc=0, st=OK, ln=OK, sec=None) == E and "n_contigs 0 is outside" in _err()
    assert _rows(sec=None, sam=OK + 8) == E and "null device buffer" in _err()
    assert _select(pp=_pp(rescue_size=508), unit=0, sec=None) == E and "rescue_size 508 must be a multiple of 8" in _err()
    assert _select(unit=0, sec=None, sam=OK + 8) == E and "score_unit 0 must be >= 1" in _err()
    assert _select(sec=None, sam=OK + 8) == E and "null device buffer" in _err()
    assert _select(sam=OK + 8, sec=OK + 4) == E and "d_sam must be 16-byte aligned" in _err()


def test_entry_point_refusals_need_no_device():
    from aim_amd import capi
    E = capi.AIM_EINVAL
    for kw, text in ((dict(ref_len=0), "ref_len must be >= 1"), (dict(ref_len=0xFE000001), "ref_len 4261412865 is above"),
                     (dict(contig=OK, nc=0, st=OK, ln=OK), "n_contigs 0 is outside 1.."), (dict(contig=OK, nc=3, st=None, ln=OK), "without its contig table"),
                     (dict(contig=OK, nc=3, st=OK, ln=None), "without its contig table"), (dict(rl=None), "null device buffer"), (dict(reads=None), "null device buffer"),
                     (dict(seg=None), "null device buffer"), (dict(sam=None), "null device buffer"), (dict(sec=None), "null device buffer"),
                     (dict(req=None), "null device buffer"), (dict(tp=None), "null device buffer"), (dict(pat=None), "null device buffer"),
                     (dict(sam=OK + 8), "d_sam must be 16-byte aligned"), (dict(req=OK + 8), "d_res_requests must be 16-byte aligned"),
                     (dict(reads=OK + 4), "d_reads must be 8-byte aligned"), (dict(pat=OK + 4), "d_res_patterns must be 8-byte aligned"),
                     (dict(seg=OK + 4), "d_seg must be 8-byte aligned"), (dict(tp=OK + 4), "d_res_text_pos must be 8-byte aligned"),
                     (dict(sec=OK + 4), "d_sec must be 8-byte aligned"), (dict(est=OK + 8), "d_est must be 16-byte aligned")):
        assert _rows(**kw) == E and _err().startswith("aim_pair_rescue_rows_secondary_device: ") and text in _err(), (kw, _err())
    # without AIM_PAIR_RESCUE the rows entry point still wants its rescue_size; the choice does not read it and needs no d_res_sam
    off = _pp(rescue=False, rescue_size=0)
    assert _rows(pp=off) == E and "rescue_size 0 is below read_size 104" in _err()
    assert _select(pp=off, res=None, pairs=OK + 8) == E and "d_pairs must be 16-byte aligned" in _err()      # (the NULL d_res_sam passed)
    for kw, text in ((dict(unit=0), "score_unit 0 must be >= 1"), (dict(unit=-3), "score_unit -3 must be >= 1"), (dict(rl=None), "null device buffer"),
                     (dict(seg=None), "null device buffer"), (dict(sam=None), "null device buffer"), (dict(cls=None), "null device buffer"),
                     (dict(sec=None), "null device buffer"), (dict(chains=None), "null device buffer"), (dict(pairs=None), "null device buffer"),
                     (dict(pq=None), "null device buffer"), (dict(res=None), "null device buffer"), (dict(sam=OK + 8), "d_sam must be 16-byte aligned"),
                     (dict(res=OK + 8), "d_res_sam must be 16-byte aligned"), (dict(pairs=OK + 8), "d_pairs must be 16-byte aligned"),
                     (dict(pq=OK + 8), "d_pair_mapq must be 16-byte aligned"), (dict(seg=OK + 4), "d_seg must be 8-byte aligned"),
                     (dict(cls=OK + 4), "d_class must be 8-byte aligned"), (dict(sec=OK + 4), "d_sec must be 8-byte aligned"),
                     (dict(chains=OK + 4), "d_chains must be 8-byte aligned"), (dict(est=OK + 8), "d_est must be 16-byte aligned")):
        assert _select(**kw) == E and _err().startswith("aim_pair_select_secondary_device: ") and text in _err(), (kw, _err())
    for kw, text in ((dict(n=7), "n_reads 7 is odd"), (dict(K=0), "K 0 is outside 1..16"), (dict(K=17), "K 17 is outside 1..16"),
                     (dict(K=16, n=1 << 28), "(K 16 + 1) does not fit 32 bits"), (dict(contig=OK, nc=0, st=OK), "n_contigs 0 is outside 1.."),
                     (dict(contig=OK, nc=2, st=None), "without its contig table"), (dict(pairs=None), "null device buffer"), (dict(seg=None), "null device buffer"),
                     (dict(sam=None), "null device buffer"), (dict(sec=None), "null device buffer"), (dict(off=None), "null device buffer"),
                     (dict(rec=None), "null device buffer"), (dict(mates=None), "null device buffer"), (dict(sam=OK + 8), "d_sam must be 16-byte aligned"),
                     (dict(pairs=OK + 8), "d_pairs must be 16-byte aligned"), (dict(rec=OK + 8), "d_records must be 16-byte aligned"),
                     (dict(mates=OK + 8), "d_mates must be 16-byte aligned"), (dict(seg=OK + 4), "d_seg must be 8-byte aligned"),
                     (dict(sec=OK + 4), "d_sec must be 8-byte aligned")):
        assert _mates(**kw) == E and _err().startswith("aim_map_mates_secondary_device: ") and text in _err(), (kw, _err())


# ---- the model against a plain enumeration ---------------------------------------------------------------------------------------------
def _enumerate_pair(t, K, m, pp, unit):
    """Rule 17c's choice and pair MAPQ of read pair m by a loop over all (K + 1)^2 index pairs, written without the model's helpers:
    (taken, (vi, vj), cost, n_best, second, span, [alt, tied, pair_mapq] per read, unpaired, reps) from the input tables."""
    import pair_model as pm
    INT_MAX = 2 ** 31 - 1
    seg, sam, sec, contig, res = t["seg"], t["sam"], t["sec"], t["contig"], t["res_sam"]
    rows = []
    for r in (2 * m, 2 * m + 1):
        c = []
        for i in range(K):
            s = r * K + i
            ok = bool(seg["flags"][s] & 1) and not sam["flags"][s] & 0x4 and sec["role"][s] != 0
            c.append((ok, int(sam["pos"][s]), int(sam["ref_span"][s]), int(sam["score"][s]), bool(sam["flags"][s] & 0x10), int(contig[s]) if contig is not None else 0))
        rows.append(c)
    reps = []
    for x, r in enumerate((2 * m, 2 * m + 1)):
        best = None
        for i in range(K):
            if rows[x][i][0] and sec["role"][r * K + i] == 1 and (best is None or sec["family"][r * K + i] < sec["family"][r * K + best]):
                best = i
        reps.append(best)

    def proper(x, y):
        if not x[0] or not y[0] or x[5] != y[5] or x[4] == y[4]:
            return None
        f, rv = (y, x) if x[4] else (x, y)
        span = rv[1] + rv[2] - f[1]
        return span if f[1] <= rv[1] and pp.min_span <= span <= pp.max_span else None

    def combos(with_rescue):
        out = []
        for i in range(K + 1):
            for j in range(K + 1):
                if (i == K or j == K) and not with_rescue or (i == K and j == K):
                    continue
                if proper(rows[0][i], rows[1][j]) is not None:
                    out.append((min(rows[0][i][3] + rows[1][j][3], INT_MAX - 1), i, j, proper(rows[0][i], rows[1][j])))
        return out

    for x in (0, 1):
        rows[x].append((False, 0, 0, 0, False, 0))
    none = not combos(False)
    for x, r in enumerate((2 * m, 2 * m + 1)):              # index K: the rescue row where it was tried and came back mapped
        L = min(max(int(t["read_len"][r]), 0), pm.READ_SIZE)
        if pp.options & 1 and none and reps[1 - x] is not None and L > 0 and not res["flags"][r] & 0x4:
            rows[x][K] = (True, int(res["pos"][r]), int(res["ref_span"][r]), int(res["score"][r]), bool(res["flags"][r] & 0x10), rows[1 - x][reps[1 - x]][5])
    all_c = sorted(combos(True))
    unpaired = None
    if reps[0] is not None and reps[1] is not None:
        unpaired = min(rows[0][reps[0]][3] + rows[1][reps[1]][3] + pp.unpaired_penalty, INT_MAX - 1)
    if not all_c or (unpaired is not None and all_c[0][0] > unpaired):
        return (False, reps, unpaired, all_c[0][0] if all_c else None)
    c, vi, vj, span = all_c[0]
    per_read = []
    for x, v in ((0, vi), (1, vj)):
        alt, tied = INT_MAX, 0
        for cc in all_c:
            if cc[1 + x] != v:
                alt = min(alt, cc[0])
                tied += cc[0] == c
        if unpaired is not None and reps[x] != v:
            alt = min(alt, unpaired)
        per_read.append((alt, min(tied, 255), 0 if tied else 60 if alt == INT_MAX else min(60, 6 * max(alt - c, 0) // unit)))
    return (True, (vi, vj), c, sum(1 for cc in all_c if cc[0] == c), all_c[1][0] if len(all_c) > 1 else INT_MAX, span, per_read)


@pytest.mark.parametrize("contigs", (False, True), ids=("one-seq", "contigs"))
@pytest.mark.parametrize("K", (1, 3, 4, 8, 16))
def test_model_equals_plain_enumeration(K, contigs):
    import pair_model as pm
    import pair_secondary_batch as pb
    import secondary_model as scm
    n = 260
    t = pb.tables(5, K, n, contigs)
    o = pb.run_model(t, K, n, cigar_base=1000, md_base=2000)
    pairs, pq = o["pairs"], o["pq"]
    pp = pb.params()
    taken = promoted = rescued = 0
    for m in range(n // 2):
        e = _enumerate_pair(t, K, m, pp, pb.SCORE_UNIT)
        p, q = pairs[m], pq[m]
        assert bool(p["flags"] & pm.PROPER) == e[0], (m, e)
        if not e[0]:
            _, reps, unpaired, best = e
            assert p["slot"].tolist() == [(2 * m + x) * K + reps[x] if reps[x] is not None else pm.NONE for x in (0, 1)]
            assert p["score_sum"] == (unpaired if unpaired is not None else pm.INT_MAX) and p["n_best"] == 0 and p["span"] == 0
            assert p["second_sum"] == (best if best is not None and unpaired is not None else pm.INT_MAX)
            assert q["alt_sum"].tolist() == [pm.INT_MAX] * 2 and q.tobytes()[8:] == bytes(8)
            for r in (2 * m, 2 * m + 1):                      # not taken: no byte changes
                sl = slice(r * K, (r + 1) * K)
                assert o["sec"][sl].tobytes() == t["sec"][sl].tobytes() and o["seg"][sl].tobytes() == t["seg"][sl].tobytes() and o["sam"][sl].tobytes() == t["sam"][sl].tobytes()
            continue
        taken += 1
        _, (vi, vj), c, n_best, second, span, per_read = e
        assert p["slot"].tolist() == [2 * m * K + vi, (2 * m + 1) * K + vj] and (p["score_sum"], p["n_best"], p["second_sum"], p["span"]) == (c, n_best, second, span), (m, e, p)
        for x, v in ((0, vi), (1, vj)):
            r = 2 * m + x
            assert (q["alt_sum"][x], q["tied"][x], q["pair_mapq"][x]) == per_read[x], (m, x, q, per_read)
            own = int(t["sec"]["mapq"][r * K + v]) if v != K and t["sec"]["role"][r * K + v] == 1 else 0
            assert q["own_mapq"][x] == own and own <= q["mapq"][x] <= max(own, min(int(q["pair_mapq"][x]), own + 40))
            # after apply the chosen slot is the role-1 slot of its family and carries the MAPQ; the family has exactly one role 1
            s = r * K + (0 if v == K else v)
            assert o["sec"]["role"][s] == 1 and o["sec"]["mapq"][s] == q["mapq"][x]
            fam = int(o["sec"]["family"][s])
            sl = slice(r * K, (r + 1) * K)
            assert ((o["sec"]["role"][sl] == 1) & (o["sec"]["family"][sl] == fam)).sum() == 1
            assert ((o["sec"]["role"][sl] != 0) == (t["sec"]["role"][sl] != 0)).all() or v == K
            if v == K:
                rescued += 1
                assert o["sec"][sl][1:].tobytes() == bytes(8 * (K - 1)) and o["sec"]["gap"][s] == 65535 and o["sec"]["flags"][s] == scm.COMPLETE
                assert q["mapq"][x] <= q["mapq"][1 - x]
            elif t["sec"]["role"][s] == 2:
                promoted += 1
                assert bool(o["sec"]["flags"][s] & scm.SWAPPED) == (v != fam) and o["sec"]["aln_mapq"][s] == 0 and o["sec"]["gap"][s] == 0
    assert taken > 20 and rescued > 3 and (promoted > 0 or K < 4), (taken, promoted, rescued)
    # the records: one line without 0x800 / 0x100 per mapped read, 0x2 on exactly the two chosen records, never on a 0x100 record
    fl = o["rec"]["sam"]["flags"].astype(np.int64)
    assert ((fl & 0x2) != 0).sum() == 2 * taken and not ((fl & 0x2) != 0)[(fl & 0x100) != 0].any() and (o["mates"]["tlen"][(fl & 0x100) != 0] == 0).all()
    assert (fl & 0x1).all() and (K < 4 or ((fl & 0x100) != 0).any())


@pytest.mark.parametrize("contigs", (False, True), ids=("one-seq", "contigs"))
@pytest.mark.parametrize("K", (1, 4, 9, 16))
def test_reduces_to_rule_14c_without_secondary_rows(K, contigs):
    """On slot arrays in which no secondary got a row, aim_map_pair_t, the rescue rows and the slot arrays after apply are rule 14c's."""
    import pair_model as pm
    import pair_secondary_batch as pb
    n = 260
    t = pb.tables(7, K, n, contigs, secondaries=False)
    assert not (t["sec"]["role"] == 2).any()
    for rescue in (True, False):
        o = pb.run_model(t, K, n, rescue=rescue, cigar_base=1000, md_base=2000)
        pp = pb.params(rescue)
        req, tpos, rows = pm.rescue_rows(pp, K, pm.READ_SIZE, t["ref_len"], n, t["read_len"], t["reads"], t["seg"], t["sam"], t["contig"], t["starts"], t["lens"])
        assert o["req"].tobytes() == req.tobytes() and o["tpos"].tobytes() == tpos.tobytes() and sorted(o["rows"]) == sorted(rows)
        pairs, seg, sam, cls, contig = pm.select(pp, K, pm.READ_SIZE, n, t["read_len"], t["seg"], t["sam"], t["cls"], t["contig"], t["res_sam"], 1000, 2000)
        assert o["pairs"].tobytes() == pairs.tobytes() and o["seg"].tobytes() == seg.tobytes() and o["sam"].tobytes() == sam.tobytes() and o["cls"].tobytes() == cls.tobytes()
        assert contig is None or o["contig"].tobytes() == contig.tobytes()
        f = pairs["flags"]
        assert (f & pm.PROPER).any() and bool((f & (pm.RESCUED_A | pm.RESCUED_B)).any()) == rescue


@pytest.mark.parametrize("K", (4, 16))
def test_alternatives_are_invariant_under_permuting_lanes_and_subsets(K):
    """What a read pair's lanes do in the second pass: each holds (alt_a, alt_b, tied_a, tied_b) of a subset of the combinations, and
    the parts meet by min and by sum. Any order and any split gives the rule's own statement; and so does the choice (pair_model.combine)."""
    import pair_model as pm
    import pair_secondary_batch as pb
    import pair_secondary_model as psm
    n = 260
    t = pb.tables(5, K, n, True)
    pp = pb.params()
    part = psm.taking_part(K, n, t["seg"], t["sam"], t["sec"])
    rng = np.random.default_rng(9)
    seen = ties = 0
    INT_MAX = pm.INT_MAX

    def one(cc, vi, vj, c):
        return (cc[0] if cc[1] != vi else INT_MAX, cc[0] if cc[2] != vj else INT_MAX, int(cc[1] != vi and cc[0] == c), int(cc[2] != vj and cc[0] == c))

    join = lambda x, y: (min(x[0], y[0]), min(x[1], y[1]), x[2] + y[2], x[3] + y[3])
    empty = (INT_MAX, INT_MAX, 0, 0)
    for m in range(n // 2):
        ca, cb = pm.read_cands(K, 2 * m, part, t["sam"], t["contig"]), pm.read_cands(K, 2 * m + 1, part, t["sam"], t["contig"])
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
        if not combos:
            continue
        seen += 1
        c, vi, vj = want[:3]
        wa, wb = psm.pair_mapq(combos, c, vi, 0, None, None, 3), psm.pair_mapq(combos, c, vj, 1, None, None, 3)
        ties += wa[1] > 0 or wb[1] > 0
        for _ in range(4):
            order = [combos[i] for i in rng.permutation(len(combos))]
            assert functools.reduce(pm.combine, order, None) == want
            parts = [one(cc, vi, vj, c) for cc in order]
            assert functools.reduce(join, parts, empty) == (wa[0], wb[0], wa[1], wb[1])
            cuts = sorted(rng.integers(0, len(order) + 1, size=3).tolist())
            lanes = [functools.reduce(join, parts[a:b], empty) for a, b in zip([0] + cuts, cuts + [len(order)])]   # four lanes, some of them empty
            assert join(join(lanes[0], lanes[1]), join(lanes[2], lanes[3])) == join(join(lanes[3], lanes[0]), join(lanes[1], lanes[2])) == (wa[0], wb[0], wa[1], wb[1])
    assert seen > 50 and ties > 5, (seen, ties)


def test_estimate_replaces_the_bounds():
    """d_est given: the model runs on the estimate's bounds, and on this batch that changes a choice and a window."""
    import pair_secondary_batch as pb
    K, n = 4, 260
    t = pb.tables(5, K, n, False)
    a, b = pb.run_model(t, K, n), pb.run_model(t, K, n, est=pb.estimate())
    assert a["pairs"].tobytes() != b["pairs"].tobytes() and a["tpos"].tobytes() != b["tpos"].tobytes()
    assert (b["pairs"]["span"][b["pairs"]["span"] > 0] >= 320).all() and (b["pairs"]["span"] <= 470).all()


def test_pair_secondary_kernels_code_objects():
    """Each new kernel exists exactly once, uses no scratch and no static LDS and stays within kPairMaxVgpr."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_regs
    lib = os.path.join(ROOT, "aim_amd", "libaim_hip.so")
    if not os.path.exists(lib):
        pytest.fail("libaim_hip.so is missing: run the build")
    regs = codeobj_regs.kernel_regs(lib)
    bound = int(re.search(r"constexpr int kPairMaxVgpr = (\d+);", open(os.path.join(ROOT, "aim_amd", "csrc", "pair.hpp")).read()).group(1))
    names = _lib().aim_pair_secondary_kernel_names().decode().split(",")
    assert len(names) == 3
    for name in names:
        found = [k for k in regs if re.search(r"\baim::%s\(" % name, k)]
        assert len(found) == 1, (name, found)
        r = regs[found[0]]
        print(name, r)
        assert r["scratch_bytes"] == 0 and r["lds_static_bytes"] == 0 and 0 < r["vgpr"] + r["agpr"] <= bound <= 512 // 8, (name, r, bound)


# ---- the mapper's side without a device -------------------------------------------------------------------------------------------------
def test_mapper_setter_refusals_and_bytes():
    """aim_mapper_pairing_secondary_device_bytes answers without a device and refuses in the setter's order -- the mapper's parameters,
    aim_mapper_set_pairing's of pp, then rule 16c's of sp --; the setter and the view refuse a NULL mapper before anything else."""
    import mapper_batch as mb
    from aim_amd import capi, engine
    lib, E = _lib(), capi.AIM_EINVAL
    mp = mb.params_with()
    pp = lambda **kw: _pp(**dict(dict(rescue_size=engine.round_up_8(200 + mp.seed.read_size)), **kw))
    sc, b = engine.secondary_params(2), C.c_uint64(0)
    fn = "aim_mapper_pairing_secondary_device_bytes: "
    call = lambda p, s: lib.aim_mapper_pairing_secondary_device_bytes(C.byref(mp), C.byref(p) if p is not None else None, C.byref(s) if s is not None else None, C.byref(b))
    bad_sc = engine.secondary_params(0)
    for p, s, text in ((pp(options=2), bad_sc, "unknown options 0x2"), (pp(min_span=-5), bad_sc, "0 <= min_span"), (pp(rescue_size=100), bad_sc, "rescue_size 100 must be a multiple of 8"),
                       (None, bad_sc, "aim_map_pair_params_t is NULL"), (pp(), bad_sc, "max_sec 0 is outside 1..15"), (pp(), engine.secondary_params(16), "max_sec 16 is outside 1..15"),
                       (pp(), None, "NULL"), (pp(), capi.MapSecParams(2, 2), "unknown option")):
        assert call(p, s) == E and _err().startswith(fn) and text in _err(), (text, _err())
    assert lib.aim_mapper_pairing_secondary_device_bytes(None, C.byref(pp()), C.byref(sc), C.byref(b)) == E and _err() == fn + "params is NULL"
    assert lib.aim_mapper_pairing_secondary_device_bytes(C.byref(mp), C.byref(pp()), C.byref(sc), None) == E and _err() == fn + "bytes is NULL"
    both = engine.mapper_pairing_secondary_device_bytes(mp, pp(), sc)
    pairs_per_slot = (mp.max_reads + 1) // 2
    lo = engine.mapper_pairing_device_bytes(mp, pp()) + engine.mapper_secondary_device_bytes(mp, sc)
    assert lo + mp.slots * 16 * pairs_per_slot <= both <= lo + mp.slots * (16 * pairs_per_slot + 256)      # the two setters' buffers plus aim_map_pair_mapq_t per pair
    ep = engine.pair_estimate_params()
    assert lib.aim_mapper_set_pairing_secondary(None, C.byref(pp()), C.byref(ep), C.byref(sc)) == E and _err() == "aim_mapper_set_pairing_secondary: mapper is NULL"
    assert lib.aim_mapper_pair_mapq(None, 0, None) == E and _err() == "aim_mapper_pair_mapq: mapper is NULL"
    src = open(os.path.join(ROOT, "aim_amd", "csrc", "capi_mapper.hip")).read()      # the order inside the setter: pp, ep, sp, then the state
    body = src[src.index("int set_pairing(const char *fn"):src.index("HIP_TRY(hipSetDevice(m->device));", src.index("int set_pairing(const char *fn"))]
    at = [body.index(x) for x in ("check_pairing(fn", "check_pair_est_params(fn", "check_secondary(fn", "state_for_pairing_secondary(fn, m)", "in_flight")]
    assert at == sorted(at)


def test_samout_paired_secondary_whole_text():
    """A proper pair whose first read has a 0x100 line: paired lines with tp:A:P / tp:A:S; the 0x100 line carries the mate fields, no 0x2,
    TLEN 0, `*` for SEQ and QUAL, MAPQ 0 and no SA."""
    from aim_amd import capi, samout
    from mapper_batch import record as _record
    w = lambda n, op: (n << 4) | op
    cigar, md = [], []
    recs = [_record(0, 0, 2, 0x1 | 0x2 | 0x20 | 0x40, 12019, 34, 0, 0, [w(8, 0)], "8", cigar, md),
            _record(0, 1, 2, 0x1 | 0x20 | 0x40 | 0x100, 4019, 0, 0, 0, [w(8, 0)], "8", cigar, md),
            _record(1, 0, 1, 0x1 | 0x2 | 0x10 | 0x80, 12719, 60, 1, 3, [w(8, 0)], "2A5", cigar, md)]
    mates = np.array([(12719, 708, 0), (12719, 0, 0), (12019, -708, 0)], dtype=capi.MAP_MATE_DTYPE)
    sec = np.zeros(3, dtype=capi.MAP_SEC_DTYPE)
    out = {"records": np.array(recs, dtype=capi.MAP_RECORD_DTYPE), "rec_offsets": np.array([0, 2, 3], dtype=np.uint32), "cigar": np.array(cigar, dtype=np.uint32),
           "md": np.frombuffer(bytes(md), dtype=np.uint8), "mates": mates, "sec": sec}
    text = "".join(l + "\n" for l in samout.record_lines(out, ["p", "p"], [b"ACGTACGT", b"AACCGGTT"], [8, 8], "chr", quals=["IIIIHHHH", "ABCDEFGH"]))
    assert text == (
        "p\t99\tchr\t12020\t34\t8M\t=\t12720\t708\tACGTACGT\tIIIIHHHH\tNM:i:0\tMD:Z:8\tAS:i:0\ttp:A:P\n"
        "p\t353\tchr\t4020\t0\t8M\t=\t12720\t0\t*\t*\tNM:i:0\tMD:Z:8\tAS:i:0\ttp:A:S\n"
        "p\t147\tchr\t12720\t60\t8M\t=\t12020\t-708\tAACCGGTT\tHGFEDCBA\tNM:i:1\tMD:Z:2A5\tAS:i:-3\ttp:A:P\n")


# ---- the premises of the GPU truth classes ----------------------------------------------------------------------------------------------
def _truth(cls):
    import pair_secondary_batch as pb
    if cls == 1:
        return pb.truth_class1()
    if cls == 2:
        return pb.truth_class2()[:4]
    if cls == 3:
        return pb.truth_class3()
    return pb.truth_class4()[:4]


def _truth_chains(cls):
    from gpu_buffers import cached

    def make():
        import chain_class_model as ccm
        import chain_model as cm
        import minimizer_model as mz
        ref, rows, rl, truth = _truth(cls)
        k, stride, w, max_occ, band, flank, min_votes, K = ccm.CHIMERIC_ROW
        req, tpos, votes, seeds, chains = cm.seed_chain(rows, rl, mz.build_index(ref, k, w), len(ref), k, stride, w, max_occ, band, flank, min_votes, K, ccm.CHIMERIC_SIZE)
        return ref, rows, rl, truth, tpos, seeds, chains, ccm.classify(K, ccm.CHIMERIC_SIZE, ccm.MASK_DEFAULT, rl, tpos, seeds, chains)
    return cached(("pair secondary truth class", cls), make)


@pytest.mark.parametrize("cls", (1, 2, 3, 4))
def test_truth_class_premises_on_the_chain_model(cls):
    """What the GPU expectations of the four truth classes rest on, asserted on the chain and class models so that a change to hashing or
    chaining cannot silently empty them: the repeat read has exactly two candidates, a primary and its secondary, on the copies and in the
    order the class assumes; an exact mate has one chain at its true place; a substituted mate has none."""
    import chain_class_model as ccm
    import pair_secondary_batch as pb
    import secondary_model as scm
    ref, rows, rl, truth, tpos, seeds, chains, klass = _truth_chains(cls)
    k, stride, w, max_occ, band, flank, min_votes, K = ccm.CHIMERIC_ROW
    near = scm.REPEAT_B - scm.REPEAT_LEN - pb.T4_GAP
    assert len(rl) == 32 and len(truth) == 16
    for m, ((lo, hi, strand), (mlo, mhi, mstrand)) in enumerate(truth):
        a, b = 2 * m, 2 * m + 1
        assert seeds["n_cands"][a] == 2
        at = [int(tpos[a * K + i]) & ((1 << 63) - 1) for i in (0, 1)]
        assert [int(klass["flags"][a * K + i]) for i in (0, 1)] == [ccm.PRIMARY, ccm.SECONDARY] and int(klass["parent"][a * K + 1]) == 0
        assert int(tpos[a * K]) >> 63 == int(tpos[a * K + 1]) >> 63 == strand
        first, second = {1: (scm.REPEAT_A, scm.REPEAT_B), 2: (scm.REPEAT_B, scm.REPEAT_A), 3: (scm.REPEAT_A, scm.REPEAT_B), 4: (near, scm.REPEAT_B)}[cls]
        assert scm.in_copy(at[0], first) and scm.in_copy(at[1], second), (cls, m, at)
        if cls == 2:                                  # the chains already prefer copy B
            assert chains["score"][a * K] > chains["score"][a * K + 1] and klass["mapq"][a * K] > 0
        else:                                         # equal chain scores: the copy of lowest position is the primary, chain MAPQ 0
            assert chains["score"][a * K] == chains["score"][a * K + 1] and klass["mapq"][a * K] == 0
        assert chains["n_anchors"][a * K] >= 10 and chains["n_anchors"][a * K + 1] >= 10          # anchor_cap 60 on either copy
        if cls == 3:
            assert seeds["n_cands"][b] == 0           # no intact 11-mer: only a rescue places the mate
        else:
            assert seeds["n_cands"][b] == 1 and abs((int(tpos[b * K]) & ((1 << 63) - 1)) - mlo) <= flank + band and int(tpos[b * K]) >> 63 == mstrand
            assert chains["n_anchors"][b * K] >= 10 and klass["mapq"][b * K] == 60


def _placed(truth, where, mate_mapped, K=2):
    """Slot tables of the 16 pairs with the repeat read's two copies in slots 0 and 1 (`where(m)` = their starts and roles) and the mate
    at its true place in slot 0, or unmapped: (seg, sam, sec) for the models."""
    import pair_model as pm
    import secondary_model as scm
    n = 2 * len(truth)
    seg, sam, sec = np.zeros(n * K, dtype=pm.SEG_DTYPE), np.zeros(n * K, dtype=pm.SAM_DTYPE), np.zeros(n * K, dtype=scm.SEC_SLOT)
    sam["flags"] = pm.SAM_UNMAPPED
    for m, ((lo, hi, strand), (mlo, mhi, mstrand)) in enumerate(truth):
        for i, (start, role, score) in enumerate(where(m)):
            s = 2 * m * K + i
            seg["flags"][s], sam["pos"][s], sam["ref_span"][s], sam["score"][s], sam["flags"][s] = pm.SEG_VALID, start, hi - lo, score, pm.SAM_REVERSE if strand else 0
            sec["role"][s], sec["family"][s] = role, 0
        if mate_mapped:
            s = (2 * m + 1) * K
            seg["flags"][s], sam["pos"][s], sam["ref_span"][s], sam["flags"][s] = pm.SEG_VALID, mlo, mhi - mlo, pm.SAM_REVERSE if mstrand else 0
            sec["role"][s] = 1
    return seg, sam, sec


def test_truth_class_premises_on_the_ends_free_model():
    """Classes 1, 2 and 4: with every copy at its place no rescue is tried, and the proper combinations are the ones the class assumes (in
    class 2 the two copies differ by 3 per covered site under the DP model). Class 3: the rescue window anchored at copy B, the
    representative, holds the substituted mate at 30 mismatches, within the cost cap; anchored at copy A, slot 0, it scores above the cap."""
    import chain_class_model as ccm
    import endsfree_model as efm
    import mapper_batch as mb
    import pair_model as pm
    import pair_secondary_batch as pb
    import pair_secondary_model as psm
    import secondary_model as scm
    import seed_model as sdm
    K, rs, L = 2, ccm.CHIMERIC_SIZE, scm.REPEAT_READ_LEN
    d = scm.REPEAT_B - scm.REPEAT_A
    for cls in (1, 2, 4):
        ref, rows, rl, truth = _truth(cls)
        n = len(rl)
        other = pb.T4_GAP + scm.REPEAT_LEN if cls == 4 else d
        scores = {}
        if cls == 2:                                  # the read against either copy, end to end: 3 per covered site apart
            covered = pb.truth_class2()[4]
            req = np.zeros(2 * len(truth), dtype=pm.REQUEST_DTYPE)
            pat, txt = np.zeros((2 * len(truth), rs), dtype=np.uint8), np.zeros((2 * len(truth), rs), dtype=np.uint8)
            for m, ((lo, hi, strand), _) in enumerate(truth):
                for x, start in enumerate((lo, lo - d)):
                    req[2 * m + x] = (L, L, 0, 2 * m + x)
                    pat[2 * m + x, :L] = rows[2 * m, :L]
                    txt[2 * m + x, :L] = sdm.revcomp(ref[start:start + L]) if strand else ref[start:start + L]
            sc = efm.dp_scores(req, pat, txt, mb.X, mb.O, mb.E, ends_free=(0, 0, 0, 0)).tolist()
            for m in range(len(truth)):
                assert sc[2 * m + 1] - sc[2 * m] == mb.X * covered[m] and covered[m] in (4, 5), (m, sc[2 * m:2 * m + 2])
                assert pb.T2_PENALTIES[1] < mb.X * covered[m] < pb.T2_PENALTIES[0]
                scores[m] = sc[2 * m:2 * m + 2]
        # slot 0 / 1 as rule 16c leaves them: the winner role 1
        where = {1: lambda m: [(truth[m][0][0] - d, 1, 0), (truth[m][0][0], 2, 0)], 4: lambda m: [(truth[m][0][0] - other, 1, 0), (truth[m][0][0], 2, 0)],
                 2: lambda m: [(truth[m][0][0], 1, scores[m][0]), (truth[m][0][0] - d, 2, scores[m][1])]}[cls]
        seg, sam, sec = _placed(truth, where, True)
        mn, mx = (pb.T4_MIN_SPAN, pb.T4_MAX_SPAN) if cls == 4 else (pb.T_MIN_SPAN, pb.T_MAX_SPAN)
        pp = pm.Params(mn, mx, pb.T_PENALTY, pm.RESCUE, mx - mn + rs)
        req, tpos, _ = psm.rescue_rows(pp, K, rs, len(ref), n, rl, rows, seg, sam, sec)
        assert not req["pattern_len"].any(), cls
        part = psm.taking_part(K, n, seg, sam, sec)
        for m in range(len(truth)):
            combos = pm.proper_combos(pp, pm.read_cands(K, 2 * m, part, sam, None), pm.read_cands(K, 2 * m + 1, part, sam, None))
            assert sorted((c[1], c[2]) for c in combos) == {1: [(1, 0)], 2: [(1, 0)], 4: [(0, 0), (1, 0)]}[cls], (cls, m, combos)
            if cls == 4:
                assert combos[0][0] == combos[1][0]
    ref, rows, rl, truth = _truth(3)
    n = len(rl)
    pp = pm.Params(pb.T_MIN_SPAN, pb.T_MAX_SPAN, pb.T_PENALTY, pm.RESCUE, pb.T_MAX_SPAN - pb.T_MIN_SPAN + rs)
    rz = pp.rescue_size
    for anchor_b in (True, False):                    # rule 17c: the representative, copy B in slot 1; rule 14c: the lowest mapped slot, copy A
        seg, sam, sec = _placed(truth, lambda m: [(truth[m][0][0] - d, 2, 12), (truth[m][0][0], 1, 0)], False)
        if anchor_b:
            req, tpos, _ = psm.rescue_rows(pp, K, rs, len(ref), n, rl, rows, seg, sam, sec)
        else:
            req, tpos, _ = pm.rescue_rows(pp, K, rs, len(ref), n, rl, rows, seg, sam)
        tried = [r for r in range(n) if req["pattern_len"][r]]
        assert tried == list(range(1, n, 2))
        pat, txt = np.zeros((len(tried), rz), dtype=np.uint8), np.zeros((len(tried), rz), dtype=np.uint8)
        for i, r in enumerate(tried):
            lo, tl = int(tpos[r]) & ~pm.MINUS_STRAND, int(req["text_len"][r])
            win = ref[lo:lo + tl]
            txt[i, :tl] = sdm.revcomp(win) if int(tpos[r]) >> 63 else win
            pat[i, :rs] = rows[r]
            inside = lo <= truth[r // 2][1][0] and truth[r // 2][1][1] <= lo + tl
            assert inside == anchor_b, (r, lo, tl, truth[r // 2])
        sc = efm.dp_scores(req[tried], pat, txt, mb.X, mb.O, mb.E, ends_free=(0, 0, rz, rz))
        assert (sc == 30 * mb.X).all() and 30 * mb.X <= pb.T3_MAX_SCORE if anchor_b else (sc > pb.T3_MAX_SCORE).all(), (anchor_b, sc.tolist())
