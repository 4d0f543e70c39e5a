"""tests/slot_padding.py on the models of rules 12c to 15c: a read's K slots followed by K' - K empty ones give every output byte of the
K slots alone, slot numbers renamed. The GPU modules say the same of the kernels, where K' also changes the lanes a read gets."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import slot_padding as sp  # noqa: E402

CIGAR_BASE, MD_BASE = 1000, 70000


def test_the_helper_itself():
    a = np.arange(1, 7, dtype=np.uint32)                         # two reads of three slots
    assert sp.pad(a, 3, 4, 2).tolist() == [1, 2, 3, 0, 4, 5, 6, 0] and sp.pad(a, 3, 5, 2, from_slot0=True).tolist() == [1, 2, 3, 1, 1, 4, 5, 6, 4, 4]
    own, rest = sp.unpad(sp.pad(a, 3, 5, 2, from_slot0=True), 3, 5, 2)
    assert own.tolist() == a.tolist() and rest.tolist() == [1, 1, 4, 4] and sp.pad(a, 3, 3, 2).tolist() == a.tolist()
    # read 1's slot 0 is 3, read 0's rescue index is 3 as well: the read decides
    assert sp.rename([3, 3, 5, sp.NONE, 6], [1, 0, 1, 1, 1], 3, 8).tolist() == [8, 8, 10, sp.NONE, 16]
    with pytest.raises(AssertionError):
        sp.rename([7], [1], 3, 8)


@pytest.mark.parametrize("K,K2", sp.PAIRS)
def test_map_records_and_contig_records(K, K2):
    import contig_model as cg
    import map_records_model as mm
    n = 65
    seg, sam, cls = mm.synthetic_tables(11, K, n)
    off, rec = mm.map_records(K, n, seg, sam, cls)
    off2, rec2 = mm.map_records(K2, n, sp.pad(seg, K, K2, n), sp.pad(sam, K, K2, n), sp.pad(cls, K, K2, n))
    assert off2.tobytes() == off.tobytes() and rec2.tobytes() == sp.records_renamed(rec, K, K2).tobytes()
    assert (np.diff(off.astype(np.int64)) > 1).any() or K == 1
    lens, starts, ref_len, d, o = cg.synthetic_clip(21, K, n, 3, seg["flags"])
    off, rec = cg.records(K, n, o["seg"], sam, cls, o["contig"], starts)
    off2, rec2 = cg.records(K2, n, sp.pad(o["seg"], K, K2, n), sp.pad(sam, K, K2, n), sp.pad(cls, K, K2, n), sp.pad(o["contig"], K, K2, n, from_slot0=True), starts)
    assert off2.tobytes() == off.tobytes() and rec2.tobytes() == sp.records_renamed(rec, K, K2).tobytes()
    assert (rec["sam"]["pad"] == cg.NONE).any() and (rec["sam"]["pad"] < 3).any()


def pair_outputs(pp, K, n, t):
    """Everything rule 14c and the record rules behind it give over the tables t, by name."""
    import contig_model as cg
    import map_records_model as mm
    import pair_model as pm
    rs = pm.READ_SIZE
    req, tpos, rows = pm.rescue_rows(pp, K, rs, t["ref_len"], n, t["read_len"], t["reads"], t["seg"], t["sam"], t["contig"], t["starts"], t["lens"])
    pairs, seg, sam, cls, contig = pm.select(pp, K, rs, n, t["read_len"], t["seg"], t["sam"], t["cls"], t["contig"], t["res_sam"], CIGAR_BASE, MD_BASE)
    off, rec = cg.records(K, n, seg, sam, cls, contig, t["starts"]) if contig is not None else mm.map_records(K, n, seg, sam, cls)
    rec2, mates = pm.mates(K, n, pairs, seg, sam, contig, t["starts"], off, rec)
    return dict(req=req, tpos=tpos, rows=rows, pairs=pairs, seg=seg, sam=sam, cls=cls, contig=contig, off=off, rec=rec2, mates=mates)


def same_after_renaming(K, K2, n, a, b, padded):
    """b, the outputs over the padded tables, against a, those over the tables themselves."""
    assert a["req"].tobytes() == b["req"].tobytes() and a["tpos"].tobytes() == b["tpos"].tobytes()
    assert sorted(a["rows"]) == sorted(b["rows"]) and all(a["rows"][r].tobytes() == b["rows"][r].tobytes() for r in a["rows"])
    assert b["pairs"].tobytes() == sp.pairs_renamed(a["pairs"], K, K2).tobytes()
    for k in ("seg", "sam", "cls", "contig"):
        if a[k] is None:
            continue
        own, rest = sp.unpad(b[k], K, K2, n)
        assert own.tobytes() == a[k].tobytes(), k
        assert rest.tobytes() == sp.unpad(padded[k], K, K2, n)[1].tobytes(), k             # apply leaves the empty slots as they were
    assert a["off"].tobytes() == b["off"].tobytes() and b["rec"].tobytes() == sp.records_renamed(a["rec"], K, K2).tobytes()
    assert a["mates"].tobytes() == b["mates"].tobytes()


@pytest.mark.parametrize("contigs", (False, True), ids=("one-seq", "contigs"))
@pytest.mark.parametrize("K,K2", sp.PAIRS)
def test_pairs(K, K2, contigs):
    import pair_model as pm
    n = 130
    t = pm.synthetic_tables(21, K, n, contigs)
    p = sp.pad_tables(t, K, K2, n)
    for pp in (pm.params(17, True), pm.params(17, False)):
        a, b = pair_outputs(pp, K, n, t), pair_outputs(pp, K2, n, p)
        same_after_renaming(K, K2, n, a, b, p)
    f = a["pairs"]["flags"]                                                                # (without rescue: proper combinations of mapped slots)
    assert (f & pm.PROPER).any() and not (f & (pm.RESCUED_A | pm.RESCUED_B)).any()
    f = pair_outputs(pm.params(17, True), K, n, t)["pairs"]["flags"]
    assert (f & (pm.RESCUED_A | pm.RESCUED_B)).any() and (a["pairs"]["slot"] == sp.NONE).any()


@pytest.mark.parametrize("contigs", (False, True), ids=("one-seq", "contigs"))
@pytest.mark.parametrize("K,K2", sp.PAIRS)
def test_pair_estimate(K, K2, contigs):
    import pair_estimate_model as em
    import pair_model as pm
    n = 130
    t = em.synthetic_tables(21, K, n, contigs)
    p = sp.pad_tables(t, K, K2, n)
    pp = pm.params(17, True)
    moved = 0
    for est_set in ((64, 1, 20, 16), (64, 1, 0, 100), (1024, 8, 20, 16), (8192, 8, 20, 16), (1024, 10 ** 6, 20, 16)):
        ep = em.EstParams(*est_set)
        e = em.estimate(pp, ep, K, pm.READ_SIZE, n, t["seg"], t["sam"], t["cls"], t["contig"])
        e2 = em.estimate(pp, ep, K2, pm.READ_SIZE, n, p["seg"], p["sam"], p["cls"], p["contig"])
        assert e.tobytes() == e2.tobytes() and len(e.tobytes()) == 48, (est_set, e, e2)
        pe = em.params_with(pp, e)
        moved += (pe.min_span, pe.max_span) != (pm.MIN_SPAN, pm.MAX_SPAN)
        same_after_renaming(K, K2, n, pair_outputs(pe, K, n, t), pair_outputs(pe, K2, n, p), p)
    assert moved
