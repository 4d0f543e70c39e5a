"""Primary / secondary chains and MAPQ without a GPU: the ABI values, symbols and struct layouts, every refusal of the two entry points
by message, rules 8c and 9c by hand on tests/chain_class_model.py, the model's properties on the synthetic batch, that the shared
batches hold what can go wrong in a kernel, what the rules give on the chaining model's chains (chimeric reads, reads from the planted
copies, plain reads), and the code objects of the two new kernels."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aim_hip.h")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from pipeline_batches import model_chains, short_reads  # noqa: E402

# (k, stride, w, max_occ, band, flank, min_votes, K): the short-read rows the MAPQ tests run, at read_size 128
SHORT_ROWS = [(11, 1, None, 8, 8, 8, 2, 4), (11, 1, 5, 8, 32, 8, 2, 4), (13, 1, 10, 8, 32, 8, 2, 4)]
PLAIN_MAPQ = {SHORT_ROWS[0]: 51, SHORT_ROWS[1]: 60, SHORT_ROWS[2]: 60}     # the least chain MAPQ of a plain read, counted on the model


def _lib():
    from aim_amd import capi
    return capi.load()


def _err():
    return _lib().aim_last_error().decode()


def _define(name):
    m = re.search(r"#define\s+%s\s+(\S+)" % name, open(HEADER).read())
    return int(m.group(1).rstrip("uUlL"), 0)


def test_constants_symbols_and_feature_bit(tmp_path):
    from aim_amd import capi, engine
    import chain_class_model as ccm
    assert _define("AIM_FEATURE_CHAIN_CLASS") == capi.FEATURE_CHAIN_CLASS == 0x10000
    assert engine.features() & capi.FEATURE_CHAIN_CLASS
    assert _lib().aim_abi_version() == 2
    assert _define("AIM_CHAIN_MASK_DEFAULT") == capi.CHAIN_MASK_DEFAULT == ccm.MASK_DEFAULT == 128
    assert (_define("AIM_CHAIN_PRIMARY"), _define("AIM_CHAIN_SECONDARY"), _define("AIM_CHAIN_SUPPLEMENTARY")) == \
        (capi.CHAIN_PRIMARY, capi.CHAIN_SECONDARY, capi.CHAIN_SUPPLEMENTARY) == (ccm.PRIMARY, ccm.SECONDARY, ccm.SUPPLEMENTARY) == (1, 2, 4)
    assert tuple(_define("AIM_MAPQ_" + n) for n in ("UNMAPPED", "SECONDARY", "SUPPLEMENTARY", "PROPER")) == \
        (capi.MAPQ_UNMAPPED, capi.MAPQ_SECONDARY, capi.MAPQ_SUPPLEMENTARY, capi.MAPQ_PROPER) == \
        (ccm.UNMAPPED, ccm.MAPQ_SECONDARY, ccm.MAPQ_SUPPLEMENTARY, ccm.PROPER) == (1, 2, 4, 8)
    assert _lib().aim_chain_class_kernel_names() == b"chain_class_kernel,read_mapq_kernel"
    assert _lib().aim_seed_chain_kernel_names() == b"seed_chain_kernel,seed_chain_minimizer_kernel"      # the names that were there stay
    assert hasattr(_lib(), "aim_chain_classify_device") and hasattr(_lib(), "aim_read_mapq_device")
    assert callable(engine.chain_classify_device) and callable(engine.read_mapq_device) and callable(engine.chain_classify)
    assert capi.CHAIN_CLASS_DTYPE == ccm.CLASS and capi.READ_MAPQ_DTYPE == ccm.MAPQ and capi.BEST_DTYPE == ccm.BEST and capi.MATE_DTYPE == ccm.MATE
    # both structs as a C compiler lays them out
    src = tmp_path / "c.c"
    cls_f, mq_f = ("sub_score", "parent", "flags", "mapq", "n_sub"), ("slot", "mapq", "chain_mapq", "aln_mapq", "flags")
    fmt = " ".join(["%zu"] * (2 + len(cls_f) + len(mq_f)))
    args = ", ".join(["sizeof(aim_chain_class_t)"] + ["offsetof(aim_chain_class_t, %s)" % f for f in cls_f] +
                     ["sizeof(aim_read_mapq_t)"] + ["offsetof(aim_read_mapq_t, %s)" % f for f in mq_f])
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "aim_hip.h"\nint main(void) { printf("%s\\n", %s); return 0; }\n' % (fmt, args))
    exe = tmp_path / "c"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [8] + [capi.CHAIN_CLASS_DTYPE.fields[f][1] for f in cls_f] + [8] + [capi.READ_MAPQ_DTYPE.fields[f][1] for f in mq_f]


def _classify(K=4, read_size=128, mask_q8=128, n_reads=4):
    """aim_chain_classify_device with NULL buffers: the parameter checks come first, with or without a device."""
    return _lib().aim_chain_classify_device(K, read_size, mask_q8, n_reads, None, None, None, None, None, None)


def _mapq(K=4, n_reads=4, score_unit=1, mates=None):
    return _lib().aim_read_mapq_device(K, n_reads, score_unit, None, mates, None, None, None)


CLASSIFY_BAD = [(dict(K=0), "K 0 is outside 1..16"), (dict(K=17), "K 17 is outside 1..16"), (dict(mask_q8=0), "mask_q8 0 is outside 1..256"),
                (dict(mask_q8=257), "mask_q8 257 is outside 1..256"), (dict(read_size=0), "read_size 0 must be"),
                (dict(read_size=100), "read_size 100 must be"), (dict(read_size=65536), "read_size 65536 must be"),
                (dict(n_reads=1 << 30), "n_reads 1073741824 * K 4 does not fit 32 bits"), (dict(), "null device buffer")]
MAPQ_BAD = [(dict(K=0), "K 0 is outside 1..16"), (dict(K=17), "K 17 is outside 1..16"), (dict(n_reads=1 << 30), "n_reads 1073741824 * K 4 does not fit 32 bits"),
            (dict(score_unit=0), "score_unit 0 must be >= 1"), (dict(score_unit=-3), "score_unit -3 must be >= 1"),
            (dict(n_reads=5, mates=1), "n_reads 5 is odd with d_mates"), (dict(), "null device buffer"), (dict(mates=1), "null device buffer")]


@pytest.mark.parametrize("kw,msg", CLASSIFY_BAD, ids=[m for _, m in CLASSIFY_BAD])
def test_classify_refusals(kw, msg):
    from aim_amd import capi
    assert _classify(**kw) == capi.AIM_EINVAL and _err().startswith("aim_chain_classify_device: " + msg), _err()


@pytest.mark.parametrize("kw,msg", MAPQ_BAD, ids=["%s %s" % (m, sorted(k)) for k, m in MAPQ_BAD])
def test_read_mapq_refusals(kw, msg):
    from aim_amd import capi
    assert _mapq(**kw) == capi.AIM_EINVAL and _err().startswith("aim_read_mapq_device: " + msg), _err()


def test_refusal_order_and_bounds_that_pass():
    """The null buffer is the last refusal; the largest legal values get that far; the Python layer raises with the message."""
    from aim_amd import capi, engine
    assert _classify(K=17, mask_q8=0, read_size=0) == capi.AIM_EINVAL and "K 17" in _err()
    assert _classify(mask_q8=0, read_size=0) == capi.AIM_EINVAL and "mask_q8 0" in _err()
    assert _classify(read_size=7, n_reads=1 << 30) == capi.AIM_EINVAL and "read_size 7" in _err()
    assert _classify(K=16, read_size=65528, mask_q8=256) == capi.AIM_EINVAL and _err() == "aim_chain_classify_device: null device buffer"
    assert _classify(K=1, mask_q8=1, read_size=8) == capi.AIM_EINVAL and "null device buffer" in _err()
    assert _mapq(score_unit=0, n_reads=5, mates=1) == capi.AIM_EINVAL and "score_unit 0" in _err()
    with pytest.raises(capi.AimError) as e:
        engine.chain_classify_device(4, 128, 300, 4, None, None, None, None, None)
    assert "mask_q8 300" in str(e.value)
    with pytest.raises(capi.AimError) as e:
        engine.read_mapq_device(4, 4, 0, None, None, None, None)
    assert "score_unit 0" in str(e.value)


def _one_read(cands, L=1000, K=None, read_size=1024, mask_q8=128, n_cands=None):
    """The model over one read whose candidates are (score, n_anchors, q_lo, q_hi, strand)."""
    import chain_class_model as ccm
    import chain_model as cm
    import seed_model as m
    K = K or len(cands)
    ch, tp, sd = np.zeros(K, dtype=cm.CHAIN), np.zeros(K, dtype=np.uint64), np.zeros(1, dtype=m.SEED)
    for i, (score, na, lo, hi, s) in enumerate(cands):
        ch[i] = (score, na, 0, lo, hi, abs(hi - lo))
        tp[i] = np.uint64(1000 + (s << 63))
    sd["n_cands"] = len(cands) if n_cands is None else n_cands
    return ccm.classify(K, read_size, mask_q8, np.array([L], dtype=np.int32), tp, sd, ch)


def test_rule_8c_by_hand():
    import chain_class_model as ccm
    P, S, X = ccm.PRIMARY, ccm.SECONDARY, ccm.SUPPLEMENTARY
    # the exact threshold overlaps: ov = 100 of min(len) = 200 at mask 128; one base less does not
    c = _one_read([(90, 12, 0, 300, 0), (50, 5, 200, 400, 0)])
    assert c["flags"].tolist() == [P, S] and c["parent"].tolist() == [0, 0] and c["sub_score"].tolist() == [50, 0] and c["n_sub"].tolist() == [1, 0]
    c = _one_read([(90, 12, 0, 300, 0), (50, 5, 201, 401, 0)])
    assert c["flags"].tolist() == [P, P | X] and c["parent"].tolist() == [0, 1] and c["sub_score"].tolist() == [0, 0]
    # mask 256: containment only; mask 1: one base of 256 is enough, one of 257 is not
    assert _one_read([(90, 12, 0, 300, 0), (50, 5, 100, 300, 0)], mask_q8=256)["flags"].tolist() == [P, S]
    assert _one_read([(90, 12, 0, 300, 0), (50, 5, 101, 301, 0)], mask_q8=256)["flags"].tolist() == [P, P | X]
    assert _one_read([(90, 12, 0, 300, 0), (50, 5, 299, 555, 0)], mask_q8=1)["flags"].tolist() == [P, S]
    assert _one_read([(90, 12, 0, 300, 0), (50, 5, 299, 556, 0)], mask_q8=1)["flags"].tolist() == [P, P | X]
    # a candidate that overlaps two primaries takes the lower one
    c = _one_read([(90, 12, 0, 300, 0), (80, 12, 400, 700, 0), (30, 4, 100, 600, 0)])
    assert c["flags"].tolist() == [P, P | X, S] and c["parent"].tolist() == [0, 1, 0] and c["sub_score"].tolist() == [30, 0, 0]
    # overlap with a secondary alone leaves a candidate primary
    c = _one_read([(90, 12, 0, 300, 0), (80, 12, 100, 500, 0), (30, 4, 400, 600, 0)])
    assert c["flags"].tolist() == [P, S, P | X] and c["parent"].tolist() == [0, 0, 2]
    # the strand-1 interval is mirrored with the clamped L: [L - 300, L) against [700, 1000) overlaps at L = 1000 only
    assert _one_read([(90, 12, 700, 1000, 0), (50, 5, 0, 300, 1)], L=1000)["flags"].tolist() == [P, S]
    assert _one_read([(90, 12, 700, 1000, 0), (50, 5, 0, 300, 1)], L=600)["flags"].tolist() == [P, P | X]
    assert _one_read([(90, 12, 724, 1024, 0), (50, 5, 0, 300, 1)], L=5000)["flags"].tolist() == [P, S]        # clamped to read_size 1 024
    assert _one_read([(90, 12, 0, 300, 0), (50, 5, 0, 300, 1)], L=-7)["flags"].tolist() == [P, P | X]         # clamped to 0: [-300, 0)
    # a malformed chain overlaps nothing; the slots from n_cands on are empty
    assert _one_read([(90, 12, 0, 300, 0), (50, 5, 200, 100, 0), (40, 5, 0, 300, 0)])["parent"].tolist() == [0, 1, 0]
    c = _one_read([(90, 12, 0, 300, 0), (50, 5, 0, 300, 0), (40, 5, 0, 300, 0)], n_cands=2)
    assert c[2].tobytes() == bytes(8) and c["n_sub"].tolist() == [1, 0, 0]
    assert _one_read([(90, 12, 0, 300, 0), (50, 5, 0, 300, 0)], K=2, n_cands=9)["flags"].tolist() == [P, S]   # n_cands above K counts as K
    # chain MAPQ: 60 (f2 = 0, m >= 10), 0 (f2 = f1), 18 (f2 = 0, n_anchors = 3), and the integer division
    assert _one_read([(90, 10, 0, 300, 0)])["mapq"].tolist() == [60]
    assert _one_read([(90, 12, 0, 300, 0), (90, 12, 0, 300, 0)])["mapq"].tolist() == [0, 0]
    assert _one_read([(90, 3, 0, 300, 0)])["mapq"].tolist() == [18]
    assert _one_read([(100, 12, 0, 300, 0), (15, 2, 0, 300, 0)])["mapq"].tolist() == [51, 0]
    assert _one_read([(7, 7, 0, 300, 0), (3, 2, 0, 300, 0)])["mapq"].tolist() == [24, 0]                     # 6 * 7 * 4 // 7
    assert _one_read([(0, 12, 0, 300, 0)])["mapq"].tolist() == [0]                                            # f1 = 0
    assert _one_read([(10, 12, 0, 300, 0), (20, 12, 0, 300, 0)])["mapq"].tolist() == [0, 0]                   # f2 > f1 (not a chain kernel's order)
    assert ccm.chain_mapq(0xFFFFFFFF, 1, 30) == 59 and ccm.chain_mapq(0xFFFFFFFF, 0, 30) == 60


def test_rule_9c_by_hand():
    import chain_class_model as ccm
    K = 4
    cls = np.zeros(4 * K, dtype=ccm.CLASS)
    cls[0:3] = [(40, 0, ccm.PRIMARY, 33, 1), (0, 0, ccm.SECONDARY, 0, 0), (0, 2, ccm.PRIMARY | ccm.SUPPLEMENTARY, 60, 0)]      # read 0
    cls[4] = (0, 0, ccm.PRIMARY, 12, 0)                                                                                          # read 1
    cls[8] = (0, 0, ccm.PRIMARY, 50, 0)                                                                                          # read 2; read 3 has none
    M = ccm.INT32_MAX

    def one(r, row, score_unit=1, mates=None):
        best = np.zeros(4, dtype=ccm.BEST)
        best["best_pair"] = ccm.NONE
        best[r] = row
        return tuple(int(x) for x in ccm.read_mapq(K, score_unit, best, mates, cls)[r])
    assert one(0, (0, 10, 40, 1)) == (0, 33, 33, 60, 0)                       # min(chain, aln)
    assert one(0, (0, 10, 13, 1)) == (0, 18, 33, 18, 0)
    assert one(0, (0, 10, 13, 1), score_unit=4) == (0, 4, 33, 4, 0)           # 18 // 4
    assert one(0, (0, 10, 10, 2)) == (0, 0, 33, 0, 0)                         # a tie
    assert one(0, (0, 10, M, 1)) == (0, 33, 33, 60, 0)                        # no second candidate
    assert one(0, (0, -200, -190, 1), score_unit=3) == (0, 20, 33, 20, 0)     # negative scores: only the difference counts
    assert one(0, (0, -200, -205, 1)) == (0, 0, 33, 0, 0)                     # max(s2 - b, 0)
    assert one(0, (1, 10, M, 1)) == (1, 33, 33, 60, ccm.MAPQ_SECONDARY)       # the secondary answers with its primary's ambiguity
    assert one(0, (2, 10, M, 1)) == (2, 60, 60, 60, ccm.MAPQ_SUPPLEMENTARY)
    assert one(0, (3, 10, M, 1)) == (3, 0, 0, 0, ccm.UNMAPPED)                # an empty slot
    assert one(0, (ccm.NONE, M, M, 0)) == (ccm.NONE, 0, 0, 0, ccm.UNMAPPED)
    assert one(0, (4, 10, M, 1)) == (4, 0, 0, 0, ccm.UNMAPPED)                # another read's slot
    assert one(1, (0, 10, M, 1)) == (0, 0, 0, 0, ccm.UNMAPPED)                # ... also below the read's own (unsigned difference)
    # mates: the pair's evidence, and the better mate's anchoring
    mates = np.zeros(2, dtype=ccm.MATE)
    mates[0] = ([0, 4], 30, 36, 1, ccm.MATE_PROPER, [0, 0])
    mates[1] = ([8, ccm.NONE], 30, 31, 1, 0, [0, 0])
    best = np.zeros(4, dtype=ccm.BEST)
    best[:] = [(0, 10, 11, 1), (4, 10, M, 1), (8, 10, 12, 1), (ccm.NONE, M, M, 0)]
    got = [tuple(int(x) for x in row) for row in ccm.read_mapq(K, 1, best, mates, cls)]
    assert got[0] == (0, 33, 33, 36, ccm.PROPER) and got[1] == (4, 33, 12, 36, ccm.PROPER)      # max(33, 12) for both mates
    assert got[2] == (8, 12, 50, 12, 0) and got[3] == (ccm.NONE, 0, 0, 0, ccm.UNMAPPED)         # not proper: the read's own aim_best_t
    mates[0]["best_pair"] = [0, 7]                                                              # the mate is unmapped: it counts as 0
    assert tuple(int(x) for x in ccm.read_mapq(K, 1, best, mates, cls)[0]) == (0, 33, 33, 36, ccm.PROPER)
    mates[0]["best_pair"] = [7, 4]
    assert tuple(int(x) for x in ccm.read_mapq(K, 1, best, mates, cls)[0]) == (7, 0, 0, 0, ccm.UNMAPPED)


_SYN = {}


def synthetic16():
    """(the synthetic batch of 4 099 reads at K = 16, its classification at mask 128), once."""
    import chain_class_model as ccm
    if not _SYN:
        d = ccm.synthetic(1, 4099, 16)
        _SYN["v"] = (d, ccm.classify(16, ccm.SYN_READ_SIZE, 128, **d))
    return _SYN["v"]


def _intervals(d, r, K, n):
    import chain_class_model as ccm
    L = min(max(int(d["read_len"][r]), 0), ccm.SYN_READ_SIZE)
    c = d["chains"][r * K:r * K + n]
    return [ccm.interval(int(c["q_lo"][i]), int(c["q_hi"][i]), int(d["text_pos"][r * K + i]) >> 63, L) for i in range(n)]


def test_model_properties_and_what_the_batch_holds():
    """Every parent is a primary of lower or equal index, primaries do not overlap pairwise, a secondary overlaps its parent and no
    earlier primary. Counted on the same pass: the batch holds the cases the GPU tests rely on."""
    import chain_class_model as ccm
    d, cls = synthetic16()
    K = 16
    count = dict(supplementary=0, deep_secondary=0, four_primaries=0, exact=0, mixed=0, above_k=0, empty=0, bad_len=0, malformed=0)
    for r in range(len(d["read_len"])):
        nc = int(d["seed"]["n_cands"][r])
        n = min(nc, K)
        c = cls[r * K:(r + 1) * K]
        iv = _intervals(d, r, K, n)
        strand = [int(d["text_pos"][r * K + i]) >> 63 for i in range(n)]
        assert c[n:].tobytes() == bytes(8 * (K - n))
        prim = [i for i in range(n) if c["flags"][i] & ccm.PRIMARY]
        assert all(c["flags"][i] in (ccm.PRIMARY, ccm.PRIMARY | ccm.SUPPLEMENTARY, ccm.SECONDARY) for i in range(n))
        assert all((c["flags"][i] == ccm.PRIMARY) == (i == 0) for i in prim)
        for i in range(n):
            p = int(c["parent"][i])
            assert p <= i and p in prim and (p == i) == (i in prim)
            if i not in prim:
                assert ccm.overlap(iv[i], iv[p], 128) and not any(ccm.overlap(iv[i], iv[j], 128) for j in prim if j < p)
                assert c["sub_score"][i] == 0 and c["n_sub"][i] == 0 and c["mapq"][i] == 0
                count["mixed"] += strand[i] != strand[p]
                ov = min(iv[i][1], iv[p][1]) - max(iv[i][0], iv[p][0])
                count["exact"] += 256 * ov == 128 * min(iv[i][1] - iv[i][0], iv[p][1] - iv[p][0])
        assert not any(ccm.overlap(iv[i], iv[j], 128) for i in prim for j in prim if j < i)
        assert sum(int(c["n_sub"][i]) for i in prim) == n - len(prim)
        count["supplementary"] += len(prim) > 1
        count["deep_secondary"] += sum(1 for i in range(n) if i not in prim and c["parent"][i] != 0)
        count["four_primaries"] += len(prim) >= 4
        count["above_k"] += nc > K
        count["empty"] += n < K
        count["bad_len"] += not 0 <= int(d["read_len"][r]) <= ccm.SYN_READ_SIZE
        count["malformed"] += sum(1 for a, b in iv if b <= a)
    print(count)
    assert all(v >= 20 for v in count.values()), count
    s = d["chains"]["score"].reshape(-1, K).astype(np.int64)
    assert all((np.diff(row[row > 0]) <= 0).all() for row in s)               # scores descend (the malformed zeros apart)
    assert len(set((cls["mapq"][cls["flags"] & ccm.PRIMARY != 0]).tolist())) >= 40


def test_synthetic_best_holds_what_can_go_wrong():
    import chain_class_model as ccm
    for K in (1, 4, 16):
        n = 1000
        best, mates = ccm.synthetic_best(3, n, K)
        own = (best["best_pair"].astype(np.int64) - np.arange(n) * K)
        assert (best["n_best"] > 1).sum() >= 20 and (best["second_score"] == ccm.INT32_MAX).sum() >= 20 and (best["best_score"] < 0).sum() >= 20
        assert (best["best_pair"] == ccm.NONE).sum() >= 20
        foreign = (best["best_pair"] != ccm.NONE) & ((own < 0) | (own >= K))
        assert foreign.sum() >= 20 and (best["best_pair"][foreign] < n * K).all()
        assert (mates["flags"] & ccm.MATE_PROPER).sum() >= 100 and (mates["flags"] == 0).sum() >= 100 and (mates["n_best"] > 1).sum() >= 10
        ok = mates["best_pair"].reshape(-1)
        assert (ok[ok != ccm.NONE] < n * K).all() and (ok == ccm.NONE).sum() >= 10


def test_chimeric_reads_have_two_primaries():
    """Each half of a chimeric read is a primary of its own, and the halves drawn around a planted copy have secondaries under a
    parent other than 0."""
    import chain_class_model as ccm
    rows, rl = ccm.chimeric_reads()
    K = ccm.CHIMERIC_ROW[7]
    req, tpos, votes, seeds, chains = model_chains("chimeric", ccm.CHIMERIC_ROW, rows, rl, ccm.CHIMERIC_SIZE)
    cls = ccm.classify(K, ccm.CHIMERIC_SIZE, 128, rl, tpos, seeds, chains)
    fl, parent = cls["flags"].reshape(-1, K), cls["parent"].reshape(-1, K)
    primaries = ((fl & ccm.PRIMARY) != 0).sum(axis=1)
    secondary = (fl & ccm.SECONDARY) != 0
    print("primaries", primaries.tolist(), "secondaries", int(secondary.sum()), "under a parent other than 0", int((secondary & (parent != 0)).sum()))
    assert len(rl) == 32 and (primaries >= 2).all()
    assert (secondary & (parent != 0)).sum() >= 1
    # the two primaries are the two halves: together they cover most of the read, and they barely overlap
    for r in range(32):
        L = int(rl[r])
        iv = [ccm.interval(int(chains["q_lo"][r * K + i]), int(chains["q_hi"][r * K + i]), int(tpos[r * K + i]) >> 63, L) for i in range(2)]
        assert sum(b - a for a, b in iv) >= 0.8 * L and min(iv[0][1], iv[1][1]) - max(iv[0][0], iv[1][0]) < 40


@pytest.mark.parametrize("row", SHORT_ROWS, ids=[str(r) for r in SHORT_ROWS])
def test_chain_mapq_on_the_model_chains(row):
    """A read from inside the planted segment has three equal chains: MAPQ 0 with sub_score == score. A plain read stands alone."""
    import chain_class_model as ccm
    K = row[7]
    rows, rl = ccm.planted_reads()
    req, tpos, votes, seeds, chains = model_chains("planted", row, rows, rl, ccm.PLANTED_SIZE)
    cls = ccm.classify(K, ccm.PLANTED_SIZE, 128, rl, tpos, seeds, chains)
    assert (seeds["n_cands"] >= 3).all() and (cls["flags"][0::K] == ccm.PRIMARY).all() and (cls["n_sub"][0::K] >= 2).all()
    assert (cls["mapq"][0::K] == 0).all() and (cls["sub_score"][0::K] == chains["score"][0::K]).all()
    assert ((cls["flags"][1::K] == ccm.SECONDARY) & (cls["flags"][2::K] == ccm.SECONDARY)).all()
    rows, rl, _, _, plain = short_reads()
    req, tpos, votes, seeds, chains = model_chains("short", row, rows, rl, 128)
    cls = ccm.classify(K, 128, 128, rl, tpos, seeds, chains)
    print(row, "plain reads", int(plain.sum()), "chain MAPQ", sorted(set(cls["mapq"][0::K][plain].tolist())))
    assert plain.sum() >= 20 and (cls["flags"][0::K][plain] == ccm.PRIMARY).all() and (cls["mapq"][0::K][plain] >= PLAIN_MAPQ[row]).all()


def test_chain_class_kernels_code_objects():
    """Each new kernel exists exactly once, uses no scratch and no LDS and stays within kChainClassMaxVgpr; the seed and chain kernels
    are still there, once each."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_regs
    lib = os.path.join(ROOT, "aim_amd", "libaim_hip.so")
    if not os.path.exists(lib):
        pytest.fail("libaim_hip.so is missing: run the build")
    regs = codeobj_regs.kernel_regs(lib)
    names = _lib().aim_chain_class_kernel_names().decode().split(",")
    assert names == ["chain_class_kernel", "read_mapq_kernel"]
    bound = int(re.search(r"constexpr int kChainClassMaxVgpr = (\d+);", open(os.path.join(ROOT, "aim_amd", "csrc", "chain_class.hpp")).read()).group(1))
    for name in names:
        found = [n for n in regs if re.search(r"\baim::%s\(" % name, n)]
        assert len(found) == 1, (name, found)
        r = regs[found[0]]
        assert r["scratch_bytes"] == 0 and r["lds_static_bytes"] == 0, (name, r)
        assert 0 < r["vgpr"] + r["agpr"] <= bound <= 512 // 8, (name, r, bound)
    for name in ("seed_candidates_kernel", "seed_minimizer_kernel", "seed_chain_kernel", "seed_chain_minimizer_kernel", "seed_chain_long_kernel"):
        assert len([n for n in regs if re.search(r"\baim::%s\(" % name, n)]) == 1, name
