"""Colinear chaining of the seed hits without a GPU: the ABI values and symbols, every refusal of aim_seed_chain_device by message,
the properties of the rule as tests/chain_model.py writes it down (chains increase strictly in p and j and re-score to their f, the
trees partition the anchors, band 0 keeps a chain on one diagonal), that the shared test batches hold what can go wrong in a kernel
(ties, more anchors than the lookback, truncated strands, links with a gap, branching trees, an end that is not the last anchor), and
the code objects of the two new kernels."""
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
from chain_model import strand_stats  # noqa: E402

READ_SIZE = 128
# (k, stride, w, max_occ, band, flank, min_votes, K): the rows of tests/pipeline_batches.py at read_size 128
ROWS = [(11, 1, None, 8, 8, 8, 2, 4), (8, 1, None, 64, 48, 16, 3, 16), (14, 3, None, 1, 16, 8, 1, 8), (11, 4, None, 2, 0, 0, 1, 1),
        (11, 1, 5, 8, 32, 8, 2, 4), (13, 1, 10, 8, 32, 8, 2, 4), (8, 1, 2, 64, 48, 16, 3, 16)]


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
    import chain_model as cm
    assert _define("AIM_FEATURE_SEED_CHAIN") == capi.FEATURE_SEED_CHAIN == 0x4000
    assert engine.features() & capi.FEATURE_SEED_CHAIN
    assert _define("AIM_SEED_CHAIN_LOOKBACK") == capi.SEED_CHAIN_LOOKBACK == cm.LOOKBACK == 64
    assert _define("AIM_SEED_CHAIN_MAX_BAND") == capi.SEED_CHAIN_MAX_BAND == cm.MAX_BAND == 4096
    assert _lib().aim_seed_chain_kernel_names() == b"seed_chain_kernel,seed_chain_minimizer_kernel"
    assert _lib().aim_seed_kernel_name() == b"seed_candidates_kernel"            # the names that were there stay
    assert hasattr(_lib(), "aim_seed_chain_device") and callable(engine.seed_chain_device) and callable(engine.seed_chain_candidates)
    assert capi.CHAIN_DTYPE == cm.CHAIN and capi.CHAIN_DTYPE.itemsize == 16
    # aim_chain_t as a C compiler lays it out
    src = tmp_path / "c.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "aim_hip.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(aim_chain_t), offsetof(aim_chain_t, score), offsetof(aim_chain_t, n_anchors), offsetof(aim_chain_t, reserved), '
                   'offsetof(aim_chain_t, q_lo), offsetof(aim_chain_t, q_hi), offsetof(aim_chain_t, ref_span)); return 0; }\n')
    exe = tmp_path / "c"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [16] + [capi.CHAIN_DTYPE.fields[n][1] for n in ("score", "n_anchors", "reserved", "q_lo", "q_hi", "ref_span")]


GOOD = dict(k=11, stride=1, max_occ=8, band=8, flank=8, min_votes=2, max_cands=4, read_size=128)
BAD = [("k", 7, "k 7 is outside 8..14"), ("k", 15, "k 15 is outside 8..14"), ("stride", 0, "stride 0 must be >= 1"),
       ("max_occ", 0, "max_occ 0 must be >= 1"), ("band", -1, "band -1 must be >= 0"), ("flank", -1, "flank -1 must be >= 0"),
       ("min_votes", 0, "min_votes 0 must be >= 1"), ("max_cands", 0, "max_cands 0 is outside 1..16"),
       ("max_cands", 17, "max_cands 17 is outside 1..16"), ("read_size", 0, "read_size 0 must be"), ("read_size", 100, "read_size 100 must be"),
       ("read_size", 4104, "read_size 4104 must be"), ("band", 4097, "band 4097 is above 4096"), ("options", 2, "unknown options 0x2"),
       ("options", 0x2100, "unknown options 0x2100")]


def _call(sp, n_reads=4, ref_len=1000):
    """aim_seed_chain_device with NULL buffers: the parameter checks come first, with or without a device."""
    return _lib().aim_seed_chain_device(None if sp is None else C.byref(sp), n_reads, None, None, None, None, ref_len, None, None, None, None, None, None)


@pytest.mark.parametrize("field,value,msg", BAD, ids=["%s=%d" % b[:2] for b in BAD])
def test_every_bound_is_refused_by_name(field, value, msg):
    from aim_amd import capi, engine
    sp = engine.seed_params(**GOOD)
    setattr(sp, field, value)
    assert _call(sp) == capi.AIM_EINVAL and _err().startswith("aim_seed_params_t: " + msg), _err()


def test_other_refusals():
    from aim_amd import capi, engine
    sp = engine.seed_params(**GOOD)
    assert _call(None) == capi.AIM_EINVAL and _err() == "aim_seed_chain_device: sp is NULL"
    assert _call(sp, ref_len=capi.SEED_MAX_REF_LEN + 1) == capi.AIM_EINVAL and _err().startswith("aim_seed_chain_device: ref_len") and "2^32 - 2^25" in _err()
    assert _call(sp, n_reads=1 << 30) == capi.AIM_EINVAL and "aim_seed_chain_device: n_reads 1073741824 * max_cands 4 does not fit 32 bits" in _err()
    assert _call(sp) == capi.AIM_EINVAL and _err() == "aim_seed_chain_device: null device buffer"
    sp.band = 4096                                                              # the largest band gets past the parameter checks
    assert _call(sp) == capi.AIM_EINVAL and "null device buffer" in _err()
    spm = engine.seed_params(11, 128, w=5)
    assert _call(spm) == capi.AIM_EINVAL and "null device buffer" in _err()
    spm.stride = 2
    assert _call(spm) == capi.AIM_EINVAL and _err().startswith("aim_seed_params_t: stride 2 must be 1"), _err()
    # aim_seed_device keeps its contract: band has no upper bound there
    sp.band = 4097
    rc = _lib().aim_seed_device(C.byref(sp), 4, None, None, None, None, 1000, None, None, None, None, None)
    assert rc == capi.AIM_EINVAL and _err() == "aim_seed_device: null device buffer"
    with pytest.raises(capi.AimError) as e:
        engine.seed_chain_device(sp, 4, None, None, None, None, 1000, None, None, None, None)
    assert "band 4097" in str(e.value)


def test_cost_by_hand():
    import chain_model as cm
    k = 11
    assert [int(cm.cost(g, k)) for g in (0, 1, 2, 3, 4, 11, 12, 60, 200, 4096)] == [0, 0, 1, 1, 1, 2, 3, 8, 21, 358]
    # g = 12: (132 >> 7) + (4 >> 1) = 1 + 2; g = 4096, k = 14: 448 + (13 >> 1)
    assert int(cm.cost(4096, 14)) == 454


_BATCH = {}


def batch(row):
    """The model over seed_model's reference and 256 reads for one parameter row, once: (outputs, [(anchors, f, pred)] per strand)."""
    import chain_model as cm
    import minimizer_model as mm
    import seed_model as m
    if "data" not in _BATCH:
        ref = m.make_reference()
        _BATCH["data"] = (ref,) + m.make_reads(ref, 256, READ_SIZE)[:2]
    if row not in _BATCH:
        ref, rows, rl = _BATCH["data"]
        k, stride, w, max_occ, band, flank, min_votes, K = row
        index = m.build_index(ref, k) if w is None else mm.build_index(ref, k, w)
        detail = []
        out = cm.seed_chain(rows, rl, index, len(ref), k, stride, w, max_occ, band, flank, min_votes, K, READ_SIZE, detail=detail)
        _BATCH[row] = (out, detail)
    return _BATCH[row]


def rescore(a, chain, k):
    """f of a chain's end from its links alone."""
    import chain_model as cm
    f = k
    for x, y in zip(chain, chain[1:]):
        d_p, d_q = a[y][0] - a[x][0], a[y][1] - a[x][1]
        f += min(d_p, d_q, k) - int(cm.cost(abs(d_p - d_q), k))
    return f


@pytest.mark.parametrize("row", ROWS, ids=[str(r) for r in ROWS])
def test_model_properties(row):
    import chain_model as cm
    import minimizer_model as mm
    import seed_model as m
    k, stride, w, max_occ, band = row[:5]
    out, detail = batch(row)
    ref, rows, rl = _BATCH["data"]
    index = m.build_index(ref, k) if w is None else mm.build_index(ref, k, w)
    n_chains = 0
    for sr, (a, f, pred) in enumerate(detail):
        n = len(a)
        assert len(set(a)) == n and a == sorted(a) and n <= m.MAX_HITS               # distinct pairs, sorted by (p, j)
        if sr < 64:     # rules 1-3 are the seeding models': the same hits, as their diagonal keys
            read = np.asarray(rows[sr // 2][:rl[sr // 2]], dtype=np.uint8)
            q = m.revcomp(read) if sr % 2 else read
            kept, trunc = cm.anchors(q, *index, k, stride, w, max_occ)
            want = m.strand_hits(q, *index, k, stride, max_occ, READ_SIZE) if w is None else mm.strand_hits(q, *index, k, w, max_occ, READ_SIZE)[:2]
            assert ([p + READ_SIZE - j for p, j in kept], trunc) == tuple(want)
        if not n:
            continue
        assert (f >= k).all() and (f <= m.MAX_HITS * 14).all()
        linked = np.nonzero(pred >= 0)[0]
        assert (pred[linked] < linked).all() and (linked - pred[linked] <= cm.LOOKBACK).all() and (f[linked] > k).all() and (f[pred < 0] == k).all()
        root, depth, ends = cm.trees(f, pred)
        # the trees partition the anchors: every anchor has one root, which is a root, and the tree sizes add up
        assert (pred[root] < 0).all() and set(root.tolist()) == set(np.nonzero(pred < 0)[0].tolist()) == set(ends)
        assert sum(int((root == t).sum()) for t in ends) == n
        for t, e in ends.items():
            members = np.nonzero(root == t)[0]
            assert f[e] == f[members].max() and e == members[f[members] == f[e]].min()
            chain = cm.path(pred, e)
            assert chain[0] == t and len(chain) == depth[e]
            pts = [a[i] for i in chain]
            assert all(x[0] < y[0] and x[1] < y[1] for x, y in zip(pts, pts[1:]))     # strictly increasing in p and j
            assert all(abs((y[0] - x[0]) - (y[1] - x[1])) <= band for x, y in zip(pts, pts[1:]))
            assert rescore(a, chain, k) == f[e]
            if band == 0:
                assert len({p - j for p, j in pts}) == 1
            n_chains += 1
    assert n_chains > 100
    req, tpos, votes, seeds, chains = out
    K = row[7]
    assert (seeds["n_cands"] <= K).all() and (chains["reserved"] == 0).all()
    for r in range(len(rl)):
        got = chains[r * K:(r + 1) * K]
        nc = int(seeds["n_cands"][r])
        assert (got[nc:].view(np.uint8) == 0).all() and (got["score"][:nc] >= k).all() and (np.diff(got["score"][:nc].astype(np.int64)) <= 0).all()
        assert (got["q_lo"][:nc] + k <= got["q_hi"][:nc]).all() and (got["q_hi"][:nc] <= rl[r]).all()
        assert (votes[r * K:(r + 1) * K] == got["score"]).all()


def test_batches_hold_what_can_go_wrong():
    """Counted on the model: the kernels are compared with it on these batches, so the batches have to contain the cases."""
    import seed_model as m
    stats = {}
    for row in ROWS[:2] + ROWS[4:5]:
        k, band = row[0], row[4]
        out, detail = batch(row)
        n = np.array([len(d[0]) for d in detail])
        total = dict(over_lookback=int((n > 64).sum()), truncated=int((out[3]["flags"] & m.TRUNCATED).sum()), full=int((n == m.MAX_HITS).sum()),
                     branching=0, gap_links=0, end_not_last=0, ties=0)
        for d in detail:
            if len(d[0]):
                for key, v in strand_stats(d, k, band, len(d[0]) <= 300).items():
                    total[key] += v
        stats[row] = total
        print(row, total)
    a, b, c = (stats[r] for r in ROWS[:2] + ROWS[4:5])
    assert a["over_lookback"] >= 100 and b["over_lookback"] >= 100          # reads with more anchors than the lookback
    assert b["truncated"] >= 4 and b["full"] >= 4                             # strands that overflow AIM_SEED_MAX_HITS
    assert all(s["ties"] >= 100 for s in (a, b, c))                           # ties among the best predecessors
    assert all(s["gap_links"] >= 1 for s in (a, b, c))                        # links with g > 0
    assert b["branching"] >= 4                                                # one anchor chosen by two successors
    assert b["end_not_last"] >= 1                                             # a chain that ends before its tree's last anchor


def test_seed_chain_kernels_code_objects():
    """Each new kernel exists exactly once, uses no scratch and no static LDS and stays within kSeedChainMaxVgpr; the kernels that
    were there are still there, once each."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_regs
    lib = os.path.join(ROOT, "aim_amd", "libaim_hip.so")
    if not os.path.exists(lib):
        pytest.fail("libaim_hip.so is missing: run the build")
    regs = codeobj_regs.kernel_regs(lib)
    names = _lib().aim_seed_chain_kernel_names().decode().split(",")
    assert names == ["seed_chain_kernel", "seed_chain_minimizer_kernel"]
    bound = int(re.search(r"constexpr int kSeedChainMaxVgpr = (\d+);", open(os.path.join(ROOT, "aim_amd", "csrc", "seed_chain.hpp")).read()).group(1))
    for name in names:
        found = [n for n in regs if re.search(r"\baim::%s\(" % name, n)]
        assert len(found) == 1, (name, found)
        r = regs[found[0]]
        assert r["scratch_bytes"] == 0 and r["lds_static_bytes"] == 0, (name, r)
        assert 0 < r["vgpr"] + r["agpr"] <= bound <= 512 // 4, (name, r, bound)
    assert len([n for n in regs if "aim::seed_candidates_kernel" in n]) == 1 and len([n for n in regs if "aim::seed_minimizer_kernel" in n]) == 1
