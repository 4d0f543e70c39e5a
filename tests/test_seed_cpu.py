"""Device-side seeding without a GPU: the ABI values and layouts, aim_index_build against the model's index (any thread count),
aim_index_sizes, aim_seed_groups_offsets, every refusal by message, properties of the rule that hold by construction (checked on the
model, tests/seed_model.py), and the kernel's code object."""
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


def _lib():
    from aim_amd import capi
    return capi.load()


def _err():
    return _lib().aim_last_error().decode()


def _define(name):
    m = re.search(r"#define\s+%s\s+(\S+)" % name, open(HEADER).read())
    return int(m.group(1).rstrip("uUlL"), 0)


@pytest.fixture(scope="module")
def reference():
    import seed_model as m
    return m.make_reference()


@pytest.fixture(scope="module")
def model_index(reference):
    import seed_model as m
    return {k: m.build_index(reference, k) for k in (8, 11)}


def test_constants_and_feature_bit():
    from aim_amd import capi, engine
    import seed_model as m
    assert _define("AIM_ABI_VERSION") == 2 == _lib().aim_abi_version()
    assert _define("AIM_FEATURE_SEED") == capi.FEATURE_SEED == 0x800
    assert _define("AIM_SEED_MAX_CANDS") == capi.SEED_MAX_CANDS == 16
    assert _define("AIM_SEED_MAX_HITS") == capi.SEED_MAX_HITS == m.MAX_HITS == 1024
    assert _define("AIM_SEED_TRUNCATED") == capi.SEED_TRUNCATED == m.TRUNCATED == 1
    assert _define("AIM_SEED_MAX_READ_SIZE") == capi.SEED_MAX_READ_SIZE == 4096
    assert _define("AIM_SEED_MAX_REF_LEN") == capi.SEED_MAX_REF_LEN == 2 ** 32 - 2 ** 25
    assert engine.features() & capi.FEATURE_SEED
    assert _lib().aim_seed_kernel_name() == b"seed_candidates_kernel"
    assert capi.SEED_DTYPE == m.SEED and capi.REQUEST_DTYPE == m.REQUEST


def test_struct_layout(tmp_path):
    """aim_seed_params_t and aim_seed_t as ctypes / numpy and as a C compiler lay them out."""
    from aim_amd import capi
    names = [f[0] for f in capi.SeedParams._fields_]
    assert names == ["k", "stride", "max_occ", "band", "flank", "min_votes", "max_cands", "read_size", "idx_base", "options"]
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "aim_hip.h"\n'
                   'int main(void) { printf("%zu %zu", sizeof(aim_seed_params_t), sizeof(aim_seed_t));\n'
                   + "".join('printf(" %%zu", offsetof(aim_seed_params_t, %s));\n' % n for n in names)
                   + 'printf(" %zu %zu %zu\\n", offsetof(aim_seed_t, n_cands), offsetof(aim_seed_t, n_hits), offsetof(aim_seed_t, flags)); return 0; }\n')
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    want = [C.sizeof(capi.SeedParams), capi.SEED_DTYPE.itemsize] + [getattr(capi.SeedParams, n).offset for n in names]
    want += [capi.SEED_DTYPE.fields[n][1] for n in ("n_cands", "n_hits", "flags")]
    assert got == want and got[:2] == [40, 16]


def test_index_sizes():
    from aim_amd import capi, engine
    for k in range(8, 15):
        for ref_len in (0, k - 1, k, k + 1, 65536, capi.SEED_MAX_REF_LEN):
            assert engine.index_sizes(k, ref_len) == (4 ** k + 1, max(ref_len - k + 1, 0))
    be, pc = C.c_uint64(), C.c_uint64()
    for k in (7, 15, -1):
        assert _lib().aim_index_sizes(k, 100, C.byref(be), C.byref(pc)) == capi.AIM_EINVAL and "k %d is outside 8..14" % k in _err()
    assert _lib().aim_index_sizes(11, capi.SEED_MAX_REF_LEN + 1, C.byref(be), C.byref(pc)) == capi.AIM_EINVAL and "ref_len" in _err()
    assert _lib().aim_index_sizes(11, 100, None, None) == capi.AIM_EINVAL and "NULL" in _err()


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("k", [8, 11])
def test_index_build_equals_model(reference, model_index, k, threads):
    from aim_amd import engine
    bucket, pos = engine.build_index(reference, k, threads=threads)
    mb, mp = model_index[k]
    assert bucket.dtype == np.uint32 and pos.dtype == np.uint32 and len(bucket) == 4 ** k + 1
    assert np.array_equal(bucket, mb) and np.array_equal(pos, mp)
    # what the reference was built to hold: nothing indexed over the N run and the lower-case bases, the planted segment three times
    import seed_model as m
    assert len(pos) < len(reference) - k + 1 - (m.N_RUN[1] + m.LOWER[1])
    covered = np.zeros(len(reference), dtype=bool)
    covered[pos] = True
    assert not covered[m.N_RUN[0] - k + 1:m.N_RUN[0] + m.N_RUN[1]].any() and not covered[m.LOWER[0] - k + 1:m.LOWER[0] + m.LOWER[1]].any()
    if k == 11:
        code = int(m.kmer_codes(reference[m.PLANT_AT[0] + 100:m.PLANT_AT[0] + 100 + k], k)[0])
        assert set(at + 100 for at in m.PLANT_AT) <= set(pos[bucket[code]:bucket[code + 1]].tolist())


def test_index_build_at_the_short_end():
    """ref_len < k: no position; ref_len = k: one (or none when the k-mer holds another byte)."""
    import seed_model as m
    from aim_amd import capi, engine
    for k in (8, 11):
        for seq in (b"", b"ACGTACG", b"ACGTACGTACG"[:k], b"ACGTACGNACG"[:k], b"ACGTACGTACGT"[:k + 1]):
            for threads in (1, 4):
                bucket, pos = engine.build_index(seq, k, threads=threads)
                mb, mp = m.build_index(np.frombuffer(seq, dtype=np.uint8), k)
                assert np.array_equal(bucket, mb) and np.array_equal(pos, mp), (k, seq)
                assert len(pos) == (len(seq) - k + 1 if len(seq) >= k and b"N" not in seq else 0)
    bucket = np.zeros(4 ** 8 + 1, dtype=np.uint32)
    assert _lib().aim_index_build(None, 100, 8, capi.ptr(bucket), None, None, 1) == capi.AIM_EINVAL and "NULL" in _err()
    assert _lib().aim_index_build(b"ACGT", 4, 7, capi.ptr(bucket), None, None, 1) == capi.AIM_EINVAL and "k 7 is outside 8..14" in _err()


def test_seed_groups_offsets():
    from aim_amd import capi, engine
    for n, K in ((0, 1), (1, 16), (1000, 4), (7, 3)):
        assert np.array_equal(engine.seed_groups_offsets(n, K), np.arange(n + 1, dtype=np.uint32) * K)
    ro = np.zeros(4, dtype=np.uint32)
    for K in (0, 17):
        assert _lib().aim_seed_groups_offsets(3, K, capi.ptr(ro)) == capi.AIM_EINVAL and "K %d is outside 1..16" % K in _err()
    assert _lib().aim_seed_groups_offsets(3, 4, None) == capi.AIM_EINVAL and "NULL read_offsets" in _err()
    assert _lib().aim_seed_groups_offsets(1 << 30, 4, capi.ptr(ro)) == capi.AIM_EINVAL and "does not fit 32 bits" in _err()
    # the CSR is one aim_groups_check accepts
    ro = engine.seed_groups_offsets(50, 4)
    assert _lib().aim_groups_check(200, 50, capi.ptr(ro), None) == capi.AIM_OK


GOOD = dict(k=11, stride=1, max_occ=8, band=8, flank=8, min_votes=2, max_cands=4, read_size=128)
BAD = [("k", 7, "k 7 is outside 8..14"), ("k", 15, "k 15 is outside 8..14"), ("stride", 0, "stride 0 must be >= 1"),
       ("max_occ", 0, "max_occ 0 must be >= 1"), ("band", -1, "band -1 must be >= 0"), ("flank", -1, "flank -1 must be >= 0"),
       ("min_votes", 0, "min_votes 0 must be >= 1"), ("max_cands", 0, "max_cands 0 is outside 1..16"),
       ("max_cands", 17, "max_cands 17 is outside 1..16"), ("read_size", 0, "read_size 0 must be"), ("read_size", 100, "read_size 100 must be"),
       ("read_size", 4104, "read_size 4104 must be")]


@pytest.mark.parametrize("field,value,msg", BAD, ids=["%s=%d" % b[:2] for b in BAD])
def test_every_bound_is_refused_by_name(field, value, msg):
    from aim_amd import capi, engine
    sp = engine.seed_params(**GOOD)
    setattr(sp, field, value)
    nulls = (None,) * 4
    rc = _lib().aim_seed_device(C.byref(sp), 4, None, None, None, None, 1000, *nulls, None)
    assert rc == capi.AIM_EINVAL and _err().startswith("aim_seed_params_t: " + msg), _err()
    with pytest.raises(ValueError) as e:
        engine.seed_params(**dict(GOOD, **{field: value}))
    assert field in str(e.value)


def test_other_refusals():
    from aim_amd import capi, engine
    lib = _lib()
    sp = engine.seed_params(**GOOD)
    nulls = (None,) * 4
    sp.options = 2
    assert lib.aim_seed_device(C.byref(sp), 4, None, None, None, None, 1000, *nulls, None) == capi.AIM_EINVAL and "options 0x2" in _err()
    sp.options = 0
    assert lib.aim_seed_device(None, 4, None, None, None, None, 1000, *nulls, None) == capi.AIM_EINVAL and "sp is NULL" in _err()
    assert lib.aim_seed_device(C.byref(sp), 4, None, None, None, None, capi.SEED_MAX_REF_LEN + 1, *nulls, None) == capi.AIM_EINVAL
    assert "ref_len" in _err() and "2^32 - 2^25" in _err()
    assert lib.aim_seed_device(C.byref(sp), 1 << 30, None, None, None, None, 1000, *nulls, None) == capi.AIM_EINVAL
    assert "n_reads 1073741824 * max_cands 4 does not fit 32 bits" in _err()
    sp1 = engine.seed_params(**dict(GOOD, max_cands=1))
    assert lib.aim_seed_device(C.byref(sp1), 0xFFFFFFFF, None, None, None, None, 1000, *nulls, None) == capi.AIM_EINVAL    # (below 2^32: on to the buffers)
    assert "null device buffer" in _err()
    assert lib.aim_seed_device(C.byref(sp), 4, None, None, None, None, 1000, *nulls, None) == capi.AIM_EINVAL and "null device buffer" in _err()


def _params(**kw):
    p = dict(GOOD, **kw)
    return dict(k=p["k"], stride=p["stride"], max_occ=p["max_occ"], band=p["band"], flank=p["flank"], min_votes=p["min_votes"], K=p["max_cands"],
                read_size=p["read_size"])


@pytest.mark.parametrize("strand", [0, 1])
def test_model_error_free_read_finds_its_position(reference, model_index, strand):
    """An error-free read outside the planted repeat and the N run, stride 1: every one of its L - k + 1 seeds hits its true
    position on one diagonal, so candidate 0 has at least that many votes, the read's strand and a window over [p, p + L). The
    derivation needs every seed to be used: a k-mer that a random reference happens to hold more than max_occ times is skipped (about
    1.6 % of the 11-mers of 64 KiB occur twice), so the reads are drawn where no k-mer count exceeds max_occ -- a condition on the
    input, read from the index, and the only way max_occ = 1 can promise anything."""
    import seed_model as m
    rng = np.random.default_rng(3 + strand)
    k, L = 11, 100
    bucket = model_index[k][0].astype(np.int64)
    codes = m.kmer_codes(reference, k)
    for max_occ, min_votes, flank in ((1, 1, 0), (8, L - k + 1, 8), (64, 2, 12)):      # (L + 2 * flank <= read_size: text_len is capped there)
        for _ in range(12):
            while True:
                p = m.clean_position(rng, L)
                c = codes[p:p + L - k + 1]
                if (bucket[c + 1] - bucket[c] <= max_occ).all():
                    break
            read = reference[p:p + L]
            read = m.revcomp(read) if strand else read.copy()
            cands, n_hits, flags = m.seed_read(read, *model_index[k], len(reference), **_params(max_occ=max_occ, min_votes=min_votes, flank=flank))
            assert cands and flags == 0
            start, s, tlen, votes = cands[0]
            assert votes >= L - k + 1 and s == strand
            assert start <= p and p + L <= start + tlen and tlen <= 128
            assert start == max(p - flank, 0)


def test_model_repeat_copies_rank_by_position(reference, model_index):
    """A read inside the planted segment: with max_occ >= 3 its three copies are candidates with equal votes in position order; with
    max_occ = 2 every one of its seeds is skipped."""
    import seed_model as m
    k, L = 11, 100
    off = 60
    read = reference[m.PLANT_AT[0] + off:m.PLANT_AT[0] + off + L].copy()
    for max_occ in (3, 8):
        cands, n_hits, flags = m.seed_read(read, *model_index[k], len(reference), **_params(max_occ=max_occ, flank=0))
        assert len(cands) >= 3
        top = cands[:3]
        assert [c[0] for c in top] == [at + off for at in m.PLANT_AT] and all(c[1] == 0 for c in top)
        assert top[0][3] == top[1][3] == top[2][3] >= L - k + 1
    cands, n_hits, flags = m.seed_read(read, *model_index[k], len(reference), **_params(max_occ=2, flank=0, min_votes=1))
    assert n_hits[0] == 0 and all(c[1] == 1 for c in cands) and flags == 0    # (its reverse complement may still hit by chance)


def test_model_clusters_from_hand_written_keys():
    """Rule 4 on keys laid out by hand: maximal runs of the sorted keys with consecutive differences <= band."""
    import seed_model as m
    assert m.clusters([5, 1, 2, 9, 3, 20], 1) == [(3, 1, 3), (1, 5, 5), (1, 9, 9), (1, 20, 20)]
    assert m.clusters([5, 1, 2, 9, 3, 20], 4) == [(5, 1, 9), (1, 20, 20)]
    assert m.clusters([7, 7, 7], 0) == [(3, 7, 7)] and m.clusters([], 3) == []


def test_model_ranking_of_crafted_clusters_of_both_strands():
    """Rule 5 through seed_read, on an index written by hand so that the expected order can be too. The read AAACCCGGTA (L = 10,
    k = 8, stride 1) has three seeds per strand and its six 8-mers are distinct. A diagonal d gets one vote from seed j when the
    index holds position d + j for that seed's 8-mer. Strand 0: d = 500 and d = 200 with three votes each, d = 900 with two;
    strand 1: d = 100 with three, d = 700 with two, d = 50 with one. Votes descending, then strand ascending, then a_lo ascending."""
    import seed_model as m
    k, rs, L = 8, 32, 10
    read = np.frombuffer(b"AAACCCGGTA", dtype=np.uint8)
    plan = {0: {500: (0, 1, 2), 200: (0, 1, 2), 900: (0, 1)}, 1: {100: (0, 1, 2), 700: (1, 2), 50: (0,)}}
    at = {}
    for s, query in ((0, read), (1, m.revcomp(read))):
        codes = m.kmer_codes(query, k)
        for d, seeds in plan[s].items():
            for j in seeds:
                at.setdefault(int(codes[j]), []).append(d + j)
    assert len(at) == 6
    bucket = np.zeros(4 ** k + 1, dtype=np.uint32)
    for c, ps in at.items():
        bucket[c + 1] = len(ps)
    np.cumsum(bucket, out=bucket)
    pos = np.array([p for c in sorted(at) for p in sorted(at[c])], dtype=np.uint32)
    kw = dict(k=k, stride=1, max_occ=8, band=0, flank=0, read_size=rs)
    want = [(200, 0, L, 3), (500, 0, L, 3), (100, 1, L, 3), (900, 0, L, 2), (700, 1, L, 2)]
    cands, n_hits, flags = m.seed_read(read, bucket, pos, 2000, min_votes=2, K=8, **kw)
    assert cands == want and n_hits == [8, 6] and flags == 0
    assert m.seed_read(read, bucket, pos, 2000, min_votes=2, K=4, **kw)[0] == want[:4]
    assert m.seed_read(read, bucket, pos, 2000, min_votes=3, K=2, **kw)[0] == want[:2]
    assert m.seed_read(read, bucket, pos, 2000, min_votes=1, K=8, **kw)[0] == want + [(50, 1, L, 1)]


def test_seed_kernel_code_object():
    """No scratch, and VGPRs within the bound seed.hpp states (kSeedMaxVgpr) for its planned 3 wavefronts per SIMD."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_regs
    lib = os.path.join(ROOT, "aim_amd", "libaim_hip.so")
    if not os.path.exists(lib):
        pytest.fail("libaim_hip.so is missing: run the build")
    bound = int(re.search(r"constexpr int kSeedMaxVgpr = (\d+);", open(os.path.join(ROOT, "aim_amd", "csrc", "seed.hpp")).read()).group(1))
    assert bound <= 512 // 3
    regs = codeobj_regs.kernel_regs(lib)
    names = [n for n in regs if "aim::seed_candidates_kernel" in n]
    assert len(names) == 1, names
    r = regs[names[0]]
    assert r["scratch_bytes"] == 0 and r["lds_static_bytes"] == 0, r
    assert 0 < r["vgpr"] + r["agpr"] <= bound, r
