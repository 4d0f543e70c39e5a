"""(w, k) minimizers without a GPU: the ABI values and every new refusal by message, aim_index_build_minimizers against the rule as
tests/minimizer_model.py writes it down (window definition; any thread count; w = 1 is aim_index_build), the local test the kernels use
against the window definition, the guarantee (an exact match of w + k - 1 bases shares a seed), the density, and the code objects of the
two new kernels."""
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

KS, WS = (8, 11, 14), (1, 2, 5, 16, 32)


def _lib():
    from aim_amd import capi
    return capi.load()


def _err():
    return _lib().aim_last_error().decode()


def _define(name):
    m = re.search(r"#define\s+%s\s+(\S+)" % name, open(HEADER).read())
    return int(m.group(1).rstrip("uUlL"), 0)


def acgt(rng, n):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)].copy()


def test_constants_and_feature_bit(tmp_path):
    from aim_amd import capi, engine
    import minimizer_model as mm
    assert _define("AIM_ABI_VERSION") == 2 == _lib().aim_abi_version()
    assert _define("AIM_FEATURE_MINIMIZERS") == capi.FEATURE_MINIMIZERS == 0x2000
    assert _define("AIM_SEED_MAX_W") == capi.SEED_MAX_W == mm.MAX_W == 32
    assert engine.features() & capi.FEATURE_MINIMIZERS
    assert _lib().aim_minimizer_kernel_names() == b"index_minimizer_kernel,seed_minimizer_kernel"
    # the names that were there stay what they were
    assert _lib().aim_seed_kernel_name() == b"seed_candidates_kernel"
    assert _lib().aim_index_kernel_names().decode().split(",")[0] == "index_code_kernel" and b"minimizer" not in _lib().aim_index_kernel_names()
    # the macro as a C compiler expands it, and the struct it travels in
    src = tmp_path / "opt.c"
    src.write_text('#include <stdio.h>\n#include "aim_hip.h"\nint main(void) { printf("%u %u %u %zu\\n", AIM_SEED_OPT_MINIMIZERS(1), '
                   'AIM_SEED_OPT_MINIMIZERS(19), AIM_SEED_OPT_MINIMIZERS(AIM_SEED_MAX_W), sizeof(aim_seed_params_t)); return 0; }\n')
    exe = tmp_path / "opt"
    subprocess.check_call(["gcc", "-std=c11", "-I" + os.path.join(ROOT, "include"), "-o", str(exe), str(src)])
    got = [int(x) for x in subprocess.check_output([str(exe)], text=True).split()]
    assert got == [capi.SEED_OPT_MINIMIZERS(1), capi.SEED_OPT_MINIMIZERS(19), capi.SEED_OPT_MINIMIZERS(32), 40] and got[:3] == [0x100, 0x1300, 0x2000]
    sp = engine.seed_params(11, 128, w=19)
    assert sp.options == 0x1300 and sp.stride == 1 and engine.seed_params(11, 128).options == 0


def test_the_order_key():
    """h by hand on a few codes, a bijection on a sample, and the one 32-bit value that hashes to 0xFFFFFFFF: it is no code of a
    k <= 14 (codes are below 4^14), so no valid k-mer's key equals the value an invalid one compares above."""
    import minimizer_model as mm

    def h1(x):
        x ^= x >> 16
        x = x * 0x85EBCA6B & 0xFFFFFFFF
        x ^= x >> 13
        x = x * 0xC2B2AE35 & 0xFFFFFFFF
        return x ^ (x >> 16)
    codes = np.array([0, 1, 2, 0xFFFF, 0x10000, 4 ** 14 - 1, 0x331DA083], dtype=np.uint64)
    assert mm.h(codes).tolist() == [h1(int(c)) for c in codes]
    assert h1(0) == 0 and h1(1) == 0x514E28B7 and h1(0x331DA083) == 0xFFFFFFFF and 0x331DA083 >= 4 ** 14
    sample = np.random.default_rng(0).integers(0, 4 ** 14, size=200000).astype(np.uint64)
    assert len(np.unique(mm.h(np.unique(sample)))) == len(np.unique(sample))
    assert mm.INVALID > 0xFFFFFFFF


def test_refusals_by_name():
    from aim_amd import capi, engine
    lib = _lib()
    bucket = np.zeros(4 ** 8 + 1, dtype=np.uint32)
    pos = np.zeros(64, dtype=np.uint32)
    seq = b"ACGTACGTACGTACGTACGT"
    for w in (0, 33, -1):
        assert lib.aim_index_build_minimizers(seq, len(seq), 8, w, capi.ptr(bucket), capi.ptr(pos), None, 1) == capi.AIM_EINVAL
        assert "w %d is outside 1..32" % w in _err()
        assert lib.aim_index_build_device_minimizers(0x10000, 1000, 11, w, 0x20000, 0x30000, 0x40000, 1 << 30, None) == capi.AIM_EINVAL
        assert "w %d is outside 1..32" % w in _err()
    assert lib.aim_index_build_minimizers(seq, len(seq), 7, 5, capi.ptr(bucket), capi.ptr(pos), None, 1) == capi.AIM_EINVAL and "k 7 is outside 8..14" in _err()
    assert lib.aim_index_build_minimizers(None, 100, 8, 5, capi.ptr(bucket), None, None, 1) == capi.AIM_EINVAL and "NULL" in _err()
    # the device build refuses what aim_index_build_device refuses, before a device is touched
    k, ref_len = 11, 1000
    sb = engine.index_device_scratch(k, ref_len)
    call = lambda *a: lib.aim_index_build_device_minimizers(*a, None)
    ref, d_b, d_p, scr = 0x10000, 0x20000, 0x30000, 0x40000
    assert call(ref, ref_len, 15, 5, d_b, d_p, scr, sb) == capi.AIM_EINVAL and "k 15 is outside 8..14" in _err()
    assert call(ref, capi.SEED_MAX_REF_LEN + 1, k, 5, d_b, d_p, scr, 1 << 40) == capi.AIM_EINVAL and "ref_len" in _err()
    assert call(ref, ref_len, k, 5, None, d_p, scr, sb) == capi.AIM_EINVAL and "d_bucket is NULL" in _err()
    assert call(ref, ref_len, k, 5, d_b, None, scr, sb) == capi.AIM_EINVAL and "d_pos is NULL" in _err()
    assert call(None, ref_len, k, 5, d_b, d_p, scr, sb) == capi.AIM_EINVAL and "d_reference is NULL" in _err()
    assert call(ref + 4, ref_len, k, 5, d_b, d_p, scr, sb) == capi.AIM_EINVAL and "not 16-byte aligned" in _err()
    assert call(ref, ref_len, k, 5, d_b, d_p, None, sb) == capi.AIM_EINVAL and "d_scratch is NULL" in _err()
    assert call(ref, ref_len, k, 5, d_b, d_p, scr + 128, sb) == capi.AIM_EINVAL and "not 256-byte aligned" in _err()
    assert call(ref, ref_len, k, 5, d_b, d_p, scr, sb - 1) == capi.AIM_EINVAL and "scratch_bytes %d is below the %d" % (sb - 1, sb) in _err()
    with pytest.raises(capi.AimError) as e:
        engine.index_build_minimizers(seq, 8, 0)
    assert "w 0 is outside 1..32" in str(e.value)


def test_seed_options():
    """options is 0 or AIM_SEED_OPT_MINIMIZERS(1..32); every other value is reported as `options 0x<value>`, 0x2 as before; stride
    must be 1 with minimizers. A good value gets past the parameter checks (to the NULL buffers)."""
    from aim_amd import capi, engine
    lib = _lib()
    nulls = (None,) * 4
    call = lambda sp: lib.aim_seed_device(C.byref(sp), 4, None, None, None, None, 1000, *nulls, None)
    for bad in (0x2, 0x1, 0x501, 0x0FF, 0x2100, 0x3F00, 0x4000, 0x4500, 0x10500, 0x80000500, 0xFFFFFFFF):
        sp = engine.seed_params(11, 128)
        sp.options = bad
        assert call(sp) == capi.AIM_EINVAL and _err() == "aim_seed_params_t: unknown options 0x%x" % bad, (hex(bad), _err())
    for w in (1, 5, 32):
        sp = engine.seed_params(11, 128, w=w)
        assert sp.options == w << 8
        assert call(sp) == capi.AIM_EINVAL and "null device buffer" in _err(), _err()
        sp.stride = 2
        assert call(sp) == capi.AIM_EINVAL and _err().startswith("aim_seed_params_t: stride 2 must be 1"), _err()
    sp = engine.seed_params(11, 128, stride=4)
    assert call(sp) == capi.AIM_EINVAL and "null device buffer" in _err()           # options 0: any stride, as before
    for kw, name in ((dict(w=0), "w"), (dict(w=33), "w"), (dict(w=2.5), "w"), (dict(w=5, stride=2), "stride")):
        with pytest.raises(ValueError) as e:
            engine.seed_params(11, 128, **kw)
        assert name in str(e.value)


_MODEL = {}


def model_case(k):
    """A reference per k (short for k = 14, whose bucket[] alone is 1 GiB) with an N run, lower-case bases, a homopolymer and a
    two-base repeat, made once."""
    if k not in _MODEL:
        rng = np.random.default_rng(100 + k)
        ref = acgt(rng, 3000 if k == 14 else 20000)
        ref[500:520] = ord("N")
        ref[900] = ord("N")
        ref[1200:1260] |= 0x20
        ref[1500:1600] = ord("A")
        ref[2000:2100] = np.tile(np.frombuffer(b"AC", dtype=np.uint8), 50)
        _MODEL[k] = ref
    return _MODEL[k]


@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("k", KS)
def test_host_build_equals_model(k, w):
    import minimizer_model as mm
    from aim_amd import engine
    ref = model_case(k)
    mb, mp = mm.build_index(ref, k, w)
    assert 0 < len(mp) <= len(ref) - k + 1 and mb[-1] == len(mp)
    for threads in (1, 7):
        bucket, pos = engine.index_build_minimizers(ref, k, w, threads=threads)
        assert bucket.dtype == np.uint32 and pos.dtype == np.uint32 and len(bucket) == 4 ** k + 1
        assert np.array_equal(pos, mp), (k, w, threads)
        assert np.array_equal(bucket, mb), (k, w, threads)
        del bucket
    if w == 1:      # every valid k-mer: the bytes of aim_index_build (and of seed_model's index)
        b1, p1 = engine.build_index(ref, k, threads=4)
        assert np.array_equal(b1, mb) and np.array_equal(p1, mp)


def test_w1_is_aim_index_build():
    """w = 1 on the seeding tests' own reference, byte for byte."""
    import seed_model as m
    from aim_amd import engine
    ref = m.make_reference()
    for k in (8, 11):
        b0, p0 = engine.build_index(ref, k, threads=3)
        b1, p1 = engine.index_build_minimizers(ref, k, 1, threads=5)
        assert b0.tobytes() == b1.tobytes() and p0.tobytes() == p1.tobytes()


def sequences(k, w):
    """What the local test is compared on: random sequences, poly-A, ACAC..., sequences with N runs, and every length 0 .. k + w + 2."""
    rng = np.random.default_rng(k * 100 + w)
    out = [acgt(rng, 400), acgt(rng, 3 * w + k), np.full(200, ord("A"), dtype=np.uint8), np.tile(np.frombuffer(b"AC", dtype=np.uint8), 100)]
    for _ in range(3):
        s = acgt(rng, 300)
        for _ in range(4):
            at, n = int(rng.integers(0, 290)), int(rng.integers(1, 2 * k))
            s[at:at + n] = ord("N")
        out.append(s)
    s = acgt(rng, 4)                                   # few distinct k-mers: many ties
    out.append(np.tile(s, 60))
    for n in range(0, k + w + 3):
        out += [acgt(rng, n), np.full(n, ord("A"), dtype=np.uint8)]
        if n > 2:
            s = acgt(rng, n)
            s[n // 2] = ord("N")
            out.append(s)
    return out


@pytest.mark.parametrize("k,w", [(8, 1), (8, 2), (8, 5), (11, 16), (8, 32), (14, 5)])
def test_local_test_equals_window_definition(k, w):
    """The kernels' formulation (L + R + 1 >= min(w, n)) selects exactly the window definition's positions -- and so does the
    library's host build, whose pos[] is that set."""
    import minimizer_model as mm
    from aim_amd import engine
    for seq in sequences(k, w):
        by_window, by_local = mm.selected(seq, k, w), mm.selected_local(seq, k, w)
        assert np.array_equal(by_window, by_local), (k, w, seq.tobytes())
        if k < 14:
            _, pos = engine.index_build_minimizers(seq, k, w, threads=2)
            assert np.array_equal(np.sort(pos), np.nonzero(by_window)[0]), (k, w, seq.tobytes())


@pytest.mark.parametrize("k,w", [(8, 1), (8, 5), (11, 16), (8, 32)])
def test_poly_a_selects_the_first_position_of_every_window(k, w):
    """All keys tie: the leftmost position of each window wins, so exactly 0 .. n - w are selected (position 0 alone below w)."""
    import minimizer_model as mm
    from aim_amd import engine
    for length in (k, k + 1, k + w - 2, k + w - 1, k + w, 150):
        if length < k:
            continue
        seq = np.full(length, ord("A"), dtype=np.uint8)
        n = length - k + 1
        want = np.arange(max(n - w, 0) + 1)
        assert np.array_equal(np.nonzero(mm.selected(seq, k, w))[0], want)
        assert np.array_equal(np.nonzero(mm.selected_local(seq, k, w))[0], want)
        bucket, pos = engine.index_build_minimizers(seq, k, w)
        assert np.array_equal(pos, want) and bucket[0] == 0 and (bucket[1:] == len(want)).all()


@pytest.fixture(scope="module")
def random_ref():
    return acgt(np.random.default_rng(77), 1 << 16)


@pytest.mark.parametrize("strand", [0, 1])
@pytest.mark.parametrize("k,w", [(11, 5), (11, 16), (11, 32), (8, 5)])
def test_the_guarantee(random_ref, k, w, strand):
    """An error-free substring of at least w + k - 1 bases: every window of the read is a window of the reference, so every selected
    read offset j has p + j in the index under its code, and with band 0 the diagonal of p collects exactly one vote per seed. The
    reads are drawn where that is all that happens -- every seed's code has at most max_occ positions, nothing is truncated, and no
    other diagonal of either strand collects as many votes (a k-mer that occurs twice in the reference could tie a read with one
    seed) -- conditions on the input, checked here."""
    import minimizer_model as mm
    import seed_model as m
    ref = random_ref
    bucket, pos = mm.build_index(ref, k, w)
    rng = np.random.default_rng(1000 * k + 10 * w + strand)
    rs, max_occ = 128, 64
    kw = dict(k=k, w=w, max_occ=max_occ, band=0, flank=0, min_votes=1, K=4, read_size=rs)
    done = 0
    for L in (w + k - 1, w + k - 1, w + k, 100, 100, 100, 128):
        if L < w + k - 1:
            continue
        for _ in range(200):
            p = int(rng.integers(0, len(ref) - L))
            piece = ref[p:p + L]
            read = m.revcomp(piece) if strand else piece.copy()
            same, other = (m.revcomp(read) if strand else read), (read if strand else m.revcomp(read))
            codes = m.kmer_codes(same, k)
            js = np.nonzero(mm.selected(same, k, w))[0]
            counts = bucket[codes[js] + 1].astype(np.int64) - bucket[codes[js]]
            rivals = [c for c in m.clusters(mm.strand_hits(same, bucket, pos, k, w, max_occ, rs)[0], 0) if c[1] != p + rs]
            rivals += m.clusters(mm.strand_hits(other, bucket, pos, k, w, max_occ, rs)[0], 0)
            if (counts <= max_occ).all() and max([c[0] for c in rivals] + [0]) < len(js):
                break
        else:
            pytest.fail("no read drawn")
        assert len(js) >= 1
        for j in js:                                   # the guarantee itself
            c = int(codes[j])
            assert p + j in pos[bucket[c]:bucket[c + 1]].tolist(), (k, w, p, j)
        cands, n_hits, flags = mm.seed_read(read, bucket, pos, len(ref), **kw)
        assert flags == 0 and n_hits[strand] == int(counts.sum())               # nothing skipped, nothing truncated
        start, s, tlen, votes = cands[0]
        assert s == strand and votes == len(js) and start == p and tlen == L, (k, w, L, cands[0], len(js))
        done += 1
    assert done >= 4


def test_density(random_ref):
    """n_pos is below half of the valid positions from w = 5 on (random sequence keeps about 2 / (w + 1); the README records the
    ratios measured here)."""
    from aim_amd import engine
    k = 11
    valid = len(engine.build_index(random_ref, k)[1])
    assert valid == len(random_ref) - k + 1
    for w in (1, 2, 5, 10, 16, 19, 32):
        n_pos = len(engine.index_build_minimizers(random_ref, k, w)[1])
        print("density k=%d w=%d n_pos=%d ratio=%.4f 2/(w+1)=%.4f" % (k, w, n_pos, n_pos / valid, 2 / (w + 1)))
        if w >= 5:
            assert n_pos < valid / 2
        if w == 1:
            assert n_pos == valid


def test_model_seeds_with_w1_are_seed_models(random_ref):
    """w = 1: the model's batch output equals seed_model's at stride 1 (every valid k-mer is its own window's minimizer)."""
    import minimizer_model as mm
    import seed_model as m
    ref = m.make_reference()
    rows, rl, _, _, _ = m.make_reads(ref, 48, 128)
    k = 8
    index = m.build_index(ref, k)
    assert all(np.array_equal(a, b) for a, b in zip(index, mm.build_index(ref, k, 1)))
    a = m.seed(rows, rl, index, len(ref), k, 1, 64, 4, 16, 3, 16, 128)
    b = mm.seed(rows, rl, index, len(ref), k, 1, 64, 4, 16, 3, 16, 128)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_minimizer_kernels_code_objects():
    """Each new kernel exists exactly once, uses no scratch and stays within the register bound its header states; neither is an
    instantiation of the kernel it stands in for."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_regs
    lib = os.path.join(ROOT, "aim_amd", "libaim_hip.so")
    if not os.path.exists(lib):
        pytest.fail("libaim_hip.so is missing: run the build")
    regs = codeobj_regs.kernel_regs(lib)
    names = _lib().aim_minimizer_kernel_names().decode().split(",")
    assert names == ["index_minimizer_kernel", "seed_minimizer_kernel"]
    for name, hpp, const, lds in (("index_minimizer_kernel", "index.hpp", "kIndexMinimizerMaxVgpr", True), ("seed_minimizer_kernel", "seed.hpp", "kSeedMinimizerMaxVgpr", False)):
        found = [n for n in regs if name in n]
        assert len(found) == 1 and re.search(r"\baim::%s\(" % name, found[0]), (name, found)
        bound = int(re.search(r"constexpr int %s = (\d+);" % const, open(os.path.join(ROOT, "aim_amd", "csrc", hpp)).read()).group(1))
        r = regs[found[0]]
        assert r["scratch_bytes"] == 0, (name, r)
        assert 0 < r["vgpr"] + r["agpr"] <= bound <= 512 // 3, (name, r, bound)
        assert (r["lds_static_bytes"] > 0) == lds, (name, r)
        if lds:      # 7 workgroups per CU, as index.hpp plans: at most 18 granules of 1 280 B
            assert r["lds_static_bytes"] <= 18 * 1280, r
    assert len([n for n in regs if "aim::seed_candidates_kernel" in n]) == 1 and len([n for n in regs if "aim::index_code_kernel" in n]) == 1
