"""The device-side index build without a GPU: the new feature bit, aim_index_device_scratch (values, monotony, refusals), every refusal
of aim_index_build_device by message before a device is touched, and the kernels' code objects (present once, no scratch memory, VGPRs
within the bounds csrc/index.hpp states)."""
import ctypes as C
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aim_hip.h")
INDEX_HPP = os.path.join(ROOT, "aim_amd", "csrc", "index.hpp")


def _lib():
    from aim_amd import capi
    return capi.load()


def _err():
    return _lib().aim_last_error().decode()


def _define(name):
    m = re.search(r"#define\s+%s\s+(\S+)" % name, open(HEADER).read())
    return int(m.group(1).rstrip("uUlL"), 0)


def tile():
    return int(re.search(r"constexpr uint32_t kIndexTile = (\d+);", open(INDEX_HPP).read()).group(1))


def test_constants_and_feature_bit():
    from aim_amd import capi, engine
    assert _define("AIM_ABI_VERSION") == 2 == _lib().aim_abi_version()
    assert _define("AIM_FEATURE_INDEX_DEVICE") == capi.FEATURE_INDEX_DEVICE == 0x1000
    assert engine.features() & capi.FEATURE_INDEX_DEVICE
    assert engine.features() & capi.FEATURE_SEED
    names = _lib().aim_index_kernel_names().decode().split(",")
    assert len(names) == len(set(names)) >= 1 and all(re.fullmatch(r"index_[a-z_]+_kernel", n) for n in names)


def test_scratch_sizes():
    from aim_amd import capi, engine
    T = tile()
    for k in (8, 11, 14):
        for ref_len in (0, 1, k - 1):
            assert engine.index_device_scratch(k, ref_len) == 0
        lens = [k, k + 1, 64, T - 1, T, T + 1, T + k - 1, T + k, 3 * T + 17, 10 ** 6, 2 ** 28, 2 ** 31, capi.SEED_MAX_REF_LEN]
        sizes = [engine.index_device_scratch(k, n) for n in lens]
        assert all(s > 0 and s % 256 == 0 for s in sizes)
        assert all(a <= b for a, b in zip(sizes, sizes[1:])) and sizes[0] < sizes[-1]
        # the formula aim_hip.h states
        for n, s in zip(lens, sizes):
            p = n - k + 1
            up = lambda x: (x + 255) // 256 * 256
            assert s == 3 * up(4 * p) + up(1024 * ((p + 4095) // 4096)) + 8192
    for k in (8, 14):
        top = engine.index_device_scratch(k, capi.SEED_MAX_REF_LEN)
        assert 12 * (capi.SEED_MAX_REF_LEN - k + 1) <= top < 13 * capi.SEED_MAX_REF_LEN
    sb = C.c_uint64()
    for k in (7, 15):
        assert _lib().aim_index_device_scratch(k, 100, C.byref(sb)) == capi.AIM_EINVAL and "k %d is outside 8..14" % k in _err()
    assert _lib().aim_index_device_scratch(11, capi.SEED_MAX_REF_LEN + 1, C.byref(sb)) == capi.AIM_EINVAL
    assert "ref_len" in _err() and "2^32 - 2^25" in _err()
    assert _lib().aim_index_device_scratch(11, 100, None) == capi.AIM_EINVAL and "NULL" in _err()


def test_refusals():
    """Every refusal names its cause and comes before a device is touched (there is none here): the pointers are never followed."""
    from aim_amd import capi, engine
    lib = _lib()
    k, ref_len = 11, 1000
    sb = engine.index_device_scratch(k, ref_len)
    ref, bucket, pos, scr = 0x10000, 0x20000, 0x30000, 0x40000        # made-up, aligned addresses
    call = lambda *a: lib.aim_index_build_device(*a, None)
    for bad_k in (7, 15):
        assert call(ref, ref_len, bad_k, bucket, pos, scr, sb) == capi.AIM_EINVAL and "k %d is outside 8..14" % bad_k in _err()
    assert call(ref, capi.SEED_MAX_REF_LEN + 1, k, bucket, pos, scr, 1 << 40) == capi.AIM_EINVAL and "ref_len" in _err() and "2^32 - 2^25" in _err()
    assert call(ref, ref_len, k, None, pos, scr, sb) == capi.AIM_EINVAL and "d_bucket is NULL" in _err()
    assert call(ref, k - 1, k, None, None, None, 0) == capi.AIM_EINVAL and "d_bucket is NULL" in _err()      # needed at every size
    assert call(ref, ref_len, k, bucket, None, scr, sb) == capi.AIM_EINVAL and "d_pos is NULL" in _err()
    assert call(ref, k, k, bucket, None, scr, sb) == capi.AIM_EINVAL and "d_pos is NULL" in _err()           # ref_len == k: one position
    assert call(None, ref_len, k, bucket, pos, scr, sb) == capi.AIM_EINVAL and "d_reference is NULL" in _err()
    assert call(ref + 4, ref_len, k, bucket, pos, scr, sb) == capi.AIM_EINVAL and "d_reference is not 16-byte aligned" in _err()
    assert call(ref, ref_len, k, bucket, pos, None, sb) == capi.AIM_EINVAL and "d_scratch is NULL" in _err()
    assert call(ref, ref_len, k, bucket, pos, scr, sb - 1) == capi.AIM_EINVAL
    assert "scratch_bytes %d is below the %d" % (sb - 1, sb) in _err()
    assert call(ref, ref_len, k, bucket, pos, scr + 128, sb) == capi.AIM_EINVAL and "d_scratch is not 256-byte aligned" in _err()
    assert call(ref, ref_len, k, bucket, pos, scr, 0) == capi.AIM_EINVAL and "scratch_bytes 0 is below" in _err()


def test_index_kernels_code_objects():
    """Every kernel aim_index_kernel_names lists exists exactly once in the library, uses no scratch memory, and stays within the
    register bound index.hpp states for it (index_scan_top_kernel -> kIndexScanTopMaxVgpr)."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_regs
    lib = os.path.join(ROOT, "aim_amd", "libaim_hip.so")
    if not os.path.exists(lib):
        pytest.fail("libaim_hip.so is missing: run the build")
    hpp = open(INDEX_HPP).read()
    regs = codeobj_regs.kernel_regs(lib)
    names = _lib().aim_index_kernel_names().decode().split(",")
    assert len(names) >= 3
    for name in names:
        found = [n for n in regs if re.search(r"\baim::%s\(" % name, n)]
        assert len(found) == 1, (name, found)
        camel = "".join(w.capitalize() for w in name[:-len("_kernel")].split("_"))          # index_scan_top -> IndexScanTop
        m = re.search(r"constexpr int k%sMaxVgpr = (\d+);" % camel, hpp)
        assert m, "index.hpp states no k%sMaxVgpr" % camel
        bound = int(m.group(1))
        r = regs[found[0]]
        assert r["scratch_bytes"] == 0, (name, r)
        assert 0 < r["vgpr"] + r["agpr"] <= bound <= 512, (name, r, bound)
