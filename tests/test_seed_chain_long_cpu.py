"""aim_seed_chain_long_device without a GPU: the ABI values, the symbol and the feature bit, every refusal by message (the parameter
checks come before any device query), that the old entry points keep their bounds, the rule as tests/chain_long_model.py writes it
down against tests/chain_model.py where the two must agree, that the batches of tests/test_seed_chain_long_gpu.py hold what they are
meant to hold, and the code object of the new kernel next to the four seed kernels that were there."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "aim_hip.h")
KERNEL_HEADER = os.path.join(ROOT, "aim_amd", "csrc", "seed_chain_long.hpp")
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(autouse=True)
def _feature():
    """Every test here is about AIM_FEATURE_SEED_CHAIN_LONG: a library without the bit fails them all, the model tests included."""
    from aim_amd import capi, engine
    assert engine.features() & capi.FEATURE_SEED_CHAIN_LONG and hasattr(capi.load(), "aim_seed_chain_long_device")


def _lib():
    from aim_amd import capi
    return capi.load()


def _err():
    return _lib().aim_last_error().decode()


def _define(name):
    m = re.search(r"#define\s+%s\s+(\S+)" % name, open(HEADER).read())
    return int(m.group(1).rstrip("uUlL"), 0)


def test_constants_symbol_and_feature_bit():
    from aim_amd import capi, engine
    import chain_long_model as clm
    assert _define("AIM_FEATURE_SEED_CHAIN_LONG") == capi.FEATURE_SEED_CHAIN_LONG == 0x8000
    assert engine.features() & capi.FEATURE_SEED_CHAIN_LONG
    assert _define("AIM_SEED_LONG_MAX_READ_SIZE") == capi.SEED_LONG_MAX_READ_SIZE == clm.MAX_READ_SIZE == 65528
    assert _define("AIM_SEED_LONG_MAX_HITS") == capi.SEED_LONG_MAX_HITS == clm.MAX_HITS == 8192
    assert capi.SEED_LONG_MAX_READ_SIZE % 8 == 0 and capi.SEED_LONG_MAX_READ_SIZE < 1 << 16 <= capi.SEED_LONG_MAX_READ_SIZE + 8   # q_hi fits uint16_t
    assert _lib().aim_seed_chain_long_kernel_name() == b"seed_chain_long_kernel"
    assert _lib().aim_seed_chain_kernel_names() == b"seed_chain_kernel,seed_chain_minimizer_kernel"      # the names that were there stay
    assert hasattr(_lib(), "aim_seed_chain_long_device") and callable(engine.seed_chain_long_device) and callable(engine.seed_chain_long_candidates)
    assert _define("AIM_SEED_MAX_READ_SIZE") == 4096 and _define("AIM_SEED_MAX_HITS") == 1024            # ... and so do the old bounds


GOOD = dict(k=11, max_occ=8, band=8, flank=8, min_votes=2, max_cands=4, read_size=8232, w=10)


def _sp(**kw):
    from aim_amd import engine
    return engine.seed_params(long_reads=True, **dict(GOOD, **kw))


def _call(sp, max_hits=2048, n_reads=4, ref_len=1000):
    """aim_seed_chain_long_device with NULL buffers: the parameter checks come first, with or without a device."""
    return _lib().aim_seed_chain_long_device(None if sp is None else C.byref(sp), max_hits, n_reads, None, None, None, None, ref_len, None, None, None,
                                             None, None, None)


@pytest.mark.parametrize("max_hits", [0, 512, 3000, 16384])
def test_max_hits_is_refused_by_name(max_hits):
    from aim_amd import capi
    assert _call(_sp(), max_hits=max_hits) == capi.AIM_EINVAL
    assert _err() == "aim_seed_chain_long_device: max_hits %d must be a power of two in 1024..8192" % max_hits, _err()


@pytest.mark.parametrize("max_hits", [1024, 2048, 4096, 8192])
def test_every_legal_max_hits_passes_the_parameter_checks(max_hits):
    from aim_amd import capi
    assert _call(_sp(), max_hits=max_hits) == capi.AIM_EINVAL and _err() == "aim_seed_chain_long_device: null device buffer", _err()


BAD = [("read_size", 65536, "read_size 65536 must be a positive multiple of 8, at most 65528"),
       ("read_size", 65532, "read_size 65532 must be a positive multiple of 8, at most 65528"),
       ("read_size", 0, "read_size 0 must be"), ("options", 0, "options 0x0 must be AIM_SEED_OPT_MINIMIZERS(w)"),
       ("options", 0x2100, "unknown options 0x2100"), ("options", 0xA02, "unknown options 0xa02"),
       ("stride", 2, "stride 2 must be 1 with AIM_SEED_OPT_MINIMIZERS"), ("stride", 0, "stride 0 must be >= 1"),
       ("band", 4097, "band 4097 is above 4096"), ("band", -1, "band -1 must be >= 0"), ("k", 7, "k 7 is outside 8..14"),
       ("k", 15, "k 15 is outside 8..14"), ("max_occ", 0, "max_occ 0 must be >= 1"), ("flank", -1, "flank -1 must be >= 0"),
       ("min_votes", 0, "min_votes 0 must be >= 1"), ("max_cands", 0, "max_cands 0 is outside 1..16"), ("max_cands", 17, "max_cands 17 is outside 1..16")]


@pytest.mark.parametrize("field,value,msg", BAD, ids=["%s=%d" % b[:2] for b in BAD])
def test_every_bound_is_refused_by_name(field, value, msg):
    from aim_amd import capi
    sp = _sp()
    setattr(sp, field, value)
    assert _call(sp) == capi.AIM_EINVAL and _err().startswith("aim_seed_params_t: " + msg), _err()


def test_other_refusals():
    from aim_amd import capi, engine
    sp = _sp()
    assert _call(None) == capi.AIM_EINVAL and _err() == "aim_seed_chain_long_device: sp is NULL"
    assert _call(sp, ref_len=capi.SEED_MAX_REF_LEN + 1) == capi.AIM_EINVAL and _err().startswith("aim_seed_chain_long_device: ref_len") and "2^32 - 2^25" in _err()
    assert _call(sp, n_reads=1 << 30) == capi.AIM_EINVAL and "aim_seed_chain_long_device: n_reads 1073741824 * max_cands 4 does not fit 32 bits" in _err()
    assert _call(sp) == capi.AIM_EINVAL and _err() == "aim_seed_chain_long_device: null device buffer"
    for rs, band, w in ((65528, 4096, 1), (8, 0, 32)):                               # the extremes get past the parameter checks
        assert _call(_sp(read_size=rs, band=band, w=w)) == capi.AIM_EINVAL and _err() == "aim_seed_chain_long_device: null device buffer", _err()
    with pytest.raises(capi.AimError) as e:
        engine.seed_chain_long_device(sp, 3000, 4, None, None, None, None, 1000, None, None, None, None)
    assert "max_hits 3000" in str(e.value)
    with pytest.raises(ValueError):
        engine.seed_params(11, 65536, w=10, long_reads=True)


def test_old_entry_points_keep_their_bounds():
    """read_size 4104 is still refused by aim_seed_device and aim_seed_chain_device, by the message they had."""
    from aim_amd import capi, engine
    sp = _sp(read_size=4104)
    msg = "aim_seed_params_t: read_size 4104 must be a positive multiple of 8, at most 4096"
    assert _lib().aim_seed_device(C.byref(sp), 4, None, None, None, None, 1000, None, None, None, None, None) == capi.AIM_EINVAL and _err() == msg
    assert _lib().aim_seed_chain_device(C.byref(sp), 4, None, None, None, None, 1000, None, None, None, None, None, None) == capi.AIM_EINVAL and _err() == msg
    with pytest.raises(ValueError):
        engine.seed_params(11, 4104, w=10)
    assert _call(sp) == capi.AIM_EINVAL and _err() == "aim_seed_chain_long_device: null device buffer"


@pytest.mark.parametrize("row", [(11, 1, 5, 8, 32, 8, 2, 4), (13, 1, 10, 8, 32, 8, 2, 4)], ids=str)
def test_model_equals_chain_model_at_1024(row):
    """With H = 1 024 the rule is aim_seed_chain_device's: the two models agree on the short batch for the minimizer rows of
    tests/test_seed_chain_gpu.py."""
    import chain_long_model as clm
    import chain_model as cm
    import minimizer_model as mm
    import seed_model as m
    k, stride, w, max_occ, band, flank, min_votes, K = row
    ref = m.make_reference()
    rows, rl = m.make_reads(ref, 256, 128)[:2]
    index = mm.build_index(ref, k, w)
    want = cm.seed_chain(rows, rl, index, len(ref), k, stride, w, max_occ, band, flank, min_votes, K, 128)
    got = clm.seed_chain_long(rows, rl, index, len(ref), k, w, max_occ, band, flank, min_votes, K, 128, 1024)
    assert (want[3]["n_cands"] > 0).sum() > 100
    for g, x in zip(got, want):
        assert g.tobytes() == x.tobytes()


def test_the_local_selection_is_the_window_rule():
    """The tiled kernel selects by the local form with L and R capped at w - 1: on the seam batch it is the window rule's set."""
    import chain_long_batches as lb
    import minimizer_model as mm
    b = lb.batch_g()
    for r in range(0, len(b["rl"]), 7):
        read = b["rows"][r][:b["rl"][r]]
        for w in (2, 32):
            assert np.array_equal(mm.selected(read, 11, w), mm.selected_local(read, 11, w)) or len(read) < 11


def test_batches_hold_what_they_are_meant_to_hold():
    """Counted on the model: the kernel is compared with it on these batches, so the batches have to contain the cases."""
    import chain_long_batches as lb
    from chain_model import strand_stats, tied
    # B: more than 1 024 anchors on the true strand, none truncated, offsets beyond 12 bits, all 8 well placed with a tight window
    b, want = lb.batch_b(), lb.expected(lb.CASE_B, lb.batch_b(), "B")
    true_hits = want[3]["n_hits"][np.arange(8), b["strand"]]
    print("B true-strand hits", true_hits.tolist(), "scores", want[4]["score"][0::4].tolist())
    assert b["deleted"].sum() == 4 and set(b["strand"].tolist()) == {0, 1}
    assert (true_hits > 1024).all() and (true_hits < 2048).all() and not want[3]["flags"].any() and (want[4]["q_hi"][0::4] > 4096).all()
    good = lb.well_placed(lb.CASE_B, b, "B")
    assert good.sum() >= 7
    assert (want[0]["text_len"][0::4][good] <= b["span"][good] + 2 * lb.CASE_B[4] + lb.B_EDITS).all()       # the window is the span, the flanks and the indels
    assert (want[4]["ref_span"][0::4][b["deleted"]] > want[4]["q_hi"][0::4][b["deleted"]].astype(np.int64) - want[4]["q_lo"][0::4][b["deleted"]] + 150).all()
    # C: scores beyond 13 bits, chains of more than 2 048 anchors
    want = lb.expected(lb.CASE_C, lb.batch_c(), "C")
    print("C hits", want[3]["n_hits"].tolist(), "scores", want[4]["score"][0::4].tolist())
    assert want[4]["score"].max() > 8191 and want[4]["n_anchors"].max() > 2048 and (want[3]["n_hits"].max(axis=1) > 2048).all() and not want[3]["flags"].any()
    # D: a sort of 8 192, scores beyond the old rank key's 14 bits, q_hi at the end of the row; truncation at the largest cap; the largest row
    want = lb.expected(lb.CASE_D1, lb.batch_d1(), "D1")
    print("D1 hits", want[3]["n_hits"].tolist(), "scores", want[4]["score"][0::4].tolist(), "q_hi", want[4]["q_hi"][0::4].tolist())
    assert (want[3]["n_hits"].max(axis=1) > 4096).all() and want[4]["score"].max() > 16383 and want[4]["q_hi"].max() > 65000 and lb.batch_d1()["strand"].sum() == 1
    want = lb.expected(lb.CASE_D2, lb.batch_d2(), "D2")
    assert (want[3]["n_hits"][np.arange(2), lb.batch_d2()["strand"]] == 8192).all() and (want[3]["flags"] == 1).all()
    want = lb.expected(lb.CASE_D3, lb.batch_d3(), "D3")
    assert lb.batch_d3()["rl"][0] == 65528 and want[3]["n_cands"][0] >= 1 and want[0]["text_len"][0] == 65528
    # E: the repeat reads truncate at 2 048, the others do not; ties and branching trees
    detail = []
    want = lb.expected(lb.CASE_E, lb.batch_e(), "E", tandem=True, detail=detail)
    print("E hits", want[3]["n_hits"].tolist())
    assert (want[3]["flags"][1::2] == 1).all() and (want[3]["n_hits"][1::2].max(axis=1) == 2048).all()
    assert not want[3]["flags"][0::2].any() and (want[3]["n_hits"][0::2].max(axis=1) > 1500).all()
    total = dict(branching=0, gap_links=0, end_not_last=0, ties=0)
    for d in detail:
        if len(d[0]):
            for key, v in strand_stats(d, lb.CASE_E[0], lb.CASE_E[3], False).items():
                total[key] += v
            total["ties"] += tied(d[0][:300], d[1][:300], d[2][:300], lb.CASE_E[0], lb.CASE_E[3])     # (a prefix: the count is slow)
    print("E", total)
    assert total["ties"] >= 100 and total["branching"] >= 4 and total["gap_links"] >= 1
    # F: w = 1, more than 3 000 hits, none truncated
    want = lb.expected(lb.CASE_F, lb.batch_f(), "F")
    print("F hits", want[3]["n_hits"].tolist())
    assert (want[3]["n_hits"].max(axis=1) > 3000).all() and not want[3]["flags"].any() and lb.well_placed(lb.CASE_F, lb.batch_f(), "F").all()
    # G: the lengths around the seams, both strands, N runs and the lower-case base
    g, T = lb.batch_g(), lb.tile()
    assert set(range(T - 40, T + 41)) | set(range(2 * T - 40, 2 * T + 41)) | {0, 10, 11, 3 * T} == set(g["rl"].tolist())
    assert set(g["strand"].tolist()) == {0, 1} and ((g["rows"] == ord("N")).sum(axis=1) >= 30).sum() >= 40 and g["rows"][93, T - 1] & 0x20
    assert g["rows"].shape[1] == 3 * T + 64 and g["rl"].max() >= 3 * T - 20
    # H: windows clamped at both ends
    want = lb.expected(lb.CASE_H, lb.batch_h(), "H")
    start = (want[1][0::4] & np.uint64((1 << 63) - 1)).astype(np.int64)
    assert (start[:2] == 0).all() and start[2] + want[0]["text_len"][0::4][2] == lb.REF_LEN


def test_seed_chain_long_kernel_code_object():
    """The new kernel exists once, uses no scratch and no static LDS and stays within kSeedChainLongMaxVgpr; the four seed kernels that
    were there report the registers profiles/chain/README.md records; the LDS of every cap fits a compute unit."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_regs
    lib = os.path.join(ROOT, "aim_amd", "libaim_hip.so")
    if not os.path.exists(lib):
        pytest.fail("libaim_hip.so is missing: run the build")
    regs = codeobj_regs.kernel_regs(lib)
    text = open(KERNEL_HEADER).read()
    bound = int(re.search(r"constexpr int kSeedChainLongMaxVgpr = (\d+);", text).group(1))
    found = [n for n in regs if re.search(r"\baim::seed_chain_long_kernel\(", n)]
    assert len(found) == 1, found
    r = regs[found[0]]
    assert r["scratch_bytes"] == 0 and r["lds_static_bytes"] == 0, r
    assert 0 < r["vgpr"] + r["agpr"] <= bound <= 128, (r, bound)
    recorded = {}
    for line in open(os.path.join(ROOT, "profiles", "chain", "README.md")):
        m = re.match(r"\s*(\d+) vgpr\s+(\d+) agpr\s+(\d+) sgpr\s+(\d+) B scratch\s+aim::(\w+)\(", line)
        if m:
            recorded[m.group(5)] = tuple(int(x) for x in m.group(1, 2, 3, 4))
    assert set(recorded) == {"seed_candidates_kernel", "seed_minimizer_kernel", "seed_chain_kernel", "seed_chain_minimizer_kernel"}
    for name, want in recorded.items():
        got = [regs[n] for n in regs if re.search(r"\baim::%s\(" % name, n)]
        assert len(got) == 1 and (got[0]["vgpr"], got[0]["agpr"], got[0]["sgpr"], got[0]["scratch_bytes"]) == want, (name, got, want)
    # the LDS size function, evaluated from the header's constants
    tile = int(re.search(r"constexpr uint32_t kSeedLongTile = (\d+);", text).group(1))
    halo, max_k = _define("AIM_SEED_MAX_W") - 1, 14
    row_bytes = (tile + 2 * halo + max_k - 1 + 3 + 3 + 15) & ~15
    key_bytes = ((tile + 2 * halo) * 4 + 15) & ~15
    assert "return (size_t)max_hits * 14u + kSeedLongTileBytes;" in text
    for H, per_cu in ((1024, 9), (2048, 5), (4096, 2), (8192, 1)):
        lds = H * 14 + row_bytes + key_bytes
        assert lds <= 160 * 1024 and (160 * 1024) // (-(-lds // 1280) * 1280) == per_cu, (H, lds)
