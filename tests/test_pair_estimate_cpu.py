"""Rule 15c without a GPU: the feature bit, the struct layouts and the kernel names; every refusal of aim_pair_estimate_device and of the
_est twins by message (none needs a device), and the three rule-14c entry points still refusing an unknown option bit; the Python model
against an independent statement of the quartiles, its edge cases and its indifference to the order of the pairs; the code objects of the
four new kernels; the premises of the shared batch (tests/pair_est_batch.py) on the chain model and the ends-free DP model; and the
command line's --estimate-span."""
import ctypes as C
import math
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


def test_feature_bit_layouts_and_kernel_names():
    import pair_estimate_model as em
    from aim_amd import capi, engine
    assert _define("AIM_FEATURE_PAIR_ESTIMATE") == capi.FEATURE_PAIR_ESTIMATE == 0x400000 and engine.features() & capi.FEATURE_PAIR_ESTIMATE
    assert _lib().aim_abi_version() == 2
    assert _define("AIM_PAIR_EST_MAX_HIST") == capi.PAIR_EST_MAX_HIST == em.MAX_HIST == 8192
    assert (_define("AIM_PAIR_EST_FALLBACK"), _define("AIM_PAIR_EST_CLAMPED"), _define("AIM_PAIR_EST_FLOORED")) == \
        (capi.PAIR_EST_FALLBACK, capi.PAIR_EST_CLAMPED, capi.PAIR_EST_FLOORED) == (em.FALLBACK, em.CLAMPED, em.FLOORED) == (1, 2, 4)
    P, E = capi.PairEstParams, capi.PairEstimate
    assert C.sizeof(P) == 16 and (P.hist_size.offset, P.min_samples.offset, P.min_mapq.offset, P.min_slack.offset) == (0, 4, 8, 12)
    assert C.sizeof(E) == 48 and (E.min_span.offset, E.max_span.offset, E.n_samples.offset, E.n_beyond.offset, E.p25.offset, E.p50.offset, E.p75.offset,
                                  E.flags.offset, E.pad.offset) == (0, 8, 16, 20, 24, 28, 32, 36, 40)
    assert capi.PAIR_ESTIMATE_DTYPE == em.ESTIMATE_DTYPE and em.ESTIMATE_DTYPE.itemsize == 48
    assert [em.ESTIMATE_DTYPE.fields[k][1] for k in ("min_span", "max_span", "n_samples", "n_beyond", "p25", "p50", "p75", "flags", "pad")] == [0, 8, 16, 20, 24, 28, 32, 36, 40]
    assert _lib().aim_pair_estimate_kernel_names() == b"pair_span_hist_kernel,pair_span_bounds_kernel,pair_rescue_rows_est_kernel,pair_select_est_kernel"
    assert _lib().aim_pair_kernel_names() == b"pair_rescue_rows_kernel,pair_select_kernel,map_mates_kernel"
    for h in (64, 2048, 8192):
        assert engine.pair_estimate_scratch(h) == 4 * h + 16
    ep = engine.pair_estimate_params()
    assert (ep.hist_size, ep.min_samples, ep.min_mapq, ep.min_slack) == (2048, 64, 20, 16)
    # the structs the issue leaves alone
    assert C.sizeof(capi.MapPairParams) == 40 and C.sizeof(capi.MapperPairsOut) == 40 and C.sizeof(capi.MapperParams) == 124


OK = 1 << 12               # any aligned address: nothing is dereferenced before the device probe


def _pp(**kw):
    from aim_amd import engine
    args = dict(min_span=0, max_span=800, unpaired_penalty=17, rescue=True, rescue_size=904)
    opts = kw.pop("options", None)
    args.update(kw)
    pp = engine.pair_params(**args)
    if opts is not None:
        pp.options = opts
    return pp


def _ep(**kw):
    from aim_amd import engine
    return engine.pair_estimate_params(**kw)


def _estimate(pp=None, ep=None, K=4, rs=104, n=8, seg=OK, sam=OK, cls=OK, contig=None, est=OK, scr=OK, sb=None, null_pp=False, null_ep=False):
    pp, ep = pp or _pp(), ep or _ep()
    sb = 4 * ep.hist_size + 16 if sb is None else sb
    return _lib().aim_pair_estimate_device(None if null_pp else C.byref(pp), None if null_ep else C.byref(ep), K, rs, n, seg, sam, cls, contig, est, scr, sb, None)


def _rows_est(pp=None, K=4, rs=104, ref_len=40000, n=8, est=OK, rl=OK, null_pp=False):
    pp = pp or _pp()
    return _lib().aim_pair_rescue_rows_device_est(None if null_pp else C.byref(pp), K, rs, ref_len, 0, None, None, n, rl, OK, OK, OK, None, OK, OK, OK, est, None)


def _select_est(pp=None, K=4, rs=104, n=8, est=OK, rl=OK, null_pp=False):
    pp = pp or _pp()
    return _lib().aim_pair_select_device_est(None if null_pp else C.byref(pp), K, rs, n, rl, OK, OK, OK, None, OK, 0, 0, OK, est, None)


RULE_14C = [  # every check of rule 14c on pp, K, read_size and n_reads: the same from the three new entry points
    (dict(null_pp=True), "aim_map_pair_params_t is NULL"),
    (dict(pp=dict(options=2)), "unknown options 0x2"),
    (dict(pp=dict(options=3)), "unknown options 0x3"),
    (dict(n=7), "n_reads 7 is odd"),
    (dict(K=0), "K 0 is outside 1..16"),
    (dict(K=17), "K 17 is outside 1..16"),
    (dict(K=16, n=1 << 28), "n_reads 268435456 * (K 16 + 1) does not fit 32 bits"),
    (dict(pp=dict(min_span=-1)), "0 <= min_span <= max_span < 2^62 (min_span -1"),
    (dict(pp=dict(min_span=300, max_span=299)), "0 <= min_span <= max_span < 2^62 (min_span 300, max_span 299)"),
    (dict(pp=dict(max_span=1 << 62, rescue_size=1 << 20)), "max_span < 2^62"),
    (dict(pp=dict(unpaired_penalty=-1)), "unpaired_penalty -1 must be >= 0"),
    (dict(rs=100), "read_size 100 must be a positive multiple of 8"),
    (dict(pp=dict(rescue_size=900)), "rescue_size 900 must be a multiple of 8"),
    (dict(pp=dict(rescue_size=96, max_span=0)), "rescue_size 96 is below read_size 104"),
    (dict(pp=dict(rescue_size=896)), "max_span 800 - min_span 0 + read_size 104 exceeds rescue_size 896"),
]


@pytest.mark.parametrize("case", RULE_14C, ids=lambda c: c[1][:28].replace(" ", "_"))
def test_rule_14c_refusals_from_the_new_entry_points(case):
    from aim_amd import capi
    kw, text = dict(case[0]), case[1]
    if "pp" in kw:
        kw["pp"] = _pp(**kw["pp"])
    for fn, call in (("aim_pair_estimate_device", _estimate), ("aim_pair_rescue_rows_device_est", _rows_est), ("aim_pair_select_device_est", _select_est)):
        assert call(**kw) == capi.AIM_EINVAL and _err().startswith(fn + ": ") and text in _err(), (fn, kw, _err())


def test_estimate_refusals_need_no_device():
    from aim_amd import capi
    E = capi.AIM_EINVAL
    fn = "aim_pair_estimate_device: "
    for kw, text in ((dict(null_ep=True), "aim_pair_est_params_t is NULL"),
                     (dict(ep=_ep(hist_size=0)), "hist_size 0 must be a multiple of 64 in 64..8192"), (dict(ep=_ep(hist_size=32)), "hist_size 32 must be"),
                     (dict(ep=_ep(hist_size=100)), "hist_size 100 must be a multiple of 64"), (dict(ep=_ep(hist_size=8256)), "hist_size 8256 must be"),
                     (dict(ep=_ep(hist_size=1 << 20)), "hist_size 1048576 must be"), (dict(ep=_ep(min_samples=0)), "min_samples must be >= 1"),
                     (dict(ep=_ep(min_mapq=61)), "min_mapq 61 is outside 0..60"), (dict(seg=None), "null device buffer"), (dict(sam=None), "null device buffer"),
                     (dict(cls=None), "null device buffer"), (dict(est=None), "null device buffer"), (dict(scr=None), "null device buffer"),
                     (dict(est=OK + 8), "d_est must be 16-byte aligned"), (dict(sam=OK + 8), "d_sam must be 16-byte aligned"),
                     (dict(seg=OK + 4), "d_seg must be 8-byte aligned"), (dict(cls=OK + 4), "d_class must be 8-byte aligned"),
                     (dict(sb=4 * 2048 + 15), "scratch_bytes 8207 is below the 8208 aim_pair_estimate_scratch reports"),
                     (dict(ep=_ep(hist_size=8192), sb=8208), "scratch_bytes 8208 is below the 32784")):
        assert _estimate(**kw) == E and _err().startswith(fn) and text in _err(), (kw, _err())
    # the rescue_size bounds are rule 14c's: checked with AIM_PAIR_RESCUE alone, as aim_pair_select_device does
    off = _pp(rescue=False, rescue_size=0)
    assert _estimate(pp=off, est=OK + 8) == E and "d_est must be 16-byte aligned" in _err()
    # the _est twins: their d_est, behind everything the originals check
    for fn, call in (("aim_pair_rescue_rows_device_est", _rows_est), ("aim_pair_select_device_est", _select_est)):
        assert call(est=None) == E and _err() == fn + ": null device buffer"
        assert call(est=OK + 8) == E and _err() == fn + ": d_est must be 16-byte aligned"
        assert call(rl=None) == E and _err() == fn + ": null device buffer"
    assert _rows_est(ref_len=0) == E and "ref_len must be >= 1" in _err()
    lib = _lib()
    assert lib.aim_mapper_set_pairing_estimated(None, C.byref(_pp()), C.byref(_ep())) == E and _err() == "aim_mapper_set_pairing_estimated: mapper is NULL"
    assert lib.aim_mapper_pair_estimate(None, 0, None) == E and _err() == "aim_mapper_pair_estimate: mapper is NULL"


def test_existing_entry_points_still_refuse_unknown_option_bits():
    """The feature is switched on by new entry points, not by a bit in aim_map_pair_params_t.options."""
    from aim_amd import capi, engine
    lib = _lib()
    pp = _pp(options=2)
    assert lib.aim_pair_rescue_rows_device(C.byref(pp), 4, 104, 40000, 0, None, None, 8, OK, OK, OK, OK, None, OK, OK, OK, None) == capi.AIM_EINVAL
    assert _err() == "aim_pair_rescue_rows_device: unknown options 0x2"
    assert lib.aim_pair_select_device(C.byref(pp), 4, 104, 8, OK, OK, OK, OK, None, OK, 0, 0, OK, None) == capi.AIM_EINVAL
    assert _err() == "aim_pair_select_device: unknown options 0x2"
    sp = engine.seed_params(11, 104, max_occ=8, band=96, flank=16, min_votes=2, max_cands=4, w=5)
    mp = engine.mapper_params(sp, 64, 40, slots=2)
    b = C.c_uint64(0)
    assert lib.aim_mapper_pairing_device_bytes(C.byref(mp), C.byref(pp), C.byref(b)) == capi.AIM_EINVAL and "unknown options 0x2" in _err()
    assert lib.aim_mapper_set_pairing(None, C.byref(pp)) == capi.AIM_EINVAL and _err() == "aim_mapper_set_pairing: mapper is NULL"


# ---- the model ---------------------------------------------------------------------------------------------------------------------
def _model_pp(min_span=0, max_span=800, rescue=True, rescue_size=904):
    import pair_model as pm
    return pm.Params(min_span, max_span, 17, pm.RESCUE if rescue else 0, rescue_size)


def _est(spans, pp=None, rs=104, **ep):
    import pair_estimate_model as em
    e = em.estimate_from_spans(pp or _model_pp(), em.EstParams(**ep), rs, spans)[0]
    assert e["pad"].tolist() == [0, 0]
    return {k: int(e[k]) for k in ("min_span", "max_span", "n_samples", "n_beyond", "p25", "p50", "p75", "flags")}


def test_quartiles_against_the_sorted_samples():
    """For random histograms p_q == sorted(samples)[ceil(q * N / 4) - 1]: the definition by cum against the order statistic."""
    rng = np.random.default_rng(15)
    for trial in range(200):
        H = int(rng.choice([64, 128, 1024]))
        N = int(rng.integers(1, 40)) if trial % 2 else int(rng.integers(40, 600))
        spans = (rng.integers(0, H, size=N) if trial % 3 else np.clip(rng.normal(H / 2, H / 16, size=N).astype(np.int64), 0, H - 1)).tolist()
        e = _est(spans, hist_size=H, min_samples=1)
        s = sorted(spans)
        assert (e["p25"], e["p50"], e["p75"]) == tuple(s[math.ceil(q * N / 4) - 1] for q in (1, 2, 3)), (trial, H, N)
        assert e["n_samples"] == N and e["n_beyond"] == 0 and not e["flags"] & 1


def test_model_edge_cases():
    import pair_estimate_model as em
    F, Cl, Fl = em.FALLBACK, em.CLAMPED, em.FLOORED
    # N = 1: all three quartiles are the sample
    assert _est([400], min_samples=1) == dict(min_span=384, max_span=416, n_samples=1, n_beyond=0, p25=400, p50=400, p75=400, flags=0)
    # min_samples - 1 against min_samples
    assert _est([400] * 63, min_samples=64) == dict(min_span=0, max_span=800, n_samples=63, n_beyond=0, p25=400, p50=400, p75=400, flags=F)
    assert _est([400] * 64, min_samples=64)["flags"] == 0 and _est([400] * 64, min_samples=64)["min_span"] == 384
    # all samples equal: IQR 0, min_slack acts
    assert _est([400] * 100, min_slack=16)["max_span"] == 416 and _est([400] * 100, min_slack=0)["min_span"] == _est([400] * 100, min_slack=0)["max_span"] == 400
    # two values: p25 = p50 the lower (4 * 1 >= 2), p75 the upper
    e = _est([300, 500], min_samples=1, pp=_model_pp(rescue=False))
    assert (e["p25"], e["p50"], e["p75"]) == (300, 300, 500) and (e["min_span"], e["max_span"], e["flags"]) == (0, 1100, Fl)
    # a span of hist_size - 1 is binned, hist_size is beyond
    e = _est([2047] * 4 + [2048] * 3 + [5000], min_samples=1, pp=_model_pp(rescue=False))
    assert (e["n_samples"], e["n_beyond"], e["p25"], e["p75"]) == (4, 4, 2047, 2047)
    assert _est([2048] * 100, min_samples=1) == dict(min_span=0, max_span=800, n_samples=0, n_beyond=100, p25=0, p50=0, p75=0, flags=F)
    # lo floored at 0: FLOORED only when the max changed lo
    assert _est([10] * 50, min_samples=1, min_slack=16)["flags"] == Fl and _est([10] * 50, min_samples=1, min_slack=16)["min_span"] == 0
    assert _est([16] * 50, min_samples=1, min_slack=16) == dict(min_span=0, max_span=32, n_samples=50, n_beyond=0, p25=16, p50=16, p75=16, flags=0)
    # the clamp: W = rescue_size - read_size = 800; hi - lo == W passes, W + 1 is clamped to p50 - W / 2 .. + W
    assert _est([1000] * 50, min_samples=1, min_slack=400) == dict(min_span=600, max_span=1400, n_samples=50, n_beyond=0, p25=1000, p50=1000, p75=1000, flags=0)
    e = _est([1000] * 25 + [1001] * 25, min_samples=1, min_slack=400)
    assert (e["p25"], e["p50"], e["p75"]) == (1000, 1000, 1001) and (e["min_span"], e["max_span"], e["flags"]) == (600, 1400, Cl)
    # ... floored by the clamp's own max when p50 < W / 2, with FLOORED from the first step kept
    e = _est([100] * 25 + [500] * 25, min_samples=1)
    assert (e["min_span"], e["max_span"], e["flags"]) == (0, 800, Cl | Fl)
    # without AIM_PAIR_RESCUE nothing is clamped
    assert _est([1000] * 25 + [1001] * 25, min_samples=1, min_slack=400, pp=_model_pp(rescue=False))["max_span"] == 1401
    # n_reads = 0: the fallback with every count zero
    import pair_model as pm
    z = np.zeros(0, dtype=pm.SEG_DTYPE), np.zeros(0, dtype=pm.SAM_DTYPE), np.zeros(0, dtype=pm.CLASS_DTYPE)
    e = em.estimate(_model_pp(300, 500, rescue_size=512), em.EstParams(), 4, 104, 0, *z)[0]
    assert e.tobytes() == np.array([(300, 500, 0, 0, 0, 0, 0, F, (0, 0))], dtype=em.ESTIMATE_DTYPE).tobytes()


@pytest.mark.parametrize("contigs", (False, True), ids=("one-seq", "contigs"))
@pytest.mark.parametrize("K", (1, 4, 16))
def test_model_on_synthetic_tables_and_under_permutation(K, contigs):
    """The extended tables hold what the sample rule distinguishes, and the estimate does not change when the pairs are permuted."""
    import map_records_model as mm
    import pair_estimate_model as em
    import pair_model as pm
    n = 600
    t = em.synthetic_tables(7, K, n, contigs)
    pp = _model_pp(300, 500, rescue_size=512)
    ep = em.EstParams(1024, 8, 20, 16)
    sm = em.samples(ep, K, n, t["seg"], t["sam"], t["cls"], t["contig"])
    mapped = mm.mapped_slots(K, n, t["seg"], t["sam"])
    single = [m for m in range(n // 2) if mapped[2 * m].sum() == 1 and mapped[2 * m + 1].sum() == 1]
    assert 25 < len(sm) < len(single) and (K == 1 or any(mapped[r].sum() > 1 for r in range(n)))
    low = [m for m in single if min(int(t["cls"]["mapq"][2 * m * K + int(np.nonzero(mapped[2 * m])[0][0])]),
                                    int(t["cls"]["mapq"][(2 * m + 1) * K + int(np.nonzero(mapped[2 * m + 1])[0][0])])) < 20]
    assert low and not set(low) & {m for m, _ in sm}
    assert em.samples(em.EstParams(1024, 8, 0, 16), K, n, t["seg"], t["sam"], t["cls"], t["contig"]) != sm          # min_mapq decides some
    if contigs:
        assert len(em.samples(ep, K, n, t["seg"], t["sam"], t["cls"], None)) > len(sm)                              # ... and so does the contig
    spans = [s for _, s in sm]
    assert min(spans) < 64 and max(spans) >= 1024 and all(s >= 0 for s in spans)
    e = em.estimate(pp, ep, K, pm.READ_SIZE, n, t["seg"], t["sam"], t["cls"], t["contig"])
    assert e["n_samples"][0] + e["n_beyond"][0] == len(sm) and e["n_beyond"][0] > 0 and e["flags"][0] & em.CLAMPED
    rng = np.random.default_rng(3)
    for _ in range(3):
        assert em.estimate(pp, ep, K, pm.READ_SIZE, n, t["seg"], t["sam"], t["cls"], t["contig"], order=rng.permutation(n // 2)).tobytes() == e.tobytes()
    # the bounds feed rule 14c's model unchanged
    pe = em.params_with(pp, e)
    assert pe.max_span - pe.min_span + pm.READ_SIZE <= pm.RESCUE_SIZE
    req, tpos, rows = pm.rescue_rows(pe, K, pm.READ_SIZE, t["ref_len"], n, t["read_len"], t["reads"], t["seg"], t["sam"], t["contig"], t["starts"], t["lens"])
    assert (req["text_len"] <= pm.RESCUE_SIZE).all()
    pm.select(pe, K, pm.READ_SIZE, n, t["read_len"], t["seg"], t["sam"], t["cls"], t["contig"], t["res_sam"])


def test_pair_estimate_kernels_code_objects():
    """Each new kernel exists exactly once, uses no scratch memory and stays within kPairMaxVgpr, read as test_pair_kernels_code_objects reads
    rule 14c's. The histogram's LDS is dynamic; the bounds kernel's static LDS is its four wave totals and three quartiles."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import codeobj_regs
    lib = os.path.join(ROOT, "aim_amd", "libaim_hip.so")
    if not os.path.exists(lib):
        pytest.fail("libaim_hip.so is missing: run the build")
    regs = codeobj_regs.kernel_regs(lib)
    bound = int(re.search(r"constexpr int kPairMaxVgpr = (\d+);", open(os.path.join(ROOT, "aim_amd", "csrc", "pair.hpp")).read()).group(1))
    assert bound == 64
    for name in _lib().aim_pair_estimate_kernel_names().decode().split(","):
        found = [n for n in regs if re.search(r"\baim::%s\(" % name, n)]
        assert len(found) == 1, (name, found)
        r = regs[found[0]]
        print(name, r)
        assert r["scratch_bytes"] == 0 and 0 < r["vgpr"] + r["agpr"] <= bound, (name, r, bound)
        assert r["lds_static_bytes"] == (28 if name == "pair_span_bounds_kernel" else 0), (name, r)


# ---- the premises of the shared batch ------------------------------------------------------------------------------------------------
def _slot_tables():
    """The slot arrays the split path would leave for the batch, from the chain model: a PRIMARY chain is a mapped slot at its window's
    start + FLANK with a span of L (the reads are error-free where they have a chain at all), a SECONDARY is never aligned."""
    import chain_class_model as ccm
    import chain_model as cm
    import minimizer_model as mnm
    import pair_est_batch as eb
    import pair_model as pm
    b, ref = eb.batch(), eb.reference()
    n, K = len(b["read_len"]), eb.K
    req, tpos, votes, seeds, chains = cm.seed_chain(b["rows"], b["read_len"], mnm.build_index(ref, eb.K_MER, eb.W), len(ref), eb.K_MER, 1, eb.W, eb.MAX_OCC, eb.BAND,
                                                    eb.FLANK, eb.MIN_VOTES, K, eb.READ_SIZE)
    cls = ccm.classify(K, eb.READ_SIZE, 128, b["read_len"], tpos, seeds, chains)
    seg, sam, mcls = np.zeros(n * K, dtype=pm.SEG_DTYPE), np.zeros(n * K, dtype=pm.SAM_DTYPE), np.zeros(n * K, dtype=pm.CLASS_DTYPE)
    sam["flags"] = pm.SAM_UNMAPPED
    for r in range(n):
        for i in range(int(seeds["n_cands"][r])):
            s = r * K + i
            mcls["mapq"][s] = cls["mapq"][s]
            if cls["flags"][s] & ccm.PRIMARY:
                seg["flags"][s] = pm.SEG_VALID
                sam["pos"][s], sam["ref_span"][s] = (int(tpos[s]) & ~(1 << 63)) + eb.FLANK, eb.L
                sam["flags"][s] = pm.SAM_REVERSE if int(tpos[s]) >> 63 else 0
    return b, ref, seeds, cls, seg, sam, mcls


def test_batch_premises_on_the_chain_model_and_the_ends_free_model():
    import chain_class_model as ccm
    import endsfree_model as efm
    import pair_est_batch as eb
    import pair_estimate_model as em
    import pair_model as pm
    b, ref, seeds, cls, seg, sam, mcls = _slot_tables()
    n, K = len(b["read_len"]), eb.K
    assert eb.N_PAIRS == 336 == len(b["truth"]) and b["rows"].shape == (672, eb.READ_SIZE) and len(ref) == 40000
    assert (ref[eb.NEAR_A:eb.NEAR_A + 150] == ref[eb.NEAR_B:eb.NEAR_B + 150]).all() and eb.NEAR_B - eb.NEAR_A == 300
    assert (ref[eb.FAR_A:eb.FAR_A + 150] == ref[eb.FAR_B:eb.FAR_B + 150]).all() and eb.FAR_B - eb.FAR_A == 20000
    ep = em.EstParams(eb.HIST_SIZE, eb.MIN_SAMPLES, eb.MIN_MAPQ, eb.MIN_SLACK)
    pp = pm.Params(eb.MIN_SPAN, eb.MAX_SPAN, eb.UNPAIRED_PENALTY, pm.RESCUE, eb.RESCUE_SIZE)
    sm = dict(em.samples(ep, K, n, seg, sam, mcls))
    beyond = 0
    for m, t in enumerate(b["truth"]):
        c = t["cls"]
        if c == "c":                                               # every class-c pair is a sample, its span its fragment length
            assert sm.get(m) == t["span"] and 300 <= t["span"] <= 500, (m, t, sm.get(m))
            for x in range(2):
                assert int(sam["pos"][(2 * m + x) * K]) == t["mates"][x][0] and int(mcls["mapq"][(2 * m + x) * K]) >= eb.MIN_MAPQ
        elif c == "l":                                             # samples, beyond the histogram
            assert sm.get(m) == 3000 >= eb.HIST_SIZE
            beyond += 1
        else:                                                      # no class-d, q, r, s or w pair is a sample
            assert m not in sm, (m, c, sm.get(m))
        if c in "wq":                                              # the repeat mate: rank 0 is the lower copy at MAPQ 0, the other copy a secondary
            r = 2 * m + t["repeat"]
            lo = t["mates"][t["repeat"]][0]
            first = eb.NEAR_A if c == "w" else eb.FAR_A
            true_first = c == "q" and t["q"] < 8
            assert int(seeds["n_cands"][r]) == 2 and cls["flags"][r * K] & ccm.PRIMARY and cls["flags"][r * K + 1] == ccm.SECONDARY
            assert int(sam["pos"][r * K]) == (lo if true_first else lo - (300 if c == "w" else 20000)) and first <= int(sam["pos"][r * K]) < first + 50
            assert int(mcls["mapq"][r * K]) == 0 < eb.MIN_MAPQ
            u = 2 * m + 1 - t["repeat"]                            # the unique mate, at its true place
            assert int(sam["pos"][u * K]) == t["mates"][1 - t["repeat"]][0] and int(mcls["mapq"][u * K]) == 60
            if c == "w":                                           # the wrong copy is 300 bases further and still proper under 0..800
                x, y = pm.cand(sam[2 * m * K], 0), pm.cand(sam[(2 * m + 1) * K], 0)
                assert 380 <= t["span"] <= 420 and pm.proper_span(pp, x, y) == t["span"] + 300 <= 800
                assert int(sam["pos"][u * K]) >= eb.NEAR_B + 150 and lo + eb.L <= eb.NEAR_B + 150
        if c in "sr":
            assert int(seeds["n_cands"][2 * m + 1]) == 0 and int(sam["pos"][2 * m * K]) == t["mates"][0][0]      # mate 2 has no chain at all
    assert beyond == 8
    # hence the quartiles are those of the class-c fragment lengths (class w is not sampled: its repeat mate has MAPQ 0), and hi < 600
    e = em.estimate(pp, ep, K, eb.READ_SIZE, n, seg, sam, mcls)
    lens = sorted(t["span"] for t in b["truth"] if t["cls"] == "c")
    assert [int(e[k][0]) for k in ("p25", "p50", "p75")] == [lens[math.ceil(q * 256 / 4) - 1] for q in (1, 2, 3)]
    assert int(e["n_samples"][0]) == 256 and int(e["n_beyond"][0]) == 8 and int(e["flags"][0]) == 0
    lo, hi = int(e["min_span"][0]), int(e["max_span"][0])
    assert 200 < lo < 350 and 450 < hi < 600, (lo, hi)
    assert all(lo <= t["span"] <= hi for t in b["truth"] if t["cls"] in "cws") and all(t["span"] + 300 > hi for t in b["truth"] if t["cls"] == "w")
    # the rescue rows under the estimated bounds, scored by the ends-free DP model: the repeat mate of class w and mate 2 of class s
    # align at their true place (0 and the ten substitutions), the unique mate of class w does not (its window lies beside the wrong copy)
    pe = em.params_with(pp, e)
    req, tpos, rows = pm.rescue_rows(pe, K, eb.READ_SIZE, len(ref), n, b["read_len"], b["rows"], seg, sam)
    want = {}
    for m, t in enumerate(b["truth"]):
        if t["cls"] == "w":
            want[2 * m + t["repeat"]], want[2 * m + 1 - t["repeat"]] = 0, None
        elif t["cls"] == "s":
            want[2 * m + 1] = 10 * eb.X
    tried = sorted(want)
    assert all(req["pattern_len"][r] == eb.L for r in tried)
    txt = np.zeros((len(tried), eb.RESCUE_SIZE), dtype=np.uint8)
    for i, r in enumerate(tried):
        w_lo, tl = int(tpos[r]) & ~pm.MINUS_STRAND, int(req["text_len"][r])
        w = ref[w_lo:w_lo + tl]
        txt[i, :tl] = eb.revcomp(w) if int(tpos[r]) >> 63 else w
        if want[r] is not None:                                    # the true interval lies inside the window
            tm = b["truth"][r // 2]["mates"][r % 2]
            assert w_lo <= tm[0] and tm[1] <= w_lo + tl and (int(tpos[r]) >> 63) == tm[2], (r, w_lo, tl, tm)
    pat = np.zeros((len(tried), eb.RESCUE_SIZE), dtype=np.uint8)
    pat[:, :eb.READ_SIZE] = b["rows"][tried]
    score = efm.dp_scores(req[tried], pat, txt, eb.X, eb.O, eb.E, ends_free=(0, 0, eb.RESCUE_SIZE, eb.RESCUE_SIZE)).tolist()
    for r, s in zip(tried, score):
        assert (s == want[r]) if want[r] is not None else (s > eb.MAX_SCORE), (r, s, want[r])


# ---- the command line ----------------------------------------------------------------------------------------------------------------
def test_estimate_span_reaches_set_pairing(tmp_path, monkeypatch, capsys):
    from aim_amd import capi, engine
    from aim_amd import map as amap
    a = amap.parser().parse_args(["--ref", "r", "--reads", "a", "-o", "o", "--reads2", "b"])
    assert not a.estimate_span and (a.est_hist_size, a.est_min_samples, a.est_min_mapq, a.est_min_slack) == (2048, 64, 20, 16)
    (tmp_path / "ref.fa").write_bytes(b">c\nACGTACGTACGTACGTACGT\n")
    (tmp_path / "a.fq").write_bytes(b"@r/1\nACGT\n+\nIIII\n")
    (tmp_path / "b.fq").write_bytes(b"@r/2\nACGT\n+\nIIII\n")
    seen = []

    class FakeMapper:
        def __init__(self, mp, ref, device=0):
            pass

        def __enter__(self):
            return self

        def __exit__(self, *exc):
            pass

        def set_pairing(self, pp, estimate=None):
            seen.append((pp, estimate))
            raise capi.AimError(capi.AIM_EINVAL, "stop here")

    monkeypatch.setattr(engine, "Mapper", FakeMapper)
    base = ["--ref", str(tmp_path / "ref.fa"), "--reads", str(tmp_path / "a.fq"), "--reads2", str(tmp_path / "b.fq"), "-o", str(tmp_path / "o.sam"), "--read-size", "104"]
    assert amap.main(base + ["--estimate-span", "--est-hist-size", "1024", "--est-min-samples", "5", "--est-min-mapq", "7", "--est-min-slack", "9"]) == 2
    assert "stop here" in capsys.readouterr().err
    pp, ep = seen[-1]
    assert (ep.hist_size, ep.min_samples, ep.min_mapq, ep.min_slack) == (1024, 5, 7, 9)
    assert (pp.min_span, pp.max_span, pp.rescue_size) == (0, 1000, 1104)              # the fallback still sizes the default --rescue-size
    assert amap.main(base + ["--estimate-span", "--min-span", "100", "--max-span", "700"]) == 2
    pp, ep = seen[-1]
    assert (pp.min_span, pp.max_span, pp.rescue_size) == (100, 700, 704) and (ep.hist_size, ep.min_samples, ep.min_mapq, ep.min_slack) == (2048, 64, 20, 16)
    assert amap.main(base) == 2 and seen[-1][1] is None                               # without the switch: plain set_pairing
