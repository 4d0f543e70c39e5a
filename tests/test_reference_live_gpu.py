"""Every kernel family that computes the reference's semantics against the live reference itself (oracle/_ref, made by
__graft_entry__.build(); the reference tree is not read here): per family of reference_rows.FAMILIES, score-only and with CIGAR where
the family plans both, at the smallest READ_SIZE of the low-complexity table that plans onto it and under that table's knobs, the
output file of the HIP results equals the reference program's, byte for byte. The batch is the in-domain part of a low-complexity
batch (reference_live.in_reference_domain) plus the sentinel pair; the reference binary runs on the CPU."""
import numpy as np
import pytest

import reference_live as L
from reference_rows import FAMILIES, apply_env, knob_env, plan_family, plan_line

pytestmark = pytest.mark.gpu

CASES = L.gpu_cases()


@pytest.fixture(scope="module")
def gpu(built):
    import ctypes as C
    from aim_amd import capi
    lib = capi.load()
    n = C.c_int()
    rc = lib.aim_device_count(C.byref(n))
    assert rc == 0 and n.value >= 1, "no HIP device visible: %s" % lib.aim_last_error()
    return lib


def test_cases_cover_every_family():
    """All eleven families, each with CIGAR or without; both where the tables plan both."""
    assert {c[0] for c in CASES} == set(FAMILIES)
    both = {f for f in FAMILIES if {(f, False), (f, True)} <= {c[:2] for c in CASES}}
    assert both >= {"nw_reg", "nw_lane", "swg_reg", "dp_group", "dp_strip", "wfa_lane", "wfa_lane_packed", "wfa_group", "wfa_wave"}


@pytest.mark.parametrize("family,cigar,fam,rs", CASES, ids=["%s-%s-%s-%d" % (c[0], "cigar" if c[1] else "score", c[2], c[3]) for c in CASES])
def test_hip_equals_live_reference(gpu, family, cigar, fam, rs, monkeypatch):
    import low_complexity as LC
    from aim_amd import engine
    from oracle import ref_run
    algo, params, name, (req, pat, txt, lost) = L.gpu_batch(fam, rs)
    assert lost <= L.MAX_LOST * L.GPU_PAIRS and len(req) == L.GPU_PAIRS - lost + 1
    apply_env(monkeypatch, knob_env(LC.FAMILIES[fam]["env"]))
    rc, line = plan_line(params, len(req))
    assert rc == 0 and plan_family(line) == family, line
    with engine.DeviceSet(1) as s:
        res, ops = s.align(params, req, pat, txt, check=False)
        launched = s.plan_describe(0)
    assert plan_family(launched) == family, launched
    stopped = res["status"] != 0
    rrc, out, log = ref_run.run(name, engine.pairs_to_text(req, pat, txt), len(req), timeout=120)
    print("%s: %d pairs (%d outside the reference's domain), %d stopped; %s" % (name, len(req), lost, int(stopped.sum()), launched))
    if stopped.any():
        # int8 SWG whose traceback finds no operation: the reference stops there, and HIP must have said so of that pair
        assert rrc == 1 and L.ABORT_SWG in log, (rrc, log[-300:])
        keep = np.nonzero(~stopped)[0]
        req, pat, txt = req[keep].copy(), np.ascontiguousarray(pat[keep]), np.ascontiguousarray(txt[keep])
        res, ops = res[keep].copy(), (None if ops is None else ops[keep])
        req["idx"] = res["idx"] = np.arange(len(keep), dtype=np.uint32)
        rrc, out, log = ref_run.run(name, engine.pairs_to_text(req, pat, txt), len(req), timeout=120)
    assert rrc == 0, (rrc, log[-300:])
    got = engine.format_output(res, ops, cigar)
    if got != out:
        a, b = got.split(b"\n"), out.split(b"\n")
        at = next((i for i, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))
        raise AssertionError("output differs at line %d: HIP %r, reference %r" % (at, a[at:at + 2], b[at:at + 2]))
