"""Every reference row the judges recorded (tests/golden/judge_r01..r06_cases.json), and the planner knob settings each row is run
under. conftest.judge_cases() / judge_abort_cases() cover r01..r05; the r06 rows are loaded here, so the reference rows are
all_reference_rows(). Inputs, parsed pairs and oracle results are made once per row and process."""
import json
import os
import re

from conftest import GOLDEN, judge_abort_cases, judge_case_input, judge_cases, judge_costs

# The planner's switches (capi_plan.hip read_knobs) that re-route a batch to another kernel: name, environment. AIM_DEBUG_FLAGS is
# left out: it acts in diagnostic builds only. AIM_SCRATCH_GB=1 reaches int8 SWG's fallback from swg_lane to dp_wave.
KNOBS = [
    ("default", {}),
    ("AIM_FORCE_WAVE", {"AIM_FORCE_WAVE": "1"}),
    ("AIM_NO_GROUP", {"AIM_NO_GROUP": "1"}),
    ("AIM_NO_LANE", {"AIM_NO_LANE": "1"}),
    ("AIM_NO_LANE_PK", {"AIM_NO_LANE_PK": "1"}),
    ("AIM_NO_LANE_EXT", {"AIM_NO_LANE_EXT": "1"}),
    ("AIM_GROUP_G=2", {"AIM_GROUP_G": "2"}),
    ("AIM_GROUP_G=4", {"AIM_GROUP_G": "4"}),
    ("AIM_GROUP_G=64", {"AIM_GROUP_G": "64"}),
    ("AIM_GROUP_WLDS=64", {"AIM_GROUP_WLDS": "64"}),
    ("AIM_GROUP_OVERLAP", {"AIM_GROUP_OVERLAP": "1"}),
    ("AIM_NO_NW_REG", {"AIM_NO_NW_REG": "1"}),
    ("AIM_NO_SWG_REG", {"AIM_NO_SWG_REG": "1"}),
    ("AIM_NO_DP_GROUP", {"AIM_NO_DP_GROUP": "1"}),
    ("AIM_NO_NW_REG+AIM_NO_SWG_REG+AIM_NO_DP_GROUP", {"AIM_NO_NW_REG": "1", "AIM_NO_SWG_REG": "1", "AIM_NO_DP_GROUP": "1"}),
    ("AIM_DPW_LEGACY", {"AIM_DPW_LEGACY": "1"}),
    ("AIM_FORCE_DPWAVE", {"AIM_FORCE_DPWAVE": "1"}),
    ("AIM_STRIP_K=20", {"AIM_STRIP_K": "20"}),
    ("AIM_STRIP_K=32", {"AIM_STRIP_K": "32"}),
    ("AIM_SCRATCH_GB=1", {"AIM_SCRATCH_GB": "1"}),
    ("AIM_FORCE_WAVE+AIM_WFA_NO_RING", {"AIM_FORCE_WAVE": "1", "AIM_WFA_NO_RING": "1"}),
    ("AIM_FORCE_WAVE+AIM_WFA_SLOTW=16", {"AIM_FORCE_WAVE": "1", "AIM_WFA_SLOTW": "16"}),
]

# Every knob setting plans under this scratch bound unless it sets its own: with a device present the bound would otherwise
# follow free memory, and the plan with it.
SCRATCH_GB = "64"

# The kernel families that compute the reference's semantics (genasm_wave_kernel has no reference).
FAMILIES = ("wfa_lane", "wfa_lane_packed", "wfa_group", "wfa_wave", "nw_reg", "nw_lane", "swg_reg", "swg_lane", "dp_group",
            "dp_strip", "dp_wave")


def _r06():
    return json.load(open(os.path.join(GOLDEN, "judge_r06_cases.json")))["cases"]


def judge_r06_cases():
    """judge r06: 28 reference digests aimed at round 6's dispatch ranges -- dp_group at 20/24/28 registers
    and with CIGAR to READ_SIZE 2560, dp_strip at 2952/3688, NW at READ_SIZE 4552..7888 off the literal path, band walks at
    e = 15 %, int8 SWG at 512..1320, wfa_group with rows wider than 48."""
    return [c for c in _r06() if "abort" not in c]


def judge_r06_abort_cases():
    """judge r06: the int8 SWG input on which the reference stops with `SWG backtrace. No backtrace operation found`."""
    return [c for c in _r06() if "abort" in c]


def all_reference_rows():
    """r01..r06: the digest rows, then the abort rows."""
    return judge_cases() + judge_r06_cases() + judge_abort_cases() + judge_r06_abort_cases()


def row_id(case):
    return case["name"]


_inputs, _oracle = {}, {}


def row_input(case):
    """(input file bytes, req, pat, txt) of a row, regenerated once per process."""
    if case["name"] not in _inputs:
        from aim_amd import engine
        data = judge_case_input(case)
        _inputs[case["name"]] = (data,) + tuple(engine.parse_pairs(data, case["read_size"]))
    return _inputs[case["name"]]


def row_params(case, **extra):
    """engine.make_params of a row; `extra` adds make_params keywords (ends_free, gap2, w32)."""
    from aim_amd import engine
    return engine.make_params(case["algo"], case["max_score"], case["read_size"], backtrace=case["backtrace"],
                              reduce=case.get("reduce", False), swg_w16=case.get("swg_cell_bytes", 0) == 2, **judge_costs(case),
                              **extra)


def row_oracle(case):
    """(results, ops, worst status) of the oracle on a row, once per process."""
    if case["name"] not in _oracle:
        from oracle import oracle
        _, req, pat, txt = row_input(case)
        p = oracle.params(case["algo"], case["max_score"], case["read_size"], backtrace=case["backtrace"],
                          reduce=case.get("reduce", False), swg_cell_bytes=case.get("swg_cell_bytes", 0), **judge_costs(case))
        _oracle[case["name"]] = oracle.align_batch(p, req["pattern_len"], req["text_len"], pat, txt, nthreads=8)
    return _oracle[case["name"]]


def knob_env(env, cus=None):
    """The environment of one knob setting: every AIM_* variable but AIM_LIB cleared, AIM_SCRATCH_GB (and AIM_CHIP_CUS when
    given) set explicitly, then the setting's own variables."""
    out = {k: v for k, v in os.environ.items() if not k.startswith("AIM_") or k == "AIM_LIB"}
    out["AIM_SCRATCH_GB"] = SCRATCH_GB
    if cus is not None:
        out["AIM_CHIP_CUS"] = str(cus)
    out.update(env)
    return out


def apply_env(monkeypatch, env):
    """Make os.environ equal `env` for the AIM_* variables (the library reads them at every plan)."""
    for k in [k for k in os.environ if k.startswith("AIM_") and k not in env]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        if k.startswith("AIM_"):
            monkeypatch.setenv(k, v)


def plan_line(params, n_pairs):
    """(rc, plan line or error) of aim_plan_describe under the current environment."""
    import ctypes as C
    from aim_amd import capi
    lib = capi.load()
    buf = C.create_string_buffer(1024)
    rc = lib.aim_plan_describe(capi.params_ref(params), n_pairs, buf, len(buf))
    return rc, (buf.value.decode() if rc == 0 else lib.aim_last_error().decode(errors="replace"))


def plan_key(line):
    """A plan line without its budget= field: two knob settings that give the same key run the same launches."""
    return re.sub(r" budget=\d+", "", line)


def plan_family(line):
    return line.split(" ", 1)[0][:-len("_kernel")]


def distinct_plans(monkeypatch, case):
    """[(knob names, plan key)] of a row: one entry per distinct plan the knob list reaches, in knob-list order (the default
    first); knob settings whose plan fails (rc != 0) are left out. Leaves os.environ as the last setting made it."""
    params, n = row_params(case), case["gen"]["n"]
    seen = {}
    for name, env in KNOBS:
        apply_env(monkeypatch, knob_env(env))
        rc, line = plan_line(params, n)
        if rc == 0:
            seen.setdefault(plan_key(line), []).append(name)
    return [(names, key) for key, names in seen.items()]
