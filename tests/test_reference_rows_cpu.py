"""The judge-r06 reference digests on the oracle, and the reach table: which kernels the planner sends every reference row
(r01..r06) to under the knob list of tests/reference_rows.py. tests/test_reference_rows_gpu.py runs each row on each of them."""
import collections
import os
import subprocess

import pytest

from conftest import ROOT, judge_costs, md5
from reference_rows import (FAMILIES, KNOBS, all_reference_rows, apply_env, judge_r06_abort_cases, judge_r06_cases, knob_env,
                            plan_family, plan_key, plan_line, row_id, row_input, row_oracle, row_params)


def test_judge_r06_fixture_shape():
    cases = judge_r06_cases() + judge_r06_abort_cases()
    assert len(judge_r06_cases()) == 28 and len(judge_r06_abort_cases()) == 1
    assert all("output_md5" in c for c in judge_r06_cases())
    names = [c["name"] for c in all_reference_rows()]
    assert len(cases) == 29 and len(names) == len(set(names))


@pytest.mark.parametrize("case", judge_r06_cases(), ids=row_id)
def test_oracle_reproduces_judge_r06_reference_digests(built, case):
    """judge r06: dp_group / dp_strip / NW off the literal path / band walks / int8 SWG / wide wfa_group rows."""
    from oracle import oracle
    res, ops, worst = row_oracle(case)
    assert worst == 0 and len(res) == case["gen"]["n"]
    assert md5(oracle.format_output(res, ops, case["backtrace"])) == case["output_md5"]


@pytest.mark.parametrize("case", judge_r06_abort_cases(), ids=row_id)
def test_oracle_aborts_where_the_reference_aborts_r06(built, case, tmp_path):
    """judge r06: int8 SWG with CIGAR at READ_SIZE 512, where the reference stops with `SWG backtrace. No backtrace operation
    found` + exit(1) (swg.c:99-104); the oracle reports AIM_PAIR_SWG_NO_OP on some pairs and its CLI stops the same way."""
    from aim_amd import capi
    res, _, worst = row_oracle(case)
    assert worst != 0 and set(res["status"].tolist()) == {0, capi.PAIR_SWG_NO_OP}
    inp, out = tmp_path / "in", tmp_path / "out"
    inp.write_bytes(row_input(case)[0])
    g, c = case["gen"], judge_costs(case)
    r = subprocess.run([os.path.join(ROOT, "oracle", "oracle_cli"), "swg", "-i", str(inp), "-o", str(out), "-n", str(g["n"]),
                        "-l", str(g["l"]), "-e", str(g["e"]), "-b", "--max-score", str(case["max_score"]), "--read-size",
                        str(case["read_size"]), "-x", str(c["mismatch"]), "-g", str(c["gap_o"]), "-a", str(c["gap_e"])],
                       capture_output=True, text=True)
    assert r.returncode == 1 and case["abort"] in r.stdout, (r.stdout, r.stderr)


# Where round 6 aimed each r06 row (Next round item 1): the kernel of its default plan.
R06_DEFAULT_FAMILY = {
    "nw_reg": ("nw_l100_e15_bt", "nw_l160_e4_bt_x4gi3gd5"),
    "swg_reg": ("swg_l100_e15_bt_w16", "swg_l150_e8_bt_w16"),
    "dp_group": ("nw_l1200_e2_sc", "nw_l1700_e2_sc_x2gi5gd3", "swg_l1450_e2_sc_w16", "nw_l1200_e5_bt", "swg_l1800_e3_bt_w16",
                 "nw_l2400_e5_bt", "tails_nw_l1200_bt", "tails_swg_l1400_sc_w16"),
    "dp_strip": ("nw_l2800_e5_sc", "swg_l2800_e5_bt_w16", "nw_l3500_e5_bt", "nw_l5000_e5_sc", "nw_l5000_e5_bt",
                 "nw_l4500_e1_bt_x7gi5gd3", "nw_l7800_e1_sc", "tails_nw_l3000_bt", "tails_nw_l5000_sc"),
    "swg_lane": ("swg_l500_e1_sc_int8", "swg_l1000_e2_sc_int8", "swg_l1150_e1_sc_int8", "swg_l500_e1_bt_int8"),
    "dp_wave": ("swg_l1300_e1_sc_int8",),
    "wfa_group": ("wfa_l1000_e10_bt_red", "wfa_l600_e8_sc_red_x4g6a2", "wfa_l1500_e4_bt_red_x2g3a1"),
}


def test_reach_table_of_the_reference_rows(built, monkeypatch):
    """Every reference row plans on its default knobs; together the rows reach all eleven reference-semantics kernel families
    through the knob list; and each r06 row's default plan is on the kernel round 6 aimed it at. The planning is stateless
    (aim_plan_describe, no device), on a 256-CU chip under the scratch bound reference_rows.SCRATCH_GB."""
    reached = collections.defaultdict(set)
    default_family, bad_default, n_plans = {}, [], 0
    for case in all_reference_rows():
        params = row_params(case)
        plans = set()
        for name, env in KNOBS:
            apply_env(monkeypatch, knob_env(env, cus=256))
            rc, line = plan_line(params, case["gen"]["n"])
            if name == "default":
                if rc != 0:
                    bad_default.append("%s: rc %d %s" % (case["name"], rc, line))
                    continue
                default_family[case["name"]] = plan_family(line)
            if rc == 0:
                plans.add(plan_key(line))
                reached[plan_family(line)].add(case["name"])
        n_plans += len(plans)
    assert not bad_default, bad_default
    missing = [f for f in FAMILIES if not reached[f]]
    assert not missing, "kernel families no reference row reaches: %s" % missing
    # every r06 row is named once above
    named = sorted(n for rows in R06_DEFAULT_FAMILY.values() for n in rows)
    assert named == sorted(c["name"] for c in judge_r06_cases() + judge_r06_abort_cases())
    moved = ["%s: %s, aimed at %s" % (n, default_family[n], fam) for fam, rows in R06_DEFAULT_FAMILY.items() for n in rows
             if default_family[n] != fam]
    assert not moved, "r06 rows whose default plan moved: %s" % moved
    assert n_plans >= 2 * len(all_reference_rows()), n_plans
