#!/usr/bin/env python3
"""Generate tests/golden/placement_plans.json: the kernel and shape aim_plan_describe names for every row of the full-row table
(tests/full_rows.py) at the pair counts the placement arrangements run it at (tests/placement.py: 1, the prefix sizes and the
row's own count), under the row's knobs, 16 GB and 256 CUs.

Needs only the built library (no device). tests/test_placement_cpu.py compares the planner with this file. Regenerate only when
a plan is meant to change (AIM_LIB selects the library):
    python tests/golden/make_placement_plans.py
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "placement_plans.json")


def main():
    env = {k: v for k, v in os.environ.items() if not k.startswith("AIM_") or k == "AIM_LIB"}
    env.update(AIM_SCRATCH_GB="16", AIM_CHIP_CUS="256")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "placement.py"), "--plans"], env=env, capture_output=True, text=True,
                       timeout=300)
    if r.returncode:
        raise RuntimeError(r.stderr[-2000:])
    plans = json.loads(r.stdout)
    with open(OUT, "w") as f:
        json.dump(plans, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s: %d rows, %d plans" % (OUT, len(plans), sum(len(v) for v in plans.values())))


if __name__ == "__main__":
    main()
