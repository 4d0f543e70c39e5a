"""The planner's decisions over a wide grid of configurations, locked: tests/golden/make_plan_sweep.py re-runs the sweep (every
env setting in its own process, no device needed) and every group of rows -- describe line or error text, aim_scratch_bytes -- and
the distinct AIM_PLAN_DEBUG lines must match the committed golden's digests. A change that is meant to move a plan regenerates
the golden."""
import gzip
import importlib.util
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _generator():
    spec = importlib.util.spec_from_file_location("make_plan_sweep", os.path.join(GOLDEN, "make_plan_sweep.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plans_match_the_golden_sweep(built):
    gen = _generator()
    with gzip.open(os.path.join(GOLDEN, "plan_sweep.json.gz"), "rt") as f:
        want = json.load(f)
    got = gen.sweep()
    assert [(s["name"], s["env"], s["grid"]) for s in got] == [(s["name"], s["env"], s["grid"]) for s in want]
    problems = []
    for g, w in zip(got, want):
        rows, form = gen.groups(g), gen.golden_form(g)
        if [k for k, _, _ in form["groups"]] != [k for k, _, _ in w["groups"]]:
            problems.append("%s: the sweep's groups differ from the golden's (regenerated with another grid?)" % g["name"])
            continue
        diff = [(a, b) for a, b in zip(form["groups"], w["groups"]) if a != b]
        for a, b in diff[:3]:
            problems.append("%s: %s (%d rows, golden %d) differs from the golden; its rows now:\n      %s" % (
                g["name"], a[0], a[1], b[1], "\n      ".join(str(r) for r in rows[a[0]][:8])))
        if len(diff) > 3:
            problems.append("%s: ... %d differing groups in all" % (g["name"], len(diff)))
        if form["stderr"] != w["stderr"]:
            problems.append("%s: AIM_PLAN_DEBUG lines differ (%d distinct, golden %d); now, first lines: %s" % (
                g["name"], form["stderr"][0], w["stderr"][0], g["stderr"][:3]))
    assert not problems, "\n".join(problems[:40])
