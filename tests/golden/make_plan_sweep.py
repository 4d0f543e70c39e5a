#!/usr/bin/env python3
"""Generate tests/golden/plan_sweep.json.gz: what the planner (make_plan, capi_plan.hip) decides over a wide grid of
configurations, as the stateless planning entry points report it.

Every row holds the params, n_pairs, the env setting, aim_plan_describe's rc and line (aim_last_error() when rc != 0) and
aim_scratch_bytes. Each env setting runs in a fresh subprocess with AIM_SCRATCH_GB and AIM_CHIP_CUS set explicitly (with a
device present the budget would otherwise follow free memory) and AIM_PLAN_DEBUG=1; its stderr lines -- the plan lines and
wfa_group's internal line (ring, unit, wlds, per_cu) -- are recorded too.

The golden keeps, per env setting, a 64-bit digest of every group of rows (one READ_SIZE of one params family: all its flags,
score caps and batch sizes) and of the debug lines: the rows themselves would make the fixture several MB.

Needs only the built library (no device). tests/test_plan_sweep_cpu.py reproduces the sweep and compares it with the golden:
a planner refactor must leave every row as it is. Regenerate only when a plan is meant to change (AIM_LIB selects the library):
    python tests/golden/make_plan_sweep.py
"""
import ctypes as C
import gzip
import hashlib
import json
import math
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tests", "golden", "plan_sweep.json.gz")

N_PAIRS = (1, 63, 4096, 1 << 22)
# READ_SIZE limits of the kernels' admission rules
BREAKPOINTS = (80, 112, 124, 128, 144, 176, 320, 1024, 1200, 1280, 1440, 1536, 1792, 2048, 16368, 16384, 32752)


def read_sizes(step):
    """Every multiple of `step` up to 2304, then a step 31 times as large to 32 752, and the breakpoints +-8."""
    rs = set(range(step, 2305, step)) | set(range(2304, 32753, 31 * step))
    for b in BREAKPOINTS:
        rs |= {b - 8, b, b + 8}
    return sorted(r for r in rs if 8 <= r <= 32752)


def launcher_score(rs, e, cost):
    """MAX_SCORE of a read that fills READ_SIZE at error rate e (the launchers' rule, read length = rs / (1 + e))."""
    return max(1, math.ceil(rs / (1.0 + e) * e * cost))


def param_specs(rs, families):
    """(tag, make_params kwargs) for one READ_SIZE. Tags name the family; the kwargs are the params."""
    out = []
    wfa_ms = sorted({5, 10, launcher_score(rs, 0.02, 5), launcher_score(rs, 0.10, 5)})
    if "wfa" in families:
        for ms in wfa_ms:
            out.append(("wfa", dict(algo="wfa", max_score=ms)))
        for ms in (5, launcher_score(rs, 0.05, 5)):
            out.append(("wfa+reduce", dict(algo="wfa", max_score=ms, reduce=True)))
        for ef in ((0, 0, 0, 0), (0, 0, 16, 16), (8, 8, 64, 64)):
            out.append(("wfa-endsfree", dict(algo="wfa", max_score=launcher_score(rs, 0.02, 5), ends_free=ef)))
        for g2 in ((24, 1), (12, 2), (4, 1)):
            out.append(("wfa-affine2p", dict(algo="wfa", max_score=launcher_score(rs, 0.02, 5), gap2=g2)))
    if "dp" in families:
        for e in (0.02, 0.10):
            out.append(("nw", dict(algo="nw", max_score=launcher_score(rs, e, 4))))
            out.append(("swg", dict(algo="swg", max_score=min(126, launcher_score(rs, e, 5)))))
        out.append(("swg-w16", dict(algo="swg", max_score=launcher_score(rs, 0.05, 5), swg_w16=True)))
    if "genasm" in families:
        out.append(("genasm", dict(algo="genasm", max_score=0)))
    return out


# score caps no read admits: the planners' out-of-memory branches
EDGE = [("wfa", dict(algo="wfa", max_score=ms, read_size=32752)) for ms in (20000, 40000, 63000, 1 << 21)] + \
       [("wfa-endsfree", dict(algo="wfa", max_score=ms, read_size=32752, ends_free=(32752, 0, 32752, 0))) for ms in (40000, 63000)] + \
       [("nw", dict(algo="nw", max_score=100, read_size=rs)) for rs in (16376, 24000, 32752)] + \
       [("swg-w16", dict(algo="swg", max_score=200, read_size=rs, swg_w16=True)) for rs in (16376, 24000, 32752)]

FLAGS_MAIN = ({}, dict(backtrace=True))
FLAGS_IO = (dict(req8=True), dict(res8=True), dict(req8=True, res8=True), dict(req8=True, backtrace=True))

WFA_KNOBS = ("AIM_FORCE_WAVE", "AIM_NO_LANE", "AIM_NO_GROUP", "AIM_NO_LANE_PK", "AIM_NO_LANE_EXT", "AIM_WFA_NO_RING")
DP_KNOBS = ("AIM_NO_DP_GROUP", "AIM_NO_NW_REG", "AIM_NO_SWG_REG", "AIM_FORCE_DPWAVE", "AIM_DPW_LEGACY")


def settings():
    """[(name, env, grid)]: the budgets on the full grid, then a reduced grid per knob setting."""
    base = {"AIM_SCRATCH_GB": "16", "AIM_CHIP_CUS": "256"}
    s = [("budget16", dict(base), "full"), ("budget4", dict(base, AIM_SCRATCH_GB="4"), "reduced"),
         ("budget1", dict(base, AIM_SCRATCH_GB="1"), "reduced")]
    s += [(k, dict(base, **{k: "1"}), "wfa") for k in WFA_KNOBS]
    s += [("AIM_GROUP_WLDS=80", dict(base, AIM_GROUP_WLDS="80"), "wfa"), ("AIM_GROUP_G=8", dict(base, AIM_GROUP_G="8"), "wfa")]
    s += [(k, dict(base, **{k: "1"}), "dp") for k in DP_KNOBS]
    s += [("AIM_NO_NW_REG+AIM_NO_SWG_REG", dict(base, AIM_NO_NW_REG="1", AIM_NO_SWG_REG="1"), "dp")]
    s += [("budget0.25", dict(base, AIM_SCRATCH_GB="0.25"), "dp")]   # (the smallest bound AIM_SCRATCH_GB admits)
    s += [("AIM_STRIP_K=8", dict(base, AIM_STRIP_K="8"), "dp"), ("AIM_DPL_SEQ_LDS=0", dict(base, AIM_DPL_SEQ_LDS="0"), "dp"),
          ("AIM_DPL_SEQ_LDS=1", dict(base, AIM_DPL_SEQ_LDS="1"), "dp"), ("AIM_DPL_NO_REG=1", dict(base, AIM_DPL_NO_REG="1"), "dp")]
    s += [("AIM_CHIP_CUS=64", dict(base, AIM_CHIP_CUS="64"), "reduced"), ("AIM_CHIP_CUS=304", dict(base, AIM_CHIP_CUS="304"), "reduced"),
          ("AIM_CHIP_CUS=64+budget1", dict(base, AIM_CHIP_CUS="64", AIM_SCRATCH_GB="1"), "reduced")]
    return s


def cases(grid):
    """[(tag, make_params kwargs, n_pairs)] of one grid, in a fixed order."""
    out = []
    # full: the default knobs; reduced: other budgets and chip sizes; wfa / dp: one knob setting, that family's params only
    fam, step, n_pairs = {"full": (("wfa", "dp", "genasm"), 8, N_PAIRS), "reduced": (("wfa", "dp", "genasm"), 64, N_PAIRS),
                          "wfa": (("wfa",), 128, (63, 1 << 22)), "dp": (("dp",), 128, (63, 1 << 22))}[grid]
    for rs in read_sizes(step):
        for tag, kw in param_specs(rs, fam):
            for fl in FLAGS_MAIN + (FLAGS_IO if grid == "full" and rs % 128 == 0 else ()):
                for n in n_pairs:
                    out.append((tag, dict(kw, read_size=rs, **fl), n))
    for tag, kw in EDGE:
        if tag.startswith("wfa") and "wfa" not in fam or not tag.startswith("wfa") and "dp" not in fam:
            continue
        for fl in FLAGS_MAIN:
            for n in N_PAIRS:
                out.append((tag, dict(kw, **fl), n))
    return out


def param_text(tag, kw):
    return tag + " " + " ".join("%s=%s" % (k, ",".join(map(str, v)) if isinstance(v, tuple) else v)
                                for k, v in sorted(kw.items()) if k != "algo")


def worker(grid):
    """Runs in the env setting's own process: one row per case."""
    sys.path.insert(0, ROOT)
    from aim_amd import capi, engine
    lib = capi.load()
    buf = C.create_string_buffer(1024)
    rows = []
    for tag, kw, n in cases(grid):
        kw = dict(kw)
        p = engine.make_params(kw.pop("algo"), kw.pop("max_score"), kw.pop("read_size"), **kw)
        ref = capi.params_ref(p)
        rc = lib.aim_plan_describe(ref, n, buf, len(buf))
        text = buf.value.decode() if rc == 0 else lib.aim_last_error().decode(errors="replace")
        rows.append([rc, text, int(lib.aim_scratch_bytes(ref, n))])
    json.dump(rows, sys.stdout)


def run_setting(name, env, grid):
    e = {k: v for k, v in os.environ.items() if not k.startswith("AIM_") or k == "AIM_LIB"}
    e.update(env)
    e["AIM_PLAN_DEBUG"] = "1"
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", grid], env=e, capture_output=True, text=True,
                       timeout=600)
    if r.returncode:
        raise RuntimeError("sweep worker %s failed (%d): %s" % (name, r.returncode, r.stderr[-2000:]))
    res = json.loads(r.stdout)
    rows = [["%s read_size=%d" % (tag, kw["read_size"]), param_text(tag, kw), n] + out for (tag, kw, n), out in zip(cases(grid), res)]
    # the plan lines themselves repeat the rows: the distinct other lines (wfa_group's internal one)
    echo = {"[aim plan] " + row[4] for row in rows}
    stderr = sorted({ln for ln in r.stderr.splitlines() if ln.startswith("[aim plan]") and ln not in echo})
    return {"name": name, "env": env, "grid": grid, "rows": rows, "stderr": stderr}


def sweep():
    todo = settings()
    with ThreadPoolExecutor(max(1, min(8, os.cpu_count() or 1))) as ex:
        return list(ex.map(lambda s: run_setting(*s), todo))


def digest(rows):
    return hashlib.sha256(json.dumps(rows, separators=(",", ":")).encode()).hexdigest()[:16]


def groups(setting):
    """{group key: [[params, n_pairs, rc, line or error, scratch bytes], ...]} of one setting's rows, in sweep order."""
    out = {}
    for row in setting["rows"]:
        out.setdefault(row[0], []).append(row[1:])
    return out


def golden_form(setting):
    """What the golden keeps of one setting: [key, rows, digest] per group, and [lines, digest] of the debug lines."""
    return {"name": setting["name"], "env": setting["env"], "grid": setting["grid"],
            "groups": [[k, len(v), digest(v)] for k, v in groups(setting).items()],
            "stderr": [len(setting["stderr"]), digest(setting["stderr"])]}


def main():
    data = sweep()
    with gzip.open(OUT, "wt", compresslevel=9) as f:
        json.dump([golden_form(s) for s in data], f, separators=(",", ":"))
    print("wrote %s: %d settings, %d rows" % (OUT, len(data), sum(len(d["rows"]) for d in data)))


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "--worker":
        worker(sys.argv[2])
    else:
        main()
