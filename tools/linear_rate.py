#!/usr/bin/env python3
"""Gap-linear WFA rates (AIM_FLAG_LINEAR): aim_align_device over HBM-resident batches, timed with HIP events like bench.py.

  python tools/linear_rate.py [--pairs N] [--steps K] [--warmup W] [--lengths 100,1000,10000] [--out FILE.jsonl]

One JSON line per (shape, penalties, CIGAR or not): pairs/s of gap-linear WFA with (x, g) = (1, 1) (edit distance) and (4, 2)
against two baselines on the same pairs: NW with the same x and g (what a user has without the flag), and global WFA
(x, o, e) = (4, 6, 2) on the same kernel family -- AIM_NO_LANE=1 AIM_NO_LANE_PK=1 for the whole process, so that global WFA runs
on wfa_group_kernel (or wfa_wave_kernel) like gap-linear does. Gap-linear MAX_SCORE: ceil(l*e) edits x max(min(x, 2g), g)
(INTEGRATION.md 7d); global WFA's and NW's are the launchers' rule. Shapes: l = 100 at e = 1 % and 5 %, l = 1000 at e = 5 %,
l = 10 000 at e = 1 %. `over_cap` is the fraction of pairs whose gap-linear score is over its MAX_SCORE. At l = 10 000 the NW
baseline is timed over --nw-long-steps steps (NW (4, 2) runs on dp_wave_kernel there, about 30 s per step)."""
import argparse
import json
import os
import subprocess
import sys

os.environ.setdefault("AIM_NO_LANE", "1")        # global WFA runs on the general kernels, like gap-linear
os.environ.setdefault("AIM_NO_LANE_PK", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np   # noqa: E402

from affine2p_rate import rate   # noqa: E402  (same timing loop)
from aim_amd import engine   # noqa: E402
from linear_model import max_score_rule   # noqa: E402

SHAPES = ((100, 0.01, 1), (100, 0.05, 1), (1000, 0.05, 8), (10000, 0.01, 256))   # (l, e, divisor of --pairs)
PENS = ((1, 1), (4, 2))


def scores(params, req, pat, txt):
    """Scores of one run through the set API (for the over-cap fraction; untimed)."""
    res, _ = engine.align(params, req, pat, txt)
    return res["score"]


def timed(params, req, pat, txt, steps, warmup):
    try:
        ms, pps, plan = rate(params, req, pat, txt, steps, warmup)
        return {"ms": ms, "pairs_per_s": pps, "plan": plan}
    except Exception as ex:   # (a baseline the scratch bound refuses is reported, not fatal)
        return {"ms": None, "pairs_per_s": None, "plan": None, "error": str(ex)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1 << 18)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--lengths", default="100,1000,10000", help="comma-separated read lengths of SHAPES to run")
    ap.add_argument("--nw-long-steps", type=int, default=1, help="timed steps of the NW baseline at l = 10 000")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the commit the rows are measured on (default: git rev-parse --short HEAD)")
    a = ap.parse_args()
    commit = a.commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    lengths = {int(v) for v in a.lengths.split(",")}
    rows = []
    for l, err, div in SHAPES:
        if l not in lengths:
            continue
        gms, rs = engine.launcher_sizes("wfa", l, err, mismatch=4, gap_o=6, gap_e=2)
        n = max(1024, a.pairs // div)
        req, pat, txt = engine.gen_pairs(42, 0, n, l, err, rs)
        for bt in (False, True):
            glob = timed(engine.make_params("wfa", gms, rs, mismatch=4, gap_o=6, gap_e=2, backtrace=bt), req, pat, txt, a.steps, a.warmup)
            for x, g in PENS:
                ms = max_score_rule(l, err, x, g)
                lin_p = engine.make_params("wfa", ms, rs, mismatch=x, gap_e=g, backtrace=bt, linear=True)
                nms, _ = engine.launcher_sizes("nw", l, err, mismatch=x, gap=g)
                nsteps = a.nw_long_steps if l >= 10000 else a.steps
                nw = timed(engine.make_params("nw", nms, rs, mismatch=x, gap=g, backtrace=bt), req, pat, txt, nsteps, a.warmup)
                lin = timed(lin_p, req, pat, txt, a.steps, a.warmup)
                over = float((scores(engine.make_params("wfa", ms, rs, mismatch=x, gap_e=g, linear=True), req, pat, txt) > ms).mean())
                row = {"l": l, "e": err, "cigar": bt, "pairs": n, "read_size": rs, "penalties": [x, g], "max_score": ms, "over_cap": over,
                       "linear_ms": lin["ms"], "linear_pairs_per_s": lin["pairs_per_s"], "linear_plan": lin["plan"],
                       "nw_max_score": nms, "nw_steps": nsteps, "nw_ms": nw["ms"], "nw_pairs_per_s": nw["pairs_per_s"], "nw_plan": nw["plan"],
                       "global_penalties": [4, 6, 2], "global_max_score": gms, "global_ms": glob["ms"],
                       "global_pairs_per_s": glob["pairs_per_s"], "global_plan": glob["plan"]}
                for k, r in (("linear_error", lin), ("nw_error", nw), ("global_error", glob)):
                    if "error" in r:
                        row[k] = r["error"]
                if lin["ms"] and nw["ms"]:
                    row["speedup_vs_nw"] = nw["ms"] / lin["ms"]
                if lin["ms"] and glob["ms"]:
                    row["speedup_vs_global"] = glob["ms"] / lin["ms"]
                rows.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
    with (open(a.out, "w") if a.out else sys.stdout) as f:
        for r in rows:
            r["commit"] = commit
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
