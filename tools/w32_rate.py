#!/usr/bin/env python3
"""32-bit WFA offset rates (AIM_FLAG_WFA_W32): aim_align_device over HBM-resident batches, timed with HIP events like bench.py.

  python tools/w32_rate.py [--steps K] [--warmup W] [--parts long,modes,genasm,slowdown] [--out FILE.jsonl]

One JSON line per row, pairs/s score-only and with CIGAR:
  long      l = 50 000 and 100 000 at e = 0.5 % and 1 %, global WFA and REDUCE (3, 4, 1), the launchers' MAX_SCORE;
  modes     affine2p (4, 4, 2, 24, 1) on --long-indel 400 pairs and ends-free (flank 100, text ends free) at l = 50 000, e = 1 %;
  genasm    edit distance (gap-linear (1, 1), MAX_SCORE = ceil(l*e)) at l = 100 000, e = 1 %, next to GenASM on the same pairs;
  slowdown  W32 against the int16 wave kernel at l = 16 000, e = 1 %, both forced onto wfa_wave_kernel (AIM_FORCE_WAVE=1),
            alternating int16 / W32 runs --rounds times in one process.
Each row records its plan line, and the statuses of one untimed run (a pair whose history outgrows a BACKTRACE arena reports
AIM_PAIR_NOMEM)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import numpy as np   # noqa: E402

from affine2p_rate import rate   # noqa: E402  (same timing loop)
from aim_amd import engine   # noqa: E402


def statuses(params, req, pat, txt):
    res, _ = engine.align(params, req, pat, txt, check=False)
    return {str(int(k)): int(v) for k, v in zip(*np.unique(res["status"], return_counts=True))}


def timed(params, req, pat, txt, steps, warmup):
    try:
        ms, pps, plan = rate(params, req, pat, txt, steps, warmup)
        return {"ms": ms, "pairs_per_s": pps, "plan": plan}
    except Exception as ex:   # (a shape the scratch bound refuses is reported, not fatal)
        return {"ms": None, "pairs_per_s": None, "plan": None, "error": str(ex)}


def row_for(name, params, req, pat, txt, a, **extra):
    r = timed(params, req, pat, txt, a.steps, a.warmup)
    row = dict(name=name, pairs=len(req), read_size=int(pat.shape[1]), max_score=params.max_score if hasattr(params, "max_score")
               else params.base.max_score, **extra, **r)
    row["status_counts"] = statuses(params, req, pat, txt)
    print(json.dumps(row), file=sys.stderr, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--pairs-50k", type=int, default=4096)
    ap.add_argument("--pairs-100k", type=int, default=2048)
    ap.add_argument("--rounds", type=int, default=3, help="slowdown: alternating int16 / W32 runs")
    ap.add_argument("--parts", default="long,modes,genasm,slowdown")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the commit the rows are measured on (default: git rev-parse --short HEAD)")
    a = ap.parse_args()
    commit = a.commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    parts = set(a.parts.split(","))
    rows = []
    if "long" in parts:
        for l in (50000, 100000):
            n = a.pairs_50k if l == 50000 else a.pairs_100k
            for err in (0.005, 0.01):
                ms, rs = engine.launcher_sizes("wfa", l, err)
                req, pat, txt = engine.gen_pairs(42, 0, n, l, err, rs)
                for red in (False, True):
                    for bt in (False, True):
                        p = engine.make_params("wfa", ms, rs, reduce=red, backtrace=bt, w32=True)
                        rows.append(row_for("reduce" if red else "global", p, req, pat, txt, a, l=l, e=err, cigar=bt))
    if "modes" in parts:
        l, err = 50000, 0.01
        ms, rs = engine.launcher_sizes("wfa", l, err, mismatch=4, gap_o=4, gap_e=2)
        req, pat, txt = engine.gen_pairs(43, 0, a.pairs_50k, l, err, rs)
        lreq, lpat, ltxt = engine.long_indel_pairs(43, 0, req, pat, txt, 400)
        for bt in (False, True):
            p = engine.make_params("wfa", ms + 24 + 400, lpat.shape[1], mismatch=4, gap_o=4, gap_e=2, gap2=(24, 1), backtrace=bt, w32=True)
            rows.append(row_for("affine2p", p, lreq, lpat, ltxt, a, l=l, e=err, cigar=bt, penalties=[4, 4, 2, 24, 1], long_indel=400))
        ms, rs = engine.launcher_sizes("wfa", l, err)
        freq, fpat, ftxt = engine.flank_pairs(44, 0, req, pat, txt, 100)
        for bt in (False, True):
            p = engine.make_params("wfa", ms, fpat.shape[1], ends_free=(0, 0, 100, 100), backtrace=bt, w32=True)
            rows.append(row_for("endsfree", p, freq, fpat, ftxt, a, l=l, e=err, cigar=bt, ends_free=[0, 0, 100, 100]))
    if "genasm" in parts:
        l, err = 100000, 0.01
        _, rs = engine.launcher_sizes("genasm", l, err)
        req, pat, txt = engine.gen_pairs(45, 0, a.pairs_100k, l, err, rs)
        ms = int(np.ceil(l * err))
        for bt in (False, True):
            p = engine.make_params("wfa", ms, rs, mismatch=1, gap_e=1, linear=True, backtrace=bt, w32=True)
            rows.append(row_for("edit_distance", p, req, pat, txt, a, l=l, e=err, cigar=bt, penalties=[1, 1]))
            g = engine.make_params("genasm", 0, rs, backtrace=bt)
            rows.append(row_for("genasm", g, req, pat, txt, a, l=l, e=err, cigar=bt))
    if "slowdown" in parts:
        l, err = 16000, 0.01
        ms, rs = engine.launcher_sizes("wfa", l, err)
        req, pat, txt = engine.gen_pairs(46, 0, a.pairs_50k, l, err, rs)
        os.environ["AIM_FORCE_WAVE"] = "1"
        try:
            for bt in (False, True):
                runs = {False: [], True: []}
                for rnd in range(a.rounds):
                    for w32 in (False, True):
                        r = timed(engine.make_params("wfa", ms, rs, backtrace=bt, w32=w32), req, pat, txt, a.steps, a.warmup)
                        runs[w32].append(r)
                ms16 = float(np.median([r["ms"] for r in runs[False]]))
                ms32 = float(np.median([r["ms"] for r in runs[True]]))
                row = dict(name="slowdown_l16000", l=l, e=err, cigar=bt, pairs=len(req), read_size=rs, max_score=ms,
                           int16_ms=[r["ms"] for r in runs[False]], w32_ms=[r["ms"] for r in runs[True]],
                           int16_pairs_per_s=len(req) / (ms16 * 1e-3), w32_pairs_per_s=len(req) / (ms32 * 1e-3),
                           w32_over_int16_time=ms32 / ms16, int16_plan=runs[False][0]["plan"], w32_plan=runs[True][0]["plan"])
                rows.append(row)
                print(json.dumps(row), file=sys.stderr, flush=True)
        finally:
            del os.environ["AIM_FORCE_WAVE"]
    with (open(a.out, "w") if a.out else sys.stdout) as f:
        for r in rows:
            r["commit"] = commit
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
