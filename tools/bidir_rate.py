#!/usr/bin/env python3
"""Bidirectional WFA rates (AIM_FLAG_WFA_BIDIR): aim_align_device over HBM-resident batches, timed with HIP events like bench.py
(the timing loop of tools/affine2p_rate.py, as tools/w32_rate.py uses it).

  python tools/bidir_rate.py [--steps K] [--warmup W] [--parts long,mid,short,nomem] [--out FILE.jsonl]

One JSON line per row, pairs/s of global gap-affine WFA (3, 4, 1) at the launchers' MAX_SCORE:
  long   l = 100 000 (e = 1 %, 2 %; 2 048 pairs) and l = 50 000 (e = 1 %, 4 096 pairs), W32: flag-less CIGAR, bidir, score-only;
  mid    l = 10 000 and 16 000 at e = 1 % and 5 %, int16: flag-less CIGAR (wfa_group / wfa_wave) and bidir;
  short  l = 1 000, e = 5 %, 262 144 pairs and l = 100, e = 1 %, 4 Mi pairs: flag-less CIGAR and bidir;
  nomem  l = 100 000, e = 1 %, 2 048 pairs under AIM_SCRATCH_GB=2: flag-less CIGAR (pairs report AIM_PAIR_NOMEM) and bidir.
Each row records its plan line and the statuses of one untimed run."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from aim_amd import engine   # noqa: E402
from w32_rate import row_for   # noqa: E402  (same rows: timing loop, plan line, status counts)


def three(name, l, err, n, w32, a, rows, kinds=("cigar", "bidir", "score"), **extra):
    ms, rs = engine.launcher_sizes("wfa", l, err)
    req, pat, txt = engine.gen_pairs(42, 0, n, l, err, rs)
    for kind in kinds:
        p = engine.make_params("wfa", ms, rs, backtrace=kind != "score", bidir=kind == "bidir", w32=w32)
        rows.append(row_for(name, p, req, pat, txt, a, l=l, e=err, kind=kind, w32=w32, **extra))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--parts", default="long,mid,short,nomem")
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the commit the rows are measured on (default: git rev-parse --short HEAD)")
    a = ap.parse_args()
    commit = a.commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    parts = set(a.parts.split(","))
    rows = []
    if "long" in parts:
        three("long", 100000, 0.01, 2048, True, a, rows)
        three("long", 50000, 0.01, 4096, True, a, rows)
        three("long", 100000, 0.02, 2048, True, a, rows)
    if "mid" in parts:
        for l, n in ((10000, 4096), (16000, 2048)):
            for err in (0.01, 0.05):
                three("mid", l, err, n, False, a, rows, kinds=("cigar", "bidir"))
    if "short" in parts:
        three("short", 1000, 0.05, 262144, False, a, rows, kinds=("cigar", "bidir"))
        three("short", 100, 0.01, 4 << 20, False, a, rows, kinds=("cigar", "bidir"))
    if "nomem" in parts:
        os.environ["AIM_SCRATCH_GB"] = "2"
        try:
            three("nomem", 100000, 0.01, 2048, True, a, rows, kinds=("cigar", "bidir"), scratch_gb=2)
        finally:
            del os.environ["AIM_SCRATCH_GB"]
    with (open(a.out, "w") if a.out else sys.stdout) as f:
        for r in rows:
            r["commit"] = commit
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
