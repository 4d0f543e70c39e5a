#!/usr/bin/env python3
"""What estimating the span bounds on the device (rule 15c, AIM_FEATURE_PAIR_ESTIMATE) costs the paired mapper, in tools/pair_rate.py's
configuration: 65 536 pairs of 100-base reads per batch, K = 4, fragments of 300..500 bases, 10 % of the pairs needing the rescue.

  python tools/pair_estimate_rate.py [--pairs 65536] [--len 100] [--rescue 10] [--rounds 5] [--reps 3] [--lib-parent PATH]

Configurations, each in a child process of its own, one after the other inside a round, so the builds alternate:
  est          this build, Mapper.set_pairing(pp, estimate=...) with the fallback 0..1000 and rescue_size 1104
  wide         this build, plain set_pairing with 0..1000 at rescue_size 1104
  true         this build, plain set_pairing with the true 300..500 at rescue_size 512
  parent_wide  } the same two on the library --lib-parent names (a build of the parent commit, through AIM_LIB)
  parent_true  }
est against parent_wide is the like-for-like cost of the estimate; est against parent_true is what a user without prior knowledge still
pays for the larger rescue rows. A child times --reps batches behind one warm-up batch; the figure of a configuration is the median over
all rounds and repetitions. `--trace`: one process, the est configuration alone, for a kernel trace taken in a run of its own
(rocprofv3 --kernel-trace --stats -- python tools/pair_estimate_rate.py --trace; profiles/pair_estimate/README.md)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"est": (0, 1000, 1104, True), "wide": (0, 1000, 1104, False), "true": (300, 500, 512, False)}


def time_config(name, L, n_pairs, rescue_pct, reps):
    import pair_rate
    from aim_amd import engine
    lo, hi, rz, estimate = CONFIGS[name]
    read_size, mp = pair_rate.params(L, 2 * n_pairs)
    ref, rows, rl = pair_rate.reads(n_pairs, L, read_size, rescue_pct)
    times = []
    with engine.Mapper(mp, ref) as m:
        pp = engine.pair_params(lo, hi, 17, rescue=True, rescue_size=rz, rescue_cigar_cap=2 * n_pairs * 16, rescue_md_cap=2 * n_pairs * 64)
        if estimate:
            m.set_pairing(pp, estimate=engine.pair_estimate_params())
        else:
            m.set_pairing(pp)
        out = None
        for _ in range(reps + 1):                        # the first batch warms up
            t0 = time.perf_counter()
            m.submit(0, rl, rows)
            out = m.wait(0)
            times.append(time.perf_counter() - t0)
        f = out["pairs"]["flags"]
        res = {"records": int(len(out["records"])), "proper": int((f & 1).sum()), "rescued": int(((f & 0x18) != 0).sum()), "tried": int(((f & 0x6) != 0).sum()),
               "seconds": times[1:]}
        if estimate:
            res["estimate"] = out["pair_estimate"]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=65536)
    ap.add_argument("--len", type=int, default=100)
    ap.add_argument("--rescue", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--lib-parent", default=None)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child or a.trace:
        from aim_amd import capi
        capi.load(strict=False)                          # (a build of the parent lacks the symbols this commit adds)
        print(json.dumps(time_config(a.child or "est", a.len, a.pairs, a.rescue, a.reps)))
        return
    runs = [(c, None) for c in ("est", "wide", "true")] + ([("wide", a.lib_parent), ("true", a.lib_parent)] if a.lib_parent else [])
    seconds, last = {}, {}
    for _ in range(a.rounds):
        for cfg, lib in runs:
            key = ("parent_" if lib else "") + cfg
            env = dict(os.environ, AIM_LIB=lib) if lib else dict(os.environ)
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", cfg, "--pairs", str(a.pairs), "--len", str(a.len), "--rescue", str(a.rescue),
                                "--reps", str(a.reps)], env=env, capture_output=True, text=True, timeout=900)
            if p.returncode:
                raise SystemExit(p.stderr)
            last[key] = json.loads(p.stdout.strip().splitlines()[-1])
            seconds.setdefault(key, []).extend(last[key]["seconds"])
    for key, s in seconds.items():
        row = {"config": key, "pairs": a.pairs, "read_len": a.len, "rescue_pct": a.rescue, "ms_median": 1e3 * statistics.median(s), "ms_min": 1e3 * min(s),
               "ms_max": 1e3 * max(s), "n": len(s)}
        row.update({k: v for k, v in last[key].items() if k != "seconds"})
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
