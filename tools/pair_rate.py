#!/usr/bin/env python3
"""Throughput of the mapper with pairing (rule 14c, AIM_FEATURE_PAIRED) against the same reads mapped single-end, with and without the
rescue, and the plan lines of the segment alignment and of the rescue alignment at rescue_size 512 (which kernel each planned onto).
One JSON line per read length with the plans, then one per configuration.

  python tools/pair_rate.py [--pairs 65536] [--lens 100,150] [--rescue 0,10,100] [--rounds 5] [--lib-parent PATH]

Reads: mate pairs cut from a seeded random reference of 4 Mi bases, fragments of 300..500 bases, K = 4. `--rescue P`: in P % of the pairs
mate 2 carries a substitution every 10th base, so it has no chain and only the rescue places it. With --lib-parent the single-end run is
repeated in a child process on that build of the library (AIM_LIB, a build of the parent commit), configuration by configuration, so the two
builds alternate; medians over the rounds. The kernels' own times come from a kernel trace (rocprofv3 --kernel-trace --stats) of this tool, taken in a run of its own
(profiles/pairs/README.md)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF_LEN, REF_SEED = 1 << 22, 99
RESCUE_SIZE = 512
_COMP = np.zeros(256, dtype=np.uint8)
for _a, _b in zip(b"ACGT", b"TGCA"):
    _COMP[_a] = _b


def reads(n_pairs, L, read_size, rescue_pct, seed=5):
    rng = np.random.default_rng(seed)
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(REF_SEED).integers(0, 4, size=REF_LEN)].copy()
    rows = np.zeros((2 * n_pairs, read_size), dtype=np.uint8)
    p = rng.integers(1000, REF_LEN - 2000, size=n_pairs)
    F = rng.integers(300, 501, size=n_pairs)
    lost = rng.random(n_pairs) * 100 < rescue_pct
    sub = np.frombuffer(b"CGTA", dtype=np.uint8)
    code = np.zeros(256, dtype=np.uint8)
    code[list(b"ACGT")] = range(4)
    for m in range(n_pairs):
        a, b = ref[p[m]:p[m] + L], ref[p[m] + F[m] - L:p[m] + F[m]].copy()
        if lost[m]:
            b[5::10] = sub[code[b[5::10]]]
        rows[2 * m, :L], rows[2 * m + 1, :L] = a, _COMP[b][::-1]
    return ref, rows, np.full(2 * n_pairs, L, dtype=np.int32)


def params(L, n_reads):
    from aim_amd import engine
    read_size = (L + 4 + 7) // 8 * 8
    sp = engine.seed_params(11, read_size, max_occ=8, band=16, flank=2, min_votes=3, max_cands=4, w=5)
    return read_size, engine.mapper_params(sp, n_reads, 40 + 3 * (L // 10 - 10), slots=1)


def plan_lines(L, n_pairs):
    """(the segment alignment's plan line, the rescue alignment's at rescue_size 512): what aim_plan_describe says the two
    aim_align_device_ref calls of a batch follow in this process -- the kernel each planned onto comes first."""
    import ctypes as C
    from aim_amd import capi, engine
    read_size, mp = params(L, 2 * n_pairs)
    out = []
    for rs, free, rows_n in ((read_size, 2 * mp.seed.flank, 2 * n_pairs * mp.seed.max_cands), (RESCUE_SIZE, RESCUE_SIZE, 2 * n_pairs)):
        p = engine.make_params("wfa", mp.max_score, rs, mismatch=mp.mismatch, gap_o=mp.gap_o, gap_e=mp.gap_e, backtrace=True, ref_texts=True, ends_free=(0, 0, free, free))
        buf = C.create_string_buffer(1024)
        capi.check(capi.load().aim_plan_describe(capi.params_ref(p), rows_n, buf, len(buf)))
        out.append(buf.value.decode())
    return out


def time_mapper(L, n_pairs, rescue_pct, paired, rounds, rescue=True):
    from aim_amd import engine
    read_size, mp = params(L, 2 * n_pairs)
    ref, rows, rl = reads(n_pairs, L, read_size, rescue_pct)
    times = []
    with engine.Mapper(mp, ref) as m:
        if paired:
            m.set_pairing(engine.pair_params(300, 500, 17, rescue=rescue, rescue_size=RESCUE_SIZE, rescue_cigar_cap=2 * n_pairs * 16, rescue_md_cap=2 * n_pairs * 64))
        out = None
        for i in range(rounds + 1):                      # the first round warms up
            t0 = time.perf_counter()
            m.submit(0, rl, rows)
            out = m.wait(0)
            times.append(time.perf_counter() - t0)
        res = {"records": int(len(out["records"]))}
        if paired:
            f = out["pairs"]["flags"]
            res.update(proper=int((f & 1).sum()), rescued=int(((f & 0x18) != 0).sum()), tried=int(((f & 0x6) != 0).sum()))
    res["seconds"] = times[1:]
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=65536)
    ap.add_argument("--lens", default="100,150")
    ap.add_argument("--rescue", default="0,10,100")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--lib-parent", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:                                          # one single-end measurement on the library AIM_LIB names
        from aim_amd import capi
        capi.load(strict=False)                          # (a build of the parent lacks the symbols this commit adds)
        L, pct = (int(x) for x in a.child.split(","))
        print(json.dumps(time_mapper(L, a.pairs, pct, False, a.rounds)))
        return
    for L in (int(x) for x in a.lens.split(",")):
        seg_plan, rescue_plan = plan_lines(L, a.pairs)
        print(json.dumps({"read_len": L, "pairs": a.pairs, "segment_plan": seg_plan, "rescue_plan": rescue_plan}), flush=True)
        for pct in (int(x) for x in a.rescue.split(",")):
            single = time_mapper(L, a.pairs, pct, False, a.rounds)
            paired = time_mapper(L, a.pairs, pct, True, a.rounds)
            bare = time_mapper(L, a.pairs, pct, True, a.rounds, rescue=False)      # select and mate fields alone: the rest is the rescue's cost
            row = {"read_len": L, "pairs": a.pairs, "rescue_pct": pct, "single_ms": 1e3 * statistics.median(single["seconds"]),
                   "paired_ms": 1e3 * statistics.median(paired["seconds"]), "paired_no_rescue_ms": 1e3 * statistics.median(bare["seconds"]),
                   "proper": paired["proper"], "tried": paired["tried"], "rescued": paired["rescued"]}
            row["paired_over_single"] = row["paired_ms"] / row["single_ms"]
            row["pairs_per_s"] = a.pairs / (row["paired_ms"] * 1e-3)
            if a.lib_parent:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "%d,%d" % (L, pct), "--pairs", str(a.pairs), "--rounds", str(a.rounds)],
                                   env=dict(os.environ, AIM_LIB=a.lib_parent), capture_output=True, text=True, timeout=600)
                if p.returncode:
                    raise SystemExit(p.stderr)
                row["parent_single_ms"] = 1e3 * statistics.median(json.loads(p.stdout.strip().splitlines()[-1])["seconds"])
            print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
