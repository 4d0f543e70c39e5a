#!/usr/bin/env python3
"""The three kernels of rule 17c (AIM_FEATURE_PAIR_SECONDARY) next to their rule-14c counterparts, stage by stage on the same slot
tables: the synthetic tables of tests/pair_secondary_batch.py (4 096 reads of K = 4, primaries and aligned secondaries) tiled to the
batch size. One JSON line per stage with the median and the range of the rounds; the two builds of a stage alternate inside a round.

  python tools/pair_secondary_rate.py [--pairs 65536] [--K 4] [--rounds 5] [--reps 20] [--trace]
  python tools/pair_secondary_rate.py --mapper [--pairs 65536] [--rounds 5]

--mapper: the mapper end to end on tools/pair_rate.py's library (100-base mates, fragments of 300..500, K = 4) with
set_pairing_secondary, with set_pairing alone and with set_secondary alone -- the three alternate inside a round, medians of the rounds --
on the repeat-free batch and on a batch in which every pair lies inside an exact two-copy repeat (the first Mi of the reference copied
2 Mi further on).

A round times `reps` enqueues of one stage between two events; apply rewrites the slot arrays, so select runs on buffers restored by
a device copy inside the timed span, for both builds alike (its cost is the line "restore"). --trace: one pass over all six stages,
for a kernel trace (rocprofv3 --kernel-trace --stats) taken in a run of its own (profiles/pair_secondary/README.md)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
CIGAR_BASE, MD_BASE = 1000, 70000


def tiled(K, n_reads):
    """pair_secondary_batch.tables(21, K, 4096, False), every array repeated to n_reads reads (a multiple of 4096)."""
    import pair_secondary_batch as pb
    base = 4096
    assert n_reads % base == 0
    t = pb.tables(21, K, base, False)
    rep = n_reads // base
    out = dict(t)
    for k in ("seg", "sam", "cls", "chains", "sec", "res_sam", "read_len"):
        out[k] = np.tile(t[k], rep)
    out["reads"] = np.tile(t["reads"], (rep, 1))
    return out


def mapper_rates(n_pairs, rounds):
    import time
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import pair_rate as pr
    from aim_amd import engine
    L = 100
    read_size, mp = pr.params(L, 2 * n_pairs)
    for batch in ("repeat_free", "repeat_in_every_pair"):
        ref, rows, rl = pr.reads(n_pairs, L, read_size, 0)
        if batch != "repeat_free":                            # every fragment inside the first Mi, which has an exact copy 2 Mi further on
            ref = ref.copy()
            ref[2 << 20:3 << 20] = ref[:1 << 20]
            rng = np.random.default_rng(6)
            p, F = rng.integers(1000, (1 << 20) - 2000, size=n_pairs), rng.integers(300, 501, size=n_pairs)
            for m in range(n_pairs):
                rows[2 * m, :L], rows[2 * m + 1, :L] = ref[p[m]:p[m] + L], pr._COMP[ref[p[m] + F[m] - L:p[m] + F[m]]][::-1]
        pp = engine.pair_params(300, 500, 17, rescue=True, rescue_size=pr.RESCUE_SIZE, rescue_cigar_cap=2 * n_pairs * 16, rescue_md_cap=2 * n_pairs * 64)
        sc = engine.secondary_params(2, records=True)
        setups = {"combined": lambda m: m.set_pairing_secondary(pp, sc), "pairing_alone": lambda m: m.set_pairing(pp), "secondary_alone": lambda m: m.set_secondary(sc)}
        mappers = {}
        try:
            for name, setup in setups.items():
                mappers[name] = engine.Mapper(mp, ref)
                setup(mappers[name])
            times, stats = {k: [] for k in setups}, {}
            for i in range(rounds + 1):                       # the first round warms up
                for name, m in mappers.items():
                    t0 = time.perf_counter()
                    m.submit(0, rl, rows)
                    out = m.wait(0)
                    times[name].append(time.perf_counter() - t0)
                    if i == 0:
                        st = {"records": int(len(out["records"]))}
                        if "pairs" in out:
                            f = out["pairs"]["flags"]
                            st.update(proper=int((f & 1).sum()), tried=int(((f & 0x6) != 0).sum()), rescued=int(((f & 0x18) != 0).sum()))
                        if "pair_mapq" in out:
                            st.update(mapq_ge_20=int((out["pair_mapq"]["mapq"] >= 20).sum()), tied_reads=int((out["pair_mapq"]["tied"] > 0).sum()))
                        stats[name] = st
            row = {"batch": batch, "pairs": n_pairs}
            for name in setups:
                t = [1e3 * x for x in times[name][1:]]
                row[name + "_ms"] = round(statistics.median(t), 3)
                row[name + "_range"] = [round(min(t), 3), round(max(t), 3)]
                row[name] = stats[name]
            print(json.dumps(row), flush=True)
        finally:
            for m in mappers.values():
                m.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=65536)
    ap.add_argument("--K", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--mapper", action="store_true")
    a = ap.parse_args()
    if a.mapper:
        mapper_rates(a.pairs, a.rounds)
        return
    import torch
    import pair_secondary_batch as pb
    from aim_amd import engine
    from gpu_buffers import put, zeros
    dev = torch.device("cuda:0")
    K, n = a.K, 2 * a.pairs
    t = tiled(K, n)
    rs, rz = pb.READ_SIZE, pb.RESCUE_SIZE
    p = pb.params()
    pp = engine.pair_params(p.min_span, p.max_span, p.unpaired_penalty, rescue=True, rescue_size=rz)
    names = ("seg", "sam", "cls", "sec")
    keep = {k: put(t[k], dev) for k in names}                     # what apply rewrites, as the stage finds it
    work = {k: torch.empty_like(v) for k, v in keep.items()}
    d_rl, d_reads, d_res_sam, d_chains = put(t["read_len"], dev), put(t["reads"], dev, 16), put(t["res_sam"], dev), put(t["chains"], dev)
    d_req, d_tp, d_pat = zeros(16 * n, dev), zeros(8 * n, dev), zeros(n * rz, dev)
    d_pairs, d_pq = zeros(32 * (n // 2), dev), zeros(16 * (n // 2), dev)
    d_off, d_rec, d_msec, d_mates = zeros(4 * (n + 1), dev), zeros(64 * n * K, dev), zeros(16 * n * K, dev), zeros(16 * n * K, dev)
    sb = engine.map_records_scratch(n)
    d_scr = zeros(sb, dev)
    P = lambda x: x.data_ptr()

    def restore():
        for k in names:
            work[k].copy_(keep[k])

    def rows14():
        engine.pair_rescue_rows_device(pp, K, rs, t["ref_len"], n, P(d_rl), P(d_reads), P(keep["seg"]), P(keep["sam"]), P(d_req), P(d_tp), P(d_pat))

    def rows17():
        engine.pair_rescue_rows_secondary_device(pp, K, rs, t["ref_len"], n, P(d_rl), P(d_reads), P(keep["seg"]), P(keep["sam"]), P(keep["sec"]), P(d_req), P(d_tp), P(d_pat))

    def select14():
        restore()
        engine.pair_select_device(pp, K, rs, n, P(d_rl), P(work["seg"]), P(work["sam"]), P(work["cls"]), P(d_res_sam), CIGAR_BASE, MD_BASE, P(d_pairs))

    def select17():
        restore()
        engine.pair_select_secondary_device(pp, K, rs, n, P(d_rl), P(work["seg"]), P(work["sam"]), P(work["cls"]), P(work["sec"]), P(d_chains), pb.SCORE_UNIT, P(d_res_sam),
                                            CIGAR_BASE, MD_BASE, P(d_pairs), P(d_pq))

    def mates14():
        engine.map_mates_device(K, n, P(d_pairs), P(work["seg"]), P(work["sam"]), P(d_off), P(d_rec), P(d_mates))

    def mates17():
        engine.map_mates_secondary_device(K, n, P(d_pairs), P(work["seg"]), P(work["sam"]), P(work["sec"]), P(d_off), P(d_rec), P(d_mates))

    def records(secondary):                                        # the record list the mate fields run behind
        if secondary:
            engine.map_records_secondary_device(K, n, 1, P(work["seg"]), P(work["sam"]), P(work["cls"]), P(work["sec"]), P(d_off), P(d_rec), P(d_msec), P(d_scr), sb)
        else:
            engine.map_records_device(K, n, P(work["seg"]), P(work["sam"]), P(work["cls"]), P(d_off), P(d_rec), P(d_scr), sb)

    if a.trace:
        rows14(); rows17(); select14(); records(False); mates14(); select17(); records(True); mates17()
        torch.cuda.synchronize()
        print(json.dumps({"trace": True, "pairs": a.pairs, "K": K}))
        return

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * e0.elapsed_time(e1) / a.reps               # microseconds per enqueue

    res = {}
    select14(); records(False)
    stages = [("restore", restore, restore), ("rescue_rows", rows14, rows17), ("select_with_restore", select14, select17)]
    for name, f14, f17 in stages:
        f14(); f17()                                               # warm up
        x, y = [], []
        for _ in range(a.rounds):
            x.append(timed(f14))
            y.append(timed(f17))
        res[name] = (x, y)
    select14(); records(False); mates14()
    x = [timed(mates14) for _ in range(a.rounds)]
    select17(); records(True); mates17()
    y = [timed(mates17) for _ in range(a.rounds)]
    res["mates"] = (x, y)
    pq = np.frombuffer(d_pq.cpu().numpy().tobytes(), dtype=engine.capi.MAP_PAIR_MAPQ_DTYPE)[:n // 2]
    pairs = np.frombuffer(d_pairs.cpu().numpy().tobytes(), dtype=engine.capi.MAP_PAIR_DTYPE)[:n // 2]
    print(json.dumps({"pairs": a.pairs, "K": K, "proper": int((pairs["flags"] & 1).sum()), "rescued": int(((pairs["flags"] & 0x18) != 0).sum()),
                      "mapq_ge_20": int((pq["mapq"] >= 20).sum()), "tied_reads": int((pq["tied"] > 0).sum())}))
    for name, (x, y) in res.items():
        print(json.dumps({"stage": name, "rule14c_us": round(statistics.median(x), 2), "rule14c_range": [round(min(x), 2), round(max(x), 2)],
                          "rule17c_us": round(statistics.median(y), 2), "rule17c_range": [round(min(y), 2), round(max(y), 2)]}), flush=True)


if __name__ == "__main__":
    main()
