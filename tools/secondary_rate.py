#!/usr/bin/env python3
"""What rule 16c costs on the MI355X: aim_mapper_t with and without aim_mapper_set_secondary over the same batches.

  python tools/secondary_rate.py [--rounds 5] [--batches 4] [--out FILE.jsonl] [--shapes 0,1] [--kinds free,dup] [--only plain|secondary]
                                 [--reads N]

Shapes: batches of 1 Mi reads of l = 100 in rows of 104 and 64 Ki reads of l = 1 000 in rows of 1 024 at K = 4 (--reads overrides the
batch size). Kinds: `free`, reads from a 1 Mi-base random reference with 2 % substitutions at min_votes 3 -- next to no read has a
secondary (random k-mer hits seldom make a chain of three), so the difference is the cost of the three stages alone --, and `dup`, the same reads over a reference whose second half is a copy of the first with 1 %
of its bases changed -- every read has one secondary, whose row is a real alignment where the empty slot was a trivial one.

Both mappers live in one process and alternate: a round is `batches` batches through the plain mapper (submit on slots 0 / 1
alternately, each wait followed by the next submit on that slot), then the same batches through the mapper with secondaries (max_sec 2,
AIM_SEC_RECORDS). The medians of `rounds` rounds are reported with their ranges, in reads/s. --only runs one of the two, which is how
a library from before the feature is measured (AIM_LIB=<that build>, --only plain) in alternation with this one from a job script.
The first batch is described in the row: how many records of the two mappers differ (random k-mer hits give a few reads of the `free`
kind a secondary too), how many locus records have a family of two or more, how many 0x100 lines there are and how many records reach MAPQ 20 with
and without the feature. One JSON line per row.
The per-kernel times of the four kernels come from a kernel-trace run of this tool (profiles/secondary/README.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K = 4
#         l, read_size, reads per batch, (k, w, max_occ, band, flank, min_votes), max_score
SHAPES = ((100, 104, 1 << 20, (11, 5, 16, 32, 8, 3), 24), (1000, 1024, 1 << 16, (11, 10, 8, 96, 16, 3), 120))
X, O, E = 3, 4, 1
REF_LEN = 1 << 20
BASES = np.frombuffer(b"ACGT", dtype=np.uint8)


def make_reference(kind, seed=5):
    rng = np.random.default_rng(seed)
    ref = BASES[rng.integers(0, 4, size=REF_LEN)].copy()
    if kind == "dup":
        half = REF_LEN // 2
        ref[half:] = ref[:half]
        at = half + rng.choice(half, size=half // 100, replace=False)
        ref[at] = BASES[(np.searchsorted(BASES, ref[at]) + 1) % 4]          # (ACGT is sorted: A C G T)
    return ref


def make_batches(ref, kind, l, rs, n, batches, seed=6):
    rng = np.random.default_rng(seed)
    comp = np.arange(256, dtype=np.uint8)
    for a, b in (b"AT", b"TA", b"CG", b"GC"):
        comp[a] = b
    out = []
    span = (REF_LEN // 2 if kind == "dup" else REF_LEN) - l
    for _ in range(batches):
        pos = rng.integers(0, span, size=n)
        rows = np.zeros((n, rs), dtype=np.uint8)
        rows[:, :l] = ref[pos[:, None] + np.arange(l)[None, :]]
        sub = rng.random((n, l)) < 0.02
        rows[:, :l][sub] = BASES[rng.integers(0, 4, size=int(sub.sum()))]
        minus = np.arange(n) % 2 == 1
        rows[minus, :l] = comp[rows[minus, :l][:, ::-1]]
        out.append((np.full(n, l, dtype=np.int32), rows))
    return out


def run(m, batches):
    """`batches` through the two slots; seconds."""
    t0 = time.perf_counter()
    for b, (rl, rows) in enumerate(batches):
        slot = b & 1
        if b >= 2:
            m.wait(slot)
        m.submit(slot, rl, rows)
    for b in range(max(0, len(batches) - 2), len(batches)):
        m.wait(b & 1)
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--kinds", default="free,dup")
    ap.add_argument("--only", default=None, choices=("plain", "secondary"))
    ap.add_argument("--reads", type=int, default=None)
    args = ap.parse_args()
    from aim_amd import capi, engine
    from gpu_buffers import copy_out
    if args.only == "plain":
        capi.load(strict=False)                          # (a build of the parent lacks the symbols this commit adds)
    fh = open(args.out, "a") if args.out else None
    for si in [int(x) for x in args.shapes.split(",")]:
        l, rs, n, (k, w, max_occ, band, flank, min_votes), max_score = SHAPES[si]
        n = args.reads or n
        for kind in args.kinds.split(","):
            ref = make_reference(kind)
            batches = make_batches(ref, kind, l, rs, n, args.batches)
            sp = engine.seed_params(k, rs, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, max_cands=K, w=w)
            mp = engine.mapper_params(sp, n, max_score, mismatch=X, gap_o=O, gap_e=E, slots=2, cigar_cap=n * K * 8, md_cap=n * K * 16)
            mappers = {}
            if args.only != "secondary":
                mappers["plain"] = engine.Mapper(mp, ref)
            if args.only != "plain":
                mappers["secondary"] = engine.Mapper(mp, ref)
                mappers["secondary"].set_secondary(engine.secondary_params(2, records=True))
            first = {}
            for name, m in mappers.items():                      # warm-up and the check
                m.submit(0, *batches[0])
                first[name] = copy_out(m.wait(0))
            row = {"l": l, "read_size": rs, "reads": n, "kind": kind, "batches": args.batches, "rounds": args.rounds, "lib": os.path.basename(capi.LIB_PATH)}
            for name, out in first.items():
                rec = out["records"]
                row[name + "_records"] = int(len(rec))
                row[name + "_unmapped"] = int((rec["sam"]["flags"] & capi.SAM_UNMAPPED != 0).sum())
            if "secondary" in first:
                sec = first["secondary"]["sec"]
                lines = (first["secondary"]["records"]["sam"]["flags"] & capi.SAM_SECONDARY) != 0
                row["secondary_lines"] = int(lines.sum())
                row["with_secondary"] = int(((sec["n_members"] >= 2) & ~lines).sum())
                row["mapq_ge_20"] = int((first["secondary"]["records"]["mapq"][~lines] >= 20).sum())
                if kind == "free" and "plain" in first:
                    a, b = first["secondary"]["records"].copy(), first["plain"]["records"].copy()
                    for r in (a, b):                             # (where a row's words and bytes land depends on scheduling)
                        r["sam"]["cigar_offset"] = 0
                        r["sam"]["md_offset"] = 0
                    row["records_that_differ"] = int((a.view(np.uint8).reshape(-1, 64) != b.view(np.uint8).reshape(-1, 64)).any(axis=1).sum()) if len(a) == len(b) else -1
            if "plain" in first:
                row["plain_mapq_ge_20"] = int((first["plain"]["records"]["mapq"] >= 20).sum())
            times = {name: [] for name in mappers}
            for _ in range(args.rounds):
                for name, m in mappers.items():
                    times[name].append(run(m, batches))
            for name, ts in times.items():
                rate = sorted(n * args.batches / t for t in ts)
                row[name + "_reads_per_s"] = round(rate[len(rate) // 2])
                row[name + "_range"] = [round(rate[0]), round(rate[-1])]
            if len(times) == 2:
                row["secondary_over_plain"] = round(row["secondary_reads_per_s"] / row["plain_reads_per_s"], 4)
            for m in mappers.values():
                m.close()
            line = json.dumps(row)
            print(line, flush=True)
            if fh:
                fh.write(line + "\n")
                fh.flush()


if __name__ == "__main__":
    main()
