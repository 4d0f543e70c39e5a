#!/usr/bin/env python3
"""Sensitivity of (w, k) minimizer seeding next to stride seeding, from the rule alone (tests/minimizer_model.py and tests/seed_model.py,
numpy on the CPU; the index is the library's host build): the share of reads whose true position is among the K candidates.

  python tools/minimizer_sensitivity.py [--k 11] [--w 5,10,19] [--reads 1000] [--length 100] [--errors 2,5] [--log2 20] [--out FILE.jsonl]

Reads are windows of a seeded random reference with e % sequential uniform substitutions, insertions and deletions (seed_model.edit),
every second one reverse-complemented. Per (w, e) one row for the minimizers of (k, w) over the minimizer index and one for stride
ceil((w + 1) / 2) over the full index -- the same expected number of seeds -- at max_occ 16, band 8, flank 8, min_votes 2, K = 4. A
read counts as found when a candidate of its strand overlaps at least half of its true window."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KW = dict(max_occ=16, band=8, flank=8, min_votes=2, K=4)


def main():
    import minimizer_model as mm
    import seed_model as m
    from aim_amd import engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", type=int, default=11)
    ap.add_argument("--w", default="5,10,19")
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--length", type=int, default=100)
    ap.add_argument("--errors", default="2,5")
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--out")
    a = ap.parse_args()
    k, L = a.k, a.length
    rs = (L + L // 10 + 7) // 8 * 8
    rng = np.random.default_rng(17)
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=1 << a.log2)].copy()
    full = engine.build_index(ref, k, threads=8)
    rows = []
    for e in [int(x) for x in a.errors.split(",")]:
        reads = []
        for r in range(a.reads):
            p = int(rng.integers(0, len(ref) - L))
            read = m.edit(rng, ref[p:p + L], -(-L * e // 100))[:rs]
            reads.append((p, r & 1, m.revcomp(read) if r & 1 else read))
        for w in [int(x) for x in a.w.split(",")]:
            stride = (w + 2) // 2
            mini = engine.index_build_minimizers(ref, k, w, threads=8)
            for mode in ("minimizers", "stride"):
                found = hits = trunc = 0
                for p, strand, read in reads:
                    if mode == "minimizers":
                        cands, n_hits, flags = mm.seed_read(read, *mini, len(ref), k=k, w=w, read_size=rs, **KW)
                    else:
                        cands, n_hits, flags = m.seed_read(read, *full, len(ref), k=k, stride=stride, read_size=rs, **KW)
                    found += any(s == strand and min(start + tlen, p + L) - max(start, p) >= L // 2 for start, s, tlen, _ in cands)
                    hits += sum(n_hits)
                    trunc += bool(flags)
                rows.append(dict(part="sensitivity", mode=mode, k=k, w=w, stride=1 if mode == "minimizers" else stride, error_percent=e, length=L,
                                 reads=a.reads, ref_len=len(ref), **KW, true_position_among_candidates=round(found / a.reads, 4),
                                 hits_per_strand=round(hits / a.reads / 2, 2), truncated_share=round(trunc / a.reads, 4)))
                print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
