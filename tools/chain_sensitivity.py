#!/usr/bin/env python3
"""Voting against chaining on the same reads, from the rules alone (tests/minimizer_model.py and tests/chain_model.py, numpy on the CPU;
the index is the library's host build).

  python tools/chain_sensitivity.py [--reads 1000] [--k 11] [--w 10] [--bands 8,32,256] [--cases 300:5,...] [--log2 20] [--out FILE.jsonl]
  python tools/chain_sensitivity.py --max-hits 4096 --reads 100 --bands 256 --cases 10000:5,20000:15,10000:3:600 [--out FILE.jsonl]

The reference is seeded random sequence with 40 diverged copies (3 % edits) of a 600-base element. A read is a window of it with e %
sequential uniform substitutions, insertions and deletions (seed_model.edit), or with D reference bases deleted in its middle and 3 %
edits; every second one is reverse-complemented. Both methods run over the (w, k) minimizer index at max_occ 16, flank 16,
min_votes 2, K = 4. Per case, method and band, two shares of the reads:
  any_of_k_covers   a candidate of the read's strand covers the true span [p, p + span) to within 8 bases at both ends;
  rank0_tight       candidate 0 does, and its window is no longer than span + 2 * flank + 40.
The default cases are L = 300 / 1 000 / 3 000 at e = 5 / 10 / 15 % and L = 1 000 with one 80- and one 200-base deletion. Rows go to
stdout and, with --out, to a JSON-lines file (profiles/chain/sensitivity.jsonl is the recorded run).
With --max-hits H the rows are those of aim_seed_chain_long_device's rule (tests/chain_long_model.py: the hit cap H, rows up to 65 528
bases) and there is no voting row: such reads are beyond aim_seed_device (profiles/chain_long/sensitivity.jsonl)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

KW = dict(max_occ=16, flank=16, min_votes=2, K=4)
SLACK, EXTRA = 8, 40
DEFAULT_CASES = ",".join("%d:%d" % (L, e) for L in (300, 1000, 3000) for e in (5, 10, 15)) + ",1000:3:80,1000:3:200"


def make_reference(rng, log2):
    import seed_model as m
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=1 << log2)].copy()
    element = ref[1000:1600].copy()
    for _ in range(40):
        at = int(rng.integers(5000, len(ref) - 5000))
        copy = m.edit(rng, element, 18)[:600]
        ref[at:at + len(copy)] = copy
    return ref


def judge(cands, p, span, strand):
    """(any of K covers, rank 0 covers and is tight) for candidates [(start, strand, text_len, ...)]."""
    covers = lambda c: c[1] == strand and c[0] <= p + SLACK and c[0] + c[2] >= p + span - SLACK
    return any(covers(c) for c in cands), bool(cands) and covers(cands[0]) and cands[0][2] <= span + 2 * KW["flank"] + EXTRA


def chain_candidates(batch, index, ref_len, k, w, band, rs, max_hits=0):
    """chain_model.seed_chain (max_hits = 0) or chain_long_model.seed_chain_long over a batch of reads, as [(start, strand, text_len,
    score)] per read."""
    import chain_long_model as clm
    import chain_model as cm
    rows = np.zeros((len(batch), rs), dtype=np.uint8)
    rl = np.zeros(len(batch), dtype=np.int32)
    for i, read in enumerate(batch):
        rows[i, :len(read)], rl[i] = read, len(read)
    if max_hits:
        req, tpos, votes, seeds, _ = clm.seed_chain_long(rows, rl, index, ref_len, k, w, KW["max_occ"], band, KW["flank"], KW["min_votes"], KW["K"], rs, max_hits)
    else:
        req, tpos, votes, seeds, _ = cm.seed_chain(rows, rl, index, ref_len, k, 1, w, KW["max_occ"], band, KW["flank"], KW["min_votes"], KW["K"], rs)
    K = KW["K"]
    return [[(int(tpos[r * K + i] & np.uint64((1 << 63) - 1)), int(tpos[r * K + i] >> np.uint64(63)), int(req["text_len"][r * K + i]), int(votes[r * K + i]))
             for i in range(int(seeds["n_cands"][r]))] for r in range(len(batch))]


def main():
    import minimizer_model as mm
    import seed_model as m
    from aim_amd import engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1000)
    ap.add_argument("--k", type=int, default=11)
    ap.add_argument("--w", type=int, default=10)
    ap.add_argument("--bands", default="8,32,256")
    ap.add_argument("--cases", default=DEFAULT_CASES, help="L:e or L:e:D, comma-separated")
    ap.add_argument("--log2", type=int, default=20)
    ap.add_argument("--max-hits", type=int, default=0, help="H: the rows of aim_seed_chain_long_device's rule, chaining only")
    ap.add_argument("--out")
    a = ap.parse_args()
    k, w = a.k, a.w
    rng = np.random.default_rng(17)
    ref = make_reference(rng, a.log2)
    index = engine.index_build_minimizers(ref, k, w, threads=8)
    rows = []
    for case in a.cases.split(","):
        L, e, D = (tuple(int(x) for x in case.split(":")) + (0,))[:3]
        rs = min((L + L // 8 + 64 + D + 7) // 8 * 8, 65528 if a.max_hits else 4096)      # the row, and the cap on a window: room for the span and both flanks
        reads = []
        for r in range(a.reads):
            p = int(rng.integers(0, len(ref) - L - D - 10))
            h = L // 2
            base = np.concatenate([ref[p:p + h], ref[p + h + D:p + L + D]]) if D else ref[p:p + L]
            read = m.edit(rng, base, -(-L * e // 100))[:rs]
            reads.append((p, L + D, r & 1, m.revcomp(read) if r & 1 else read))
        for band in [int(x) for x in a.bands.split(",")]:
            for method in ("chaining",) if a.max_hits else ("voting", "chaining"):
                if method == "voting":
                    cands = [mm.seed_read(read, *index, len(ref), k=k, w=w, band=band, read_size=rs, **KW)[0] for _, _, _, read in reads]
                else:
                    cands = chain_candidates([read for _, _, _, read in reads], index, len(ref), k, w, band, rs, a.max_hits)
                got = [judge(c, p, span, strand) for c, (p, span, strand, _) in zip(cands, reads)]
                rows.append(dict(part="sensitivity", method=method, k=k, w=w, band=band, length=L, error_percent=e, deletion=D, reads=a.reads,
                                 ref_len=len(ref), **KW, **({"max_hits": a.max_hits} if a.max_hits else {}), any_of_k_covers=round(sum(g[0] for g in got) / a.reads, 4),
                                 rank0_tight=round(sum(g[1] for g in got) / a.reads, 4)))
                print(json.dumps(rows[-1]), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
