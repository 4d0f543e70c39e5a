#!/usr/bin/env python3
"""Chaining against voting on the MI355X: seed_chain_kernel / seed_chain_minimizer_kernel (aim_seed_chain_device) next to the voting
kernel of the same seed source (aim_seed_device), on the same reads, index and parameters.

  python tools/chain_rate.py [--lengths 100,1000] [--k 11,13] [--w 10] [--reads N] [--steps 7] [--rounds 5] [--out FILE.jsonl]

Per (length, k) two seed sources: the full index at stride 1 and the (w, k) minimizer index. Reads are windows of a 16 MiB random
reference with 1 % substitutions, every second one reverse-complemented, in rows of the next multiple of 128; max_occ 16, flank 8,
min_votes 2, K = 4, band 8 at l = 100 and 32 beyond. The two kernels alternate for `rounds` rounds; a round times `steps` calls with
HIP events and keeps their median, and the row reports the median over the rounds with its range, the time per read, reads/s, hits
per read, and the bytes the algorithm needs -- read rows, two bucket words per seed and strand, 4 B per hit, the slots -- against the
8 TB/s HBM roofline. With AIM_LIB set to a build with -DAIM_SEED_CHAIN_AB_NO_DP (python -m aim_amd.build --variant nodp --flags ...)
the chaining rows are those of the kernel without its DP loop: what is left is hits, sort and rank. One JSON line per row."""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

K = 4
KW = dict(max_occ=16, flank=8, min_votes=2, max_cands=K)


def make_reads(ref, n, L, rs, seed=11):
    """n reads of L bases in rows of rs: a window of the reference with L // 100 substitutions; every second one reverse-complemented."""
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, len(ref) - L, size=n)
    rows = np.zeros((n, rs), dtype=np.uint8)
    for lo in range(0, n, 1 << 14):
        p = pos[lo:lo + (1 << 14)]
        rows[lo:lo + len(p), :L] = ref[p[:, None] + np.arange(L)[None, :]]
    for _ in range(max(L // 100, 1)):
        rows[np.arange(n), rng.integers(0, L, size=n)] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)]
    comp = np.arange(256, dtype=np.uint8)
    for a, b in (b"AT", b"TA", b"CG", b"GC"):
        comp[a] = b
    rows[1::2, :L] = comp[rows[1::2, :L][:, ::-1]]
    return rows, np.full(n, L, dtype=np.int32), pos


def main():
    import torch
    torch.cuda.init()   # (before the library: the device buffers are torch's)
    import seed_rate
    from aim_amd import capi, engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--lengths", default="100,1000")
    ap.add_argument("--k", default="11,13")
    ap.add_argument("--w", type=int, default=10)
    ap.add_argument("--reads", type=int, default=0, help="default: 2^18 at l = 100, 2^15 beyond")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    ref = seed_rate.reference()
    vote_names = {None: capi.load().aim_seed_kernel_name().decode(), a.w: capi.load().aim_minimizer_kernel_names().decode().split(",")[1]}
    chain_names = dict(zip((None, a.w), capi.load().aim_seed_chain_kernel_names().decode().split(",")))
    out = []
    for k in [int(x) for x in a.k.split(",")]:
        index = {None: engine.build_index(ref, k, threads=16), a.w: engine.index_build_minimizers(ref, k, a.w, threads=16)}
        d_index = {w: tuple(torch.from_numpy(x.view(np.uint8)).to(dev) for x in ix) for w, ix in index.items()}
        for L in [int(x) for x in a.lengths.split(",")]:
            rs, band = (L + 127) // 128 * 128, 8 if L <= 100 else 32
            n = a.reads or (1 << 18 if L <= 100 else 1 << 15)
            rows, rl, _ = make_reads(ref, n, L, rs)
            for w in (None, a.w):
                sp = engine.seed_params(k, rs, band=band, w=w, **KW)
                o = [engine.seed_candidates(sp, d_index[w], len(ref), rl, rows), engine.seed_chain_candidates(sp, d_index[w], len(ref), rl, rows)]
                ptr = lambda d, *names: [d[x].data_ptr() for x in names]
                common = lambda d: ptr(d, "d_read_len", "d_reads", "d_bucket", "d_pos") + [len(ref)] + ptr(d, "d_req", "d_text_pos", "d_votes", "d_seed")
                calls = [lambda: engine.seed_device(sp, n, *common(o[0]), stream),
                         lambda: engine.seed_chain_device(sp, n, *common(o[1]), o[1]["d_chains"].data_ptr(), stream)]
                med = [[], []]
                for r in range(a.rounds):
                    for i in (0, 1):
                        med[i].append(seed_rate.events_ms(torch, calls[i], a.steps, a.warmup if r == 0 else 0)[0])
                assert np.array_equal(o[0]["seed"]["n_hits"], o[1]["seed"]["n_hits"])          # the same hits in both
                hits = int(o[0]["seed"]["n_hits"].astype(np.int64).sum())
                seeds = (L - k + 1) if w is None else round(2 * (L - k + 1) / (w + 1))
                for i, method in enumerate(("voting", "chaining")):
                    ms = statistics.median(med[i])
                    need = n * rs + n * 4 + 2 * n * seeds * 8 + hits * 4 + n * K * (28 + 16 * i) + n * 16
                    out.append(dict(part="chain_rate", method=method, kernel=(vote_names, chain_names)[i][w], lib=os.path.basename(capi.LIB_PATH), reads=n,
                                    length=L, read_size=rs, k=k, w=w, band=band, **KW, ref_len=len(ref), ms=round(ms, 4), ms_min=round(min(med[i]), 4),
                                    ms_max=round(max(med[i]), 4), rounds=a.rounds, steps=a.steps, us_per_read=round(ms * 1e3 / n, 4),
                                    reads_per_s=round(n / ms * 1e3), hits_per_read=round(hits / n, 1),
                                    truncated_share=round(float((o[i]["seed"]["flags"] & capi.SEED_TRUNCATED != 0).mean()), 4),
                                    found=round(float((o[i]["seed"]["n_cands"] > 0).mean()), 4), algorithmic_bytes=need,
                                    share_of_8tb_per_s=round(need / ms / 1e6 / 8000, 5),
                                    ratio_to_voting=round(ms / statistics.median(med[0]), 2)))
                    print(json.dumps(out[-1]), flush=True)
                del o
                torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
