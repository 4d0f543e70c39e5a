#!/usr/bin/env python3
"""What classification and MAPQ cost on the MI355X: chain_class_kernel and read_mapq_kernel (aim_chain_classify_device,
aim_read_mapq_device) on synthetic chain-kernel outputs, next to the chaining they follow.

  python tools/chain_class_rate.py [--reads 1048576] [--ks 4,16] [--lanes 0,8,16] [--steps 7] [--inner 20] [--out FILE.jsonl]

Per K: the arrays of tests/chain_class_model.py's synthetic() and synthetic_best(), built for 4 096 reads and tiled to --reads (every
read is independent; a selection is shifted with its tile). A call takes tens of microseconds, so a timed window is `inner` calls back
to back between two HIP events; a row is the median of `steps` windows, per call, with its range,
the bytes the algorithm needs -- 24 B in and 8 B out per slot plus 20 B per read for the classification; 16 B of aim_best_t, two
8-byte class rows and 8 B out per read for the MAPQ, 16 B more per read with mates -- and their share of the 8 TB/s HBM roofline.
--lanes lists AIM_CLASS_G values: 0 is the default group width (4, 8 or 16 lanes by K); 8 and 16 widen it where K would take fewer.
The last row is seed_chain_minimizer_kernel on --reads reads of l = 100 (k 11, w 10, tools/chain_rate.py's reads and parameters),
measured in the same process: the step classification follows. One JSON line per row."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

TILE = 4096


def tiled(arr, times):
    return np.ascontiguousarray(np.concatenate([arr] * times))


def main():
    import torch
    torch.cuda.init()   # (before the library: the device buffers are torch's)
    import chain_class_model as ccm
    import chain_rate
    import seed_rate
    from aim_amd import capi, engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=1 << 20)
    ap.add_argument("--ks", default="4,16")
    ap.add_argument("--lanes", default="0,8,16")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20, help="calls of a new kernel per timed window (one call takes tens of microseconds)")
    ap.add_argument("--out")
    a = ap.parse_args()
    assert a.reads % TILE == 0
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1).copy()).to(dev)
    names = capi.load().aim_chain_class_kernel_names().decode().split(",")
    n, times = a.reads, a.reads // TILE
    out = []

    def row(**kw):
        out.append(dict(part="chain_class_rate", lib=os.path.basename(capi.LIB_PATH), reads=n, steps=a.steps, inner=a.inner, **kw))
        print(json.dumps(out[-1]), flush=True)

    def events_ms(call, inner):
        """Median, least and greatest time of one call over `steps` windows of `inner` back-to-back calls between two HIP events."""
        def window():
            for _ in range(inner):
                call()
        return tuple(x / inner for x in seed_rate.events_ms(torch, window, a.steps, a.warmup))

    def timed(call, need):
        ms, lo, hi = events_ms(call, a.inner)
        return dict(ms=round(ms, 4), ms_min=round(lo, 4), ms_max=round(hi, 4), ns_per_read=round(ms * 1e6 / n, 4), algorithmic_bytes=need,
                    share_of_8tb_per_s=round(need / ms / 1e6 / 8000, 4))
    for K in [int(x) for x in a.ks.split(",")]:
        d = ccm.synthetic(1, TILE, K)
        want = ccm.classify(K, ccm.SYN_READ_SIZE, capi.CHAIN_MASK_DEFAULT, **d)
        t = {k: up(tiled(v, times)) for k, v in d.items()}
        d_cls = torch.zeros(n * K * 8, dtype=torch.uint8, device=dev)
        for lanes in [int(x) for x in a.lanes.split(",")]:
            default = 4 if K <= 4 else 8 if K <= 8 else 16
            if lanes and lanes <= default:
                continue
            os.environ.pop("AIM_CLASS_G", None)
            if lanes:
                os.environ["AIM_CLASS_G"] = str(lanes)
            d_cls.fill_(0xEE)
            call = lambda: engine.chain_classify_device(K, ccm.SYN_READ_SIZE, capi.CHAIN_MASK_DEFAULT, n, t["read_len"].data_ptr(), t["text_pos"].data_ptr(),
                                                        t["seed"].data_ptr(), t["chains"].data_ptr(), d_cls.data_ptr(), stream)
            r = timed(call, n * K * 32 + n * 20)
            got = d_cls.cpu().numpy().view(capi.CHAIN_CLASS_DTYPE)
            assert got[:TILE * K].tobytes() == want.tobytes() and got[-TILE * K:].tobytes() == want.tobytes()       # the rows are the model's
            row(kernel=names[0], K=K, lanes=lanes or default, default_lanes=lanes == 0, mask_q8=capi.CHAIN_MASK_DEFAULT, **r)
        os.environ.pop("AIM_CLASS_G", None)
        best, mates = ccm.synthetic_best(3, TILE, K)

        def shifted(sel):                       # a tile's selections point into that tile's slots
            sel = np.concatenate([np.where(sel == ccm.NONE, np.uint64(ccm.NONE), sel.astype(np.uint64) + np.uint64(i * TILE * K)) for i in range(times)])
            return sel.astype(np.uint32)
        big_best = tiled(best, times)
        big_best["best_pair"] = shifted(best["best_pair"])
        big_mates = tiled(mates, times)
        big_mates["best_pair"] = shifted(mates["best_pair"].reshape(-1)).reshape(-1, 2)
        d_best, d_mates, d_mapq = up(big_best), up(big_mates), torch.zeros(n * 8, dtype=torch.uint8, device=dev)
        for with_mates in (False, True):
            d_mapq.fill_(0xEE)
            call = lambda: engine.read_mapq_device(K, n, 3, d_best.data_ptr(), d_mates.data_ptr() if with_mates else None, d_cls.data_ptr(),
                                                   d_mapq.data_ptr(), stream)
            r = timed(call, n * (16 + 16 + 8) + (n * 16 if with_mates else 0))
            got = d_mapq.cpu().numpy().view(capi.READ_MAPQ_DTYPE)
            want_mapq = ccm.read_mapq(K, 3, best, mates if with_mates else None, want)
            assert (got[:TILE][["mapq", "chain_mapq", "aln_mapq", "flags"]].tobytes() == want_mapq[["mapq", "chain_mapq", "aln_mapq", "flags"]].tobytes())
            row(kernel=names[1], K=K, mates=with_mates, score_unit=3, **r)
        del t, d_cls, d_best, d_mates, d_mapq
        torch.cuda.empty_cache()
    # the chaining the classification follows: tools/chain_rate.py's minimizer row at l = 100
    k, w, L, rs = 11, 10, 100, 128
    ref = seed_rate.reference()
    rows, rl, _ = chain_rate.make_reads(ref, n, L, rs)
    sp = engine.seed_params(k, rs, band=8, w=w, **chain_rate.KW)
    index = tuple(torch.from_numpy(x.view(np.uint8)).to(dev) for x in engine.index_build_minimizers(ref, k, w, threads=16))
    o = engine.seed_chain_candidates(sp, index, len(ref), rl, rows)
    ptr = lambda *names: [o[x].data_ptr() for x in names]
    call = lambda: engine.seed_chain_device(sp, n, *ptr("d_read_len", "d_reads", "d_bucket", "d_pos"), len(ref),
                                            *ptr("d_req", "d_text_pos", "d_votes", "d_seed", "d_chains"), stream)
    ms, lo, hi = events_ms(call, 1)
    row(kernel=capi.load().aim_seed_chain_kernel_names().decode().split(",")[1], K=chain_rate.K, length=L, read_size=rs, k=k, w=w, ms=round(ms, 4),
        ms_min=round(lo, 4), ms_max=round(hi, 4), ns_per_read=round(ms * 1e6 / n, 4))
    # ... and the classification of exactly these chains
    engine.chain_classify(sp, o)
    call = lambda: engine.chain_classify_device(chain_rate.K, rs, capi.CHAIN_MASK_DEFAULT, n, *ptr("d_read_len", "d_text_pos", "d_seed", "d_chains", "d_class"), stream)
    r = timed(call, n * chain_rate.K * 32 + n * 20)
    fl = o["class"]["flags"]
    row(kernel=names[0], K=chain_rate.K, lanes=4, default_lanes=True, mask_q8=capi.CHAIN_MASK_DEFAULT, on="the chains of the row above",
        share_of_chaining=round(r["ms"] / ms, 4), primaries=int((fl & capi.CHAIN_PRIMARY != 0).sum()), secondaries=int((fl & capi.CHAIN_SECONDARY != 0).sum()), **r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
