#!/usr/bin/env python3
"""Device-side seeding (aim_seed_device): what the kernel costs, next to the verification pass it feeds, and what it saves end to end.

  python tools/seed_rate.py --mode kernel [--reads N] [--configs 11:1,11:4,13:1,13:4] [--steps K] [--warmup W] [--out FILE.jsonl]
  python tools/seed_rate.py --mode e2e [--reads N] [--host-reads M] [--rounds R] [--out FILE.jsonl]
  python tools/seed_rate.py --mode kernel --w 5,10,19 [--k 11,13] [--length 100|1000] [--reads N] [--rounds 5] [--out FILE.jsonl]

kernel  N reads (default 1 Mi) of l = 100 with one substitution each (e = 1 %), both strands, against a 16 MiB random reference:
        seed_candidates_kernel per (k, stride) at max_occ 16, band 8, flank 8, min_votes 2, K = 4, timed with HIP events (median of
        `steps` calls), reads/s, and the bytes the algorithm needs -- read rows, two bucket words per seed and strand, 4 B per hit,
        the slots -- against the 8 TB/s HBM roofline (the bucket and pos reads are random 4-B words: the memory system moves whole
        sectors for them, so the algorithmic figure is a lower bound on the traffic). Next to it the score-only pass of the
        verification that follows (aim_align_device_groups on the kernel's own output, REF_TEXTS | READ_GROUPS | ENDSFREE).
e2e     reads in, aim_best_t out, two ways, alternating for `rounds` rounds in one process:
        `device`  upload the read rows into buffers allocated once, aim_seed_device, aim_align_device_groups on its device buffers,
                  download aim_best_t;
        `host`    what a caller did before: seed on the host (tests/seed_model.py, the rule in numpy / Python), then send the
                  candidates through aim_align_device_groups. The host seeder is timed on --host-reads reads (default 2 048: it is
                  pure Python and takes about a millisecond per read) and its share of that path's time is reported.
--w     (w, k) minimizers against strides: per (k, w) seed_minimizer_kernel over the minimizer index and seed_candidates_kernel over
        the full index at stride = ceil((w + 1) / 2), which looks up the same expected number of seeds, on the same reads of --length
        bases (rows of the next multiple of 128), alternating for `rounds` rounds of `steps` calls: time per read, hits per strand and
        the share of reads truncated, found (n_cands > 0) and whose true position lies in one of the K windows.
One JSON line per row (stdout, and --out)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L, RS, K = 100, 128, 4
REF_LEN = 1 << 24
SEED_KW = dict(max_occ=16, band=8, flank=8, min_votes=2, max_cands=K)


def reference(n=REF_LEN, seed=3):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, size=n)].copy()


def make_reads(ref, n, seed=11):
    """n reads of L bases in rows of RS: a window of the reference with one substitution; every second one reverse-complemented."""
    rng = np.random.default_rng(seed)
    pos = rng.integers(0, len(ref) - L, size=n)
    rows = np.zeros((n, RS), dtype=np.uint8)
    for lo in range(0, n, 1 << 16):
        p = pos[lo:lo + (1 << 16)]
        rows[lo:lo + len(p), :L] = ref[p[:, None] + np.arange(L)[None, :]]
    at = rng.integers(0, L, size=n)
    rows[np.arange(n), at] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=n)]
    comp = np.arange(256, dtype=np.uint8)
    for a, b in (b"AT", b"TA", b"CG", b"GC"):
        comp[a] = b
    rows[1::2, :L] = comp[rows[1::2, :L][:, ::-1]]
    return rows, np.full(n, L, dtype=np.int32), pos


def events_ms(torch, call, steps, warmup):
    for _ in range(warmup):
        call()
    times = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        call()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times), min(times), max(times)


def verify_setup(torch, engine, capi, n, ref, dev):
    params = engine.make_params("wfa", 20, RS, read_groups=True, ref_texts=True, ends_free=(0, 0, 2 * SEED_KW["flank"], 2 * SEED_KW["flank"]))
    offs = engine.seed_groups_offsets(n, K)
    d = dict(params=params, d_off=torch.from_numpy(offs.view(np.uint8).copy()).to(dev), d_ref=torch.zeros(len(ref) + 64, dtype=torch.uint8, device=dev),
             d_res=torch.zeros(n * 24, dtype=torch.uint8, device=dev), d_best=torch.zeros(n * 16, dtype=torch.uint8, device=dev))
    d["d_ref"][:len(ref)] = torch.from_numpy(ref).to(dev)
    d["sb"] = capi.load().aim_scratch_bytes(capi.params_ref(params), n * K)
    d["d_scr"] = torch.zeros(d["sb"], dtype=torch.uint8, device=dev)
    return d


def verify_call(engine, v, n, d_req, d_reads, d_tp, ref_len, stream):
    engine.align_device_groups(v["params"], n * K, n, d_req.data_ptr(), d_reads.data_ptr(), None, d_tp.data_ptr(), v["d_ref"].data_ptr(), ref_len,
                               v["d_off"].data_ptr(), v["d_res"].data_ptr(), None, v["d_best"].data_ptr(), v["d_scr"].data_ptr(), v["sb"], stream)


def kernel_rows(n, configs, steps, warmup):
    import torch
    torch.cuda.init()   # (before the library: the device buffers are torch's)
    from aim_amd import capi, engine
    dev = torch.device("cuda:0")
    ref = reference()
    rows, rl, _ = make_reads(ref, n)
    stream = torch.cuda.current_stream().cuda_stream
    v = verify_setup(torch, engine, capi, n, ref, dev)
    out, index = [], {}
    for k, stride in configs:
        if k not in index:
            bucket, pos = engine.build_index(ref, k, threads=16)
            index[k] = (torch.from_numpy(bucket.view(np.uint8)).to(dev), torch.from_numpy(pos.view(np.uint8)).to(dev))
        sp = engine.seed_params(k, RS, stride=stride, **SEED_KW)
        o = engine.seed_candidates(sp, index[k], len(ref), rl, rows)

        def seed_call():
            engine.seed_device(sp, n, o["d_read_len"].data_ptr(), o["d_reads"].data_ptr(), o["d_bucket"].data_ptr(), o["d_pos"].data_ptr(), len(ref),
                               o["d_req"].data_ptr(), o["d_text_pos"].data_ptr(), o["d_votes"].data_ptr(), o["d_seed"].data_ptr(), stream)
        med, lo, hi = events_ms(torch, seed_call, steps, warmup)
        vmed, vlo, vhi = events_ms(torch, lambda: verify_call(engine, v, n, o["d_req"], o["d_reads"], o["d_text_pos"], len(ref), stream), steps, warmup)
        best = v["d_best"].cpu().numpy().view(capi.BEST_DTYPE)
        seeds = (L - k) // stride + 1
        hits = int(o["seed"]["n_hits"].astype(np.int64).sum())
        need = n * RS + n * 4 + 2 * n * seeds * 8 + hits * 4 + n * K * 28 + n * 16
        out.append(dict(part="kernel", kernel=capi.load().aim_seed_kernel_name().decode(), reads=n, k=k, stride=stride, **SEED_KW, ref_len=len(ref),
                        seed_ms=round(med, 4), seed_ms_min=round(lo, 4), seed_ms_max=round(hi, 4), reads_per_s=round(n / med * 1e3),
                        hits_per_read=round(hits / n, 2), algorithmic_bytes=need, algorithmic_gb_per_s=round(need / med / 1e6, 1),
                        share_of_8tb_per_s=round(need / med / 1e6 / 8000, 4), found=round(float((o["seed"]["n_cands"] > 0).mean()), 4),
                        truncated=int((o["seed"]["flags"] & capi.SEED_TRUNCATED).sum()), verify_ms=round(vmed, 4), verify_ms_min=round(vlo, 4),
                        verify_ms_max=round(vhi, 4), verify_candidates_per_s=round(n * K / vmed * 1e3),
                        mapped_score_le_2=round(float((best["best_score"] <= 2).mean()), 4)))
        print(json.dumps(out[-1]), flush=True)
    return out


def minimizer_rows(n, ks, ws, steps, warmup, rounds):
    import torch
    torch.cuda.init()   # (before the library: the device buffers are torch's)
    from aim_amd import capi, engine
    dev = torch.device("cuda:0")
    ref = reference()
    rows, rl, true_pos = make_reads(ref, n)
    stream = torch.cuda.current_stream().cuda_stream
    names = [capi.load().aim_minimizer_kernel_names().decode().split(",")[1], capi.load().aim_seed_kernel_name().decode()]
    out = []
    for k in ks:
        full = engine.build_index(ref, k, threads=16)
        for w in ws:
            stride = (w + 2) // 2
            index = [engine.index_build_minimizers(ref, k, w, threads=16), full]
            sps = [engine.seed_params(k, RS, w=w, **SEED_KW), engine.seed_params(k, RS, stride=stride, **SEED_KW)]
            o = [engine.seed_candidates(sp, tuple(torch.from_numpy(a.view(np.uint8)).to(dev) for a in ix), len(ref), rl, rows) for sp, ix in zip(sps, index)]

            def call(i):
                engine.seed_device(sps[i], n, o[i]["d_read_len"].data_ptr(), o[i]["d_reads"].data_ptr(), o[i]["d_bucket"].data_ptr(), o[i]["d_pos"].data_ptr(),
                                   len(ref), o[i]["d_req"].data_ptr(), o[i]["d_text_pos"].data_ptr(), o[i]["d_votes"].data_ptr(), o[i]["d_seed"].data_ptr(), stream)
            med = [[], []]
            for r in range(rounds):
                for i in (0, 1):
                    med[i].append(events_ms(torch, lambda: call(i), steps, warmup if r == 0 else 0)[0])
            for i in (0, 1):
                start = (o[i]["text_pos"] & np.uint64((1 << 63) - 1)).astype(np.int64).reshape(n, K)
                tlen = o[i]["req"]["text_len"].astype(np.int64).reshape(n, K)
                hit = ((start <= true_pos[:, None]) & (true_pos[:, None] + L <= start + tlen) & (tlen > 0)).any(axis=1)
                ms = statistics.median(med[i])
                out.append(dict(part="minimizers", kernel=names[i], reads=n, length=L, read_size=RS, k=k, w=w, stride=1 if i == 0 else stride, **SEED_KW,
                                ref_len=len(ref), index_positions=len(index[i][1]), seed_ms=round(ms, 4), seed_ms_min=round(min(med[i]), 4),
                                seed_ms_max=round(max(med[i]), 4), rounds=rounds, ns_per_read=round(ms * 1e6 / n, 2),
                                hits_per_strand=round(float(o[i]["seed"]["n_hits"].mean()), 2),
                                truncated_share=round(float((o[i]["seed"]["flags"] & capi.SEED_TRUNCATED != 0).mean()), 5),
                                found=round(float((o[i]["seed"]["n_cands"] > 0).mean()), 4), true_position_in_k_windows=round(float(hit.mean()), 4)))
                print(json.dumps(out[-1]), flush=True)
            del o
            torch.cuda.empty_cache()
    return out


def e2e_rows(n, host_n, rounds):
    import torch
    torch.cuda.init()
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import seed_model
    from aim_amd import capi, engine
    dev = torch.device("cuda:0")
    ref = reference()
    k, stride = 11, 1
    rows, rl, _ = make_reads(ref, n)
    bucket, pos = engine.build_index(ref, k, threads=16)
    d_index = (torch.from_numpy(bucket.view(np.uint8)).to(dev), torch.from_numpy(pos.view(np.uint8)).to(dev))
    sp = engine.seed_params(k, RS, stride=stride, **SEED_KW)
    stream = torch.cuda.current_stream().cuda_stream
    host_n = min(host_n, n)
    warm = min(host_n, 64)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
    v = {}
    for m in sorted({n, host_n, warm}):     # per batch size: the verification buffers and the device path's own, allocated once
        v[m] = verify_setup(torch, engine, capi, m, ref, dev)
        v[m].update(d_rl=torch.zeros(m * 4, dtype=torch.uint8, device=dev), d_rows=torch.zeros(m * RS + 64, dtype=torch.uint8, device=dev),
                    d_req=torch.zeros(m * K * 16, dtype=torch.uint8, device=dev), d_tp=torch.zeros(m * K * 8, dtype=torch.uint8, device=dev),
                    d_votes=torch.zeros(m * K * 4, dtype=torch.uint8, device=dev), d_seed=torch.zeros(m * 16, dtype=torch.uint8, device=dev))

    def device_way(m):
        w = v[m]
        t0 = time.perf_counter()
        w["d_rows"][:m * RS].copy_(torch.from_numpy(rows[:m].reshape(-1)))
        w["d_rl"].copy_(torch.from_numpy(rl[:m].view(np.uint8)))
        engine.seed_device(sp, m, w["d_rl"].data_ptr(), w["d_rows"].data_ptr(), d_index[0].data_ptr(), d_index[1].data_ptr(), len(ref),
                           w["d_req"].data_ptr(), w["d_tp"].data_ptr(), w["d_votes"].data_ptr(), w["d_seed"].data_ptr(), stream)
        verify_call(engine, w, m, w["d_req"], w["d_rows"], w["d_tp"], len(ref), stream)     # no candidate array visits the host
        best = w["d_best"].cpu().numpy().view(capi.BEST_DTYPE)
        return time.perf_counter() - t0, 0.0, best

    def host_way(m):
        t0 = time.perf_counter()
        req, tpos, _, _ = seed_model.seed(rows[:m], rl[:m], (bucket, pos), len(ref), k, stride, SEED_KW["max_occ"], SEED_KW["band"], SEED_KW["flank"],
                                          SEED_KW["min_votes"], K, RS)
        t1 = time.perf_counter()
        d_req, d_tp, d_rows = up(req), up(tpos), torch.zeros(m * RS + 64, dtype=torch.uint8, device=dev)
        d_rows[:m * RS] = up(rows[:m])
        verify_call(engine, v[m], m, d_req, d_rows, d_tp, len(ref), stream)
        best = v[m]["d_best"].cpu().numpy().view(capi.BEST_DTYPE)
        return time.perf_counter() - t0, t1 - t0, best

    out = []
    device_way(warm), host_way(warm)         # warm-up: code objects, allocator
    for r in range(rounds):
        for name, fn, m in (("device", device_way, n), ("host", host_way, host_n), ("device_small", device_way, host_n)):
            dt, seeder, best = fn(m)
            out.append(dict(part="e2e", variant=name, round=r, reads=m, k=k, stride=stride, seconds=round(dt, 4), reads_per_s=round(m / dt),
                            host_seeder_seconds=round(seeder, 4), host_seeder_share=round(seeder / dt, 4),
                            mapped_score_le_2=round(float((best["best_score"] <= 2).mean()), 4)))
            print(json.dumps(out[-1]), flush=True)
    return out


def main():
    global L, RS
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["kernel", "e2e"], default="kernel")
    ap.add_argument("--reads", type=int, default=1 << 20)
    ap.add_argument("--host-reads", type=int, default=2048)
    ap.add_argument("--configs", default="11:1,11:4,13:1,13:4")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--w", default="", help="minimizer windows, e.g. 5,10,19 (kernel mode): seed_minimizer_kernel against the stride that looks up as many seeds")
    ap.add_argument("--k", default="11,13", help="with --w: the k values")
    ap.add_argument("--length", type=int, default=L, help="with --w: read length (rows of the next multiple of 128)")
    ap.add_argument("--out")
    a = ap.parse_args()
    if a.mode == "kernel" and a.w:
        L, RS = a.length, (a.length + 127) // 128 * 128
        rows = minimizer_rows(a.reads, [int(x) for x in a.k.split(",")], [int(x) for x in a.w.split(",")], a.steps, a.warmup, max(a.rounds, 5))
    elif a.mode == "kernel":
        rows = kernel_rows(a.reads, [tuple(int(x) for x in c.split(":")) for c in a.configs.split(",")], a.steps, a.warmup)
    else:
        rows = e2e_rows(a.reads, a.host_reads, a.rounds)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
