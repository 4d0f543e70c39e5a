#!/usr/bin/env python3
"""seed_chain_long_kernel (aim_seed_chain_long_device) on the MI355X: what the tiled hit phase and the wider keys cost next to
seed_chain_minimizer_kernel on an input both take, and what chaining a long read costs next to verifying its candidates.

  python tools/chain_long_rate.py --part overhead [--k 11,13] [--w 10] [--reads N] [--steps 7] [--rounds 5] [--out FILE.jsonl]
  python tools/chain_long_rate.py --part long [--lengths 5000,10000,20000,60000] [--errors 1,5] [--w 10,19] [--hits 2048,4096,8192]
                                  [--reads N] [--steps 7] [--rounds 5] [--no-verify] [--out FILE.jsonl]

overhead  tools/chain_rate.py's minimizer row: reads of l = 1 000 with 1 % substitutions in rows of 1 024 over the (w, k) minimizer index
          of a 16 MiB random reference, max_occ 16, band 32, flank 8, min_votes 2, K = 4. seed_chain_minimizer_kernel and
          seed_chain_long_kernel at H = 1 024 alternate for `rounds` rounds; a round times `steps` calls with HIP events and keeps their
          median. The output bytes of the two are compared before anything is timed. With AIM_LIB set to a build with
          -DAIM_SEED_CHAIN_AB_NO_DP (python -m aim_amd.build --variant nodp --flags ...) both kernels run without their DP loop.
long      reads of l bases with e % edits (a third each substitutions, deletions and insertions), every second one reverse-complemented,
          k = 11, max_occ 16, band 256, flank 0, min_votes 2, K = 4: per (l, e, w, H) the time per read, the anchors per read and
          strand, the share of truncated reads and the workgroups per CU that H leaves; per (l, e, w) the score-only verification of
          the K candidates the kernel produced at the largest H (aim_align_device_groups, REF_TEXTS | READ_GROUPS, WFA-adaptive at the
          launchers' MAX_SCORE for (l, e), AIM_FLAG_WFA_W32 from read_size 32 760 on), and which of the two takes longer.
One JSON line per row (stdout, and --out)."""
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
COMP = np.arange(256, dtype=np.uint8)
for _a, _b in (b"AT", b"TA", b"CG", b"GC"):
    COMP[_a] = _b


def lds_and_per_cu(H):
    """seed_chain_long_lds_bytes and lds_workgroups_per_cu (csrc/seed_chain_long.hpp, csrc/aim_device.hpp)."""
    lds = 14 * H + 2912
    return lds, (160 * 1024) // (-(-lds // 1280) * 1280)


def make_long_reads(ref, n, L, e_percent, rs, seed=11):
    """n reads in rows of rs: a window of L reference bases with L * e / 100 edits, a third each substitutions, deletions and insertions
    at uniform positions; every second one reverse-complemented."""
    rng = np.random.default_rng(seed)
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    rows, rl = np.zeros((n, rs), dtype=np.uint8), np.zeros(n, dtype=np.int32)
    third = L * e_percent // 300
    for r in range(n):
        p = int(rng.integers(0, len(ref) - L))
        read = ref[p:p + L].copy()
        read[rng.integers(0, L, size=third)] = acgt[rng.integers(0, 4, size=third)]
        read = np.delete(read, rng.integers(0, len(read), size=third))
        read = np.insert(read, rng.integers(0, len(read), size=third), acgt[rng.integers(0, 4, size=third)])[:rs]
        if r & 1:
            read = COMP[read[::-1]]
        rows[r, :len(read)], rl[r] = read, len(read)
    return rows, rl


def timed(torch, seed_rate, calls, steps, warmup, rounds):
    """calls alternate for `rounds` rounds; per call the list of the rounds' medians (ms)."""
    med = [[] for _ in calls]
    for r in range(rounds):
        for i, call in enumerate(calls):
            med[i].append(seed_rate.events_ms(torch, call, steps, warmup if r == 0 else 0)[0])
    return med


OUT = {"path": None}


def emit(row):
    """One JSON line to stdout and, as it is produced, to --out."""
    print(json.dumps(row), flush=True)
    if OUT["path"]:
        with open(OUT["path"], "a") as f:
            f.write(json.dumps(row) + "\n")
    return row


def summary(ms):
    return dict(ms=round(statistics.median(ms), 4), ms_min=round(min(ms), 4), ms_max=round(max(ms), 4))


def overhead_rows(a, torch, seed_rate, capi, engine, ref, dev, stream):
    out = []
    L, rs, band = 1000, 1024, 32
    kw = dict(max_occ=16, flank=8, min_votes=2, max_cands=K)
    import chain_rate
    n = a.reads or 1 << 15
    rows, rl, _ = chain_rate.make_reads(ref, n, L, rs)
    for k in [int(x) for x in a.k.split(",")]:
        for w in [int(x) for x in a.w.split(",")][:1]:
            index = tuple(torch.from_numpy(x.view(np.uint8)).to(dev) for x in engine.index_build_minimizers(ref, k, w, threads=16))
            sp = engine.seed_params(k, rs, band=band, w=w, **kw)
            o = [engine.seed_chain_candidates(sp, index, len(ref), rl, rows), engine.seed_chain_long_candidates(sp, 1024, index, len(ref), rl, rows)]
            for name in ("req", "text_pos", "votes", "seed", "chains"):
                assert o[0][name].tobytes() == o[1][name].tobytes(), name          # the same bytes before anything is timed
            ptr = lambda d, *names: [d[x].data_ptr() for x in names]
            common = lambda d: ptr(d, "d_read_len", "d_reads", "d_bucket", "d_pos") + [len(ref)] + ptr(d, "d_req", "d_text_pos", "d_votes", "d_seed", "d_chains")
            calls = [lambda: engine.seed_chain_device(sp, n, *common(o[0]), stream), lambda: engine.seed_chain_long_device(sp, 1024, n, *common(o[1]), stream)]
            med = timed(torch, seed_rate, calls, a.steps, a.warmup, a.rounds)
            hits = int(o[0]["seed"]["n_hits"].astype(np.int64).sum())
            for i, kernel in enumerate((capi.load().aim_seed_chain_kernel_names().decode().split(",")[1], capi.load().aim_seed_chain_long_kernel_name().decode())):
                out.append(dict(part="chain_long_overhead", kernel=kernel, lib=os.path.basename(capi.LIB_PATH), reads=n, length=L, read_size=rs, k=k, w=w,
                                band=band, **kw, max_hits=1024, ref_len=len(ref), **summary(med[i]), rounds=a.rounds, steps=a.steps,
                                us_per_read=round(statistics.median(med[i]) * 1e3 / n, 4), hits_per_read=round(hits / n, 1),
                                ratio_to_seed_chain_minimizer=round(statistics.median(med[i]) / statistics.median(med[0]), 3)))
                emit(out[-1])
            del o
            torch.cuda.empty_cache()
    return out


def long_rows(a, torch, seed_rate, capi, engine, ref, dev, stream):
    out = []
    k = 11
    kw = dict(max_occ=16, flank=0, min_votes=2, max_cands=K)
    caps = [int(x) for x in a.hits.split(",")]
    d_ref = torch.zeros(len(ref) + 64, dtype=torch.uint8, device=dev)
    d_ref[:len(ref)] = torch.from_numpy(ref).to(dev)
    for w in [int(x) for x in a.w.split(",")]:
        index = tuple(torch.from_numpy(x.view(np.uint8)).to(dev) for x in engine.index_build_minimizers(ref, k, w, threads=16))
        for L in [int(x) for x in a.lengths.split(",")]:
            rs = min((L + L // 16 + 64) // 8 * 8, capi.SEED_LONG_MAX_READ_SIZE)
            n = a.reads or (2048 if L <= 20000 else 1024)
            for e in [int(x) for x in a.errors.split(",")]:
                rows, rl = make_long_reads(ref, n, L, e, rs)
                sp = engine.seed_params(k, rs, band=256, w=w, long_reads=True, **kw)
                chain_ms, o = {}, None
                for H in caps:
                    o = engine.seed_chain_long_candidates(sp, H, index, len(ref), rl, rows)
                    ptr = lambda *names: [o[x].data_ptr() for x in names]
                    args = ptr("d_read_len", "d_reads", "d_bucket", "d_pos") + [len(ref)] + ptr("d_req", "d_text_pos", "d_votes", "d_seed", "d_chains")
                    ms = timed(torch, seed_rate, [lambda: engine.seed_chain_long_device(sp, H, n, *args, stream)], a.steps, a.warmup, a.rounds)[0]
                    lds, per_cu = lds_and_per_cu(H)
                    chain_ms[H] = statistics.median(ms)
                    out.append(dict(part="chain_long", kernel="seed_chain_long_kernel", lib=os.path.basename(capi.LIB_PATH), reads=n, length=L, error_percent=e,
                                    read_size=rs, k=k, w=w, band=256, **kw, max_hits=H, lds_bytes=lds, workgroups_per_cu=per_cu, ref_len=len(ref),
                                    **summary(ms), rounds=a.rounds, steps=a.steps, us_per_read=round(chain_ms[H] * 1e3 / n, 3),
                                    reads_per_s=round(n / chain_ms[H] * 1e3), anchors_per_read_strand=round(float(o["seed"]["n_hits"].max(axis=1).mean()), 1),
                                    truncated_share=round(float((o["seed"]["flags"] & capi.SEED_TRUNCATED != 0).mean()), 4),
                                    found=round(float((o["seed"]["n_cands"] > 0).mean()), 4), mean_cands=round(float(o["seed"]["n_cands"].mean()), 2)))
                    emit(out[-1])
                if not a.no_verify:      # the K candidates of the largest H, score only
                    H = caps[-1]
                    ms_cap, _ = engine.launcher_sizes("wfa", L, e / 100.0)
                    try:
                        params = engine.make_params("wfa", ms_cap, rs, reduce=True, read_groups=True, ref_texts=True, w32=rs >= 32760)
                        sb = capi.load().aim_scratch_bytes(capi.params_ref(params), n * K)
                        if sb > a.verify_scratch_gb * (1 << 30):
                            raise capi.AimError(0, "scratch %d B is above --verify-scratch-gb" % sb)
                        offs = engine.seed_groups_offsets(n, K)
                        d_off = torch.from_numpy(offs.view(np.uint8).copy()).to(dev)
                        d_res = torch.zeros(n * capi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                        d_best = torch.zeros(n * 16, dtype=torch.uint8, device=dev)
                        d_scr = torch.zeros(max(sb, 16), dtype=torch.uint8, device=dev)
                        call = lambda: engine.align_device_groups(params, n * K, n, o["d_req"].data_ptr(), o["d_reads"].data_ptr(), None, o["d_text_pos"].data_ptr(),
                                                                  d_ref.data_ptr(), len(ref), d_off.data_ptr(), d_res.data_ptr(), None, d_best.data_ptr(),
                                                                  d_scr.data_ptr(), sb, stream)
                        vms = timed(torch, seed_rate, [call], max(a.steps // 2, 1), 1, 1)[0]
                        best = d_best.cpu().numpy().view(capi.BEST_DTYPE)
                        v = statistics.median(vms)
                        out.append(dict(part="chain_long_verify", kernel=capi.load().aim_kernel_name(capi.params_ref(params)).decode(), reads=n, length=L,
                                        error_percent=e, read_size=rs, w=w, max_hits=H, max_score=ms_cap, pairs=n * K, scratch_bytes=int(sb), **summary(vms),
                                        us_per_read=round(v * 1e3 / n, 3), aligned_share=round(float((best["best_score"] >= 0).mean()), 4),
                                        chain_us_per_read=round(chain_ms[H] * 1e3 / n, 3), longer="verification" if v > chain_ms[H] else "chaining",
                                        verify_over_chain=round(v / chain_ms[H], 2)))
                        del d_scr
                    except capi.AimError as err:
                        out.append(dict(part="chain_long_verify", reads=n, length=L, error_percent=e, read_size=rs, w=w, max_hits=H, max_score=ms_cap,
                                        refused=str(err)))
                    emit(out[-1])
                del o
                torch.cuda.empty_cache()
    return out


def main():
    import torch
    torch.cuda.init()   # (before the library: the device buffers are torch's)
    import seed_rate
    from aim_amd import capi, engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("overhead", "long"), required=True)
    ap.add_argument("--lengths", default="5000,10000,20000,60000")
    ap.add_argument("--errors", default="1,5")
    ap.add_argument("--k", default="11,13")
    ap.add_argument("--w", default="10,19")
    ap.add_argument("--hits", default="2048,4096,8192")
    ap.add_argument("--reads", type=int, default=0, help="default: 2^15 for overhead; 2 048 up to l = 20 000 and 1 024 beyond for long")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--verify-scratch-gb", type=float, default=64.0)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    ref = seed_rate.reference()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        OUT["path"] = a.out
    (overhead_rows if a.part == "overhead" else long_rows)(a, torch, seed_rate, capi, engine, ref, dev, stream)


if __name__ == "__main__":
    main()
