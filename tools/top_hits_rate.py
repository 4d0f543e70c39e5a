#!/usr/bin/env python3
"""The N best candidates per read (AIM_FLAG_TOP_HITS): what the ranking costs and what the flag saves end to end.

  python tools/top_hits_rate.py --mode select [--hits 1,2,4,8] [--steps K] [--warmup W]
  [AIM_LIB=<another build>] python tools/top_hits_rate.py --mode e2e [--variants hits,today] [--hits 2,4] [--steps K] [--out FILE.jsonl]

select  aim_align_device_hits on 4 Mi HBM-resident candidates in reads of 8 (WFA-adaptive l = 100, e = 1 %, score-only RES8, reference
        windows), `steps` calls per max_hits timed with HIP events, next to aim_align_device_groups on the same batch; run it under
        `rocprofv3 --kernel-trace --stats` to read hit_select_kernel's own time next to group_select_kernel's and the score-only pass's.
e2e     hit rows/s through aim_set_submit / aim_set_wait with two slots and pinned inputs, the same batch with compact CIGAR:
        `hits`   one AIM_FLAG_TOP_HITS batch per step, max_hits = N;
        `today`  what a caller does without the flag, on any library of this ABI (AIM_LIB=<the parent build>): an
                 AIM_FLAG_READ_GROUPS batch (the winners' CIGARs and aim_best_t), then -- the host knows each read's winner and that a
                 runner-up exists, not which candidate it is -- a flag-less AIM_FLAG_REF_TEXTS batch with CIGAR of every read's other
                 candidates, gathered on the host, of which it keeps the N - 1 best per read by (score, index). The second batch of
                 step i overlaps the first of step i + 1.
One JSON line per row (stdout, and --out)."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N = 1 << 22
K = 8


def load():
    """Any library of this ABI: one built before a symbol existed (AIM_LIB=<the parent build>) simply lacks it."""
    from aim_amd import capi
    return capi.load(strict=False)


def reference(n, seed=3):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, size=n)].copy()


def batch(ref, rs, n=N, base_reads=2048):
    """n candidates in reads of K: a generated set of base_reads reads repeated (the rate does not depend on which reads repeat)."""
    from aim_amd import engine
    req, rows, offs, tpos, txt, pats = engine.group_pairs(100 + K, 0, base_reads, K, 100, 0.01, ref, rs)
    reps = n // len(req)
    reqb = np.tile(req, reps)
    reqb["idx"] = np.arange(len(reqb), dtype=np.uint32)
    return reqb, np.tile(rows, (reps, 1)), np.arange(base_reads * reps + 1, dtype=np.uint32) * K, np.tile(tpos, reps)


def select_rows(steps, warmup, hits):
    import torch
    torch.cuda.init()   # (before the library: the device buffers are torch's)
    from aim_amd import capi, engine
    lib = load()
    dev = torch.device("cuda:0")
    ref = reference(1 << 24)
    ms, rs = engine.launcher_sizes("wfa", 100, 0.01)
    req, rows, offs, tpos = batch(ref, rs)
    n, nr = len(req), len(offs) - 1
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    d_req, d_rows, d_off, d_tp = t(engine.to_request8(req)), t(rows), t(offs), t(tpos)
    d_ref = torch.zeros(len(ref) + 64, dtype=torch.uint8, device=dev)
    d_ref[: len(ref)] = torch.from_numpy(ref).to(dev)
    d_best = torch.zeros(nr * 16, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    out = []
    for mh in [0] + hits:                      # 0: aim_align_device_groups, the same batch without the flag
        params = engine.make_params("wfa", ms, rs, reduce=True, res8=True, req8=True, ref_texts=True, read_groups=True, top_hits=mh > 0)
        hoff = engine.hits_offsets(offs, mh) if mh else None
        nh = int(hoff[-1]) if mh else nr
        d_res = torch.zeros(nh * 8, dtype=torch.uint8, device=dev)
        d_hoff = t(hoff) if mh else None
        d_pair = torch.zeros(nh * 4, dtype=torch.uint8, device=dev) if mh else None
        sb = lib.aim_scratch_bytes(C.byref(params), n)
        d_scr = torch.zeros(sb, dtype=torch.uint8, device=dev)

        def call():
            if mh:
                engine.align_device_hits(params, n, nr, d_req.data_ptr(), d_rows.data_ptr(), None, d_tp.data_ptr(), d_ref.data_ptr(), len(ref),
                                         d_off.data_ptr(), d_res.data_ptr(), None, d_best.data_ptr(), mh, d_hoff.data_ptr(), nh, d_pair.data_ptr(),
                                         d_scr.data_ptr(), sb, stream)
            else:
                capi.check(lib.aim_align_device_groups(C.byref(params), n, nr, d_req.data_ptr(), d_rows.data_ptr(), None, d_tp.data_ptr(),
                                                       d_ref.data_ptr(), len(ref), d_off.data_ptr(), d_res.data_ptr(), None, d_best.data_ptr(),
                                                       d_scr.data_ptr(), sb, stream))
        for _ in range(warmup):
            call()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(steps):
            call()
        b.record()
        torch.cuda.synchronize()
        ms_call = a.elapsed_time(b) / steps
        buf = C.create_string_buffer(1024)
        capi.check(lib.aim_plan_describe(C.byref(params), n, buf, 1024))
        out.append(dict(part="select", candidates=n, reads=nr, k=K, max_hits=mh, hit_rows=nh, call_ms=round(ms_call, 4),
                        candidates_per_s=round(n / ms_call * 1e3), plan=buf.value.decode()))
        print(json.dumps(out[-1]), flush=True)
        del d_res, d_scr
    return out


class Pinned:
    def __init__(self, lib):
        self.lib, self.ptrs = lib, []

    def __call__(self, a):
        from aim_amd import capi
        p = C.c_void_p()
        capi.check(self.lib.aim_host_alloc(C.byref(p), max(1, a.nbytes)))
        buf = np.ctypeslib.as_array((C.c_uint8 * max(1, a.nbytes)).from_address(p.value))[: a.nbytes].view(a.dtype).reshape(a.shape)
        buf[...] = a
        self.ptrs.append(p)
        return buf

    def free(self):
        for p in self.ptrs:
            self.lib.aim_host_free(p)
        self.ptrs = []


def e2e_rows(steps, warmup, hits, variants):
    from aim_amd import engine
    lib = load()
    ref = reference(1 << 24)
    ms, rs = engine.launcher_sizes("wfa", 100, 0.01)
    req, rows, offs, tpos = batch(ref, rs)
    n, nr = len(req), len(offs) - 1
    kw = dict(reduce=True, req8=True, ref_texts=True, backtrace=True)
    out = []
    for variant in variants:
        for mh in hits:
            pin = Pinned(lib)
            pr, prow, poff, ptp = pin(np.ascontiguousarray(engine.to_request8(req))), pin(rows), pin(offs), pin(tpos)
            nh = nr * min(K, mh)
            t0 = None
            if variant == "hits":
                params = engine.make_params("wfa", ms, rs, read_groups=True, top_hits=True, **kw)
                with engine.DeviceSet(1) as s:
                    s.configure_slots(params, n, slots=2, max_runs=8 * nh)
                    s.set_reference(ref)
                    args = dict(pat=prow, read_offsets=poff, text_pos=ptp, cigar_runs_cap=8 * nh, max_hits=mh)
                    total = warmup + steps
                    for i in range(total):
                        if i == warmup:
                            t0 = time.perf_counter()
                        s.submit(0, i % 2, pr, **args)
                        if i:
                            s.wait(0, (i - 1) % 2)
                    s.wait(0, (total - 1) % 2)
                    dt = time.perf_counter() - t0
                    plan = s.plan_describe(0)
            else:
                # the read's other candidates, K - 1 per read, as a flag-less batch: requests, text_pos and pattern rows gathered on the host
                n2 = nr * (K - 1)
                pg = engine.make_params("wfa", ms, rs, read_groups=True, **kw)
                p0 = engine.make_params("wfa", ms, rs, **kw)
                req2, tp2, pat2 = pin(np.zeros(n2, dtype=pr.dtype)), pin(np.zeros(n2, dtype=np.uint64)), pin(np.zeros((n2, rs), dtype=np.uint8))
                all_c = np.arange(n, dtype=np.int64).reshape(nr, K)
                read_of = np.repeat(np.arange(nr, dtype=np.int64), K - 1)
                with engine.DeviceSet(1) as sa, engine.DeviceSet(1) as sb:
                    sa.configure_slots(pg, n, slots=2, max_runs=8 * nr)
                    sb.configure_slots(p0, n2, slots=2, max_runs=8 * n2)
                    sa.set_reference(ref)
                    sb.set_reference(ref)
                    first = dict(pat=prow, read_offsets=poff, text_pos=ptp, cigar_runs_cap=8 * nr)

                    def second(o, slot):     # the winners are known: everything else goes out again
                        win = o["best"]["best_pair"].astype(np.int64)
                        others = all_c[all_c != win[:, None]].reshape(-1)
                        np.take(pr, others, out=req2)
                        np.take(ptp, others, out=tp2)
                        np.take(prow, read_of, axis=0, out=pat2)
                        sb.submit(0, slot, req2, pat=pat2, text_pos=tp2, cigar_runs_cap=8 * n2)

                    def keep(o):             # the N - 1 best of them per read, by (score, index)
                        sc = o["cig"]["score"].reshape(nr, K - 1)
                        return np.argsort(sc, axis=1, kind="stable")[:, :max(0, mh - 1)]

                    total = warmup + steps
                    sa.submit(0, 0, pr, **first)
                    for i in range(total):
                        if i == warmup:
                            t0 = time.perf_counter()
                        o = sa.wait(0, i % 2)
                        if i + 1 < total:
                            sa.submit(0, (i + 1) % 2, pr, **first)
                        if i:
                            keep(sb.wait(0, (i - 1) % 2))    # (its buffers are free again before they are refilled: one pinned set)
                        second(o, i % 2)
                    keep(sb.wait(0, (total - 1) % 2))
                    dt = time.perf_counter() - t0
                    plan = sa.plan_describe(0) + " || " + sb.plan_describe(0)
            pin.free()
            out.append(dict(part="e2e", variant=variant, max_hits=mh, k=K, candidates=n, reads=nr, hit_rows=nh, slots=2, batches=steps,
                            seconds_per_batch=round(dt / steps, 4), hit_rows_per_s=round(steps * nh / dt), lib=os.environ.get("AIM_LIB", "default"),
                            plan=plan))
            print(json.dumps(out[-1]), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["select", "e2e"], default="select")
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--hits", default="1,2,4,8")
    ap.add_argument("--variants", default="hits,today")
    ap.add_argument("--out")
    a = ap.parse_args()
    hits = [int(x) for x in a.hits.split(",")]
    rows = select_rows(a.steps, a.warmup, hits) if a.mode == "select" else e2e_rows(a.steps, a.warmup, hits, a.variants.split(","))
    if a.out:
        with open(a.out, "a") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
