#!/usr/bin/env python3
"""Reads with candidates (AIM_FLAG_READ_GROUPS): what the selection costs and what the flag saves end to end.

  python tools/read_groups_rate.py [--steps K] [--warmup W] [--parts select,e2e] [--ks 1,4,8,16] [--out FILE.jsonl]

select  aim_align_device_groups on 4 Mi HBM-resident candidates in groups of 8 (WFA-adaptive l = 100, score-only RES8), `steps`
        calls timed with HIP events; run it under `rocprofv3 --kernel-trace --stats` to read group_select_kernel's own time (the
        row's `select_bytes` is what that kernel moves: the candidates' result rows, the offsets, aim_best_t and sel);
e2e     candidates/s through aim_set_submit / aim_set_wait with two slots (pinned inputs), WFA-adaptive l = 100, e = 1 %, groups of K,
        score-only (RES8) and compact CIGAR, REQ8 and reference windows throughout: the flag with one pattern row per read (ASCII, and
        packed 2 bits per base), against the AIM_FLAG_REF_TEXTS path that sends every candidate with its packed pattern (and computes every CIGAR) and picks
        each read's best candidate on the host. H2D bytes per candidate from the buffers sent; the plan line of each.
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

HBM_GBS = 8000.0
N = 1 << 22


def reference(n, seed=3):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, size=n)].copy()


def groups(ref, k, rs, n=N, base_reads=2048):
    """n candidates in reads of k: a generated set of base_reads reads repeated (the rate does not depend on which reads repeat)."""
    from aim_amd import engine
    req, rows, offs, tpos, txt, pats = engine.group_pairs(100 + k, 0, base_reads, k, 100, 0.01, ref, rs)
    reps = n // len(req)
    reqb = np.tile(req, reps)
    reqb["idx"] = np.arange(len(reqb), dtype=np.uint32)
    offsb = np.arange(base_reads * reps + 1, dtype=np.uint32) * k
    return reqb, np.tile(rows, (reps, 1)), offsb, np.tile(tpos, reps), np.tile(pats, (reps, 1))


def select_rows(steps, warmup):
    import torch
    torch.cuda.init()   # (before the library: the device buffers are torch's)
    from aim_amd import capi, engine
    lib = capi.load()
    dev = torch.device("cuda:0")
    ref = reference(1 << 24)
    ms, rs = engine.launcher_sizes("wfa", 100, 0.01)
    req, rows, offs, tpos, _ = groups(ref, 8, rs)
    req8 = engine.to_request8(req)
    n, nr = len(req), len(offs) - 1
    params = engine.make_params("wfa", ms, rs, reduce=True, res8=True, req8=True, ref_texts=True, read_groups=True)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    d_req, d_rows, d_off, d_tp = t(req8), t(rows), t(offs), t(tpos)
    d_ref = torch.zeros(len(ref) + 64, dtype=torch.uint8, device=dev)
    d_ref[: len(ref)] = torch.from_numpy(ref).to(dev)
    d_res = torch.zeros(nr * 8, dtype=torch.uint8, device=dev)
    d_best = torch.zeros(nr * 16, dtype=torch.uint8, device=dev)
    sb = lib.aim_scratch_bytes(C.byref(params), n)
    d_scr = torch.zeros(sb, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def call():
        capi.check(lib.aim_align_device_groups(C.byref(params), n, nr, d_req.data_ptr(), d_rows.data_ptr(), None, d_tp.data_ptr(), d_ref.data_ptr(),
                                               len(ref), d_off.data_ptr(), d_res.data_ptr(), None, d_best.data_ptr(), d_scr.data_ptr(), sb, stream))
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
    row = dict(part="select", candidates=n, reads=nr, k=8, call_ms=round(ms_call, 4), candidates_per_s=round(n / ms_call * 1e3),
               select_bytes=n * 24 + (nr + 1) * 4 + nr * 20, hbm_gbs_roofline=HBM_GBS, plan=buf.value.decode())
    print(json.dumps(row), flush=True)
    return [row]


def e2e_rows(steps, warmup, ks):
    from aim_amd import capi, engine
    lib = capi.load()
    ref = reference(1 << 24)
    ms, rs = engine.launcher_sizes("wfa", 100, 0.01)
    rows_out = []
    for k in ks:
        req, rows, offs, tpos, pats = groups(ref, k, rs)
        n, nr = len(req), len(offs) - 1
        r8 = engine.to_request8(req)
        for cigar in (False, True):
            kw = dict(reduce=True, req8=True, ref_texts=True, **(dict(backtrace=True) if cigar else dict(res8=True)))
            for variant in ("host", "ascii", "packed"):
                use_groups = variant != "host"
                params = engine.make_params("wfa", ms, rs, read_groups=use_groups, **kw)
                cap = (8 * nr if use_groups else 8 * n) if cigar else 0
                host = []

                def pinned(a):
                    if a is None:
                        return None
                    p = C.c_void_p()
                    capi.check(lib.aim_host_alloc(C.byref(p), max(1, a.nbytes)))
                    buf = np.ctypeslib.as_array((C.c_uint8 * max(1, a.nbytes)).from_address(p.value))[: a.nbytes].view(a.dtype).reshape(a.shape)
                    buf[...] = a
                    host.append(p)
                    return buf
                pr, ptp = pinned(np.ascontiguousarray(r8)), pinned(tpos)
                if variant == "packed":
                    pk = tuple(pinned(None if x is None else np.ascontiguousarray(x)) for x in engine.pack_batch(req[offs[:-1]], rows, None))
                    poff = pinned(offs)
                    kwargs = dict(packed=pk, read_offsets=poff, text_pos=ptp, cigar_runs_cap=cap)
                    h2d = 8 + 8 + (nr * pk[0].shape[1] * 4 + (nr + 1) * 4 + len(pk[2]) * (4 + rs)) / n
                elif use_groups:
                    prow, poff = pinned(rows), pinned(offs)
                    kwargs = dict(pat=prow, read_offsets=poff, text_pos=ptp, cigar_runs_cap=cap)
                    h2d = 8 + 8 + (nr * rs + (nr + 1) * 4) / n
                else:
                    packed = engine.pack_batch(r8, pats, None)
                    pk = tuple(pinned(None if x is None else np.ascontiguousarray(x)) for x in packed)
                    kwargs = dict(packed=pk, text_pos=ptp, cigar_runs_cap=cap)
                    h2d = 8 + 8 + pk[0].shape[1] * 4 + len(pk[2]) * (4 + rs) / n
                with engine.DeviceSet(1) as s:
                    s.configure_slots(params, n, slots=2, max_raw=max(1, n // 64), max_runs=cap)
                    s.set_reference(ref)

                    def pick(out):   # the caller's selection without the flag: each read's lowest score, lowest index on a tie
                        sc = (out["cig"]["score"] if cigar else out["res"]["score"]).reshape(-1, k)
                        return np.argmin(sc, axis=1)

                    for i in range(warmup):
                        s.submit(0, i % 2, pr, **kwargs)
                        o = s.wait(0, i % 2)
                        if not use_groups:
                            pick(o)
                    t = time.perf_counter()
                    for i in range(steps):
                        s.submit(0, i % 2, pr, **kwargs)
                        if i:
                            o = s.wait(0, (i - 1) % 2)
                            if not use_groups:
                                pick(o)
                    o = s.wait(0, (steps - 1) % 2)
                    if not use_groups:
                        pick(o)
                    dt = time.perf_counter() - t
                    plan = s.plan_describe(0)
                for p in host:
                    lib.aim_host_free(p)
                rows_out.append(dict(part="e2e", k=k, candidates=n, reads=nr, cigar=cigar, read_groups=use_groups, read_rows=variant, slots=2, batches=steps,
                                     candidates_per_s=round(steps * n / dt), h2d_bytes_per_candidate=round(h2d, 2), plan=plan))
                print(json.dumps(rows_out[-1]), flush=True)
    return rows_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parts", default="select,e2e")
    ap.add_argument("--ks", default="1,4,8,16")
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = []
    if "select" in a.parts:
        rows += select_rows(a.steps, a.warmup)
    if "e2e" in a.parts:
        rows += e2e_rows(a.steps, a.warmup, [int(x) for x in a.ks.split(",")])
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
