#!/usr/bin/env python3
"""Paired-end selection (AIM_FLAG_MATE_PAIRS): what the selection kernel costs and what the flag saves end to end.

  python tools/mate_pairs_rate.py [--steps S] [--warmup W] [--parts select,e2e] [--ks 2,4,8] [--variants host,mates] [--out FILE.jsonl]

select  aim_align_device_mates and aim_align_device_groups on the same 4 Mi HBM-resident candidates in reads of K (WFA-adaptive l = 100,
        e = 1 %, score-only RES8, reference windows), `steps` calls each timed with HIP events: the difference is what the pairing adds
        to a batch. Run it under `rocprofv3 --kernel-trace --stats` to read mate_select_kernel next to group_select_kernel.
e2e     candidates/s through aim_set_submit / aim_set_wait with two slots (pinned inputs), 4 Mi candidates per batch, score-only (RES8)
        and compact CIGAR, REQ8 throughout. "mates": the flag, packed read rows. "host": the only way a library without the flag gives
        the same answer -- every candidate sent with its packed pattern (and every CIGAR computed), the selection rule applied on the
        host (numpy, vectorised over the read pairs; host_pairing_seconds is its share of the timed window). The host variant runs
        on any library (AIM_LIB=... for the parent build).
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
SPAN = (340, 460)
INT32_MAX = 2 ** 31 - 1
MINUS = np.uint64(1 << 63)


def load_library():
    """Any library of this ABI: one built before a symbol existed (AIM_LIB=<the parent build>) simply lacks it."""
    from aim_amd import capi
    return capi.load(strict=False)


def batch(k, rs, n=N, base_pairs=1024):
    """n candidates in reads of k: a generated set of base_pairs read pairs repeated (the rate does not depend on which repeat)."""
    from aim_amd import engine
    ref, req, rows, offs, tpos, txt, pats, truth = engine.mate_pairs(200 + k, base_pairs, 100, 0.01, 400, k, 0.4, read_size=rs)
    reps = n // len(req)
    reqb = np.tile(req, reps)
    reqb["idx"] = np.arange(len(reqb), dtype=np.uint32)
    offsb = np.arange(2 * base_pairs * reps + 1, dtype=np.uint32) * k
    return ref, reqb, np.tile(rows, (reps, 1)), offsb, np.tile(tpos, reps), np.tile(pats, (reps, 1))


def host_pairing(score, tpos, tlen, k, lo, hi, penalty):
    """The selection rule on per-candidate scores (every candidate OK), vectorised over read pairs of k x k candidates: (sel, proper)."""
    nm = len(score) // (2 * k)
    s = score.astype(np.int64).reshape(nm, 2, k)
    start = (tpos & ~MINUS).astype(np.int64).reshape(nm, 2, k)
    minus = ((tpos & MINUS) != 0).reshape(nm, 2, k)
    end = start + tlen.astype(np.int64).reshape(nm, 2, k)
    si, sj = start[:, 0, :, None], start[:, 1, None, :]
    mi, mj = minus[:, 0, :, None], minus[:, 1, None, :]
    start_f, start_r = np.where(mi, sj, si), np.where(mi, si, sj)
    span = np.where(mi, end[:, 0, :, None], end[:, 1, None, :]) - start_f
    ok = (mi != mj) & (start_f <= start_r) & (span >= lo) & (span <= hi)
    cost = np.where(ok, np.minimum(s[:, 0, :, None] + s[:, 1, None, :], INT32_MAX - 1), np.int64(1) << 40).reshape(nm, k * k)
    q = np.argmin(cost, axis=1)                       # (the first minimum: lowest i, then lowest j)
    best = np.argmin(s, axis=2)
    unpaired = np.minimum(np.take_along_axis(s, best[:, :, None], 2)[:, :, 0].sum(axis=1) + penalty, INT32_MAX - 1)
    proper = cost[np.arange(nm), q] <= unpaired
    sel = np.where(proper[:, None], np.stack([q // k, q % k], axis=1), best)
    return (sel + (np.arange(2 * nm).reshape(nm, 2) * k)).reshape(-1), proper


def select_rows(steps, warmup, ks):
    import torch
    torch.cuda.init()   # (before the library: the device buffers are torch's)
    from aim_amd import capi, engine
    lib = load_library()
    dev = torch.device("cuda:0")
    ms, rs = engine.launcher_sizes("wfa", 100, 0.01)
    out = []
    for k in ks:
        ref, req, rows, offs, tpos, _ = batch(k, rs)
        req8 = engine.to_request8(req)
        n, nr = len(req), len(offs) - 1
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
        d_req, d_rows, d_off, d_tp = t(req8), t(rows), t(offs), t(tpos)
        d_ref = torch.zeros(len(ref) + 64, dtype=torch.uint8, device=dev)
        d_ref[: len(ref)] = torch.from_numpy(ref).to(dev)
        d_res = torch.zeros(nr * 8, dtype=torch.uint8, device=dev)
        d_best = torch.zeros(nr * 16, dtype=torch.uint8, device=dev)
        d_mates = torch.zeros((nr // 2) * 32, dtype=torch.uint8, device=dev)
        stream = torch.cuda.current_stream().cuda_stream
        times = {}
        for name in ("groups", "mates"):
            params = engine.make_params("wfa", ms, rs, reduce=True, res8=True, req8=True, ref_texts=True, read_groups=True, mate_pairs=name == "mates")
            sb = lib.aim_scratch_bytes(C.byref(params), n)
            d_scr = torch.zeros(sb, dtype=torch.uint8, device=dev)

            def call():
                if name == "mates":
                    engine.align_device_mates(params, n, nr, d_req.data_ptr(), d_rows.data_ptr(), d_tp.data_ptr(), d_ref.data_ptr(), len(ref),
                                              d_off.data_ptr(), d_res.data_ptr(), None, d_best.data_ptr(), (SPAN[0], SPAN[1], 2 * (ms + 1)),
                                              d_mates.data_ptr(), d_scr.data_ptr(), sb, stream)
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
            times[name] = a.elapsed_time(b) / steps
            del d_scr
        proper = int((d_mates.cpu().numpy().view(capi.MATE_DTYPE)["flags"] & 1).sum())
        row = dict(part="select", k=k, candidates=n, reads=nr, groups_call_ms=round(times["groups"], 4), mates_call_ms=round(times["mates"], 4),
                   pairing_adds_ms=round(times["mates"] - times["groups"], 4), proper_read_pairs=proper, read_pairs=nr // 2)
        print(json.dumps(row), flush=True)
        out.append(row)
    return out


def e2e_rows(steps, warmup, ks, variants):
    from aim_amd import capi, engine
    lib = load_library()
    have_flag = bool(engine.features() & 0x100)
    ms, rs = engine.launcher_sizes("wfa", 100, 0.01)
    mates = (SPAN[0], SPAN[1], 2 * (ms + 1))
    rows_out = []
    for k in ks:
        ref, req, rows, offs, tpos, pats = batch(k, rs)
        n, nr = len(req), len(offs) - 1
        r8 = engine.to_request8(req)
        tlen = req["text_len"]
        for cigar in (False, True):
            kw = dict(reduce=True, req8=True, ref_texts=True, **(dict(backtrace=True) if cigar else dict(res8=True)))
            for variant in variants:
                use_flag = variant == "mates"
                if use_flag and not have_flag:
                    continue
                params = engine.make_params("wfa", ms, rs, read_groups=True, mate_pairs=True, **kw) if use_flag else engine.make_params("wfa", ms, rs, **kw)
                cap = (8 * nr if use_flag else 8 * n) if cigar else 0
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
                if use_flag:
                    pk = tuple(pinned(None if x is None else np.ascontiguousarray(x)) for x in engine.pack_batch(req[offs[:-1]], rows, None))
                    kwargs = dict(packed=pk, read_offsets=pinned(offs), text_pos=ptp, cigar_runs_cap=cap, mates=mates)
                else:
                    pk = tuple(pinned(None if x is None else np.ascontiguousarray(x)) for x in engine.pack_batch(r8, pats, None))
                    kwargs = dict(packed=pk, text_pos=ptp, cigar_runs_cap=cap)
                with engine.DeviceSet(1) as s:
                    s.configure_slots(params, n, slots=2, max_raw=max(1, n // 64), max_runs=cap)
                    s.set_reference(ref)
                    n_proper, pairing_s = [0], [0.0]

                    def finish(o):   # without the flag the caller pairs on the host
                        if use_flag:
                            n_proper[0] = int((o["mates"]["flags"] & 1).sum())
                        else:
                            t0 = time.perf_counter()
                            sel, proper = host_pairing(o["cig"]["score"] if cigar else o["res"]["score"], tpos, tlen, k, *mates)
                            pairing_s[0] += time.perf_counter() - t0
                            n_proper[0] = int(proper.sum())
                    for i in range(warmup):
                        s.submit(0, i % 2, pr, **kwargs)
                        finish(s.wait(0, i % 2))
                    pairing_s[0] = 0.0
                    t = time.perf_counter()
                    for i in range(steps):
                        s.submit(0, i % 2, pr, **kwargs)
                        if i:
                            finish(s.wait(0, (i - 1) % 2))
                    finish(s.wait(0, (steps - 1) % 2))
                    dt = time.perf_counter() - t
                    plan = s.plan_describe(0)
                for p in host:
                    lib.aim_host_free(p)
                rows_out.append(dict(part="e2e", k=k, candidates=n, reads=nr, cigar=cigar, variant=variant, library=os.path.basename(capi.LIB_PATH),
                                     slots=2, batches=steps, candidates_per_s=round(steps * n / dt), seconds=round(dt, 3),
                                     host_pairing_seconds=round(pairing_s[0], 3), proper_read_pairs=n_proper[0], plan=plan))
                print(json.dumps(rows_out[-1]), flush=True)
    return rows_out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parts", default="select,e2e")
    ap.add_argument("--ks", default="2,4,8")
    ap.add_argument("--variants", default="host,mates")
    ap.add_argument("--out")
    a = ap.parse_args()
    ks = [int(x) for x in a.ks.split(",")]
    rows = []
    if "select" in a.parts:
        rows += select_rows(a.steps, a.warmup, ks)
    if "e2e" in a.parts:
        rows += e2e_rows(a.steps, a.warmup, ks, a.variants.split(","))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
