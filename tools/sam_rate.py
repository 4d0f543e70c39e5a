"""Measurements of AIM_FLAG_SAM_FIELDS, one JSON line per row.

    python tools/sam_rate.py --mode kernel [--lengths 100,1000,10000] [--error 0.01] [--mbytes 256] [--reps 10] [--rounds 5]
    [AIM_LIB=<another build>] python tools/sam_rate.py --mode e2e [--rows 4194304] [--steps 6] [--variants ops,runs,sam,sam_runs]

kernel: both mappings of the record kernel (aim_sam_device) on synthetic ops rows; the mappings alternate over --rounds rounds and
each row carries every round's time, the median and the spread.
e2e: WFA-adaptive l = 100, e = 1 %, reference windows, packed reads, REQ8, through two slots of aim_set_submit / aim_set_wait with every
host buffer pinned (aim_host_alloc). Variants: `ops` returns result rows + ops rows, `runs` compact CIGAR headers + runs (both without
the flag, so they run on a library built before it: AIM_LIB), `sam` the records alone, `sam_runs` records + compact CIGAR. rows/s and
D2H bytes per row. The figures without the flag EXCLUDE the host-side conversion to POS / CIGAR / NM / MD a caller still has to do
(and cannot do for MD without a host copy of the reference). Under `rocprofv3 --kernel-trace --stats` the `sam_runs` variant puts
sam_lane_kernel next to cigar_rle_kernel and the alignment kernels on the same batch.

kernel mode in detail:

Rows are made on the host: 'M' with 'X' / 'I' / 'D' at the given rate, on both strands, against a random reference; the ops buffer
holds about --mbytes of rows. Each mapping is forced with AIM_SAM_WAVE_MIN (0: one row per wavefront, 1 << 30: one row per lane),
run once to warm up and --reps times between two device synchronisations. bytes = the algorithmic traffic: ops ranges and result rows
read, text_pos read, reference bytes read (one per 'X' / 'I'), records, words and MD bytes written. The figure is a kernel-only rate: no
alignment, no PCIe. The switch point (kSamWaveMinReadSize, sam_fields.hpp) is where the two mappings cross."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_rows(n, length, error, rs, seed=1):
    from aim_amd import capi
    rng = np.random.default_rng(seed)
    ops = np.full((n, 2 * rs), ord("M"), dtype=np.uint8)
    r = rng.random((n, length))
    body = np.full((n, length), ord("M"), dtype=np.uint8)
    body[r < error] = ord("X")
    body[r < 2 * error / 3] = ord("I")
    body[r < error / 3] = ord("D")
    body[:, 0] = body[:, -1] = ord("M")
    ops[:, 2 * rs - length:] = body
    res = np.zeros(n, dtype=capi.RESULT_DTYPE)
    res["begin_offset"], res["end_offset"], res["idx"] = 2 * rs - length, 2 * rs, np.arange(n)
    return res, ops, int((body != ord("M")).sum()), int((body == ord("X")).sum() + (body == ord("I")).sum())


def kernel_mode(a):
    from aim_amd import capi, engine
    lib = capi.load()
    hip = C.CDLL(next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line))
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipFree.argtypes = [C.c_void_p]

    def up(arr):
        v = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        p = C.c_void_p()
        assert hip.hipMalloc(C.byref(p), len(v) + 64) == 0
        assert hip.hipMemcpy(p, v.ctypes.data, len(v), 1) == 0
        return p

    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(7).integers(0, 4, size=1 << 26)]
    d_ref = up(ref)
    for length in (int(x) for x in a.lengths.split(",")):
        rs = engine.round_up_8(int(length * (1 + a.error)) + 8)
        n = max(64, (a.mbytes << 20) // (2 * rs))
        res, ops, edits, ref_reads = make_rows(n, length, a.error, rs)
        tpos = np.random.default_rng(3).integers(0, len(ref) - 2 * length, size=n).astype(np.uint64)
        tpos[1::2] |= np.uint64(1 << 63)
        bufs = [up(res), up(ops), up(tpos), up(np.zeros(n, dtype=capi.REQUEST_DTYPE))]
        d_res, d_ops, d_tp, d_req = bufs
        ccap, mcap = n * 4 + 4 * edits, n * 12 + 4 * edits
        d_sam, d_cg, d_md, d_cur = (up(np.zeros(k, dtype=np.uint8)) for k in (n * 48, 4 * ccap, mcap, 8))
        params = engine.make_params("wfa", 1 << 20, rs, backtrace=True, ref_texts=True)
        call = lambda: capi.check(lib.aim_sam_device(capi.params_ref(params), n, d_req, d_tp, None, d_res, d_ops, d_ref, len(ref), 0, d_sam,
                                                     d_cg, ccap, d_md, mcap, d_cur, None))
        maps = (("row_per_lane", str(1 << 30)), ("row_per_wavefront", "0"))
        times = {name: [] for name, _ in maps}
        cur = np.zeros(2, dtype=np.uint32)
        for rnd in range(a.rounds + 1):                  # round 0 warms both mappings up and is dropped
            for name, knob in maps:
                os.environ["AIM_SAM_WAVE_MIN"] = knob
                assert engine.sam_kernel_name(params) == ("sam_wave_kernel" if knob == "0" else "sam_lane_kernel")
                call()
                hip.hipDeviceSynchronize()
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    call()
                hip.hipDeviceSynchronize()
                if rnd:
                    times[name].append((time.perf_counter() - t0) / a.reps * 1e6)
        hip.hipMemcpy(cur.ctypes.data, d_cur, 8, 2)
        nbytes = n * (length + 24 + 8 + 48) + ref_reads + 4 * int(cur[0]) + int(cur[1])
        for name, _ in maps:
            t = sorted(times[name])
            us = t[len(t) // 2]
            print(json.dumps(dict(part="kernel", length=length, read_size=rs, rows=n, error=a.error, mapping=name, reps=a.reps, us_rounds=[round(x, 1) for x in times[name]],
                                  us_median=round(us, 1), us_min=round(t[0], 1), us_max=round(t[-1], 1), rows_per_s=round(n / us * 1e6),
                                  cigar_words=int(cur[0]), md_bytes=int(cur[1]), algorithmic_bytes=nbytes, tb_per_s=round(nbytes / us / 1e6, 3),
                                  of_8tbs_roofline=round(nbytes / us / 1e6 / 8.0, 3))), flush=True)
        for p in bufs + [d_sam, d_cg, d_md, d_cur]:
            hip.hipFree(p)


def e2e_mode(a):
    from aim_amd import capi, engine
    lib = capi.load(strict=False)
    have = bool(lib.aim_features() & capi.FEATURE_SAM_FIELDS)
    ms, rs = engine.launcher_sizes("wfa", 100, 0.01)
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(7).integers(0, 4, size=1 << 24)].copy()
    base = 4096
    n = a.rows // base * base
    req0, pat0, tpos0, _ = engine.ref_pairs(1, 0, base, 100, 0.01, ref, rs)
    pp0, _, raw, _, _ = engine.pack_batch(req0, pat0, None)
    assert len(raw) == 0
    req = engine.to_request8(np.tile(req0, n // base))
    req["idx"] = np.arange(n, dtype=np.uint32)
    host = []

    def pinned(nbytes, init=None):
        p = C.c_void_p()
        capi.check(lib.aim_host_alloc(C.byref(p), max(1, nbytes)))
        host.append(p)
        buf = np.ctypeslib.as_array((C.c_uint8 * max(1, nbytes)).from_address(p.value))
        if init is not None:
            buf[:nbytes] = np.ascontiguousarray(init).view(np.uint8).reshape(-1)
        return buf

    h_req, h_pp, h_tp = pinned(req.nbytes, req), pinned(n * pp0.shape[1] * 4, np.tile(pp0, (n // base, 1))), pinned(n * 8, np.tile(tpos0, n // base))
    wcap, mcap, rcap = 6 * n, 16 * n, 8 * n
    out = [dict(res=pinned(n * 24), ops=pinned(n * 2 * rs), cig=pinned(n * 16), runs=pinned(rcap * 4), sam=pinned(n * 48), words=pinned(wcap * 4),
                md=pinned(mcap)) for _ in range(2)]
    for variant in a.variants.split(","):
        flag = variant.startswith("sam")
        if flag and not have:
            continue
        params = engine.make_params("wfa", ms, rs, reduce=True, backtrace=True, req8=True, ref_texts=True, sam=flag)
        runs = variant in ("runs", "sam_runs")
        ios = []
        for o in out:
            sio = capi.BatchIOSam()
            rio = sio.mates.groups
            io = rio.base
            io.n_pairs, io.requests, io.packed_patterns, rio.text_pos = n, h_req.ctypes.data, h_pp.ctypes.data, h_tp.ctypes.data
            if variant == "ops":
                io.results, io.ops = o["res"].ctypes.data, o["ops"].ctypes.data
            if runs:
                io.cigars, io.runs, io.runs_cap = o["cig"].ctypes.data, o["runs"].ctypes.data, rcap
            if flag:
                sio.sam, sio.sam_cigar, sio.sam_cigar_cap, sio.sam_md, sio.sam_md_cap = o["sam"].ctypes.data, o["words"].ctypes.data, wcap, o["md"].ctypes.data, mcap
            ios.append(sio)
        with engine.DeviceSet(1) as s:
            s.configure_slots(params, n, slots=2, max_raw=64, max_runs=rcap if runs else 0)
            s.set_reference(ref)
            if flag:
                s.sam_capacity(wcap, mcap)
            nr = C.c_uint32()
            sub = lambda i: capi.check(lib.aim_set_submit(s.handle, 0, i % 2, C.byref(ios[i % 2].mates.groups.base)))
            wait = lambda i: capi.check(lib.aim_set_wait(s.handle, 0, i % 2, C.byref(nr)))
            for i in range(2):
                sub(i)
                wait(i)
            t0 = time.perf_counter()
            for i in range(a.steps):
                sub(i)
                if i:
                    wait(i - 1)
            wait(a.steps - 1)
            dt = time.perf_counter() - t0
            plan = s.plan_describe(0)
        d2h = 0.0
        if variant == "ops":
            d2h += 24 + 2 * rs
        if runs:
            d2h += 16 + 4.0 * nr.value / n
        if flag:
            rec = out[(a.steps - 1) % 2]["sam"][:n * 48].view(capi.SAM_DTYPE)
            assert not (rec["status"] & capi.SAM_OVERFLOW).any()
            d2h += 48 + (4.0 * int(rec["n_cigar"].sum(dtype=np.int64)) + int(rec["md_len"].sum(dtype=np.int64))) / n
        print(json.dumps(dict(part="e2e", variant=variant, library=os.path.basename(capi.LIB_PATH), rows=n, slots=2, batches=a.steps, seconds=round(dt, 4),
                              rows_per_s=round(a.steps * n / dt), d2h_bytes_per_row=round(d2h, 1), h2d_bytes_per_row=8 + pp0.shape[1] * 4 + 8,
                              host_conversion_included=bool(flag), plan=plan)), flush=True)
    for p in host:
        lib.aim_host_free(p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", default="kernel", choices=["kernel", "e2e"])
    ap.add_argument("--lengths", default="100,1000,10000")
    ap.add_argument("--error", type=float, default=0.01)
    ap.add_argument("--mbytes", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--rows", type=int, default=4 << 20)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--variants", default="ops,runs,sam,sam_runs")
    a = ap.parse_args()
    (kernel_mode if a.mode == "kernel" else e2e_mode)(a)


if __name__ == "__main__":
    main()
