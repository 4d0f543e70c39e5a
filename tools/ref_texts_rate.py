#!/usr/bin/env python3
"""Reference-window texts (AIM_FLAG_REF_TEXTS): what the gather costs and what it saves end to end.

  python tools/ref_texts_rate.py [--steps K] [--warmup W] [--parts gather,e2e] [--out FILE.jsonl]

gather  the gather pass alone at l = 100, 1 000 and 10 000 on each strand: aim_align_device_ref minus aim_align_device of the same
        HBM-resident batch (WFA-adaptive score-only, HIP events, `steps` launches each), reported as GB/s of text-row bytes written
        plus window bytes read, against the 8 TB/s HBM roofline;
e2e     PCIe-inclusive pairs/s through aim_set_submit / aim_set_wait with two slots (pinned host buffers), explicit packed texts
        against AIM_FLAG_REF_TEXTS with packed patterns, for WFA-adaptive l = 100, e = 1 % (score-only RES8 and compact CIGAR) and
        NW l = 1 000, e = 5 % (score-only), with the H2D bytes per pair of each and the plan line.
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


def reference(n, seed=1):
    return np.frombuffer(b"ACGT", dtype=np.uint8)[np.random.default_rng(seed).integers(0, 4, size=n)].copy()


def tile(n, req, pat, tpos, txt):
    """n pairs from a smaller generated set (the rate does not depend on which windows repeat)."""
    k = -(-n // len(req))
    req2 = np.tile(req, k)[:n].copy()
    req2["idx"] = np.arange(n, dtype=np.uint32)
    return req2, np.tile(pat, (k, 1))[:n].copy(), np.tile(tpos, k)[:n].copy(), np.tile(txt, (k, 1))[:n].copy()


def gather_rows(steps, warmup):
    import torch
    torch.cuda.init()   # (before the library: the device buffers are torch's)
    from aim_amd import capi, engine
    lib = capi.load()
    dev = torch.device("cuda:0")
    ref = reference(1 << 26)
    d_ref = torch.zeros(len(ref) + 64, dtype=torch.uint8, device=dev)
    d_ref[: len(ref)] = torch.from_numpy(ref).to(dev)
    rows = []
    for l, n in ((100, 1 << 22), (1000, 1 << 19), (10000, 1 << 15)):
        ms, rs = engine.launcher_sizes("wfa", l, 0.01)
        req, pat, tpos, txt = tile(n, *engine.ref_pairs(l, 0, 4096, l, 0.0, ref, rs, minus_fraction=0.0))
        p0 = engine.make_params("wfa", ms, rs, reduce=True, res8=True)
        p1 = engine.make_params("wfa", ms, rs, reduce=True, res8=True, ref_texts=True)
        for strand in (0, 1):
            tp = tpos | np.uint64(strand << 63)
            txt_s = txt if not strand else np.stack([engine.ref_window(ref, int(tp[i]) & ((1 << 63) - 1), l, True) for i in range(4096)])
            txt_s = np.tile(np.pad(txt_s, ((0, 0), (0, rs - txt_s.shape[1]))), (-(-n // 4096), 1))[:n] if strand else txt
            pat_s = txt_s   # (e = 0: each pattern is its text, so both strands cost the alignment kernel the same)
            d_req = torch.from_numpy(req.view(np.uint8).copy()).to(dev)
            d_pat = torch.from_numpy(np.ascontiguousarray(pat_s)).to(dev)
            d_txt = torch.zeros(n * rs + 64, dtype=torch.uint8, device=dev)
            d_txt[: n * rs] = torch.from_numpy(np.ascontiguousarray(txt_s).reshape(-1)).to(dev)
            d_tp = torch.from_numpy(tp.view(np.uint8).copy()).to(dev)
            d_res = torch.zeros(n * 8, dtype=torch.uint8, device=dev)
            sb = max(lib.aim_scratch_bytes(C.byref(p0), n), lib.aim_scratch_bytes(C.byref(p1), n))
            d_scr = torch.zeros(sb, dtype=torch.uint8, device=dev)
            stream = torch.cuda.current_stream().cuda_stream

            def explicit():
                capi.check(lib.aim_align_device(C.byref(p0), n, d_req.data_ptr(), d_pat.data_ptr(), d_txt.data_ptr(), d_res.data_ptr(), None,
                                                d_scr.data_ptr(), sb, stream))

            def by_ref():
                capi.check(lib.aim_align_device_ref(C.byref(p1), n, d_req.data_ptr(), d_pat.data_ptr(), d_tp.data_ptr(), d_ref.data_ptr(), len(ref),
                                                    d_res.data_ptr(), None, d_scr.data_ptr(), sb, stream))

            def timed(fn):
                for _ in range(warmup):
                    fn()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                a.record()
                for _ in range(steps):
                    fn()
                b.record()
                torch.cuda.synchronize()
                return a.elapsed_time(b) / steps

            t0, t1 = timed(explicit), timed(by_ref)
            res_ref = d_res.cpu().numpy().view(capi.RESULT8_DTYPE).copy()
            explicit()
            torch.cuda.synchronize()
            same = bool(np.array_equal(res_ref, d_res.cpu().numpy().view(capi.RESULT8_DTYPE)))
            moved = n * rs + n * l + n * 24        # rows written + window bytes read + requests / text_pos read
            dt = max(t1 - t0, 1e-6)
            rows.append(dict(part="gather", l=l, strand=strand, pairs=n, read_size=rs, explicit_ms=round(t0, 4), ref_ms=round(t1, 4),
                             gather_ms=round(t1 - t0, 4), gather_gbs=round(moved / dt / 1e6, 1),
                             roofline_frac=round(moved / dt / 1e6 / HBM_GBS, 3), results_equal=same))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def e2e_rows(steps, warmup):
    from aim_amd import capi, engine
    lib = capi.load()
    ref = reference(1 << 26, seed=2)
    rows = []
    for algo, l, e, n, kw, runs in (("wfa", 100, 0.01, 1 << 22, dict(reduce=True, res8=True, req8=True), False),
                                    ("wfa", 100, 0.01, 1 << 22, dict(reduce=True, backtrace=True, req8=True), True),
                                    ("nw", 1000, 0.05, 1 << 17, dict(), False)):
        ms, rs = engine.launcher_sizes(algo, l, e)
        req, pat, tpos, txt = tile(n, *engine.ref_pairs(l + 7, 0, 8192, l, e, ref, rs))
        for use_ref in (False, True):
            params = engine.make_params(algo, ms, rs, ref_texts=use_ref, **kw)
            r = engine.to_request8(req) if kw.get("req8") else req
            packed = engine.pack_batch(r, pat, None if use_ref else txt)
            cap = 8 * n if runs else 0
            with engine.DeviceSet(1) as s:
                s.configure_slots(params, n, slots=2, max_raw=max(1, n // 64), max_runs=cap)
                if use_ref:
                    s.set_reference(ref)
                # pinned staging (aim_host_alloc), as a pipelined caller holds it
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
                pr = pinned(np.ascontiguousarray(r))
                pk = tuple(pinned(None if x is None else np.ascontiguousarray(x)) for x in packed)
                ptp = pinned(tpos) if use_ref else None
                kwargs = dict(packed=pk, cigar_runs_cap=cap, text_pos=ptp)

                def batch(slot):
                    s.submit(0, slot, pr, **kwargs)
                for i in range(warmup):
                    batch(i % 2)
                    s.wait(0, i % 2)
                t = time.perf_counter()
                for i in range(steps):
                    batch(i % 2)
                    if i:
                        s.wait(0, (i - 1) % 2)
                s.wait(0, (steps - 1) % 2)
                dt = time.perf_counter() - t
                plan = s.plan_describe(0)
                for p in host:
                    lib.aim_host_free(p)
            h2d = r.dtype.itemsize + pk[0].shape[1] * 4 + (8 if use_ref else pk[1].shape[1] * 4) + len(pk[2]) * (4 + rs * (1 if use_ref else 2)) / n
            rows.append(dict(part="e2e", algo=algo, l=l, error=e, pairs=n, cigar=runs, ref_texts=use_ref, slots=2, batches=steps,
                             pairs_per_s=round(steps * n / dt), h2d_bytes_per_pair=round(h2d, 2), n_raw=len(pk[2]), plan=plan))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parts", default="gather,e2e")
    ap.add_argument("--out")
    a = ap.parse_args()
    rows = []
    if "gather" in a.parts:
        rows += gather_rows(a.steps, a.warmup)
    if "e2e" in a.parts:
        rows += e2e_rows(a.steps, a.warmup)
    if a.out:
        with open(a.out, "w") as f:
            for r in rows:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
