#!/usr/bin/env python3
"""The index built on the device (aim_index_build_device): what each kernel costs, how far the passes are from the HBM roofline, and
what the whole build saves against the host build plus its upload.

  python tools/index_rate.py [--k 11,14] [--log2 24,28,31] [--repeat] [--rounds 5] [--no-trace] [--out-dir profiles/index] [--w 5,10,19]

For every k and every reference -- seeded random A C G T of 2^24, 2^28 and 2^31 bases (generated on the device and copied to the host;
the last is skipped, and the row says so, when reference + index + scratch do not fit AIM_SCRATCH_GB or, without it, 3/4 of the free
device memory) and, with --repeat, one repeat-heavy reference of 6 000 000 bases whose second half is 10 000 copies of one 300-base unit
-- one JSON row (stdout and <out-dir>/index_rate_<name>_k<k>.json):
  e2e      the device build (reference resident, buffers allocated once; a host clock around the call and a stream synchronise) and
           the alternative a caller has without it: aim_index_build with 16 threads, then one pinned host-to-device copy of bucket[]
           and of pos[:n_pos]. The two alternate for `rounds` rounds after one warm-up each; median, min and max of both, and the
           ratio of the medians. The device result is compared with the host's (bucket and pos[:n_pos]) once.
  kernels  per-kernel time from a `rocprofv3 --kernel-trace` run of its own with nothing else traced (this program as a child, three
           builds, the first dropped), summed per kernel name over one build, and the bytes the algorithm needs for that kernel (stated
           in csrc/index.hpp) against the 8 TB/s roofline.
With --w the row (<out-dir>/index_rate_<name>_k<k>_minimizers.json) compares aim_index_build_device_minimizers at every listed window
with aim_index_build_device in the same library instead: the builds alternate within each of `rounds` rounds, and the row holds their
times, n_pos over the positions, the per-kernel times of a trace per window, the code pass against the roofline and the share of the
build that sorts positions the index does not keep. Up to 2^24 bases the result is compared with aim_index_build_minimizers."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TILE, PARTS = 4096, 2048


def device_reference(torch, dev, n, repeat, seed=5):
    """uint8 tensor of n + 16 bytes on the device: random A C G T, or (repeat) a random first half and copies of one 300-base unit."""
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    lut = torch.tensor(list(b"ACGT"), dtype=torch.uint8, device=dev)
    d = torch.zeros(n + 16, dtype=torch.uint8, device=dev)
    for lo in range(0, n, 1 << 28):
        m = min(1 << 28, n - lo)
        d[lo:lo + m] = lut[torch.randint(0, 4, (m,), generator=g, device=dev)]
    if repeat:
        unit = d[:300].clone()
        d[n // 2:n] = unit.repeat((n - n // 2 + 299) // 300)[:n - n // 2]
    return d


def algorithmic_bytes(k, n_pos_cap, n_codes):
    """Bytes each kernel must move for one build (csrc/index.hpp, BYTES PER POSITION), summed over its launches."""
    passes = (2 * k + 1 + 7) // 8
    tiles = (n_pos_cap + TILE - 1) // TILE
    table = 256 * 4 * tiles
    scans = passes * table + (n_codes + 1) * 4
    return {"index_code_kernel": n_pos_cap * (1 + 4), "index_hist_kernel": passes * (n_pos_cap * 4 + table),
            "index_scatter_kernel": n_pos_cap * (12 + 16 * (passes - 2) + 12) + passes * table,
            "index_scan_sums_kernel": scans, "index_scan_top_kernel": (passes + 1) * PARTS * 8, "index_scan_apply_kernel": 2 * scans}


def setup(k, log2, repeat):
    import torch
    torch.cuda.init()   # (before the library: the device buffers are torch's)
    from aim_amd import engine
    dev = torch.device("cuda:0")
    n = 6000000 if repeat else 1 << log2
    be, pc = engine.index_sizes(k, n)
    sb = engine.index_device_scratch(k, n)
    need = n + 16 + 4 * be + 4 * pc + sb + 4 * pc      # reference, index, scratch, and the host path's own pos[] on the device
    free_b, _ = torch.cuda.mem_get_info(dev)
    budget = float(os.environ["AIM_SCRATCH_GB"]) * 2 ** 30 if os.environ.get("AIM_SCRATCH_GB") else free_b * 0.75
    if need > budget:
        return None, dict(skipped="needs %.1f GB of device memory, the budget is %.1f GB" % (need / 2 ** 30, budget / 2 ** 30))
    d_ref = device_reference(torch, dev, n, repeat)
    s = dict(torch=torch, engine=engine, dev=dev, n=n, be=be, pc=pc, sb=sb, d_ref=d_ref, d_bucket=torch.empty(be * 4, dtype=torch.uint8, device=dev),
             d_pos=torch.empty(pc * 4, dtype=torch.uint8, device=dev), d_scr=torch.empty(sb, dtype=torch.uint8, device=dev),
             stream=torch.cuda.current_stream(dev))

    def build(w=0):
        ptrs = (s["d_bucket"].data_ptr(), s["d_pos"].data_ptr(), s["d_scr"].data_ptr(), sb, s["stream"].cuda_stream)
        if w:
            engine.index_build_device_minimizers(d_ref.data_ptr(), n, k, w, *ptrs)
        else:
            engine.index_build_device(d_ref.data_ptr(), n, k, *ptrs)
        s["stream"].synchronize()
    s["build"] = build
    return s, {}


def child(k, log2, repeat, ws):
    s, why = setup(k, log2, repeat)
    if s is None:
        sys.exit(3)
    for w in [0] + ws:
        for _ in range(3):
            s["build"](w)


def trace(k, log2, repeat, ws=()):
    """[{kernel name: microseconds per build}, ...] for the plain build and every window of `ws`, from ONE rocprofv3 --kernel-trace run
    of this program's --child mode: three builds each, the first of each dropped."""
    ws = list(ws)
    with tempfile.TemporaryDirectory() as td:
        cmd = ["rocprofv3", "--kernel-trace", "-d", td, "-o", "p", "--output-format", "csv", "--", sys.executable, os.path.abspath(__file__), "--child",
               "--k", str(k), "--log2", str(log2)] + (["--repeat"] if repeat else []) + (["--w", ",".join(str(w) for w in ws)] if ws else [])
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
        if r.returncode:
            return [{"error": "rocprofv3 run failed (%d): %s" % (r.returncode, r.stderr[-300:])}] * (1 + len(ws))
        rows = []
        for f in glob.glob(td + "/**/*kernel_trace.csv", recursive=True):
            rows += [(int(x["Start_Timestamp"]), int(x["End_Timestamp"]), x["Kernel_Name"]) for x in csv.DictReader(open(f))]
    from aim_amd import capi
    plain = capi.load().aim_index_kernel_names().decode().split(",")
    first = [plain[0], capi.load().aim_minimizer_kernel_names().decode().split(",")[0]]     # a build starts with one of the two code passes
    rows = sorted(x for x in rows if any(nm in x[2] for nm in plain + first))
    starts = [i for i, x in enumerate(rows) if any(nm in x[2] for nm in first)]
    if len(starts) != 3 * (1 + len(ws)):
        return [{"error": "expected %d builds in the trace, found %d" % (3 * (1 + len(ws)), len(starts))}] * (1 + len(ws))
    starts.append(len(rows))
    res = []
    for g in range(1 + len(ws)):
        names = [first[1 if g else 0]] + plain[1:]
        out = {nm: 0.0 for nm in names}
        launches = {nm: 0 for nm in names}
        span = 0.0
        for b in (3 * g + 1, 3 * g + 2):                 # the group's first build is the warm-up
            for s0, e0, kn in rows[starts[b]:starts[b + 1]]:
                nm = next(x for x in names if x in kn)
                out[nm] += (e0 - s0) / 1e3 / 2
                launches[nm] += 1
            span += (rows[starts[b + 1] - 1][1] - rows[starts[b]][0]) / 2e3
        res.append({"us_per_build": {nm: round(v, 1) for nm, v in out.items()}, "launches_per_build": {nm: launches[nm] // 2 for nm in names},
                    "span_us_per_build": round(span, 1)})
    return res


def row(k, log2, repeat, rounds, want_trace):
    name = "repeat6M" if repeat else "random2p%d" % log2
    out = dict(reference=name, k=k)
    s, why = setup(k, log2, repeat)
    if s is None:
        out.update(why)
        return name, out
    torch, engine, n = s["torch"], s["engine"], s["n"]
    ref = s["d_ref"][:n].cpu().numpy()
    bucket = torch.empty(s["be"], dtype=torch.int32).pin_memory().numpy().view(np.uint32)
    pos = torch.empty(max(s["pc"], 1), dtype=torch.int32).pin_memory().numpy().view(np.uint32)
    d_b2, d_p2 = torch.empty(s["be"] * 4, dtype=torch.uint8, device=s["dev"]), torch.empty(s["pc"] * 4, dtype=torch.uint8, device=s["dev"])
    import ctypes as C
    from aim_amd import capi

    def host_way():
        t0 = time.perf_counter()
        n_pos = C.c_uint64()
        capi.check(capi.load().aim_index_build(capi.ptr(ref), n, k, capi.ptr(bucket), capi.ptr(pos), C.byref(n_pos), 16))
        t1 = time.perf_counter()
        d_b2.copy_(torch.from_numpy(bucket.view(np.uint8)), non_blocking=True)
        d_p2[:n_pos.value * 4].copy_(torch.from_numpy(pos[:n_pos.value].view(np.uint8)), non_blocking=True)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, t1 - t0, n_pos.value

    def device_way():
        t0 = time.perf_counter()
        s["build"]()
        return time.perf_counter() - t0

    device_way()
    _, _, n_pos = host_way()
    same = bool(torch.equal(s["d_bucket"], d_b2) and torch.equal(s["d_pos"][:n_pos * 4], d_p2[:n_pos * 4]))
    dt, ht, hb = [], [], []
    for _ in range(rounds):
        dt.append(device_way())
        a, b, _ = host_way()
        ht.append(a)
        hb.append(b)
    stats = lambda v: dict(median_s=round(statistics.median(v), 5), min_s=round(min(v), 5), max_s=round(max(v), 5))
    out.update(ref_len=n, n_pos=n_pos, passes=(2 * k + 1 + 7) // 8, scratch_bytes=s["sb"], index_bytes=4 * (s["be"] + n_pos), equals_host_build=same, rounds=rounds,
               device_build=stats(dt), host_build_plus_copy=stats(ht), host_build_alone=stats(hb),
               host_over_device=round(statistics.median(ht) / statistics.median(dt), 2),
               positions_per_s_device=round(s["pc"] / statistics.median(dt)))
    need = algorithmic_bytes(k, s["pc"], 4 ** k)
    out["algorithmic_bytes"] = need
    out["algorithmic_bytes_per_position"] = round(sum(need.values()) / max(s["pc"], 1), 1)
    out["whole_build_share_of_8tb_per_s"] = round(sum(need.values()) / statistics.median(dt) / 8e12, 4)
    del s, d_b2, d_p2
    torch.cuda.empty_cache()
    if want_trace:
        t = trace(k, log2, repeat)[0]
        out["kernels"] = t
        if "us_per_build" in t:
            out["kernel_share_of_8tb_per_s"] = {nm: round(need[nm] / (us * 1e-6) / 8e12, 4) for nm, us in t["us_per_build"].items() if us > 0}
    return name, out


def row_minimizers(k, log2, repeat, rounds, ws, want_trace):
    name = "repeat6M" if repeat else "random2p%d" % log2
    out = dict(reference=name, k=k, windows=ws)
    s, why = setup(k, log2, repeat)
    if s is None:
        out.update(why)
        return name, out
    torch, engine, n = s["torch"], s["engine"], s["n"]

    def timed(w):
        t0 = time.perf_counter()
        s["build"](w)
        return time.perf_counter() - t0

    n_pos, same = {}, {}
    for w in [0] + ws:                                # warm-up, n_pos and the comparison with the host build
        timed(w)
        n_pos[w] = int(s["d_bucket"][(s["be"] - 1) * 4:].cpu().numpy().view(np.uint32)[0])
        if w and n <= 1 << 24:
            hb, hp = engine.index_build_minimizers(s["d_ref"][:n].cpu().numpy(), k, w, threads=16)
            same[w] = bool(np.array_equal(s["d_bucket"].cpu().numpy().view(np.uint32), hb)
                           and np.array_equal(s["d_pos"][:4 * n_pos[w]].cpu().numpy().view(np.uint32), hp))
    times = {w: [] for w in [0] + ws}
    for _ in range(rounds):
        for w in [0] + ws:
            times[w].append(timed(w))
    stats = lambda v: dict(median_s=round(statistics.median(v), 5), min_s=round(min(v), 5), max_s=round(max(v), 5))
    need = algorithmic_bytes(k, s["pc"], 4 ** k)
    out.update(ref_len=n, positions=s["pc"], rounds=rounds, passes=(2 * k + 1 + 7) // 8, plain=dict(n_pos=n_pos[0], device_build=stats(times[0])))
    pc, sb = s["pc"], s["sb"]
    del s
    torch.cuda.empty_cache()
    traces = trace(k, log2, repeat, ws) if want_trace else None
    for g, w in enumerate(ws, 1):
        r = dict(n_pos=n_pos[w], n_pos_over_positions=round(n_pos[w] / max(pc, 1), 4), two_over_w_plus_1=round(2 / (w + 1), 4),
                 equals_host_build=same.get(w), device_build=stats(times[w]),
                 over_plain=round(statistics.median(times[w]) / statistics.median(times[0]), 3))
        if want_trace:
            t = traces[g]
            r["kernels"] = t
            if "us_per_build" in t:
                us = t["us_per_build"]
                code = us["index_minimizer_kernel"]
                # the code pass moves what index_code_kernel moves (1 B read, 4 B written per position) plus the halo's share
                code_bytes = need["index_code_kernel"] * (1 + 2 * (w - 1) / TILE * 1 / 5)
                r["code_pass_bytes_per_position"] = round(code_bytes / max(pc, 1), 3)
                r["code_pass_share_of_8tb_per_s"] = round(code_bytes / (code * 1e-6) / 8e12, 4) if code > 0 else None
                sort_us = sum(us[nm] for nm in us if nm != "index_minimizer_kernel")
                r["sort_share_of_kernel_time"] = round(sort_us / max(sort_us + code, 1e-9), 4)
                # the hist / scatter / table-scan passes run over all positions; 1 - n_pos / positions of them hold the sentinel key
                r["sorting_sentinels_share_of_kernel_time"] = round(sort_us / max(sort_us + code, 1e-9) * (1 - n_pos[w] / max(pc, 1)), 4)
        out["w%d" % w] = r
    if want_trace:
        out["plain"]["kernels"] = traces[0]
    return name, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--k", default="11,14")
    ap.add_argument("--log2", default="24,28,31")
    ap.add_argument("--repeat", action="store_true", help="the repeat-heavy reference instead of the random ones")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--w", default="", help="minimizer windows, e.g. 5,10,19: compare aim_index_build_device_minimizers with the plain build")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out-dir", default=os.path.join(ROOT, "profiles", "index"))
    a = ap.parse_args()
    ks, logs = [int(x) for x in a.k.split(",")], [int(x) for x in a.log2.split(",")]
    ws = [int(x) for x in a.w.split(",")] if a.w else []
    if a.child:
        return child(ks[0], logs[0], a.repeat, ws)
    os.makedirs(a.out_dir, exist_ok=True)
    for k in ks:
        for lg in ([0] if a.repeat else logs):
            if ws:
                name, out = row_minimizers(k, lg, a.repeat, max(a.rounds, 5), ws, not a.no_trace)
            else:
                name, out = row(k, lg, a.repeat, max(a.rounds, 5), not a.no_trace)
            print(json.dumps(out), flush=True)
            with open(os.path.join(a.out_dir, "index_rate_%s_k%d%s.json" % (name, k, "_minimizers" if ws else "")), "w") as f:
                json.dump(out, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
