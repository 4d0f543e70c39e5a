#!/usr/bin/env python3
"""AIM_FLAG_WFA_ESCALATE: what a generous MAX_SCORE costs with and without the flag on a batch of mostly clean reads.

  python tools/escalate_rate.py [--steps K] [--warmup W] [--pairs N] [--parent LIB.so] [--out DIR]

Batch: l = 100, penalties (3, 4, 1), MAX_SCORE 25, N pairs (default 4 Mi; 1 Mi with CIGAR), HBM-resident, through aim_align_device.
mixed_pairs with e_clean = 1 %, e_tail = 5 % and tail fraction f in {0, 1, 5, 20, 100 %}. Per f and per output ({idx, score} rows;
result + ops rows): the flag on this library against the flag-less run of --parent (default: this library), each in a child process of
its own, HIP events around `steps` launches after `warmup`. Output "runs" is the compact CIGAR: packed batches through aim_set_submit /
aim_set_wait with `cigars` (1 Mi pairs, host-to-host wall time, transfers included), where the flag-less plan fuses its run output and the
two-stage plan runs cigar_rle_kernel over ops rows. One JSON line per row on stdout and in DIR/escalate_rate.jsonl (default
profiles/escalate/), with the commit the figures were taken on.

  python tools/escalate_rate.py --kernel-stats CSV [--pairs N]
reads the kernel statistics of `rocprofv3 --kernel-trace --stats -- python tools/escalate_rate.py --child --escalate --output score`
and prints the selection kernels' own average times, with the result bytes escalate_select_kernel reads per second against the 8 TB/s
HBM roofline."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBS = 8000.0
L, MS, FRACTIONS = 100, 25, (0.0, 0.01, 0.05, 0.2, 1.0)


def child(args):
    import torch
    torch.cuda.init()
    from aim_amd import capi, engine
    lib = capi.load()
    dev = torch.device("cuda:0")
    rs = engine.launcher_sizes("wfa", L, 0.05)[1]
    bt = args.output == "ops"
    n = args.pairs
    kw = dict(backtrace=True) if bt else dict(res8=True)
    rows = []
    for f in FRACTIONS:
        req, pat, txt, tail = engine.mixed_pairs(1, n, L, 0.01, 0.05, f, rs)
        d_req = torch.from_numpy(req.view(np.uint8).copy()).to(dev)
        d_pat = torch.zeros(n * rs + 64, dtype=torch.uint8, device=dev)
        d_txt = torch.zeros(n * rs + 64, dtype=torch.uint8, device=dev)
        d_pat[: n * rs] = torch.from_numpy(pat.reshape(-1)).to(dev)
        d_txt[: n * rs] = torch.from_numpy(txt.reshape(-1)).to(dev)
        d_res = torch.zeros(n * (24 if bt else 8), dtype=torch.uint8, device=dev)
        d_ops = torch.zeros(n * 2 * rs + 64, dtype=torch.uint8, device=dev) if bt else None
        sides = [("flag" if args.escalate else "flagless", engine.make_params("wfa", MS, rs, escalate=args.escalate, **kw))]
        if args.escalate and f == 0.0:
            sides.append(("lane_cap10", engine.make_params("wfa", 10, rs, **kw)))
        for name, p in sides:
            sb = lib.aim_scratch_bytes(capi.params_ref(p), n)
            d_scr = torch.zeros(sb, dtype=torch.uint8, device=dev)
            stream = torch.cuda.current_stream().cuda_stream
            buf = C.create_string_buffer(1024)
            lib.aim_plan_describe(capi.params_ref(p), n, buf, len(buf))

            def go():
                capi.check(lib.aim_align_device(capi.params_ref(p), n, d_req.data_ptr(), d_pat.data_ptr(), d_txt.data_ptr(), d_res.data_ptr(),
                                                d_ops.data_ptr() if bt else None, d_scr.data_ptr(), sb, stream))
            for _ in range(args.warmup):
                go()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            a.record()
            for _ in range(args.steps):
                go()
            b.record()
            torch.cuda.synchronize()
            ms = a.elapsed_time(b) / args.steps
            score = d_res.cpu().numpy().view(capi.RESULT_DTYPE if bt else capi.RESULT8_DTYPE)["score"]
            rows.append(dict(side=name, output=args.output, f=f, pairs=n, ms=round(ms, 4), pairs_per_s=round(n / ms * 1e3, 1),
                             over_cap10=int((score > 10).sum()), score_sum=int(score.astype(np.int64).sum()), plan=buf.value.decode()))
            print(json.dumps(rows[-1]), flush=True)
            del d_scr
    return 0


def child_runs(args):
    """compact CIGAR through the set API: packed batch in, aim_cigar_t + runs out"""
    import time
    from aim_amd import capi, engine
    rs = engine.launcher_sizes("wfa", L, 0.05)[1]
    n = args.pairs
    params = engine.make_params("wfa", MS, rs, escalate=args.escalate, backtrace=True, req8=True)
    for f in FRACTIONS:
        req, pat, txt, tail = engine.mixed_pairs(1, n, L, 0.01, 0.05, f, rs)
        packed = engine.pack_batch_native(params, req, pat, txt)
        with engine.DeviceSet(1) as s:
            s.configure_slots(params, n, slots=1, max_raw=max(1, len(packed[2])), max_runs=16 * n)
            out = None
            for k in range(args.warmup + args.steps):
                if k == args.warmup:
                    t0 = time.perf_counter()
                s.submit(0, 0, req, packed=packed, cigar_runs_cap=16 * n)
                out = s.wait(0, 0)
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            h2d, kernel, d2h = s.timers()
            plan = s.plan_describe(0)
        score = out["cig"]["score"]
        row = dict(side="flag" if args.escalate else "flagless", output="runs", f=f, pairs=n, ms=round(ms, 4), pairs_per_s=round(n / ms * 1e3, 1),
                   kernel_ms=round(kernel / (args.warmup + args.steps), 4), over_cap10=int((score > 10).sum()), score_sum=int(score.astype(np.int64).sum()),
                   n_runs=int(len(out["runs"])), plan=plan)
        print(json.dumps(row), flush=True)
    return 0


def kernel_stats(path, pairs):
    import csv
    rows = list(csv.DictReader(open(path)))
    for r in rows:
        name = r.get("Name") or r.get("Kernel_Name") or ""
        if "escalate_" not in name:
            continue
        avg_ns = float(r.get("AverageNs") or r.get("Average") or 0)
        out = dict(row="selection_kernel", kernel=name.split("(")[0], calls=int(float(r.get("Calls") or 0)), avg_us=round(avg_ns / 1e3, 2))
        if "select" in name and avg_ns:
            out["result_gbs"] = round(pairs * 8 / avg_ns, 1)          # {idx, score} rows read, bytes per ns = GB/s
            out["roofline_frac"] = round(pairs * 8 / avg_ns / HBM_GBS, 4)
        print(json.dumps(out), flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pairs", type=int, default=0)
    ap.add_argument("--parent", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "escalate"))
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--escalate", action="store_true")
    ap.add_argument("--output", default="score")
    ap.add_argument("--kernel-stats", default="")
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats, args.pairs or (1 << 22))
    if args.child:
        return child_runs(args) if args.output == "runs" else child(args)
    os.makedirs(args.out, exist_ok=True)
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or "unknown (no git metadata)"
    rows = []
    for output, n in (("score", args.pairs or (1 << 22)), ("ops", args.pairs or (1 << 20)), ("runs", args.pairs or (1 << 20))):
        for esc in (True, False):
            env = dict(os.environ)
            if not esc and args.parent:
                env["AIM_LIB"] = os.path.abspath(args.parent)
            cmd = [sys.executable, os.path.abspath(__file__), "--child", "--steps", str(args.steps), "--warmup", str(args.warmup), "--pairs", str(n),
                   "--output", output] + (["--escalate"] if esc else [])
            r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
            if r.returncode:
                print(r.stdout + r.stderr, file=sys.stderr)
                return r.returncode
            rows += [dict(json.loads(x), library="this" if esc or not args.parent else "parent") for x in r.stdout.splitlines() if x.startswith("{")]
    by = {(r["side"], r["output"], r["f"]): r for r in rows}
    summary = []
    for output in ("score", "ops", "runs"):
        for f in FRACTIONS:
            a, b = by[("flag", output, f)], by[("flagless", output, f)]
            summary.append(dict(row="speedup", output=output, f=f, flag_pairs_per_s=a["pairs_per_s"], flagless_pairs_per_s=b["pairs_per_s"],
                                ratio=round(a["pairs_per_s"] / b["pairs_per_s"], 3), results_equal=a["score_sum"] == b["score_sum"]))
        if output == "runs":
            continue
        a, lane = by[("flag", output, 0.0)], by[("lane_cap10", output, 0.0)]
        dt = max(a["ms"] - lane["ms"], 1e-6)
        res_bytes = a["pairs"] * (8 if output == "score" else 24)
        summary.append(dict(row="flag_f0_minus_lane_cap10", output=output, ms=round(dt, 4), result_gbs=round(res_bytes / dt / 1e6, 1),
                            roofline_frac=round(res_bytes / dt / 1e6 / HBM_GBS, 4)))
    with open(os.path.join(args.out, "escalate_rate.jsonl"), "w") as fh:
        for r in [dict(row="meta", commit=commit, steps=args.steps, warmup=args.warmup)] + rows + summary:
            fh.write(json.dumps(r) + "\n")
    for r in summary:
        print(json.dumps(r), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
