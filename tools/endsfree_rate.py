#!/usr/bin/env python3
"""Ends-free WFA rates (AIM_FLAG_ENDSFREE): aim_align_device over HBM-resident batches, timed with HIP events like bench.py.

  python tools/endsfree_rate.py [--pairs N] [--steps K] [--warmup W] [--out FILE.jsonl]

Rows: the overhead check and the flanked rates (gen_dataset --flank F inputs, TB = TE = F). One JSON line per row.
The overhead check times ends-free with zero free lengths against global WFA forced onto the same kernel: AIM_NO_LANE=1
AIM_NO_LANE_PK=1 for the whole process (both run on wfa_group_kernel), and once more with AIM_FORCE_WAVE=1 (both on
wfa_wave_kernel)."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

os.environ.setdefault("AIM_NO_LANE", "1")        # the global rows run on the general kernel, like the ends-free ones
os.environ.setdefault("AIM_NO_LANE_PK", "1")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np   # noqa: E402
import torch         # noqa: E402

from aim_amd import capi, engine   # noqa: E402


def rate(params, req, pat, txt, steps, warmup):
    lib = capi.load()
    dev = torch.device("cuda", 0)
    n, rs = len(req), params.read_size

    def to_dev(a, pad=64):
        t = torch.zeros(a.nbytes + pad, dtype=torch.uint8, device=dev)
        t[: a.nbytes].copy_(torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)))
        return t

    d_req, d_pat, d_txt = to_dev(req), to_dev(pat), to_dev(txt)
    d_res = torch.zeros(n * 24 + 64, dtype=torch.uint8, device=dev)
    bt = bool(params.flags & capi.FLAG_BACKTRACE)
    d_ops = torch.zeros(n * 2 * rs + 64, dtype=torch.uint8, device=dev) if bt else None
    pr = capi.params_ref(params)
    sb = lib.aim_scratch_bytes(pr, n)
    assert sb > 0, lib.aim_last_error()
    d_scr = torch.zeros(sb, dtype=torch.uint8, device=dev)
    st = torch.cuda.current_stream(dev)

    def step():
        capi.check(lib.aim_align_device(pr, n, d_req.data_ptr(), d_pat.data_ptr(), d_txt.data_ptr(), d_res.data_ptr(),
                                        d_ops.data_ptr() if bt else None, d_scr.data_ptr(), sb, st.cuda_stream))

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step()
    b.record()
    torch.cuda.synchronize()
    ms = a.elapsed_time(b) / steps
    buf = C.create_string_buffer(512)
    lib.aim_plan_describe(pr, n, buf, len(buf))
    return ms, n / (ms * 1e-3), buf.value.decode()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the commit the rows are measured on (default: git rev-parse --short HEAD)")
    a = ap.parse_args()
    commit = a.commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    rows = []
    for l, err, bt in ((100, 0.01, False), (100, 0.01, True), (1000, 0.05, True)):
        ms, rs = engine.launcher_sizes("wfa", l, err)
        n = a.pairs if l < 1000 else a.pairs // 8
        req, pat, txt = engine.gen_pairs(42, 0, n, l, err, rs)
        glob = engine.make_params("wfa", ms, rs, backtrace=bt)
        ef0 = engine.make_params("wfa", ms, rs, backtrace=bt, ends_free=(0, 0, 0, 0))
        g = rate(glob, req, pat, txt, a.steps, a.warmup)
        z = rate(ef0, req, pat, txt, a.steps, a.warmup)
        os.environ["AIM_FORCE_WAVE"] = "1"   # (the stateless entry points read the AIM_* switches at every call)
        w = rate(glob, req, pat, txt, a.steps, a.warmup)
        zw = rate(ef0, req, pat, txt, a.steps, a.warmup)
        del os.environ["AIM_FORCE_WAVE"]
        rows.append({"row": "overhead", "l": l, "e": err, "cigar": bt, "pairs": n, "global_ms": g[0], "endsfree0_ms": z[0],
                     "slowdown": z[0] / g[0] - 1.0, "global_wave_ms": w[0], "endsfree0_wave_ms": zw[0],
                     "slowdown_wave": zw[0] / w[0] - 1.0, "global_plan": g[2], "endsfree_plan": z[2]})
    for l, err, flank, bt in ((100, 0.01, 16, False), (100, 0.01, 16, True), (1000, 0.05, 50, True)):
        ms, rs = engine.launcher_sizes("wfa", l, err)
        n = a.pairs if l < 1000 else a.pairs // 8
        req, pat, txt = engine.gen_pairs(42, 0, n, l, err, rs)
        req, pat, txt = engine.flank_pairs(42, 0, req, pat, txt, flank)
        t = rate(engine.make_params("wfa", ms, pat.shape[1], backtrace=bt, ends_free=(0, 0, flank, flank)), req, pat, txt,
                 a.steps, a.warmup)
        rows.append({"row": "flanked", "l": l, "e": err, "flank": flank, "cigar": bt, "pairs": n, "ms": t[0], "pairs_per_s": t[1],
                     "plan": t[2]})
    with (open(a.out, "w") if a.out else sys.stdout) as f:
        for r in rows:
            r["commit"] = commit
            f.write(json.dumps(r) + "\n")
    if a.out:
        for r in rows:
            print(json.dumps(r))


if __name__ == "__main__":
    main()
