#!/usr/bin/env python3
"""Dual-cost gap-affine WFA rates (AIM_FLAG_AFFINE2P): aim_align_device over HBM-resident batches, timed with HIP events like
bench.py.

  python tools/affine2p_rate.py [--pairs N] [--steps K] [--warmup W] [--out FILE.jsonl]

One JSON line per (shape, CIGAR or not): pairs/s and time_ratio (affine2p time / global time) of affine2p (x, o1, e1, o2, e2) = (4, 4, 2, 24, 1) against global WFA with the
same piece 1 on the same kernel -- AIM_NO_LANE=1 AIM_NO_LANE_PK=1 for the whole process, so that global WFA runs on
wfa_group_kernel (or wfa_wave_kernel) like affine2p does. MAX_SCORE is the launchers' rule for piece 1 (a dual-affine cost never
exceeds it). Shapes: l = 100 at e = 1 % and 5 %, l = 1000 at e = 5 % with one 50..100-base indel per pair (gen_dataset
--long-indel 100), l = 10 000 at e = 1 %."""
import argparse
import ctypes as C
import json
import os
import re
import subprocess
import sys
from math import gcd

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


def hist_per_pair(plan):
    """History bytes per pair of a wfa_group plan line with CIGAR (hist= over chunk=); None for other plans."""
    h, c = re.search(r" hist=(\d+)", plan), re.search(r" chunk=(\d+)", plan)
    return int(h.group(1)) / int(c.group(1)) if h and c and int(h.group(1)) else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=1 << 18)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    ap.add_argument("--commit", default=None, help="the commit the rows are measured on (default: git rev-parse --short HEAD)")
    a = ap.parse_args()
    commit = a.commit or subprocess.run(["git", "rev-parse", "--short", "HEAD"], cwd=ROOT, capture_output=True, text=True).stdout.strip() or None
    x, o, e, o2, e2 = 4, 4, 2, 24, 1
    rows = []
    for l, err, indel, div in ((100, 0.01, 0, 1), (100, 0.05, 0, 1), (1000, 0.05, 100, 8), (10000, 0.01, 0, 256)):
        ms, rs = engine.launcher_sizes("wfa", l, err, mismatch=x, gap_o=o, gap_e=e)
        n = max(1024, a.pairs // div)
        req, pat, txt = engine.gen_pairs(42, 0, n, l, err, rs)
        if indel:
            req, pat, txt = engine.long_indel_pairs(42, 0, req, pat, txt, indel)
        rs = pat.shape[1]
        for bt in (False, True):
            glob = engine.make_params("wfa", ms, rs, mismatch=x, gap_o=o, gap_e=e, backtrace=bt)
            dual = engine.make_params("wfa", ms, rs, mismatch=x, gap_o=o, gap_e=e, backtrace=bt, gap2=(o2, e2))
            g = rate(glob, req, pat, txt, a.steps, a.warmup)
            d = rate(dual, req, pat, txt, a.steps, a.warmup)
            rows.append({"l": l, "e": err, "long_indel": indel, "cigar": bt, "pairs": n, "max_score": ms, "penalties": [x, o, e, o2, e2],
                         "global_unit": gcd(gcd(x, o + e), e), "affine2p_unit": gcd(gcd(gcd(gcd(x, o + e), e), o2 + e2), e2),
                         "global_ms": g[0], "global_pairs_per_s": g[1], "affine2p_ms": d[0], "affine2p_pairs_per_s": d[1],
                         "time_ratio": d[0] / g[0],   # affine2p time / global time: 2.0 = twice as slow
                         "global_hist_bytes_per_pair": hist_per_pair(g[2]), "affine2p_hist_bytes_per_pair": hist_per_pair(d[2]),
                         "global_plan": g[2], "affine2p_plan": d[2]})
            print(json.dumps(rows[-1]), file=sys.stderr, flush=True)
    with (open(a.out, "w") if a.out else sys.stdout) as f:
        for r in rows:
            r["commit"] = commit
            f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
