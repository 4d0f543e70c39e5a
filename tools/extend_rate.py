#!/usr/bin/env python3
"""What extending split-read segments costs on the MI355X: aim_extend_segments_device (extend_sides_kernel, then extend_apply_kernel)
next to split_segments_kernel, which it follows, and to aim_align_device_ref over the same segment rows, which follows it.

  python tools/extend_rate.py [--steps 7] [--warmup 2] [--out FILE.jsonl] [--shapes 0,1] [--fractions 0,0.1,1] [--no-align]

Shapes: 1 Mi reads of l = 100 in rows of 104 and 64 Ki reads of l = 1 000 in rows of 1 024 at K = 4, each with 0 %, 10 % and 100 % of
the reads split. A read is a window of a random reference; a split read is two windows, the second on the minus strand in every odd
read, and its two chains stop 5 bases short of the junction, so that each inner side has 5 bases to recover before the other half's
bases begin. The segments come from aim_split_segments_device on the device. The extension rewrites them in place, so every timed call
is preceded by a device copy that puts the split outputs back (outside the two HIP events); the median of `steps` calls after a
warm-up, with its range. The entry point launches both kernels between the same two events: the per-kernel times come from a
kernel-trace run of this tool (profiles/extend/README.md), not from here. The first 64 reads of every batch are checked against
tests/extend_model.py. Algorithmic bytes of the extension: per slot the 8-byte segment record read twice and 24 B of aim_extend_t
written and read; per side run 28 B of records and the n + m staged bases; per touched slot 32 B of records read and written and a
pattern row of read_size written with its bytes read. One JSON line per row."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, FLANK, SHORT = 4, 16, 5
SHAPES = ((100, 104, 1 << 20), (1000, 1024, 1 << 16))
FRACTIONS = (0.0, 0.1, 1.0)


def batch(ref, l, rs, n, fraction, seed=5):
    """Chain-kernel outputs and classes for n reads of l bases in rows of rs, `fraction` of them split in two halves."""
    import chain_class_model as ccm
    import chain_model as cm
    import seed_model as m
    rng = np.random.default_rng([seed, l, int(fraction * 100)])
    comp = np.arange(256, dtype=np.uint8)
    for a, b in (b"AT", b"TA", b"CG", b"GC"):
        comp[a] = b
    half = l // 2
    two = rng.random(n) < fraction
    minus2 = two & ((np.arange(n) & 1) != 0)
    pA = rng.integers(4 * rs, len(ref) - 4 * rs, size=n)
    pB = rng.integers(4 * rs, len(ref) - 4 * rs, size=n)
    reads = np.zeros((n, rs), dtype=np.uint8)
    for lo in range(0, n, 1 << 16):
        sl = slice(lo, min(lo + (1 << 16), n))
        reads[sl, :l] = ref[pA[sl, None] + np.arange(l)[None, :]]
        second = ref[pB[sl, None] + np.arange(l - half)[None, :]]
        second = np.where(minus2[sl, None], comp[second[:, ::-1]], second)
        reads[sl, half:l] = np.where(two[sl, None], second, reads[sl, half:l])
    chains, cls = np.zeros((n, K), dtype=cm.CHAIN), np.zeros((n, K), dtype=ccm.CLASS)
    req, tpos = np.zeros((n, K), dtype=m.REQUEST), np.zeros((n, K), dtype=np.uint64)
    seeds = np.zeros(n, dtype=m.SEED)
    seeds["n_cands"] = np.where(two, 2, 1)
    req["pattern_len"] = l
    req["idx"] = np.arange(n * K, dtype=np.uint32).reshape(n, K)
    # candidate 0: the whole read, or its first half less SHORT bases; candidate 1 of a split read: the second half less SHORT bases
    q_lo0, q_hi0 = np.zeros(n, dtype=np.int64), np.where(two, half - SHORT, l)
    q_lo1 = np.where(minus2, 0, half + SHORT)                         # chain-query coordinates: a minus chain counts from the read's end
    q_hi1 = np.where(minus2, l - half - SHORT, l)
    p_lo1 = np.where(minus2, pB, pB + SHORT)
    for i, (q_lo, q_hi, p_lo, minus, on) in enumerate(((q_lo0, q_hi0, pA, np.zeros(n, dtype=bool), np.ones(n, dtype=bool)), (q_lo1, q_hi1, p_lo1, minus2, two))):
        span = q_hi - q_lo
        start = p_lo - q_lo - FLANK
        tl = np.minimum(span + q_lo + (l - q_hi) + 2 * FLANK, rs)
        chains["score"][:, i], chains["n_anchors"][:, i] = np.where(on, 10 * span - i, 0), np.where(on, 12, 0)
        chains["q_lo"][:, i], chains["q_hi"][:, i], chains["ref_span"][:, i] = np.where(on, q_lo, 0), np.where(on, q_hi, 0), np.where(on, span, 0)
        req["text_len"][:, i] = np.where(on, tl, 0)
        tpos[:, i] = np.where(on, start.astype(np.uint64) | (minus.astype(np.uint64) << np.uint64(63)), 0)
        cls["parent"][:, i], cls["flags"][:, i], cls["mapq"][:, i] = i, np.where(on, ccm.PRIMARY | (ccm.SUPPLEMENTARY if i else 0), 0), np.where(on, 60, 0)
    return dict(read_len=np.full(n, l, dtype=np.int32), reads=reads, req=req.reshape(-1), text_pos=tpos.reshape(-1), seed=seeds,
                chains=chains.reshape(-1), cls=cls.reshape(-1)), int(two.sum())


def main():
    import torch
    torch.cuda.init()   # (before the library: the device buffers are torch's)
    import extend_model as em
    import seed_rate
    import split_model as sm
    from aim_amd import capi, engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--fractions", default=",".join(str(f) for f in FRACTIONS))
    ap.add_argument("--no-align", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    lib = capi.load()
    up = lambda x, slack=0: torch.cat([torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev), torch.zeros(slack, dtype=torch.uint8, device=dev)])
    out = []

    def row(**kw):
        out.append(dict(tool="extend_rate", lib=os.path.basename(capi.LIB_PATH), steps=a.steps, **kw))
        print(json.dumps(out[-1]), flush=True)

    def timed(call, before=None):
        import statistics
        times = []
        for i in range(a.warmup + a.steps):
            if before is not None:
                before()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                times.append(e0.elapsed_time(e1))
        return dict(ms=round(statistics.median(times), 4), ms_min=round(min(times), 4), ms_max=round(max(times), 4))

    ref = seed_rate.reference()
    d_ref = up(ref, 64)
    p = em.Params(1, 3, 4, 1, 20, 400, 31, 64)
    ep = engine.extend_params(*p)
    x, g_o, g_e = 3, 4, 1
    for si in (int(s) for s in a.shapes.split(",")):
        l, rs, n = SHAPES[si]
        for fraction in (float(f) for f in a.fractions.split(",")):
            d, n_split = batch(ref, l, rs, n, fraction)
            t = {k: up(v, 64 if k == "reads" else 0) for k, v in d.items()}
            slots = n * K
            o_req, o_tp, o_seg = (torch.full((slots * b,), 0xEE, dtype=torch.uint8, device=dev) for b in (16, 8, 8))
            o_pat = torch.full((slots * rs + 64,), 0xEE, dtype=torch.uint8, device=dev)
            o_ext = torch.full((slots * 24,), 0xEE, dtype=torch.uint8, device=dev)
            split = lambda: engine.split_segments_device(K, rs, FLANK, len(ref), n, t["read_len"].data_ptr(), t["reads"].data_ptr(), t["req"].data_ptr(),
                                                         t["text_pos"].data_ptr(), t["seed"].data_ptr(), t["chains"].data_ptr(), t["cls"].data_ptr(),
                                                         o_req.data_ptr(), o_tp.data_ptr(), o_pat.data_ptr(), o_seg.data_ptr(), stream)
            r_split = timed(split)
            keep = [x_.clone() for x_ in (o_req, o_tp, o_pat, o_seg)]

            def restore():
                for dst, src in zip((o_req, o_tp, o_pat, o_seg), keep):
                    dst.copy_(src)

            extend = lambda: engine.extend_segments_device(ep, K, rs, len(ref), n, t["read_len"].data_ptr(), t["reads"].data_ptr(), d_ref.data_ptr(), o_req.data_ptr(),
                                                           o_tp.data_ptr(), o_pat.data_ptr(), o_seg.data_ptr(), o_ext.data_ptr(), stream)
            r_ext = timed(extend, before=restore)
            # the first 64 reads against the model
            mm = 64
            host = [x_[:mm * K * b].cpu().numpy() for x_, b in zip(keep, (16, 8, rs, 8))]
            want, want_ext = em.extend_segments(p, K, rs, len(ref), d["read_len"][:mm], d["reads"][:mm], ref, host[0].view(capi.REQUEST_DTYPE), host[1].view(np.uint64),
                                                host[2].reshape(mm * K, rs), host[3].view(sm.SEGMENT))
            got = [x_[:mm * K * b].cpu().numpy() for x_, b in zip((o_req, o_tp, o_pat, o_seg, o_ext), (16, 8, rs, 8, 24))]
            assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want + (want_ext,))), "the rows are not the model's"
            ext = o_ext.cpu().numpy().view(capi.EXTEND_DTYPE)
            seg = keep[3].cpu().numpy().view(capi.SEGMENT_DTYPE)
            run = int((ext["stop"] != 0).sum())
            touched = int(((ext["dq"] != 0) | (ext["dr"] != 0)).any(axis=1).sum())
            staged = run * (28 + 2 * min(l // 2, p.max_ext) + p.band)            # (n and m of a side here: half a read, capped by max_ext)
            need = slots * (8 + 8 + 24 + 24) + staged + touched * (64 + rs + l // 2)
            more = dict(l=l, read_size=rs, reads=n, K=K, split_reads=n_split, sides_run=run, slots_touched=touched, recovered_bases=int(ext["dq"].sum()),
                        max_stop=int(ext["stop"].max()))
            row(part="split", kernel="split_segments_kernel", fraction=fraction, **more, **r_split)
            row(part="extend", kernel="extend_sides_kernel+extend_apply_kernel", fraction=fraction, algorithmic_bytes=need,
                share_of_8tb_per_s=round(need / r_ext["ms"] / 1e6 / 8000, 5), share_of_split=round(r_ext["ms"] / r_split["ms"], 4), **more, **r_ext)
            if not a.no_align:
                params = engine.make_params("wfa", 40, rs, mismatch=x, gap_o=g_o, gap_e=g_e, backtrace=True, ref_texts=True, ends_free=(0, 0, 2 * FLANK, 2 * FLANK))
                d_res = torch.zeros(slots * capi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
                d_ops = torch.zeros(slots * 2 * rs + 64, dtype=torch.uint8, device=dev)
                sb = lib.aim_scratch_bytes(capi.params_ref(params), slots)
                d_scr = torch.zeros(max(sb, 16), dtype=torch.uint8, device=dev)
                align = lambda: capi.check(lib.aim_align_device_ref(capi.params_ref(params), slots, o_req.data_ptr(), o_pat.data_ptr(), o_tp.data_ptr(), d_ref.data_ptr(),
                                                                   len(ref), d_res.data_ptr(), d_ops.data_ptr(), d_scr.data_ptr(), sb, stream))
                r_al = timed(align)                                  # (over the extended rows the last extend call left)
                row(part="align", call="aim_align_device_ref", kernel=lib.aim_kernel_name(capi.params_ref(params)).decode(), fraction=fraction,
                    extend_share_of_align=round(r_ext["ms"] / r_al["ms"], 5), **more, **r_al)
                del d_res, d_ops, d_scr
            del t, o_req, o_tp, o_seg, o_pat, o_ext, keep
            torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
