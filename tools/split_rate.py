#!/usr/bin/env python3
"""What splitting costs on the MI355X: split_segments_kernel (aim_split_segments_device) next to the AIM_FLAG_REF_TEXTS gather pass, the
project's other row gather, and next to the chaining it follows; aim_sam_device_split next to aim_sam_device on the same rows.

  python tools/split_rate.py [--parts split,gather,chain,sam] [--steps 7] [--warmup 2] [--out FILE.jsonl]

split   1 Mi reads of l = 100 in rows of 104, 64 Ki reads of l = 1 000 and 4 Ki reads of l = 10 000, all at K = 4, each twice: every read
        with one primary (candidate 0 over the whole read; the other slots empty) and every read with two primaries (two halves on
        alternating strands). One call between two HIP events, the median of `steps` calls after a warm-up, with its range. Algorithmic
        bytes: the read row once and K segment rows (read_size each), 48 B in and 32 B out per slot, 20 B per read. The first 64 reads
        of every batch are checked against tests/split_model.py.
gather  tools/ref_texts_rate.py's gather rows, in the same process: the same roofline share for the pass that builds text rows.
chain   seed_chain_minimizer_kernel on 1 Mi reads of l = 100 (tools/chain_rate.py's reads and parameters), the classification and the
        split of exactly those chains: the split as a fraction of the chaining.
sam     aim_align_device_ref over the segment rows of 256 Ki of those reads, then aim_sam_device and aim_sam_device_split on the rows,
        alternating over five rounds; once with the real segments (single primaries: no clip) and once with segments that clip five
        bases at both ends of every row (two more CIGAR words per record).
One JSON line per row."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

K, FLANK, REF_LEN = 4, 16, 1 << 26
ROWS = ((100, 104, 1 << 20), (1000, 1024, 1 << 16), (10000, 10008, 1 << 12))


def batch(l, rs, n, two, seed=5):
    """Chain-kernel outputs and classes for n reads of l bases in rows of rs, built with numpy: one primary per read, or two halves
    (six bases apart, the second on the other strand in every odd read)."""
    import chain_class_model as ccm
    import chain_model as cm
    import seed_model as m
    rng = np.random.default_rng([seed, l, int(two)])
    reads = np.zeros((n, rs), dtype=np.uint8)
    reads[:, :l] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=(n, l), dtype=np.uint8)]
    chains, cls = np.zeros((n, K), dtype=cm.CHAIN), np.zeros((n, K), dtype=ccm.CLASS)
    req, tpos = np.zeros((n, K), dtype=m.REQUEST), np.zeros((n, K), dtype=np.uint64)
    seeds = np.zeros(n, dtype=m.SEED)
    seeds["n_cands"] = 2 if two else 1
    req["pattern_len"] = l
    req["idx"] = np.arange(n * K, dtype=np.uint32).reshape(n, K)
    half = l // 2
    spans = ((0, half - 3), (half + 3, l)) if two else ((0, l),)
    for i, (lo, hi) in enumerate(spans):
        minus = (np.arange(n) & 1).astype(np.uint64) if i else np.zeros(n, dtype=np.uint64)
        q_lo = np.where(minus != 0, l - hi, lo)                    # chain-query coordinates of the read interval [lo, hi)
        p_lo = rng.integers(2 * rs, REF_LEN - 2 * rs, size=n)
        chains["score"][:, i], chains["n_anchors"][:, i] = 10 * (hi - lo) - i, 12
        chains["q_lo"][:, i], chains["q_hi"][:, i], chains["ref_span"][:, i] = q_lo, q_lo + (hi - lo), hi - lo
        start = p_lo - q_lo - FLANK
        req["text_len"][:, i] = np.minimum(l + 2 * FLANK, rs)
        tpos[:, i] = start.astype(np.uint64) | (minus << np.uint64(63))
        cls["parent"][:, i], cls["flags"][:, i], cls["mapq"][:, i] = i, ccm.PRIMARY | (ccm.SUPPLEMENTARY if i else 0), 60
    return dict(read_len=np.full(n, l, dtype=np.int32), reads=reads, req=req.reshape(-1), text_pos=tpos.reshape(-1), seed=seeds,
                chains=chains.reshape(-1), cls=cls.reshape(-1))


def main():
    import torch
    torch.cuda.init()   # (before the library: the device buffers are torch's)
    import seed_rate
    import split_model as sm
    from aim_amd import capi, engine
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="split,gather,chain,sam")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    lib = capi.load()
    names = lib.aim_split_kernel_names().decode().split(",")
    up = lambda x, slack=0: torch.cat([torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev), torch.zeros(slack, dtype=torch.uint8, device=dev)])
    out = []

    def row(**kw):
        out.append(dict(tool="split_rate", lib=os.path.basename(capi.LIB_PATH), steps=a.steps, **kw))
        print(json.dumps(out[-1]), flush=True)

    def timed(call, need=None):
        ms, lo, hi = seed_rate.events_ms(torch, call, a.steps, a.warmup)
        r = dict(ms=round(ms, 4), ms_min=round(lo, 4), ms_max=round(hi, 4))
        if need is not None:
            r.update(algorithmic_bytes=need, share_of_8tb_per_s=round(need / ms / 1e6 / 8000, 4))
        return r

    def split_bytes(n, rs):
        return n * (rs + K * rs + K * 80 + 20)

    if "split" in a.parts:
        for l, rs, n in ROWS:
            for two in (False, True):
                d = batch(l, rs, n, two)
                t = {k: up(v, 64 if k == "reads" else 0) for k, v in d.items()}
                o_req, o_tp, o_seg = (torch.full((n * K * b,), 0xEE, dtype=torch.uint8, device=dev) for b in (16, 8, 8))
                o_pat = torch.full((n * K * rs + 64,), 0xEE, dtype=torch.uint8, device=dev)
                call = lambda: engine.split_segments_device(K, rs, FLANK, REF_LEN, n, t["read_len"].data_ptr(), t["reads"].data_ptr(), t["req"].data_ptr(),
                                                            t["text_pos"].data_ptr(), t["seed"].data_ptr(), t["chains"].data_ptr(), t["cls"].data_ptr(),
                                                            o_req.data_ptr(), o_tp.data_ptr(), o_pat.data_ptr(), o_seg.data_ptr(), stream)
                r = timed(call, split_bytes(n, rs))
                m = 64
                want = sm.segments(K, rs, FLANK, REF_LEN, d["read_len"][:m], d["reads"][:m], d["req"][:m * K], d["text_pos"][:m * K], d["seed"][:m],
                                   d["chains"][:m * K], d["cls"][:m * K])
                got = (o_req[:m * K * 16].cpu().numpy(), o_tp[:m * K * 8].cpu().numpy(), o_pat[:m * K * rs].cpu().numpy(), o_seg[:m * K * 8].cpu().numpy())
                assert all(g.tobytes() == w.tobytes() for g, w in zip(got, want)), "the rows are not the model's"
                row(part="split", kernel=names[0], l=l, read_size=rs, reads=n, K=K, primaries_per_read=2 if two else 1, ns_per_read=round(r["ms"] * 1e6 / n, 3), **r)
                del t, o_req, o_tp, o_seg, o_pat
                torch.cuda.empty_cache()
    if "gather" in a.parts:
        import ref_texts_rate
        for g in ref_texts_rate.gather_rows(a.steps, a.warmup):     # (gather_rows prints each row itself)
            out.append(dict(tool="split_rate", **g))
        torch.cuda.empty_cache()
    if "chain" in a.parts or "sam" in a.parts:
        import chain_rate
        k, w, L, rs, n = 11, 10, 100, 128, 1 << 20
        ref = seed_rate.reference()
        rows, rl, _ = chain_rate.make_reads(ref, n, L, rs)
        sp = engine.seed_params(k, rs, band=8, w=w, **chain_rate.KW)
        index = tuple(torch.from_numpy(x.view(np.uint8)).to(dev) for x in engine.index_build_minimizers(ref, k, w, threads=16))
        o = engine.split_segments(sp, engine.chain_classify(sp, engine.seed_chain_candidates(sp, index, len(ref), rl, rows)), len(ref))
        ptr = lambda *keys: [o[x].data_ptr() for x in keys]
        Kc = chain_rate.K
        if "chain" in a.parts:
            chain = timed(lambda: engine.seed_chain_device(sp, n, *ptr("d_read_len", "d_reads", "d_bucket", "d_pos"), len(ref),
                                                           *ptr("d_req", "d_text_pos", "d_votes", "d_seed", "d_chains"), stream))
            row(part="chain", kernel=lib.aim_seed_chain_kernel_names().decode().split(",")[1], l=L, read_size=rs, reads=n, K=Kc, k=k, w=w, **chain)
            cls = timed(lambda: engine.chain_classify_device(Kc, rs, capi.CHAIN_MASK_DEFAULT, n, *ptr("d_read_len", "d_text_pos", "d_seed", "d_chains", "d_class"), stream))
            row(part="chain", kernel="chain_class_kernel", on="the chains of the row above", reads=n, K=Kc, share_of_chaining=round(cls["ms"] / chain["ms"], 5), **cls)
            sp_t = timed(lambda: engine.split_segments_device(Kc, rs, sp.flank, len(ref), n, *ptr("d_read_len", "d_reads", "d_req", "d_text_pos", "d_seed", "d_chains",
                                                                                                "d_class", "d_seg_req", "d_seg_text_pos", "d_seg_patterns", "d_seg"), stream),
                         n * (rs + Kc * rs + Kc * 80 + 20))
            fl = o["seg"]["flags"]
            row(part="chain", kernel=names[0], on="the chains of the row above", reads=n, K=Kc, read_size=rs, share_of_chaining=round(sp_t["ms"] / chain["ms"], 5),
                segments=int((fl != 0).sum()), supplementary=int((fl & capi.SEG_SUPPLEMENTARY != 0).sum()), **sp_t)
        if "sam" in a.parts:
            n2 = 1 << 18
            rows_n = n2 * Kc
            x, g_o, g_e = 3, 4, 1
            params = engine.make_params("wfa", 40, rs, mismatch=x, gap_o=g_o, gap_e=g_e, backtrace=True, ref_texts=True, ends_free=(0, 0, 2 * sp.flank, 2 * sp.flank))
            d_ref = torch.zeros(len(ref) + 64, dtype=torch.uint8, device=dev)
            d_ref[:len(ref)] = torch.from_numpy(ref).to(dev)
            d_res = torch.zeros(rows_n * capi.RESULT_DTYPE.itemsize, dtype=torch.uint8, device=dev)
            d_ops = torch.zeros(rows_n * 2 * rs + 64, dtype=torch.uint8, device=dev)
            sb = lib.aim_scratch_bytes(capi.params_ref(params), rows_n)
            d_scr = torch.zeros(max(sb, 16), dtype=torch.uint8, device=dev)
            capi.check(lib.aim_align_device_ref(capi.params_ref(params), rows_n, *ptr("d_seg_req", "d_seg_patterns", "d_seg_text_pos"), d_ref.data_ptr(), len(ref),
                                                d_res.data_ptr(), d_ops.data_ptr(), d_scr.data_ptr(), sb, stream))
            ccap, mcap = rows_n * 8, rows_n * 16
            d_sam = torch.zeros(rows_n * 48, dtype=torch.uint8, device=dev)
            d_cg, d_md, d_cur = torch.zeros(ccap * 4, dtype=torch.uint8, device=dev), torch.zeros(mcap, dtype=torch.uint8, device=dev), torch.zeros(8, dtype=torch.uint8, device=dev)
            clipped = o["seg"][:rows_n].copy()                    # five bases off both ends of every segment: two more words per record
            live = clipped["flags"] != 0
            clipped["q_begin"][live] += 5
            clipped["q_end"][live] -= 5
            d_clip = up(clipped)
            common = (params, rows_n, o["d_seg_req"].data_ptr(), o["d_seg_text_pos"].data_ptr(), None, d_res.data_ptr(), d_ops.data_ptr(), d_ref.data_ptr(), len(ref), 0,
                      d_sam.data_ptr(), d_cg.data_ptr(), ccap, d_md.data_ptr(), mcap, d_cur.data_ptr())
            calls = {"aim_sam_device": lambda: engine.sam_device(*common, stream),
                     "aim_sam_device_split": lambda: engine.sam_device_split(*common, o["d_seg"].data_ptr(), stream),
                     "aim_sam_device_split, 5 + 5 bases clipped": lambda: engine.sam_device_split(*common, d_clip.data_ptr(), stream)}
            for rnd in range(5):
                for name, call in calls.items():
                    r = timed(call)
                    cur = d_cur.cpu().numpy().view(np.uint32)
                    sam = d_sam.cpu().numpy().view(capi.SAM_DTYPE)
                    plain = engine.sam_kernel_name(params)
                    kernel = plain if name == "aim_sam_device" else plain.replace("_kernel", "_split_kernel")
                    row(part="sam", round=rnd, call=name, kernel=kernel, rows=rows_n, read_size=rs, mapped=int((sam["flags"] & 4 == 0).sum()),
                        cigar_words=int(cur[0]), md_bytes=int(cur[1]), **r)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            for r in out:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
