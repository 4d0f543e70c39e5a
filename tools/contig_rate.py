#!/usr/bin/env python3
"""What references of several sequences cost on the MI355X (rule 13c of include/aim_hip.h).

  python tools/contig_rate.py [--parts clip,mapper] [--steps 7] [--warmup 2] [--rounds 5] [--parent-lib build_ab/lib_parent.so] [--out FILE.jsonl]

clip    contig_clip_kernel (aim_contig_clip_device) next to split_segments_kernel on the same batch: 1 Mi reads of l = 100 in rows of 104
        and 64 Ki reads of l = 1 000 in rows of 1 024 at K = 4 (tools/split_rate.py's batches, one primary per read), at 1, 25 and 2^20
        contigs of equal length laid out over the batch's positions. One call between two HIP events, the median of `steps` calls with its
        range; the segment buffers are put back to the split's output before every timed call, outside the events, so that every call
        clips what the first one clipped. Algorithmic bytes: 12 B per slot (aim_segment_t in, d_contig out), 44 B more per valid slot
        (both text_pos, both text_len, the chain's last two fields, read_len, the contig's start and length), 16 B per clipped slot. The first 64
        reads are checked against tests/contig_model.py.
mapper  Mapper.from_contigs on three contigs against the one-sequence engine.Mapper of --parent-lib (a build of the parent commit) on
        their concatenation: tools/mapper_rate.py's two shapes without split reads, each side in a child process of its own (a process
        loads one library), the two alternating over `rounds` rounds; medians and ranges of reads/s.
One JSON line per row."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

N_CONTIGS = (1, 25, 1 << 20)
SPACER = 16


def equal_contigs(n_contigs, ref_len):
    """n contigs of equal length with SPACER between them, covering at least [0, ref_len)."""
    import contig_model as cg
    each = max(-(-ref_len // n_contigs) - SPACER, 1) if n_contigs > 1 else ref_len
    lens = np.full(n_contigs, each, dtype=np.uint32)
    starts, total = cg.layout(lens, SPACER)
    return lens, starts, total


def clip_part(a, row):
    import torch
    import contig_model as cg
    import seed_rate
    import split_model as sm
    import split_rate
    from aim_amd import capi, engine
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    K, FLANK, REF_LEN = split_rate.K, split_rate.FLANK, split_rate.REF_LEN
    up = lambda x, slack=0: torch.cat([torch.from_numpy(np.ascontiguousarray(x).view(np.uint8).reshape(-1)).to(dev), torch.zeros(slack, dtype=torch.uint8, device=dev)])
    names = capi.load().aim_contig_kernel_names().decode().split(",")
    for l, rs, n in split_rate.ROWS[:2]:
        d = split_rate.batch(l, rs, n, False)
        t = {k: up(v, 64 if k == "reads" else 0) for k, v in d.items()}
        S = n * K
        o_req, o_tp, o_seg = (torch.zeros(S * b, dtype=torch.uint8, device=dev) for b in (16, 8, 8))
        o_pat = torch.zeros(S * rs + 64, dtype=torch.uint8, device=dev)
        split = lambda: engine.split_segments_device(K, rs, FLANK, REF_LEN, n, t["read_len"].data_ptr(), t["reads"].data_ptr(), t["req"].data_ptr(),
                                                     t["text_pos"].data_ptr(), t["seed"].data_ptr(), t["chains"].data_ptr(), t["cls"].data_ptr(),
                                                     o_req.data_ptr(), o_tp.data_ptr(), o_pat.data_ptr(), o_seg.data_ptr(), stream)
        ms, lo, hi = seed_rate.events_ms(torch, split, a.steps, a.warmup)
        need = n * (rs + K * rs + K * 80 + 20)
        row(part="clip", kernel="split_segments_kernel", l=l, read_size=rs, reads=n, K=K, ms=round(ms, 4), ms_min=round(lo, 4), ms_max=round(hi, 4),
            algorithmic_bytes=need, share_of_8tb_per_s=round(need / ms / 1e6 / 8000, 4))
        keep = (o_req.clone(), o_tp.clone(), o_seg.clone())
        d_ct = torch.zeros(S * 4, dtype=torch.uint8, device=dev)
        m = 64
        h_split = [x[:m * K * b].cpu().numpy() for x, b in zip(keep, (16, 8, 8))]
        for nc in N_CONTIGS:
            lens, starts, total = equal_contigs(nc, REF_LEN)
            d_st, d_ln = up(starts), up(lens)
            call = lambda: engine.contig_clip_device(K, rs, FLANK, total, nc, d_st.data_ptr(), d_ln.data_ptr(), n, t["read_len"].data_ptr(), t["req"].data_ptr(),
                                                     t["text_pos"].data_ptr(), t["chains"].data_ptr(), o_req.data_ptr(), o_tp.data_ptr(), o_seg.data_ptr(),
                                                     d_ct.data_ptr(), stream)
            times = []
            for i in range(a.warmup + a.steps):
                for dst, src in zip((o_req, o_tp, o_seg), keep):
                    dst.copy_(src)
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                call()
                e1.record()
                torch.cuda.synchronize()
                if i >= a.warmup:
                    times.append(e0.elapsed_time(e1))
            ms = float(np.median(times))
            seg = o_seg.cpu().numpy().view(capi.SEGMENT_DTYPE)
            valid, clipped = int((seg["flags"] & capi.SEG_VALID != 0).sum()), int((seg["flags"] & capi.SEG_CONTIG_CLIPPED != 0).sum())
            want = cg.clip(K, rs, FLANK, total, starts, lens, d["read_len"][:m], d["req"][:m * K], d["text_pos"][:m * K], d["chains"][:m * K],
                           h_split[0].view(capi.REQUEST_DTYPE), h_split[1].view(np.uint64), h_split[2].view(sm.SEGMENT))
            got = (o_req[:m * K * 16].cpu().numpy(), o_tp[:m * K * 8].cpu().numpy(), o_seg[:m * K * 8].cpu().numpy(), d_ct[:m * K * 4].cpu().numpy())
            for g, w in zip(got, (want["seg_req"], want["seg_text_pos"], want["seg"], want["contig"])):
                assert g.tobytes() == w.tobytes(), "the rows are not the model's"
            need = 12 * S + 44 * valid + 16 * clipped
            row(part="clip", kernel=names[0], l=l, read_size=rs, reads=n, K=K, n_contigs=nc, step=1 << max(0, (nc - 1).bit_length() - 10), valid_slots=valid,
                clipped_slots=clipped, ms=round(ms, 4), ms_min=round(min(times), 4), ms_max=round(max(times), 4), algorithmic_bytes=need,
                share_of_8tb_per_s=round(need / ms / 1e6 / 8000, 5))
        del t, o_req, o_tp, o_seg, o_pat, keep
        torch.cuda.empty_cache()


MAPPER_CHILD = '''
import json, sys, time
import numpy as np
sys.path.insert(0, %(root)r); sys.path.insert(0, %(root)r + "/tools"); sys.path.insert(0, %(root)r + "/tests")
import torch
torch.cuda.init()
from aim_amd import capi
capi.load(strict=False)   # (the parent's library lacks rule 13c's symbols)
import mapper_rate as mr
import contig_model as cg
from aim_amd import engine
contigs, si, batches_n = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
l, rs, n, (k, w, max_occ, band, flank, min_votes), max_score = mr.SHAPES[si]
rng = np.random.default_rng(1)
ref = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=mr.REF_LEN)]
cuts = (mr.REF_LEN // 3, 2 * mr.REF_LEN // 3)
seqs = [ref[:cuts[0]], ref[cuts[0]:cuts[1]], ref[cuts[1]:]]
sp = engine.seed_params(k, rs, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, max_cands=mr.K, w=w)
mp = engine.mapper_params(sp, n, max_score, mismatch=mr.X, gap_o=mr.O, gap_e=mr.E, extend=engine.extend_params(), slots=2)
batches = mr.make_batches(ref, l, rs, n, 0.0, batches_n)
m = engine.Mapper.from_contigs(mp, seqs) if contigs else engine.Mapper(mp, cg.concat(seqs, cg.spacer_for(band)))
with m:
    mr.mapper_round(m, batches[:2])
    s, d2h, recs = mr.mapper_round(m, batches)
print(json.dumps({"reads_per_s": batches_n * n / s, "records": recs, "d2h_bytes": d2h}))
'''


def mapper_part(a, row):
    import mapper_rate as mr
    for si in (0, 1):
        rates = {"contigs": [], "parent": []}
        recs = {}
        for rnd in range(a.rounds):
            for side in ("contigs", "parent"):
                env = dict(os.environ)
                if side == "parent":
                    env["AIM_LIB"] = os.path.abspath(a.parent_lib)
                else:
                    env.pop("AIM_LIB", None)
                p = subprocess.run([sys.executable, "-c", MAPPER_CHILD % {"root": ROOT}, "1" if side == "contigs" else "0", str(si), str(a.batches)], env=env,
                                   capture_output=True, text=True, timeout=600)
                if p.returncode:
                    raise SystemExit(p.stdout + p.stderr)
                r = json.loads(p.stdout.strip().splitlines()[-1])
                rates[side].append(r["reads_per_s"])
                recs[side] = r["records"]
        l, rs, n = mr.SHAPES[si][:3]
        med = lambda xs: float(np.median(xs))
        row(part="mapper", l=l, read_size=rs, reads_per_batch=n, batches=a.batches, rounds=a.rounds, n_contigs=3, records=recs,
            contigs_reads_per_s=med(rates["contigs"]), contigs_range=[min(rates["contigs"]), max(rates["contigs"])],
            parent_reads_per_s=med(rates["parent"]), parent_range=[min(rates["parent"]), max(rates["parent"])], ratio=med(rates["contigs"]) / med(rates["parent"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="clip,mapper")
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--parent-lib", default=os.path.join(ROOT, "build_ab", "lib_parent.so"))
    ap.add_argument("--out")
    a = ap.parse_args()
    out = []

    def row(**kw):
        out.append(dict(tool="contig_rate", **kw))
        print(json.dumps(out[-1]), flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(out[-1]) + "\n")
    if "mapper" in a.parts:       # (first: its children open the device themselves, before this process does)
        mapper_part(a, row)
    if "clip" in a.parts:
        import torch
        torch.cuda.init()   # (before the library: the device buffers are torch's)
        clip_part(a, row)


if __name__ == "__main__":
    main()
