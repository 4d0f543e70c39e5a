#!/usr/bin/env python3
"""What the mapper object buys on the MI355X: aim_mapper_t with two slots against the same stages driven by hand from Python, one
synchronize per batch.

  python tools/mapper_rate.py [--rounds 5] [--batches 6] [--out FILE.jsonl] [--shapes 0,1] [--fractions 0,0.1,1] [--no-extend]

Shapes: batches of 32 Ki reads of l = 100 in rows of 104 and 4 Ki reads of l = 1 000 in rows of 1 024 at K = 4, each with 0 %, 10 % and
100 % of the reads split. A read is a window of a 4 Mi-base random reference with 2 % substitutions; a split read is two windows, the
second on the minus strand in every odd read.

Both sides run in one process, alternating: a round is `batches` batches through the mapper (submit on slots 0 / 1 alternately, each
wait followed by the next submit on that slot), then the same batches by hand: per batch one H2D copy of the reads, the six stage calls
enqueued on one stream over buffers allocated once (chain, classify, split, extend, aim_align_device_ref, aim_sam_device_split), one
synchronize, then what a caller copies today: all n_reads * K aim_sam_t, class and segment rows, the cursors, and the CIGAR words and MD
bytes in use. The medians of `rounds` rounds are reported with their ranges: reads/s and D2H bytes per read for both. The first batch's
records are checked against the hand-driven rows through the record model (tests/map_records_model.py). One JSON line per row.
The per-kernel times of map_count_kernel / map_records_kernel come from a kernel-trace run of this tool (profiles/mapper/README.md)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

K = 4
#         l, read_size, reads per batch, (k, w, max_occ, band, flank, min_votes), max_score
SHAPES = ((100, 104, 1 << 15, (11, 5, 16, 32, 8, 2), 24), (1000, 1024, 1 << 12, (11, 10, 8, 96, 16, 2), 120))
FRACTIONS = (0.0, 0.1, 1.0)
X, O, E = 3, 4, 1
REF_LEN = 1 << 22


def make_batches(ref, l, rs, n, fraction, batches, seed=5):
    comp = np.arange(256, dtype=np.uint8)
    for a, b in (b"AT", b"TA", b"CG", b"GC"):
        comp[a] = b
    acgt = np.frombuffer(b"ACGT", dtype=np.uint8)
    out = []
    for bi in range(batches):
        rng = np.random.default_rng([seed, l, int(fraction * 100), bi])
        half = l // 2
        two = rng.random(n) < fraction
        minus2 = two & ((np.arange(n) & 1) != 0)
        pA = rng.integers(0, len(ref) - l, size=n)
        pB = rng.integers(0, len(ref) - l, size=n)
        reads = np.zeros((n, rs), dtype=np.uint8)
        reads[:, :l] = ref[pA[:, None] + np.arange(l)[None, :]]
        second = ref[pB[:, None] + np.arange(l - half)[None, :]]
        second = np.where(minus2[:, None], comp[second[:, ::-1]], second)
        reads[:, half:l] = np.where(two[:, None], second, reads[:, half:l])
        n_sub = max(1, l // 50)
        at = rng.integers(0, l, size=(n, n_sub))
        reads[np.arange(n)[:, None], at] = acgt[rng.integers(0, 4, size=(n, n_sub))]
        out.append((np.full(n, l, dtype=np.int32), reads))
    return out


class ByHand:
    """The stages on torch buffers allocated once; run(read_len, reads) enqueues everything, synchronizes once and copies back what a
    caller copies today. Returns (sam rows, class rows, seg rows, cigar words, md bytes, D2H bytes)."""

    def __init__(self, sp, ref, n, max_score, extend):
        import torch
        from aim_amd import capi, engine
        self.torch, self.capi, self.engine = torch, capi, engine
        self.sp, self.n, self.ref_len = sp, n, len(ref)
        self.extend = engine.extend_params() if extend else None
        dev = self.dev = torch.device("cuda:0")
        rs, S = sp.read_size, n * K
        self.params = engine.make_params("wfa", max_score, rs, mismatch=X, gap_o=O, gap_e=E, backtrace=True, ref_texts=True, ends_free=(0, 0, 2 * sp.flank, 2 * sp.flank))
        z = lambda nbytes: torch.zeros(max(int(nbytes), 16), dtype=torch.uint8, device=dev)
        self.d_ref = z(len(ref) + 64)
        self.d_ref[:len(ref)] = torch.from_numpy(ref).to(dev)
        self.d_bucket, self.d_pos, _ = engine.build_index_device(ref, sp.k, w=sp.options >> 8)
        self.d = {name: z(nb) for name, nb in (("rl", 4 * n), ("reads", n * rs + 64), ("req", 16 * S), ("tp", 8 * S), ("votes", 4 * S), ("seed", 16 * n), ("chains", 16 * S),
                                               ("cls", 8 * S), ("sreq", 16 * S), ("stp", 8 * S), ("spat", S * rs + 64), ("seg", 8 * S), ("ext", 24 * S),
                                               ("res", 24 * S), ("ops", 2 * S * rs + 64), ("sam", 48 * S), ("cur", 8))}
        self.ccap, self.mcap = S * 64, S * 256
        self.d["cigar"], self.d["md"] = z(4 * self.ccap), z(self.mcap)
        self.sb = capi.load().aim_scratch_bytes(capi.params_ref(self.params), S)
        self.d["scr"] = z(self.sb)
        self.h_rl = torch.zeros(n, dtype=torch.int32).pin_memory()
        self.h_reads = torch.zeros(n * rs, dtype=torch.uint8).pin_memory()
        torch.cuda.synchronize()

    def run(self, rl, reads):
        torch, capi, engine, sp, n, d = self.torch, self.capi, self.engine, self.sp, self.n, self.d
        p = {k: v.data_ptr() for k, v in d.items()}
        rs, S = sp.read_size, n * K
        st = torch.cuda.current_stream(self.dev).cuda_stream
        self.h_rl.numpy()[:] = rl
        self.h_reads.numpy()[:] = reads.reshape(-1)
        d["rl"].view(torch.int32)[:n].copy_(self.h_rl, non_blocking=True)
        d["reads"][:n * rs].copy_(self.h_reads, non_blocking=True)
        engine.seed_chain_device(sp, n, p["rl"], p["reads"], self.d_bucket.data_ptr(), self.d_pos.data_ptr(), self.ref_len, p["req"], p["tp"], p["votes"], p["seed"],
                                 p["chains"], st)
        engine.chain_classify_device(K, rs, 128, n, p["rl"], p["tp"], p["seed"], p["chains"], p["cls"], st)
        engine.split_segments_device(K, rs, sp.flank, self.ref_len, n, p["rl"], p["reads"], p["req"], p["tp"], p["seed"], p["chains"], p["cls"], p["sreq"], p["stp"],
                                     p["spat"], p["seg"], st)
        if self.extend is not None:
            engine.extend_segments_device(self.extend, K, rs, self.ref_len, n, p["rl"], p["reads"], self.d_ref.data_ptr(), p["sreq"], p["stp"], p["spat"], p["seg"],
                                          p["ext"], st)
        capi.check(capi.load().aim_align_device_ref(capi.params_ref(self.params), S, p["sreq"], p["spat"], p["stp"], self.d_ref.data_ptr(), self.ref_len, p["res"],
                                                    p["ops"], p["scr"], self.sb, st))
        engine.sam_device_split(self.params, S, p["sreq"], p["stp"], None, p["res"], p["ops"], self.d_ref.data_ptr(), self.ref_len, 0, p["sam"], p["cigar"], self.ccap,
                                p["md"], self.mcap, p["cur"], p["seg"], st)
        torch.cuda.synchronize()
        cur = d["cur"].cpu().numpy().view(np.uint32)
        sam = d["sam"][:48 * S].cpu().numpy().view(capi.SAM_DTYPE)
        cls = d["cls"][:8 * S].cpu().numpy().view(capi.CHAIN_CLASS_DTYPE)
        seg = d["seg"][:8 * S].cpu().numpy().view(capi.SEGMENT_DTYPE)
        nc, nm = min(int(cur[0]), self.ccap), min(int(cur[1]), self.mcap)
        cigar, md = d["cigar"][:4 * nc].cpu().numpy().view(np.uint32), d["md"][:nm].cpu().numpy()
        return sam, cls, seg, cigar, md, 8 + (48 + 8 + 8) * S + 4 * nc + nm


def mapper_round(m, batches):
    """All batches over slots 0 / 1; returns (seconds, D2H bytes, records)."""
    t0 = time.perf_counter()
    d2h = recs = 0
    for i, (rl, reads) in enumerate(batches):
        if i >= 2:
            out = m.wait(i & 1)
            d2h += 12 + 64 * len(out["records"]) + 4 * len(out["rec_offsets"]) + 4 * len(out["cigar"]) + len(out["md"])
            recs += len(out["records"])
        m.submit(i & 1, rl, reads)
    for i in range(max(len(batches) - 2, 0), len(batches)):
        out = m.wait(i & 1)
        d2h += 12 + 64 * len(out["records"]) + 4 * len(out["rec_offsets"]) + 4 * len(out["cigar"]) + len(out["md"])
        recs += len(out["records"])
    return time.perf_counter() - t0, d2h, recs


def check_first(m, hand, batch):
    import map_records_model as mm
    import mapper_batch as mb
    rl, reads = batch
    m.submit(0, rl, reads)
    got = {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else v) for k, v in m.wait(0).items()}
    sam, cls, seg, cigar, md, _ = hand.run(rl, reads)
    off, rec = mm.map_records(K, len(rl), seg, sam, cls)
    g, w = mb.canon(got), mb.canon({"records": rec, "rec_offsets": off, "cigar": cigar, "md": md})
    if g != w:
        raise SystemExit("mapper and hand-driven records differ")
    mapped = (rec["sam"]["flags"] & mm.SAM_UNMAPPED) == 0
    return int(mapped.sum()), len(rec)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--out")
    ap.add_argument("--shapes", default="0,1")
    ap.add_argument("--fractions", default="0,0.1,1")
    ap.add_argument("--no-extend", action="store_true")
    a = ap.parse_args()
    import torch
    torch.cuda.init()
    from aim_amd import engine
    rng = np.random.default_rng(1)
    ref = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, size=REF_LEN)]
    med = lambda xs: float(np.median(xs))
    for si in (int(x) for x in a.shapes.split(",")):
        l, rs, n, (k, w, max_occ, band, flank, min_votes), max_score = SHAPES[si]
        sp = engine.seed_params(k, rs, max_occ=max_occ, band=band, flank=flank, min_votes=min_votes, max_cands=K, w=w)
        mp = engine.mapper_params(sp, n, max_score, mismatch=X, gap_o=O, gap_e=E, extend=None if a.no_extend else engine.extend_params(), slots=2)
        hand = ByHand(sp, ref, n, max_score, not a.no_extend)
        with engine.Mapper(mp, ref) as m:
            for fraction in (float(x) for x in a.fractions.split(",")):
                batches = make_batches(ref, l, rs, n, fraction, a.batches)
                mapped, records = check_first(m, hand, batches[0])
                mapper_round(m, batches[:2])                                # warm-up of both sides
                hand.run(*batches[0])
                tm, th, bm, bh = [], [], 0, 0
                for _ in range(a.rounds):
                    s, bm, recs = mapper_round(m, batches)
                    tm.append(len(batches) * n / s)
                    t0 = time.perf_counter()
                    bh = sum(hand.run(rl, reads)[5] for rl, reads in batches)
                    th.append(len(batches) * n / (time.perf_counter() - t0))
                row = {"l": l, "read_size": rs, "K": K, "reads_per_batch": n, "batches": a.batches, "rounds": a.rounds, "split_fraction": fraction,
                       "extend": not a.no_extend, "first_batch_records": records, "first_batch_mapped_records": mapped,
                       "mapper_reads_per_s": med(tm), "mapper_range": [min(tm), max(tm)], "mapper_d2h_bytes_per_read": bm / (len(batches) * n),
                       "hand_reads_per_s": med(th), "hand_range": [min(th), max(th)], "hand_d2h_bytes_per_read": bh / (len(batches) * n),
                       "speedup": med(tm) / med(th)}
                line = json.dumps(row)
                print(line, flush=True)
                if a.out:
                    with open(a.out, "a") as f:
                        f.write(line + "\n")
        del hand
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
