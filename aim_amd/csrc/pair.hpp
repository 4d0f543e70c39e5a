// pair.hpp -- the device side of AIM_FEATURE_PAIRED (aim_hip.h, rule 14c): reads 2m and 2m + 1 of a batch as mates, over the slot-shaped
// rows the split path leaves (aim_segment_t, aim_sam_t, aim_chain_class_t and, for several sequences, the contig per slot r * K + i).
//
//   * pair_rescue_rows_kernel: per read pair, whether a proper combination exists among the mapped slots, and per read b the row of the
//     rescue alignment -- the window its mate's representative implies, clipped to the anchor's contig -- or an empty row, plus the
//     read copied into a pattern row of rescue_size bytes.
//   * pair_select_kernel: per read pair, the proper combination of lowest cost over the mapped slots and the mapped rescue rows (index
//     K), against the unpaired cost -> aim_map_pair_t; where a rescue row is in the winning combination it is folded into the read's
//     slot 0 in place (apply), so rules 12c / 13c run unchanged behind it.
//   * pair_rescue_rows_est_kernel, pair_select_est_kernel: the same two bodies with min_span / max_span loaded from the aim_pair_estimate_t
//     of rule 15c (pair_estimate.hpp) in device memory instead of taken from the arguments.
//   * map_mates_kernel: behind the record kernel, one record per lane: the paired SAM flag bits into the record and aim_map_mate_t.
//
// The first two give a read pair G = 4, 8 or 16 consecutive lanes by K (chain_class_lanes), with candidate i of BOTH reads in lane i
// of the group. Lane i meets candidate j of the mate through K broadcasts inside the group, keeps the best of its row of combinations,
// and the lanes' partial results meet in a butterfly of log2(G) exchanges (the reduction of mates.hpp, carried over with the span
// added: commutative and associative, so the result does not depend on which lane saw which combination). A rescue row is no lane's: it
// is loaded by every lane of the group (one address, a broadcast) and paired with the lane's own candidate of the other read. The
// group's bits of one wave ballot are a read's mapped slots, the lowest set bit its representative. A group never leaves a 16-lane row.
//
// Apply is fused into pair_select_kernel: a read pair's slots are read and written by its own group alone, every load of a slot comes
// before the stores to it in program order of the same lanes, and no group reads another pair's slots, so nothing depends on the grid.
//
// No LDS, no scratch, no atomics, vector stores only; all three walk the batch with a grid-sized stride.
#pragma once

#include <climits>

#include "aim_device.hpp"
#include "chain_class.hpp"

namespace aim {

constexpr int kPairMaxVgpr = 64;          // 8 wavefronts per SIMD; the bound tests/test_pairs_cpu.py checks in the code object
constexpr int kPairThreads = 256;
constexpr uint32_t kPairPerCu = 8;        // workgroups per compute unit of the resident grid: 32 wavefronts

struct PairArgs {
    uint32_t K, n_reads, read_size, rescue_size, options, n_contigs;
    int32_t unpaired_penalty;
    uint32_t cigar_base, md_base;
    int64_t min_span, max_span, ref_len;
    const int32_t *read_len;
    const char *reads;                    // [n_reads][read_size]                         (rows kernel)
    aim_segment_t *seg;                   // the slot arrays; written by select's apply alone
    aim_sam_t *sam;
    aim_chain_class_t *cls;
    uint32_t *contig;                     // or nullptr: one sequence
    const uint32_t *contig_start, *contig_len;
    aim_request_t *res_req;               // [n_reads]                                    (rows kernel)
    uint64_t *res_text_pos;               // [n_reads]
    char *res_patterns;                   // [n_reads][rescue_size]
    const aim_sam_t *res_sam;             // [n_reads], or nullptr without AIM_PAIR_RESCUE (select kernel)
    aim_map_pair_t *pairs;                // [n_reads / 2]
};

struct MatesArgs {
    uint32_t K, n_reads, n_contigs;
    const aim_map_pair_t *pairs;
    const aim_segment_t *seg;
    const aim_sam_t *sam;
    const uint32_t *contig;               // or nullptr
    const uint32_t *contig_start;
    const uint32_t *rec_offsets;
    aim_map_record_t *records;
    aim_map_mate_t *mates;
};

// The grid of a kernel that walks `units` items, per_block to a workgroup: what is resident at the most.
inline uint32_t pair_grid(const Knobs &kn, uint64_t units, uint32_t per_block)
{
    const uint64_t blocks = (units + per_block - 1u) / per_block;
    return (uint32_t)(blocks < resident_grid(kn, kPairPerCu) ? blocks : resident_grid(kn, kPairPerCu));
}

// The device helpers: what tu_pair.hip's kernels and those of rule 17c (pair_secondary.hpp in tu_pair_secondary.hip) share.
#if defined(AIM_TU_PAIR) || defined(AIM_TU_PAIR_SECONDARY)

static_assert(sizeof(aim_sam_t) == 48 && sizeof(aim_map_record_t) == 64 && sizeof(aim_segment_t) == 8 && sizeof(aim_chain_class_t) == 8 &&
                  sizeof(aim_map_pair_t) == 32 && sizeof(aim_map_mate_t) == 16 && sizeof(aim_request_t) == 16,
              "rows of 12, 16, 2, 2, 8, 4 and 4 dwords");

// What rule 14c reads of a record, slot or rescue row. fl bit 0: mapped (rule 12c), bit 1: AIM_SAM_REVERSE.
struct PairCand {
    uint32_t pos_lo, pos_hi, span, fl, contig;
    int score;
};

// (seg_valid: the slot's AIM_SEG_VALID; a rescue row passes `usable`)
__device__ __forceinline__ PairCand pair_load(const aim_sam_t *rows, bool live, uint64_t row, bool seg_valid, uint32_t contig)
{
    PairCand c = {0u, 0u, 0u, 0u, contig, 0};
    if (live) {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(rows) + row * 12u;
        const uint4 w0 = *reinterpret_cast<const uint4 *>(w);
        const uint32_t fs = w[10];
        c.score = (int)w0.y;
        c.pos_lo = w0.z;
        c.pos_hi = w0.w;
        c.span = w[4];
        c.fl = ((seg_valid && !(fs & AIM_SAM_UNMAPPED)) ? 1u : 0u) | ((fs & AIM_SAM_REVERSE) ? 2u : 0u);
    }
    return c;
}

__device__ __forceinline__ PairCand pair_load_slot(const PairArgs &a, bool live, uint64_t slot)
{
    const uint32_t seg1 = live ? reinterpret_cast<const uint32_t *>(a.seg)[slot * 2u + 1u] : 0u;
    const uint32_t contig = live && a.contig ? a.contig[slot] : 0u;
    return pair_load(a.sam, live, slot, ((seg1 >> 16) & AIM_SEG_VALID) != 0, contig);
}

__device__ __forceinline__ PairCand pair_bcast(PairCand c, uint32_t lane, uint32_t G)
{
    PairCand o;
    o.pos_lo = (uint32_t)__shfl((int)c.pos_lo, (int)lane, (int)G);
    o.pos_hi = (uint32_t)__shfl((int)c.pos_hi, (int)lane, (int)G);
    o.span = (uint32_t)__shfl((int)c.span, (int)lane, (int)G);
    o.fl = (uint32_t)__shfl((int)c.fl, (int)lane, (int)G);
    o.contig = (uint32_t)__shfl((int)c.contig, (int)lane, (int)G);
    o.score = __shfl(c.score, (int)lane, (int)G);
    return o;
}

// The span of the combination (x of read 2m, y of read 2m + 1) when it is proper, else -1 (a proper span is >= min_span >= 0).
__device__ __forceinline__ int64_t pair_span(const PairArgs &a, PairCand x, PairCand y)
{
    if (!(x.fl & y.fl & 1u) || x.contig != y.contig || !((x.fl ^ y.fl) & 2u)) return -1;
    const bool x_rev = (x.fl & 2u) != 0;
    const int64_t px = (int64_t)((uint64_t)x.pos_hi << 32 | x.pos_lo), py = (int64_t)((uint64_t)y.pos_hi << 32 | y.pos_lo);
    const int64_t pos_f = x_rev ? py : px, pos_r = x_rev ? px : py;
    const int64_t s = pos_r + (int64_t)(x_rev ? x.span : y.span) - pos_f;
    return (pos_f <= pos_r && s >= a.min_span && s <= a.max_span) ? s : -1;
}

// What a set of combinations of one read pair contributes (MateSel of mates.hpp, with the winner's span). cnt == 0: none is proper.
struct PairSel {
    int cost;
    uint32_t ij, cnt;                     // i << 8 | j: its order is "lowest i, then lowest j" (indices are at most AIM_SEED_MAX_CANDS)
    int sec;
    uint32_t span_lo, span_hi;
};

// commutative and associative (the tie-break is by (i, j), not by position); field-wise selects on values: nothing may take an address
__device__ __forceinline__ PairSel pair_combine(PairSel a, PairSel b)
{
    const bool tie = a.cnt && b.cnt && a.cost == b.cost;
    const bool a_wins = !b.cnt || (a.cnt && (a.cost < b.cost || (tie && a.ij < b.ij)));
    PairSel r;
    r.cost = a_wins ? a.cost : b.cost;
    r.ij = a_wins ? a.ij : b.ij;
    r.cnt = tie ? a.cnt + b.cnt : (a_wins ? a.cnt : b.cnt);
    r.sec = min(min(a.sec, b.sec), a_wins ? b.cost : a.cost);
    r.span_lo = a_wins ? a.span_lo : b.span_lo;
    r.span_hi = a_wins ? a.span_hi : b.span_hi;
    return r;
}

__device__ __forceinline__ PairSel pair_none() { return PairSel{INT_MAX, UINT_MAX, 0u, INT_MAX, 0u, 0u}; }

__device__ __forceinline__ int pair_clamp(int64_t v) { return (int)min(v, (int64_t)INT_MAX - 1); }

// v with the combination (i, j) of x and y added when it is proper (pair_span and the cost do not ask which of the two is read 2m's)
__device__ __forceinline__ PairSel pair_add(const PairArgs &a, PairSel v, PairCand x, PairCand y, uint32_t i, uint32_t j)
{
    const int64_t s = pair_span(a, x, y);
    const bool ok = s >= 0;                // (what is not proper joins as pair_none(): cnt 0 and cost INT_MAX reach no field of the result)
    const PairSel one = {ok ? pair_clamp((int64_t)x.score + y.score) : INT_MAX, ok ? (i << 8 | j) : UINT_MAX, ok ? 1u : 0u, INT_MAX,
                         ok ? (uint32_t)s : 0u, ok ? (uint32_t)((uint64_t)s >> 32) : 0u};
    return pair_combine(v, one);
}

// every lane of the group ends with the group's result (uniform control flow: every lane takes every exchange)
__device__ __forceinline__ PairSel pair_butterfly(PairSel v, uint32_t G)
{
    for (uint32_t d = 1; d < G; d <<= 1) {
        PairSel o;
        o.cost = __shfl_xor(v.cost, (int)d, (int)G);
        o.ij = (uint32_t)__shfl_xor((int)v.ij, (int)d, (int)G);
        o.cnt = (uint32_t)__shfl_xor((int)v.cnt, (int)d, (int)G);
        o.sec = __shfl_xor(v.sec, (int)d, (int)G);
        o.span_lo = (uint32_t)__shfl_xor((int)v.span_lo, (int)d, (int)G);
        o.span_hi = (uint32_t)__shfl_xor((int)v.span_hi, (int)d, (int)G);
        v = pair_combine(v, o);
    }
    return v;
}

// A lane's part of the combinations among the mapped slots of a read pair, row i of them: lane i holds candidate i of read 2m (A) and of
// read 2m + 1 (B). The group has a proper combination when any lane's part has one: one ballot, no exchange.
__device__ __forceinline__ PairSel pair_mapped_row(const PairArgs &a, PairCand A, PairCand B, uint32_t cand, uint32_t G)
{
    PairSel v = pair_none();
    for (uint32_t j = 0; j < a.K; ++j) v = pair_add(a, v, A, pair_bcast(B, j, G), cand, j);
    return v;
}

__device__ __forceinline__ uint32_t pair_read_len(const PairArgs &a, bool live, uint32_t r)
{
    return live ? (uint32_t)min(max(a.read_len[r], 0), (int)a.read_size) : 0u;
}

#endif

#ifdef AIM_TU_PAIR   // the kernels live in tu_pair.hip alone; capi_pair.hip sees the arguments and the launchers

// G: lanes per read pair, 4, 8 or 16 and at least K (workgroup-uniform, like every loop bound below: every lane takes every exchange).
// The body is pair_rescue_rows_body.inc: one text for this kernel and its rule-15c twin.
__global__ __launch_bounds__(kPairThreads) void pair_rescue_rows_kernel(PairArgs a, uint32_t G)
{
#include "pair_rescue_rows_body.inc"
}

// Rule 15c: the bounds are the estimate's, which the kernel in front of this one on the stream wrote (two uniform 64-bit loads).
__global__ __launch_bounds__(kPairThreads) void pair_rescue_rows_est_kernel(PairArgs a, uint32_t G, const aim_pair_estimate_t *est)
{
    a.min_span = est->min_span;
    a.max_span = est->max_span;
#include "pair_rescue_rows_body.inc"
}

// (the body: pair_select_body.inc, shared with the rule-15c twin below)
__global__ __launch_bounds__(kPairThreads) void pair_select_kernel(PairArgs a, uint32_t G)
{
#include "pair_select_body.inc"
}

__global__ __launch_bounds__(kPairThreads) void pair_select_est_kernel(PairArgs a, uint32_t G, const aim_pair_estimate_t *est)
{
    a.min_span = est->min_span;
    a.max_span = est->max_span;
#include "pair_select_body.inc"
}

// One record per lane. The mate's mapped slots come from the slot arrays (as apply left them), never from other lanes' records.
__global__ __launch_bounds__(kPairThreads) void map_mates_kernel(MatesArgs a)
{
    const uint32_t K = a.K;
    const uint64_t n_rec = min((uint64_t)a.rec_offsets[a.n_reads], (uint64_t)a.n_reads * K);   // (never beyond d_records and d_mates)
    for (uint64_t t = (uint64_t)blockIdx.x * kPairThreads + threadIdx.x; t < n_rec; t += (uint64_t)gridDim.x * kPairThreads) {
        uint4 *row = reinterpret_cast<uint4 *>(a.records) + t * 4u;
        const uint4 w0 = row[0], w2 = row[2], w3 = row[3];
        const uint32_t r = w3.x, slot = w3.w;
        if (r >= a.n_reads) continue;                                          // (never for records of the record kernel)
        const uint32_t mate = r ^ 1u;
        const uint4 *pr = reinterpret_cast<const uint4 *>(a.pairs + (r >> 1));
        const uint4 p0 = pr[0], p1 = pr[1];
        const bool proper = (p1.y & AIM_PAIR_PROPER) != 0;
        // a chosen rescue row (r * K + K) lies in slot r * K since apply
        uint32_t own = (r & 1u) ? p0.y : p0.x, other = (r & 1u) ? p0.x : p0.y;
        if (own == r * K + K) own = r * K;
        if (other == mate * K + K) other = mate * K;
        uint32_t ms = UINT_MAX;                                                // the mate's reference record: its representative ...
        for (uint32_t i = K; i-- > 0u;) {
            const uint32_t s = mate * K + i;
            const uint32_t seg1 = reinterpret_cast<const uint32_t *>(a.seg)[(uint64_t)s * 2u + 1u];
            const uint32_t fs = reinterpret_cast<const uint32_t *>(a.sam)[(uint64_t)s * 12u + 10u];
            if (((seg1 >> 16) & AIM_SEG_VALID) && !(fs & AIM_SAM_UNMAPPED)) ms = s;
        }
        const bool mate_mapped = ms != UINT_MAX;
        if (mate_mapped && proper && other - mate * K < K) ms = other;         // ... or, in a proper pair, its chosen slot
        const bool chosen = proper && slot == own, reverse = (w2.z & AIM_SAM_REVERSE) != 0, mapped = !(w2.z & AIM_SAM_UNMAPPED);
        uint32_t flags = 0x1u | ((r & 1u) ? 0x80u : 0x40u) | (mate_mapped ? 0u : 0x8u) | (chosen ? 0x2u : 0u);
        uint64_t mpos = 0;
        uint32_t mc = a.contig ? AIM_CONTIG_NONE : 0u;
        if (mate_mapped) {
            const uint32_t *mw = reinterpret_cast<const uint32_t *>(a.sam) + (uint64_t)ms * 12u;
            if (mw[10] & AIM_SAM_REVERSE) flags |= 0x20u;
            mc = a.contig ? a.contig[ms] : 0u;
            mpos = ((uint64_t)mw[3] << 32 | mw[2]) - ((a.contig && mc < a.n_contigs) ? a.contig_start[mc] : 0u);
        } else if (mapped) {
            mpos = (uint64_t)w0.w << 32 | w0.z;                                // the record's own, already local to its contig
            mc = a.contig ? w2.w : 0u;
        }
        const int64_t span = min((int64_t)((uint64_t)p1.w << 32 | p1.z), (int64_t)INT_MAX);
        const int tlen = chosen ? (int)(reverse ? -span : span) : 0;
        reinterpret_cast<uint32_t *>(row)[10] = w2.z | flags;                  // sam.flags (status, the upper half, is kept)
        reinterpret_cast<uint4 *>(a.mates)[t] = make_uint4((uint32_t)mpos, (uint32_t)(mpos >> 32), (uint32_t)tlen, mc);
    }
}

void pair_rescue_rows_launch(const PairArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s)
{
    hipLaunchKernelGGL(pair_rescue_rows_kernel, dim3(grid), dim3(kPairThreads), 0, s, a, lanes);
}

void pair_select_launch(const PairArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s)
{
    hipLaunchKernelGGL(pair_select_kernel, dim3(grid), dim3(kPairThreads), 0, s, a, lanes);
}

void pair_rescue_rows_est_launch(const PairArgs &a, uint32_t lanes, uint32_t grid, const aim_pair_estimate_t *est, hipStream_t s)
{
    hipLaunchKernelGGL(pair_rescue_rows_est_kernel, dim3(grid), dim3(kPairThreads), 0, s, a, lanes, est);
}

void pair_select_est_launch(const PairArgs &a, uint32_t lanes, uint32_t grid, const aim_pair_estimate_t *est, hipStream_t s)
{
    hipLaunchKernelGGL(pair_select_est_kernel, dim3(grid), dim3(kPairThreads), 0, s, a, lanes, est);
}

void map_mates_launch(const MatesArgs &a, uint32_t grid, hipStream_t s)
{
    hipLaunchKernelGGL(map_mates_kernel, dim3(grid), dim3(kPairThreads), 0, s, a);
}
#else
void pair_rescue_rows_launch(const PairArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s);
void pair_select_launch(const PairArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s);
void pair_rescue_rows_est_launch(const PairArgs &a, uint32_t lanes, uint32_t grid, const aim_pair_estimate_t *est, hipStream_t s);
void pair_select_est_launch(const PairArgs &a, uint32_t lanes, uint32_t grid, const aim_pair_estimate_t *est, hipStream_t s);
void map_mates_launch(const MatesArgs &a, uint32_t grid, hipStream_t s);
#endif

}  // namespace aim
