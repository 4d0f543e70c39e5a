// pair_estimate.hpp -- the device side of AIM_FEATURE_PAIR_ESTIMATE (aim_hip.h, rule 15c): the span bounds of rule 14c estimated from the
// batch itself, over the slot arrays as they stand behind aim_sam_device_split.
//
//   * pair_span_hist_kernel: per read pair, whether it is a SAMPLE -- either read has exactly one mapped slot, both reach min_mapq, they
//     lie on one contig, on opposite strands, the forward one first -- and the histogram of the samples' spans, one bin per base.
//   * pair_span_bounds_kernel: one workgroup: the quartiles of the histogram by its prefix sums, the bounds rule, the 48 bytes of
//     aim_pair_estimate_t.
//
// The first takes the lane layout of pair_rescue_rows_kernel (pair.hpp): a read pair has G = 4, 8 or 16 consecutive lanes by K
// (chain_class_lanes) with candidate i of BOTH reads in lane i; one ballot per read is its mapped-slot mask, popcount == 1 says "neither
// unmapped nor split" and the set bit names the slot, whose fields reach lane 0 of the group by broadcasts. Lane 0 owns the sample.
// A workgroup counts into a histogram of its own in LDS (hist_size dwords of dynamic LDS, at most 32 KB, and one dword for the samples
// beyond it; zeroed at entry, LDS atomic adds) and adds its non-zero bins to the global one at the end, consecutive lanes taking
// consecutive bins. Those integer adds are the only atomics, as with bucket[] in the index build: a sum of counts does not depend on the
// order of its terms, so nothing of the result depends on the grid. No scratch, vector stores only, a grid-sized stride over the batch.
#pragma once

#include "aim_device.hpp"
#include "chain_class.hpp"

namespace aim {

constexpr int kPairEstThreads = 256;
constexpr uint32_t kPairEstPerCu = 8;     // as kPairPerCu: workgroups per compute unit of the resident grid
constexpr uint32_t kPairEstBlocksPerWg = 4;   // blocks of read pairs a workgroup of the histogram kernel walks at least (measured: 65 536 pairs, K = 4:
                                              // 25.0 / 16.6 / 13.1 / 22.3 us at 1 / 2 / 4 / 16 blocks per workgroup -- the flush's global adds against the walk)

struct PairEstArgs {
    uint32_t K, n_reads, hist_size, min_mapq;
    uint32_t dbg_poison_lds;              // as in KArgs (AIM_DEBUG_POISON_LDS)
    const aim_segment_t *seg;
    const aim_sam_t *sam;
    const aim_chain_class_t *cls;
    const uint32_t *contig;               // or nullptr: one sequence
    uint32_t *hist;                       // [hist_size] the bins, then [hist_size]: n_beyond     (bounds kernel: nullptr = all zero)
    // the bounds kernel alone
    uint32_t min_samples, min_slack, options, read_size, rescue_size;
    int64_t min_span, max_span;           // the fallback: aim_map_pair_params_t's own
    aim_pair_estimate_t *est;
};

#ifdef AIM_TU_PAIR_ESTIMATE   // the kernels live in tu_pair_estimate.hip alone; capi_pair.hip sees the arguments and the launchers

static_assert(sizeof(aim_sam_t) == 48 && sizeof(aim_segment_t) == 8 && sizeof(aim_chain_class_t) == 8 && sizeof(aim_pair_estimate_t) == 48,
              "rows of 12, 2, 2 and 12 dwords");

// What rule 15c reads of a slot. fl bit 0: mapped (rule 12c), bit 1: AIM_SAM_REVERSE.
struct EstCand {
    uint32_t pos_lo, pos_hi, span, fl, contig, mapq;
};

__device__ __forceinline__ EstCand est_load_slot(const PairEstArgs &a, bool live, uint64_t slot)
{
    EstCand c = {0u, 0u, 0u, 0u, 0u, 0u};
    if (live) {
        const uint32_t *w = reinterpret_cast<const uint32_t *>(a.sam) + slot * 12u;
        const uint32_t seg1 = reinterpret_cast<const uint32_t *>(a.seg)[slot * 2u + 1u];
        const uint32_t fs = w[10];
        c.pos_lo = w[2];
        c.pos_hi = w[3];
        c.span = w[4];
        c.fl = ((((seg1 >> 16) & AIM_SEG_VALID) && !(fs & AIM_SAM_UNMAPPED)) ? 1u : 0u) | ((fs & AIM_SAM_REVERSE) ? 2u : 0u);
        c.contig = a.contig ? a.contig[slot] : 0u;
        c.mapq = (reinterpret_cast<const uint32_t *>(a.cls)[slot * 2u + 1u] >> 16) & 0xffu;
    }
    return c;
}

__device__ __forceinline__ EstCand est_bcast(EstCand c, uint32_t lane, uint32_t G)
{
    EstCand o;
    o.pos_lo = (uint32_t)__shfl((int)c.pos_lo, (int)lane, (int)G);
    o.pos_hi = (uint32_t)__shfl((int)c.pos_hi, (int)lane, (int)G);
    o.span = (uint32_t)__shfl((int)c.span, (int)lane, (int)G);
    o.fl = (uint32_t)__shfl((int)c.fl, (int)lane, (int)G);
    o.contig = (uint32_t)__shfl((int)c.contig, (int)lane, (int)G);
    o.mapq = (uint32_t)__shfl((int)c.mapq, (int)lane, (int)G);
    return o;
}

// G: lanes per read pair, 4, 8 or 16 and at least K (workgroup-uniform, like every loop bound below: every lane takes every exchange).
// Dynamic LDS: 4 * (hist_size + 1) bytes.
__global__ __launch_bounds__(kPairEstThreads) void pair_span_hist_kernel(PairEstArgs a, uint32_t G)
{
    extern __shared__ __align__(16) uint32_t est_bins[];                     // [hist_size], then the count beyond
    const uint32_t H = a.hist_size;
    debug_poison_lds(a.dbg_poison_lds, 4u * (H + 1u), reinterpret_cast<char *>(est_bins));
    for (uint32_t i = threadIdx.x; i <= H; i += kPairEstThreads) est_bins[i] = 0u;
    __syncthreads();
    const uint32_t kPairs = kPairEstThreads / G;
    const uint32_t cand = threadIdx.x & (G - 1u);
    const uint32_t base = (threadIdx.x & (uint32_t)(kWave - 1)) & ~(G - 1u);
    const uint32_t gm = (1u << G) - 1u;
    const uint32_t n_mates = a.n_reads / 2u, n_blocks = (n_mates + kPairs - 1u) / kPairs;   // (slots, reads and pairs are 32-bit)
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint32_t m = blk * kPairs + threadIdx.x / G;
        const bool pair_live = m < n_mates, live = pair_live && cand < a.K;
        const EstCand A = est_load_slot(a, live, (uint64_t)(2u * m) * a.K + cand), B = est_load_slot(a, live, (uint64_t)(2u * m + 1u) * a.K + cand);
        const uint32_t mask_a = (uint32_t)(__ballot(A.fl & 1u) >> base) & gm, mask_b = (uint32_t)(__ballot(B.fl & 1u) >> base) & gm;
        const EstCand x = est_bcast(A, mask_a ? (uint32_t)__ffs(mask_a) - 1u : 0u, G), y = est_bcast(B, mask_b ? (uint32_t)__ffs(mask_b) - 1u : 0u, G);
        if (!(pair_live && cand == 0u)) continue;                            // (no exchange and no barrier below this line of the loop)
        if (__popc(mask_a) != 1 || __popc(mask_b) != 1 || x.mapq < a.min_mapq || y.mapq < a.min_mapq || x.contig != y.contig || !((x.fl ^ y.fl) & 2u)) continue;
        const bool x_rev = (x.fl & 2u) != 0;
        const int64_t px = (int64_t)((uint64_t)x.pos_hi << 32 | x.pos_lo), py = (int64_t)((uint64_t)y.pos_hi << 32 | y.pos_lo);
        const int64_t pos_f = x_rev ? py : px, pos_r = x_rev ? px : py;
        if (pos_f > pos_r) continue;
        const int64_t s = pos_r + (int64_t)(x_rev ? x.span : y.span) - pos_f;   // >= 0: pos_f <= pos_r
        atomicAdd(&est_bins[s < (int64_t)H ? (uint32_t)s : H], 1u);           // (an index of at most H: inside the H + 1 dwords)
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i <= H; i += kPairEstThreads) {           // bin H is the count beyond: one add per workgroup
        const uint32_t v = est_bins[i];
        if (v) atomicAdd(a.hist + i, v);
    }
}

// One workgroup. Thread t sums the bins [t * run, (t + 1) * run), a wave scan and the four waves' totals in LDS give its exclusive
// prefix, and it walks its run once more for the quartiles that cross inside it: p_q is the smallest s with 4 * cum(s) >= q * n.
__global__ __launch_bounds__(kPairEstThreads) void pair_span_bounds_kernel(PairEstArgs a)
{
    __shared__ uint32_t wt[kPairEstThreads / kWave];
    __shared__ uint32_t pq[3];
    debug_poison_lds(a.dbg_poison_lds, (uint32_t)sizeof wt, reinterpret_cast<char *>(wt));
    debug_poison_lds(a.dbg_poison_lds, (uint32_t)sizeof pq, reinterpret_cast<char *>(pq));
    const uint32_t tid = threadIdx.x, lane = tid & (uint32_t)(kWave - 1), wave = tid / (uint32_t)kWave;
    const uint32_t H = a.hist ? a.hist_size : 0u;
    const uint32_t run = (H + kPairEstThreads - 1u) / kPairEstThreads;
    const uint32_t lo = min(tid * run, H), hi = min(lo + run, H);
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += a.hist[i];
    uint32_t inc = sum;                                                      // inclusive over the wave
    for (uint32_t d = 1; d < (uint32_t)kWave; d <<= 1) {
        const uint32_t o = (uint32_t)__shfl_up((int)inc, d);
        if (lane >= d) inc += o;
    }
    if (lane == (uint32_t)kWave - 1u) wt[wave] = inc;
    if (tid < 3u) pq[tid] = 0u;
    __syncthreads();
    uint32_t before = inc - sum, n = 0;
    for (uint32_t w = 0; w < (uint32_t)(kPairEstThreads / kWave); ++w) {
        if (w < wave) before += wt[w];
        n += wt[w];
    }
    uint64_t cum = before;
    for (uint32_t i = lo; i < hi; ++i) {
        const uint64_t was = cum;
        cum += a.hist[i];
        for (uint32_t q = 1; q <= 3u; ++q)
            if (4u * was < (uint64_t)q * n && 4u * cum >= (uint64_t)q * n) pq[q - 1u] = i;   // bin i is the first that reaches q quarters: one thread, one bin
    }
    __syncthreads();
    if (tid == 0u) {
        const uint32_t beyond = a.hist ? a.hist[a.hist_size] : 0u;
        const int64_t p25 = pq[0], p50 = pq[1], p75 = pq[2];
        int64_t b_lo = a.min_span, b_hi = a.max_span;
        uint32_t flags = AIM_PAIR_EST_FALLBACK;
        if (n >= a.min_samples) {
            const int64_t slack = max(3 * (p75 - p25), (int64_t)a.min_slack);
            flags = p25 - slack < 0 ? AIM_PAIR_EST_FLOORED : 0u;
            b_lo = max(p25 - slack, (int64_t)0);
            b_hi = p75 + slack;
            const int64_t W = (int64_t)a.rescue_size - (int64_t)a.read_size;
            if ((a.options & AIM_PAIR_RESCUE) && b_hi - b_lo > W) {
                b_lo = max(p50 - W / 2, (int64_t)0);
                b_hi = b_lo + W;
                flags |= AIM_PAIR_EST_CLAMPED;
            }
        }
        uint4 *out = reinterpret_cast<uint4 *>(a.est);
        out[0] = make_uint4((uint32_t)b_lo, (uint32_t)((uint64_t)b_lo >> 32), (uint32_t)b_hi, (uint32_t)((uint64_t)b_hi >> 32));
        out[1] = make_uint4(n, beyond, (uint32_t)p25, (uint32_t)p50);
        out[2] = make_uint4((uint32_t)p75, flags, 0u, 0u);
    }
}

void pair_span_hist_launch(const PairEstArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s)
{
    hipLaunchKernelGGL(pair_span_hist_kernel, dim3(grid), dim3(kPairEstThreads), 4u * (a.hist_size + 1u), s, a, lanes);
}

void pair_span_bounds_launch(const PairEstArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(pair_span_bounds_kernel, dim3(1), dim3(kPairEstThreads), 0, s, a);
}
#else
void pair_span_hist_launch(const PairEstArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s);
void pair_span_bounds_launch(const PairEstArgs &a, hipStream_t s);
#endif

}  // namespace aim
