// chain_class.hpp -- the device side of AIM_FEATURE_CHAIN_CLASS (aim_hip.h, rules 8c and 9c): what the chain kernels' K candidates of a
// read are to each other, and how far to trust the read's winner.
//
//   * chain_class_kernel: per read, the read interval of each chain, which chains overlap an earlier primary (secondary) and which
//     do not (primary; beyond candidate 0 supplementary), the best score under each primary and the chain MAPQ -> aim_chain_class_t per
//     slot. It runs behind aim_seed_chain_device or aim_seed_chain_long_device on their own buffers.
//   * read_mapq_kernel: per read, after aim_align_device_groups / aim_align_device_mates over the same slots: the chain MAPQ of the
//     chosen candidate's primary and the alignment MAPQ from aim_best_t / aim_mate_t -> aim_read_mapq_t.
//
// chain_class_kernel gives a read G = 4, 8 or 16 consecutive lanes, the smallest of them that holds K, so a wavefront classifies 16, 8
// or 4 reads at a time; lane i of the group keeps candidate i in registers. The parent loop is sequential over i and parallel over the
// earlier primaries: (lo_i, hi_i, score_i) are broadcast inside the group, every primary lane tests its overlap with i, and the group's
// bits of one wave ballot name the lowest such lane -- the parent -- to all lanes at once, so the parent counts its new secondary in
// the same step. A group never leaves a 16-lane row. Measured at K = 4 over 1 Mi reads (profiles/chain_class/README.md): 28 us per
// call with G = 4, 47 with G = 8, 87 with G = 16 -- hence the smallest group that holds K. Slots r * K + i are consecutive across a
// group and across the groups of a wavefront: loads and stores are contiguous. The one division of the rule has a quotient of at most
// 60: quot60 below.
//
// Both kernels walk the batch with a grid-sized stride, so the launch is whatever is resident and n_reads * G threads need not fit a
// launch. No LDS, no scratch, no atomics, vector stores only; a read belongs to one wavefront.
#pragma once

#include <climits>

#include "aim_device.hpp"

namespace aim {

constexpr int kChainClassMaxVgpr = 64;      // 8 wavefronts per SIMD; the bound tests/test_chain_class_cpu.py checks in the code object
constexpr int kChainClassThreads = 256;
constexpr uint32_t kChainClassPerCu = 8;    // workgroups per compute unit of the resident grid: 32 wavefronts

struct ChainClassArgs {
    uint32_t K, read_size, mask_q8, n_reads;
    const int32_t *read_len;
    const uint64_t *text_pos;
    const aim_seed_t *seed;
    const aim_chain_t *chains;
    aim_chain_class_t *cls;
};

struct ReadMapqArgs {
    uint32_t K, n_reads;
    int32_t score_unit;
    const aim_best_t *best;
    const aim_mate_t *mates;     // or nullptr
    const aim_chain_class_t *cls;
    aim_read_mapq_t *out;
};

// Lanes per read: the smallest of 4, 8, 16 that holds K candidates.
constexpr uint32_t chain_class_lanes(uint32_t K) { return K <= 4 ? 4u : K <= 8 ? 8u : 16u; }

// min(60, num / den) for den >= 1 without a 64-bit division: below 60 the quotient comes from a float estimate, which is off by one at
// the most (num < 2^38, den < 2^32; 24 bits of mantissa against a quotient below 2^6), and two exact products put it right.
__device__ __forceinline__ uint32_t quot60(uint64_t num, uint64_t den)
{
    if (num >= 60u * den) return 60u;
    uint32_t q = min((uint32_t)((float)num / (float)den), 59u);
    while ((uint64_t)q * den > num) --q;
    while ((uint64_t)(q + 1u) * den <= num) ++q;
    return q;
}
// (above the unit guard: secondary.hpp's rule 16c takes the same quotient)

#ifdef AIM_TU_CHAIN_CLASS   // the kernels live in tu_chain_class.hip alone; capi_pipeline.hip sees the arguments and the launchers

// Both 8-byte rows as the two dwords they are stored as: one dwordx2 store per row instead of a dword and four bytes.
struct ClassWords {
    uint32_t w0, w1;
};
static_assert(sizeof(aim_chain_class_t) == 8 && sizeof(aim_read_mapq_t) == 8 && alignof(aim_chain_class_t) == 4 && alignof(aim_read_mapq_t) == 4,
              "rows of two dwords");
__device__ __forceinline__ uint32_t class_parent(const ClassWords &c) { return c.w1 & 0xffu; }
__device__ __forceinline__ uint32_t class_flags(const ClassWords &c) { return (c.w1 >> 8) & 0xffu; }
__device__ __forceinline__ uint32_t class_mapq(const ClassWords &c) { return (c.w1 >> 16) & 0xffu; }

// G: lanes per read, 4, 8 or 16 and at least K (workgroup-uniform, like every loop bound below: every lane takes every shuffle).
__global__ __launch_bounds__(kChainClassThreads) void chain_class_kernel(ChainClassArgs a, uint32_t G)
{
    const uint32_t kReads = kChainClassThreads / G;             // reads per workgroup
    const uint32_t cand = threadIdx.x & (G - 1u);
    const uint32_t base = (threadIdx.x & (uint32_t)(kWave - 1)) & ~(G - 1u);   // the group's first lane
    const uint64_t n_blocks = ((uint64_t)a.n_reads + kReads - 1u) / kReads;
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t r = blk * kReads + threadIdx.x / G;
        const bool live = r < a.n_reads && cand < a.K;
        const uint64_t slot = r * a.K + cand;
        uint32_t n = 0, score = 0, m = 0;
        int32_t lo = 0, hi = 0;
        if (live) {
            n = min(a.seed[r].n_cands, a.K);
            const int32_t L = min(max(a.read_len[r], 0), (int32_t)a.read_size);
            const aim_chain_t c = a.chains[slot];
            const bool minus = (a.text_pos[slot] >> 63) != 0;
            lo = minus ? L - (int32_t)c.q_hi : (int32_t)c.q_lo;
            hi = minus ? L - (int32_t)c.q_lo : (int32_t)c.q_hi;
            score = c.score;
            m = min((uint32_t)c.n_anchors, 10u);
        }
        const bool valid = cand < n;                             // (n is 0 in a lane that is not live, and one value in a live group)
        const int32_t len = hi - lo;
        bool primary = valid && cand == 0;                       // decided for the candidates below i; false above
        uint32_t parent = 0, n_sub = 0, sub = 0;
        for (uint32_t i = 1; i < a.K; ++i) {
            const int32_t lo_i = __shfl(lo, (int)i, (int)G), hi_i = __shfl(hi, (int)i, (int)G);
            const uint32_t score_i = (uint32_t)__shfl((int)score, (int)i, (int)G);
            const int32_t len_i = hi_i - lo_i;
            const int32_t ov = min(hi, hi_i) - max(lo, lo_i);
            // |ov|, len <= 2^17 and mask_q8 <= 256: the products stay below 2^26
            const bool hit = primary && i < n && len > 0 && len_i > 0 && ov > 0 && 256 * ov >= (int32_t)a.mask_q8 * min(len, len_i);
            const uint32_t over = (uint32_t)(__ballot(hit) >> base) & ((1u << G) - 1u);   // the primaries below i that overlap it
            if (i < n) {
                const uint32_t p = over ? (uint32_t)__ffs(over) - 1u : i;
                if (cand == i) {
                    parent = p;
                    primary = !over;
                } else if (over && cand == p) {
                    ++n_sub;
                    sub = max(sub, score_i);
                }
            }
        }
        ClassWords w = {0u, 0u};                                 // an empty slot
        if (valid) {
            uint32_t flags = AIM_CHAIN_SECONDARY, mapq = 0;      // (a secondary is never a parent: its n_sub and sub are 0)
            if (primary) {
                flags = AIM_CHAIN_PRIMARY | (cand ? AIM_CHAIN_SUPPLEMENTARY : 0u);
                if (score && sub <= score) mapq = quot60(6ull * m * (uint64_t)(score - sub), score);
            }
            w.w0 = sub;
            w.w1 = parent | flags << 8 | mapq << 16 | n_sub << 24;
        }
        if (live) reinterpret_cast<ClassWords *>(a.cls)[slot] = w;
    }
}

// Rule 9c's "unmapped" test and chain evidence for read r and its chosen slot. False: unmapped. Reads d_class inside r's K slots only.
__device__ __forceinline__ bool mapq_chain(const ReadMapqArgs &a, uint64_t r, uint32_t sel, uint32_t *chain_mapq, uint32_t *flags)
{
    const ClassWords *cls = reinterpret_cast<const ClassWords *>(a.cls);
    const uint32_t first = (uint32_t)(r * a.K);                  // (n_reads * K fits 32 bits)
    if (sel == UINT_MAX || sel - first >= a.K) return false;
    const ClassWords c = cls[sel];
    if (!class_flags(c)) return false;
    const uint32_t parent = class_parent(c);
    *flags = class_flags(c);
    *chain_mapq = parent == sel - first ? class_mapq(c) : parent < a.K ? class_mapq(cls[first + parent]) : 0u;
    return true;
}

// One read per lane.
__global__ __launch_bounds__(kChainClassThreads) void read_mapq_kernel(ReadMapqArgs a)
{
    for (uint64_t r = (uint64_t)blockIdx.x * kChainClassThreads + threadIdx.x; r < a.n_reads; r += (uint64_t)gridDim.x * kChainClassThreads) {
        const aim_best_t b = a.best[r];
        uint32_t sel = b.best_pair, nb = b.n_best, mate_sel = UINT_MAX;
        int32_t s1 = b.best_score, s2 = b.second_score;
        bool proper = false;
        if (a.mates) {
            const aim_mate_t *mt = a.mates + (r >> 1);           // (fields from memory: a copy indexed by r & 1 would live in LDS)
            sel = mt->best_pair[r & 1u];
            if (mt->flags & AIM_MATE_PROPER) {
                proper = true;
                mate_sel = mt->best_pair[(r & 1u) ^ 1u];
                s1 = mt->score_sum;
                s2 = mt->second_sum;
                nb = mt->n_best;
            }
        }
        ClassWords w = {sel, AIM_MAPQ_UNMAPPED << 24};
        uint32_t chain = 0, flags = 0;
        if (mapq_chain(a, r, sel, &chain, &flags)) {
            const int64_t gap = max((int64_t)s2 - (int64_t)s1, (int64_t)0);
            const uint32_t aln = nb > 1u ? 0u : s2 == INT_MAX ? 60u : quot60(6ull * (uint64_t)gap, (uint64_t)a.score_unit);
            uint32_t anchored = chain;
            if (proper) {                                        // a pair is as well anchored as its better mate
                uint32_t mate_chain = 0, mate_flags = 0;
                if (mapq_chain(a, r ^ 1u, mate_sel, &mate_chain, &mate_flags)) anchored = max(chain, mate_chain);
            }
            const uint32_t out = (flags & AIM_CHAIN_SECONDARY ? AIM_MAPQ_SECONDARY : 0u) | (flags & AIM_CHAIN_SUPPLEMENTARY ? AIM_MAPQ_SUPPLEMENTARY : 0u) |
                                 (proper ? AIM_MAPQ_PROPER : 0u);
            w.w1 = min(aln, anchored) | chain << 8 | aln << 16 | out << 24;
        }
        reinterpret_cast<ClassWords *>(a.out)[r] = w;
    }
}

void chain_class_launch(const ChainClassArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s)
{
    hipLaunchKernelGGL(chain_class_kernel, dim3(grid), dim3(kChainClassThreads), 0, s, a, lanes);
}

void read_mapq_launch(const ReadMapqArgs &a, uint32_t grid, hipStream_t s)
{
    hipLaunchKernelGGL(read_mapq_kernel, dim3(grid), dim3(kChainClassThreads), 0, s, a);
}
#else
void chain_class_launch(const ChainClassArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s);
void read_mapq_launch(const ReadMapqArgs &a, uint32_t grid, hipStream_t s);
#endif

}  // namespace aim
