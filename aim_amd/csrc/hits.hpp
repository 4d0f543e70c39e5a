// hits.hpp -- the device side of AIM_FLAG_TOP_HITS (aim_hip.h): the N best candidates of every read, in rank order.
//
//   * hit_select_kernel: from the score-only pass's result rows, the CSR and hit_offsets -> hit_pair[H]. It runs behind
//     group_select_kernel (groups.hpp), which keeps writing aim_best_t and sel; rank 0 of a read is its sel.
//
// The ranking is a total order on a read's candidates: AIM_PAIR_OK ones by (score, batch index), then the others by batch index.
// Every candidate therefore has a unique key (class, score, index), and round j of max_hits rounds takes, per read, the smallest key
// strictly greater than the key round j - 1 emitted -- one more pass of group_select_kernel's segmented scan, with a minimum instead of
// its four-field combine. The state between rounds is one key per read, kept in the lane that owns the read; a per-lane sorted list of
// N keys merged through one scan would do N times the shuffles per step on an array the compiler has to index dynamically.
//
// No LDS allocation, no scratch, vector stores only; a read belongs to one wavefront, so no workgroup waits on another.
#pragma once

#include <climits>

#include "aim_device.hpp"
#include "groups.hpp"   // kGroupReadsPerWave

namespace aim {

#pragma GCC visibility push(hidden)
void hit_select_launch(const aim_result_t *res, uint32_t n_pairs, const uint32_t *roff, uint32_t n_reads, const uint32_t *hoff, uint32_t max_hits,
                       uint32_t n_hits, uint32_t *hit_pair, hipStream_t s);
#pragma GCC visibility pop

#ifdef AIM_TU_GROUPS   // (groups.hpp: one unit for its kernels, these and mates.hpp's)
// cls 0: AIM_PAIR_OK, s = the score with its sign bit flipped (int32 order as uint32 order); cls 1: any other status, s = 0.
// cls 2 is no candidate: greater than every key a candidate has.
struct HitKey {
    uint32_t cls, s, idx;
};

__device__ __forceinline__ bool hit_less(const HitKey &a, const HitKey &b)
{
    if (a.cls != b.cls) return a.cls < b.cls;
    if (a.s != b.s) return a.s < b.s;
    return a.idx < b.idx;
}

__device__ __forceinline__ HitKey hit_shfl(const HitKey &v, int src)
{
    HitKey o;
    o.cls = __shfl(v.cls, src, kWave);
    o.s = __shfl(v.s, src, kWave);
    o.idx = __shfl(v.idx, src, kWave);
    return o;
}

// One wave64 per kGroupReadsPerWave consecutive reads, as group_select_kernel splits them. Lane j owns read r0 + j: where its
// candidates end, where its hit rows start, how many it gets and the key its last round emitted. A round walks the wave's candidates
// 64 at a time: each lane loads one candidate's {score, status}, finds its read by a binary search inside the wave's reads, pulls that
// read's last key from the owning lane and keeps its own key only if it is greater; a segmented inclusive min-scan (6 lane shifts)
// combines the lanes of each read, a read that continues past a chunk is carried (wave-uniform) into the next one, and the owning
// lane pulls the result from the lane of the read's last candidate. It writes hit_pair[hit_offsets[r] + round].
// Rows are written only inside [hit_offsets[r], min(hit_offsets[r + 1], n_hits)) and only with a candidate of the batch: hit_offsets
// that disagree with the CSR leave rows at the value the caller's memset gave them, never an index outside the batch.
__global__ __launch_bounds__(256) void hit_select_kernel(const aim_result_t *res, uint32_t n_pairs, const uint32_t *roff, uint32_t n_reads,
                                                         const uint32_t *hoff, uint32_t max_hits, uint32_t n_hits, uint32_t *hit_pair)
{
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    const uint32_t r0 = wave * kGroupReadsPerWave;
    if (r0 >= n_reads) return;                                   // (wave-uniform)
    const uint32_t r1 = min(r0 + kGroupReadsPerWave, n_reads);
    const uint32_t c0 = min(roff[r0], n_pairs);
    const uint32_t c1 = min(max(roff[r1], c0), n_pairs);
    const HitKey none{2u, 0u, UINT_MAX};
    // the read this lane owns
    const uint32_t rj = r0 + (uint32_t)lane;
    const bool own = rj < r1;
    uint32_t jbeg = 0, jend = 0, hbeg = 0, hcnt = 0;
    if (own) {
        jbeg = min(max(roff[rj], c0), c1);
        jend = rj + 1 < r1 ? min(roff[rj + 1], c1) : c1;
        hbeg = min(hoff[rj], n_hits);
        const uint32_t hend = min(hoff[rj + 1], n_hits);
        hcnt = hend > hbeg ? min(hend - hbeg, max_hits) : 0u;
    }
    HitKey last = none;
    for (uint32_t round = 0; round < max_hits; ++round) {
        if (!__any(round < hcnt)) break;                         // (wave-uniform)
        uint32_t cseg = UINT_MAX;                                // the carried read and the minimum of its earlier chunks
        HitKey cv = none;
        HitKey got = none;
        for (uint32_t base = c0; base < c1; base += kWave) {
            const uint32_t c = base + (uint32_t)lane;
            const bool active = c < c1;
            uint32_t r = UINT_MAX;
            if (active) {
                uint32_t lo = r0, hi = r1 - 1;
                while (lo < hi) {
                    const uint32_t mid = lo + (hi - lo + 1) / 2;
                    if (roff[mid] <= c) lo = mid;
                    else hi = mid - 1;
                }
                r = lo;
            }
            const HitKey thr = hit_shfl(last, active ? (int)(r - r0) : 0);
            HitKey v = none;
            if (active) {
                const aim_result_t *x = res + c;
                const bool ok = x->status == AIM_PAIR_OK;
                const HitKey k{ok ? 0u : 1u, ok ? (uint32_t)x->score ^ 0x80000000u : 0u, c};
                if (round == 0 || hit_less(thr, k)) v = k;
            }
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) {
                const HitKey o = hit_shfl(v, max(lane - d, 0));
                const uint32_t oseg = __shfl(r, max(lane - d, 0), kWave);
                if (lane >= d && oseg == r && hit_less(o, v)) v = o;
            }
            if (active && r == cseg && hit_less(cv, v)) v = cv;  // the read carried from the previous chunk
            // the owning lane takes its read's minimum from the lane of the read's last candidate, when that lies in this chunk
            const bool here = own && jend > jbeg && jend - 1u >= base && jend - 1u - base < (uint32_t)kWave;
            const HitKey fin = hit_shfl(v, here ? (int)(jend - 1u - base) : 0);
            if (here) got = fin;
            const int tail = (int)min((uint32_t)(kWave - 1), c1 - 1u - base);   // the chunk's last active lane (wave-uniform)
            cseg = (uint32_t)__builtin_amdgcn_readlane((int)r, tail);
            cv.cls = (uint32_t)__builtin_amdgcn_readlane((int)v.cls, tail);
            cv.s = (uint32_t)__builtin_amdgcn_readlane((int)v.s, tail);
            cv.idx = (uint32_t)__builtin_amdgcn_readlane((int)v.idx, tail);
        }
        if (round < hcnt && got.cls != 2u) hit_pair[hbeg + round] = got.idx;
        last = got;
    }
}

void hit_select_launch(const aim_result_t *res, uint32_t n_pairs, const uint32_t *roff, uint32_t n_reads, const uint32_t *hoff, uint32_t max_hits,
                       uint32_t n_hits, uint32_t *hit_pair, hipStream_t s)
{
    hipLaunchKernelGGL(hit_select_kernel, group_select_grid(n_reads), dim3(256), 0, s, res, n_pairs, roff, n_reads, hoff, max_hits, n_hits, hit_pair);
}
#endif  // AIM_TU_GROUPS

}  // namespace aim
