// groups.hpp -- the device side of AIM_FLAG_READ_GROUPS (aim_hip.h): reads and their candidates in one batch.
//
//   * group_map_kernel: the candidate -> read map of the CSR read_offsets (one binary search per candidate);
//   * group_unpack_kernel: the same expansion from packed read rows plus a raw side list of reads (reference-window batches);
//   * group_rows_kernel: row gathers between the read level and the candidate level -- each read's pattern row expanded into its
//     candidates' rows for the score-only pass, and the winners' pattern / text rows gathered into the second pass's batch;
//   * group_select_kernel: per read, the AIM_PAIR_OK candidate of lowest score (lowest index on a tie), the runner-up score and
//     the tie count, from the score-only pass's result rows -> aim_best_t + the selected candidate;
//   * group_results_kernel: without BACKTRACE there is no second pass: the selected result rows, as result_t or {idx, score}.
//
// Pure data movement plus one segmented wave reduction: no LDS allocation, no scratch, vector stores only.
#pragma once

#include <climits>

#include "aim_device.hpp"
#include "batch_io.hpp"   // packed_row_dwords, blocks_256, row_gather

namespace aim {

constexpr uint32_t kGroupReadsPerWave = 64;

// The kernels of this header, hits.hpp and mates.hpp are instantiated in ONE translation unit (tu_groups.hip defines AIM_TU_GROUPS);
// every other includer sees the launchers' declarations and the constants host code reads. A launcher owns its kernel's grid and block;
// the caller checks hipGetLastError().
#pragma GCC visibility push(hidden)
void group_map_launch(const uint32_t *roff, uint32_t n_reads, uint32_t n_pairs, uint32_t *cand_read, hipStream_t s);
// (nothing is launched for n_rows == 0)
void group_rows_launch(const KArgs &ka, const char *src, uint32_t n_src, const uint32_t *src_idx, uint32_t n_rows, int text, char *out, hipStream_t s);
void group_raw_slot_launch(const uint32_t *raw_pairs, uint32_t n_raw, uint32_t n_reads, uint32_t *raw_slot, hipStream_t s);
void group_unpack_launch(const KArgs &ka, const uint32_t *packed, const uint32_t *map, const uint32_t *raw_slot, const char *raw_rows, uint32_t n_raw,
                         uint32_t n_reads, char *out, hipStream_t s);
void group_select_launch(const aim_result_t *res, uint32_t n_pairs, const uint32_t *roff, uint32_t n_reads, aim_best_t *best, uint32_t *sel, hipStream_t s);
void group_results_launch(const aim_result_t *res1, const uint32_t *sel, uint32_t n_reads, int res8, void *out, hipStream_t s);
#pragma GCC visibility pop

#ifdef AIM_TU_GROUPS
// cand_read[c] = the read r with read_offsets[r] <= c < read_offsets[r + 1]. A CSR the host check would refuse yields some r in
// [0, n_reads), never an access outside read_offsets[0 .. n_reads].
__global__ __launch_bounds__(256) void group_map_kernel(const uint32_t *roff, uint32_t n_reads, uint32_t n_pairs, uint32_t *cand_read)
{
    const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= n_pairs) return;
    uint32_t lo = 0, hi = n_reads - 1;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (roff[mid] <= c) lo = mid;
        else hi = mid - 1;
    }
    cand_read[c] = lo;
}

// Row k of `out` is row src_idx[k] of `src` (rows of READ_SIZE bytes; src_idx clamped below n_src), zero at and past row k's
// pattern_len (text: text_len) as the requests in `a` give it. One thread moves W = 4 NW bytes (16-B loads and stores where READ_SIZE
// is a multiple of 16, else 8-B); loads stay inside the source row.
template <int NW>
__global__ __launch_bounds__(256) void group_rows_kernel(KArgs a, const char *src, uint32_t n_src, const uint32_t *src_idx, uint32_t n_rows, int text,
                                                         char *out)
{
    const int rs = a.p.read_size;
    const uint32_t per_row = (uint32_t)rs / (4u * NW);
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)n_rows * per_row) return;
    const uint32_t row = (uint32_t)(t / per_row), piece = (uint32_t)(t - (uint64_t)row * per_row);
    const uint32_t j = min(src_idx[row], n_src - 1u);
    const aim_request_t rq = load_request(a, row);
    const int rem = (text ? rq.text_len : rq.pattern_len) - (int)piece * 4 * NW;
    const char *s = src + (uint64_t)j * rs + (uint64_t)piece * 4 * NW;
    uint32_t w[NW];
    if constexpr (NW == 4) {
        const uint4 v = *reinterpret_cast<const uint4 *>(s);
        w[0] = v.x; w[1] = v.y; w[2] = v.z; w[3] = v.w;
    } else {
        const uint2 v = *reinterpret_cast<const uint2 *>(s);
        w[0] = v.x; w[1] = v.y;
    }
    if (rem < 4 * NW) {
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int r = rem - 4 * i;
            w[i] &= r >= 4 ? ~0u : (r <= 0 ? 0u : ((1u << (8 * r)) - 1u));
        }
    }
    char *d = out + (uint64_t)row * rs + (uint64_t)piece * 4 * NW;
    if constexpr (NW == 4) *reinterpret_cast<uint4 *>(d) = make_uint4(w[0], w[1], w[2], w[3]);
    else *reinterpret_cast<uint2 *>(d) = make_uint2(w[0], w[1]);
}

// Packed read rows (AIM_FLAG_REF_TEXTS batches): raw_slot[r] = j for the j-th read of the raw side list, UINT_MAX (memset) otherwise.
__global__ __launch_bounds__(256) void group_raw_slot_kernel(const uint32_t *raw_pairs, uint32_t n_raw, uint32_t n_reads, uint32_t *raw_slot)
{
    const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n_raw) return;
    const uint32_t r = raw_pairs[j];
    if (r < n_reads) raw_slot[r] = j;
}

// ... and the candidates' ASCII pattern rows from them: candidate c's row is its read's packed row expanded (unpack_rows_kernel's
// decode, 8 bases per thread) or, for a raw read, its raw row; zero at and past c's pattern_len.
__global__ __launch_bounds__(256) void group_unpack_kernel(KArgs a, const uint32_t *packed, const uint32_t *map, const uint32_t *raw_slot,
                                                           const char *raw_rows, uint32_t n_raw, uint32_t n_reads, char *out)
{
    const int rs = a.p.read_size;
    const uint32_t per_row = (uint32_t)rs / 8u;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)a.n_pairs * per_row) return;
    const uint32_t c = (uint32_t)(t / per_row), piece = (uint32_t)(t - (uint64_t)c * per_row);
    const uint32_t r = min(map[c], n_reads - 1u), j = raw_slot[r];
    uint32_t w0, w1;
    if (j < n_raw) {
        const uint2 v = reinterpret_cast<const uint2 *>(raw_rows + (uint64_t)j * rs)[piece];
        w0 = v.x; w1 = v.y;
    } else {
        const uint32_t bits = reinterpret_cast<const uint16_t *>(packed + (uint64_t)r * packed_row_dwords(rs))[piece];
        const uint32_t lo = (bits & 3u) | ((bits & 0xCu) << 6) | ((bits & 0x30u) << 12) | ((bits & 0xC0u) << 18);
        const uint32_t hb = bits >> 8;
        const uint32_t hi = (hb & 3u) | ((hb & 0xCu) << 6) | ((hb & 0x30u) << 12) | ((hb & 0xC0u) << 18);
        w0 = __builtin_amdgcn_perm(0u, 0x47544341u, lo);
        w1 = __builtin_amdgcn_perm(0u, 0x47544341u, hi);
    }
    const int rem = load_request(a, c).pattern_len - (int)piece * 8;
    if (rem < 8) {
        const uint64_t keep = rem <= 0 ? 0ull : ((1ull << (8 * rem)) - 1ull);
        w0 &= (uint32_t)keep;
        w1 &= (uint32_t)(keep >> 32);
    }
    reinterpret_cast<uint2 *>(out + (uint64_t)c * rs)[piece] = make_uint2(w0, w1);
}

// ---- best-of selection ----------------------------------------------------------------------------------------------------
// What a run of candidates of one read contributes: the lowest OK score, its (lowest) index, how many OK candidates have it, and the
// lowest OK score among the others (INT_MAX when there is none). cnt == 0: no OK candidate.
struct GroupSel {
    int s;
    uint32_t idx;
    uint32_t cnt;
    int sec;
};

// a covers candidates before b's
__device__ __forceinline__ GroupSel group_combine(const GroupSel &a, const GroupSel &b)
{
    if (!b.cnt) return a;
    if (!a.cnt) return b;
    if (a.s < b.s) return GroupSel{a.s, a.idx, a.cnt, min(a.sec, b.s)};
    if (b.s < a.s) return GroupSel{b.s, b.idx, b.cnt, min(b.sec, a.s)};
    return GroupSel{a.s, a.idx, a.cnt + b.cnt, a.s};
}

// One wave64 per kGroupReadsPerWave consecutive reads. It walks their candidates 64 at a time: each lane loads one candidate's
// {score, status}, finds its read by a binary search inside the wave's reads, and a segmented inclusive scan (6 lane shifts) combines
// the lanes of each read. A read that continues past a chunk is carried (wave-uniform) into the next one, so a read of any size is
// one pass over its candidates, and many short reads share a chunk. The lane holding a read's last candidate writes its aim_best_t
// (one 16-B store) and sel.
__global__ __launch_bounds__(256) void group_select_kernel(const aim_result_t *res, uint32_t n_pairs, const uint32_t *roff, uint32_t n_reads,
                                                           aim_best_t *best, uint32_t *sel)
{
    const int lane = threadIdx.x & (kWave - 1);
    const uint32_t wave = blockIdx.x * (blockDim.x / kWave) + threadIdx.x / kWave;
    const uint32_t r0 = wave * kGroupReadsPerWave;
    if (r0 >= n_reads) return;                                   // (wave-uniform)
    const uint32_t r1 = min(r0 + kGroupReadsPerWave, n_reads);
    const uint32_t c0 = min(roff[r0], n_pairs);
    const uint32_t c1 = min(max(roff[r1], c0), n_pairs);
    uint32_t cseg = UINT_MAX;                                    // the carried read and what its earlier chunks gave
    GroupSel cv{INT_MAX, UINT_MAX, 0u, INT_MAX};
    for (uint32_t base = c0; base < c1; base += kWave) {
        const uint32_t c = base + (uint32_t)lane;
        const bool active = c < c1;
        uint32_t r = UINT_MAX, end = 0;
        GroupSel v{INT_MAX, UINT_MAX, 0u, INT_MAX};
        if (active) {
            uint32_t lo = r0, hi = r1 - 1;
            while (lo < hi) {
                const uint32_t mid = lo + (hi - lo + 1) / 2;
                if (roff[mid] <= c) lo = mid;
                else hi = mid - 1;
            }
            r = lo;
            end = r + 1 < r1 ? min(roff[r + 1], c1) : c1;
            const aim_result_t *x = res + c;
            if (x->status == AIM_PAIR_OK) v = GroupSel{x->score, c, 1u, INT_MAX};
        }
#pragma unroll
        for (int d = 1; d < kWave; d <<= 1) {
            GroupSel o;
            o.s = __shfl_up(v.s, d, kWave);
            o.idx = __shfl_up(v.idx, d, kWave);
            o.cnt = __shfl_up(v.cnt, d, kWave);
            o.sec = __shfl_up(v.sec, d, kWave);
            const uint32_t oseg = __shfl_up(r, d, kWave);
            if (lane >= d && oseg == r) v = group_combine(o, v);
        }
        if (active && r == cseg) v = group_combine(cv, v);       // the read carried from the previous chunk
        if (active && c + 1 == end) {
            const bool any = v.cnt != 0;
            const uint32_t first = min(roff[r], n_pairs - 1u);
            if (best)
                *reinterpret_cast<uint4 *>(best + r) = make_uint4(any ? v.idx : UINT_MAX, (uint32_t)(any ? v.s : INT_MAX),
                                                                  (uint32_t)(any ? v.sec : INT_MAX), v.cnt);
            sel[r] = any ? v.idx : first;
        }
        const int last = (int)min((uint32_t)(kWave - 1), c1 - 1u - base);   // the chunk's last active lane (wave-uniform)
        cseg = (uint32_t)__builtin_amdgcn_readlane((int)r, last);
        cv.s = __builtin_amdgcn_readlane(v.s, last);
        cv.idx = (uint32_t)__builtin_amdgcn_readlane((int)v.idx, last);
        cv.cnt = (uint32_t)__builtin_amdgcn_readlane((int)v.cnt, last);
        cv.sec = __builtin_amdgcn_readlane(v.sec, last);
    }
}

// No BACKTRACE: read r's row is the score-only pass's row of sel[r] (result_t, or {idx, score} under AIM_FLAG_RES8 with
// AIM_SCORE_FAILED for a pair that stopped with a status, as store_result writes it).
__global__ __launch_bounds__(256) void group_results_kernel(const aim_result_t *res1, const uint32_t *sel, uint32_t n_reads, int res8, void *out)
{
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n_reads) return;
    const aim_result_t x = res1[sel[r]];
    if (res8) {
        *reinterpret_cast<uint2 *>(static_cast<aim_result8_t *>(out) + r) =
            make_uint2(x.idx, (uint32_t)(x.status == AIM_PAIR_OK ? x.score : AIM_SCORE_FAILED));
    } else {
        static_cast<aim_result_t *>(out)[r] = x;
    }
}

// ---- the launchers declared at the top ---------------------------------------------------------------------------------------
void group_map_launch(const uint32_t *roff, uint32_t n_reads, uint32_t n_pairs, uint32_t *cand_read, hipStream_t s)
{
    hipLaunchKernelGGL(group_map_kernel, blocks_256(n_pairs), dim3(256), 0, s, roff, n_reads, n_pairs, cand_read);
}

void group_rows_launch(const KArgs &ka, const char *src, uint32_t n_src, const uint32_t *src_idx, uint32_t n_rows, int text, char *out, hipStream_t s)
{
    if (!n_rows) return;
    const RowGather g = row_gather(ka.p.read_size, n_rows);
    if (g.nw == 4) hipLaunchKernelGGL(group_rows_kernel<4>, g.grid, dim3(256), 0, s, ka, src, n_src, src_idx, n_rows, text, out);
    else hipLaunchKernelGGL(group_rows_kernel<2>, g.grid, dim3(256), 0, s, ka, src, n_src, src_idx, n_rows, text, out);
}

void group_raw_slot_launch(const uint32_t *raw_pairs, uint32_t n_raw, uint32_t n_reads, uint32_t *raw_slot, hipStream_t s)
{
    hipLaunchKernelGGL(group_raw_slot_kernel, blocks_256(n_raw), dim3(256), 0, s, raw_pairs, n_raw, n_reads, raw_slot);
}

void group_unpack_launch(const KArgs &ka, const uint32_t *packed, const uint32_t *map, const uint32_t *raw_slot, const char *raw_rows, uint32_t n_raw,
                         uint32_t n_reads, char *out, hipStream_t s)
{
    hipLaunchKernelGGL(group_unpack_kernel, blocks_256((uint64_t)ka.n_pairs * (uint64_t)(ka.p.read_size / 8)), dim3(256), 0, s, ka, packed, map, raw_slot,
                       raw_rows, n_raw, n_reads, out);
}

// group_select_kernel and hit_select_kernel (hits.hpp): four wavefronts per workgroup, kGroupReadsPerWave reads per wavefront
inline dim3 group_select_grid(uint32_t n_reads)
{
    const uint32_t waves = (n_reads + kGroupReadsPerWave - 1) / kGroupReadsPerWave;
    return dim3((waves + 3) / 4);
}

void group_select_launch(const aim_result_t *res, uint32_t n_pairs, const uint32_t *roff, uint32_t n_reads, aim_best_t *best, uint32_t *sel, hipStream_t s)
{
    hipLaunchKernelGGL(group_select_kernel, group_select_grid(n_reads), dim3(256), 0, s, res, n_pairs, roff, n_reads, best, sel);
}

void group_results_launch(const aim_result_t *res1, const uint32_t *sel, uint32_t n_reads, int res8, void *out, hipStream_t s)
{
    hipLaunchKernelGGL(group_results_kernel, blocks_256(n_reads), dim3(256), 0, s, res1, sel, n_reads, res8, out);
}
#endif  // AIM_TU_GROUPS

}  // namespace aim
