// split.hpp -- the device side of AIM_FEATURE_SPLIT (aim_hip.h, rule 10c): one alignable segment row per primary chain of a read.
//
// split_segments_kernel runs behind aim_chain_classify_device on the chain kernels' own buffers. Per read it decides, for each of the K
// slots, whether the slot is a primary, which of its sides are open, the read interval [a', b') and the reference window of the
// segment, and writes aim_request_t / text_pos / aim_segment_t per slot; then it gathers the K pattern rows: read[a', b') shifted to
// the row's start and zero-filled for a primary, the whole read row for every other slot (rule 7's empty slot).
//
// Mapping. A read gets a group of G = 16 or 64 lanes. Lane i < K of the group keeps slot i in registers: the "no other primary starts
// lower / ends higher" tests are K steps of group-wide shuffles, as in chain_class_kernel. The K destination rows of a read are
// contiguous (slot rows follow each other), so the gather is one flat walk over K * read_size / 8 units of 8 bytes: lane l of the
// group takes units l, l + G, ...; consecutive lanes store consecutive 8-byte words (a wavefront writes 512 contiguous bytes per
// step) and read consecutive, mostly shared, dwords of the source row, which a' shifts by any number of bytes: three aligned dword
// loads and two alignbyte's per unit. The unit's slot comes from a float quotient put right by one product; the slot's (a', length)
// comes from its lane by one shuffle.
//   G = 16 for rows up to kSplitWideMin bytes: four reads per wavefront, so that short rows (13 units at read_size 104) do not leave
//   most lanes idle; G = 64 above. Long rows are also cut into `parts` (a power of two) interleaved shares, each walked by a group of
//   its own, which repeats the cheap decision and leaves the per-slot records to share 0: a batch of a few thousand long reads still
//   fills the device. parts depends on K and read_size alone, never on the grid, and no output byte depends on either.
// Measured (profiles/split/README.md): 0.37-0.55 of the 8 TB/s roofline in algorithmic bytes at K = 4, against 0.64-0.75 for the
// AIM_FLAG_REF_TEXTS gather. What bounds it was not measured with counters. The loads per store do not seem to: a copy without branches (indices clamped into the row, four
// steps unrolled) and one aligned 8-byte load for the rows that need no shift each left the times where they were or behind. The supposition that
// remains: a group walks a dependent chain per read -- the slot records, the shuffles, the row loads, the stores -- at full occupancy.
// The kernel walks (read, share) items with a grid-sized stride. No LDS, no scratch, no atomics, vector stores only; an output byte
// has exactly one writer.
#pragma once

#include "aim_device.hpp"

namespace aim {

constexpr int kSplitMaxVgpr = 64;           // 8 wavefronts per SIMD; the bound tests/test_split_cpu.py checks in the code object
constexpr int kSplitThreads = 256;
constexpr uint32_t kSplitPerCu = 8;         // workgroups per compute unit of the resident grid: 32 wavefronts
constexpr uint32_t kSplitWideMin = 512;     // read_size from which a read gets a whole wavefront
constexpr uint32_t kSplitShareUnits = 1024; // units (8 B) of one share of a long read: 16 steps of a wavefront

struct SplitArgs {
    uint32_t K, read_size, n_reads, parts_log2;
    int64_t flank, ref_len;
    const int32_t *read_len;
    const char *reads;
    const aim_request_t *requests;
    const uint64_t *text_pos;
    const aim_seed_t *seed;
    const aim_chain_t *chains;
    const aim_chain_class_t *cls;
    aim_request_t *seg_requests;
    uint64_t *seg_text_pos;
    char *seg_patterns;
    aim_segment_t *seg;
};

// Lanes per read and shares per read: functions of K and read_size alone.
constexpr uint32_t split_lanes(uint32_t read_size) { return read_size < kSplitWideMin ? 16u : 64u; }
inline uint32_t split_parts_log2(uint32_t K, uint32_t read_size)
{
    const uint32_t units = K * (read_size / 8u);
    uint32_t lg = 0;
    while (lg < 6u && (units >> (lg + 1u)) >= kSplitShareUnits) ++lg;
    return lg;
}

#ifdef AIM_TU_SPLIT   // the kernel lives in tu_split.hip alone; capi_pipeline.hip sees the arguments and the launcher

static_assert(sizeof(aim_segment_t) == 8 && sizeof(aim_request_t) == 16 && sizeof(aim_chain_t) == 16, "rows as rule 10c lays them out");

template <int G>
__global__ __launch_bounds__(kSplitThreads) void split_segments_kernel(SplitArgs a)
{
    constexpr uint32_t kGroups = kSplitThreads / G;               // (read, share) items per workgroup
    const uint32_t sub = threadIdx.x & (G - 1u);
    const uint32_t parts = 1u << a.parts_log2;
    const uint64_t n_items = (uint64_t)a.n_reads << a.parts_log2;
    const uint64_t n_blocks = (n_items + kGroups - 1u) / kGroups;
    const uint32_t U = a.read_size >> 3;                          // units per row
    const uint32_t total = a.K * U;                               // units per read, at most 16 * 8 191
    const float inv_u = 1.0f / (float)U;
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t item = blk * kGroups + threadIdx.x / G;
        const bool item_live = item < n_items;
        const uint64_t r = item_live ? item >> a.parts_log2 : 0;
        const uint32_t part = (uint32_t)item & (parts - 1u);
        const bool live = item_live && sub < a.K;
        const uint64_t slot = r * a.K + sub;

        // ---- the decision: lane i < K of the group holds slot i ----
        int32_t L = 0, lo = 0, hi = 0;
        bool primary = false, minus = false;
        aim_chain_t c = {0u, 0, 0, 0, 0, 0u};
        aim_request_t rq = {0, 0, 0, 0u};
        uint64_t tp = 0;
        if (live) {
            const uint32_t n = min(a.seed[r].n_cands, a.K);
            L = min(max(a.read_len[r], 0), (int32_t)a.read_size);
            c = a.chains[slot];
            tp = a.text_pos[slot];
            rq = a.requests[slot];
            minus = (tp >> 63) != 0;
            lo = minus ? L - (int32_t)c.q_hi : (int32_t)c.q_lo;
            hi = minus ? L - (int32_t)c.q_lo : (int32_t)c.q_hi;
            primary = sub < n && (a.cls[slot].flags & AIM_CHAIN_PRIMARY) != 0;
        }
        bool left_open = true, right_open = true;
        for (uint32_t j = 0; j < a.K; ++j) {                      // (workgroup-uniform bound: every lane takes every shuffle)
            const int32_t lo_j = __shfl(lo, (int)j, G), hi_j = __shfl(hi, (int)j, G);
            const bool other = __shfl((int)primary, (int)j, G) != 0 && j != sub;
            left_open = left_open && !(other && lo_j < lo);
            right_open = right_open && !(other && hi_j > hi);
        }
        // the read interval, kept inside the read whatever the chain says (a malformed chain never makes an access outside the row)
        int32_t qa = left_open ? 0 : min(max(lo, 0), L);
        int32_t qb = right_open ? L : min(max(hi, qa), L);
        if (!primary) { qa = 0; qb = (int32_t)a.read_size; }      // every other slot: the whole read row
        if (live && part == 0) {
            aim_request_t o = {L, 0, 0, rq.idx};
            uint64_t otp = 0;
            uint32_t w0 = 0, w1 = 0;                              // aim_segment_t as its two dwords
            if (primary) {
                const int64_t start = (int64_t)(tp & ~AIM_REF_MINUS_STRAND), E = start + (int64_t)rq.text_len;
                const bool low_open = minus ? right_open : left_open, high_open = minus ? left_open : right_open;
                int64_t p_lo = 0;
                bool loose = false;
                if (start > 0) p_lo = start + (int64_t)c.q_lo + a.flank;
                else if (rq.text_len > 0 && rq.text_len < (int32_t)a.read_size && E < a.ref_len)
                    p_lo = E - ((int64_t)L - (int64_t)c.q_hi) - a.flank - (int64_t)c.ref_span;
                else loose = true;
                const int64_t p_hi = p_lo + (int64_t)c.ref_span;
                const int64_t seg_start = (low_open || loose) ? start : min(max(p_lo, (int64_t)0), a.ref_len);
                const int64_t seg_end = max(seg_start, (high_open || loose) ? E : min(max(p_hi, (int64_t)0), a.ref_len));
                o.pattern_len = qb - qa;
                o.text_len = (int32_t)min(seg_end - seg_start, (int64_t)a.read_size);
                otp = (uint64_t)seg_start | (minus ? AIM_REF_MINUS_STRAND : 0ull);
                const uint32_t flags = AIM_SEG_VALID | (sub ? AIM_SEG_SUPPLEMENTARY : 0u) | (left_open ? AIM_SEG_LEFT_OPEN : 0u) |
                                       (right_open ? AIM_SEG_RIGHT_OPEN : 0u) | (loose ? AIM_SEG_LOOSE : 0u);
                w0 = (uint32_t)qa | (uint32_t)qb << 16;
                w1 = (uint32_t)L | flags << 16 | sub << 24;
            }
            a.seg_requests[slot] = o;
            a.seg_text_pos[slot] = otp;
            reinterpret_cast<uint2 *>(a.seg)[slot] = make_uint2(w0, w1);   // (d_seg is 8-byte aligned: one dwordx2 store per row)
        }

        // ---- the rows: unit u of the read is bytes [8t, 8t + 8) of slot i's row, u = i * U + t ----
        const uint32_t span = (uint32_t)qa | (uint32_t)(qb - qa) << 16;   // (both at most 65 528)
        const uint32_t *src = reinterpret_cast<const uint32_t *>(a.reads + r * a.read_size);
        uint2 *dst = reinterpret_cast<uint2 *>(a.seg_patterns + r * a.K * a.read_size);
        for (uint32_t u0 = part * (uint32_t)G; u0 < total; u0 += parts * (uint32_t)G) {   // (uniform over the wavefront)
            const uint32_t u = u0 + sub;
            uint32_t i = (uint32_t)((float)u * inv_u);            // u < 2^17: exact in a float, the quotient off by one at the most
            i = min(i, a.K - 1u);
            int32_t t = (int32_t)(u - i * U);
            if (t < 0) { --i; t += (int32_t)U; } else if (t >= (int32_t)U && i + 1u < a.K) { ++i; t -= (int32_t)U; }
            const uint32_t sp = (uint32_t)__shfl((int)span, (int)i, G);
            if (!item_live || u >= total) continue;
            const uint32_t off = sp & 0xffffu, len = sp >> 16;
            const uint32_t at = off + 8u * (uint32_t)t;            // first source byte of the unit
            const uint32_t end = off + len;                       // one past the segment's last source byte, at most read_size
            const uint32_t w = at >> 2, sh = at & 3u;
            // only dwords that hold a byte of [off, end) are loaded, and those lie inside the row
            const uint32_t d0 = 4u * w < end ? src[w] : 0u;
            const uint32_t d1 = 4u * (w + 1u) < end ? src[w + 1u] : 0u;
            const uint32_t d2 = (sh && 4u * (w + 2u) < end) ? src[w + 2u] : 0u;
            uint2 v;
            v.x = __builtin_amdgcn_alignbyte(d1, d0, sh);
            v.y = __builtin_amdgcn_alignbyte(d2, d1, sh);
            const int32_t keep = (int32_t)len - 8 * t;            // bytes of the unit inside the segment; zero behind it
            if (keep < 8) {
                v.y = keep <= 4 ? 0u : (v.y & (0xffffffffu >> (8 * (8 - keep))));
                v.x = keep <= 0 ? 0u : keep >= 4 ? v.x : (v.x & (0xffffffffu >> (8 * (4 - keep))));
            }
            dst[u] = v;
        }
    }
}

void split_segments_launch(const SplitArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s)
{
    if (lanes == 16u) hipLaunchKernelGGL(split_segments_kernel<16>, dim3(grid), dim3(kSplitThreads), 0, s, a);
    else hipLaunchKernelGGL(split_segments_kernel<64>, dim3(grid), dim3(kSplitThreads), 0, s, a);
}
#else
void split_segments_launch(const SplitArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s);
#endif

}  // namespace aim
