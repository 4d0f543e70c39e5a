// extend.hpp -- the device side of AIM_FEATURE_EXTEND (aim_hip.h, rule 11c): the inner sides of split-read segments extended to the
// breakpoint by a score-only x-drop WFA, then the touched slots rewritten in place.
//
// extend_sides_kernel runs behind split_segments_kernel on its four outputs. A work item is (slot, side): item = 2 * slot + side.
// Nearly all items are dead (single-primary reads, empty slots, open sides), so a wavefront takes 64 consecutive items, lane i decides
// item i from its segment record, a ballot names the live ones and the wavefront runs those one after another: no atomics and no
// compaction, so no output byte depends on the grid. Every item's part of aim_extend_t has one writer, and the kernel writes nothing else.
//
// One side. Lane l holds diagonal k = l - band (band <= 31: 63 diagonals). The wavefront offsets are text offsets h in int16, kNull
// where a diagonal has no point; a point outside the matrix (h > m or h - k > n) is kNull, never clamped, and nothing is inherited
// from a start value. Levels step by g = gcd(x', o' + e', e'): no other cost occurs. The M ring holds the last max(x', o' + e') / g + 1
// levels and the I and D rings the last e' / g + 1, in LDS, one column of 64 entries per level; a lane reads and writes its own column
// only, and the k - 1 / k + 1 sources of I and D come by two cross-lane moves. Q and T are staged into LDS once per side with the
// reversal and the complement applied, so the match loop is the same for all four orientations. Per level one wave-wide maximum of
// (v + h, lowest diagonal) gives R, B and the result cell with rule 11c's ties; then the stop test, also for the levels the step skips.
// The level loop ends at max_cost at the latest.
// LDS indices: a ring row is a counter kept below the depth the host sized the ring with (ExtendArgs::dm, di); a column is the lane;
// Q and T are indexed below n <= max_ext and m <= max_ext + band, the capacities extend_plan() sizes them with.
//
// extend_apply_kernel: a wavefront takes 64 consecutive slots, lane i rewrites the two small records of slot i where its aim_extend_t
// is not zero, and the wavefront then copies each touched slot's pattern row from d_reads: a plain copy, one dword per lane and step.
// No LDS, no scratch, no atomics, vector stores only in both kernels.
// Measured: profiles/extend/README.md.
#pragma once

#include "aim_device.hpp"

namespace aim {

constexpr int kExtendMaxVgpr = 64;          // 8 wavefronts per SIMD; the bound tests/test_extend_cpu.py checks in the code object
constexpr int kExtendThreads = 64;          // extend_sides_kernel: one wavefront per workgroup (its LDS is the wavefront's own)
constexpr int kExtendApplyThreads = 256;
constexpr uint32_t kExtendApplyPerCu = 8;
constexpr uint32_t kExtendLdsPerCu = 128u * 1024u;   // what the resident grid of extend_sides_kernel may take of a CU's 160 KiB
constexpr int kExtendNull = -32640;         // 0x8080: both bytes 0x80, so that the rings are cleared with dword stores

struct ExtendArgs {
    uint32_t K, read_size, n_reads;
    int32_t match, xs, oes, es, g;          // a; x' / g, (o' + e') / g, e' / g; g
    int32_t xdrop2, max_cost, band, max_ext; // 2 Z (clamped where it can never fire)
    uint32_t dm, di;                        // rows of the M ring and of the I and D rings
    uint32_t q_cap, t_cap;                  // bytes of the staged Q and T
    uint32_t lds_bytes, dbg_poison_lds;
    int64_t ref_len;
    const int32_t *read_len;
    const char *reads;
    const char *ref;
    aim_request_t *seg_requests;
    uint64_t *seg_text_pos;
    char *seg_patterns;
    aim_segment_t *seg;
    aim_extend_t *ext;
};

inline int32_t extend_gcd(int32_t a, int32_t b) { while (b) { const int32_t t = a % b; a = b; b = t; } return a; }

// The transformed penalties, the level step, the ring depths and the LDS layout: functions of the parameters alone.
inline void extend_plan(const aim_extend_params_t &p, ExtendArgs &a)
{
    const int32_t x2 = 2 * (p.match + p.mismatch), o2 = 2 * p.gap_o, e2 = 2 * p.gap_e + p.match;
    a.g = extend_gcd(extend_gcd(x2, o2 + e2), e2);
    a.match = p.match; a.xs = x2 / a.g; a.oes = (o2 + e2) / a.g; a.es = e2 / a.g;
    a.xdrop2 = 2 * std::min(p.xdrop, 1 << 23);
    a.max_cost = p.max_cost; a.band = p.band; a.max_ext = p.max_ext;
    a.dm = (uint32_t)std::max(a.xs, a.oes) + 1u;
    a.di = (uint32_t)a.es + 1u;
    a.q_cap = ((uint32_t)p.max_ext + 3u) & ~3u;
    a.t_cap = ((uint32_t)(p.max_ext + p.band) + 3u) & ~3u;
    a.lds_bytes = (a.dm + 2u * a.di) * 128u + a.q_cap + a.t_cap;
}

#ifdef AIM_TU_EXTEND   // the kernels live in tu_extend.hip alone; capi_pipeline.hip sees the arguments and the launchers

static_assert(sizeof(aim_extend_t) == 24 && sizeof(aim_segment_t) == 8 && sizeof(aim_request_t) == 16, "rows as rule 11c lays them out");

extern __shared__ __attribute__((aligned(16))) char extend_smem[];

// AIM_FLAG_REF_TEXTS' complement of one byte: A <-> T, C <-> G in either case, every other byte kept.
__device__ __forceinline__ uint32_t extend_comp(uint32_t c)
{
    const uint32_t u = c & 0xDFu;
    return c ^ ((u == 0x41u || u == 0x54u) ? 0x15u : (u == 0x43u || u == 0x47u) ? 0x04u : 0u);
}

__global__ __launch_bounds__(kExtendThreads, 8) void extend_sides_kernel(ExtendArgs a)
{
    debug_poison_lds(a.dbg_poison_lds, a.lds_bytes, extend_smem);
    int16_t *Mr = reinterpret_cast<int16_t *>(extend_smem);
    int16_t *Ir = Mr + a.dm * 64u;
    int16_t *Dr = Ir + a.di * 64u;
    uint8_t *Q = reinterpret_cast<uint8_t *>(Dr + a.di * 64u);
    uint8_t *T = Q + a.q_cap;
    const uint32_t lane = threadIdx.x;
    const int32_t band = a.band;
    const int32_t k = (int32_t)lane - band;
    const bool diag_on = lane <= 2u * (uint32_t)band;             // (at most lanes 0..62: lane 63 never holds a point)
    const uint64_t n_items = (uint64_t)a.n_reads * a.K * 2u;
    const uint64_t n_groups = (n_items + 63u) / 64u;
    for (uint64_t grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
        // ---- the decision: lane i holds item i ----
        const uint64_t item = grp * 64u + lane;
        const uint64_t slot = item >> 1;
        const uint32_t side = (uint32_t)item & 1u;
        int32_t n_l = 0, m_l = 0;
        uint32_t how = 0;                                          // bit 0: Q runs down the row, bit 1: T runs down the reference, bit 2: minus
        uint64_t q_at = 0, t_at = 0;                               // where Q[0] lies in d_reads and T[0] in the reference
        if (item < n_items) {
            const uint2 sw = reinterpret_cast<const uint2 *>(a.seg)[slot];
            const uint32_t flags = (sw.y >> 16) & 0xffu;
            if ((flags & AIM_SEG_VALID) && !(flags & AIM_SEG_LOOSE) && !(flags & (side ? AIM_SEG_RIGHT_OPEN : AIM_SEG_LEFT_OPEN))) {
                const uint64_t r = slot / a.K;
                const int32_t L = min(max(a.read_len[r], 0), (int32_t)a.read_size);
                const int32_t qb = (int32_t)(sw.x & 0xffffu), qe = (int32_t)(sw.x >> 16);
                const int32_t tl = a.seg_requests[slot].text_len;
                const uint64_t tp = a.seg_text_pos[slot];
                const uint64_t start = tp & ~AIM_REF_MINUS_STRAND;
                const bool minus = (tp >> 63) != 0;
                if (qb <= qe && qe <= L && tl >= 0 && tl <= (int32_t)a.read_size && start + (uint64_t)tl <= (uint64_t)a.ref_len) {
                    const int32_t inner = ((flags & AIM_SEG_LEFT_OPEN) ? 0 : 1) + ((flags & AIM_SEG_RIGHT_OPEN) ? 0 : 1);
                    const bool up = (side != 0u) != minus;
                    n_l = side ? min(L - qe, a.max_ext) : min(qb, a.max_ext);
                    const int64_t room = up ? a.ref_len - (int64_t)(start + (uint64_t)tl) : (int64_t)start;
                    m_l = (int32_t)min((int64_t)min(n_l + band, ((int32_t)a.read_size - tl) / inner), room);
                    if (n_l <= 0 || m_l <= 0) n_l = m_l = 0;
                    how = (side ? 0u : 1u) | (up ? 0u : 2u) | (minus ? 4u : 0u);
                    q_at = r * a.read_size + (uint64_t)(side ? qe : qb - 1);          // (not read when n is 0)
                    t_at = up ? start + (uint64_t)tl : start - 1u;
                }
            }
        }
        uint64_t todo = __ballot(n_l > 0);
        uint32_t r_dq = 0, r_dr = 0, r_stop = 0;
        int32_t r_score = 0;
        while (todo) {                                             // (wave-uniform)
            const int src = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1u;
            const int32_t n = __builtin_amdgcn_readlane(n_l, src), m = __builtin_amdgcn_readlane(m_l, src);
            const uint32_t hw = (uint32_t)__builtin_amdgcn_readlane((int)how, src);
            const uint64_t qa = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)q_at, src) |
                                (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(q_at >> 32), src) << 32;
            const uint64_t ta = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)t_at, src) |
                                (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(t_at >> 32), src) << 32;
            // ---- stage Q and T, clear the rings ----
            __syncthreads();                                       // (the side before is done with Q and T)
            for (int32_t i = (int32_t)lane; i < n; i += 64) Q[i] = (uint8_t)a.reads[(hw & 1u) ? qa - (uint64_t)i : qa + (uint64_t)i];
            for (int32_t i = (int32_t)lane; i < m; i += 64) {
                const uint32_t c = (uint8_t)a.ref[(hw & 2u) ? ta - (uint64_t)i : ta + (uint64_t)i];
                T[i] = (uint8_t)((hw & 4u) ? extend_comp(c) : c);
            }
            uint32_t *ring = reinterpret_cast<uint32_t *>(Mr);
            for (uint32_t i = lane; i < (a.dm + 2u * a.di) * 32u; i += 64u) ring[i] = 0x80808080u;
            __syncthreads();
            // ---- the levels ----
            int32_t R = 0, best = 0, best_anti = 0, best_lane = band, stop = a.max_cost, last_alive = 0;
            uint32_t cur = 0, curi = 0;                            // the ring rows of level j: j mod dm, j mod di
            for (int32_t j = 0;; ++j) {
                const int32_t s = j * a.g;                         // (at most max_cost)
                int32_t h = kExtendNull, inew = kExtendNull, dnew = kExtendNull;
                if (j == 0) {
                    if (k == 0) h = 0;
                } else {
                    const uint32_t rx = cur >= (uint32_t)a.xs ? cur - (uint32_t)a.xs : cur + a.dm - (uint32_t)a.xs;
                    const uint32_t ro = cur >= (uint32_t)a.oes ? cur - (uint32_t)a.oes : cur + a.dm - (uint32_t)a.oes;
                    const uint32_t re = curi >= (uint32_t)a.es ? curi - (uint32_t)a.es : curi + a.di - (uint32_t)a.es;
                    const int32_t mx = Mr[rx * 64u + lane], mo = Mr[ro * 64u + lane], ie = Ir[re * 64u + lane], de = Dr[re * 64u + lane];
                    const int32_t from_i = __shfl_up(max(mo, ie), 1), from_d = __shfl_down(max(mo, de), 1);
                    inew = lane == 0u ? kExtendNull : from_i + 1;  // a text base more, from diagonal k - 1
                    dnew = lane == 63u ? kExtendNull : from_d;     // a read base more, from diagonal k + 1
                    h = mx + 1;
                    // a point is kept only inside the matrix and on a diagonal of the band
                    if (!(diag_on && inew >= 0 && inew <= m && inew - k <= n)) inew = kExtendNull;
                    if (!(diag_on && dnew >= 0 && dnew <= m && dnew - k <= n && dnew - k >= 0)) dnew = kExtendNull;
                    if (!(diag_on && h >= 0 && h <= m && h - k <= n)) h = kExtendNull;
                    h = max(h, max(inew, dnew));
                }
                if (h >= 0) {
                    int32_t v = h - k;
                    while (h < m && v < n && Q[v] == T[h]) { ++h; ++v; }
                }
                Mr[cur * 64u + lane] = (int16_t)h;
                Ir[curi * 64u + lane] = (int16_t)inew;
                Dr[curi * 64u + lane] = (int16_t)dnew;
                // the furthest point of the level, the lowest diagonal among equals
                int32_t key = h >= 0 ? (((2 * h - k) << 6) | (int32_t)(63u - lane)) : -1;
                for (int off = 32; off; off >>= 1) key = max(key, __shfl_xor(key, off));
                if (key >= 0) {
                    const int32_t anti = key >> 6, val = a.match * anti - s;
                    last_alive = j;
                    R = max(R, anti);
                    if (val > best) { best = val; best_anti = anti; best_lane = 63 - (key & 63); }
                }
                // the first level from s on at which the test fires, while R and B stay as they are
                const int32_t fire = max(s, a.match * R - best + a.xdrop2 + 1);
                const bool dead = j - last_alive >= (int32_t)a.dm - 1;    // no level can hold a point any more
                if (fire < s + a.g || dead) { stop = min(fire, a.max_cost); break; }
                if (s + a.g > a.max_cost) break;
                cur = cur + 1u == a.dm ? 0u : cur + 1u;
                curi = curi + 1u == a.di ? 0u : curi + 1u;
            }
            if ((int)lane == src) {
                const int32_t bh = (best_anti + best_lane - band) >> 1, bv = bh - (best_lane - band);
                r_dq = best > 0 ? (uint32_t)bv : 0u;
                r_dr = best > 0 ? (uint32_t)bh : 0u;
                r_score = best >> 1;
                r_stop = (uint32_t)stop;
            }
        }
        if (item < n_items) {
            aim_extend_t *e = a.ext + slot;
            e->dq[side] = (uint16_t)r_dq;
            e->dr[side] = (uint16_t)r_dr;
            e->stop[side] = (uint16_t)r_stop;
            e->pad[side] = 0;
            e->score[side] = r_score;
        }
    }
}

__global__ __launch_bounds__(kExtendApplyThreads) void extend_apply_kernel(ExtendArgs a)
{
    constexpr uint32_t kWaves = kExtendApplyThreads / 64u;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t n_slots = (uint64_t)a.n_reads * a.K;
    const uint64_t n_groups = (n_slots + 63u) / 64u;
    for (uint64_t grp = (uint64_t)blockIdx.x * kWaves + threadIdx.x / 64u; grp < n_groups; grp += (uint64_t)gridDim.x * kWaves) {
        const uint64_t slot = grp * 64u + lane;
        uint32_t span = 0;                                         // the new q_begin | the new length << 16
        bool touched = false;
        if (slot < n_slots) {
            const aim_extend_t e = a.ext[slot];
            const bool left = (e.dq[0] | e.dr[0]) != 0, right = (e.dq[1] | e.dr[1]) != 0;
            touched = left || right;
            if (touched) {
                const uint2 sw = reinterpret_cast<const uint2 *>(a.seg)[slot];
                aim_request_t rq = a.seg_requests[slot];
                const uint64_t tp = a.seg_text_pos[slot];
                const bool minus = (tp >> 63) != 0;
                int64_t start = (int64_t)(tp & ~AIM_REF_MINUS_STRAND), end = start + (int64_t)rq.text_len;
                // the side that ran up the reference moves seg_end, the other one seg_start: left runs up on the minus strand
                if (minus) { end += e.dr[0]; start -= e.dr[1]; } else { start -= e.dr[0]; end += e.dr[1]; }
                // (the sides kernel keeps both inside the read; the clamps only keep a foreign d_ext from leaving the row)
                const int32_t qb = max((int32_t)(sw.x & 0xffffu) - (int32_t)e.dq[0], 0);
                const int32_t qe = max(min((int32_t)(sw.x >> 16) + (int32_t)e.dq[1], (int32_t)a.read_size), qb);
                rq.pattern_len = qe - qb;
                rq.text_len = (int32_t)(end - start);
                a.seg_requests[slot] = rq;
                a.seg_text_pos[slot] = (uint64_t)start | (minus ? AIM_REF_MINUS_STRAND : 0ull);
                const uint32_t add = (left ? AIM_SEG_EXT_LEFT : 0u) | (right ? AIM_SEG_EXT_RIGHT : 0u);
                reinterpret_cast<uint2 *>(a.seg)[slot] = make_uint2((uint32_t)qb | (uint32_t)qe << 16, sw.y | add << 16);
                span = (uint32_t)qb | (uint32_t)(qe - qb) << 16;
            }
        }
        uint64_t todo = __ballot(touched);
        while (todo) {                                             // (wave-uniform)
            const int src = __ffsll((unsigned long long)todo) - 1;
            todo &= todo - 1u;
            const uint32_t sp = (uint32_t)__builtin_amdgcn_readlane((int)span, src);
            const uint32_t off = sp & 0xffffu, len = sp >> 16;
            const uint64_t s2 = grp * 64u + (uint32_t)src;
            const uint8_t *row = reinterpret_cast<const uint8_t *>(a.reads) + (s2 / a.K) * a.read_size + off;
            uint32_t *dst = reinterpret_cast<uint32_t *>(a.seg_patterns + s2 * a.read_size);
            for (uint32_t w = lane; w < a.read_size / 4u; w += 64u) {
                uint32_t v = 0;
                for (uint32_t b = 0; b < 4u; ++b)
                    if (4u * w + b < len) v |= (uint32_t)row[4u * w + b] << (8u * b);
                dst[w] = v;
            }
        }
    }
}

void extend_launch(const ExtendArgs &a, uint32_t grid_sides, uint32_t grid_apply, hipStream_t s)
{
    hipLaunchKernelGGL(extend_sides_kernel, dim3(grid_sides), dim3(kExtendThreads), a.lds_bytes, s, a);
    hipLaunchKernelGGL(extend_apply_kernel, dim3(grid_apply), dim3(kExtendApplyThreads), 0, s, a);
}
#else
void extend_launch(const ExtendArgs &a, uint32_t grid_sides, uint32_t grid_apply, hipStream_t s);
#endif

}  // namespace aim
