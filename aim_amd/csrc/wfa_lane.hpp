// wfa_lane.hpp -- short-read WFA / WFA-adaptive fast path: ONE PAIR PER LANE, 64 pairs per wavefront,
// everything after staging in registers.
//
// Same results as affine_wfa_compute (WFA/DPU-WRAM/dpu/wfa.c:342-379) for configurations whose
// wavefront structure is known at compile time: penalties (X, O, E) and a score cap MAXS are template
// parameters, so which scores have a wavefront, their [lo, hi] ranges and which of them carry I/D
// components (affine_wfa_compute_next, wfa.c:268-340) are constants; only the offsets are data.
// WFA-adaptive's reduction (wfa.c:69-140) needs a wavefront of >= 10 diagonals, which these shapes
// never reach (checked at compile time), so -DREDUCE is inert exactly as in the reference.
//
// Data path per wavefront of 64 pairs:
//   HBM --(LDS-DMA, 1 KiB per wave-instruction, no VGPRs; the next group's DMA goes out piece by piece
//   once the image is in registers: the P side between the P pack's steps, the T side and the request
//   thinned out over the T pack, the diagonal construction and two thirds of the score loop, so that each
//   of a CU's 8 waves has a load about to issue in every phase; all of it older than the result store,
//   which the loop top's counted wait leaves in flight -- where there is one: score-only {idx, score} results collect in an
//   LDS ring and leave eight groups at a time, in front of an iteration's DMA, AIM_LANE_RES_RING)--> linear LDS image --> each lane reads ITS row with
//   ds_read_b128 at compile-time offsets (row = odd number of 16-B slots: conflict-free), validates the
//   alphabet and packs 2 bits/base with v_dot4: pattern and text become RS/16 dwords each in VGPRs.
//   affine_wfa_extend (wfa.c:186-208) becomes bit-parallel: for diagonal k, D_k = P xor (T shifted by k
//   bases) is a mismatch bit-vector; extending from pattern position v is "first set bit at or after v",
//   clamped to min(plen, tlen - k).  No loop, no divergence, no memory access.
// Pairs containing anything but A/C/G/T (the reference compares raw bytes, host.c:126-127) cannot be
// packed.  When a wavefront holds at least one such pair (wave-uniform test), its mismatch bit-vectors are
// built from the RAW bytes instead (byte-wise P[v] != T[v+k], exact for any byte values) and everything
// downstream is unchanged -- no to-do list, no second kernel, no counter to reset between launches.
#pragma once

#include <cassert>
#include <utility>

#include "aim_device.hpp"

// ---- build-time knobs (A/B tested on MI355X) ------------------------------------
#ifndef AIM_LANE_MIN_WAVES
#define AIM_LANE_MIN_WAVES 1      // __launch_bounds__ 2nd argument: minimum waves per SIMD (caps VGPRs)
#endif
#ifndef AIM_LANE_FULLWAIT
#define AIM_LANE_FULLWAIT 0       // diagnostic: 1 = drain the whole VM queue at the loop top (round-1 behaviour) instead of the counted wait
#endif
#ifndef AIM_LANE_INTERLEAVE
#define AIM_LANE_INTERLEAVE 2     // where the next group's 15 LDS-DMA instructions (7 P + 7 T + 1 request at READ_SIZE 112) are issued:
#endif                            // 0 = one burst in front of the pack (round-1 structure); 1 = one piece after every pack step, all inside the
                                  // pack phase; 2 = P as in 1, T's pieces and the request piece thinned out over the T pack, the diagonal
                                  // construction and the score loop (LaneSpread), so that a wave has a load about to issue in every phase.
                                  // The CIGAR instantiation stays on 1 under 2 (measured 8-10 % slower on 2, profiles/lane_issue)
#ifndef AIM_LANE_SPREAD_PCT
#define AIM_LANE_SPREAD_PCT 67    // schedule 2: the share of the score loop's cells by which the last piece is out (LaneSpread; 100 / 67 / 33
#endif                            // measured, profiles/lane_issue: later pieces land later and the loop top waits for them)
#ifndef AIM_LANE_ASM_ROWS
#define AIM_LANE_ASM_ROWS 1       // 1 = the loop top's LDS reads (request, P rows, T rows) are one inline-asm statement the compiler does not see
#endif                            // (read_group): it otherwise puts s_waitcnt vmcnt(0) in front of them and undoes the counted wait (-2 %)
#ifndef AIM_LANE_NT_STORE
#define AIM_LANE_NT_STORE 0       // 1 = score-only result stores are nontemporal (measured +1 % slower on the direct store, NOTES A.1 item 6)
#endif
#ifndef AIM_LANE_RES_RING
#define AIM_LANE_RES_RING 8       // score-only {idx, score} (AIM_FLAG_RES8) results: K > 0 = the results of K full groups collect in an LDS ring
#endif                            // (ds_write_b64 per lane and group) and leave as K / 2 global_store_dwordx4 at the top of the following iteration,
                                  // in front of that iteration's DMA; 0 = one global_store_dwordx2 per lane and group. 0, 4 or 8 (LDS: 512 B per slot;
                                  // K <= 10 keeps AIM_LANE_WGS_PER_CU workgroups on a CU). 8 with sc1 stores: -5.6 % (profiles/lane_store); 8 with
                                  // plain stores or sc1 without the ring: nothing in production; 4 did not pass the stream + store floor
#ifndef AIM_LANE_STORE_X4
#define AIM_LANE_STORE_X4 0       // direct {idx, score} store: 1 = lane pairs exchange their results (DPP) and the even lanes store 16 B
#endif                            // (measured: nothing, with or without sc1, profiles/lane_store)
#ifndef AIM_LANE_STORE_SC1
#define AIM_LANE_STORE_SC1 1      // cache policy sc1 instead of plain: 1 = on the {idx, score} stores (direct and ring), 2 = also on the default layout's two
#endif                            // (2 measured on the default-layout row: see profiles/lane_store)
#ifndef AIM_LANE_PACK_X2
#define AIM_LANE_PACK_X2 0        // 1 = pack from 2 * code (no per-dword shift); off until measured and parity-checked on the GPU
#endif
#ifndef AIM_LANE_STAMPS
#define AIM_LANE_STAMPS 0         // diagnostic build only: s_memtime per segment, summed per wave into scratch
#endif
#ifndef AIM_LANE_DIAG
#define AIM_LANE_DIAG 0           // diagnostic builds only (results are wrong): 1 = stop after the row loads + next DMA issue,
#endif                            // 2 = stop after pack/validate, 3 = everything but the result store, 4 = 1 without the result store
#ifndef AIM_LANE_RES_STAGE
#define AIM_LANE_RES_STAGE 1     // CIGAR instantiation only: results of a full group staged in LDS, stored as coalesced 16-B pieces
#endif
#ifndef AIM_LANE_DMA_AUX
#define AIM_LANE_DMA_AUX 2        // cache policy of the sequence DMA: 2 = nt (rows are read exactly once; +5 % measured), 0 = default
#endif
#ifndef AIM_LANE_WGS_PER_CU
#define AIM_LANE_WGS_PER_CU 8     // persistent single-wave workgroups per CU = resident waves at this VGPR count
                                  // (a grid larger than the residency runs in uneven rounds: 11/CU measured 15-20 % slower)
#endif
// slots of the result ring that kernel and plan agree on (the diagnostic builds without a result store have none)
#define AIM_LANE_RING_SLOTS ((AIM_LANE_DIAG == 3 || AIM_LANE_DIAG == 4) ? 0 : AIM_LANE_RES_RING)
#if AIM_LANE_STAMPS
#define AIM_STAMP(i) do { unsigned long long t_; __builtin_amdgcn_sched_barrier(0); \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); __builtin_amdgcn_sched_barrier(0); \
        stamp_sum[i] += t_ - stamp_last; stamp_last = t_; } while (0)
#else
#define AIM_STAMP(i) do { } while (0)
#endif

namespace aim {

constexpr int kLaneNull = -16384;   // AFFINE_WAVEFRONT_OFFSET_NULL (common.h:100)

// Compile-time wavefront structure (affine_wfa_compute_next bounds logic, wfa.c:272-335, without
// reduction; klo/khi == lo/hi).
template <int X, int O, int E, int MAXS>
struct WfShape {
    bool present[MAXS + 1];
    bool hasI[MAXS + 1];
    bool hasD[MAXS + 1];
    int lo[MAXS + 1];
    int hi[MAXS + 1];
    int kmin, kmax, maxw;
    constexpr WfShape() : present{}, hasI{}, hasD{}, lo{}, hi{}, kmin(0), kmax(0), maxw(1)
    {
        present[0] = true;
        for (int s = 1; s <= MAXS; ++s) {
            const int ss = s - X, so = s - O - E, se = s - E;
            const bool m_sub_null = ss < 0 || !present[ss];
            const bool m_o_null = so < 0 || !present[so];
            const bool i_e_null = se < 0 || !present[se] || !hasI[se];
            const bool d_e_null = se < 0 || !present[se] || !hasD[se];
            const bool i_out_null = m_o_null && i_e_null;
            const bool d_out_null = m_o_null && d_e_null;
            if (m_sub_null && i_out_null && d_out_null) continue;
            const int sub_lo = m_sub_null ? 1 : lo[ss], sub_hi = m_sub_null ? -1 : hi[ss];
            const int o_lo = m_o_null ? 1 : lo[so], o_hi = m_o_null ? -1 : hi[so];
            const bool e_none = i_e_null && d_e_null;
            const int e_lo = e_none ? 1 : lo[se], e_hi = e_none ? -1 : hi[se];
            int l = sub_lo < o_lo ? sub_lo : o_lo;
            l = (l < e_lo ? l : e_lo) - 1;
            int h = sub_hi > o_hi ? sub_hi : o_hi;
            h = (h > e_hi ? h : e_hi) + 1;
            present[s] = true;
            hasI[s] = !i_out_null;
            hasD[s] = !d_out_null;
            lo[s] = l;
            hi[s] = h;
            if (l < kmin) kmin = l;
            if (h > kmax) kmax = h;
            if (h - l + 1 > maxw) maxw = h - l + 1;
        }
    }
};

// Where the cells of a shape's wavefronts live in a per-lane history column (wfa_scores_dynamic<HIST>): row s of M starts at
// m[s] (cell of diagonal lo[s]), I at i[s], D at d[s]; after them 3 descriptor words per score (klo, khi, flags) at meta + 3 s.
template <int X, int O, int E, int MAXS>
struct WfHist {
    int m[MAXS + 1], i[MAXS + 1], d[MAXS + 1];
    int meta, total;
    constexpr WfHist() : m{}, i{}, d{}, meta(0), total(0)
    {
        constexpr WfShape<X, O, E, MAXS> SH{};
        int at = 0;
        for (int s = 0; s <= MAXS; ++s) {
            const int w = SH.present[s] ? SH.hi[s] - SH.lo[s] + 1 : 0;
            m[s] = at; at += w;
            i[s] = at; at += (SH.present[s] && SH.hasI[s]) ? w : 0;
            d[s] = at; at += (SH.present[s] && SH.hasD[s]) ? w : 0;
        }
        meta = at;
        total = at + 3 * (MAXS + 1);
    }
};
enum { LF_PRESENT = 1, LF_MNULL = 2, LF_INULL = 4, LF_DNULL = 8, LF_HASI = 16, LF_HASD = 32 };   // = wfa_group.hpp's GF_*

// first set flag at or after pattern position v in a 2-bit-per-base flag vector (flags on even bits)
template <int NP>
__device__ __forceinline__ int first_stop(const uint32_t (&m)[NP], int v)
{
    const int wi = v >> 4;
    const uint32_t lowmask = ~0u << ((v & 15) * 2);
    int res = NP * 16;
#pragma unroll
    for (int j = NP - 1; j >= 0; --j) {
        uint32_t mj = m[j];
        mj = (j == wi) ? (mj & lowmask) : mj;
        mj = (j < wi) ? 0u : mj;
        const int pos = j * 16 + (__builtin_ctz(mj | 0x80000000u) >> 1);
        res = mj ? pos : res;
    }
    return res;
}

// LDS-DMA destinations are given as BYTE OFFSETS into the workgroup's LDS (what M0 carries), not as generic pointers:
// a generic->LDS pointer cast inside the loop costs a null check and a select per instruction.
typedef __attribute__((address_space(3))) void *lds_ptr_t;
__device__ __forceinline__ lds_ptr_t lds_at(uint32_t byte_off) { return (lds_ptr_t)(uintptr_t)byte_off; }

// One 64-pair group of one sequence array, HBM -> LDS, by LDS-DMA (global_load_lds_dwordx4): the group's rows are
// contiguous in HBM ([64][RS] bytes), so NCH wave-instructions of 1 KiB copy them verbatim; no VGPR is used and the copy
// stays in flight while the wave computes. Full groups (all but the batch's last) issue the NCH pieces back to back with
// no predicate (the per-piece exec-mask test of round 1 cost ~10 scalar instructions and a branch per piece: "DMA issue"
// was 21 % of the loop); lanes past the batch tail are masked in the last group only.
// piece I of a full group: the instruction's immediate offset advances the global AND the LDS address, so pieces 0..3 share
// one (address, M0) pair and pieces 4..7 the next (+4 KiB)
template <int... I>
__device__ __forceinline__ void dma_full_pieces(uint32_t lds_off, const char *g_lane, std::integer_sequence<int, I...>)
{
    (__builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(g_lane + (I >> 2) * 4096),
                                      lds_at(lds_off + (I >> 2) * 4096), 16, (I & 3) * 1024, AIM_LANE_DMA_AUX), ...);
}

template <int I>
__device__ __forceinline__ void dma_piece(uint32_t lds_off, const char *g_lane)
{
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(g_lane + (I >> 2) * 4096),
                                      lds_at(lds_off + (I >> 2) * 4096), 16, (I & 3) * 1024, AIM_LANE_DMA_AUX);
    __builtin_amdgcn_sched_barrier(0);   // stays where it is written: between two pack steps
}

// Schedule 2 (AIM_LANE_INTERLEAVE == 2): where the NP + 1 pieces of the T side (NP row pieces, then the request piece) go. The
// places a piece can go to ("slots") are counted in program order: slot j + 1 follows the T pack's step j, slot NP + 1 the diagonal
// construction, and one slot follows every cell (score, diagonal) of the score loop. due(slot) pieces are out once that slot has
// passed: an even hand-out that ends at the cell which closes PCT percent of the score loop.
template <int X, int O, int E, int MAXS, int NP, int PCT>
struct LaneSpread {
    int cells, last;
    constexpr LaneSpread() : cells(0), last(0)
    {
        constexpr WfShape<X, O, E, MAXS> SH{};
        for (int s = 0; s <= MAXS; ++s) cells += SH.present[s] ? SH.hi[s] - SH.lo[s] + 1 : 0;
        const int c = (cells * PCT + 99) / 100;
        last = NP + 1 + (c < 1 ? 1 : c);
    }
    constexpr int due(int slot) const { return slot >= last ? NP + 1 : (slot * (NP + 1)) / last; }
};

// f(integral_constant<int, I>) for from <= I < to. Both bounds are constants wherever this is called (an unrolled loop's slot
// number run through LaneSpread::due), so what is left is the pieces themselves: no test, no branch.
template <typename F, int... I>
__device__ __forceinline__ void lane_pieces(int from, int to, F &f, std::integer_sequence<int, I...>)
{
    ((I >= from && I < to ? f(std::integral_constant<int, I>{}) : void()), ...);
}
// f for every piece from `first` on: one jump on a wave-uniform counter into an unrolled run (the score loop leaves early when
// every pair of the wave has finished; what it had not issued by then goes out here), not a test per piece.
template <int N, typename F>
__device__ __forceinline__ void lane_pieces_from(int first, F &f)
{
    static_assert(N <= 8, "one case per piece");
    switch (first) {
    case 0: if constexpr (0 < N) f(std::integral_constant<int, 0>{}); [[fallthrough]];
    case 1: if constexpr (1 < N) f(std::integral_constant<int, 1>{}); [[fallthrough]];
    case 2: if constexpr (2 < N) f(std::integral_constant<int, 2>{}); [[fallthrough]];
    case 3: if constexpr (3 < N) f(std::integral_constant<int, 3>{}); [[fallthrough]];
    case 4: if constexpr (4 < N) f(std::integral_constant<int, 4>{}); [[fallthrough]];
    case 5: if constexpr (5 < N) f(std::integral_constant<int, 5>{}); [[fallthrough]];
    case 6: if constexpr (6 < N) f(std::integral_constant<int, 6>{}); [[fallthrough]];
    case 7: if constexpr (7 < N) f(std::integral_constant<int, 7>{}); [[fallthrough]];
    default: break;
    }
}

template <int RS, int NCH>
__device__ __forceinline__ void dma_rows(uint32_t lds_off, const char *base, uint32_t pair0, uint32_t n_pairs, int lane)
{
    const char *g = base + (uint64_t)pair0 * RS;
    if (pair0 + kWave <= n_pairs) {   // wave-uniform
        dma_full_pieces(lds_off, g + (uint32_t)lane * 16u, std::make_integer_sequence<int, NCH>{});
    } else {
        const uint32_t rows = n_pairs - pair0;
        const uint32_t n_chunks = (rows * RS + 15) / 16;   // arrays carry >= 16 B of tail slack (aim_hip.h)
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const uint32_t c = i * kWave + lane;
            if (c < n_chunks)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(g + (uint64_t)c * 16),
                                                 lds_at(lds_off + i * kWave * 16), 16, 0, AIM_LANE_DMA_AUX);
        }
    }
}

// The group's 64 request descriptors, HBM -> LDS, by LDS-DMA like the rows (one wave-instruction for a full group), so the
// loop holds NO ordinary global load: a register-destination load makes the compiler put s_waitcnt vmcnt(0) in front of the
// next write of its destination register -- on every path that reaches it, the steady-state one included -- and that queue also
// holds the previous group's result store: waiting for a store's acknowledgement (~1-2 us under load) once per group is what
// the "residual wait" of round 1 was. The batch's last, partial group copies its requests dword by dword (no slack behind the
// request array is needed), into the same LDS slots.
__device__ __forceinline__ void stage_requests(uint32_t lds_off, const KArgs &a, uint32_t pair0, int lane)
{
    const uint32_t rqb = (a.p.flags & AIM_FLAG_REQ8) ? 8u : 16u;            // bytes per request
    const char *g = reinterpret_cast<const char *>(a.req) + (uint64_t)pair0 * rqb;
    if (pair0 + kWave <= a.n_pairs) {
        if ((uint32_t)lane * 16u < kWave * rqb)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(g + (uint64_t)lane * 16),
                                             lds_at(lds_off), 16, 0, 0);
    } else {
        const uint32_t n_dw = (a.n_pairs - pair0) * (rqb / 4u);             // <= 64 * 4
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t c = i * kWave + lane;
            if (c < n_dw)
                __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(g + (uint64_t)c * 4),
                                                 lds_at(lds_off + i * kWave * 4), 4, 0, 0);
        }
    }
}

typedef uint32_t lane_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t lane_u32x2 __attribute__((ext_vector_type(2)));

// Where a lane's staged request lies: 8 bytes {plen | tlen << 16, idx} (REQ8), or 16 bytes {plen, tlen, -, idx}. Read as one
// 8-byte word at `lo` and one dword at `hi`, so that both layouts take the same instructions (REQ8 reads idx twice).
struct LaneReqAddr { uint32_t lo, hi; };
__device__ __forceinline__ LaneReqAddr staged_request_addr(uint32_t lds_req_off, const KArgs &a, int lane)
{
    const bool r8 = a.p.flags & AIM_FLAG_REQ8;
    LaneReqAddr q;
    q.lo = lds_req_off + (uint32_t)lane * (r8 ? 8u : 16u);
    q.hi = q.lo + (r8 ? 4u : 12u);
    return q;
}
__device__ __forceinline__ aim_request_t decode_staged_request(const lane_u32x2 &lo, uint32_t hi, const KArgs &a)
{
    aim_request_t r;
    r.padding = 0; r.idx = hi;
    if (a.p.flags & AIM_FLAG_REQ8) { r.pattern_len = (int16_t)(lo.x & 0xffffu); r.text_len = (int16_t)(lo.x >> 16); }
    else { r.pattern_len = (int)lo.x; r.text_len = (int)lo.y; }
    return r;
}

// The loop top's LDS reads: this lane's request and its two rows, 16 B at a time at compile-time offsets (RS/16 odd =>
// ds_read_b128 is conflict-free), all back when this returns.
// They are ONE inline-asm statement on purpose. The compiler knows that LDS-DMA writes LDS and orders every ds_read it emits
// behind every LDS-DMA that may still be in flight; where paths with and without a result store meet (the loop top) it can
// only do that with s_waitcnt vmcnt(0), which also waits for the previous group's result store -- the acknowledgement latency
// the counted wait at the loop top exists to avoid, paid once per group (stamped: 2 050 of 10 500 ticks per group sat in front
// of the row reads). Reads it does not see it does not guard; the kernel's own counted vmcnt wait in front of this call is what
// orders them behind the DMA. The reads and their lgkmcnt wait share the statement (early-clobber outputs) so that no register
// is visible to the compiler, for a copy or a spill, before its data has landed.
template <int RS, int NP>
__device__ __forceinline__ void read_group(const LaneReqAddr &qa, uint32_t row_addr, lane_u32x2 &q_lo, uint32_t &q_hi,
                                           lane_u32x4 (&P)[NP], lane_u32x4 (&T)[NP])
{
    static_assert(NP == 5 || NP == 7, "READ_SIZE 80 or 112");
#if AIM_LANE_ASM_ROWS
    if constexpr (NP == 7) {
        asm volatile("ds_read_b64 %0, %[qlo]\n\tds_read_b32 %1, %[qhi]\n\t"
                     "ds_read_b128 %2, %[row]\n\tds_read_b128 %3, %[row] offset:16\n\tds_read_b128 %4, %[row] offset:32\n\t"
                     "ds_read_b128 %5, %[row] offset:48\n\tds_read_b128 %6, %[row] offset:64\n\tds_read_b128 %7, %[row] offset:80\n\t"
                     "ds_read_b128 %8, %[row] offset:96\n\t"
                     "ds_read_b128 %9, %[row] offset:%c[tb]\n\tds_read_b128 %10, %[row] offset:%c[tb]+16\n\tds_read_b128 %11, %[row] offset:%c[tb]+32\n\t"
                     "ds_read_b128 %12, %[row] offset:%c[tb]+48\n\tds_read_b128 %13, %[row] offset:%c[tb]+64\n\tds_read_b128 %14, %[row] offset:%c[tb]+80\n\t"
                     "ds_read_b128 %15, %[row] offset:%c[tb]+96\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(q_lo), "=&v"(q_hi), "=&v"(P[0]), "=&v"(P[1]), "=&v"(P[2]), "=&v"(P[3]), "=&v"(P[4]), "=&v"(P[5]), "=&v"(P[6]),
                       "=&v"(T[0]), "=&v"(T[1]), "=&v"(T[2]), "=&v"(T[3]), "=&v"(T[4]), "=&v"(T[5]), "=&v"(T[6])
                     : [qlo] "v"(qa.lo), [qhi] "v"(qa.hi), [row] "v"(row_addr), [tb] "n"(kWave * RS)
                     : "memory");
    } else {
        asm volatile("ds_read_b64 %0, %[qlo]\n\tds_read_b32 %1, %[qhi]\n\t"
                     "ds_read_b128 %2, %[row]\n\tds_read_b128 %3, %[row] offset:16\n\tds_read_b128 %4, %[row] offset:32\n\t"
                     "ds_read_b128 %5, %[row] offset:48\n\tds_read_b128 %6, %[row] offset:64\n\t"
                     "ds_read_b128 %7, %[row] offset:%c[tb]\n\tds_read_b128 %8, %[row] offset:%c[tb]+16\n\tds_read_b128 %9, %[row] offset:%c[tb]+32\n\t"
                     "ds_read_b128 %10, %[row] offset:%c[tb]+48\n\tds_read_b128 %11, %[row] offset:%c[tb]+64\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(q_lo), "=&v"(q_hi), "=&v"(P[0]), "=&v"(P[1]), "=&v"(P[2]), "=&v"(P[3]), "=&v"(P[4]),
                       "=&v"(T[0]), "=&v"(T[1]), "=&v"(T[2]), "=&v"(T[3]), "=&v"(T[4])
                     : [qlo] "v"(qa.lo), [qhi] "v"(qa.hi), [row] "v"(row_addr), [tb] "n"(kWave * RS)
                     : "memory");
    }
#else
    typedef const __attribute__((address_space(3))) lane_u32x4 *lds_row_t;
    q_lo = *reinterpret_cast<const __attribute__((address_space(3))) lane_u32x2 *>((uintptr_t)qa.lo);
    q_hi = *reinterpret_cast<const __attribute__((address_space(3))) uint32_t *>((uintptr_t)qa.hi);
#pragma unroll
    for (int j = 0; j < NP; ++j) P[j] = reinterpret_cast<lds_row_t>((uintptr_t)row_addr)[j];
#pragma unroll
    for (int j = 0; j < NP; ++j) T[j] = reinterpret_cast<lds_row_t>((uintptr_t)(row_addr + kWave * RS))[j];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
}

// The score-only {idx, score} result stores, 8 B (one lane's result) and 16 B (two neighbouring results). AIM_LANE_STORE_SC1: with
// the sc1 cache policy, which only an inline-asm statement can ask for (the s_nop covers the wait state between a store of more
// than 64 bits and the next write of its data registers, which the compiler cannot see to here).
__device__ __forceinline__ void lane_store8(void *dst, const lane_u32x2 &v)
{
#if AIM_LANE_STORE_SC1
    asm volatile("global_store_dwordx2 %0, %1, off sc1" :: "v"(dst), "v"(v) : "memory");
#else
    if (AIM_LANE_NT_STORE) __builtin_nontemporal_store(v, reinterpret_cast<lane_u32x2 *>(dst)); else *reinterpret_cast<lane_u32x2 *>(dst) = v;
#endif
}
__device__ __forceinline__ void lane_store16(void *dst, const lane_u32x4 &v)
{
#if AIM_LANE_STORE_SC1
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" :: "v"(dst), "v"(v) : "memory");
#else
    if (AIM_LANE_NT_STORE) __builtin_nontemporal_store(v, reinterpret_cast<lane_u32x4 *>(dst)); else *reinterpret_cast<lane_u32x4 *>(dst) = v;
#endif
}

// The result ring (AIM_LANE_RES_RING = K slots of 64 x {idx, score} behind the request slots). Both of its LDS accesses are
// inline-asm statements for read_group's reason: an LDS access the compiler emits gets s_waitcnt vmcnt(0) in front of it while
// LDS-DMA may be in flight -- the write at the end of an iteration would drain the next group's 15 pieces once per group, a
// read in the flush the stores in front of it. Neither touches the rows or requests the DMA writes, so no order is needed.
__device__ __forceinline__ void ring_put(uint32_t lds_addr, uint32_t idx, uint32_t score)
{
    lane_u32x2 v; v.x = idx; v.y = score;
    asm volatile("ds_write_b64 %0, %1\n\ts_waitcnt lgkmcnt(0)" :: "v"(lds_addr), "v"(v) : "memory");
}
// The first `count` slots leave as 16-B stores: lane l carries results 2 (l & 31) and 2 (l & 31) + 1 of slot 2 q + (l >> 5) in
// store q, so one instruction covers two slots (two groups, 512 contiguous bytes each) and the LDS read is linear, 16 B per lane.
// lds_lane = ring + 16 lane; dst_lane = the lane's 16 bytes in the group of slot (lane >> 5); step = bytes from slot s to s + 2.
// Only full groups enter the ring, so no store reaches beyond its group's 512 bytes (the result array has no slack).
template <int K, bool FULL>
__device__ __forceinline__ void ring_flush(uint32_t lds_lane, char *dst_lane, uint64_t step, uint32_t count, int lane)
{
    static_assert(K == 4 || K == 8, "two slots per store instruction");
    lane_u32x4 v[K / 2];
    if constexpr (K == 8) {
        asm volatile("ds_read_b128 %0, %4\n\tds_read_b128 %1, %4 offset:1024\n\tds_read_b128 %2, %4 offset:2048\n\tds_read_b128 %3, %4 offset:3072\n\t"
                     "s_waitcnt lgkmcnt(0)"
                     : "=&v"(v[0]), "=&v"(v[1]), "=&v"(v[2]), "=&v"(v[3]) : "v"(lds_lane) : "memory");
    } else {
        asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:1024\n\ts_waitcnt lgkmcnt(0)"
                     : "=&v"(v[0]), "=&v"(v[1]) : "v"(lds_lane) : "memory");
    }
#pragma unroll
    for (int q = 0; q < K / 2; ++q) {
        if (FULL || 2u * q + ((uint32_t)lane >> 5) < count) {   // FULL: count == K, no lane is masked
            lane_store16(dst_lane + q * step, v[q]);
        }
    }
}

// Validate A/C/G/T over [0, len) and pack 2 bits/base: 16 bases -> one dword. `after_step(integral_constant<int, j>)` runs
// after the j-th 16-base step (the kernel issues one piece of the next group's DMA there).
// MASKED = false: every byte of the step lies inside the sequence of EVERY lane (the caller proved it wave-wide), so the
// bytes are compared unmasked and the differences accumulate with v_sad_u8 (one op instead of xor + and + or).
// MASKED = true: per-lane byte masks from the length. The choice is a TEMPLATE argument on purpose: as a run-time (even
// wave-uniform) test per dword it compiled to two scalar branches per dword -- 112 per group -- and the pack phase ran at
// less than a quarter of its issue rate.
template <int J, bool MASKED, int NP, typename StepF>
__device__ __forceinline__ void pack_step(const lane_u32x4 (&raw)[NP], int len, uint32_t (&out)[NP], uint32_t &bad, StepF &after_step)
{
    const uint32_t a[4] = {raw[J].x, raw[J].y, raw[J].z, raw[J].w};
    uint32_t b[4];
#if AIM_LANE_PACK_X2
    // One instruction less per dword: keep the 2-bit codes where they sit in the byte (bits 1..2, i.e. 2*code, no shift), decode
    // back through a table indexed by 2*code, and let v_dot4 produce 2 * (c0 + 4 c1 + 16 c2 + 64 c3); the factor 2 is removed once
    // per 16 bases when the four 9-bit pieces are joined (they are even, so OR-ing them at a distance of 8 bits cannot collide).
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t t2 = a[i] & 0x06060606u;                                    // 2 * code per byte: A0 C2 T4 G6
        const uint32_t rec = __builtin_amdgcn_perm(0x00470054u, 0x00430041u, t2);  // "A.C." | "T.G." indexed by 2 * code
        if (MASKED) {
            const int rem = len - 4 * (4 * J + i);
            const uint32_t mask = rem >= 4 ? ~0u : (rem <= 0 ? 0u : ((1u << (8 * rem)) - 1u));
            bad |= (rec ^ a[i]) & mask;
        } else {
            bad = __builtin_amdgcn_sad_u8(rec, a[i], bad);
        }
        b[i] = __builtin_amdgcn_udot4(t2, 0x40100401u, 0u, false);                 // 2 * packed byte, <= 510
    }
    out[J] = ((b[0] | (b[1] << 8) | (b[2] << 16)) >> 1) | (b[3] << 23);
#else
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t t = (a[i] >> 1) & 0x03030303u;                    // 2-bit code per byte: A0 C1 T2 G3
        const uint32_t rec = __builtin_amdgcn_perm(0u, 0x47544341u, t);  // decode back: "ACTG"[code]
        if (MASKED) {
            const int rem = len - 4 * (4 * J + i);
            const uint32_t mask = rem >= 4 ? ~0u : (rem <= 0 ? 0u : ((1u << (8 * rem)) - 1u));
            bad |= (rec ^ a[i]) & mask;
        } else {
            bad = __builtin_amdgcn_sad_u8(rec, a[i], bad);
        }
        b[i] = __builtin_amdgcn_udot4(t, 0x40100401u, 0u, false);       // c0 + 4 c1 + 16 c2 + 64 c3
    }
    out[J] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
#endif
    after_step(std::integral_constant<int, J>{});
}
// FAST: steps 0 .. NP-2 unmasked (requires len >= 16*(NP-1) for every lane of the wave), last step masked; else all masked.
template <bool FAST, int NP, typename StepF, int... J>
__device__ __forceinline__ uint32_t pack_row_seq(const lane_u32x4 (&raw)[NP], int len, uint32_t (&out)[NP], StepF &after_step,
                                                 std::integer_sequence<int, J...>)
{
    uint32_t bad = 0;
    (pack_step<J, (!FAST || J == NP - 1), NP>(raw, len, out, bad, after_step), ...);
    return bad;
}
template <bool FAST, int NP, typename StepF>
__device__ __forceinline__ uint32_t pack_row(const lane_u32x4 (&raw)[NP], int len, uint32_t (&out)[NP], StepF after_step)
{
    return pack_row_seq<FAST, NP>(raw, len, out, after_step, std::make_integer_sequence<int, NP>{});
}

enum : uint32_t { LANE_TODO_COUNT = 0, LANE_TODO_LIST = 16 };   // dword offsets inside the to-do region (wfa_group.hpp only)

// Mismatch flags of diagonal k straight from the raw rows, for ANY byte values: bit 2i of out[j] is set
// <=> P[16j+i] != T[16j+i+k] (the layout first_stop() scans; the packed path sets one or both bits of a pair).
// Cold path: only run for wavefronts that hold a pair with a byte outside A/C/G/T.
template <int NP>
__device__ __forceinline__ void raw_diag(const lane_u32x4 (&rawP)[NP], const lane_u32x4 (&rawT)[NP], int k, uint32_t (&out)[NP])
{
    uint32_t pw[4 * NP], tw[4 * NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        pw[4 * j] = rawP[j].x; pw[4 * j + 1] = rawP[j].y; pw[4 * j + 2] = rawP[j].z; pw[4 * j + 3] = rawP[j].w;
        tw[4 * j] = rawT[j].x; tw[4 * j + 1] = rawT[j].y; tw[4 * j + 2] = rawT[j].z; tw[4 * j + 3] = rawT[j].w;
    }
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        uint32_t b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int w = 4 * j + i;
            const int o = 4 * w + k;                              // byte offset of T[4w + k]
            const int wi = (o >= 0) ? (o >> 2) : -((-o + 3) >> 2);   // floor(o / 4)
            const int sh = o - 4 * wi;                            // 0..3
            const uint32_t lo = (wi >= 0 && wi < 4 * NP) ? tw[wi] : 0u;
            const uint32_t hi = (wi + 1 >= 0 && wi + 1 < 4 * NP) ? tw[wi + 1] : 0u;
            const uint32_t ts = sh ? __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)sh) : lo;
            const uint32_t x = pw[w] ^ ts;
            const uint32_t nz = ((((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) >> 7) & 0x01010101u;   // 1 per non-zero byte
            b[i] = __builtin_amdgcn_udot4(nz, 0x40100401u, 0u, false);
        }
        out[j] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
    }
}



// ---------------------------------------------------------------------------------------------------
// Shapes whose wavefronts can reach the 10 diagonals at which WFA-adaptive's reduction applies (wfa.c:69-140), e.g. the
// launcher's MAX_SCORE 10 for l = 100, e = 2 % -- the configuration that fell off a 10x cliff onto wfa_group_kernel in
// round 1. The score loop stays statically unrolled over the NON-reduced shape, which is a superset of every reduced one
// (a reduction only raises klo / lowers khi, and a wavefront's bounds are min/max over its sources' bounds). What the
// reduction makes data-dependent -- klo, khi, the null flags, and through them which wavefronts exist -- is carried per
// lane in ordinary variables: for every score below the first reducible one they are compile-time constants and fold
// away, above it they are a handful of integer selects. Every fetch is range-gated by the source's klo/khi exactly like
// AFFINE_WAVEFRONT_COND_FETCH (common.h:121-124), so cells of the static superset that the reference never allocates are
// computed but never read. Score-only (with CIGAR the history of a 13-wide shape does not fit the register file).
// HIST: every computed cell (after extension) and every score's final descriptor are also written to this lane's history
// column hist[i * kWave] (int16, lane-interleaved LDS) for wfa_backtrace_dynamic.
// on_cell() runs after every extended cell, in program order (wfa_lane_kernel's schedule 2 hands out LDS-DMA pieces there).
struct LaneNoCell { __device__ __forceinline__ void operator()() const {} };
template <int X, int O, int E, int MAXS, int NP, int KW, bool HIST = false, typename CellF = LaneNoCell>
__device__ __forceinline__ int wfa_scores_dynamic(const uint32_t (&dk)[KW][NP], int plen, int tlen, int ms_run, bool reduce, bool active,
                                                  int16_t *hist = nullptr, CellF on_cell = CellF{})
{
    constexpr WfShape<X, O, E, MAXS> SH{};
    constexpr WfHist<X, O, E, MAXS> HX{};
    bool hasi[MAXS + 1], hasd[MAXS + 1];
    static_assert(KW == SH.kmax - SH.kmin + 1, "diagonal window");
    static_assert(SH.kmax < 16 && SH.kmin > -16, "diagonal shifts are single-word funnel shifts");
    const int ak = tlen - plen;
    int Mv[MAXS + 1][KW], Iv[MAXS + 1][KW], Dv[MAXS + 1][KW];
    int klo[MAXS + 1], khi[MAXS + 1];
    bool pres[MAXS + 1], mnul[MAXS + 1], inul[MAXS + 1], dnul[MAXS + 1];
    int score = MAXS + 1;
    bool done = false;
#pragma unroll
    for (int s = 0; s <= MAXS; ++s) {
        if (!SH.present[s]) {
            pres[s] = false; mnul[s] = inul[s] = dnul[s] = true; klo[s] = 0; khi[s] = -1; hasi[s] = hasd[s] = false;
            if (HIST) { hist[(HX.meta + 3 * s) * kWave] = 0; hist[(HX.meta + 3 * s + 1) * kWave] = -1; hist[(HX.meta + 3 * s + 2) * kWave] = 0; }
            continue;
        }
        if (s == 0) {   // wavefronts[0] = allocate_new_score(0, 0, 0, 0); M[0] = 0 (wfa.c:347-348)
            pres[0] = true; mnul[0] = false; inul[0] = dnul[0] = true; klo[0] = khi[0] = 0; hasi[0] = hasd[0] = false;
            Mv[0][-SH.kmin] = 0;
        } else {        // affine_wfa_compute_next, wfa.c:268-340
            const int ss = s - X, so = s - O - E, se = s - E;
            const bool m_sub_null = ss < 0 || !SH.present[ss] || !pres[ss < 0 ? 0 : ss] || mnul[ss < 0 ? 0 : ss];
            const bool m_o_null = so < 0 || !SH.present[so] || !pres[so < 0 ? 0 : so] || mnul[so < 0 ? 0 : so];
            const bool i_e_null = se < 0 || !SH.present[se] || !pres[se < 0 ? 0 : se] || inul[se < 0 ? 0 : se];
            const bool d_e_null = se < 0 || !SH.present[se] || !pres[se < 0 ? 0 : se] || dnul[se < 0 ? 0 : se];
            const bool i_out_null = m_o_null && i_e_null, d_out_null = m_o_null && d_e_null;
            pres[s] = !(m_sub_null && i_out_null && d_out_null);
            const int sub_lo = m_sub_null ? 1 : klo[ss < 0 ? 0 : ss], sub_hi = m_sub_null ? -1 : khi[ss < 0 ? 0 : ss];
            const int o_lo = m_o_null ? 1 : klo[so < 0 ? 0 : so], o_hi = m_o_null ? -1 : khi[so < 0 ? 0 : so];
            const bool e_none = i_e_null && d_e_null;
            const int e_lo = e_none ? 1 : klo[se < 0 ? 0 : se], e_hi = e_none ? -1 : khi[se < 0 ? 0 : se];
            klo[s] = min(min(sub_lo, o_lo), e_lo) - 1;
            khi[s] = max(max(sub_hi, o_hi), e_hi) + 1;
            mnul[s] = false; inul[s] = i_out_null; dnul[s] = d_out_null;
            hasi[s] = !i_out_null; hasd[s] = !d_out_null;
#pragma unroll
            for (int k = SH.lo[s]; k <= SH.hi[s]; ++k) {   // affine_wfa_compute_offsets, wfa.c:231-266
                const int kk = k - SH.kmin;
                const int km1 = kk > 0 ? kk - 1 : 0, kp1 = kk + 1 < KW ? kk + 1 : KW - 1;   // clamped: only read when in range
                const int sso = so < 0 ? 0 : so, sse = se < 0 ? 0 : se, sss = ss < 0 ? 0 : ss;
                int ins = -10;
                {
                    const int ins_g = (!m_o_null && o_lo <= k - 1 && k - 1 <= o_hi) ? Mv[sso][km1] : kLaneNull;
                    const int ins_i = (!i_e_null && e_lo <= k - 1 && k - 1 <= e_hi) ? Iv[sse][km1] : kLaneNull;
                    const int v = (ins_g == kLaneNull && ins_i == kLaneNull) ? kLaneNull : max(ins_g, ins_i) + 1;
                    ins = i_out_null ? -10 : v;
                    Iv[s][kk] = v;
                    if (HIST && SH.hasI[s]) hist[(HX.i[s] + k - SH.lo[s]) * kWave] = (int16_t)v;
                }
                int del = -10;
                {
                    const int del_g = (!m_o_null && o_lo <= k + 1 && k + 1 <= o_hi) ? Mv[sso][kp1] : kLaneNull;
                    const int del_d = (!d_e_null && e_lo <= k + 1 && k + 1 <= e_hi) ? Dv[sse][kp1] : kLaneNull;
                    const int v = max(del_g, del_d);
                    del = d_out_null ? -10 : v;
                    Dv[s][kk] = v;
                    if (HIST && SH.hasD[s]) hist[(HX.d[s] + k - SH.lo[s]) * kWave] = (int16_t)v;
                }
                int sub = -10;
                if (!m_sub_null) sub = (sub_lo <= k && k <= sub_hi) ? Mv[sss][kk] + 1 : kLaneNull;
                Mv[s][kk] = max(del, max(sub, ins));
            }
        }
        // affine_wfa_extend (wfa.c:186-208), bit-parallel
#pragma unroll
        for (int k = SH.lo[s]; k <= SH.hi[s]; ++k) {
            const int kk = k - SH.kmin;
            int off = Mv[s][kk];
            const int v = off - k;
            const int limit = min(plen, tlen - k);
            if (off >= 0 && v >= 0 && v < limit) {
                const int stop = min(first_stop<NP>(dk[kk], v), limit);
                off += stop - v;
            }
            Mv[s][kk] = off;
            if (HIST) hist[(HX.m[s] + k - SH.lo[s]) * kWave] = (int16_t)off;
            on_cell();
        }
        // affine_wfa_reduce_wvs (WFA-adaptive, wfa.c:69-140): only shapes that can hold >= 10 diagonals get this code
        if (SH.hi[s] - SH.lo[s] + 1 >= 10) {
            const bool apply = reduce && pres[s] && !mnul[s] && (khi[s] - klo[s] + 1) >= 10;
            int dist[KW];
            int min_distance = max(plen, tlen);
#pragma unroll
            for (int k = SH.lo[s]; k <= SH.hi[s]; ++k) {
                const int kk = k - SH.kmin;
                const int off = Mv[s][kk];
                dist[kk] = max(plen - (off - k), tlen - off);
                if (klo[s] <= k && k <= khi[s]) min_distance = min(min_distance, dist[kk]);
            }
            // first / last diagonal of [klo, khi] within 50 of the best (the reference's two scans stop there)
            int kfirst = 0x7fffffff, klast = -0x7fffffff;
#pragma unroll
            for (int k = SH.lo[s]; k <= SH.hi[s]; ++k) {
                const int kk = k - SH.kmin;
                const bool ok = klo[s] <= k && k <= khi[s] && (dist[kk] - min_distance) <= 50;
                kfirst = ok ? min(kfirst, k) : kfirst;
                klast = ok ? max(klast, k) : klast;
            }
            int nklo = klo[s], nkhi = khi[s];
            const int top_limit = min(ak - 1, khi[s]);
            if (klo[s] < top_limit) nklo = min(top_limit, kfirst);
            const int bottom_limit = max(ak + 1, nklo);
            if (khi[s] > bottom_limit) nkhi = max(bottom_limit, klast);
            const bool kill = nklo > nkhi;
            if (apply) {
                mnul[s] = kill; inul[s] = inul[s] || kill; dnul[s] = dnul[s] || kill;
                klo[s] = kill ? klo[s] : nklo;
                khi[s] = kill ? khi[s] : nkhi;
            }
        }
        if (HIST) {   // final descriptor of this score (after the reduction)
            hist[(HX.meta + 3 * s) * kWave] = (int16_t)klo[s];
            hist[(HX.meta + 3 * s + 1) * kWave] = (int16_t)khi[s];
            hist[(HX.meta + 3 * s + 2) * kWave] = (int16_t)((pres[s] ? LF_PRESENT : 0) | (mnul[s] ? LF_MNULL : 0) | (inul[s] ? LF_INULL : 0) | (dnul[s] ? LF_DNULL : 0) |
                                                            (hasi[s] ? LF_HASI : 0) | (hasd[s] ? LF_HASD : 0));
        }
        // affine_wfa_end_reached (wfa.c:210-230); the run-time MAX_SCORE cap is a term of the test (wfa.c:368-376)
        {
            int m_end = kLaneNull;
#pragma unroll
            for (int k = SH.lo[s]; k <= SH.hi[s]; ++k) m_end = (k == ak) ? Mv[s][k - SH.kmin] : m_end;
            if (!done && pres[s] && !mnul[s] && klo[s] <= ak && ak <= khi[s] && m_end >= tlen && s <= ms_run) { done = true; score = s; }
        }
        if (__ballot(!done && active) == 0ull) break;   // every pair of this wave has finished
    }
    if (!done) score = ms_run + 1;                      // wfa.c:368-376
    return score;
}

template <int X, int O, int E, int MAXS, int RS, bool BT, bool DYN = false>
__global__ __launch_bounds__(64, DYN ? 2 : AIM_LANE_MIN_WAVES) void wfa_lane_kernel(KArgs a)   // DYN: 2 waves per SIMD (<= 256 VGPRs), else the grid runs in two rounds
{
    constexpr WfShape<X, O, E, MAXS> SH{};
    static_assert(DYN || SH.maxw < 10, "WFA-adaptive reduction could fire: shape needs the dynamic-bounds score loop (DYN)");
    static_assert(!(DYN && BT), "the dynamic-bounds score loop is score-only");
    static_assert(RS % 16 == 0 && (RS / 16) % 2 == 1, "row stride must be an odd number of 16-B slots");
    constexpr int NCH = RS / 16;                // 1-KiB DMA pieces per array per group (64 rows * RS / 1024)
    constexpr int NP = RS / 16;                 // packed dwords per sequence
    constexpr int KW = SH.kmax - SH.kmin + 1;
    // schedule 2: T's pieces and the request piece reach into the score loop. Not with CIGAR: that instantiation drains the whole
    // VM queue at the loop top and has the backtrace behind the score loop; later pieces cost it 8-10 % (profiles/lane_issue).
    constexpr bool SPREAD_T = AIM_LANE_INTERLEAVE == 2 && !BT;
    constexpr int NTP = NP + 1;                           // pieces of the T side: NP of rows, then the request piece
    // (the dynamic-bounds shape was measured with the hand-out over its whole, much longer score loop only: equal to schedule 1)
    constexpr LaneSpread<X, O, E, MAXS, NP, DYN ? 100 : AIM_LANE_SPREAD_PCT> SP{};
    extern __shared__ __attribute__((aligned(16))) char smem[];
    debug_poison_lds(a, smem);
    // [64 P rows][64 T rows][64 request descriptors (<= 16 B each)][result staging (CIGAR) | result ring (score-only {idx, score})]
    uint32_t *resL = reinterpret_cast<uint32_t *>(smem) + 2 * kWave * (RS / 4) + kWave * 4;                  // 64 x aim_result_t (24 B) staged for a coalesced store (CIGAR only)
    const uint32_t lds0 = (uint32_t)(uintptr_t)(lds_ptr_t)smem;   // LDS byte offset of the dynamic segment
    const uint32_t offP = lds0, offT = lds0 + kWave * RS, offQ = lds0 + 2 * kWave * RS;
    const int lane = threadIdx.x;
    const uint32_t n_groups = (a.n_pairs + kWave - 1) / kWave;
    const int ms_run = a.p.max_score;           // runtime MAX_SCORE <= MAXS

    // static XCD slices (an atomic work ticket was measured 3.5x slower: one word serves ~88 tickets/us)
    auto next_group = [&](uint32_t it_, uint32_t *g_) -> bool { return xcd_unit(n_groups, it_, g_); };
    uint32_t grp;
    bool have = next_group(0, &grp);
    const bool res8 = a.p.flags & AIM_FLAG_RES8;       // wave-uniform
    const LaneReqAddr req_addr = staged_request_addr(offQ, a, lane);
    const uint32_t row_addr = offP + (uint32_t)lane * RS;   // this lane's P row; its T row lies kWave * RS further
    if (have) {
        dma_rows<RS, NCH>(offP, a.patterns, grp * kWave, a.n_pairs, lane);
        dma_rows<RS, NCH>(offT, a.texts, grp * kWave, a.n_pairs, lane);
        stage_requests(offQ, a, grp * kWave, lane);
    }
    uint32_t stores_in_flight = 0;                     // result-store instructions the previous iteration issued after its DMA
    // Result ring (score-only, {idx, score} layout): slot s holds the results of the full group ring_grp0 + s * bpx -- a wave's
    // groups are affine in its iteration number (xcd_unit) -- and ring_fill slots are filled. A full ring is drained at the top
    // of the next iteration, what is left behind the loop. The batch's partial last group (the last iteration of the one wave
    // that has it) never enters the ring. All of it is wave-uniform.
    constexpr int RING = BT ? 0 : AIM_LANE_RING_SLOTS;
    const uint32_t offR = offQ + kWave * 16;
    const uint32_t bpx = gridDim.x >> 3;
    uint32_t ring_fill = 0, ring_grp0 = 0;
    auto ring_drain = [&](auto FULL, uint32_t count) __attribute__((always_inline)) {
        if constexpr (RING > 0) {
            char *dst = reinterpret_cast<char *>(a.res) + ((uint64_t)ring_grp0 + ((uint32_t)lane >> 5) * bpx) * (kWave * 8u) + ((uint32_t)lane & 31u) * 16u;
            ring_flush<RING, decltype(FULL)::value>(offR + (uint32_t)lane * 16u, dst, (uint64_t)bpx * (2u * kWave * 8u), count, lane);
        }
    };
#if AIM_LANE_STAMPS
    unsigned long long stamp_sum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, stamp_last;
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(stamp_last) :: "memory");
#endif
    for (uint32_t it = 0; have; ++it) {
        const uint32_t pair = grp * kWave + lane;
        const bool active = pair < a.n_pairs;
        // Result staging (below) is used with CIGAR only. Same-box A/B, 3 interleaved pairs each: with CIGAR -2.0 % time;
        // score-only +2.6 % (slower) -- there the ~30 us the 24-B result store costs (removal decomposition)
        // is the price of a write stream inside a read stream at the HBM ceiling, not of its access pattern.
        const bool full_group = BT && AIM_LANE_RES_STAGE && (grp + 1u) * kWave <= a.n_pairs;   // wave-uniform
        AIM_STAMP(0);                           // loop overhead / previous store
        // This group's DMA (rows + requests) has landed. VM operations complete in issue order (loads, stores and LDS-DMA
        // share vmcnt on gfx9), and the only operations younger than that DMA are the previous group's result stores, so a
        // COUNTED wait leaves exactly those in flight instead of paying their acknowledgement latency once per group.
        // One wavefront per workgroup: no barrier is needed, only the wait and a scheduling fence.
        if (BT || AIM_LANE_FULLWAIT || stores_in_flight == 0) asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
        else if (stores_in_flight == 1) asm volatile("s_waitcnt vmcnt(1) lgkmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(2) lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        AIM_STAMP(1);                           // wait for DMA
        // This lane's request and both its rows into registers; once they are back, every buffer of the group is free and the
        // next group's DMA may go into it: its HBM latency flies under the pack + compute below.
        // (Waiting for the P rows only and letting the T reads fly under the P pack was measured worth nothing, NOTES A.1
        // item 6, and would leave registers in flight across compiler-scheduled code.)
        lane_u32x4 rawP[NP], rawT[NP];
        lane_u32x2 rq_lo;
        uint32_t rq_hi;
        __builtin_amdgcn_sched_barrier(0);
        read_group<RS, NP>(req_addr, row_addr, rq_lo, rq_hi, rawP, rawT);
        __builtin_amdgcn_sched_barrier(0);
        if constexpr (RING > 0) {
            // A full ring leaves here: the VM queue is empty (the wait above was vmcnt(0) on this path), so these stores are its
            // oldest entries, in front of this iteration's DMA, and have the whole iteration to be acknowledged.
            if (ring_fill == RING) {
                ring_drain(std::true_type{}, RING);
                ring_fill = 0;
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        // This group's {idx, score} results (score-only, AIM_FLAG_RES8), called with every lane on; `on` = this lane has one.
        auto store_res8 = [&](uint32_t idx, uint32_t sc, bool on) __attribute__((always_inline)) {
            if (RING > 0 && (grp + 1u) * kWave <= a.n_pairs) {   // wave-uniform: a full group goes into the ring, no global store
                if (ring_fill == 0) ring_grp0 = grp;
                ring_put(offR + ring_fill * (kWave * 8u) + (uint32_t)lane * 8u, idx, sc);
                ++ring_fill;
                stores_in_flight = 0;
                return;
            }
            aim_result8_t *dst = reinterpret_cast<aim_result8_t *>(a.res) + pair;
            lane_u32x2 v2; v2.x = idx; v2.y = sc;
#if AIM_LANE_STORE_X4
            // the odd neighbour's result into the even lane (quad_perm [1,1,3,3]); an even lane whose neighbour has none stores 8 B
            const uint32_t nidx = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)idx, 0xF5, 0xf, 0xf, false);
            const uint32_t nsc = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)sc, 0xF5, 0xf, 0xf, false);
            if (!(lane & 1)) {
                if (on && pair + 1u < a.n_pairs) {
                    lane_u32x4 v4; v4.x = idx; v4.y = sc; v4.z = nidx; v4.w = nsc;
                    lane_store16(dst, v4);
                } else if (on) {
                    lane_store8(dst, v2);
                }
            }
#else
            if (on) lane_store8(dst, v2);   // ONE global_store_dwordx2 per lane (512 contiguous bytes per wavefront)
#endif
            stores_in_flight = 1;
        };
        const aim_request_t rq = decode_staged_request(rq_lo, rq_hi, a);
        const int plen = active ? rq.pattern_len : 0, tlen = active ? rq.text_len : 0;   // lanes past the batch tail read stale LDS
        uint32_t ngrp = 0;
        const bool nhave = next_group(it + 1, &ngrp);
        const bool inter = AIM_LANE_INTERLEAVE && !AIM_LANE_DIAG && nhave && (ngrp + 1u) * kWave <= a.n_pairs;   // wave-uniform
        AIM_STAMP(2);                           // LDS row reads
        // The next group's DMA. Issued as ONE burst, 15 KiB from each of the CU's 8 wavefronts back-pressure the vector-memory
        // queue and the wave sits in the issue of its own glds instructions (stamped: 3 350 of 13 400 ticks per group, 220 per
        // instruction, at 67 % of the streaming ceiling). Full groups therefore hand their pieces out one by one between the
        // pack steps below; only the batch's last (partial) group is issued here in one go.
        if (nhave && !inter) {
            dma_rows<RS, NCH>(offP, a.patterns, ngrp * kWave, a.n_pairs, lane);
            dma_rows<RS, NCH>(offT, a.texts, ngrp * kWave, a.n_pairs, lane);
            stage_requests(offQ, a, ngrp * kWave, lane);
        }
        const char *gP_next = a.patterns + (uint64_t)ngrp * (kWave * RS) + (uint32_t)lane * 16u;
        const char *gT_next = a.texts + (uint64_t)ngrp * (kWave * RS) + (uint32_t)lane * 16u;
        __builtin_amdgcn_sched_barrier(0);      // keep the DMA issue ahead of the ALU work
        AIM_STAMP(3);                           // DMA issue (burst mode only)
#if AIM_LANE_DIAG == 1 || AIM_LANE_DIAG == 4
        {   // removal decomposition: the streaming floor of this structure (DMA + LDS reads [+ result store])
            uint32_t x = 0;
#pragma unroll
            for (int j = 0; j < NP; ++j) x ^= rawP[j].x ^ rawP[j].y ^ rawP[j].z ^ rawP[j].w ^ rawT[j].x ^ rawT[j].y ^ rawT[j].z ^ rawT[j].w;
            // as production: the stores stay in flight over the loop top (without this the counted wait was vmcnt(0) and every
            // group paid the store's acknowledgement, which overstated the store's share in the removal decomposition), and
            // {idx, score} results take production's way out (store_res8: the ring, or the direct store and its variants)
            if (AIM_LANE_DIAG == 1 && res8) {
                store_res8(rq.idx, x, active);
            } else {
                if (active && (AIM_LANE_DIAG == 1 || x == 0x12345678u)) {
                    aim_result_t r;
                    r.max_operations = plen + tlen; r.begin_offset = 0; r.end_offset = 0; r.score = (int)x; r.status = 0; r.idx = rq.idx;
                    store_result(a, pair, r);
                }
                stores_in_flight = AIM_LANE_DIAG == 1 ? 2u : 0u;
            }
            have = nhave; grp = ngrp;
            continue;
        }
#endif
        const int minlen = active ? min(plen, tlen) : 0x7fffffff;
        const int min_len_wave = __builtin_amdgcn_readfirstlane(wave_min_i32(minlen));
        uint32_t P[NP], T[NP];
        // four instantiations of the pack phase, selected by two wave-uniform tests made ONCE per group
        uint32_t bad;
        // piece I of the next group's T side
        auto t_piece = [&](auto I) __attribute__((always_inline)) {
            constexpr int i = decltype(I)::value;
            if constexpr (i < NP) dma_piece<i>(offT, gT_next);
            else { stage_requests(offQ, a, ngrp * kWave, lane); __builtin_amdgcn_sched_barrier(0); }
        };
        auto pack_both = [&](auto FAST, auto INTER) __attribute__((always_inline)) {
            constexpr bool fast = decltype(FAST)::value, with_dma = decltype(INTER)::value;
            bad = pack_row<fast, NP>(rawP, plen, P, [&](auto J) { if (with_dma) dma_piece<decltype(J)::value>(offP, gP_next); });
            bad |= pack_row<fast, NP>(rawT, tlen, T, [&](auto J) {
                constexpr int j = decltype(J)::value;
                if (with_dma && SPREAD_T) lane_pieces(SP.due(j), SP.due(j + 1), t_piece, std::make_integer_sequence<int, NTP>{});
                else if (with_dma) dma_piece<j>(offT, gT_next);
            });
            if (with_dma && !SPREAD_T) stage_requests(offQ, a, ngrp * kWave, lane);
        };
        const bool fast = min_len_wave >= 16 * (NP - 1);
        if (fast && inter) pack_both(std::true_type{}, std::true_type{});
        else if (fast) pack_both(std::true_type{}, std::false_type{});
        else if (inter) pack_both(std::false_type{}, std::true_type{});
        else pack_both(std::false_type{}, std::false_type{});

        AIM_STAMP(4);                           // pack + validate
#if AIM_LANE_DIAG == 2
        {
            uint32_t x = bad;
#pragma unroll
            for (int j = 0; j < NP; ++j) x ^= P[j] ^ T[j];
            if (active) {
                aim_result_t r;
                r.max_operations = plen + tlen; r.begin_offset = 0; r.end_offset = 0; r.score = (int)x; r.status = 0; r.idx = rq.idx;
                store_result(a, pair, r);
            }
            stores_in_flight = res8 ? 1u : 2u;
            have = nhave; grp = ngrp;
            continue;
        }
#endif
        const int ak = tlen - plen;   // alignment_k
        int Mv[MAXS + 1][KW], Iv[MAXS + 1][KW], Dv[MAXS + 1][KW];
        int score = MAXS + 1;
        bool done = false;
        // Diagonals and score loop, instantiated twice: with the hand-out of the T side's remaining pieces (schedule 2, the steady
        // state) and without (burst iterations: the batch's partial last group and each wave's last one). The choice is made once
        // per group; a run-time test at every slot would be a scalar branch per cell.
        auto score_phase = [&](auto SPREAD) __attribute__((always_inline)) {
        constexpr bool spread = decltype(SPREAD)::value;
        int slot = NP, t_out = SP.due(NP);   // the T pack has passed slots 1 .. NP; both are constants at every use once the loops are unrolled
        auto at_slot = [&]() __attribute__((always_inline)) {
            if constexpr (spread) {
                ++slot;
                lane_pieces(t_out, SP.due(slot), t_piece, std::make_integer_sequence<int, NTP>{});
                t_out = SP.due(slot);
            }
        };
        // ---- mismatch bit-vectors per diagonal: bit pair v of dk[k] != 0  <=>  P[v] != T[v + k] ----
        uint32_t dk[KW][NP];
        if (__ballot(active && bad != 0u) != 0ull) {
            // some pair of this wavefront has a byte outside A/C/G/T ('N' in real reads): compare raw bytes (cold path)
#pragma unroll
            for (int kk = 0; kk < KW; ++kk) raw_diag<NP>(rawP, rawT, SH.kmin + kk, dk[kk]);
        } else {
#pragma unroll
            for (int kk = 0; kk < KW; ++kk) {
                const int k = SH.kmin + kk;
#pragma unroll
                for (int j = 0; j < NP; ++j) {
                    uint32_t ts;
                    if (k == 0) ts = T[j];
                    else if (k > 0) ts = __builtin_amdgcn_alignbit(j + 1 < NP ? T[j + 1] : 0u, T[j], 2 * k);
                    else ts = __builtin_amdgcn_alignbit(T[j], j > 0 ? T[j - 1] : 0u, 32 + 2 * k);
                    dk[kk][j] = P[j] ^ ts;
                }
            }
        }
        at_slot();                    // (the cold raw-byte construction above issues nothing: its pieces go out here)

        // ---- affine_wfa_compute, statically unrolled over scores and diagonals -----------------
        if constexpr (DYN) {
            score = wfa_scores_dynamic<X, O, E, MAXS, NP, KW, false, decltype(at_slot)>(dk, plen, tlen, ms_run, (a.p.flags & AIM_FLAG_REDUCE) != 0, active,
                                                                                        nullptr, at_slot);
            done = score <= ms_run;
        } else {
#pragma unroll
        for (int s = 0; s <= MAXS; ++s) {
            // runtime MAX_SCORE below the template cap: the reference leaves its loop as "exceeded" when the score passes
            // MAX_SCORE and never tests the end condition there (wfa.c:368-376). The test must precede the skip of absent
            // scores: placed only at the end of the body it was never reached when MAX_SCORE itself has no wavefront, and a
            // pair whose score is exactly MAX_SCORE+1 was then aligned and backtraced instead of reported as exceeded
            // (same score either way, so only CIGAR output showed it; found by tools/fuzz_parity.py).
            // (round 2: the cap is a term of the end test below instead of two scalar branches per score: wavefronts past the
            // run-time cap are computed and ignored, which is the same answer)
            if (!SH.present[s]) continue;
            if (s > 0) {
                const int ss = s - X, so = s - O - E, se = s - E;
                const bool sub_ok = ss >= 0 && SH.present[ss];
                const bool o_ok = so >= 0 && SH.present[so];
                const bool ie_ok = se >= 0 && SH.present[se] && SH.hasI[se];
                const bool de_ok = se >= 0 && SH.present[se] && SH.hasD[se];
#pragma unroll
                for (int k = SH.lo[s]; k <= SH.hi[s]; ++k) {   // affine_wfa_compute_offsets, wfa.c:231-266
                    const int kk = k - SH.kmin;
                    const int km1 = kk > 0 ? kk - 1 : 0, kp1 = kk + 1 < KW ? kk + 1 : KW - 1;   // clamped: only read when in range
                    int ins = -10;
                    if (SH.hasI[s]) {
                        const int ins_g = (o_ok && SH.lo[so] <= k - 1 && k - 1 <= SH.hi[so]) ? Mv[so][km1] : kLaneNull;
                        const int ins_i = (ie_ok && SH.lo[se] <= k - 1 && k - 1 <= SH.hi[se]) ? Iv[se][km1] : kLaneNull;
                        ins = (ins_g == kLaneNull && ins_i == kLaneNull) ? kLaneNull : max(ins_g, ins_i) + 1;
                        Iv[s][kk] = ins;
                    }
                    int del = -10;
                    if (SH.hasD[s]) {
                        const int del_g = (o_ok && SH.lo[so] <= k + 1 && k + 1 <= SH.hi[so]) ? Mv[so][kp1] : kLaneNull;
                        const int del_d = (de_ok && SH.lo[se] <= k + 1 && k + 1 <= SH.hi[se]) ? Dv[se][kp1] : kLaneNull;
                        del = max(del_g, del_d);
                        Dv[s][kk] = del;
                    }
                    int sub = -10;
                    if (sub_ok) sub = (SH.lo[ss] <= k && k <= SH.hi[ss]) ? Mv[ss][kk] + 1 : kLaneNull;
                    Mv[s][kk] = max(del, max(sub, ins));
                }
            } else {
                Mv[0][-SH.kmin] = 0;
            }
            // affine_wfa_extend (wfa.c:186-208), bit-parallel; then affine_wfa_end_reached (wfa.c:210-230)
            int m_end = kLaneNull;
            bool end_in_range = false;
#pragma unroll
            for (int k = SH.lo[s]; k <= SH.hi[s]; ++k) {
                const int kk = k - SH.kmin;
                int off = Mv[s][kk];
                const int v = off - k;
                const int limit = min(plen, tlen - k);
                if (off >= 0 && v >= 0 && v < limit) {
                    const int stop = min(first_stop<NP>(dk[kk], v), limit);
                    off += stop - v;
                }
                Mv[s][kk] = off;
                if (k == ak) { m_end = off; end_in_range = true; }
                at_slot();
            }
            if (!done && end_in_range && m_end >= tlen && s <= ms_run) { done = true; score = s; }
            if (__ballot(!done && active) == 0ull) break;   // every pair of this wave has finished
        }
        if (!done) score = ms_run + 1;                              // wfa.c:368-376
        }
        // The score loop ends early when every pair of the wave has finished: what it had not issued goes out now, so that every
        // piece is older than the result store and the loop top's counted wait stays what it is.
        if constexpr (spread) lane_pieces_from<NTP>(t_out, t_piece);
        };
        if (SPREAD_T && inter) score_phase(std::true_type{});
        else score_phase(std::false_type{});
        AIM_STAMP(5);                           // diagonals + WFA (schedule 2: and the issue of the T side's pieces)

        int begin_offset = plen + tlen - 1;     // edit_cigar_allocate, wfa.c:57-67
        int status = AIM_PAIR_OK;
        // (the 'M' prefill's wave-uniform bounds, see below: taken where every lane is on)
        // (gaps of total length L cost at least o + L e: with the pair's own score, L <= (score - o) / e; a pair beyond MAX_SCORE prints its last byte only)
        const int gap_len = done ? max(0, score - O) / E : 0;
        const int w_lo = BT ? wave_min_i32(active ? max(0, (done ? min(plen, tlen) - gap_len : plen + tlen - 1)) >> 4 : (1 << 20)) : 0;
        const int w_hi = BT ? -wave_min_i32(active ? -((plen + tlen + 15) >> 4) : 0) : 0;
        if (BT && active) {
            // memset(cigar->operations, 'M', 2*READ_SIZE) (wfa.c:465): constant data, no VGPR image. Match runs of the backtrace then only move
            // begin_offset; edit ops are patched in as bytes. Only ops[begin_offset, end_offset) is ever looked at (host.c:347-349, edit_cigar_print), and
            // a CIGAR with gaps of total length L has plen + (insertions) = tlen + (deletions) <= max(plen, tlen) + L operations, so begin_offset >=
            // min(plen, tlen) - L, L <= (score - o) / e: the 16-byte pieces in front of that (and behind plen + tlen) are not written -- 7 of a row's 14
            // are at l = 100 (round 5).
            char *ops = a.ops + (uint64_t)pair * (2 * RS);
            uint4 *orow = reinterpret_cast<uint4 *>(ops);
            const uint4 mm = make_uint4(0x4D4D4D4Du, 0x4D4D4D4Du, 0x4D4D4D4Du, 0x4D4D4D4Du);
#pragma unroll
            for (int j = 0; j < (2 * RS) / 16; ++j)
                if (j >= w_lo && j < w_hi) orow[j] = mm;
            if (done) {
                // affine_wavefronts_backtrace (wfa_backtracing.c:210-351) over the register-resident history.
                // The fetchers (wfa_backtracing.c:73-172) become static select chains; kNone marks "no such cell"
                // (score < 0, wavefronts[s] == NULL, d_null / iwavefront == NULL, k outside [klo, khi]).
                constexpr int kNone = (int)0x80000000;
                auto getM = [&](int s_, int k_) {
                    int r = kNone;
#pragma unroll
                    for (int s2 = 0; s2 <= MAXS; ++s2)
                        if (SH.present[s2])
#pragma unroll
                            for (int k2 = SH.lo[s2]; k2 <= SH.hi[s2]; ++k2) r = (s_ == s2 && k_ == k2) ? Mv[s2][k2 - SH.kmin] : r;
                    return r;
                };
                auto getI = [&](int s_, int k_) {
                    int r = kNone;
#pragma unroll
                    for (int s2 = 0; s2 <= MAXS; ++s2)
                        if (SH.present[s2] && SH.hasI[s2])
#pragma unroll
                            for (int k2 = SH.lo[s2]; k2 <= SH.hi[s2]; ++k2) r = (s_ == s2 && k_ == k2) ? Iv[s2][k2 - SH.kmin] : r;
                    return r;
                };
                auto getD = [&](int s_, int k_) {
                    int r = kNone;
#pragma unroll
                    for (int s2 = 0; s2 <= MAXS; ++s2)
                        if (SH.present[s2] && SH.hasD[s2])
#pragma unroll
                            for (int k2 = SH.lo[s2]; k2 <= SH.hi[s2]; ++k2) r = (s_ == s2 && k_ == k2) ? Dv[s2][k2 - SH.kmin] : r;
                    return r;
                };
                auto valid_loc = [&](int kk_, int off_) {
                    const int v_ = off_ - kk_, h_ = off_;
                    return v_ > 0 && v_ <= plen && h_ > 0 && h_ <= tlen;
                };
                auto put = [&](char ch) {
                    if (begin_offset >= 0 && begin_offset < 2 * RS) ops[begin_offset] = ch;
                    --begin_offset;
                };
                enum { BT_M = 0, BT_I = 1, BT_D = 2 };
                int sc = score, k = ak;
                int offset = getM(sc, k);
                bool valid = valid_loc(k, offset);
                int bt = BT_M;
                int v = offset - k, h = offset;
                while (v > 0 && h > 0 && sc > 0) {
                    if (!valid) {
                        valid = valid_loc(k, offset);
                        if (valid) {   // add_trailing_gap, wfa_backtracing.c:48-69
                            if (k < ak) for (int i = k; i < ak; ++i) put('I');
                            else if (k > ak) for (int i = ak; i < k; ++i) put('D');
                        }
                    }
                    const int s_o = sc - (O + E), s_e = sc - E, s_x = sc - X;
                    int del_ext = kLaneNull, del_open = kLaneNull, ins_ext = kLaneNull, ins_open = kLaneNull, misms = kLaneNull;
                    if (bt != BT_I) {
                        const int a1 = getD(s_e, k + 1), a2 = getM(s_o, k + 1);
                        if (a1 != kNone) del_ext = a1;
                        if (a2 != kNone) del_open = a2;
                    }
                    if (bt != BT_D) {
                        const int a1 = getI(s_e, k - 1), a2 = getM(s_o, k - 1);
                        if (a1 != kNone) ins_ext = a1 + 1;
                        if (a2 != kNone) ins_open = a2 + 1;
                    }
                    if (bt == BT_M) {
                        const int a1 = getM(s_x, k);
                        if (a1 != kNone) misms = a1 + 1;
                    }
                    const int max_all = max(misms, max(max(ins_ext, ins_open), max(del_ext, del_open)));
                    if (bt == BT_M) {
                        const int num_matches = offset - max_all;
                        if (num_matches > 0) begin_offset -= num_matches;   // 'M' already in place
                        offset = max_all;
                        v = offset - k;
                        h = offset;
                        if (v <= 0 || h <= 0) break;
                    }
                    char op;
                    if (max_all == del_ext) { op = 'D'; sc = s_e; ++k; bt = BT_D; }
                    else if (max_all == del_open) { op = 'D'; sc = s_o; ++k; bt = BT_M; }
                    else if (max_all == ins_ext) { op = 'I'; sc = s_e; --k; --offset; bt = BT_I; }
                    else if (max_all == ins_open) { op = 'I'; sc = s_o; --k; --offset; bt = BT_M; }
                    else if (max_all == misms) { op = 'X'; sc = s_x; --offset; }
                    else { status = AIM_PAIR_WFA_NO_LINK; break; }
                    if (valid) put(op);
                    v = offset - k;
                    h = offset;
                }
                if (status == AIM_PAIR_OK) {
                    if (sc == 0) {
                        if (offset > 0) begin_offset -= offset;
                    } else {
                        for (; v > 0; --v) put('D');
                        for (; h > 0; --h) put('I');
                    }
                    ++begin_offset;
                }
            }
        }
        if (!BT && res8) {   // wave-uniform; score-only pairs have no status but AIM_PAIR_OK
            bool on = active;
#if AIM_LANE_DIAG == 3
            on = on && score == 0x12345678;
#endif
            store_res8(rq.idx, (uint32_t)score, on);
        } else if (active) {
            {
                aim_result_t r;
                r.max_operations = plen + tlen;
                r.begin_offset = begin_offset;
                r.end_offset = plen + tlen;
                r.score = score;
                r.status = status;
                r.idx = rq.idx;
#if AIM_LANE_DIAG == 3
                if (score == 0x12345678)
#endif
#if AIM_LANE_RES_STAGE
                if (full_group) {
                    // 24-B structs at a 24-B stride per lane touch every line piecemeal in two instructions; the removal
                    // decomposition priced this store at ~30 of 203 us. Staged in LDS, the 1 536 B of a group leave as 96
                    // contiguous 16-B pieces (full lines), nontemporal: nothing on the device reads them again.
                    uint32_t *rl = resL + lane * 6;
                    rl[0] = (uint32_t)r.max_operations; rl[1] = (uint32_t)r.begin_offset; rl[2] = (uint32_t)r.end_offset;
                    rl[3] = (uint32_t)r.score; rl[4] = (uint32_t)r.status; rl[5] = (uint32_t)r.idx;
                } else
#endif
                if (BT) {
                    store_result(a, pair, r);
                } else {               // TWO stores per lane: dwordx4 + dwordx2 (24-B struct, 8-B aligned)
                    uint32_t *dst = reinterpret_cast<uint32_t *>(a.res + pair);
#if AIM_LANE_STORE_SC1 >= 2
                    lane_u32x4 v4; v4.x = (uint32_t)r.max_operations; v4.y = (uint32_t)r.begin_offset; v4.z = (uint32_t)r.end_offset; v4.w = (uint32_t)r.score;
                    lane_u32x2 v2; v2.x = (uint32_t)r.status; v2.y = r.idx;
                    lane_store16(dst, v4);
                    lane_store8(dst + 4, v2);
#else
                    *reinterpret_cast<uint4 *>(dst) = make_uint4((uint32_t)r.max_operations, (uint32_t)r.begin_offset, (uint32_t)r.end_offset, (uint32_t)r.score);
                    *reinterpret_cast<uint2 *>(dst + 4) = make_uint2((uint32_t)r.status, r.idx);
#endif
                }
            }
        }
        if (BT || AIM_LANE_DIAG == 3) stores_in_flight = 0;
        else if (!res8) stores_in_flight = 2;   // every iteration has at least one active lane ({idx, score}: set by store_res8)
#if AIM_LANE_RES_STAGE
        if (full_group) {   // wave-uniform
            typedef uint32_t aim_u32x4 __attribute__((ext_vector_type(4)));
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const aim_u32x4 *src = reinterpret_cast<const aim_u32x4 *>(resL);
            aim_u32x4 *dst = reinterpret_cast<aim_u32x4 *>(a.res + (size_t)grp * kWave);
            const aim_u32x4 c0 = src[lane];
            __builtin_nontemporal_store(c0, dst + lane);
            if (lane < 32) { const aim_u32x4 c1 = src[64 + lane]; __builtin_nontemporal_store(c1, dst + 64 + lane); }
        }
#endif
        have = nhave;
        grp = ngrp;
        AIM_STAMP(6);                           // result store issue
    }
    if (ring_fill) ring_drain(std::false_type{}, ring_fill);       // the groups since the last full ring (a slot may lack its partner: lanes 32 .. 63 masked)
#if AIM_LANE_STAMPS
    if (lane == 0) {
        unsigned long long *dbg = reinterpret_cast<unsigned long long *>(a.scratch + a.scratch_per_wave) + (size_t)blockIdx.x * 8;
        for (int i = 0; i < 8; ++i) dbg[i] = stamp_sum[i];
    }
#endif
}

// ---------------------------------------------------------------------------------------------------
// host-side planning / dispatch
// ---------------------------------------------------------------------------------------------------
// persistent grid: AIM_LANE_WGS_PER_CU single-wave workgroups per CU, LDS 2 x 64 rows x 112 B = 14 KiB each

constexpr int kLaneDynMaxScore = 10;   // the dynamic-bounds instantiation: MAX_SCORE 6..10 (l = 100: e up to 2 %), score-only

// The penalty sets the one-pair-per-lane kernels are built for, each with the largest MAX_SCORE of its STATIC shape (no wavefront 10 diagonals wide: the
// reduction cannot fire, WfShape::maxw): the reference's default 3 / 4 / 1 and the sets its launcher is run with in the tests and judge digests
// (run-wfa-pim-wram.py:17-24 takes any -x -g -a) -- MAX_SCORE = ceil(l e) max(x, o + e) at l = 100, e = 1 % is 5 / 8 / 4 / 6. F(X, O, E, MAXS).
#define AIM_LANE_COST_SETS(F) F(3, 4, 1, 5) F(4, 6, 2, 8) F(2, 3, 1, 4) F(5, 4, 2, 6)

// MAX_SCORE of the static shape built for these penalties, or -1
inline int wfa_lane_static_max_score(const aim_params_t &p)
{
#define AIM_LANE_COST_TEST(X, O, E, MS) if (p.mismatch == X && p.gap_o == O && p.gap_e == E) return MS;
    AIM_LANE_COST_SETS(AIM_LANE_COST_TEST)
#undef AIM_LANE_COST_TEST
    return -1;
}

inline bool wfa_lane_supported(const aim_params_t &p, bool allow_dynamic = true)
{
    if (p.algo != AIM_ALGO_WFA) return false;
    const int ms = wfa_lane_static_max_score(p);
    if (ms < 0) return false;
    if (p.read_size != 80 && p.read_size != 112) return false;           // odd number of 16-B slots per row (conflict-free row reads)
    if (p.max_score <= ms) return true;
    if (p.mismatch != 3 || p.gap_o != 4 || p.gap_e != 1) return false;   // the dynamic-bounds shape: the reference's default penalties only
    return allow_dynamic && p.max_score <= kLaneDynMaxScore && !(p.flags & AIM_FLAG_BACKTRACE);
}

inline size_t wfa_lane_todo_bytes(uint32_t n_pairs) { return ((size_t)(LANE_TODO_LIST + n_pairs) * 4 + 255) & ~(size_t)255; }

inline void wfa_lane_plan(const aim_params_t &p, uint32_t n_pairs, const Knobs &kn, uint32_t *grid, uint32_t *block, size_t *lds)
{
    const uint32_t n_groups = (n_pairs + kWave - 1) / kWave;
    uint32_t g = resident_grid(kn, AIM_LANE_WGS_PER_CU);
    const uint32_t need = ((n_groups + 7u) / 8u) * 8u;
    if (g > need) g = need < 8u ? 8u : need;
    *grid = g;
    *block = kWave;
    *lds = (size_t)2 * kWave * p.read_size + kWave * 16 + ((p.flags & AIM_FLAG_BACKTRACE) ? kWave * sizeof(aim_result_t) : 0);
    // the result ring of the score-only {idx, score} layout: 512 B per slot behind the request slots. It must not cost a resident
    // workgroup (10 per CU in two rounds measured 50 % slower): 15 360 + 512 K at READ_SIZE 112 rounds to 16 granules up to K = 10
    static_assert(AIM_LANE_RING_SLOTS == 0 || AIM_LANE_RING_SLOTS == 4 || AIM_LANE_RING_SLOTS == 8, "AIM_LANE_RES_RING: 0, 4 or 8");
    if (!(p.flags & AIM_FLAG_BACKTRACE) && (p.flags & AIM_FLAG_RES8)) *lds += (size_t)AIM_LANE_RING_SLOTS * kWave * 8;
    assert(lds_workgroups_per_cu(*lds) >= AIM_LANE_WGS_PER_CU);
}

// Kernels are instantiated in ONE translation unit (tu_*.hip defines AIM_TU_WFA_LANE); every other includer sees the declaration only.
#ifdef AIM_TU_WFA_LANE
void wfa_lane_launch(const aim_params_t &p, uint32_t grid, uint32_t block, size_t lds, const KArgs &ka, hipStream_t s)
{
    (void)block;
    const bool bt = p.flags & AIM_FLAG_BACKTRACE;
    if (p.max_score > wfa_lane_static_max_score(p)) {   // dynamic-bounds shape (3 / 4 / 1, score-only)
        if (p.read_size == 80) hipLaunchKernelGGL((wfa_lane_kernel<3, 4, 1, kLaneDynMaxScore, 80, false, true>), dim3(grid), dim3(kWave), lds, s, ka);
        else hipLaunchKernelGGL((wfa_lane_kernel<3, 4, 1, kLaneDynMaxScore, 112, false, true>), dim3(grid), dim3(kWave), lds, s, ka);
        return;
    }
#define AIM_LANE_LAUNCH(X, O, E, MS)                                                                                             \
    if (p.mismatch == X && p.gap_o == O && p.gap_e == E) {                                                                       \
        if (p.read_size == 80) {                                                                                                 \
            if (bt) hipLaunchKernelGGL((wfa_lane_kernel<X, O, E, MS, 80, true>), dim3(grid), dim3(kWave), lds, s, ka);           \
            else hipLaunchKernelGGL((wfa_lane_kernel<X, O, E, MS, 80, false>), dim3(grid), dim3(kWave), lds, s, ka);             \
        } else if (p.read_size == 112) {                                                                                         \
            if (bt) hipLaunchKernelGGL((wfa_lane_kernel<X, O, E, MS, 112, true>), dim3(grid), dim3(kWave), lds, s, ka);          \
            else hipLaunchKernelGGL((wfa_lane_kernel<X, O, E, MS, 112, false>), dim3(grid), dim3(kWave), lds, s, ka);            \
        }                                                                                                                        \
        return;                                                                                                                  \
    }
    AIM_LANE_COST_SETS(AIM_LANE_LAUNCH)
#undef AIM_LANE_LAUNCH
}
#else
void wfa_lane_launch(const aim_params_t &p, uint32_t grid, uint32_t block, size_t lds, const KArgs &ka, hipStream_t s);
#endif

}  // namespace aim
