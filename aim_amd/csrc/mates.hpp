// mates.hpp -- the device side of AIM_FLAG_MATE_PAIRS (aim_hip.h): paired-end candidate selection over a READ_GROUPS batch.
//
//   * mate_select_kernel: reads 2m and 2m + 1 are mates. After group_select_kernel has picked every read's independent winner, this
//     kernel enumerates the K1 x K2 combinations of a read pair's candidates, keeps the proper ones (both OK, opposite strands, the
//     strand-0 window not right of the strand-1 window, window span inside [min_span, max_span]), reduces them to the one of lowest
//     cost (score_i + score_j; ties: lowest i, then lowest j) plus the tie count and the runner-up cost, and compares it with the
//     unpaired choice (the independent winners' scores + unpaired_penalty). It writes the read pair's aim_mate_t and, where the
//     proper combination wins, overwrites sel[2m] / sel[2m + 1]. Everything downstream of sel is READ_GROUPS' own.
//
// Brute force, O(K1 * K2) per read pair. No LDS, no scratch, no atomics, vector stores only.
#pragma once

#include <climits>

#include "aim_device.hpp"

namespace aim {

struct MateArgs {
    int64_t min_span, max_span;
    int32_t unpaired_penalty;
    uint32_t n_mates;       // read pairs: n_reads / 2
    uint32_t lanes;         // W: lanes per read pair, a power of two in 1 .. 64 (results do not depend on it)
};

// mate_select_kernel over the n_reads / 2 read pairs of a batch of ka.n_pairs candidates; n_mates and lanes of `ma` are filled in here
#pragma GCC visibility push(hidden)
void mate_select_launch(const KArgs &ka, MateArgs ma, uint32_t n_reads, const aim_result_t *res, const uint64_t *tpos, const uint32_t *roff,
                        const aim_best_t *best, uint32_t *sel, aim_mate_t *mates, hipStream_t s);
#pragma GCC visibility pop

#ifdef AIM_TU_GROUPS   // (groups.hpp: one unit for its kernels, hits.hpp's and these)
// What a set of combinations of one read pair contributes: the lowest proper cost, its combination (lowest i, then lowest j), how many
// proper combinations have that cost and the lowest cost among the others (INT_MAX when there is none). cnt == 0: no proper combination.
struct MateSel {
    int cost;
    uint32_t i, j;
    uint32_t cnt;
    int sec;
};

// commutative and associative (the tie-break is by (i, j), not by position), so lanes may hold any subset of the combinations
// (field-wise selects on values: nothing here may take an address, or the struct lands in scratch)
__device__ __forceinline__ MateSel mate_combine(MateSel a, MateSel b)
{
    const bool tie = a.cnt && b.cnt && a.cost == b.cost;
    const bool a_wins = !b.cnt || (a.cnt && (a.cost < b.cost || (tie && (a.i < b.i || (a.i == b.i && a.j < b.j)))));
    MateSel r;
    r.cost = a_wins ? a.cost : b.cost;
    r.i = a_wins ? a.i : b.i;
    r.j = a_wins ? a.j : b.j;
    r.cnt = tie ? a.cnt + b.cnt : (a_wins ? a.cnt : b.cnt);
    // the loser's best cost is the lowest cost it contributes to "the others" (an empty side has cost INT_MAX; a tie: the cost itself)
    r.sec = min(min(a.sec, b.sec), a_wins ? b.cost : a.cost);
    return r;
}

// a 64-bit sum as the int32 cost it is reported as
__device__ __forceinline__ int mate_clamp(int64_t v)
{
    return (int)min(v, (int64_t)INT_MAX - 1);
}

// candidate c's text_len (>= 0), from either request layout
__device__ __forceinline__ uint32_t mate_text_len(const KArgs &a, uint32_t c)
{
    const int tl = (a.p.flags & AIM_FLAG_REQ8) ? (int)reinterpret_cast<const aim_request8_t *>(a.req)[c].text_len : a.req[c].text_len;
    return (uint32_t)max(tl, 0);
}

// W = ma.lanes consecutive lanes per read pair (a wavefront holds 64 / W read pairs). Lane l of a read pair takes the combinations
// q = l, l + W, ... of its K1 * K2 (q = i * K2 + j), so a read pair of any size is a loop over chunks of W combinations; the lanes'
// partial results meet in a butterfly of log2(W) lane exchanges after the loop (uniform control flow). Lane 0 of the read pair writes
// aim_mate_t (two 16-B stores) and, for a proper choice, the two sel entries.
// a.req / a.p.flags: the batch's requests (text_len); res: the score-only rows; best: group_select_kernel's rows (never nullptr).
// Every index is clamped: a CSR or text_pos the host checks would refuse yields unspecified rows, never an access outside
// roff[0 .. n_reads], res / req / tpos[0 .. n_pairs) and best / sel[0 .. n_reads).
__global__ __launch_bounds__(256) void mate_select_kernel(KArgs a, MateArgs ma, const aim_result_t *res, const uint64_t *tpos, const uint32_t *roff,
                                                          const aim_best_t *best, uint32_t *sel, aim_mate_t *mates)
{
    const uint32_t W = ma.lanes;                         // (a power of two)
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const uint64_t m64 = t >> (uint32_t)__builtin_ctz(W);
    if (m64 >= ma.n_mates) return;                       // (whole read pairs leave: W divides the wavefront)
    const uint32_t m = (uint32_t)m64, l = (uint32_t)t & (W - 1u);
    const uint32_t n = a.n_pairs, ra = 2u * m, rb = ra + 1u;
    const uint32_t a0 = min(roff[ra], n), a1 = min(max(roff[rb], a0), n);
    const uint32_t b0 = min(roff[rb], n), b1 = min(max(roff[rb + 1u], b0), n);
    const uint32_t K1 = a1 - a0, K2 = b1 - b0;
    MateSel v{INT_MAX, UINT_MAX, UINT_MAX, 0u, INT_MAX};
    if (K2) {
        // q = i * K2 + j advances by W per step: (i, j) += (W / K2, W % K2) with one carry
        const uint32_t di = W / K2, dj = W - di * K2;
        uint32_t i = l / K2, j = l - i * K2;
        while (i < K1) {
            const uint32_t ci = a0 + i, cj = b0 + j;
            const uint64_t ti = tpos[ci], tj = tpos[cj];
            if (res[ci].status == AIM_PAIR_OK && res[cj].status == AIM_PAIR_OK && ((ti ^ tj) & AIM_REF_MINUS_STRAND)) {
                // f: the strand-0 candidate, r: the strand-1 candidate
                const bool i_minus = (ti & AIM_REF_MINUS_STRAND) != 0;
                const uint64_t si = ti & ~AIM_REF_MINUS_STRAND, sj = tj & ~AIM_REF_MINUS_STRAND;
                const uint64_t start_f = i_minus ? sj : si, start_r = i_minus ? si : sj;
                const uint64_t span = start_r + mate_text_len(a, i_minus ? ci : cj) - start_f;   // end_r - start_f
                if (start_f <= start_r && span >= (uint64_t)ma.min_span && span <= (uint64_t)ma.max_span)
                    v = mate_combine(v, MateSel{mate_clamp((int64_t)res[ci].score + res[cj].score), ci, cj, 1u, INT_MAX});
            }
            i += di;
            j += dj;
            if (j >= K2) {
                j -= K2;
                ++i;
            }
        }
    }
    for (uint32_t d = 1; d < W; d <<= 1) {               // (uniform: every lane of the wavefront that is still here takes part)
        MateSel o;
        o.cost = __shfl_xor(v.cost, (int)d, kWave);
        o.i = __shfl_xor(v.i, (int)d, kWave);
        o.j = __shfl_xor(v.j, (int)d, kWave);
        o.cnt = __shfl_xor(v.cnt, (int)d, kWave);
        o.sec = __shfl_xor(v.sec, (int)d, kWave);
        v = mate_combine(v, o);
    }
    if (l) return;
    const aim_best_t ba = best[ra], bb = best[rb];
    const bool has_a = ba.n_best != 0, has_b = bb.n_best != 0;
    uint4 lo = make_uint4(has_a ? ba.best_pair : UINT_MAX, has_b ? bb.best_pair : UINT_MAX, (uint32_t)INT_MAX, (uint32_t)INT_MAX);
    uint4 hi = make_uint4(0u, 0u, 0u, 0u);               // n_best, flags, pad
    if (has_a && has_b) {
        const int unpaired = mate_clamp((int64_t)ba.best_score + bb.best_score + ma.unpaired_penalty);
        if (v.cnt && v.cost <= unpaired) {               // (a tie goes to the proper combination)
            lo = make_uint4(v.i, v.j, (uint32_t)v.cost, (uint32_t)v.sec);
            hi.x = v.cnt;
            hi.y = AIM_MATE_PROPER;
            sel[ra] = v.i;
            sel[rb] = v.j;
        } else {
            lo.z = (uint32_t)unpaired;
            lo.w = (uint32_t)(v.cnt ? v.cost : INT_MAX);
        }
    }
    if (mates) {
        uint4 *out = reinterpret_cast<uint4 *>(mates + m);
        out[0] = lo;
        out[1] = hi;
    }
}

void mate_select_launch(const KArgs &ka, MateArgs ma, uint32_t n_reads, const aim_result_t *res, const uint64_t *tpos, const uint32_t *roff,
                        const aim_best_t *best, uint32_t *sel, aim_mate_t *mates, hipStream_t s)
{
    // lanes per read pair: the power of two that covers an average read pair's combinations (any value gives the same rows)
    ma.n_mates = n_reads / 2;
    const uint64_t k = ((uint64_t)ka.n_pairs + n_reads - 1) / n_reads, combos = k * k;
    ma.lanes = 1;
    while (ma.lanes < (uint32_t)kWave && ma.lanes < combos) ma.lanes <<= 1;
    const uint64_t threads = (uint64_t)ma.n_mates * ma.lanes;
    hipLaunchKernelGGL(mate_select_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s, ka, ma, res, tpos, roff, best, sel, mates);
}
#endif  // AIM_TU_GROUPS

}  // namespace aim
