// pair_secondary.hpp -- the device side of AIM_FEATURE_PAIR_SECONDARY (aim_hip.h, rule 17c): rule 14c's pairing over every slot rule 16c
// part 2 gave a role, secondaries included, and a MAPQ per read from the runner-up among the combinations.
//
//   * pair_sec_rescue_rows_kernel: pair_rescue_rows_kernel with the slots that take part read from d_sec and the anchor of a rescue the
//     mate's representative -- the slot of role 1 in the family of lowest j -- instead of its lowest mapped slot.
//   * pair_sec_select_kernel: rule 14c's choice over those slots and the rescue rows -> aim_map_pair_t; for a taken combination a
//     second pass of K broadcasts with (vi, vj) known gives each read the best cost and the ties among the combinations that place it
//     elsewhere -> aim_map_pair_mapq_t; apply, fused: the chosen slot's MAPQ into d_sec, a chosen secondary and its locus record
//     exchange roles, a chosen rescue row is folded into slot 0 as in rule 14c and becomes a one-member family.
//   * map_mates_sec_kernel: map_mates_kernel with the mate's representative read from d_sec.
//
// The lane layout, the candidate, the span and the butterfly are pair.hpp's: a read pair has G = 4, 8 or 16 consecutive lanes by K,
// candidate i of BOTH reads and its two d_sec entries in lane i. Role and family of another slot come from shuffles inside the group,
// the representative from a min-butterfly over family << 8 | lane. Both span bounds come from the arguments, or from an
// aim_pair_estimate_t in device memory when the caller passes one (two uniform 64-bit loads): one kernel serves both cases.
//
// Apply: a read pair's slots and d_sec entries are read and written by its own group alone, and every load of them comes before the
// stores in program order of the same lanes, so nothing depends on the grid. No LDS, no scratch, no atomics, vector stores only.
#pragma once

#include <climits>

#include "aim_device.hpp"
#include "chain_class.hpp"
#include "pair.hpp"

namespace aim {

struct PairSecArgs {
    PairArgs p;                           // rule 14c's arguments, min_span / max_span the fallback when est is given
    int32_t score_unit;
    aim_sec_slot_t *sec;                  // [n_reads * K]; written by select's apply alone
    const aim_chain_t *chains;            // [n_reads * K]                              (select kernel)
    const aim_pair_estimate_t *est;       // or nullptr: the bounds are p's
    aim_map_pair_mapq_t *pair_mapq;       // [n_reads / 2]                              (select kernel)
};

struct MatesSecArgs {
    MatesArgs m;
    const aim_sec_slot_t *sec;
};

#ifdef AIM_TU_PAIR_SECONDARY   // the kernels live in tu_pair_secondary.hip alone; capi_pair_secondary.hip sees the arguments and the launchers

static_assert(sizeof(aim_map_pair_mapq_t) == 16 && sizeof(aim_sec_slot_t) == 8 && sizeof(aim_chain_t) == 16, "rows of 4, 2 and 4 dwords");

constexpr uint32_t kPairSecOwnPlus = 40;   // pairing lifts a read's own MAPQ by this much at the most (bwa-mem's paired MAPQ)

__device__ __forceinline__ PairArgs pair_sec_bounds(const PairSecArgs &s)
{
    PairArgs a = s.p;
    if (s.est) {                          // (uniform: the kernel in front of this one on the stream wrote it)
        a.min_span = s.est->min_span;
        a.max_span = s.est->max_span;
    }
    return a;
}

// A slot of rule 17c: pair_load_slot's candidate, taking part when it is mapped and d_sec gave it a role; s0 is its first d_sec dword.
__device__ __forceinline__ PairCand pair_sec_load(const PairArgs &a, const aim_sec_slot_t *sec, bool live, uint64_t slot, uint32_t *s0)
{
    PairCand c = pair_load_slot(a, live, slot);
    *s0 = live ? reinterpret_cast<const uint32_t *>(sec)[slot * 2u] : 0u;
    if (!(*s0 & 0xffu)) c.fl &= ~1u;
    return c;
}

// The lane of the read's representative -- role 1, the lowest family -- in every lane of the group, or G when the read has none.
__device__ __forceinline__ uint32_t pair_sec_rep(uint32_t s0, bool part, uint32_t cand, uint32_t G)
{
    uint32_t key = (part && (s0 & 0xffu) == 1u) ? ((s0 & 0xff00u) | cand) : 0xffffu;
    for (uint32_t d = 1; d < G; d <<= 1) key = min(key, (uint32_t)__shfl_xor((int)key, (int)d, (int)G));
    return key == 0xffffu ? G : key & 0xffu;
}

__global__ __launch_bounds__(kPairThreads) void pair_sec_rescue_rows_kernel(PairSecArgs s, uint32_t G)
{
    const PairArgs a = pair_sec_bounds(s);
    const uint32_t kPairs = kPairThreads / G;
    const uint32_t cand = threadIdx.x & (G - 1u);
    const uint32_t base = (threadIdx.x & (uint32_t)(kWave - 1)) & ~(G - 1u);
    const uint32_t gm = (1u << G) - 1u;
    const uint32_t n_mates = a.n_reads / 2u, n_blocks = (n_mates + kPairs - 1u) / kPairs;
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint32_t m = blk * kPairs + threadIdx.x / G;
        const bool pair_live = m < n_mates, live = pair_live && cand < a.K;
        uint32_t sa, sb;
        const PairCand A = pair_sec_load(a, s.sec, live, 2u * m * a.K + cand, &sa), B = pair_sec_load(a, s.sec, live, (2u * m + 1u) * a.K + cand, &sb);
        const uint32_t rep_a = pair_sec_rep(sa, A.fl & 1u, cand, G), rep_b = pair_sec_rep(sb, B.fl & 1u, cand, G);
        const bool none_proper = !((uint32_t)(__ballot(pair_mapped_row(a, A, B, cand, G).cnt != 0u) >> base) & gm);
        for (uint32_t side = 0; side < 2u; ++side) {                        // side: the read b of the row; its mate is the anchor's read
            const uint32_t b = 2u * m + side;
            const uint32_t rep = side ? rep_a : rep_b;                       // the mate's representative
            const PairCand anchor = pair_bcast(side ? A : B, rep & (G - 1u), G);
            const uint32_t L = pair_read_len(a, pair_live, b);
            int64_t lo = 0, hi = 0;
            if ((a.options & AIM_PAIR_RESCUE) && rep < G && none_proper && L) {   // the rescue is tried
                int64_t c_lo = 0, c_hi = a.ref_len;
                if (a.contig && anchor.contig < a.n_contigs) {               // (no load outside the table)
                    c_lo = a.contig_start[anchor.contig];
                    c_hi = c_lo + a.contig_len[anchor.contig];
                }
                const int64_t P = (int64_t)((uint64_t)anchor.pos_hi << 32 | anchor.pos_lo);
                if (anchor.fl & 2u) {
                    const int64_t E = P + anchor.span;
                    lo = max(E - a.max_span, c_lo);
                    hi = min(E - a.min_span + L, c_hi);
                } else {
                    lo = max(P + a.min_span - L, c_lo);
                    hi = min(P + a.max_span, c_hi);
                }
            }
            const bool row = hi - lo >= (int64_t)L && L;                     // else the empty row: lengths 0, text_pos 0
            if (pair_live && cand == 0) {
                const uint64_t tp = row ? ((uint64_t)lo | ((anchor.fl & 2u) ? 0ull : AIM_REF_MINUS_STRAND)) : 0ull;
                reinterpret_cast<uint4 *>(a.res_req)[b] = make_uint4(row ? L : 0u, row ? (uint32_t)(hi - lo) : 0u, 0u, b);
                reinterpret_cast<uint2 *>(a.res_text_pos)[b] = make_uint2((uint32_t)tp, (uint32_t)(tp >> 32));
            }
            if (row) {                                                       // the read as given, at the stride of the rescue alignment
                const uint2 *src = reinterpret_cast<const uint2 *>(a.reads + (uint64_t)b * a.read_size);
                uint2 *dst = reinterpret_cast<uint2 *>(a.res_patterns + (uint64_t)b * a.rescue_size);
                for (uint32_t w = cand; w < a.read_size / 8u; w += G) dst[w] = src[w];
            }
        }
    }
}

// pair_add that also says whether the combination was proper: the second pass asks that alone and needs no coordinates again
__device__ __forceinline__ PairSel pair_sec_add(const PairArgs &a, PairSel v, PairCand x, PairCand y, uint32_t i, uint32_t j, bool *ok)
{
    const int64_t sp = pair_span(a, x, y);
    *ok = sp >= 0;
    const PairSel one = {*ok ? pair_clamp((int64_t)x.score + y.score) : INT_MAX, *ok ? (i << 8 | j) : UINT_MAX, *ok ? 1u : 0u, INT_MAX,
                         *ok ? (uint32_t)sp : 0u, *ok ? (uint32_t)((uint64_t)sp >> 32) : 0u};
    return pair_combine(v, one);
}

// What the second pass keeps per read: the lowest cost among the proper combinations that place the read elsewhere, and how many of
// them cost what the taken one costs. Both reduce over lanes by min and by sum.
struct PairSecAlt {
    int alt_a, alt_b;
    uint32_t tied;                        // read 2m's count | read 2m + 1's << 16 (at most 17 * 17 each)
};

// the proper combination (i, j) of scores x and y
__device__ __forceinline__ PairSecAlt pair_sec_alt_add(PairSecAlt t, bool ok, int x, int y, uint32_t i, uint32_t j, uint32_t vi, uint32_t vj, int c)
{
    const int cost = pair_clamp((int64_t)x + y);
    const bool for_a = ok && i != vi, for_b = ok && j != vj;
    t.alt_a = for_a ? min(t.alt_a, cost) : t.alt_a;
    t.alt_b = for_b ? min(t.alt_b, cost) : t.alt_b;
    t.tied += ((for_a && cost == c) ? 1u : 0u) | ((for_b && cost == c) ? 0x10000u : 0u);
    return t;
}

// rule 16c's anchor_cap of a slot's own chain
__device__ __forceinline__ uint32_t pair_sec_cap(const aim_chain_t *chains, uint64_t slot)
{
    const uint2 ch = *reinterpret_cast<const uint2 *>(reinterpret_cast<const uint32_t *>(chains) + slot * 4u);   // score, n_anchors | reserved << 16
    return ch.x ? 6u * min(ch.y & 0xffffu, 10u) : 0u;
}

__device__ __forceinline__ uint32_t pair_sec_mapq(uint32_t tied, int alt, int c, int32_t unit)
{
    return tied ? 0u : alt == INT_MAX ? 60u : quot60(6ull * (uint64_t)max((int64_t)alt - c, (int64_t)0), (uint64_t)unit);
}

// Apply to read r of the pair, whose chosen index is v (uniform over the group) and whose MAPQ is mapq; v_s0 is the first d_sec dword
// of the chosen slot. anchor_*: of the mate's representative, for a chosen rescue row.
__device__ __forceinline__ void pair_sec_apply(const PairSecArgs &s, const PairArgs &a, uint32_t r, uint32_t cand, uint32_t v, uint32_t mapq, uint32_t v_s0, uint32_t anchor_contig, uint64_t anchor_family_slot)
{
    const uint32_t K = a.K;
    const uint64_t slot = (uint64_t)r * K + cand;
    uint2 *out = reinterpret_cast<uint2 *>(s.sec) + slot;
    const uint2 own = *out;                                                  // (the lane's own entry: no other lane writes it)
    const uint32_t s0 = own.x, s1 = own.y;
    if (v == K) {                                                            // rule 14c's apply; the read becomes a one-member family 0
        if (cand == 0) {
            const uint4 *row = reinterpret_cast<const uint4 *>(a.res_sam) + (uint64_t)r * 3u;
            const uint4 w0 = row[0], w1 = row[1], w2 = row[2];
            const uint32_t mq = reinterpret_cast<const uint32_t *>(a.cls)[anchor_family_slot * 2u + 1u] & 0x00ff0000u;   // the chain MAPQ of the anchor's family
            uint4 *dst = reinterpret_cast<uint4 *>(a.sam) + slot * 3u;
            dst[0] = w0;
            dst[1] = make_uint4(w1.x, w1.y, w1.z + a.cigar_base, w1.w);    // cigar_offset
            dst[2] = make_uint4(w2.x + a.md_base, w2.y, w2.z, w2.w);       // md_offset
            const uint32_t L = pair_read_len(a, true, r);
            reinterpret_cast<uint2 *>(a.seg)[slot] = make_uint2(L << 16, L | (AIM_SEG_VALID | AIM_SEG_LEFT_OPEN | AIM_SEG_RIGHT_OPEN) << 16);
            if (a.contig) a.contig[slot] = anchor_contig;
            uint32_t *c1 = reinterpret_cast<uint32_t *>(a.cls) + slot * 2u + 1u;
            *c1 = (*c1 & ~0x00ff0000u) | mq;
            *out = make_uint2(1u | mapq << 16, 1u | AIM_SEC_COMPLETE << 8 | 65535u << 16);
        } else {
            uint32_t *s1p = reinterpret_cast<uint32_t *>(a.seg) + slot * 2u + 1u;
            *s1p &= ~(AIM_SEG_VALID << 16);
            *out = make_uint2(0u, 0u);
        }
        return;
    }
    const uint32_t v_role = v_s0 & 0xffu, v_fam = (v_s0 >> 8) & 0xffu;
    if (cand == v) {
        if (v_role == 1u) {
            *out = make_uint2((s0 & 0xff00ffffu) | mapq << 16, s1);
        } else {                                                             // promoted: the locus record, no alignment runner-up of its own
            const uint32_t flags = (((s1 >> 8) & 0xffu) & ~AIM_SEC_SWAPPED) | (v != v_fam ? AIM_SEC_SWAPPED : 0u);
            *out = make_uint2(1u | v_fam << 8 | mapq << 16, (s1 & 0xffu) | flags << 8);
        }
    } else if (v_role != 1u && (s0 & 0xffffu) == (1u | v_fam << 8)) {        // demoted: its family's locus record until now
        *out = make_uint2((s0 & 0xff00ff00u) | 2u, s1);
    }
}

__global__ __launch_bounds__(kPairThreads) void pair_sec_select_kernel(PairSecArgs s, uint32_t G)
{
    const PairArgs a = pair_sec_bounds(s);
    const uint32_t kPairs = kPairThreads / G;
    const uint32_t cand = threadIdx.x & (G - 1u);
    const uint32_t base = (threadIdx.x & (uint32_t)(kWave - 1)) & ~(G - 1u);
    const uint32_t gm = (1u << G) - 1u, K = a.K;
    const uint32_t n_mates = a.n_reads / 2u, n_blocks = (n_mates + kPairs - 1u) / kPairs;
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint32_t m = blk * kPairs + threadIdx.x / G;
        const bool pair_live = m < n_mates, live = pair_live && cand < K;
        const uint32_t ra = 2u * m, rb = ra + 1u;
        uint32_t sa0, sb0;
        const PairCand A = pair_sec_load(a, s.sec, live, ra * K + cand, &sa0), B = pair_sec_load(a, s.sec, live, rb * K + cand, &sb0);
        const uint32_t rep_a = pair_sec_rep(sa0, A.fl & 1u, cand, G), rep_b = pair_sec_rep(sb0, B.fl & 1u, cand, G);
        const bool has_a = rep_a < G, has_b = rep_b < G;
        // lane i's row of combinations; bit j of `proper`: (i, j) is proper -- bit K: (i, K) with read 2m + 1's rescue row, bit 31: (K, i)
        PairSel v = pair_none();
        uint32_t proper = 0;
        for (uint32_t j = 0; j < K; ++j) {
            bool ok;
            v = pair_sec_add(a, v, A, pair_bcast(B, j, G), cand, j, &ok);
            proper |= (ok ? 1u : 0u) << j;
        }
        // of the two representatives -- the anchors of the rescue -- what the choice needs: the contig and the score
        const uint32_t contig_a = (uint32_t)__shfl((int)A.contig, (int)(rep_a & (G - 1u)), (int)G), contig_b = (uint32_t)__shfl((int)B.contig, (int)(rep_b & (G - 1u)), (int)G);
        const bool both = has_a && has_b;
        const int unpaired = pair_clamp((int64_t)__shfl(A.score, (int)(rep_a & (G - 1u)), (int)G) + __shfl(B.score, (int)(rep_b & (G - 1u)), (int)G) + a.unpaired_penalty);
        const bool rescue = (a.options & AIM_PAIR_RESCUE) && !((uint32_t)(__ballot(v.cnt != 0u) >> base) & gm);
        const bool tried_a = rescue && has_b && pair_read_len(a, pair_live, ra), tried_b = rescue && has_a && pair_read_len(a, pair_live, rb);
#pragma unroll 1
        for (uint32_t side = 0; side < 2u; ++side) {                           // (i, K) with read 2m + 1's row, then (K, j) with read 2m's; (K, K) is excluded
            const PairCand R = pair_load(a.res_sam, side ? tried_a : tried_b, side ? ra : rb, true, side ? contig_b : contig_a);
            bool ok;
            v = pair_sec_add(a, v, side ? B : A, R, side ? K : cand, side ? cand : K, &ok);
            proper |= (ok ? 1u : 0u) << (side ? 31u : K);
        }
        v = pair_butterfly(v, G);
        const uint32_t vi = v.ij >> 8, vj = v.ij & 0xffu;
        const bool take = v.cnt && (!both || v.cost <= unpaired);              // (a tie goes to the proper combination)
        if (pair_live && cand == 0) {                                          // aim_map_pair_t, as rule 14c writes it
            uint4 lo = make_uint4(has_a ? ra * K + rep_a : UINT_MAX, has_b ? rb * K + rep_b : UINT_MAX, (uint32_t)INT_MAX, (uint32_t)INT_MAX);
            uint4 hi = make_uint4(0u, (tried_a ? AIM_PAIR_RESCUE_TRIED_A : 0u) | (tried_b ? AIM_PAIR_RESCUE_TRIED_B : 0u), 0u, 0u);
            if (take) {
                lo = make_uint4(ra * K + vi, rb * K + vj, (uint32_t)v.cost, (uint32_t)v.sec);
                hi.x = v.cnt;
                hi.y |= AIM_PAIR_PROPER | (vi == K ? AIM_PAIR_RESCUED_A : 0u) | (vj == K ? AIM_PAIR_RESCUED_B : 0u);
                hi.z = v.span_lo;
                hi.w = v.span_hi;
            } else if (both) {
                lo.z = (uint32_t)unpaired;
                lo.w = (uint32_t)(v.cnt ? v.cost : INT_MAX);
            }
            uint4 *out = reinterpret_cast<uint4 *>(a.pairs + m);
            out[0] = lo;
            out[1] = hi;
        }
        // the second pass: with (vi, vj) known, what places either read elsewhere (of v, the cost alone is still needed)
        const int c = v.cost;
        PairSecAlt t = {INT_MAX, INT_MAX, 0u};
#pragma unroll 1
        for (uint32_t j = 0; j < K; ++j) t = pair_sec_alt_add(t, (proper >> j) & 1u, A.score, __shfl(B.score, (int)j, (int)G), cand, j, vi, vj, c);
        // (a bit of `proper` for a rescue row implies that the row was tried: one address per group, a broadcast)
        const int res_b = tried_b ? (int)reinterpret_cast<const uint32_t *>(a.res_sam)[(uint64_t)rb * 12u + 1u] : 0;
        const int res_a = tried_a ? (int)reinterpret_cast<const uint32_t *>(a.res_sam)[(uint64_t)ra * 12u + 1u] : 0;
        t = pair_sec_alt_add(t, (proper >> K) & 1u, A.score, res_b, cand, K, vi, vj, c);
        t = pair_sec_alt_add(t, proper >> 31, res_a, B.score, K, cand, vi, vj, c);
#pragma unroll 1
        for (uint32_t d = 1; d < G; d <<= 1) {
            t.alt_a = min(t.alt_a, __shfl_xor(t.alt_a, (int)d, (int)G));
            t.alt_b = min(t.alt_b, __shfl_xor(t.alt_b, (int)d, (int)G));
            t.tied += (uint32_t)__shfl_xor((int)t.tied, (int)d, (int)G);
        }
        if (both && rep_a != vi) t.alt_a = min(t.alt_a, unpaired);
        if (both && rep_b != vj) t.alt_b = min(t.alt_b, unpaired);
        const uint32_t tied_a = t.tied & 0xffffu, tied_b = t.tied >> 16;
        // the chosen slots' own MAPQ and the cap of their chains
        uint32_t va0 = 0, vb0 = 0, cap_a = 0, cap_b = 0;                       // one address per group: a broadcast
        if (take && vi < K) {
            va0 = reinterpret_cast<const uint32_t *>(s.sec)[((uint64_t)ra * K + vi) * 2u];
            cap_a = pair_sec_cap(s.chains, (uint64_t)ra * K + vi);
        }
        if (take && vj < K) {
            vb0 = reinterpret_cast<const uint32_t *>(s.sec)[((uint64_t)rb * K + vj) * 2u];
            cap_b = pair_sec_cap(s.chains, (uint64_t)rb * K + vj);
        }
        const uint32_t own_a = (vi != K && (va0 & 0xffu) == 1u) ? (va0 >> 16) & 0xffu : 0u, own_b = (vj != K && (vb0 & 0xffu) == 1u) ? (vb0 >> 16) & 0xffu : 0u;
        const uint32_t pm_a = pair_sec_mapq(tied_a, t.alt_a, c, s.score_unit), pm_b = pair_sec_mapq(tied_b, t.alt_b, c, s.score_unit);
        const uint32_t lift_a = max(own_a, min(pm_a, own_a + kPairSecOwnPlus)), lift_b = max(own_b, min(pm_b, own_b + kPairSecOwnPlus));
        uint32_t mapq_a = min(lift_a, cap_a), mapq_b = min(lift_b, cap_b);
        if (vi == K) mapq_a = min(lift_a, mapq_b);                             // a rescue row is as sure as its anchor's read, at the most
        if (vj == K) mapq_b = min(lift_b, mapq_a);
        if (pair_live && cand == 0) {
            uint4 q = make_uint4((uint32_t)INT_MAX, (uint32_t)INT_MAX, 0u, 0u);
            if (take)
                q = make_uint4((uint32_t)t.alt_a, (uint32_t)t.alt_b, mapq_a | mapq_b << 8 | pm_a << 16 | pm_b << 24,
                               own_a | own_b << 8 | min(tied_a, 255u) << 16 | min(tied_b, 255u) << 24);
            reinterpret_cast<uint4 *>(s.pair_mapq)[m] = q;
        }
        // apply: each lane stores to its own slots alone, after everything it loads of them; what it needs of other slots of the pair
        // -- the chosen slot's d_sec, the anchor's family and contig -- is loaded in every lane in front of the first store
        if (take && live) {
            uint32_t fam_a = 0, fam_b = 0;                                     // of the representatives: the anchors of a chosen rescue row
            if (vj == K) fam_a = min((reinterpret_cast<const uint32_t *>(s.sec)[((uint64_t)ra * K + rep_a) * 2u] >> 8) & 0xffu, K - 1u);
            if (vi == K) fam_b = min((reinterpret_cast<const uint32_t *>(s.sec)[((uint64_t)rb * K + rep_b) * 2u] >> 8) & 0xffu, K - 1u);
            pair_sec_apply(s, a, ra, cand, vi, mapq_a, va0, contig_b, (uint64_t)rb * K + fam_b);
            pair_sec_apply(s, a, rb, cand, vj, mapq_b, vb0, contig_a, (uint64_t)ra * K + fam_a);
        }
    }
}

// One record per lane. The mate's representative comes from d_sec (as apply left it), never from other lanes' records.
__global__ __launch_bounds__(kPairThreads) void map_mates_sec_kernel(MatesSecArgs s)
{
    const MatesArgs &a = s.m;
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
        uint32_t ms = UINT_MAX, best = 0x100u;                                 // the mate's reference record: its representative ...
        for (uint32_t i = 0; i < K; ++i) {
            const uint32_t x = reinterpret_cast<const uint32_t *>(s.sec)[(uint64_t)(mate * K + i) * 2u];
            const uint32_t fam = (x >> 8) & 0xffu;
            if ((x & 0xffu) == 1u && fam < best) {
                best = fam;
                ms = mate * K + i;
            }
        }
        const bool mate_mapped = ms != UINT_MAX;
        if (mate_mapped && proper && other - mate * K < K) ms = other;         // ... or, in a proper pair, its chosen slot
        const bool reverse = (w2.z & AIM_SAM_REVERSE) != 0, mapped = !(w2.z & AIM_SAM_UNMAPPED);
        const bool chosen = proper && slot == own && !(w2.z & AIM_SAM_SECONDARY);   // (a 0x100 record is never one of the pair)
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

void pair_sec_rescue_rows_launch(const PairSecArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s)
{
    hipLaunchKernelGGL(pair_sec_rescue_rows_kernel, dim3(grid), dim3(kPairThreads), 0, s, a, lanes);
}

void pair_sec_select_launch(const PairSecArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s)
{
    hipLaunchKernelGGL(pair_sec_select_kernel, dim3(grid), dim3(kPairThreads), 0, s, a, lanes);
}

void map_mates_sec_launch(const MatesSecArgs &a, uint32_t grid, hipStream_t s)
{
    hipLaunchKernelGGL(map_mates_sec_kernel, dim3(grid), dim3(kPairThreads), 0, s, a);
}
#else
void pair_sec_rescue_rows_launch(const PairSecArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s);
void pair_sec_select_launch(const PairSecArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s);
void map_mates_sec_launch(const MatesSecArgs &a, uint32_t grid, hipStream_t s);
#endif

}  // namespace aim
