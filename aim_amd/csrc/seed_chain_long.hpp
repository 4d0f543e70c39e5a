// seed_chain_long.hpp -- colinear chaining for long reads (aim_hip.h, AIM_FEATURE_SEED_CHAIN_LONG): aim_seed_chain_device's rule over
// minimizer seeds with a caller-chosen hit cap H = 1 024 .. 8 192 per strand and read rows of up to 65 528 bases.
//
//   * seed_chain_long_kernel: one read per 64-lane wavefront (a workgroup is one wavefront), persistent over the reads through xcd_unit,
//     like seed_chain_minimizer_kernel (seed_chain.hpp), whose phases it keeps: hits, sort, chain, rank for strand 0 and then strand 1
//     over the same LDS arrays, and one fill. Everything per read lives in LDS or registers; no scratch, no traffic between workgroups.
//
// SHARED STEPS. The k-mer code, the selection, the index lookup and the sort are seed.hpp's steps; the chain DP, the min_votes filter
// and the fill's writer are seed_chain.hpp's, instantiated with ChainLong's widths. What is this kernel's own, and why it is a kernel
// of its own rather than a parameter of seed_chain_minimizer_kernel: the tiled hit phase, the runtime hit cap, and the rank key.
//
// The phases, where they differ from seed_chain.hpp's:
//   hits     LDS does not grow with read_size. The strand's query is walked in tiles of kSeedLongTile k-mer positions [t0, t1); a tile
//            stages, from global memory, the bytes of the positions [t0 - (w - 1), t1 + (w - 1)) clipped to the query, k - 1 more for the
//            last k-mer: strand 0 reads them forward from the row's start, strand 1 is the reverse complement and reads the row from the
//            far end, with the complement folded into the code as in seed.hpp. The tile then gets its own order keys, and the selection
//            is the local form of the rule (L + R + 1 >= min(w, n), both runs capped at w - 1), which never looks further than the
//            halo. Tiles ascend, a step takes 64 consecutive positions and a wave prefix sum places the runs: the hits are appended in
//            (j, p) order, so the truncation at H drops what the rule drops. A hit is the 48-bit anchor p << 16 | j in a 64-bit entry.
//   chain    seed_chain_dp's lane ring, one DPP max-reduction per step, no backtrack pass. dq < 65 536 and band <= 4 096 bound an
//            admissible dp by 69 631; f <= H * 14 < 2^17, so score << 6 | nearness has 23 bits and ends[root] = f << 13 | (8191 - index)
//            has 30.
//   rank     (score, strand, p_lo, q_lo) no longer fits 64 bits. Within a strand the anchors are sorted by (p, j) and distinct, so the
//            sorted index of a chain's root orders (p_lo, q_lo): the rank key is (kSeedLongMaxScore - score) << 14 | strand << 13 | root
//            index, 31 bits, and (p_lo, q_lo) are fetched from the root's anchor when the round's winner is kept.
//
// LDS BANKS. As seed_chain.hpp: seed_sort on 64-bit entries, consecutive entries everywhere else.
//
// OCCUPANCY. LDS per workgroup = 14 * H bytes (8 of anchors, 4 of ends, 2 of counts per hit) + kSeedLongTileBytes = 2 912 B of tile
// buffers (608 B of bases, 2 304 B of keys), whatever read_size is. In granules of 1 280 B and wavefronts per CU:
//         H       LDS          granules   wavefronts per CU
//     1 024    17 248 B           14             9
//     2 048    31 584 B           25             5
//     4 096    60 256 B           48             2
//     8 192   117 600 B           92             1
// LDS-bound throughout; above 64 KB the launch raises hipFuncAttributeMaxDynamicSharedMemorySize. kSeedChainLongMaxVgpr = 128 is the
// register budget of 4 wavefronts per SIMD, which LDS never lets it reach. No scratch, no static LDS.
#pragma once

#include "seed_chain.hpp"

namespace aim {

constexpr int kSeedChainLongMaxVgpr = 128;     // the bound tests/test_seed_chain_long_cpu.py checks in the code object
constexpr uint32_t kSeedLongTile = 512;        // k-mer positions per tile of the hit phase
constexpr uint32_t kSeedLongHalo = AIM_SEED_MAX_W - 1;                                                             // positions on each side
constexpr uint32_t kSeedLongTileRowBytes = (kSeedLongTile + 2 * kSeedLongHalo + kMinMaxK - 1 + 3 + 3 + 15) & ~15u;   // bases, dword-aligned at both ends
constexpr uint32_t kSeedLongTileKeyBytes = ((kSeedLongTile + 2 * kSeedLongHalo) * 4 + 15) & ~15u;
constexpr uint32_t kSeedLongTileBytes = kSeedLongTileRowBytes + kSeedLongTileKeyBytes;
constexpr uint32_t kSeedLongMaxScore = AIM_SEED_LONG_MAX_HITS * 14;   // f <= H * 14
static_assert(((uint64_t)kSeedLongMaxScore << 14 | 0x3FFFu) < (uint64_t)INT_MAX, "the rank key is a positive int32_t below INT_MAX");
static_assert(kSeedLongMaxScore < (1u << 17) && AIM_SEED_LONG_MAX_HITS == (1u << 13), "ends[] is f << 13 | index, the rank key score << 14 | strand << 13 | root");
static_assert(AIM_SEED_LONG_MAX_READ_SIZE < (1 << 16), "an anchor is p << 16 | j");

struct SeedChainLongArgs {
    SeedChainArgs c;
    uint32_t max_hits;       // H: a power of two, 1 024 .. AIM_SEED_LONG_MAX_HITS
};

// Dynamic LDS of one workgroup: anchors[H], ends[H], counts[H] and the tile buffers. It does not depend on read_size.
constexpr size_t seed_chain_long_lds_bytes(uint32_t max_hits) { return (size_t)max_hits * 14u + kSeedLongTileBytes; }
static_assert(seed_chain_long_lds_bytes(AIM_SEED_LONG_MAX_HITS) <= 160u * 1024u, "one workgroup fits a CU's LDS at the largest cap");

#ifdef AIM_TU_SEED_CHAIN_LONG   // the kernel lives in tu_seed_chain_long.hip alone; capi_pipeline.hip sees the arguments and the launcher

// seed_chain_append with the cap H and the anchor p << 16 | j. Returns the new count (wave-uniform; past H only "overflowed" matters).
__device__ __forceinline__ uint32_t seed_long_append(const SeedArgs &a, uint64_t *ks, uint32_t H, uint32_t count, uint32_t code, bool ok, uint32_t j, int lane)
{
    uint32_t b0;
    const uint32_t n = seed_run(a, H, code, ok, &b0);
    const uint32_t incl = seed_scan_add(n, lane);
    const uint32_t at = count + incl - n;
    for (uint32_t q = 0; q < n && at + q < H; ++q) ks[at + q] = ((uint64_t)a.pos[b0 + q] << ChainLong::kJBits) | j;
    return count + (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
}

// Rules 1-3 for strand s of a read of L bases at `g` (the row, dword-aligned): the kept hits into anchors[0, H). Returns the count.
__device__ __forceinline__ uint32_t seed_long_hits(const SeedArgs &a, const uint32_t *g, int32_t L, int s, uint32_t H, uint64_t *anchors, uint32_t *trow4,
                                                   uint32_t *tk, int lane)
{
    const int32_t k = a.sp.k;
    const uint32_t reach = min(a.sp.options >> 8, (uint32_t)AIM_SEED_MAX_W) - 1u;   // (w >= 1 is checked)
    const uint32_t n = L >= k ? (uint32_t)(L - k) + 1u : 0u;
    const uint32_t need = min(reach + 1u, n);                                       // min(w, n)
    const uint8_t *trow = reinterpret_cast<const uint8_t *>(trow4);
    uint32_t count = 0;
    for (uint32_t t0 = 0; t0 < n && count <= H; t0 += kSeedLongTile) {
        const uint32_t t1 = min(t0 + kSeedLongTile, n);
        const uint32_t klo = t0 > reach ? t0 - reach : 0u, khi = min(t1 + reach, n);       // the positions whose keys the tile needs
        // their bases are the query's [klo, khi + k - 1): these bytes of the read
        const int32_t b0 = s ? L - (int32_t)khi - (k - 1) : (int32_t)klo;
        const int32_t b1 = s ? L - (int32_t)klo : (int32_t)khi + (k - 1);
        const int32_t a0 = b0 & ~3;
        asm volatile("" ::: "memory");   // the previous tile's LDS reads are issued before this one lands
        for (int32_t w = lane; w < ((b1 - a0 + 3) >> 2); w += kWave) trow4[w] = g[(a0 >> 2) + w];
        asm volatile("" ::: "memory");
        for (uint32_t i = (uint32_t)lane; i < khi - klo; i += kWave) {   // keys
            bool ok = true;
            const uint32_t code = seed_code(trow - a0, L, (int32_t)(klo + i), k, s, &ok);   // trow[i] is the read's byte a0 + i
            tk[i] = ok ? min_hash(code) : kMinInvalid;
        }
        asm volatile("" ::: "memory");
        for (uint32_t base = t0; base < t1 && count <= H; base += kWave) {   // select, hits (rules 2-3)
            const uint32_t j = base + (uint32_t)lane;
            uint32_t key;
            const bool selected = seed_minimizer_selected(tk, klo, j, j < t1, n, reach, need, &key);
            count = seed_long_append(a, anchors, H, count, min_unhash(key), selected, j, lane);
        }
    }
    return count;
}

// One kept chain, in the lane that holds it. rank = (kSeedLongMaxScore - score) << 14 | strand << 13 | root index; all ones: none.
struct ChainLongSlot {
    uint32_t rank, n_anchors;
    uint64_t root, end;      // the anchors, p << 16 | j
};

// The sort, chain, rank and keep phases for strand s, whose `count` hits are in anchors[]. The strand's best chains, at most K, go to
// the lanes lane0 .. lane0 + K - 1 of `mine`; returns their number (wave-uniform).
__device__ __forceinline__ uint32_t seed_long_strand(const SeedArgs &a, uint32_t H, uint64_t *anchors, uint32_t *ends, uint16_t *counts, uint32_t count, int s,
                                                     uint32_t lane0, ChainLongSlot &mine, int lane)
{
    const uint32_t n = min(count, H);
    const uint32_t rounds = min((uint32_t)a.sp.max_cands, seed_chain_dp<ChainLong>(a, H, anchors, ends, counts, count, lane));
    // rank: round i's winner stays in lane lane0 + i
    uint32_t last = 0;
    for (uint32_t round = 0; round < rounds; ++round) {
        uint32_t best = INT_MAX, best_end = 0;                      // (the keys have 31 bits and stay below INT_MAX: none)
        for (uint32_t i = (uint32_t)lane; i < n; i += kWave) {
            const uint32_t e = ends[i];
            if (!e) continue;
            const uint32_t key = ((kSeedLongMaxScore - (e >> ChainLong::kEndBits)) << 14) | ((uint32_t)s << 13) | i;
            if ((round == 0 || key > last) && key < best) {
                best = key;
                best_end = ChainLong::kEndMask - (e & ChainLong::kEndMask);
            }
        }
        const uint32_t win = (uint32_t)wave_min_i32((int)best);
        // (rounds <= the number of chains and the keys are unique: every round finds one)
        const int src = __ffsll((unsigned long long)__ballot(best == win)) - 1;
        const uint32_t end_at = (uint32_t)__builtin_amdgcn_readlane((int)best_end, src);
        if ((uint32_t)lane == lane0 + round) {
            mine.rank = win;
            mine.root = anchors[win & ChainLong::kEndMask];
            mine.end = anchors[end_at];
            mine.n_anchors = counts[end_at];
        }
        last = win;
    }
    asm volatile("" ::: "memory");   // the next strand's hits land after these reads
    return rounds;
}

// Fill from the chains the lanes hold (lanes 0..15 strand 0, 16..31 strand 1): a chain's slot is the number of kept chains with a
// smaller rank key.
__device__ __forceinline__ void seed_long_fill(const SeedChainLongArgs &la, uint32_t r, int32_t L, const ChainLongSlot &mine, uint32_t n_kept,
                                               const uint32_t (&count)[2], int lane)
{
    const uint32_t K = (uint32_t)la.c.s.sp.max_cands;
    uint32_t rank = 0;
#pragma unroll
    for (int o = 0; o < 32; ++o) rank += (uint32_t)__builtin_amdgcn_readlane((int)mine.rank, o) < mine.rank ? 1u : 0u;
    ChainFound c;
    c.score = kSeedLongMaxScore - (mine.rank >> 14);
    c.strand = (mine.rank >> 13) & 1u;
    c.n_anchors = mine.n_anchors;
    c.p_lo = (int64_t)(mine.root >> ChainLong::kJBits);
    c.q_lo = (int64_t)(mine.root & ChainLong::kJMask);
    c.p_end = (int64_t)(mine.end >> ChainLong::kJBits);
    c.q_end = (int64_t)(mine.end & ChainLong::kJMask);
    seed_chain_write(la.c, la.max_hits, r, L, lane < 32 && mine.rank != UINT_MAX && rank < K, rank, c, min(K, n_kept), count, lane);
}

__global__ __launch_bounds__(64) void seed_chain_long_kernel(SeedChainLongArgs la)
{
    extern __shared__ __align__(16) char seed_long_smem[];
    const SeedArgs &a = la.c.s;
    debug_poison_lds(a.dbg_poison_lds, a.dbg_lds_bytes, seed_long_smem);
    const int lane = threadIdx.x;
    const uint32_t H = la.max_hits;
    const int32_t rs = a.sp.read_size;
    uint64_t *anchors = reinterpret_cast<uint64_t *>(seed_long_smem);                      // [H]
    uint32_t *ends = reinterpret_cast<uint32_t *>(seed_long_smem + (size_t)H * 8u);        // [H]
    uint16_t *counts = reinterpret_cast<uint16_t *>(seed_long_smem + (size_t)H * 12u);     // [H]
    uint32_t *trow4 = reinterpret_cast<uint32_t *>(seed_long_smem + (size_t)H * 14u);      // the tile's bases
    uint32_t *tk = reinterpret_cast<uint32_t *>(seed_long_smem + (size_t)H * 14u + kSeedLongTileRowBytes);   // the tile's order keys

    for (uint32_t it = 0;; ++it) {
        uint32_t r;
        if (!xcd_unit(a.n_reads, it, &r)) break;
        const int32_t L = min(max(a.read_len[r], 0), rs);
        const uint32_t *g = reinterpret_cast<const uint32_t *>(a.reads + (uint64_t)r * (uint64_t)rs);
        uint32_t count[2] = {0u, 0u};
        uint32_t n_kept = 0;
        ChainLongSlot mine = {UINT_MAX, 0, 0, 0};
#pragma unroll 1
        for (int s = 0; s < 2; ++s) {
            count[s] = seed_long_hits(a, g, L, s, H, anchors, trow4, tk, lane);
            n_kept += seed_long_strand(a, H, anchors, ends, counts, count[s], s, s ? 16u : 0u, mine, lane);
        }
        seed_long_fill(la, r, L, mine, n_kept, count, lane);
    }
}

void seed_chain_long_launch(const SeedChainLongArgs &a, uint32_t grid, size_t lds, hipStream_t s)
{
    if (lds > 64u * 1024u)
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&seed_chain_long_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(seed_chain_long_kernel, dim3(grid), dim3(kWave), lds, s, a);
}
#else
void seed_chain_long_launch(const SeedChainLongArgs &a, uint32_t grid, size_t lds, hipStream_t s);
#endif

}  // namespace aim
