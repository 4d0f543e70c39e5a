// seed_chain_long.hpp -- colinear chaining for long reads (aim_hip.h, AIM_FEATURE_SEED_CHAIN_LONG): aim_seed_chain_device's rule over
// minimizer seeds with a caller-chosen hit cap H = 1 024 .. 8 192 per strand and read rows of up to 65 528 bases.
//
//   * seed_chain_long_kernel: one read per 64-lane wavefront (a workgroup is one wavefront), persistent over the reads through xcd_unit,
//     like seed_chain_minimizer_kernel (seed_chain.hpp), whose phases it keeps: hits, sort, chain, rank for strand 0 and then strand 1
//     over the same LDS arrays, and one fill. Everything per read lives in LDS or registers; no scratch, no traffic between workgroups.
//
// What differs from seed_chain.hpp, and why this is a kernel of its own rather than a parameter of that one: every width below is part
// of seed_chain_strand's code, and that kernel's code object stays as it is.
//   hits     LDS does not grow with read_size. The strand's query is walked in tiles of kSeedLongTile k-mer positions [t0, t1); a tile
//            stages, from global memory, the bytes of the positions [t0 - (w - 1), t1 + (w - 1)) clipped to the query, k - 1 more for the
//            last k-mer: strand 0 reads them forward from the row's start, strand 1 is the reverse complement and reads the row from the
//            far end, with the complement folded into the code as in seed.hpp. The tile then gets its own order keys, and the selection
//            is the local form of the rule (L + R + 1 >= min(w, n), both runs capped at w - 1), which never looks further than the
//            halo. Tiles ascend, a step takes 64 consecutive positions and a wave prefix sum places the runs: the hits are appended in
//            (j, p) order, so the truncation at H drops what the rule drops. A hit is the 48-bit anchor p << 16 | j in a 64-bit entry.
//   chain    seed_chain_strand's lane ring, one DPP max-reduction per step, no backtrack pass. dq < 65 536 and band <= 4 096 bound an
//            admissible dp by 69 631; f <= H * 14 < 2^17, so score << 6 | nearness has 23 bits and ends[root] = f << 13 | (8191 - index)
//            has 30.
//   rank     (score, strand, p_lo, q_lo) no longer fits 64 bits. Within a strand the anchors are sorted by (p, j) and distinct, so the
//            sorted index of a chain's root orders (p_lo, q_lo): the rank key is (kSeedLongMaxScore - score) << 14 | strand << 13 | root
//            index, 31 bits, and (p_lo, q_lo) are fetched from the root's anchor when the round's winner is kept.
//
// LDS BANKS. As seed_chain.hpp: 64-bit entries, the upper 16 lanes of each half take their upper partner first below distance 32.
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

#ifdef AIM_TU_SEED_CHAIN_LONG   // the kernel lives in tu_seed_chain_long.hip alone; aim_capi.hip sees the arguments and the launcher

// seed_chain_sort (seed_chain.hpp) entry for entry.
__device__ __forceinline__ void seed_long_sort(uint64_t *key, uint32_t N, int lane)
{
    for (uint32_t k2 = 2; k2 <= N; k2 <<= 1) {
        for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
            for (uint32_t t = (uint32_t)lane; t < N / 2; t += kWave) {
                const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u));      // the lower partner
                const bool up = (i & k2) == 0;
                const bool hi_first = j < 32u && (t & 16u);
                const uint32_t a0 = hi_first ? (i | j) : i, a1 = a0 ^ j;
                const uint64_t x = key[a0], y = key[a1];
                const uint64_t lo_v = hi_first ? y : x, hi_v = hi_first ? x : y;
                if ((lo_v > hi_v) == up) {
                    key[a0] = y;
                    key[a1] = x;
                }
            }
            asm volatile("" ::: "memory");   // same-wave LDS traffic is ordered; compiler fence only
        }
    }
}

// The code of strand s's k-mer at query offset q, from the tile's bytes: trow[i] is the read's byte a0 + i. Forward for s = 0, backward
// with the complement folded in for s = 1 (seed_code's rule). *ok is cleared when it covers a byte other than upper-case A C G T.
__device__ __forceinline__ uint32_t seed_long_code(const uint8_t *trow, int32_t a0, int32_t L, int32_t q, int32_t k, int s, bool *ok)
{
    const uint8_t *f = trow + ((s ? L - 1 - q : q) - a0);
    uint32_t code = 0;
    for (int i = 0; i < k; ++i) {
        const uint32_t x = s ? f[-i] : f[i];
        *ok = *ok && seed_is_base(x);
        code |= (((x >> 1) & 3u) ^ (s ? 2u : 0u)) << (2 * i);
    }
    return code;
}

// The local selection for position j (active: j is one of the tile's own positions) over the tile's keys, tk[i] the key of position
// klo + i: L + R + 1 >= need = min(w, n), at most `reach` = w - 1 reads per side, none of which leaves [max(j - reach, 0), min(j + reach, n - 1)].
__device__ __forceinline__ bool seed_long_selected(const uint32_t *tk, uint32_t klo, uint32_t j, bool active, uint32_t n, uint32_t reach, uint32_t need,
                                                   uint32_t *mine_out)
{
    const uint32_t mine = active ? tk[j - klo] : kMinInvalid;
    bool left = mine != kMinInvalid, right = left;                          // the run on that side still extends
    uint32_t span = 1;                                                      // L + R + 1
    for (uint32_t d = 1; d <= reach; ++d) {
        if (!__ballot(left || right)) break;
        left = left && j >= d && tk[j - d - klo] > mine;
        right = right && j + d < n && tk[j + d - klo] >= mine;
        span += (uint32_t)left + (uint32_t)right;
    }
    *mine_out = mine;
    return mine != kMinInvalid && span >= need;
}

// seed_chain_append with the cap H and the anchor p << 16 | j. Returns the new count (wave-uniform; past H only "overflowed" matters).
__device__ __forceinline__ uint32_t seed_long_append(const SeedArgs &a, uint64_t *ks, uint32_t H, uint32_t count, uint32_t code, bool ok, uint32_t j, int lane)
{
    const uint32_t n_codes = 1u << (2 * a.sp.k), max_occ = (uint32_t)a.sp.max_occ;
    const uint64_t pos_cap = a.ref_len >= (uint64_t)a.sp.k ? a.ref_len - (uint64_t)a.sp.k + 1u : 0u;
    uint32_t b0 = 0, n = 0;
    if (ok && code < n_codes) {
        b0 = a.bucket[code];
        const uint32_t b1 = a.bucket[code + 1u];
        n = b1 - b0;
        if (b1 < b0 || n > max_occ || (uint64_t)b1 > pos_cap) n = 0;
        n = min(n, H + 1u);                          // the sums below stay far from 2^32
    }
    const uint32_t incl = seed_scan_add(n, lane);
    const uint32_t at = count + incl - n;
    for (uint32_t q = 0; q < n && at + q < H; ++q) ks[at + q] = ((uint64_t)a.pos[b0 + q] << 16) | j;
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
            const uint32_t code = seed_long_code(trow, a0, L, (int32_t)(klo + i), k, s, &ok);
            tk[i] = ok ? min_hash(code) : kMinInvalid;
        }
        asm volatile("" ::: "memory");
        for (uint32_t base = t0; base < t1 && count <= H; base += kWave) {   // select, hits (rules 2-3)
            const uint32_t j = base + (uint32_t)lane;
            uint32_t key;
            const bool selected = seed_long_selected(tk, klo, j, j < t1, n, reach, need, &key);
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

// seed_chain_strand with the widths of this kernel: the chain, rank and keep phases for strand s, whose `count` hits are in anchors[].
// The strand's best chains, at most K, go to the lanes lane0 .. lane0 + K - 1 of `mine`; returns their number (wave-uniform).
__device__ __forceinline__ uint32_t seed_long_strand(const SeedArgs &a, uint32_t H, uint64_t *anchors, uint32_t *ends, uint16_t *counts, uint32_t count, int s,
                                                     uint32_t lane0, ChainLongSlot &mine, int lane)
{
    const uint32_t k = (uint32_t)a.sp.k, band = (uint32_t)a.sp.band, K = (uint32_t)a.sp.max_cands, min_votes = (uint32_t)a.sp.min_votes;
    const uint32_t n = min(count, H);
    asm volatile("" ::: "memory");
    if (n > 1) {
        uint32_t N = kWave;
        while (N < n) N <<= 1;
        for (uint32_t i = n + (uint32_t)lane; i < N; i += kWave) anchors[i] = ULLONG_MAX;
        asm volatile("" ::: "memory");
        seed_long_sort(anchors, N, lane);
    }
    for (uint32_t i = (uint32_t)lane; i < n; i += kWave) ends[i] = 0;
    asm volatile("" ::: "memory");

    // chain: the ring. rf == 0 marks a lane that holds no anchor yet (f >= k >= 8 otherwise).
    uint32_t rp = 0, rf = 0, rroot = 0, rcnt = 0;
    int32_t rj = 0;
    for (uint32_t base = 0; base < n; base += kWave) {
        const uint32_t m = min((uint32_t)kWave, n - base);
        const uint64_t nk = (uint32_t)lane < m ? anchors[base + (uint32_t)lane] : 0;
        const uint32_t np = (uint32_t)(nk >> 16), nj = (uint32_t)nk & 0xFFFFu;
#ifdef AIM_SEED_CHAIN_AB_NO_DP   // A/B timing builds only (aim_amd/build.py --variant): every anchor stays a root, so what is left is hits, sort and rank
        for (uint32_t t = 0; t < 0; ++t) {
#else
        for (uint32_t t = 0; t < m; ++t) {
#endif
            const uint32_t pi = (uint32_t)__builtin_amdgcn_readlane((int)np, (int)t);
            const int32_t ji = __builtin_amdgcn_readlane((int)nj, (int)t);
            // admissible: dp > 0, dq > 0 and |dp - dq| <= band. The anchors are sorted, so dp >= 0 in uint32_t; band <= 4096 and
            // dq < 65536 bound an admissible dp by 69631, below which the difference is exact in 32 bits.
            const uint32_t dp = pi - rp;
            const int32_t dq = ji - rj;
            const int32_t d = (int32_t)dp - dq;
            const uint32_t g = (uint32_t)(d < 0 ? -d : d);
            const bool ok = rf != 0 && dp - 1u < 65536u + AIM_SEED_CHAIN_MAX_BAND - 1u && dq > 0 && g <= band;
            const int32_t gain = (int32_t)min(min(dp, (uint32_t)dq), k);
            const int32_t cost = (int32_t)(((g * k) >> 7) + ((32u - (uint32_t)__clz((int)g)) >> 1));   // (g = 0: 0)
            const int32_t sc = (int32_t)rf + gain - cost;
            const uint32_t nearness = ((uint32_t)lane - t) & 63u;      // lane t holds anchor i - 64, lane t - 1 anchor i - 1
            const int32_t key = ok && sc > (int32_t)k ? (sc << 6) | (int32_t)nearness : 0;
            uint32_t f = k, root = base + t, cnt = 1;
            if (__ballot(key != 0)) {                               // (wave-uniform)
                const int32_t best = INT_MAX - wave_min_i32(INT_MAX - key);
                const int src = (int)((t + ((uint32_t)best & 63u)) & 63u);
                f = (uint32_t)best >> 6;
                root = (uint32_t)__builtin_amdgcn_readlane((int)rroot, src);
                cnt = (uint32_t)__builtin_amdgcn_readlane((int)rcnt, src) + 1u;
            }
            if ((uint32_t)lane == t) {
                rp = pi;
                rj = ji;
                rf = f;
                rroot = root;
                rcnt = cnt;
            }
        }
        if ((uint32_t)lane < m) {     // the lanes hold the chunk's anchors
            const uint32_t i = base + (uint32_t)lane;
            atomicMax(&ends[rroot], (rf << 13) | (8191u - i));     // greatest f, the lowest index on a tie
            counts[i] = (uint16_t)rcnt;
        }
    }
    asm volatile("" ::: "memory");

    // rank: drop the chains below min_votes, then round i's winner stays in lane lane0 + i
    uint32_t n_chains = 0;
    for (uint32_t base = 0; base < n; base += kWave) {
        const uint32_t i = base + (uint32_t)lane;
        uint32_t e = i < n ? ends[i] : 0u;
        if (e && counts[8191u - (e & 8191u)] < min_votes) ends[i] = e = 0;
        n_chains += (uint32_t)__popcll(__ballot(e != 0));
    }
    asm volatile("" ::: "memory");
    const uint32_t rounds = min(K, n_chains);
    uint32_t last = 0;
    for (uint32_t round = 0; round < rounds; ++round) {
        uint32_t best = INT_MAX, best_end = 0;                      // (the keys have 31 bits and stay below INT_MAX: none)
        for (uint32_t i = (uint32_t)lane; i < n; i += kWave) {
            const uint32_t e = ends[i];
            if (!e) continue;
            const uint32_t key = ((kSeedLongMaxScore - (e >> 13)) << 14) | ((uint32_t)s << 13) | i;
            if ((round == 0 || key > last) && key < best) {
                best = key;
                best_end = 8191u - (e & 8191u);
            }
        }
        const uint32_t win = (uint32_t)wave_min_i32((int)best);
        // (rounds <= n_chains and the keys are unique: every round finds one)
        const int src = __ffsll((unsigned long long)__ballot(best == win)) - 1;
        const uint32_t end_at = (uint32_t)__builtin_amdgcn_readlane((int)best_end, src);
        if ((uint32_t)lane == lane0 + round) {
            mine.rank = win;
            mine.root = anchors[win & 8191u];
            mine.end = anchors[end_at];
            mine.n_anchors = counts[end_at];
        }
        last = win;
    }
    asm volatile("" ::: "memory");   // the next strand's hits land after these reads
    return rounds;
}

// seed_chain_fill for ChainLongSlot: the slots of read r from the chains the lanes hold (lanes 0..15 strand 0, 16..31 strand 1), and its
// aim_seed_t.
__device__ __forceinline__ void seed_long_fill(const SeedChainLongArgs &la, uint32_t r, int32_t L, const ChainLongSlot &mine, uint32_t n_kept,
                                               const uint32_t (&count)[2], int lane)
{
    const SeedArgs &a = la.c.s;
    const uint32_t K = (uint32_t)a.sp.max_cands, H = la.max_hits;
    const uint32_t n_cands = min(K, n_kept);
    uint32_t rank = 0;                 // kept chains with a smaller rank key
#pragma unroll
    for (int o = 0; o < 32; ++o) rank += (uint32_t)__builtin_amdgcn_readlane((int)mine.rank, o) < mine.rank ? 1u : 0u;
    const bool holds = lane < 32 && mine.rank != UINT_MAX && rank < K;
    const bool empty = lane >= 32 && lane < 48 && (uint32_t)(lane - 32) >= n_cands && (uint32_t)(lane - 32) < K;
    if (holds || empty) {
        const uint32_t slot = r * K + (holds ? rank : (uint32_t)(lane - 32));
        aim_request_t q;
        q.pattern_len = L;
        q.text_len = 0;
        q.padding = 0;
        q.idx = a.sp.idx_base + slot;
        uint64_t tp = 0;
        uint32_t votes = 0;
        aim_chain_t c = {};
        if (holds) {
            const int64_t k = a.sp.k;
            const uint32_t score = kSeedLongMaxScore - (mine.rank >> 14);
            const uint64_t strand = (mine.rank >> 13) & 1u;
            const int64_t p_lo = (int64_t)(mine.root >> 16), q_lo = (int64_t)(mine.root & 0xFFFFu);
            const int64_t p_hi = (int64_t)(mine.end >> 16) + k, q_hi = (int64_t)(mine.end & 0xFFFFu) + k;
            const int64_t lo = p_lo - q_lo - (int64_t)a.sp.flank;
            const int64_t hi = p_hi + ((int64_t)L - q_hi) + (int64_t)a.sp.flank;
            const int64_t start = max(lo, (int64_t)0);
            const int64_t end = max(start, min(hi, (int64_t)a.ref_len));
            q.text_len = (int32_t)min(end - start, (int64_t)a.sp.read_size);
            tp = (uint64_t)start | (strand << 63);
            votes = score;
            c.score = score;
            c.n_anchors = (uint16_t)mine.n_anchors;
            c.q_lo = (uint16_t)q_lo;
            c.q_hi = (uint16_t)q_hi;
            c.ref_span = (uint32_t)(p_hi - p_lo);
        }
        a.req[slot] = q;
        a.text_pos[slot] = tp;
        a.votes[slot] = votes;
        if (la.c.chains) la.c.chains[slot] = c;
    }
    if (lane == kWave - 1) {
        aim_seed_t sd;
        sd.n_cands = n_cands;
        sd.n_hits[0] = min(count[0], H);
        sd.n_hits[1] = min(count[1], H);
        sd.flags = (count[0] > H || count[1] > H) ? AIM_SEED_TRUNCATED : 0u;
        a.seed[r] = sd;
    }
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
