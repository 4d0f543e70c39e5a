// seed_chain.hpp -- colinear chaining of the seed hits (aim_hip.h, AIM_FEATURE_SEED_CHAIN): reads and a k-mer index in, the K best chains
// per read out as candidate windows, with each chain's read interval.
//
//   * seed_chain_kernel / seed_chain_minimizer_kernel: one read per 64-lane wavefront (a workgroup is one wavefront), persistent over
//     the reads through xcd_unit, with the seeds of seed_candidates_kernel / seed_minimizer_kernel. Staging, the k-mer codes, the
//     minimizer selection, the index lookup and the sort are seed.hpp's steps; the append keeps (p, j) instead of the diagonal.
//     Everything per read lives in LDS or registers; there is no scratch and no traffic between workgroups.
//
// SHARED STEPS. This header owns the one copy of the chain steps, under AIM_SEED_DEVICE_CODE, for its own kernels and for
// seed_chain_long_kernel (seed_chain_long.hpp): ChainWidths (the bit widths of an anchor and of an ends[] entry, compile-time, and the
// admissible-dp bound they give), seed_chain_dp (pad and sort, the lane-ring DP with its LDS-maximum epilogue, the min_votes filter)
// and seed_chain_write (the window, aim_request_t, aim_chain_t and aim_seed_t of the fill). A kernel keeps what its key widths decide:
// its append, its K rank rounds and the decoding of its rank key in the fill. AIM_TU_SEED_CHAIN only says which unit defines the
// __global__ kernels and the launcher.
//
// The rule is stated in full in aim_hip.h. The two strands run one after the other over the same LDS arrays:
//   hits     as in seed.hpp, 64 seeds per step; a hit is the 44-bit key p << 12 | j in a 64-bit LDS entry.
//   sort     seed_sort (seed.hpp) over 64-bit entries, padded with all ones.
//   chain    the DP, sequential over the sorted anchors. The lookback is the wavefront width: lane i % 64 owns anchor i's
//            (p, j, f, root, count) in registers, so at step i the 64 lanes hold exactly the predecessors i - 64 .. i - 1 (lane i % 64
//            still holds i - 64) and a step reads no LDS: anchor i's (p, j) is a v_readlane of the chunk the lanes loaded, every lane
//            scores its own predecessor, a DPP max-reduction (wave_min_i32's ladder) over score << 6 | nearness picks the link, and
//            two more v_readlane carry the root and the count along it. After each chunk of 64 steps the lanes hold that chunk's
//            anchors: each adds f << 10 | (1023 - index) to its root's entry of ends[] with an LDS maximum and stores its count.
//            No backtrack pass: ends[root] is the chain's score and end, count[end] its length.
//   rank     roots of chains below min_votes are cleared; K rounds of "smallest remaining rank key" as in seed_finish keep the
//            strand's best chains in lanes 0..15 (strand 0) and 16..31 (strand 1).
//   fill     a chain's slot is the number of kept chains with a smaller rank key (the keys are unique); the lane that holds it writes
//            the slot with plain vector stores, lanes 32..47 write the empty slots, lane 63 the aim_seed_t.
//
// LDS BANKS. The sort is seed_sort on 64-bit entries (seed.hpp, LDS BANKS). The chunk load and the rank passes read consecutive entries.
//
// OCCUPANCY. LDS per workgroup = 8 KB of anchors + 4 KB of ends + 2 KB of counts = 14 336 B, plus the row and 16 bytes, plus 4 B per
// read position of order keys for the minimizer kernel. In granules of 1 280 B and wavefronts per CU:
//     read_size    seed_chain_kernel         seed_chain_minimizer_kernel
//        128       14 480 B, 12, 10          14 992 B, 12, 10
//      1 024       15 376 B, 13,  9          19 472 B, 16,  8
//      4 096       18 448 B, 15,  8          34 832 B, 28,  4
// LDS-bound at 2-3 wavefronts per SIMD; kSeedChainMaxVgpr = 128 is the register budget of 4. No scratch.
#pragma once

#include "seed.hpp"

namespace aim {

constexpr int kSeedChainMaxVgpr = 128;                        // the bound tests/test_seed_chain_cpu.py checks in the code object
constexpr uint32_t kChainLookback = AIM_SEED_CHAIN_LOOKBACK;  // = kWave: the ring of the chain phase
constexpr uint32_t kChainAnchorBytes = kSeedHits * 8;         // anchors[1024], uint64_t
constexpr uint32_t kChainEndBytes = kSeedHits * 4;            // ends[1024], uint32_t
constexpr uint32_t kChainCountBytes = kSeedHits * 2;          // counts[1024], uint16_t
constexpr uint32_t kChainStateBytes = kChainAnchorBytes + kChainEndBytes + kChainCountBytes;
static_assert(kChainLookback == (uint32_t)kWave, "the ring holds one predecessor per lane");

struct SeedChainArgs {
    SeedArgs s;
    aim_chain_t *chains;     // may be NULL
};

// Dynamic LDS of one workgroup: anchors, ends, counts, the row and 16 bytes past it.
constexpr size_t seed_chain_lds_bytes(int32_t read_size) { return kChainStateBytes + (size_t)read_size + 16; }
// seed_chain_minimizer_kernel's: one more dword per read position, the strand's order keys
constexpr size_t seed_chain_minimizer_lds_bytes(int32_t read_size) { return seed_chain_lds_bytes(read_size) + 4u * (size_t)read_size; }

#ifdef AIM_SEED_DEVICE_CODE   // the chain steps seed_chain_long.hpp shares with the kernels below; one copy of each

// The widths of a chaining kernel's LDS entries: an anchor is p << JB | j, and ends[root] is f << EB | (kEndMask - index of the chain's
// end), so that an LDS maximum keeps the greatest f and, on a tie, the lowest index.
template <int JB, int EB>
struct ChainWidths {
    static constexpr int kJBits = JB, kEndBits = EB;
    static constexpr uint32_t kJMask = (1u << JB) - 1u, kEndMask = (1u << EB) - 1u;
    // admissible: dp > 0, dq > 0 and |dp - dq| <= band. dq < 2^JB and band <= AIM_SEED_CHAIN_MAX_BAND bound an admissible dp by this,
    // below which dp - dq is exact in 32 bits: 8 191 for seed_chain.hpp's kernels, 69 631 for seed_chain_long.hpp's.
    static constexpr uint32_t kMaxDp = (1u << JB) + AIM_SEED_CHAIN_MAX_BAND - 1u;
};
using ChainShort = ChainWidths<12, 10>;   // j < 4 096, kSeedHits = 1 024 anchors: the kernels below
using ChainLong = ChainWidths<16, 13>;    // j < 65 536, up to 8 192 anchors: seed_chain_long_kernel
static_assert(AIM_SEED_MAX_READ_SIZE <= (1 << ChainShort::kJBits) && kSeedHits == (1u << ChainShort::kEndBits), "ChainShort holds j and an anchor index");

// The sort and chain phases for one strand, whose `count` hits are in anchors[] (H: the hit cap), and the min_votes filter: afterwards
// ends[root] is non-zero exactly for the roots of the chains that are kept for ranking, counts[end] their length. Returns their number
// (wave-uniform).
template <typename W>
__device__ __forceinline__ uint32_t seed_chain_dp(const SeedArgs &a, uint32_t H, uint64_t *anchors, uint32_t *ends, uint16_t *counts, uint32_t count, int lane)
{
    const uint32_t k = (uint32_t)a.sp.k, band = (uint32_t)a.sp.band, min_votes = (uint32_t)a.sp.min_votes;
    const uint32_t n = min(count, H);
    asm volatile("" ::: "memory");
    if (n > 1) {
        uint32_t N = kWave;
        while (N < n) N <<= 1;
        for (uint32_t i = n + (uint32_t)lane; i < N; i += kWave) anchors[i] = ULLONG_MAX;
        asm volatile("" ::: "memory");
        seed_sort(anchors, N, lane);
    }
    for (uint32_t i = (uint32_t)lane; i < n; i += kWave) ends[i] = 0;
    asm volatile("" ::: "memory");

    // chain: the ring. rf == 0 marks a lane that holds no anchor yet (f >= k >= 8 otherwise).
    uint32_t rp = 0, rf = 0, rroot = 0, rcnt = 0;
    int32_t rj = 0;
    for (uint32_t base = 0; base < n; base += kWave) {
        const uint32_t m = min((uint32_t)kWave, n - base);
        const uint64_t nk = (uint32_t)lane < m ? anchors[base + (uint32_t)lane] : 0;
        const uint32_t np = (uint32_t)(nk >> W::kJBits), nj = (uint32_t)nk & W::kJMask;
#ifdef AIM_SEED_CHAIN_AB_NO_DP   // A/B timing builds only (aim_amd/build.py --variant): every anchor stays a root, so what is left is hits, sort and rank
        for (uint32_t t = 0; t < 0; ++t) {
#else
        for (uint32_t t = 0; t < m; ++t) {
#endif
            const uint32_t pi = (uint32_t)__builtin_amdgcn_readlane((int)np, (int)t);
            const int32_t ji = __builtin_amdgcn_readlane((int)nj, (int)t);
            // admissible (ChainWidths::kMaxDp). The anchors are sorted, so dp >= 0 in uint32_t.
            const uint32_t dp = pi - rp;
            const int32_t dq = ji - rj;
            const int32_t d = (int32_t)dp - dq;
            const uint32_t g = (uint32_t)(d < 0 ? -d : d);
            const bool ok = rf != 0 && dp - 1u < W::kMaxDp && dq > 0 && g <= band;
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
            atomicMax(&ends[rroot], (rf << W::kEndBits) | (W::kEndMask - i));     // greatest f, the lowest index on a tie
            counts[i] = (uint16_t)rcnt;
        }
    }
    asm volatile("" ::: "memory");

    // drop the chains below min_votes
    uint32_t n_chains = 0;
    for (uint32_t base = 0; base < n; base += kWave) {
        const uint32_t i = base + (uint32_t)lane;
        uint32_t e = i < n ? ends[i] : 0u;
        if (e && counts[W::kEndMask - (e & W::kEndMask)] < min_votes) ends[i] = e = 0;
        n_chains += (uint32_t)__popcll(__ballot(e != 0));
    }
    asm volatile("" ::: "memory");
    return n_chains;
}

// One kept chain as the fill writes it: the root anchor (p_lo, q_lo) and the end anchor (p_end, q_end), both k-mer starts.
struct ChainFound {
    uint32_t score, strand, n_anchors;
    int64_t p_lo, q_lo, p_end, q_end;
};

// Fill: the slots of read r and its aim_seed_t. A lane below 32 with `holds` writes slot `slot_at` from the chain `c` it holds, lanes
// 32..47 write the empty slots from n_cands on, all with plain vector stores; lane 63 writes the aim_seed_t. H: the hit cap.
__device__ __forceinline__ void seed_chain_write(const SeedChainArgs &ca, uint32_t H, uint32_t r, int32_t L, bool holds, uint32_t slot_at, const ChainFound &c,
                                                 uint32_t n_cands, const uint32_t (&count)[2], int lane)
{
    const SeedArgs &a = ca.s;
    const uint32_t K = (uint32_t)a.sp.max_cands;
    const bool empty = lane >= 32 && lane < 48 && (uint32_t)(lane - 32) >= n_cands && (uint32_t)(lane - 32) < K;
    if (holds || empty) {
        const uint32_t slot = r * K + (holds ? slot_at : (uint32_t)(lane - 32));
        aim_request_t q;
        q.pattern_len = L;
        q.text_len = 0;
        q.padding = 0;
        q.idx = a.sp.idx_base + slot;
        uint64_t tp = 0;
        uint32_t votes = 0;
        aim_chain_t ch = {};
        if (holds) {
            const int64_t k = a.sp.k;
            const int64_t p_hi = c.p_end + k, q_hi = c.q_end + k;
            const int64_t lo = c.p_lo - c.q_lo - (int64_t)a.sp.flank;
            const int64_t hi = p_hi + ((int64_t)L - q_hi) + (int64_t)a.sp.flank;
            const int64_t start = max(lo, (int64_t)0);
            const int64_t end = max(start, min(hi, (int64_t)a.ref_len));
            q.text_len = (int32_t)min(end - start, (int64_t)a.sp.read_size);
            tp = (uint64_t)start | ((uint64_t)c.strand << 63);
            votes = c.score;
            ch.score = c.score;
            ch.n_anchors = (uint16_t)c.n_anchors;
            ch.q_lo = (uint16_t)c.q_lo;
            ch.q_hi = (uint16_t)q_hi;
            ch.ref_span = (uint32_t)(p_hi - c.p_lo);
        }
        a.req[slot] = q;
        a.text_pos[slot] = tp;
        a.votes[slot] = votes;
        if (ca.chains) ca.chains[slot] = ch;
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

#endif

#ifdef AIM_TU_SEED_CHAIN   // the kernels live in tu_seed_chain.hip alone; capi_pipeline.hip sees SeedChainArgs and the launchers

// seed_append with the anchor p << 12 | j in place of the diagonal key.
__device__ __forceinline__ uint32_t seed_chain_append(const SeedArgs &a, uint64_t *ks, uint32_t count, uint32_t code, bool ok, int32_t j, int lane)
{
    uint32_t b0;
    const uint32_t n = seed_run(a, kSeedHits, code, ok, &b0);
    const uint32_t incl = seed_scan_add(n, lane);
    const uint32_t at = count + incl - n;
    for (uint32_t q = 0; q < n && at + q < kSeedHits; ++q) ks[at + q] = ((uint64_t)a.pos[b0 + q] << ChainShort::kJBits) | (uint32_t)j;
    return count + (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
}

// One kept chain, in the lane that holds it. rank = (16383 - score) << 45 | strand << 44 | p_lo << 12 | q_lo; all ones: none.
struct ChainSlot {
    uint64_t rank, end;      // end: the end anchor, p << 12 | j
    uint32_t n_anchors;
};

// The sort, chain, rank and keep phases for strand s, whose `count` hits are in anchors[]. The strand's best chains, at most K, go to
// the lanes lane0 .. lane0 + K - 1 of `mine`; returns their number (wave-uniform).
__device__ __forceinline__ uint32_t seed_chain_strand(const SeedArgs &a, uint64_t *anchors, uint32_t *ends, uint16_t *counts, uint32_t count, int s,
                                                      uint32_t lane0, ChainSlot &mine, int lane)
{
    const uint32_t n = min(count, kSeedHits);
    const uint32_t rounds = min((uint32_t)a.sp.max_cands, seed_chain_dp<ChainShort>(a, kSeedHits, anchors, ends, counts, count, lane));
    // rank: round i's winner stays in lane lane0 + i
    uint64_t last = 0;
    for (uint32_t round = 0; round < rounds; ++round) {
        uint64_t best = ULLONG_MAX;
        uint32_t best_end = 0;
        for (uint32_t i = (uint32_t)lane; i < n; i += kWave) {
            const uint32_t e = ends[i];
            if (!e) continue;
            const uint64_t key = ((uint64_t)(16383u - (e >> ChainShort::kEndBits)) << 45) | ((uint64_t)s << 44) | anchors[i];
            if ((round == 0 || key > last) && key < best) {
                best = key;
                best_end = ChainShort::kEndMask - (e & ChainShort::kEndMask);
            }
        }
        const uint64_t win = seed_min_u64(best);
        // (rounds <= the number of chains and the keys are unique: every round finds one)
        const int src = __ffsll((unsigned long long)__ballot(best == win)) - 1;
        const uint32_t end_at = (uint32_t)__builtin_amdgcn_readlane((int)best_end, src);
        if ((uint32_t)lane == lane0 + round) {
            mine.rank = win;
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
__device__ __forceinline__ void seed_chain_fill(const SeedChainArgs &ca, uint32_t r, int32_t L, const ChainSlot &mine, uint32_t n_kept,
                                                const uint32_t (&count)[2], int lane)
{
    const uint32_t K = (uint32_t)ca.s.sp.max_cands;
    uint32_t rank = 0;
    const uint32_t lo32 = (uint32_t)mine.rank, hi32 = (uint32_t)(mine.rank >> 32);
#pragma unroll
    for (int o = 0; o < 32; ++o) {
        const uint64_t other = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)hi32, o) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)lo32, o);
        rank += other < mine.rank ? 1u : 0u;
    }
    ChainFound c;
    c.score = 16383u - (uint32_t)(mine.rank >> 45);
    c.strand = (uint32_t)(mine.rank >> 44) & 1u;
    c.n_anchors = mine.n_anchors;
    c.p_lo = (int64_t)((mine.rank >> ChainShort::kJBits) & 0xFFFFFFFFull);
    c.q_lo = (int64_t)(mine.rank & ChainShort::kJMask);
    c.p_end = (int64_t)(mine.end >> ChainShort::kJBits);
    c.q_end = (int64_t)(mine.end & ChainShort::kJMask);
    seed_chain_write(ca, kSeedHits, r, L, lane < 32 && mine.rank != ULLONG_MAX && rank < K, rank, c, min(K, n_kept), count, lane);
}

// The kernel body; MINIMIZERS selects rule 2 (the stride of seed_candidates_kernel, or the (w, k) minimizers of seed_minimizer_kernel).
template <bool MINIMIZERS>
__device__ __forceinline__ void seed_chain_reads(const SeedChainArgs &ca)
{
    extern __shared__ __align__(16) char seed_chain_smem[];
    const SeedArgs &a = ca.s;
    debug_poison_lds(a.dbg_poison_lds, a.dbg_lds_bytes, seed_chain_smem);
    const int lane = threadIdx.x;
    const int32_t k = a.sp.k, stride = a.sp.stride, rs = a.sp.read_size;
    uint64_t *anchors = reinterpret_cast<uint64_t *>(seed_chain_smem);                                       // [kSeedHits]
    uint32_t *ends = reinterpret_cast<uint32_t *>(seed_chain_smem + kChainAnchorBytes);                      // [kSeedHits]
    uint16_t *counts = reinterpret_cast<uint16_t *>(seed_chain_smem + kChainAnchorBytes + kChainEndBytes);   // [kSeedHits]
    uint32_t *row4 = reinterpret_cast<uint32_t *>(seed_chain_smem + kChainStateBytes);
    const uint8_t *row = reinterpret_cast<const uint8_t *>(row4);
    uint32_t *hk = reinterpret_cast<uint32_t *>(seed_chain_smem + seed_chain_lds_bytes(rs));                 // [rs], MINIMIZERS only
    const uint32_t reach = min(a.sp.options >> 8, (uint32_t)AIM_SEED_MAX_W) - 1u;                            // (MINIMIZERS: w >= 1 is checked)

    for (uint32_t it = 0;; ++it) {
        uint32_t r;
        if (!xcd_unit(a.n_reads, it, &r)) break;
        const int32_t L = min(max(a.read_len[r], 0), rs);
        asm volatile("" ::: "memory");   // the previous read's LDS reads are issued before this row lands
        seed_stage(a, row4, r, L, lane);
        asm volatile("" ::: "memory");

        uint32_t count[2] = {0u, 0u};
        uint32_t n_kept = 0;
        ChainSlot mine = {ULLONG_MAX, 0, 0};
#pragma unroll 1
        for (int s = 0; s < 2; ++s) {
            if (MINIMIZERS) {
                const uint32_t n = L >= k ? (uint32_t)(L - k) + 1u : 0u;
                const uint32_t need = min(reach + 1u, n);                                       // min(w, n)
                for (uint32_t j = (uint32_t)lane; j < n; j += kWave) {   // keys
                    bool ok = true;
                    const uint32_t code = seed_code(row, L, (int32_t)j, k, s, &ok);
                    hk[j] = ok ? min_hash(code) : kMinInvalid;
                }
                asm volatile("" ::: "memory");
                for (uint32_t base = 0; base < n && count[s] <= kSeedHits; base += kWave) {   // select, hits (rules 2-3)
                    const uint32_t j = base + (uint32_t)lane;
                    uint32_t key;
                    const bool selected = seed_minimizer_selected(hk, 0u, j, j < n, n, reach, need, &key);
                    count[s] = seed_chain_append(a, anchors, count[s], min_unhash(key), selected, (int32_t)j, lane);
                }
            } else {
                const uint32_t n_seeds = L >= k ? (uint32_t)(L - k) / (uint32_t)stride + 1u : 0u;
                for (uint32_t base = 0; base < n_seeds && count[s] <= kSeedHits; base += kWave) {   // hits (rules 2-3)
                    const uint32_t m = base + (uint32_t)lane;
                    bool ok = m < n_seeds;
                    const int32_t j = ok ? (int32_t)m * stride : 0;
                    const uint32_t code = ok ? seed_code(row, L, j, k, s, &ok) : 0u;
                    count[s] = seed_chain_append(a, anchors, count[s], code, ok, j, lane);
                }
            }
            n_kept += seed_chain_strand(a, anchors, ends, counts, count[s], s, s ? 16u : 0u, mine, lane);
        }
        seed_chain_fill(ca, r, L, mine, n_kept, count, lane);
    }
}

__global__ __launch_bounds__(64) void seed_chain_kernel(SeedChainArgs a) { seed_chain_reads<false>(a); }
__global__ __launch_bounds__(64) void seed_chain_minimizer_kernel(SeedChainArgs a) { seed_chain_reads<true>(a); }

void seed_chain_launch(const SeedChainArgs &a, bool minimizers, uint32_t grid, size_t lds, hipStream_t s)
{
    if (minimizers)
        hipLaunchKernelGGL(seed_chain_minimizer_kernel, dim3(grid), dim3(kWave), lds, s, a);
    else
        hipLaunchKernelGGL(seed_chain_kernel, dim3(grid), dim3(kWave), lds, s, a);
}
#else
void seed_chain_launch(const SeedChainArgs &a, bool minimizers, uint32_t grid, size_t lds, hipStream_t s);
#endif

}  // namespace aim
