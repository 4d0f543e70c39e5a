// seed.hpp -- device-side seeding (aim_hip.h, AIM_FEATURE_SEED): reads and a k-mer index in, K candidate windows per read out.
//
//   * seed_candidates_kernel: one read per 64-lane wavefront (a workgroup is one wavefront), persistent over the reads through
//     xcd_unit like the per-pair kernels. Everything per read lives in LDS; there is no scratch and no traffic between workgroups.
//
//   * seed_minimizer_kernel: the same with the (w, k) minimizers of each strand's query as its seeds (AIM_SEED_OPT_MINIMIZERS). It
//     shares seed_append (lookup and append) and seed_finish (sort, cluster, rank, fill) with the kernel above and is described where
//     it stands: one more LDS array, 4 B per read position, for the strand's order keys.
//
// SHARED STEPS. This header owns the one copy of every step the five seed kernels have in common (these two, seed_chain.hpp's two and
// seed_chain_long.hpp's one), under AIM_SEED_DEVICE_CODE, which tu_seed.hip, tu_seed_chain.hip and tu_seed_chain_long.hip define:
// seed_stage (the row into LDS), seed_code (a strand's k-mer code), seed_minimizer_selected (the local (w, k) selection), seed_run (the
// index lookup with its bounds checks, the only reader of bucket[]), seed_sort (the bitonic network, on 32- or 64-bit keys) and the wave
// scans. An append is seed_run, a prefix sum and a store loop around the kernel's own key: seed_append here, seed_chain_append and
// seed_long_append in the chaining headers. Two kernels keep seed_code's rule in place, everything else calls the steps:
// seed_candidates_kernel codes both strands of a seed in one fused loop (with two seed_code calls its code object leaves the recorded
// register counts, 98 SGPRs become 97), and seed_minimizer_kernel keeps its loop inline (through the function the compiler lays the
// select loop's blocks out differently and the kernel measured 2 % slower; profiles/seed_shared/README.md).
// AIM_TU_SEED only says which unit defines the __global__ kernels and launchers below.
//
// The rule is stated in full in aim_hip.h; the phases below follow its numbering.
//   stage    the read row, once, into LDS (dwords).
//   hits     lanes take seeds, 64 per step. The strand-0 code is read forward from the row and the strand-1 code backward from the same
//            bytes with the complement folded in (code ^ 2). Two bucket reads give a seed's run of positions; a wave prefix sum of the run
//            lengths gives every lane its append position, which makes the (j, p) order of rule 3 exact.
//   sort     an in-wave bitonic network over each strand's keys in LDS, padded with 0xFFFFFFFF (no key reaches it: ref_len <= 2^32 - 2^25).
//   cluster  boundary flags from the neighbours and a segmented max-scan of the head positions; a cluster's votes are stored at its tail
//            (0 elsewhere and below min_votes), so a_hi is the key there and a_lo the key `votes - 1` entries before it.
//   rank     K rounds of "smallest remaining rank key" in the pattern of hit_select_kernel: the key (1024 - votes, strand, a_lo) is
//            unique per cluster, round i keeps its winner in lane i, and lanes 0..K-1 then write their slots, empty ones included.
//
// LDS BANKS. ds_read_b32 / ds_write_b32 bank on (address / 4) % 32 within each 32-lane half. A compare-exchange stage at distance
// j >= 32 touches consecutive dwords per half: conflict-free. At j < 32 the 32 lower partners of a half all have bit log2(j) clear and
// would fall two to a bank; there the upper 16 lanes of each half read their UPPER partner first (address | j), so a half covers 32
// distinct residues in each of its two reads and writes. The cluster and rank passes read consecutive entries. The chaining kernels sort
// 64-bit entries with the same network: ds_read_b64 / ds_write_b64 bank on the entry index modulo 32 within each 32-lane half, so the
// reasoning holds entry for entry.
//
// OCCUPANCY. LDS per workgroup = 8 KB of keys + 4 KB of votes + the row: 12 432 B at read_size 128, ten 1 280-B granules, so 12
// wavefronts per CU = 3 per SIMD, LDS-bound. The register budget that keeps it so is 512 / 3 = 170; kSeedMaxVgpr = 128 leaves room for
// a fourth wavefront should the LDS shrink. No scratch.
#pragma once

#include <climits>

#include "aim_device.hpp"
#include "minimizer.hpp"

namespace aim {

constexpr int kSeedMaxVgpr = 128;                          // the bound tests/test_seed_cpu.py checks in the code object
constexpr int kSeedMinimizerMaxVgpr = 128;                 // seed_minimizer_kernel's (tests/test_minimizers_cpu.py)
constexpr uint32_t kSeedHits = AIM_SEED_MAX_HITS;          // keys per strand
constexpr uint32_t kSeedKeyBytes = 2 * kSeedHits * 4;      // keys[2][1024]
constexpr uint32_t kSeedVoteBytes = 2 * kSeedHits * 2;     // vt[2][1024], uint16_t

struct SeedArgs {
    aim_seed_params_t sp;
    uint32_t n_reads;
    const int32_t *read_len;
    const char *reads;
    const uint32_t *bucket, *pos;
    uint64_t ref_len;
    aim_request_t *req;
    uint64_t *text_pos;
    uint32_t *votes;
    aim_seed_t *seed;
    uint32_t dbg_poison_lds, dbg_lds_bytes;   // as in KArgs (AIM_DEBUG_POISON_LDS)
};

// Dynamic LDS of one workgroup: keys, votes, the row and 16 bytes past it.
constexpr size_t seed_lds_bytes(int32_t read_size) { return kSeedKeyBytes + kSeedVoteBytes + (size_t)read_size + 16; }
// seed_minimizer_kernel's: one more dword per read position, the strand's order keys
constexpr size_t seed_minimizer_lds_bytes(int32_t read_size) { return seed_lds_bytes(read_size) + 4u * (size_t)read_size; }

#ifdef AIM_SEED_DEVICE_CODE   // device code: the three tu_seed*.hip define it. The steps below are the only copy of each, for all five seed kernels

__device__ __forceinline__ uint32_t seed_scan_add(uint32_t v, int lane)   // inclusive wave prefix sum
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, kWave);
        if (lane >= d) v += o;
    }
    return v;
}

__device__ __forceinline__ uint32_t seed_scan_max(uint32_t v, int lane)   // inclusive wave prefix maximum
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, kWave);
        if (lane >= d) v = max(v, o);
    }
    return v;
}

__device__ __forceinline__ bool seed_is_base(uint32_t c)   // upper-case A C G T
{
    const uint32_t d = c - 65u;
    return d < 20u && ((0x80045u >> d) & 1u);
}

// Ascending bitonic sort of key[0, N), N a power of two >= 64, by one wavefront; Key is uint32_t or uint64_t (see LDS BANKS above).
template <typename Key>
__device__ __forceinline__ void seed_sort(Key *key, uint32_t N, int lane)
{
    for (uint32_t k2 = 2; k2 <= N; k2 <<= 1) {
        for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
            for (uint32_t t = (uint32_t)lane; t < N / 2; t += kWave) {
                const uint32_t i = ((t & ~(j - 1u)) << 1) | (t & (j - 1u));      // the lower partner
                const bool up = (i & k2) == 0;
                const bool hi_first = j < 32u && (t & 16u);
                const uint32_t a0 = hi_first ? (i | j) : i, a1 = a0 ^ j;
                const Key x = key[a0], y = key[a1];
                const Key lo_v = hi_first ? y : x, hi_v = hi_first ? x : y;
                if ((lo_v > hi_v) == up) {
                    key[a0] = y;
                    key[a1] = x;
                }
            }
            asm volatile("" ::: "memory");   // same-wave LDS traffic is ordered; compiler fence only
        }
    }
}

__device__ __forceinline__ uint64_t seed_min_u64(uint64_t v)   // wave-wide minimum, in every lane
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t lo = __shfl_xor((uint32_t)v, d, kWave), hi = __shfl_xor((uint32_t)(v >> 32), d, kWave);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o < v ? o : v;
    }
    return v;
}

// stage: the read row r, once, into LDS (dwords)
__device__ __forceinline__ void seed_stage(const SeedArgs &a, uint32_t *row4, uint32_t r, int32_t L, int lane)
{
    const uint32_t *g = reinterpret_cast<const uint32_t *>(a.reads + (uint64_t)r * (uint64_t)a.sp.read_size);
    for (int w = lane; w < (L + 3) >> 2; w += kWave) row4[w] = g[w];
}

// The code of strand s's k-mer at query offset j: read forward from the row (s = 0), or backward from the same bytes with the complement
// folded in (s = 1). row[i] is the read's byte i: a kernel that holds only the bytes from a0 on passes its buffer moved back by a0.
// *ok is cleared when the k-mer covers a byte other than upper-case A C G T.
__device__ __forceinline__ uint32_t seed_code(const uint8_t *row, int32_t L, int32_t j, int32_t k, int s, bool *ok)
{
    const uint8_t *f = s ? row + (L - 1 - j) : row + j;
    uint32_t code = 0;
    for (int i = 0; i < k; ++i) {
        const uint32_t x = s ? f[-i] : f[i];
        *ok = *ok && seed_is_base(x);
        code |= (((x >> 1) & 3u) ^ (s ? 2u : 0u)) << (2 * i);
    }
    return code;
}

// The local minimizer selection for position j of a strand's n order keys, hk[i] the key of position klo + i: L + R + 1 >= need =
// min(w, n), at most `reach` = w - 1 reads per side, none of which leaves [max(j - reach, 0), min(j + reach, n - 1)]. !active: the lane
// has no position. *mine_out receives j's key (kMinInvalid for !active).
__device__ __forceinline__ bool seed_minimizer_selected(const uint32_t *hk, uint32_t klo, uint32_t j, bool active, uint32_t n, uint32_t reach, uint32_t need,
                                                        uint32_t *mine_out)
{
    const uint32_t mine = active ? hk[j - klo] : kMinInvalid;
    bool left = mine != kMinInvalid, right = left;                          // the run on that side still extends
    uint32_t span = 1;                                                      // L + R + 1
    for (uint32_t d = 1; d <= reach; ++d) {
        if (!__ballot(left || right)) break;
        left = left && j >= d && hk[j - d - klo] > mine;
        right = right && j + d < n && hk[j + d - klo] >= mine;
        span += (uint32_t)left + (uint32_t)right;
    }
    *mine_out = mine;
    return mine != kMinInvalid && span >= need;
}

// The index lookup, and the only reader of bucket[]: the run pos[*b0, *b0 + n) of the lane's seed; n = 0 for no seed, an absent or
// over-frequent code and index entries that point outside the arrays. `cap` is the strand's hit cap.
__device__ __forceinline__ uint32_t seed_run(const SeedArgs &a, uint32_t cap, uint32_t code, bool ok, uint32_t *b0)
{
    const uint32_t n_codes = 1u << (2 * a.sp.k), max_occ = (uint32_t)a.sp.max_occ;
    const uint64_t pos_cap = a.ref_len >= (uint64_t)a.sp.k ? a.ref_len - (uint64_t)a.sp.k + 1u : 0u;
    uint32_t n = 0;
    *b0 = 0;
    if (ok && code < n_codes) {
        *b0 = a.bucket[code];
        const uint32_t b1 = a.bucket[code + 1u];
        n = b1 - *b0;
        if (b1 < *b0 || n > max_occ || (uint64_t)b1 > pos_cap) n = 0;
        n = min(n, cap + 1u);                        // past the cap only "overflowed" matters: the sums below stay far from 2^32
    }
    return n;
}

// Rules 2-3 for the 64 seeds of one step and one strand: the lane's seed (code `code` at query offset j; !ok: no seed) looks its run of
// positions up, and a wave prefix sum of the run lengths gives every lane its append position behind the `count` hits found so far.
// Returns the new count (wave-uniform; it stops meaning anything exact once it has passed the cap). This is the append of the voting
// kernels, whose key is the hit's diagonal p - j + read_size; seed_chain_append (seed_chain.hpp) is the same around another key.
__device__ __forceinline__ uint32_t seed_append(const SeedArgs &a, uint32_t *ks, uint32_t count, uint32_t code, bool ok, int32_t j, int lane)
{
    uint32_t b0;
    const uint32_t n = seed_run(a, kSeedHits, code, ok, &b0);
    const uint32_t incl = seed_scan_add(n, lane);
    const uint32_t at = count + incl - n;
    const uint32_t bias = (uint32_t)a.sp.read_size - (uint32_t)j;
    for (uint32_t q = 0; q < n && at + q < kSeedHits; ++q) ks[at + q] = a.pos[b0 + q] + bias;
    return count + (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
}

// Rules 3-7 for one read whose hits are in keys[2][kSeedHits]: sort, cluster, rank, and the read's slots and aim_seed_t.
__device__ __forceinline__ void seed_finish(const SeedArgs &a, uint32_t *keys, uint16_t *vt, uint32_t r, int32_t L, const uint32_t (&count)[2], int lane)
{
    const int32_t rs = a.sp.read_size;
    const uint32_t K = (uint32_t)a.sp.max_cands, band = (uint32_t)a.sp.band, min_votes = (uint32_t)a.sp.min_votes;
    const uint32_t nh[2] = {min(count[0], kSeedHits), min(count[1], kSeedHits)};
    const uint32_t sflags = (count[0] > kSeedHits || count[1] > kSeedHits) ? AIM_SEED_TRUNCATED : 0u;
    asm volatile("" ::: "memory");

    // sort and cluster (rule 4)
    uint32_t n_clusters = 0;         // clusters with votes >= min_votes, both strands (wave-uniform)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        const uint32_t n = nh[s];
        uint32_t *ks = keys + s * kSeedHits;
        uint16_t *vs = vt + s * kSeedHits;
        if (n > 1) {
            uint32_t N = kWave;
            while (N < n) N <<= 1;
            for (uint32_t i = n + (uint32_t)lane; i < N; i += kWave) ks[i] = UINT_MAX;
            asm volatile("" ::: "memory");
            seed_sort(ks, N, lane);
        }
        uint32_t carry = 0;          // head position of the run that reaches into this chunk
        for (uint32_t base = 0; base < n; base += kWave) {
            const uint32_t i = base + (uint32_t)lane;
            const bool active = i < n;
            uint32_t head_at = 0, votes = 0;
            bool tail = false;
            if (active) {
                const uint32_t cur = ks[i];
                const bool head = i == 0 || cur - ks[i - 1] > band;
                tail = i + 1 == n || ks[i + 1] - cur > band;
                head_at = head ? i : 0u;
            }
            head_at = max(seed_scan_max(head_at, lane), carry);
            carry = (uint32_t)__builtin_amdgcn_readlane((int)head_at, kWave - 1);
            if (tail) votes = i - head_at + 1u;
            if (votes < min_votes) votes = 0;
            if (active) vs[i] = (uint16_t)votes;
            n_clusters += (uint32_t)__popcll(__ballot(votes != 0));
        }
    }
    asm volatile("" ::: "memory");

    // rank (rule 5): round i's winner stays in lane i
    uint32_t my_lo = 0, my_hi = 0, my_votes = 0, my_s = 0;
    uint32_t n_cands = 0;
    uint64_t last = 0;
    const uint32_t rounds = min(K, n_clusters);
    for (uint32_t round = 0; round < rounds; ++round) {
        uint64_t best = ULLONG_MAX;
        uint32_t best_hi = 0;
#pragma unroll
        for (int s = 0; s < 2; ++s) {
            const uint32_t *ks = keys + s * kSeedHits;
            const uint16_t *vs = vt + s * kSeedHits;
            for (uint32_t i = (uint32_t)lane; i < nh[s]; i += kWave) {
                const uint32_t v = vs[i];
                if (!v) continue;
                const uint64_t key = ((uint64_t)(kSeedHits - v) << 33) | ((uint64_t)s << 32) | ks[i - v + 1u];
                if ((round == 0 || key > last) && key < best) {
                    best = key;
                    best_hi = ks[i];
                }
            }
        }
        const uint64_t win = seed_min_u64(best);
        // (rounds <= n_clusters and the keys are unique: every round finds one)
        const int src = __ffsll((unsigned long long)__ballot(best == win)) - 1;
        const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)best_hi, src);
        if ((uint32_t)lane == round) {
            my_lo = (uint32_t)win;
            my_hi = hi;
            my_votes = kSeedHits - (uint32_t)(win >> 33);
            my_s = (uint32_t)(win >> 32) & 1u;
        }
        last = win;
        ++n_cands;
    }

    // fill (rules 6-7): lanes 0..K-1 write their slots
    if ((uint32_t)lane < K) {
        const uint32_t slot = r * K + (uint32_t)lane;
        aim_request_t q;
        q.pattern_len = L;
        q.text_len = 0;
        q.padding = 0;
        q.idx = a.sp.idx_base + slot;
        uint64_t tp = 0;
        uint32_t votes = 0;
        if ((uint32_t)lane < n_cands) {
            const int64_t lo = (int64_t)my_lo - (int64_t)rs - (int64_t)a.sp.flank;
            const int64_t hi = lo + (int64_t)L + 2 * (int64_t)a.sp.flank + (int64_t)min(my_hi - my_lo, (uint32_t)rs);
            const int64_t start = max(lo, (int64_t)0);
            const int64_t end = max(start, min(hi, (int64_t)a.ref_len));
            q.text_len = (int32_t)min(end - start, (int64_t)rs);
            tp = (uint64_t)start | ((uint64_t)my_s << 63);
            votes = my_votes;
        }
        a.req[slot] = q;
        a.text_pos[slot] = tp;
        a.votes[slot] = votes;
    }
    if (lane == 0) {
        aim_seed_t sd;
        sd.n_cands = n_cands;
        sd.n_hits[0] = nh[0];
        sd.n_hits[1] = nh[1];
        sd.flags = sflags;
        a.seed[r] = sd;
    }
}

#endif

#ifdef AIM_TU_SEED   // the kernels live in tu_seed.hip alone; capi_pipeline.hip sees SeedArgs and the launchers

__global__ __launch_bounds__(64) void seed_candidates_kernel(SeedArgs a)
{
    extern __shared__ __align__(16) char seed_smem[];
    debug_poison_lds(a.dbg_poison_lds, a.dbg_lds_bytes, seed_smem);
    const int lane = threadIdx.x;
    uint32_t *keys = reinterpret_cast<uint32_t *>(seed_smem);                          // [2][kSeedHits]
    uint16_t *vt = reinterpret_cast<uint16_t *>(seed_smem + kSeedKeyBytes);            // [2][kSeedHits]
    uint32_t *row4 = reinterpret_cast<uint32_t *>(seed_smem + kSeedKeyBytes + kSeedVoteBytes);
    const uint8_t *row = reinterpret_cast<const uint8_t *>(row4);
    const int32_t k = a.sp.k, stride = a.sp.stride, rs = a.sp.read_size;

    for (uint32_t it = 0;; ++it) {
        uint32_t r;
        if (!xcd_unit(a.n_reads, it, &r)) break;
        const int32_t L = min(max(a.read_len[r], 0), rs);
        asm volatile("" ::: "memory");   // the previous read's LDS reads are issued before this row lands
        seed_stage(a, row4, r, L, lane);
        asm volatile("" ::: "memory");

        // hits (rules 1-3)
        const uint32_t n_seeds = L >= k ? (uint32_t)(L - k) / (uint32_t)stride + 1u : 0u;
        uint32_t count[2] = {0u, 0u};    // hits found so far, wave-uniform; counting stops once it has passed kSeedHits
        for (uint32_t base = 0; base < n_seeds; base += kWave) {
            if (count[0] > kSeedHits && count[1] > kSeedHits) break;
            const uint32_t m = base + (uint32_t)lane;
            const bool active = m < n_seeds;
            const int32_t j = active ? (int32_t)m * stride : 0;
            uint32_t c0 = 0, c1 = 0;           // seed_code's rule for both strands at once (see SHARED STEPS)
            bool ok0 = active, ok1 = active;
            if (active) {
                const uint8_t *f = row + j, *b = row + (L - 1 - j);
                for (int i = 0; i < k; ++i) {
                    const uint32_t x = f[i], y = b[-i];
                    ok0 = ok0 && seed_is_base(x);
                    ok1 = ok1 && seed_is_base(y);
                    c0 |= ((x >> 1) & 3u) << (2 * i);
                    c1 |= (((y >> 1) & 3u) ^ 2u) << (2 * i);
                }
            }
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                if (count[s] > kSeedHits) continue;              // (wave-uniform)
                count[s] = seed_append(a, keys + s * kSeedHits, count[s], s ? c1 : c0, s ? ok1 : ok0, j, lane);
            }
        }
        seed_finish(a, keys, vt, r, L, count, lane);
    }
}

// The minimizer seeder (aim_hip.h, AIM_SEED_OPT_MINIMIZERS): seed_candidates_kernel with rule 2 replaced -- a strand's seeds are the
// (w, k) minimizers of its query -- and everything from the append on shared with it. Per strand:
//   keys    hk[j] = min_hash(code) of the query's k-mer at j, kMinInvalid where it is invalid (minimizer.hpp), for all n = L - k + 1
//           positions: the strand-1 query is read backward from the same row with the complement folded in, as above.
//   select  64 positions per step; the local test of index_minimizer_kernel (L + R + 1 >= min(w, n)) on hk, at most w - 1 reads per side
//           of consecutive dwords over the lanes (conflict-free). A lane that is not selected appends n = 0 hits, so the (j, p) order
//           of rule 3 is exact.
// LDS per workgroup = seed_lds_bytes + 4 * read_size for hk: 12 944 B at read_size 128 (11 granules of 1 280 B: 11 wavefronts per CU)
// and 32 784 B at 4 096 (26 granules: 4 per CU, one per SIMD). No scratch; kSeedMinimizerMaxVgpr as kSeedMaxVgpr.
__global__ __launch_bounds__(64) void seed_minimizer_kernel(SeedArgs a)
{
    extern __shared__ __align__(16) char seed_smem[];
    debug_poison_lds(a.dbg_poison_lds, a.dbg_lds_bytes, seed_smem);
    const int lane = threadIdx.x;
    const int32_t k = a.sp.k, rs = a.sp.read_size;
    uint32_t *keys = reinterpret_cast<uint32_t *>(seed_smem);                          // [2][kSeedHits]
    uint16_t *vt = reinterpret_cast<uint16_t *>(seed_smem + kSeedKeyBytes);            // [2][kSeedHits]
    uint32_t *row4 = reinterpret_cast<uint32_t *>(seed_smem + kSeedKeyBytes + kSeedVoteBytes);
    const uint8_t *row = reinterpret_cast<const uint8_t *>(row4);
    uint32_t *hk = reinterpret_cast<uint32_t *>(seed_smem + seed_lds_bytes(rs));       // [rs] (read_size is a multiple of 8)
    const uint32_t reach = min(a.sp.options >> 8, (uint32_t)AIM_SEED_MAX_W) - 1u;      // neighbours looked at on each side (w >= 1 is checked)

    for (uint32_t it = 0;; ++it) {
        uint32_t r;
        if (!xcd_unit(a.n_reads, it, &r)) break;
        const int32_t L = min(max(a.read_len[r], 0), rs);
        asm volatile("" ::: "memory");   // the previous read's LDS reads are issued before this row lands
        seed_stage(a, row4, r, L, lane);
        asm volatile("" ::: "memory");

        const uint32_t n = L >= k ? (uint32_t)(L - k) + 1u : 0u;
        const uint32_t need = min(reach + 1u, n);                                       // min(w, n)
        uint32_t count[2] = {0u, 0u};
#pragma unroll 1
        for (int s = 0; s < 2; ++s) {
            for (uint32_t j = (uint32_t)lane; j < n; j += kWave) {   // keys
                const uint8_t *f = s ? row + (L - 1 - (int32_t)j) : row + j;   // seed_code's rule, in place (see SHARED STEPS)
                uint32_t code = 0;
                bool ok = true;
                for (int i = 0; i < k; ++i) {
                    const uint32_t x = s ? f[-i] : f[i];
                    ok = ok && seed_is_base(x);
                    code |= (((x >> 1) & 3u) ^ (s ? 2u : 0u)) << (2 * i);
                }
                hk[j] = ok ? min_hash(code) : kMinInvalid;
            }
            asm volatile("" ::: "memory");
            for (uint32_t base = 0; base < n && count[s] <= kSeedHits; base += kWave) {   // select, hits (rules 2-3)
                const uint32_t j = base + (uint32_t)lane;
                uint32_t mine;
                const bool selected = seed_minimizer_selected(hk, 0u, j, j < n, n, reach, need, &mine);
                count[s] = seed_append(a, keys + s * kSeedHits, count[s], min_unhash(mine), selected, (int32_t)j, lane);
            }
            asm volatile("" ::: "memory");   // the next strand's keys land after this strand's reads of hk
        }
        seed_finish(a, keys, vt, r, L, count, lane);
    }
}

void seed_launch(const SeedArgs &a, uint32_t grid, size_t lds, hipStream_t s)
{
    hipLaunchKernelGGL(seed_candidates_kernel, dim3(grid), dim3(kWave), lds, s, a);
}
void seed_minimizer_launch(const SeedArgs &a, uint32_t grid, size_t lds, hipStream_t s)
{
    hipLaunchKernelGGL(seed_minimizer_kernel, dim3(grid), dim3(kWave), lds, s, a);
}
#else
void seed_launch(const SeedArgs &a, uint32_t grid, size_t lds, hipStream_t s);
void seed_minimizer_launch(const SeedArgs &a, uint32_t grid, size_t lds, hipStream_t s);
#endif

}  // namespace aim
