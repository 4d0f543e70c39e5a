// index.hpp -- the k-mer index of aim_index_build, built on the device (aim_hip.h, AIM_FEATURE_INDEX_DEVICE): ASCII reference bytes in,
// bucket[4^k + 1] and pos[] out, byte for byte what the host build writes.
//
// The job is a stable sort of the positions 0 .. ref_len - k by their k-mer's 2k-bit code. A position whose k-mer covers a byte other
// than upper-case A C G T gets the key 4^k, which sorts behind every code: those positions fill the unspecified tail of pos[], and
// pos_capacity = ref_len - k + 1 is exactly the room for them. The sort is a least-significant-digit radix sort with 8-bit digits,
// ceil((2k + 1) / 8) passes (3 up to k = 11, 4 from k = 12), over tiles of kIndexTile positions:
//
//   index_code_kernel       keys[p] from the reference bytes (a tile and its k - 1 bytes of halo staged in LDS), and the count of every
//                           code into bucket[] with integer atomics -- counts only: a sum does not depend on the order of arrival.
//   index_minimizer_kernel  aim_index_build_device_minimizers' code pass, in index_code_kernel's place: the code only for the (w, k)
//                           minimizers of the reference, the key 4^k for every other position (described above the kernel).
//   index_scan_*_kernel     exclusive prefix sum of a uint32 array in three launches (sums of up to kIndexScanParts contiguous parts; the
//                           scan of those sums by one workgroup; every part rescanned from its offset). Used once over bucket[] and
//                           once per pass over the digit table.
//   index_hist_kernel       table[digit][tile] = how many keys of the tile hold that digit.
//   index_scatter_kernel    after the scan table[digit][tile] is where the tile's first key of that digit goes; an entry lands at that
//                           plus its stable rank among the tile's keys of the same digit. The last pass writes positions straight into
//                           pos[] and no keys.
//
// STABLE AND DETERMINISTIC BY CONSTRUCTION. Nothing that decides where an entry lands is an atomic. A wavefront owns 1 024 consecutive
// entries of the tile and takes them 64 at a time: eight ballots (one per digit bit) give every lane the mask of the lanes that hold
// its digit, the population count below the lane is its rank in the step, and the lowest lane of each mask adds the mask's size to the
// wavefront's own LDS counter of that digit -- a plain read and write, ordered because LDS operations of one wavefront execute in
// order. After a barrier one thread per digit turns the four wavefronts' counters into bases (table entry + the earlier wavefronts'
// counts). One bucket that holds every position (poly-A) is the same code path at the same speed: one mask of 64 lanes per step.
// Every dependency between workgroups is a kernel boundary: no look-back, no flags, no spinning.
//
// LDS BANKS. The counters are ds_read_b32 / ds_write_b32 on (address / 4) % 32 within each 32-lane half, issued by the mask leaders
// only: one lane per distinct digit of the step, so distinct addresses always, and two leaders collide only when their digits agree
// modulo 32 (8 digits per bank). Random digits put 32 leaders per half on 32 banks with the usual birthday collisions (about 2 extra
// cycles per step, against 8 ballots and two global accesses per entry); a repeat-heavy tile has few leaders and no collisions. The
// base pass reads and writes counters at stride 256 dwords per thread over consecutive digits: consecutive banks per half. The code
// kernel reads the staged tile byte by byte: four consecutive lanes share a dword (broadcast), a half covers 8 consecutive dwords.
// The scan kernels keep 16 wave totals in LDS and every lane reads the same ones (broadcast). The minimizer kernel's neighbour reads
// hk[i - d] / hk[i + d] are consecutive dwords over the lanes at every distance d: 32 distinct banks per half.
//
// OCCUPANCY. 256 threads per workgroup. LDS is 4 KB (counters) or 4 112 B (tile + halo): four 1 280-B granules, so LDS allows 32
// workgroups per CU and is never the limit. The register bounds below keep 8 workgroups (8 wavefronts per SIMD, the hardware cap) for
// the streaming kernels; the scatter kernel holds 16 keys, 16 positions and 16 ranks per lane and is planned at 128 registers = 4
// wavefronts per SIMD, enough to hide its two dependent global accesses per entry. The minimizer kernel keeps the staged bytes of a
// tile and its halo (4 176 B) and one key per staged position (16 632 B): 20 816 B, 17 granules, 7 workgroups per CU = 7 wavefronts per
// SIMD, LDS-bound, with registers (64) for 8. No scratch memory in any of them.
//
// BYTES PER POSITION (P passes): code 1 read + 4 written; every pass reads the keys twice (histogram, scatter), the positions once from
// pass 1 on, and writes keys (not in the last pass) and positions: 5 + 16 + 20 (P - 2) + 16 = 57 B at P = 3 and 77 B at P = 4, plus
// 1 KB of table per tile, read twice and written twice per pass (1 B per position and pass), and 12 B per bucket entry for its scan.
// 64-bit arithmetic wherever tile * kIndexTile or digit * n_tiles + tile appears: ref_len reaches 2^32 - 2^25.
#pragma once

#include "aim_device.hpp"
#include "minimizer.hpp"

namespace aim {

constexpr uint32_t kIndexTile = 4096;                      // positions per tile (tests/test_index_device_*.py read it)
constexpr int kIndexThreads = 256;
constexpr int kIndexWaves = kIndexThreads / kWave;
constexpr int kIndexSteps = (int)kIndexTile / kIndexThreads;   // 64-entry steps per wavefront and tile
constexpr uint32_t kIndexDigits = 256;
constexpr uint32_t kIndexScanParts = 2048;                 // at most this many parts per scan (one workgroup scans their sums)
constexpr uint32_t kIndexScanBlock = 4 * kIndexThreads;    // entries a workgroup scans between two barriers
// the bounds tests/test_index_device_cpu.py checks in the code object (see OCCUPANCY above)
constexpr int kIndexCodeMaxVgpr = 64;
constexpr int kIndexHistMaxVgpr = 64;
constexpr int kIndexScanSumsMaxVgpr = 64;
constexpr int kIndexScanTopMaxVgpr = 64;
constexpr int kIndexScanApplyMaxVgpr = 64;
constexpr int kIndexScatterMaxVgpr = 128;
constexpr int kIndexMinimizerMaxVgpr = 64;                 // (tests/test_minimizers_cpu.py)
constexpr uint32_t kIndexMaxW = AIM_SEED_MAX_W;
// index_minimizer_kernel stages the tile, w - 1 positions of halo on each side, k - 1 bytes behind, and up to 3 bytes in front that
// align the first staged byte to a dword
constexpr uint32_t kIndexMinKeys = kIndexTile + 2 * (kIndexMaxW - 1);
constexpr uint32_t kIndexMinBytes = (kIndexMinKeys + (uint32_t)kMinMaxK - 1 + 3 + 15) / 16 * 16;

inline int index_passes(int32_t k) { return (2 * k + 1 + 7) / 8; }

// Where everything lives in d_scratch: three arrays of one dword per position (keys A, keys B, the second position buffer -- pos[]
// itself is the first), the digit table and the scan's part sums, each rounded up to 256 bytes.
struct IndexLayout {
    uint64_t n;          // positions, ref_len - k + 1 (0 below k)
    uint32_t n_tiles;
    uint64_t key_a, key_b, pos_s, table, parts, total;
};
inline IndexLayout index_layout(int32_t k, uint64_t ref_len)
{
    IndexLayout L{};
    if (ref_len < (uint64_t)k) return L;
    auto up = [](uint64_t x) { return (x + 255u) & ~255ull; };
    L.n = ref_len - (uint64_t)k + 1u;
    L.n_tiles = (uint32_t)((L.n + kIndexTile - 1u) / kIndexTile);
    const uint64_t arr = up(4u * L.n);
    L.key_a = 0;
    L.key_b = arr;
    L.pos_s = 2 * arr;
    L.table = 3 * arr;
    L.parts = L.table + up((uint64_t)kIndexDigits * 4u * L.n_tiles);
    L.total = L.parts + up(4u * kIndexScanParts);
    return L;
}

struct IndexArgs {
    const char *ref;
    uint64_t ref_len;
    int32_t k;
    uint32_t shift;                    // the pass's digit is (key >> shift) & 255
    uint64_t n;                        // positions
    uint32_t n_tiles;
    const uint32_t *key_in, *pos_in;   // pos_in NULL (pass 0): entry i is position i
    uint32_t *key_out, *pos_out;       // key_out NULL: the last pass
    uint32_t *table;                   // [256][n_tiles]
    uint32_t *bucket;
    uint32_t dbg_poison_lds;           // as in KArgs (AIM_DEBUG_POISON_LDS)
    int32_t w;                         // index_minimizer_kernel alone: the window, 1..kIndexMaxW
};

struct IndexScanArgs {
    uint32_t *data;
    uint64_t n, per_part;              // part g is data[g * per_part, min((g + 1) * per_part, n)); per_part is a multiple of kIndexScanBlock
    uint32_t *part;                    // [n_parts]
    uint32_t n_parts;
    uint32_t dbg_poison_lds;
};

#ifdef AIM_TU_INDEX   // the kernels live in tu_index.hip alone; capi_pipeline.hip sees the argument blocks and the launchers

__device__ __forceinline__ uint32_t index_scan_add(uint32_t v, int lane)   // inclusive wave prefix sum
{
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const uint32_t o = __shfl_up(v, d, kWave);
        if (lane >= d) v += o;
    }
    return v;
}

__device__ __forceinline__ bool index_is_base(uint32_t c)   // upper-case A C G T (seed_is_base)
{
    const uint32_t d = c - 65u;
    return d < 20u && ((0x80045u >> d) & 1u);
}

// The lanes of the wavefront that are valid and hold this lane's digit.
__device__ __forceinline__ uint64_t index_match(uint32_t d, bool valid)
{
    uint64_t m = __ballot(valid);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        const bool bit = (d >> b) & 1u;
        const uint64_t s = __ballot(bit);
        m &= bit ? s : ~s;
    }
    return m;
}

// One 64-entry step of a wavefront's stable count: returns how many earlier entries of this wavefront (earlier steps, lower lanes)
// hold the lane's digit, and adds the step to the wavefront's counters. Same-wave LDS traffic is ordered; the fences are for the compiler.
__device__ __forceinline__ uint32_t index_count_step(uint32_t *mine, uint32_t d, bool valid, int lane)
{
    const uint64_t m = index_match(d, valid);
    const int leader = __ffsll((unsigned long long)m) - 1;
    uint32_t old = 0;
    asm volatile("" ::: "memory");
    if (valid && lane == leader) {
        old = mine[d];
        mine[d] = old + (uint32_t)__popcll(m);
    }
    asm volatile("" ::: "memory");
    old = __shfl(old, valid ? leader : lane, kWave);
    return old + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
}

// Counts of the code pass: a run of equal codes in the wavefront (consecutive positions: poly-A, satellites) is one add of its length.
__device__ __forceinline__ void index_count_keys(uint32_t *bucket, uint32_t key, uint32_t sentinel, int lane)
{
    const uint32_t prev = __shfl_up(key, 1, kWave);
    const bool change = lane == 0 || prev != key;
    const uint64_t chg = __ballot(change);
    if (change && key != sentinel) {
        const uint64_t above = lane == kWave - 1 ? 0ull : chg >> (lane + 1);
        const uint32_t len = above ? (uint32_t)__ffsll((unsigned long long)above) : (uint32_t)(kWave - lane);
        atomicAdd(&bucket[key], len);
    }
}

__global__ __launch_bounds__(kIndexThreads) void index_code_kernel(IndexArgs a)
{
    __shared__ __align__(16) uint32_t tile4[(kIndexTile + 16) / 4];
    debug_poison_lds(a.dbg_poison_lds, (uint32_t)sizeof tile4, reinterpret_cast<char *>(tile4));
    const uint8_t *tile = reinterpret_cast<const uint8_t *>(tile4);
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int32_t k = a.k;
    const uint32_t sentinel = 1u << (2 * k);
    for (uint32_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        const uint64_t base = (uint64_t)t * kIndexTile;
        const uint64_t end = min(base + kIndexTile + (uint64_t)(k - 1), a.ref_len);   // bytes staged: the tile and its halo
        const uint32_t nd = (uint32_t)((end - base + 3u) >> 2);                     // (the reference has 16 bytes of slack)
        __syncthreads();   // the previous tile has been read
        const uint32_t *g = reinterpret_cast<const uint32_t *>(a.ref + base);
        for (uint32_t w = (uint32_t)tid; w < nd; w += kIndexThreads) tile4[w] = g[w];
        __syncthreads();
#pragma unroll 2
        for (int r = 0; r < kIndexSteps; ++r) {
            const uint32_t lp = (uint32_t)(r * kIndexThreads + tid);
            const uint64_t i = base + lp;
            const bool valid = i < a.n;
            uint32_t code = 0;
            bool ok = valid;
            if (valid) {
                const uint8_t *f = tile + lp;
                for (int j = 0; j < k; ++j) {
                    const uint32_t x = f[j];
                    ok = ok && index_is_base(x);
                    code |= ((x >> 1) & 3u) << (2 * j);
                }
            }
            const uint32_t key = ok ? code : sentinel;
            if (valid) a.key_out[i] = key;
            index_count_keys(a.bucket, key, sentinel, lane);
        }
    }
}

// The code pass of aim_index_build_device_minimizers: index_code_kernel with one more condition on a position -- it keeps its code only
// when it is a (w, k) minimizer of the reference (the rule in aim_hip.h), and gets the sentinel 4^k otherwise. Everything behind the
// code pass sees keys and counts as before.
//   stage   the bytes of the positions [plo, phi) = the tile and w - 1 positions on each side, clamped to [0, n), and the k - 1 bytes
//           behind the last one: dwords from the aligned byte below plo (the reference has 16 bytes of slack behind ref_len).
//   keys    hk[q - plo] = min_hash(code) of every staged position, kMinInvalid where the k-mer is invalid: each key computed once per
//           tile (the halo positions a second time by the neighbouring tile: 2 (w - 1) / kIndexTile, 1.5 % at w = 32).
//   select  the local test: a valid position i is selected iff L + R + 1 >= min(w, n), L the run of strictly greater keys to its left,
//           R the run of greater-or-equal keys to its right, each capped at w - 1 and at the sequence's ends. The staged range covers
//           exactly those neighbours. The loop over the distance d ends as soon as no lane of the wavefront still extends a run.
// LDS: 4 176 B of bytes + 16 632 B of keys, 20 816 B static with alignment, 17 granules of 1 280 B: 7 workgroups per CU (7 wavefronts per SIMD),
// which LDS bounds; kIndexMinimizerMaxVgpr = 64 would allow 8. No scratch. BANKS: the key pass reads bytes like index_code_kernel
// (four lanes share a dword) and writes consecutive dwords; the neighbour reads hk[li - d] / hk[li + d] are ds_read_b32 of consecutive
// dwords over the lanes at every d: 32 distinct banks per half, conflict-free.
// BYTES PER POSITION: 1 read + 4 written, as index_code_kernel, plus the halo's share.
__global__ __launch_bounds__(kIndexThreads) void index_minimizer_kernel(IndexArgs a)
{
    __shared__ __align__(16) uint32_t tile4[kIndexMinBytes / 4];
    __shared__ __align__(16) uint32_t hk[kIndexMinKeys];
    debug_poison_lds(a.dbg_poison_lds, (uint32_t)sizeof tile4, reinterpret_cast<char *>(tile4));
    debug_poison_lds(a.dbg_poison_lds, (uint32_t)sizeof hk, reinterpret_cast<char *>(hk));
    const uint8_t *tile = reinterpret_cast<const uint8_t *>(tile4);
    const int tid = threadIdx.x, lane = tid & (kWave - 1);
    const int32_t k = a.k;
    const uint32_t sentinel = 1u << (2 * k);
    const uint32_t reach = min((uint32_t)a.w, kIndexMaxW) - 1u;                     // neighbours looked at on each side
    const uint32_t need = (uint32_t)min((uint64_t)(reach + 1u), a.n);               // min(w, n)
    for (uint32_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        const uint64_t base = (uint64_t)t * kIndexTile;
        const uint64_t plo = base >= reach ? base - reach : 0u;                     // (base is 0 or at least kIndexTile: plo = 0 only in tile 0)
        const uint64_t phi = min(base + kIndexTile + reach, a.n);                   // staged positions [plo, phi), phi - plo <= kIndexMinKeys
        const uint64_t b0 = plo & ~3ull;
        const uint32_t skew = (uint32_t)(plo - b0);                                 // staged position q's bytes start at tile + skew + (q - plo)
        const uint32_t nk = (uint32_t)(phi - plo);
        const uint32_t nd = (nk + skew + (uint32_t)(k - 1) + 3u) >> 2;              // <= kIndexMinBytes / 4; phi + k - 1 <= ref_len
        __syncthreads();   // the previous tile has been read
        const uint32_t *g = reinterpret_cast<const uint32_t *>(a.ref + b0);
        for (uint32_t w = (uint32_t)tid; w < nd; w += kIndexThreads) tile4[w] = g[w];
        __syncthreads();
        for (uint32_t q = (uint32_t)tid; q < nk; q += kIndexThreads) {
            const uint8_t *f = tile + skew + q;
            uint32_t code = 0;
            bool ok = true;
            for (int j = 0; j < k; ++j) {
                const uint32_t x = f[j];
                ok = ok && index_is_base(x);
                code |= ((x >> 1) & 3u) << (2 * j);
            }
            hk[q] = ok ? min_hash(code) : kMinInvalid;
        }
        __syncthreads();
        const uint32_t off = (uint32_t)(base - plo);                                // hk index of the tile's first position
        for (int r = 0; r < kIndexSteps; ++r) {
            const uint32_t lp = (uint32_t)(r * kIndexThreads + tid);
            const uint64_t i = base + lp;
            const bool valid = i < a.n;
            const uint32_t li = off + lp;
            const uint32_t mine = valid ? hk[li] : kMinInvalid;
            bool left = mine != kMinInvalid, right = left;                          // the run on that side still extends
            uint32_t span = 1;                                                      // L + R + 1
            for (uint32_t d = 1; d <= reach; ++d) {
                if (!__ballot(left || right)) break;
                left = left && li >= d && hk[li - d] > mine;
                right = right && li + d < nk && hk[li + d] >= mine;
                span += (uint32_t)left + (uint32_t)right;
            }
            const uint32_t key = mine != kMinInvalid && span >= need ? min_unhash(mine) : sentinel;
            if (valid) a.key_out[i] = key;
            index_count_keys(a.bucket, key, sentinel, lane);
        }
    }
}

__global__ __launch_bounds__(kIndexThreads) void index_hist_kernel(IndexArgs a)
{
    __shared__ __align__(16) uint32_t cnt[kIndexWaves * kIndexDigits];
    debug_poison_lds(a.dbg_poison_lds, (uint32_t)sizeof cnt, reinterpret_cast<char *>(cnt));
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    uint32_t *mine = cnt + wave * kIndexDigits;
    for (uint32_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        const uint64_t base = (uint64_t)t * kIndexTile + (uint64_t)(wave * kIndexSteps * kWave);
        uint32_t key[kIndexSteps];
#pragma unroll
        for (int r = 0; r < kIndexSteps; ++r) {
            const uint64_t i = base + (uint64_t)(r * kWave + lane);
            key[r] = i < a.n ? a.key_in[i] : 0u;
        }
        __syncthreads();   // the previous tile's counters have been read
#pragma unroll
        for (int j = 0; j < (int)kIndexDigits / kWave; ++j) mine[j * kWave + lane] = 0;
#pragma unroll
        for (int r = 0; r < kIndexSteps; ++r) {
            const bool valid = base + (uint64_t)(r * kWave + lane) < a.n;
            (void)index_count_step(mine, (key[r] >> a.shift) & 255u, valid, lane);
        }
        __syncthreads();
        uint32_t sum = 0;
#pragma unroll
        for (int w = 0; w < kIndexWaves; ++w) sum += cnt[w * kIndexDigits + tid];
        a.table[(uint64_t)tid * a.n_tiles + t] = sum;
    }
}

__global__ __launch_bounds__(kIndexThreads) void index_scatter_kernel(IndexArgs a)
{
    __shared__ __align__(16) uint32_t cnt[kIndexWaves * kIndexDigits];
    debug_poison_lds(a.dbg_poison_lds, (uint32_t)sizeof cnt, reinterpret_cast<char *>(cnt));
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    uint32_t *mine = cnt + wave * kIndexDigits;
    for (uint32_t t = blockIdx.x; t < a.n_tiles; t += gridDim.x) {
        const uint64_t base = (uint64_t)t * kIndexTile + (uint64_t)(wave * kIndexSteps * kWave);
        uint32_t key[kIndexSteps], pos[kIndexSteps], rank[kIndexSteps];
#pragma unroll
        for (int r = 0; r < kIndexSteps; ++r) {
            const uint64_t i = base + (uint64_t)(r * kWave + lane);
            key[r] = i < a.n ? a.key_in[i] : 0u;
            pos[r] = a.pos_in ? (i < a.n ? a.pos_in[i] : 0u) : (uint32_t)i;
        }
        const uint32_t first = a.table[(uint64_t)tid * a.n_tiles + t];   // thread d: where the tile's first key of digit d goes
        __syncthreads();   // the previous tile's bases have been read
#pragma unroll
        for (int j = 0; j < (int)kIndexDigits / kWave; ++j) mine[j * kWave + lane] = 0;
#pragma unroll
        for (int r = 0; r < kIndexSteps; ++r) {
            const bool valid = base + (uint64_t)(r * kWave + lane) < a.n;
            rank[r] = index_count_step(mine, (key[r] >> a.shift) & 255u, valid, lane);
        }
        __syncthreads();
        {   // counters -> bases: the table entry, then each wavefront behind the ones before it
            uint32_t run = first;
#pragma unroll
            for (int w = 0; w < kIndexWaves; ++w) {
                const uint32_t c = cnt[w * kIndexDigits + tid];
                cnt[w * kIndexDigits + tid] = run;
                run += c;
            }
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < kIndexSteps; ++r) {
            if (base + (uint64_t)(r * kWave + lane) < a.n) {
                const uint64_t at = (uint64_t)mine[(key[r] >> a.shift) & 255u] + rank[r];
                if (at < a.n) {   // (always: the table is the scan of this tile's own counts)
                    if (a.key_out) a.key_out[at] = key[r];
                    a.pos_out[at] = pos[r];
                }
            }
        }
    }
}

// Sum over the workgroup, in every thread. wt: kIndexWaves dwords of LDS.
__device__ __forceinline__ uint32_t index_block_sum(uint32_t v, uint32_t *wt, int tid)
{
    const uint32_t incl = index_scan_add(v, tid & (kWave - 1));
    __syncthreads();
    if ((tid & (kWave - 1)) == kWave - 1) wt[tid >> 6] = incl;
    __syncthreads();
    uint32_t s = 0;
#pragma unroll
    for (int w = 0; w < kIndexWaves; ++w) s += wt[w];
    return s;
}

__global__ __launch_bounds__(kIndexThreads) void index_scan_sums_kernel(IndexScanArgs a)
{
    __shared__ uint32_t wt[kIndexWaves];
    debug_poison_lds(a.dbg_poison_lds, (uint32_t)sizeof wt, reinterpret_cast<char *>(wt));
    const int tid = threadIdx.x;
    for (uint32_t g = blockIdx.x; g < a.n_parts; g += gridDim.x) {
        const uint64_t lo = min((uint64_t)g * a.per_part, a.n), hi = min(lo + a.per_part, a.n);
        uint32_t s = 0;
        for (uint64_t i = lo + (uint64_t)tid; i < hi; i += kIndexThreads) s += a.data[i];
        s = index_block_sum(s, wt, tid);
        if (tid == 0) a.part[g] = s;
    }
}

__global__ __launch_bounds__(kIndexThreads) void index_scan_top_kernel(IndexScanArgs a)   // one workgroup: part[] -> its exclusive prefix sums
{
    __shared__ uint32_t wt[kIndexWaves];
    debug_poison_lds(a.dbg_poison_lds, (uint32_t)sizeof wt, reinterpret_cast<char *>(wt));
    constexpr int per = (int)kIndexScanParts / kIndexThreads;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    uint32_t v[per], s = 0;
#pragma unroll
    for (int j = 0; j < per; ++j) {
        const uint32_t g = (uint32_t)(tid * per + j);
        v[j] = g < a.n_parts ? a.part[g] : 0u;
        s += v[j];
    }
    const uint32_t incl = index_scan_add(s, lane);
    if (lane == kWave - 1) wt[wave] = incl;
    __syncthreads();
    uint32_t run = incl - s;
#pragma unroll
    for (int w = 0; w < kIndexWaves; ++w) run += w < wave ? wt[w] : 0u;
#pragma unroll
    for (int j = 0; j < per; ++j) {
        const uint32_t g = (uint32_t)(tid * per + j);
        if (g < a.n_parts) a.part[g] = run;
        run += v[j];
    }
}

__global__ __launch_bounds__(kIndexThreads) void index_scan_apply_kernel(IndexScanArgs a)   // data[] -> its exclusive prefix sums, part by part
{
    constexpr int sub = (int)kIndexScanBlock / kIndexThreads;
    __shared__ uint32_t wt[sub * kIndexWaves];
    debug_poison_lds(a.dbg_poison_lds, (uint32_t)sizeof wt, reinterpret_cast<char *>(wt));
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6;
    for (uint32_t g = blockIdx.x; g < a.n_parts; g += gridDim.x) {
        const uint64_t lo = min((uint64_t)g * a.per_part, a.n), hi = min(lo + a.per_part, a.n);
        uint32_t run = a.part[g];
        for (uint64_t blk = lo; blk < hi; blk += kIndexScanBlock) {
            uint32_t v[sub], incl[sub];
#pragma unroll
            for (int j = 0; j < sub; ++j) {
                const uint64_t i = blk + (uint64_t)(j * kIndexThreads + tid);
                v[j] = i < hi ? a.data[i] : 0u;
                incl[j] = index_scan_add(v[j], lane);
            }
            __syncthreads();   // the previous block's totals have been read
            if (lane == kWave - 1) {
#pragma unroll
                for (int j = 0; j < sub; ++j) wt[j * kIndexWaves + wave] = incl[j];
            }
            __syncthreads();
            uint32_t before[sub], total = 0;
#pragma unroll
            for (int q = 0; q < sub * kIndexWaves; ++q) {   // (q = j * kIndexWaves + w: the order of the entries)
                if (q % kIndexWaves == 0) before[q / kIndexWaves] = total;
                const uint32_t x = wt[q];
                if (q % kIndexWaves < wave) before[q / kIndexWaves] += x;
                total += x;
            }
#pragma unroll
            for (int j = 0; j < sub; ++j) {
                const uint64_t i = blk + (uint64_t)(j * kIndexThreads + tid);
                if (i < hi) a.data[i] = run + before[j] + incl[j] - v[j];
            }
            run += total;
        }
    }
}

void index_launch_code(const IndexArgs &a, uint32_t grid, hipStream_t s) { hipLaunchKernelGGL(index_code_kernel, dim3(grid), dim3(kIndexThreads), 0, s, a); }
void index_launch_minimizer(const IndexArgs &a, uint32_t grid, hipStream_t s) { hipLaunchKernelGGL(index_minimizer_kernel, dim3(grid), dim3(kIndexThreads), 0, s, a); }
void index_launch_hist(const IndexArgs &a, uint32_t grid, hipStream_t s) { hipLaunchKernelGGL(index_hist_kernel, dim3(grid), dim3(kIndexThreads), 0, s, a); }
void index_launch_scatter(const IndexArgs &a, uint32_t grid, hipStream_t s) { hipLaunchKernelGGL(index_scatter_kernel, dim3(grid), dim3(kIndexThreads), 0, s, a); }
void index_launch_scan(const IndexScanArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(index_scan_sums_kernel, dim3(a.n_parts), dim3(kIndexThreads), 0, s, a);
    hipLaunchKernelGGL(index_scan_top_kernel, dim3(1), dim3(kIndexThreads), 0, s, a);
    hipLaunchKernelGGL(index_scan_apply_kernel, dim3(a.n_parts), dim3(kIndexThreads), 0, s, a);
}
#else
void index_launch_code(const IndexArgs &a, uint32_t grid, hipStream_t s);
void index_launch_minimizer(const IndexArgs &a, uint32_t grid, hipStream_t s);
void index_launch_hist(const IndexArgs &a, uint32_t grid, hipStream_t s);
void index_launch_scatter(const IndexArgs &a, uint32_t grid, hipStream_t s);
void index_launch_scan(const IndexScanArgs &a, hipStream_t s);   // sums, top, apply
#endif

}  // namespace aim
