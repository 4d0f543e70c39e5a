// batch_io.hpp -- the wire formats either side of the alignment kernels:
//
//   * unpack_rows_kernel / scatter_raw_rows_kernel: a PACKED batch (2 bits per base + a side list of pairs that hold a
//     byte outside A/C/G/T, which travel as raw rows) is expanded in HBM into the reference's own layout --
//     char[n][READ_SIZE] ASCII rows (WFA/DPU-WRAM/host/host.c:126-127, 258-268) -- so every alignment kernel runs
//     unchanged and bit-exact.  What crosses PCIe is READ_SIZE/4 bytes per sequence instead of READ_SIZE.
//   * gather_text_rows_kernel / gather_text_packed_kernel / gather_todo_rows_kernel (AIM_FLAG_REF_TEXTS): texts named as
//     (position, strand) windows of a device-resident reference are gathered into the same char[n][READ_SIZE] rows (or into
//     packed rows plus a to-do list of the windows holding a byte outside A/C/G/T, for the fused packed lane kernel).
//   * cigar_rle_kernel: the run-length encoding edit_cigar_print does on the host (host.c:69-89) done on the device
//     over ops[begin_offset, end_offset), so that ~3 runs per pair cross PCIe instead of 2*READ_SIZE op bytes.
//
// All are pure data movement: HBM-bound, coalesced, no LDS.
#pragma once

#include "aim_device.hpp"
#include "batch_sizes.hpp"

namespace aim {

// ---- packed batches --------------------------------------------------------------------------------------------------
// code = (ascii >> 1) & 3: A 0, C 1, T 2, G 3 (the mapping the kernels use internally); base i of a sequence sits at bits
// [2*(i%16), 2*(i%16)+1] of dword i/16 of its row; a row is ceil(READ_SIZE/16) dwords.
__host__ __device__ inline uint32_t packed_row_dwords(int read_size) { return (uint32_t)(read_size + 15) / 16u; }

// ---- launchers -------------------------------------------------------------------------------------------------------
// The kernels below are instantiated in ONE translation unit (tu_batch_io.hip defines AIM_TU_BATCH_IO); every other includer sees
// these declarations, packed_row_dwords and the two grid rules only. A launcher owns its kernel's grid and block; the caller checks
// hipGetLastError().
inline dim3 blocks_256(uint64_t threads) { return dim3((unsigned)((threads + 255) / 256)); }   // one thread per element, 256 per workgroup
// The row gathers (gather_text_rows_kernel here, group_rows_kernel in groups.hpp): a thread moves 4 nw bytes of one row -- 16-B stores
// where the row stride READ_SIZE allows them, else 8-B.
struct RowGather { int nw; dim3 grid; };
inline RowGather row_gather(int read_size, uint32_t n_rows)
{
    const int nw = (read_size & 15) == 0 ? 4 : 2;
    return RowGather{nw, blocks_256((uint64_t)n_rows * (uint64_t)(read_size / (4 * nw)))};
}
#pragma GCC visibility push(hidden)
// grid.y = planes: 1 expands / scatters the pattern rows only (the texts of a reference batch are gathered), 2 both
void unpack_rows_launch(const KArgs &ka, const uint32_t *packedP, const uint32_t *packedT, char *outP, char *outT, unsigned planes, hipStream_t s);
void scatter_raw_rows_launch(int read_size, uint32_t n_raw, const uint32_t *raw_pairs, const char *rawP, const char *rawT, char *outP, char *outT,
                             unsigned planes, hipStream_t s);
void pack_rows_launch(const KArgs &ka, uint32_t *packedP, uint32_t *packedT, uint32_t *flag_bits, uint32_t *todo, hipStream_t s);
void gather_elems_launch(const uint32_t *src, const uint32_t *idx, uint32_t n, uint32_t dw, uint32_t *dst, hipStream_t s);
void scatter_elems_launch(const uint32_t *src, const uint32_t *idx, uint32_t n, uint32_t dw, uint32_t *dst, hipStream_t s);
void cigar_rle_launch(const KArgs &ka, aim_cigar_t *hdr, uint32_t *runs, uint32_t runs_cap, uint32_t *cursor, hipStream_t s);   // pairs 0 .. ka.n_pairs - 1
void cigar_rle_todo_launch(const KArgs &ka, const uint32_t *todo, aim_cigar_t *hdr, uint32_t *runs, uint32_t runs_cap, uint32_t *cursor, hipStream_t s);
void unpack_todo_rows_launch(const KArgs &ka, const uint32_t *todo, const uint32_t *packedP, const uint32_t *packedT, char *outP, char *outT, hipStream_t s);
// AIM_FLAG_REF_TEXTS: text rows [n_rows][READ_SIZE] of `out` gathered from the reference; row r is the window of pair idx[r]
// (idx == nullptr: pair r). ka carries the params and the requests. Nothing is launched for n_rows == 0.
void gather_text_rows_launch(const KArgs &ka, const uint64_t *text_pos, const char *ref, uint64_t ref_len, const uint32_t *idx, uint32_t n_rows, char *out,
                             hipStream_t s);
void gather_text_packed_launch(const KArgs &ka, const uint64_t *text_pos, const char *ref, uint64_t ref_len, uint32_t *packedT, uint32_t *flag_bits,
                               uint32_t *todo, hipStream_t s);
void gather_todo_rows_launch(const KArgs &ka, const uint32_t *todo, const uint64_t *text_pos, const char *ref, uint64_t ref_len, const uint32_t *packedP,
                             char *outP, char *outT, hipStream_t s);
// escalate_select_kernel, then escalate_list_kernel on the same grid: the pairs of `res` whose score is `over`, as the list `todo`
void escalate_list_launch(const uint32_t *res, uint32_t n_pairs, uint32_t stride_dw, uint32_t score_dw, int32_t over, uint2 *masks, uint32_t *counts,
                          uint32_t *todo, hipStream_t s);
#pragma GCC visibility pop

#ifdef AIM_TU_BATCH_IO
// One thread expands 8 bases (16 packed bits -> 8 ASCII bytes); bytes at or beyond the sequence length are zero, like
// the parser's rows.  grid.y: 0 = patterns, 1 = texts.
__global__ __launch_bounds__(256) void unpack_rows_kernel(KArgs a, const uint32_t *packedP, const uint32_t *packedT, char *outP, char *outT)
{
    const int rs = a.p.read_size;
    const uint32_t per_row = (uint32_t)rs / 8u;                    // 8-byte pieces per ASCII row
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)a.n_pairs * per_row) return;
    const uint32_t pair = (uint32_t)(t / per_row), piece = (uint32_t)(t - (uint64_t)pair * per_row);
    const bool is_text = blockIdx.y != 0;
    const aim_request_t rq = load_request(a, pair);
    const int len = is_text ? rq.text_len : rq.pattern_len;
    const uint16_t *src = reinterpret_cast<const uint16_t *>((is_text ? packedT : packedP) + (uint64_t)pair * packed_row_dwords(rs));
    const uint32_t bits = src[piece];
    // spread the eight 2-bit codes into bytes, then look "ACTG"[code] up with v_perm
    const uint32_t lo = (bits & 3u) | ((bits & 0xCu) << 6) | ((bits & 0x30u) << 12) | ((bits & 0xC0u) << 18);
    const uint32_t hb = bits >> 8;
    const uint32_t hi = (hb & 3u) | ((hb & 0xCu) << 6) | ((hb & 0x30u) << 12) | ((hb & 0xC0u) << 18);
    uint32_t w0 = __builtin_amdgcn_perm(0u, 0x47544341u, lo);
    uint32_t w1 = __builtin_amdgcn_perm(0u, 0x47544341u, hi);
    const int rem = len - (int)piece * 8;                          // valid bytes of this piece
    if (rem < 8) {
        const uint64_t keep = rem <= 0 ? 0ull : ((1ull << (8 * rem)) - 1ull);
        w0 &= (uint32_t)keep;
        w1 &= (uint32_t)(keep >> 32);
    }
    uint2 *dst = reinterpret_cast<uint2 *>((is_text ? outT : outP) + (uint64_t)pair * rs) + piece;
    *dst = make_uint2(w0, w1);
}

// Side list: raw_pairs[j] is the batch index of the j-th pair that could not be packed; its ASCII rows are copied verbatim.
__global__ __launch_bounds__(256) void scatter_raw_rows_kernel(int read_size, uint32_t n_raw, const uint32_t *raw_pairs, const char *rawP,
                                                               const char *rawT, char *outP, char *outT)
{
    const uint32_t per_row = (uint32_t)read_size / 8u;
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)n_raw * per_row) return;
    const uint32_t j = (uint32_t)(t / per_row), piece = (uint32_t)(t - (uint64_t)j * per_row);
    const uint32_t pair = raw_pairs[j];
    const bool is_text = blockIdx.y != 0;
    const uint2 v = reinterpret_cast<const uint2 *>((is_text ? rawT : rawP) + (uint64_t)j * read_size)[piece];
    reinterpret_cast<uint2 *>((is_text ? outT : outP) + (uint64_t)pair * read_size)[piece] = v;
}

// The inverse of unpack_rows_kernel: ASCII rows -> packed rows on the device, for configurations only the packed lane kernel
// covers (READ_SIZE other than 80 / 112) when the batch arrived as ASCII rows (the default ABI). One thread packs 16 bases
// (one output dword) and validates them by decoding back; a pair with a byte outside A/C/G/T inside either sequence is
// appended ONCE (flag bit per pair) to the to-do list {count @0, pair ids @16..} that the general kernel drains afterwards
// over the ASCII rows -- the same hand-over wfa_group_kernel uses. grid.y: 0 = patterns, 1 = texts.
typedef uint32_t pk_in_u32x4 __attribute__((ext_vector_type(4), aligned(4)));
__global__ __launch_bounds__(256) void pack_rows_kernel(KArgs a, uint32_t *packedP, uint32_t *packedT, uint32_t *flag_bits, uint32_t *todo)
{
    const int rs = a.p.read_size;
    const uint32_t npw = packed_row_dwords(rs);
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)a.n_pairs * npw) return;
    const uint32_t pair = (uint32_t)(t / npw), j = (uint32_t)(t - (uint64_t)pair * npw);
    const bool is_text = blockIdx.y != 0;
    const aim_request_t rq = load_request(a, pair);
    const int len = is_text ? rq.text_len : rq.pattern_len;
    const char *row = (is_text ? a.texts : a.patterns) + (uint64_t)pair * rs + 16u * j;   // (the arrays carry >= 16 B of tail slack)
    const pk_in_u32x4 v = *reinterpret_cast<const pk_in_u32x4 *>(row);
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
    uint32_t out = 0, bad = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rem = len - (int)(16u * j + 4u * i);
        const uint32_t mask = rem >= 4 ? ~0u : (rem <= 0 ? 0u : ((1u << (8 * rem)) - 1u));
        const uint32_t av = w[i] & mask;
        const uint32_t c = (av >> 1) & 0x03030303u & mask;
        const uint32_t rec = __builtin_amdgcn_perm(0u, 0x47544341u, c) & mask;
        bad |= rec ^ av;
        out |= __builtin_amdgcn_udot4(c, 0x40100401u, 0u, false) << (8 * i);
    }
    (is_text ? packedT : packedP)[t] = out;
    if (bad) {
        const uint32_t bit = 1u << (pair & 31u);
        const uint32_t old = atomicOr(&flag_bits[pair >> 5], bit);
        if (!(old & bit)) {
            const uint32_t slot = atomicAdd(&todo[0], 1u);
            todo[16 + slot] = pair;
        }
    }
}

// Raw side pass of a packed batch whose alignment kernel read the packed rows itself (aim_capi.hip): the pairs of the side
// list are aligned by the ASCII kernels as a small batch of their own -- requests gathered, results scattered back.
// Elements are `dw` dwords (requests 2 / 4, results 2 / 6, aim_cigar_t 4).
__global__ __launch_bounds__(256) void gather_elems_kernel(const uint32_t *src, const uint32_t *idx, uint32_t n, uint32_t dw, uint32_t *dst)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)n * dw) return;
    const uint32_t j = (uint32_t)(t / dw), w = (uint32_t)(t - (uint64_t)j * dw);
    dst[t] = src[(uint64_t)idx[j] * dw + w];
}
__global__ __launch_bounds__(256) void scatter_elems_kernel(const uint32_t *src, const uint32_t *idx, uint32_t n, uint32_t dw, uint32_t *dst)
{
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)n * dw) return;
    const uint32_t j = (uint32_t)(t / dw), w = (uint32_t)(t - (uint64_t)j * dw);
    dst[(uint64_t)idx[j] * dw + w] = src[t];
}

// ---- compact CIGAR -------------------------------------------------------------------------------------------------
// One pair per lane.  Pass 1 counts the runs of ops[begin, end) word-wise (a run starts where a byte differs from its
// predecessor), the wavefront reserves its runs with ONE atomic add on the batch cursor, pass 2 writes them:
// run = (length << 8) | op character.  Placement in the run buffer depends on scheduling, content does not: each header
// carries its own offset.
__device__ __forceinline__ uint32_t nonzero_byte_mask(uint32_t x)   // 0x80 in every non-zero byte
{
    return (((x & 0x7f7f7f7fu) + 0x7f7f7f7fu) | x) & 0x80808080u;
}

// one wavefront of 64 pairs: `pair` is this lane's pair (any value when !active); all 64 lanes must call
__device__ __forceinline__ void cigar_rle_wave(const KArgs &a, uint32_t pair, bool active, int lane, aim_cigar_t *hdr, uint32_t *runs, uint32_t runs_cap,
                                               uint32_t *cursor)
{
    const int rs = a.p.read_size;
    aim_result_t r;
    r.begin_offset = 0; r.end_offset = 0; r.score = 0; r.status = AIM_PAIR_OK; r.idx = 0; r.max_operations = 0;
    if (active) r = a.res[pair];
    // edit_cigar_print (host.c:69-89) always prints ops[begin_offset] as a first run, then extends / splits up to end_offset
    int b = r.begin_offset < 0 ? 0 : r.begin_offset;
    int e = r.end_offset > 2 * rs ? 2 * rs : r.end_offset;
    if (e <= b) e = b + 1;
    if (b >= 2 * rs) { b = 2 * rs - 1; e = 2 * rs; }
    // (ends-free pairs over MAX_SCORE carry an empty CIGAR, begin_offset == end_offset: no run, aim_hip.h AIM_FLAG_ENDSFREE)
    const bool walk = active && r.status == AIM_PAIR_OK && !((a.p.flags & AIM_FLAG_ENDSFREE) && r.end_offset <= r.begin_offset);
    const uint32_t *row = reinterpret_cast<const uint32_t *>(a.ops + (uint64_t)pair * 2 * rs);
    // boundary mask of word w: bit 8j+7 set <=> byte 4w+j differs from byte 4w+j-1, restricted to positions in (b, e)
    auto boundaries = [&](int w, uint32_t cur, uint32_t prev) -> uint32_t {
        uint32_t m = nonzero_byte_mask(cur ^ __builtin_amdgcn_alignbyte(cur, prev, 3u));   // cur ^ (bytes shifted up by one, prev's top byte in)
        const int lo = b + 1 - 4 * w, hi = e - 4 * w;                                     // keep byte j iff lo <= j < hi
        if (lo > 0) m &= lo >= 4 ? 0u : (0xffffffffu << (8 * lo));
        if (hi < 4) m &= hi <= 0 ? 0u : (0xffffffffu >> (8 * (4 - hi)));
        return m;
    };
    uint32_t n_runs = 0;
    if (walk) {
        n_runs = 1;
        uint32_t prev = 0;
        for (int w = b >> 2; w <= (e - 1) >> 2; ++w) {
            const uint32_t cur = row[w];
            n_runs += (uint32_t)__builtin_popcount(boundaries(w, cur, prev));
            prev = cur;
        }
    }
    // wave-level exclusive prefix sum of n_runs (DPP row scans + row broadcasts), one atomic for the wavefront
    uint32_t incl = n_runs;
#define AIM_RLE_SCAN(ctrl, rmask) incl += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)incl, ctrl, rmask, 0xf, false)
    AIM_RLE_SCAN(0x111, 0xf);   // row_shr:1
    AIM_RLE_SCAN(0x112, 0xf);   // row_shr:2
    AIM_RLE_SCAN(0x114, 0xf);   // row_shr:4
    AIM_RLE_SCAN(0x118, 0xf);   // row_shr:8
    AIM_RLE_SCAN(0x142, 0xa);   // row_bcast:15
    AIM_RLE_SCAN(0x143, 0xc);   // row_bcast:31
#undef AIM_RLE_SCAN
    const uint32_t total = (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
    uint32_t base = 0;
    if (lane == 0 && total) base = atomicAdd(cursor, total);
    base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    const uint32_t off = base + incl - n_runs;
    // aim_cigar_t carries n_runs in 16 bits and a run its length in 24: a pair beyond either (GenASM long reads with > 65 535
    // runs, l >~ 330 kb at e = 10 %) reports AIM_CIGAR_OVERFLOW -- the caller then gathers ops rows -- instead of a truncated count
    const bool fits = off + n_runs <= runs_cap && n_runs <= 0xffffu && (e - b) < (1 << 24);
    if (walk && fits) {
        uint32_t prev = 0, at = off;
        int start = b;
        for (int w = b >> 2; w <= (e - 1) >> 2; ++w) {
            const uint32_t cur = row[w];
            uint32_t m = boundaries(w, cur, prev);
            while (m) {
                const int j = __builtin_ctz(m) >> 3;              // byte index of the boundary inside the word
                const int pos = 4 * w + j;
                const uint32_t op = (j ? (cur >> (8 * (j - 1))) : (prev >> 24)) & 0xffu;   // the byte before the boundary
                runs[at++] = ((uint32_t)(pos - start) << 8) | op;
                start = pos;
                m &= m - 1;
            }
            prev = cur;
        }
        const uint32_t lw = row[(e - 1) >> 2];
        runs[at] = ((uint32_t)(e - start) << 8) | ((lw >> (8 * ((e - 1) & 3))) & 0xffu);
    }
    if (active) {
        aim_cigar_t h;
        h.idx = r.idx;
        h.score = r.score;
        h.run_offset = off;
        h.n_runs = (uint16_t)((walk && fits) ? n_runs : 0u);
        h.status = (uint16_t)((uint32_t)r.status | ((walk && !fits) ? AIM_CIGAR_OVERFLOW : 0u));
        hdr[pair] = h;
    }
}

__global__ __launch_bounds__(64) void cigar_rle_kernel(KArgs a, aim_cigar_t *hdr, uint32_t *runs, uint32_t runs_cap, uint32_t *cursor)
{
    const int lane = threadIdx.x;
    const uint32_t pair = blockIdx.x * kWave + lane;
    cigar_rle_wave(a, pair, pair < a.n_pairs, lane, hdr, runs, runs_cap, cursor);
}

// The same over a device-side list of pairs (the to-do list of wfa_group_kernel: {count @0, pair ids @16..}, wfa_lane.hpp
// LANE_TODO_*): the general kernel aligned those pairs into result_t + ops rows; a fused batch wants their compact CIGAR.
__global__ __launch_bounds__(64) void cigar_rle_todo_kernel(KArgs a, const uint32_t *todo, aim_cigar_t *hdr, uint32_t *runs, uint32_t runs_cap, uint32_t *cursor)
{
    const int lane = threadIdx.x;
    const uint32_t count = todo[0];
    for (uint32_t base = blockIdx.x * kWave; base < count; base += gridDim.x * kWave) {
        const uint32_t i = base + lane;
        const bool active = i < count;
        const uint32_t pair = active ? todo[16 + i] : 0u;
        cigar_rle_wave(a, pair, active, lane, hdr, runs, runs_cap, cursor);
    }
}

// ... and the expansion of exactly those pairs' packed rows into the ASCII rows the general kernel reads (8 bases per thread).
__global__ __launch_bounds__(256) void unpack_todo_rows_kernel(KArgs a, const uint32_t *todo, const uint32_t *packedP, const uint32_t *packedT, char *outP, char *outT)
{
    const int rs = a.p.read_size;
    const uint32_t per_row = (uint32_t)rs / 8u;
    const uint64_t total = (uint64_t)todo[0] * per_row * 2u;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const bool is_text = t & 1u;
        const uint64_t u = t >> 1;
        const uint32_t pair = todo[16 + (uint32_t)(u / per_row)], piece = (uint32_t)(u % per_row);
        const aim_request_t rq = load_request(a, pair);
        const int len = is_text ? rq.text_len : rq.pattern_len;
        const uint16_t *src = reinterpret_cast<const uint16_t *>((is_text ? packedT : packedP) + (uint64_t)pair * packed_row_dwords(rs));
        const uint32_t bits = src[piece];
        const uint32_t lo = (bits & 3u) | ((bits & 0xCu) << 6) | ((bits & 0x30u) << 12) | ((bits & 0xC0u) << 18);
        const uint32_t hb = bits >> 8;
        const uint32_t hi = (hb & 3u) | ((hb & 0xCu) << 6) | ((hb & 0x30u) << 12) | ((hb & 0xC0u) << 18);
        uint32_t w0 = __builtin_amdgcn_perm(0u, 0x47544341u, lo);
        uint32_t w1 = __builtin_amdgcn_perm(0u, 0x47544341u, hi);
        const int rem = len - (int)piece * 8;
        if (rem < 8) {
            const uint64_t keep = rem <= 0 ? 0ull : ((1ull << (8 * rem)) - 1ull);
            w0 &= (uint32_t)keep;
            w1 &= (uint32_t)(keep >> 32);
        }
        reinterpret_cast<uint2 *>((is_text ? outT : outP) + (uint64_t)pair * rs)[piece] = make_uint2(w0, w1);
    }
}

// ---- reference windows (AIM_FLAG_REF_TEXTS) -------------------------------------------------------------------------------
// text_pos = window start (bits 0..62) | strand << 63. Strand 0: text[i] = ref[pos + i]; strand 1: text[i] = comp(ref[pos + len - 1 - i]),
// comp swapping A<->T, C<->G, a<->t, c<->g and keeping every other byte. Loads never leave [0, ref_len + kRefSlack): a window the
// host check would refuse (stateless callers) reads zeros where it runs out, never outside the buffer.
constexpr uint64_t kRefSlack = 16;                 // addressable bytes behind the reference (aim_hip.h: the row buffers' slack)
constexpr uint64_t kRefPosMask = ~(1ull << 63);

// per-byte complement of four bytes: A^T = a^t = 0x15, C^G = c^g = 0x04 (selects built from exact per-byte equality masks)
__device__ __forceinline__ uint32_t ref_comp4(uint32_t x)
{
    const uint32_t u = x & 0xDFDFDFDFu;             // fold case (bit 5): only 'A' / 'a' map to 0x41, etc.
    const uint32_t zA = ~nonzero_byte_mask(u ^ 0x41414141u), zT = ~nonzero_byte_mask(u ^ 0x54545454u);
    const uint32_t zC = ~nonzero_byte_mask(u ^ 0x43434343u), zG = ~nonzero_byte_mask(u ^ 0x47474747u);
    const uint32_t at = ((zA | zT) & 0x80808080u) >> 7, cg = ((zC | zG) & 0x80808080u) >> 7;   // 0x01 per selected byte
    return x ^ (at * 0x15u) ^ (cg * 0x04u);
}

typedef uint32_t ref_u32x2 __attribute__((ext_vector_type(2), aligned(4)));

// NW dwords of the reference from byte offset s (may be negative or past the end: such dwords read as zero). Aligned wide loads of
// NW + 1 dwords, then a byte funnel (v_alignbyte) to the unaligned start.
template <int NW>
__device__ __forceinline__ void ref_load(const char *ref, int64_t s, uint64_t lim, uint32_t (&w)[NW])
{
    const int64_t a = s & ~(int64_t)3;
    const uint32_t sh = (uint32_t)(s & 3);
    const uint32_t *p = reinterpret_cast<const uint32_t *>(ref + a);
    uint32_t d[NW + 1];
    if (a >= 0 && (uint64_t)a + 4u * (NW + 1) <= lim) {
        if constexpr (NW == 4) {
            const pk_in_u32x4 v = *reinterpret_cast<const pk_in_u32x4 *>(p);
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
        } else {
            const ref_u32x2 v = *reinterpret_cast<const ref_u32x2 *>(p);
            d[0] = v.x; d[1] = v.y;
        }
        d[NW] = p[NW];
    } else {
#pragma unroll
        for (int k = 0; k <= NW; ++k) {
            const int64_t ak = a + 4 * k;
            d[k] = (ak >= 0 && (uint64_t)ak + 4u <= lim) ? p[k] : 0u;
        }
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = __builtin_amdgcn_alignbyte(d[i + 1], d[i], sh);
}

// Bytes [o, o + 4 NW) of one text row: the window's bytes, zero at and past len.
template <int NW>
__device__ __forceinline__ void ref_piece(const char *ref, uint64_t ref_len, uint64_t tp, int len, int o, uint32_t (&w)[NW])
{
    const int rem = len - o;
#pragma unroll
    for (int i = 0; i < NW; ++i) w[i] = 0u;
    if (rem <= 0) return;
    const uint64_t lim = ref_len + kRefSlack;
    const uint64_t pos = min(tp & kRefPosMask, lim);   // (no overflow below for positions a check would refuse)
    if (!(tp >> 63)) {
        ref_load<NW>(ref, (int64_t)pos + o, lim, w);
    } else {
        // the source of bytes o .. o + 4 NW - 1 is ref[pos + len - o - 4 NW, pos + len - o), read forward, then reversed with
        // v_perm (dword order and bytes) and complemented
        uint32_t f[NW];
        ref_load<NW>(ref, (int64_t)pos + len - o - 4 * NW, lim, f);
#pragma unroll
        for (int i = 0; i < NW; ++i) w[i] = ref_comp4(__builtin_amdgcn_perm(0u, f[NW - 1 - i], 0x00010203u));
    }
    if (rem < 4 * NW) {
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int r = rem - 4 * i;
            w[i] &= r >= 4 ? ~0u : (r <= 0 ? 0u : ((1u << (8 * r)) - 1u));
        }
    }
}

// ASCII text rows: one thread writes W = 4 NW bytes of one row (16-B stores when READ_SIZE is a multiple of 16, else 8-B).
// Row r is the window of pair idx[r] (idx == nullptr: pair r); rows [0, n_rows) of `out`.
template <int NW>
__global__ __launch_bounds__(256) void gather_text_rows_kernel(KArgs a, const uint64_t *text_pos, const char *ref, uint64_t ref_len, const uint32_t *idx,
                                                               uint32_t n_rows, char *out)
{
    const int rs = a.p.read_size;
    const uint32_t per_row = (uint32_t)rs / (4u * NW);
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)n_rows * per_row) return;
    const uint32_t row = (uint32_t)(t / per_row), piece = (uint32_t)(t - (uint64_t)row * per_row);
    const uint32_t pair = idx ? idx[row] : row;
    const int len = load_request(a, pair).text_len;
    uint32_t w[NW];
    ref_piece<NW>(ref, ref_len, text_pos[pair], len, (int)piece * 4 * NW, w);
    char *dst = out + (uint64_t)row * rs + (uint64_t)piece * 4 * NW;
    if constexpr (NW == 4) *reinterpret_cast<uint4 *>(dst) = make_uint4(w[0], w[1], w[2], w[3]);
    else *reinterpret_cast<uint2 *>(dst) = make_uint2(w[0], w[1]);
}

// Packed text rows for the fused packed lane kernel: one thread gathers 16 bases and packs them into one dword (pack_rows_kernel's
// encoding and check); a window holding a byte outside A/C/G/T is appended once (flag bit per pair) to the to-do list
// {count @0, pair ids @16..}, whose pairs gather_todo_rows_kernel then writes as ASCII rows for the general kernel.
__global__ __launch_bounds__(256) void gather_text_packed_kernel(KArgs a, const uint64_t *text_pos, const char *ref, uint64_t ref_len, uint32_t *packedT,
                                                                 uint32_t *flag_bits, uint32_t *todo)
{
    const int rs = a.p.read_size;
    const uint32_t npw = packed_row_dwords(rs);
    const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (uint64_t)a.n_pairs * npw) return;
    const uint32_t pair = (uint32_t)(t / npw), j = (uint32_t)(t - (uint64_t)pair * npw);
    const int len = load_request(a, pair).text_len;
    uint32_t w[4];
    ref_piece<4>(ref, ref_len, text_pos[pair], len, (int)(16u * j), w);
    uint32_t out = 0, bad = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int rem = len - (int)(16u * j + 4u * i);
        const uint32_t mask = rem >= 4 ? ~0u : (rem <= 0 ? 0u : ((1u << (8 * rem)) - 1u));
        const uint32_t c = (w[i] >> 1) & 0x03030303u & mask;
        const uint32_t rec = __builtin_amdgcn_perm(0u, 0x47544341u, c) & mask;
        bad |= rec ^ w[i];
        out |= __builtin_amdgcn_udot4(c, 0x40100401u, 0u, false) << (8 * i);
    }
    packedT[t] = out;
    if (bad) {
        const uint32_t bit = 1u << (pair & 31u);
        const uint32_t old = atomicOr(&flag_bits[pair >> 5], bit);
        if (!(old & bit)) {
            const uint32_t slot = atomicAdd(&todo[0], 1u);
            todo[16 + slot] = pair;
        }
    }
}

// The to-do pairs of gather_text_packed_kernel as ASCII rows (8 bytes per thread): the pattern expanded from its packed row, the text
// gathered from the reference.
__global__ __launch_bounds__(256) void gather_todo_rows_kernel(KArgs a, const uint32_t *todo, const uint64_t *text_pos, const char *ref, uint64_t ref_len,
                                                               const uint32_t *packedP, char *outP, char *outT)
{
    const int rs = a.p.read_size;
    const uint32_t per_row = (uint32_t)rs / 8u;
    const uint64_t total = (uint64_t)todo[0] * per_row * 2u;
    for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
        const bool is_text = t & 1u;
        const uint64_t u = t >> 1;
        const uint32_t pair = todo[16 + (uint32_t)(u / per_row)], piece = (uint32_t)(u % per_row);
        const aim_request_t rq = load_request(a, pair);
        uint32_t w[2];
        if (is_text) {
            ref_piece<2>(ref, ref_len, text_pos[pair], rq.text_len, (int)piece * 8, w);
        } else {
            const uint32_t bits = reinterpret_cast<const uint16_t *>(packedP + (uint64_t)pair * packed_row_dwords(rs))[piece];
            const uint32_t lo = (bits & 3u) | ((bits & 0xCu) << 6) | ((bits & 0x30u) << 12) | ((bits & 0xC0u) << 18);
            const uint32_t hb = bits >> 8;
            const uint32_t hi = (hb & 3u) | ((hb & 0xCu) << 6) | ((hb & 0x30u) << 12) | ((hb & 0xC0u) << 18);
            w[0] = __builtin_amdgcn_perm(0u, 0x47544341u, lo);
            w[1] = __builtin_amdgcn_perm(0u, 0x47544341u, hi);
            const int rem = rq.pattern_len - (int)piece * 8;
            if (rem < 8) {
                const uint64_t keep = rem <= 0 ? 0ull : ((1ull << (8 * rem)) - 1ull);
                w[0] &= (uint32_t)keep;
                w[1] &= (uint32_t)(keep >> 32);
            }
        }
        reinterpret_cast<uint2 *>((is_text ? outT : outP) + (uint64_t)pair * rs)[piece] = make_uint2(w[0], w[1]);
    }
}

// ---- AIM_FLAG_WFA_ESCALATE: the second stage's work list --------------------------------------------------------------------
// The first stage ran the whole batch at a low cap c on a lane kernel; the pairs it left over the cap report c + 1. Their ids go, in
// ascending pair order, to a to-do list {count @0, pair ids @16..} that the full-cap plan drains. One pass over the results:
// escalate_select_kernel reads each score once and keeps one ballot mask per 64 pairs plus one count per workgroup (kEscTile pairs);
// escalate_list_kernel (same grid) turns masks and counts into list positions -- a workgroup's base is the sum of the counts before it --
// so the list does not depend on scheduling. Plain vector stores, no atomics. The masks and counts are read 1/64th of the results' bytes.
// (kEscTile, escalate_mask_bytes and escalate_count_bytes: batch_sizes.hpp, which the planner includes without these kernels)

// res: result_t rows (stride_dw 6, score_dw 3) or {idx, score} rows (2, 1)
__global__ __launch_bounds__(256) void escalate_select_kernel(const uint32_t *res, uint32_t n_pairs, uint32_t stride_dw, uint32_t score_dw, int32_t over,
                                                              uint2 *masks, uint32_t *counts)
{
    __shared__ uint32_t wave_n[4];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n_groups = (n_pairs + 63u) / 64u;
    const uint32_t g0 = blockIdx.x * (kEscTile / 64u) + wave * 16u;
    uint32_t mine = 0;
    for (uint32_t j = 0; j < 16u; ++j) {
        const uint32_t g = g0 + j;
        if (g >= n_groups) break;                            // (wave-uniform)
        const uint32_t pair = g * 64u + lane;
        const bool hit = pair < n_pairs && (int32_t)res[(uint64_t)pair * stride_dw + score_dw] == over;
        const unsigned long long m = __ballot(hit);
        mine += (uint32_t)__builtin_popcountll(m);
        if (lane == 0) masks[g] = make_uint2((uint32_t)m, (uint32_t)(m >> 32));
    }
    if (lane == 0) wave_n[wave] = mine;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
}

__global__ __launch_bounds__(256) void escalate_list_kernel(uint32_t n_pairs, const uint2 *masks, const uint32_t *counts, uint32_t *todo)
{
    __shared__ uint32_t part[4];
    __shared__ uint32_t goff[64];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t n_groups = (n_pairs + 63u) / 64u;
    // list positions before this workgroup: the counts of the workgroups before it
    // (every workgroup re-reads the counts before it: B^2 / 2 dwords over a grid of B = n / 4096 workgroups -- 2 MB at 4 Mi pairs, 32 MB at
    //  16 Mi, against the 32-128 MB of result rows the first kernel read; a batch is bounded by the device buffers long before this matters)
    uint32_t sum = 0;
    for (uint32_t b = threadIdx.x; b < blockIdx.x; b += 256u) sum += counts[b];
    for (int o = 32; o; o >>= 1) sum += __shfl_xor(sum, o);
    if (lane == 0) part[wave] = sum;
    // ... and before each of its 64 groups (wavefront 0: an exclusive scan of the groups' populations)
    const uint32_t gt = blockIdx.x * (kEscTile / 64u) + lane;
    uint32_t pop = 0;
    if (wave == 0 && gt < n_groups) { const uint2 m = masks[gt]; pop = (uint32_t)(__builtin_popcount(m.x) + __builtin_popcount(m.y)); }
    uint32_t incl = pop;
    for (int o = 1; o < 64; o <<= 1) { const uint32_t v = __shfl_up(incl, o); if ((int)lane >= o) incl += v; }
    if (wave == 0) goff[lane] = incl - pop;
    __syncthreads();
    const uint32_t base = part[0] + part[1] + part[2] + part[3];
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) todo[0] = base + counts[blockIdx.x];   // the list's count
    for (uint32_t j = 0; j < 16u; ++j) {
        const uint32_t gl = wave * 16u + j, g = blockIdx.x * (kEscTile / 64u) + gl;
        if (g >= n_groups) break;
        const uint2 mw = masks[g];
        const unsigned long long m = ((unsigned long long)mw.y << 32) | mw.x;
        if ((m >> lane) & 1ull) todo[16u + base + goff[gl] + (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull))] = g * 64u + lane;
    }
}

// ---- the launchers declared at the top ---------------------------------------------------------------------------------------
void unpack_rows_launch(const KArgs &ka, const uint32_t *packedP, const uint32_t *packedT, char *outP, char *outT, unsigned planes, hipStream_t s)
{
    const dim3 grid(blocks_256((uint64_t)ka.n_pairs * (uint64_t)(ka.p.read_size / 8)).x, planes);
    hipLaunchKernelGGL(unpack_rows_kernel, grid, dim3(256), 0, s, ka, packedP, packedT, outP, outT);
}

void scatter_raw_rows_launch(int read_size, uint32_t n_raw, const uint32_t *raw_pairs, const char *rawP, const char *rawT, char *outP, char *outT,
                             unsigned planes, hipStream_t s)
{
    const dim3 grid(blocks_256((uint64_t)n_raw * (uint64_t)(read_size / 8)).x, planes);
    hipLaunchKernelGGL(scatter_raw_rows_kernel, grid, dim3(256), 0, s, read_size, n_raw, raw_pairs, rawP, rawT, outP, outT);
}

void pack_rows_launch(const KArgs &ka, uint32_t *packedP, uint32_t *packedT, uint32_t *flag_bits, uint32_t *todo, hipStream_t s)
{
    const dim3 grid(blocks_256((uint64_t)ka.n_pairs * packed_row_dwords(ka.p.read_size)).x, 2);
    hipLaunchKernelGGL(pack_rows_kernel, grid, dim3(256), 0, s, ka, packedP, packedT, flag_bits, todo);
}

void gather_elems_launch(const uint32_t *src, const uint32_t *idx, uint32_t n, uint32_t dw, uint32_t *dst, hipStream_t s)
{
    hipLaunchKernelGGL(gather_elems_kernel, blocks_256((uint64_t)n * dw), dim3(256), 0, s, src, idx, n, dw, dst);
}

void scatter_elems_launch(const uint32_t *src, const uint32_t *idx, uint32_t n, uint32_t dw, uint32_t *dst, hipStream_t s)
{
    hipLaunchKernelGGL(scatter_elems_kernel, blocks_256((uint64_t)n * dw), dim3(256), 0, s, src, idx, n, dw, dst);
}

void cigar_rle_launch(const KArgs &ka, aim_cigar_t *hdr, uint32_t *runs, uint32_t runs_cap, uint32_t *cursor, hipStream_t s)
{
    hipLaunchKernelGGL(cigar_rle_kernel, dim3((ka.n_pairs + 63) / 64), dim3(64), 0, s, ka, hdr, runs, runs_cap, cursor);
}

void cigar_rle_todo_launch(const KArgs &ka, const uint32_t *todo, aim_cigar_t *hdr, uint32_t *runs, uint32_t runs_cap, uint32_t *cursor, hipStream_t s)
{
    hipLaunchKernelGGL(cigar_rle_todo_kernel, dim3(256), dim3(64), 0, s, ka, todo, hdr, runs, runs_cap, cursor);
}

void unpack_todo_rows_launch(const KArgs &ka, const uint32_t *todo, const uint32_t *packedP, const uint32_t *packedT, char *outP, char *outT, hipStream_t s)
{
    hipLaunchKernelGGL(unpack_todo_rows_kernel, dim3(256), dim3(256), 0, s, ka, todo, packedP, packedT, outP, outT);
}

void gather_text_rows_launch(const KArgs &ka, const uint64_t *text_pos, const char *ref, uint64_t ref_len, const uint32_t *idx, uint32_t n_rows, char *out,
                             hipStream_t s)
{
    if (!n_rows) return;
    const RowGather g = row_gather(ka.p.read_size, n_rows);
    if (g.nw == 4) hipLaunchKernelGGL(gather_text_rows_kernel<4>, g.grid, dim3(256), 0, s, ka, text_pos, ref, ref_len, idx, n_rows, out);
    else hipLaunchKernelGGL(gather_text_rows_kernel<2>, g.grid, dim3(256), 0, s, ka, text_pos, ref, ref_len, idx, n_rows, out);
}

void gather_text_packed_launch(const KArgs &ka, const uint64_t *text_pos, const char *ref, uint64_t ref_len, uint32_t *packedT, uint32_t *flag_bits,
                               uint32_t *todo, hipStream_t s)
{
    hipLaunchKernelGGL(gather_text_packed_kernel, blocks_256((uint64_t)ka.n_pairs * packed_row_dwords(ka.p.read_size)), dim3(256), 0, s, ka, text_pos, ref,
                       ref_len, packedT, flag_bits, todo);
}

void gather_todo_rows_launch(const KArgs &ka, const uint32_t *todo, const uint64_t *text_pos, const char *ref, uint64_t ref_len, const uint32_t *packedP,
                             char *outP, char *outT, hipStream_t s)
{
    hipLaunchKernelGGL(gather_todo_rows_kernel, dim3(256), dim3(256), 0, s, ka, todo, text_pos, ref, ref_len, packedP, outP, outT);
}

void escalate_list_launch(const uint32_t *res, uint32_t n_pairs, uint32_t stride_dw, uint32_t score_dw, int32_t over, uint2 *masks, uint32_t *counts,
                          uint32_t *todo, hipStream_t s)
{
    const dim3 grid((n_pairs + kEscTile - 1) / kEscTile);
    hipLaunchKernelGGL(escalate_select_kernel, grid, dim3(256), 0, s, res, n_pairs, stride_dw, score_dw, over, masks, counts);
    hipLaunchKernelGGL(escalate_list_kernel, grid, dim3(256), 0, s, n_pairs, masks, counts, todo);
}
#endif  // AIM_TU_BATCH_IO

}  // namespace aim
