// contig.hpp -- the device side of AIM_FEATURE_CONTIGS (aim_hip.h, rule 13c): every valid segment's window kept inside the contig its
// chain lies on, and that contig's number per slot.
//
// contig_clip_kernel runs behind split_segments_kernel (and the extension) on their buffers. A lane takes one slot r * K + i: it
// recovers rule 10c's p_lo from the candidate's own window -- the same arithmetic as split.hpp, kept here as a second copy so that
// split_segments_kernel's instructions stay what they were --, finds c = max{ j : starts[j] <= A } and clips [seg_start, seg_end) to
// [starts[c], starts[c] + lens[c]). Consecutive lanes read consecutive rows: dwordx2 loads of aim_segment_t, text_pos and the chain's
// last two fields, dword loads of the two text_len's.
//
// The lookup. Twenty dependent global loads per lane (n up to 2^20) would make the kernel: instead each workgroup stages the sampled
// table T[j] = starts[j * step], j < ceil(n / step) <= 1024, in 4 KB of LDS once (the rest filled with 0xFFFFFFFF, above every anchor),
// with step the smallest power of two that fits. A lane walks T in ten steps without a branch (a conditional add each), which leaves
// starts[t * step] <= A < starts[(t + 1) * step], and closes in on c with log2(step) loads of starts[] -- none at all up to 1 024
// contigs. Lanes of a wavefront mostly hit the same few entries: LDS broadcasts, and the global steps stay in one or two lines.
//
// Measured (profiles/contigs/README.md): 43 us for 1 Mi reads at K = 4 (0.28 of the 8 TB/s roofline in algorithmic bytes), the same at 1
// and 25 contigs; 138 us at 2^20 contigs with every slot clipped. What bounds it was not measured with counters.
//
// The kernel walks the slots with a grid-sized stride. No atomics, no scratch, vector stores only; an output byte has one writer and
// none depends on the grid.
#pragma once

#include "aim_device.hpp"

namespace aim {

constexpr int kContigMaxVgpr = 64;          // 8 wavefronts per SIMD; the bound tests/test_contigs_cpu.py checks in the code object
constexpr int kContigThreads = 256;
constexpr uint32_t kContigPerCu = 8;        // workgroups per compute unit of the resident grid: 32 wavefronts
constexpr uint32_t kContigTable = 1024;     // entries of the sampled table: 4 KB of LDS

struct ContigArgs {
    uint32_t K, read_size, n_slots, n_contigs, step_log2, dbg_poison_lds;
    int64_t flank, ref_len;
    const uint32_t *start, *len;            // [n_contigs]
    const int32_t *read_len;
    const aim_request_t *requests;
    const uint64_t *text_pos;
    const aim_chain_t *chains;
    aim_request_t *seg_requests;
    uint64_t *seg_text_pos;
    aim_segment_t *seg;
    uint32_t *contig;
};

// log2 of the smallest power of two `step` with ceil(n / step) <= kContigTable.
inline uint32_t contig_step_log2(uint32_t n)
{
    uint32_t lg = 0;
    while ((((uint64_t)n + (1ull << lg) - 1u) >> lg) > kContigTable) ++lg;
    return lg;
}

#ifdef AIM_TU_CONTIG   // the kernel lives in tu_contig.hip alone; capi_mapper.hip sees the arguments and the launcher

static_assert(sizeof(aim_segment_t) == 8 && sizeof(aim_request_t) == 16 && sizeof(aim_chain_t) == 16, "rows as rule 10c lays them out");

__global__ __launch_bounds__(kContigThreads) void contig_clip_kernel(ContigArgs a)
{
    __shared__ uint32_t table[kContigTable];
    if (a.dbg_poison_lds) {                                       // debugging aid: nothing may depend on what LDS held before
        for (uint32_t j = threadIdx.x; j < kContigTable; j += kContigThreads) table[j] = (a.dbg_poison_lds & 0xffu) * 0x01010101u;
        __syncthreads();
    }
    for (uint32_t j = threadIdx.x; j < kContigTable; j += kContigThreads) {
        const uint64_t at = (uint64_t)j << a.step_log2;
        table[j] = at < a.n_contigs ? a.start[at] : 0xFFFFFFFFu;
    }
    __syncthreads();
    const uint32_t n_blocks = (uint32_t)(((uint64_t)a.n_slots + kContigThreads - 1u) / kContigThreads);
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t slot64 = (uint64_t)blk * kContigThreads + threadIdx.x;
        if (slot64 >= a.n_slots) continue;                        // (no barrier and no cross-lane step below)
        const uint32_t slot = (uint32_t)slot64;
        const uint2 sg = reinterpret_cast<const uint2 *>(a.seg)[slot];
        const uint32_t flags = (sg.y >> 16) & 0xffu;
        uint32_t c = AIM_CONTIG_NONE;
        if (flags & AIM_SEG_VALID) {
            const uint64_t stp = a.seg_text_pos[slot];
            const int64_t seg_start = (int64_t)(stp & ~AIM_REF_MINUS_STRAND);
            const int64_t seg_end = seg_start + (int64_t)a.seg_requests[slot].text_len;
            // ---- the anchor: rule 10c's p_lo of the candidate's window ----
            const int64_t start = (int64_t)(a.text_pos[slot] & ~AIM_REF_MINUS_STRAND);
            const int32_t text_len = a.requests[slot].text_len;
            const uint2 ch = reinterpret_cast<const uint2 *>(a.chains)[2u * (uint64_t)slot + 1u];   // q_lo | q_hi << 16, ref_span
            const int64_t q_lo = ch.x & 0xffffu, q_hi = ch.x >> 16, span = ch.y;
            const int64_t L = min(max(a.read_len[slot / a.K], 0), (int32_t)a.read_size);
            const int64_t E = start + (int64_t)text_len;
            int64_t A = seg_start;
            if (!(flags & AIM_SEG_LOOSE)) {
                if (start > 0) A = start + q_lo + a.flank;
                else if (text_len > 0 && text_len < (int32_t)a.read_size && E < a.ref_len) A = E - (L - q_hi) - a.flank - span;
            }
            A = min(max(A, (int64_t)0), a.ref_len - 1);
            const uint32_t key = (uint32_t)A;                     // (ref_len fits 32 bits)
            // ---- the contig: ten steps in LDS, then log2(step) in memory ----
            uint32_t t = 0;
#pragma unroll
            for (uint32_t b = kContigTable / 2u; b; b >>= 1) t += table[t + b] <= key ? b : 0u;
            c = t << a.step_log2;
            for (uint32_t b = (1u << a.step_log2) >> 1; b; b >>= 1) {
                const uint32_t j = c + b;
                if (j < a.n_contigs && a.start[j] <= key) c = j;
            }
            const int64_t c_lo = a.start[c], c_hi = c_lo + (int64_t)a.len[c];
            const int64_t s2 = max(seg_start, c_lo);
            const int64_t e2 = max(s2, min(seg_end, c_hi));
            if (s2 != seg_start || e2 != seg_end) {
                a.seg_text_pos[slot] = (uint64_t)s2 | (stp & AIM_REF_MINUS_STRAND);
                a.seg_requests[slot].text_len = (int32_t)(e2 - s2);
                reinterpret_cast<uint32_t *>(a.seg)[2u * (uint64_t)slot + 1u] = sg.y | (AIM_SEG_CONTIG_CLIPPED << 16);
            }
        }
        a.contig[slot] = c;
    }
}

void contig_clip_launch(const ContigArgs &a, uint32_t grid, hipStream_t s)
{
    hipLaunchKernelGGL(contig_clip_kernel, dim3(grid), dim3(kContigThreads), 0, s, a);
}
#else
void contig_clip_launch(const ContigArgs &a, uint32_t grid, hipStream_t s);
#endif

}  // namespace aim
