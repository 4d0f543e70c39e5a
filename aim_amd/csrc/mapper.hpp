// mapper.hpp -- the device side of AIM_FEATURE_MAPPER (aim_hip.h, rule 12c): the slot-shaped outputs of the split path (aim_segment_t,
// aim_sam_t and aim_chain_class_t per slot r * K + i) turned into a dense list of records per read, with the chain MAPQ inside the record.
//
//   * map_count_kernel: per read, c_r = the number of its mapped slots, or 1 when it has none -> rec_offsets[r]; rec_offsets[n_reads] = 0.
//   * index_launch_scan (index.hpp; three launches) turns rec_offsets[0, n_reads] into its exclusive prefix sums in place, so that
//     rec_offsets[n_reads] is the number of records.
//   * map_records_kernel: per read, the mapped slots again, their rank by (q_begin, i) and the representative, and each record written
//     at rec_offsets[r] + rank as four 16-byte stores.
//   * map_records_contig_kernel (rule 13c) takes its place for a reference of several sequences: the slot's contig in the record.
//
// Both kernels give a read G = 4, 8 or 16 consecutive lanes by K, as chain_class_kernel does (chain_class_lanes), with candidate i in
// lane i of the group; the group's bits of one wave ballot are the read's mapped slots, their population count is c_r, the lowest set
// bit the representative, and K ballots of "my key is below candidate j's" give every candidate its rank. A group never leaves a
// 16-lane row. Slots r * K + i are consecutive across a group and across the groups of a wavefront.
//
// Where a record lands depends on the prefix sums alone: every dependency between workgroups is a kernel boundary, no workgroup waits
// for another, no atomic is involved, and the kernels use no LDS and no scratch memory (the scan keeps its own few dwords of LDS).
// Both walk the batch with a grid-sized stride.
#pragma once

#include "aim_device.hpp"
#include "chain_class.hpp"

namespace aim {

constexpr int kMapMaxVgpr = 64;          // 8 wavefronts per SIMD; the bound tests/test_mapper_cpu.py checks in the code object
constexpr int kMapThreads = 256;
constexpr uint32_t kMapPerCu = 8;        // workgroups per compute unit of the resident grid: 32 wavefronts

struct MapArgs {
    uint32_t K, n_reads;
    const aim_segment_t *seg;
    const aim_sam_t *sam;
    const aim_chain_class_t *cls;
    uint32_t *rec_offsets;               // [n_reads + 1]: counts after map_count_kernel, offsets after the scan
    aim_map_record_t *records;
};

#ifdef AIM_TU_MAPPER   // the kernels live in tu_mapper.hip alone; capi_mapper.hip sees the arguments and the launchers

static_assert(sizeof(aim_sam_t) == 48 && sizeof(aim_map_record_t) == 64 && sizeof(aim_segment_t) == 8 && sizeof(aim_chain_class_t) == 8,
              "rows of 12, 16, 2 and 2 dwords");

// What rule 12c reads of a slot, and the read's mapped slots as the group's bits of one ballot.
struct MapSlot {
    uint32_t seg0, seg1;                 // aim_segment_t as its two dwords: q_begin | q_end << 16, read_len | flags << 16 | cand << 24
    uint32_t fs;                         // aim_sam_t's dword 10: flags | status << 16
    uint32_t mask;                       // bit i: candidate i of the read is mapped
};

__device__ __forceinline__ MapSlot map_slot(const MapArgs &a, bool live, uint64_t slot, uint32_t base, uint32_t G)
{
    MapSlot s = {0u, 0u, 0u, 0u};
    if (live) {
        const uint2 sg = reinterpret_cast<const uint2 *>(a.seg)[slot];
        s.seg0 = sg.x;
        s.seg1 = sg.y;
        s.fs = reinterpret_cast<const uint32_t *>(a.sam)[slot * 12u + 10u];
    }
    const bool mapped = live && ((s.seg1 >> 16) & AIM_SEG_VALID) && !(s.fs & AIM_SAM_UNMAPPED);
    s.mask = (uint32_t)(__ballot(mapped) >> base) & ((1u << G) - 1u);
    return s;
}

// G: lanes per read, 4, 8 or 16 and at least K (workgroup-uniform, like every loop bound below: every lane takes every ballot).
__global__ __launch_bounds__(kMapThreads) void map_count_kernel(MapArgs a, uint32_t G)
{
    const uint32_t kReads = kMapThreads / G;
    const uint32_t cand = threadIdx.x & (G - 1u);
    const uint32_t base = (threadIdx.x & (uint32_t)(kWave - 1)) & ~(G - 1u);
    const uint64_t n_blocks = ((uint64_t)a.n_reads + kReads - 1u) / kReads;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.rec_offsets[a.n_reads] = 0u;     // the scan's last entry: the total lands here
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t r = blk * kReads + threadIdx.x / G;
        const bool live = r < a.n_reads && cand < a.K;
        const MapSlot s = map_slot(a, live, r * a.K + cand, base, G);
        if (r < a.n_reads && cand == 0) a.rec_offsets[r] = s.mask ? (uint32_t)__popc(s.mask) : 1u;
    }
}

__global__ __launch_bounds__(kMapThreads) void map_records_kernel(MapArgs a, uint32_t G)
{
    const uint32_t kReads = kMapThreads / G;
    const uint32_t cand = threadIdx.x & (G - 1u);
    const uint32_t base = (threadIdx.x & (uint32_t)(kWave - 1)) & ~(G - 1u);
    const uint64_t n_blocks = ((uint64_t)a.n_reads + kReads - 1u) / kReads;
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t r = blk * kReads + threadIdx.x / G;
        const bool live = r < a.n_reads && cand < a.K;
        const uint64_t slot = r * a.K + cand;
        const MapSlot s = map_slot(a, live, slot, base, G);
        const bool mapped = (s.mask >> cand) & 1u;
        const uint32_t q = s.seg0 & 0xffffu;
        uint32_t rank = 0;
        for (uint32_t j = 0; j < a.K; ++j) {                                  // rank of candidate j: the mapped keys (q_begin, i) below its own
            const uint32_t q_j = (uint32_t)__shfl((int)q, (int)j, (int)G);
            const bool below = mapped && (q < q_j || (q == q_j && cand < j));
            const uint32_t bits = (uint32_t)(__ballot(below) >> base) & ((1u << G) - 1u);
            if (cand == j) rank = (uint32_t)__popc(bits);
        }
        const bool unmapped_read = live && cand == 0 && !s.mask;              // its one record comes from candidate 0's row
        if (mapped || unmapped_read) {                                        // (an if, not a continue: every lane reaches the next round's ballots)
            const uint4 *row = reinterpret_cast<const uint4 *>(a.sam) + slot * 3u;
            uint4 w0 = row[0], w1 = row[1], w2 = row[2], w3;
            if (mapped) {
                const uint32_t rep = (uint32_t)__ffs(s.mask) - 1u;                      // the mapped slot of lowest i: the one non-supplementary line
                const uint32_t flags = cand == rep ? (s.fs & ~AIM_SAM_SUPPLEMENTARY) : (s.fs | AIM_SAM_SUPPLEMENTARY);
                const uint32_t c1 = reinterpret_cast<const uint32_t *>(a.cls)[slot * 2u + 1u];
                w2.z = flags;
                w3.x = (uint32_t)r;
                w3.y = s.seg0;
                w3.z = ((c1 >> 16) & 0xffu) | ((s.seg1 >> 16) & 0xffu) << 8 | rank << 16 | (uint32_t)__popc(s.mask) << 24;
            } else {
                w0.z = w0.w = 0u;                                                       // pos
                w1 = make_uint4(0u, 0u, 0u, 0u);                                        // ref_span, nm, cigar_offset, n_cigar
                w2.x = w2.y = 0u;                                                       // md_offset, md_len
                w2.z = AIM_SAM_UNMAPPED | (s.fs & 0xffff0000u);                         // status is kept
                w3.x = (uint32_t)r;
                w3.y = 0u;
                w3.z = 1u << 24;
            }
            w3.w = (uint32_t)slot;                                                      // (n_reads * K fits 32 bits)
            uint4 *out = reinterpret_cast<uint4 *>(a.records) + ((uint64_t)a.rec_offsets[r] + (mapped ? rank : 0u)) * 4u;
            out[0] = w0;
            out[1] = w1;
            out[2] = w2;
            out[3] = w3;
        }
    }
}

// Rule 13c's record kernel: map_records_kernel once more, with the slot's contig in the record -- a mapped record's pos becomes local to
// contig[slot] and its pad names it, the record of an unmapped read gets AIM_CONTIG_NONE. It is a copy, not a template over one body:
// a shared body, force-inlined into both, compiled map_records_kernel to other instructions (349 against its 357, the same 38 VGPRs),
// and that kernel keeps its instructions. What the two share beyond map_slot is the text between the marks; a change to one belongs in the other.
__global__ __launch_bounds__(kMapThreads) void map_records_contig_kernel(MapArgs a, uint32_t G, const uint32_t *contig, uint32_t n_contigs, const uint32_t *contig_start)
{
    // ---- as map_records_kernel ----
    const uint32_t kReads = kMapThreads / G;
    const uint32_t cand = threadIdx.x & (G - 1u);
    const uint32_t base = (threadIdx.x & (uint32_t)(kWave - 1)) & ~(G - 1u);
    const uint64_t n_blocks = ((uint64_t)a.n_reads + kReads - 1u) / kReads;
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t r = blk * kReads + threadIdx.x / G;
        const bool live = r < a.n_reads && cand < a.K;
        const uint64_t slot = r * a.K + cand;
        const MapSlot s = map_slot(a, live, slot, base, G);
        const bool mapped = (s.mask >> cand) & 1u;
        const uint32_t q = s.seg0 & 0xffffu;
        uint32_t rank = 0;
        for (uint32_t j = 0; j < a.K; ++j) {
            const uint32_t q_j = (uint32_t)__shfl((int)q, (int)j, (int)G);
            const bool below = mapped && (q < q_j || (q == q_j && cand < j));
            const uint32_t bits = (uint32_t)(__ballot(below) >> base) & ((1u << G) - 1u);
            if (cand == j) rank = (uint32_t)__popc(bits);
        }
        const bool unmapped_read = live && cand == 0 && !s.mask;
        if (mapped || unmapped_read) {
            const uint4 *row = reinterpret_cast<const uint4 *>(a.sam) + slot * 3u;
            uint4 w0 = row[0], w1 = row[1], w2 = row[2], w3;
            if (mapped) {
                const uint32_t rep = (uint32_t)__ffs(s.mask) - 1u;
                const uint32_t flags = cand == rep ? (s.fs & ~AIM_SAM_SUPPLEMENTARY) : (s.fs | AIM_SAM_SUPPLEMENTARY);
                const uint32_t c1 = reinterpret_cast<const uint32_t *>(a.cls)[slot * 2u + 1u];
                w2.z = flags;
                w3.x = (uint32_t)r;
                w3.y = s.seg0;
                w3.z = ((c1 >> 16) & 0xffu) | ((s.seg1 >> 16) & 0xffu) << 8 | rank << 16 | (uint32_t)__popc(s.mask) << 24;
                // ---- rule 13c: the contig-local position and the contig ----
                const uint32_t c = contig[slot];
                const uint64_t pos = ((uint64_t)w0.w << 32 | w0.z) - (c < n_contigs ? contig_start[c] : 0u);   // (no load outside the table)
                w0.z = (uint32_t)pos;
                w0.w = (uint32_t)(pos >> 32);
                w2.w = c;                                                               // pad
                // ---- as map_records_kernel ----
            } else {
                w0.z = w0.w = 0u;
                w1 = make_uint4(0u, 0u, 0u, 0u);
                w2.x = w2.y = 0u;
                w2.z = AIM_SAM_UNMAPPED | (s.fs & 0xffff0000u);
                w2.w = AIM_CONTIG_NONE;                                                 // rule 13c: pad of an unmapped read
                w3.x = (uint32_t)r;
                w3.y = 0u;
                w3.z = 1u << 24;
            }
            w3.w = (uint32_t)slot;
            uint4 *out = reinterpret_cast<uint4 *>(a.records) + ((uint64_t)a.rec_offsets[r] + (mapped ? rank : 0u)) * 4u;
            out[0] = w0;
            out[1] = w1;
            out[2] = w2;
            out[3] = w3;
        }
    }
}

void map_records_contig_launch(const MapArgs &a, uint32_t lanes, uint32_t grid, const uint32_t *contig, uint32_t n_contigs, const uint32_t *contig_start, hipStream_t s)
{
    hipLaunchKernelGGL(map_records_contig_kernel, dim3(grid), dim3(kMapThreads), 0, s, a, lanes, contig, n_contigs, contig_start);
}

void map_count_launch(const MapArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s)
{
    hipLaunchKernelGGL(map_count_kernel, dim3(grid), dim3(kMapThreads), 0, s, a, lanes);
}

void map_records_launch(const MapArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s)
{
    hipLaunchKernelGGL(map_records_kernel, dim3(grid), dim3(kMapThreads), 0, s, a, lanes);
}
#else
void map_records_contig_launch(const MapArgs &a, uint32_t lanes, uint32_t grid, const uint32_t *contig, uint32_t n_contigs, const uint32_t *contig_start, hipStream_t s);
void map_count_launch(const MapArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s);
void map_records_launch(const MapArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s);
#endif

}  // namespace aim
