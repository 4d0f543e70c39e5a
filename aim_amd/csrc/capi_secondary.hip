// capi_secondary.hip -- the stateless entry points of rule 16c (include/aim_hip.h, AIM_FEATURE_SECONDARY): aim_secondary_rows_device,
// aim_secondary_select_device and aim_map_records_secondary_device (kernels in secondary.hpp, the prefix sums by index.hpp's scan).
// The mapper's side -- aim_mapper_set_secondary, aim_mapper_secondary -- lives with aim_mapper_t in capi_mapper.hip.
// Host code only. What this unit shares with the others is in capi_common.hpp.
#include <algorithm>
#include <climits>
#include <cstdio>
#include <cstring>

#include "capi_common.hpp"
#include "index.hpp"
#include "secondary.hpp"

using namespace aim::capi;

extern "C" {

const char *aim_secondary_kernel_names(void) { return "secondary_rows_kernel,secondary_select_kernel,map_count_sec_kernel,map_records_sec_kernel"; }

int aim_secondary_rows_device(uint32_t K, uint32_t read_size, int32_t flank, uint64_t ref_len, uint32_t n_reads, const int32_t *d_read_len, const char *d_reads,
                              const void *d_requests, const uint64_t *d_text_pos, const aim_seed_t *d_seed, const aim_chain_t *d_chains,
                              const aim_chain_class_t *d_class, void *d_seg_requests, uint64_t *d_seg_text_pos, char *d_seg_patterns, aim_segment_t *d_seg,
                              uint32_t max_sec, void *hip_stream)
{
    const char *fn = "aim_secondary_rows_device";
    if (!(cands_ok(fn, K) && read_size_ok(fn, read_size) && slots_ok(fn, n_reads, K) && (flank >= 0 || refuse("%s: flank %d must be >= 0", fn, flank)) &&
          ref_len_ok(fn, ref_len, false) && ((max_sec >= 1 && max_sec <= AIM_SEC_MAX) || refuse("%s: max_sec %u is outside 1..%u", fn, max_sec, AIM_SEC_MAX)) &&
          buffers_ok(fn, n_reads, d_read_len && d_reads && d_requests && d_text_pos && d_seed && d_chains && d_class && d_seg_requests && d_seg_text_pos && d_seg_patterns && d_seg)))
        return AIM_EINVAL;
    return launch_batch(n_reads, [&](const aim::Knobs &kn) {
        aim::SecRowsArgs a;
        memset(&a, 0, sizeof a);
        // lanes per read and shares per row come from K and read_size alone; only the grid is the device's
        const uint32_t lanes = aim::chain_class_lanes(K);
        a.K = K; a.read_size = read_size; a.n_reads = n_reads; a.parts_log2 = aim::sec_parts_log2(lanes, read_size); a.max_sec = max_sec;
        a.flank = flank; a.ref_len = (int64_t)ref_len;
        a.read_len = d_read_len; a.reads = d_reads; a.requests = static_cast<const aim_request_t *>(d_requests); a.text_pos = d_text_pos;
        a.seed = d_seed; a.chains = d_chains; a.cls = d_class;
        a.seg_requests = static_cast<aim_request_t *>(d_seg_requests); a.seg_text_pos = d_seg_text_pos; a.seg_patterns = d_seg_patterns; a.seg = d_seg;
        const uint32_t per_block = aim::kSecThreads / lanes;
        const uint64_t items = (uint64_t)n_reads << a.parts_log2;
        const uint32_t grid = (uint32_t)std::min<uint64_t>(aim::resident_grid(kn, aim::kSecPerCu), (items + per_block - 1u) / per_block);
        if (kn.plan_debug)
            fprintf(stderr, "[aim plan] secondary_rows_kernel grid=%u block=%d lanes=%u parts=%u reads=%u K=%u read_size=%u max_sec=%u\n", grid, aim::kSecThreads,
                    lanes, 1u << a.parts_log2, n_reads, K, read_size, max_sec);
        aim::secondary_rows_launch(a, lanes, grid, (hipStream_t)hip_stream);
    });
}

int aim_secondary_select_device(uint32_t K, uint32_t n_reads, const aim_segment_t *d_seg, const aim_sam_t *d_sam, const aim_chain_class_t *d_class,
                                const aim_chain_t *d_chains, int32_t max_score, int32_t score_unit, aim_sec_slot_t *d_sec, void *hip_stream)
{
    const char *fn = "aim_secondary_select_device";
    if (!(cands_ok(fn, K) && slots_ok(fn, n_reads, K) &&
          ((max_score >= 0 && max_score < INT_MAX) || refuse("%s: max_score %d is outside 0..%d", fn, max_score, INT_MAX - 1)) &&
          (score_unit >= 1 || refuse("%s: score_unit %d must be >= 1", fn, score_unit)) && buffers_ok(fn, n_reads, d_seg && d_sam && d_class && d_chains && d_sec)))
        return AIM_EINVAL;
    return launch_batch(n_reads, [&](const aim::Knobs &kn) {
        const aim::SecSelectArgs a = {K, n_reads, max_score, score_unit, d_seg, d_sam, d_class, d_chains, d_sec};
        const uint32_t lanes = aim::chain_class_lanes(K), per_block = aim::kSecThreads / lanes;
        const uint32_t grid = (uint32_t)std::min<uint64_t>(aim::resident_grid(kn, aim::kSecPerCu), ((uint64_t)n_reads + per_block - 1u) / per_block);
        if (kn.plan_debug)
            fprintf(stderr, "[aim plan] secondary_select_kernel grid=%u block=%d lanes=%u reads=%u K=%u\n", grid, aim::kSecThreads, lanes, n_reads, K);
        aim::secondary_select_launch(a, lanes, grid, (hipStream_t)hip_stream);
    });
}

int aim_map_records_secondary_device(uint32_t K, uint32_t n_reads, uint32_t options, const aim_segment_t *d_seg, const aim_sam_t *d_sam,
                                     const aim_chain_class_t *d_class, const aim_sec_slot_t *d_sec, const uint32_t *d_contig, uint32_t n_contigs,
                                     const uint32_t *d_contig_start, uint32_t *d_rec_offsets, aim_map_record_t *d_records, aim_map_sec_t *d_sec_records,
                                     void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
    const char *fn = "aim_map_records_secondary_device";
    const size_t need = aim_map_records_scratch(n_reads);
    if (!(cands_ok(fn, K) && slots_ok(fn, n_reads, K) && (d_rec_offsets || refuse("%s: d_rec_offsets is NULL", fn)) &&
          (!(options & ~AIM_SEC_RECORDS) || refuse("%s: unknown options 0x%x", fn, options)) &&
          (!d_contig || (n_contigs >= 1 && n_contigs <= AIM_CONTIG_MAX) || refuse("%s: n_contigs %u is outside 1..%u", fn, n_contigs, AIM_CONTIG_MAX)) &&
          (!d_contig || d_contig_start || refuse("%s: d_contig_start is NULL", fn)) &&
          buffers_ok(fn, n_reads, d_seg && d_sam && d_class && d_sec && d_records && d_sec_records && d_scratch) &&
          (!(((uintptr_t)d_sam | (uintptr_t)d_records | (uintptr_t)d_sec_records) & 15u) || refuse("%s: d_sam, d_records and d_sec_records must be 16-byte aligned", fn)) &&
          (!n_reads || scratch_bytes >= need || refuse("%s: scratch_bytes %zu is below the %zu aim_map_records_scratch reports", fn, scratch_bytes, need))))
        return AIM_EINVAL;
    hipStream_t stream = (hipStream_t)hip_stream;
    int n_dev = 0;
    if (const int rc = aim_device_count(&n_dev)) return rc;
    if (!n_reads) {
        HIP_TRY(hipMemsetAsync(d_rec_offsets, 0, 4, stream));
        return AIM_OK;
    }
    const aim::Knobs kn = with_chip(read_knobs());
    // Debugging aid, as in aim_map_records_device: results must not depend on what the scratch held before.
    if (kn.poison_scratch >= 0) HIP_TRY(hipMemsetAsync(d_scratch, kn.poison_scratch & 0xff, need, stream));
    const aim::MapSecArgs a = {K, n_reads, options, d_contig ? n_contigs : 0u, d_seg, d_sam, d_class, d_sec, d_contig, d_contig_start, d_rec_offsets, d_records, d_sec_records};
    const uint32_t lanes = aim::chain_class_lanes(K), per_block = aim::kSecThreads / lanes;
    const uint32_t resident = aim::resident_grid(kn, aim::kSecPerCu);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(resident, ((uint64_t)n_reads + per_block - 1u) / per_block);
    aim::IndexScanArgs s;
    memset(&s, 0, sizeof s);
    s.data = d_rec_offsets; s.n = (uint64_t)n_reads + 1u; s.dbg_poison_lds = poison_lds_word(kn); s.part = static_cast<uint32_t *>(d_scratch);
    s.n_parts = (uint32_t)std::min<uint64_t>(std::min(resident, aim::kIndexScanParts), (s.n + aim::kIndexScanBlock - 1u) / aim::kIndexScanBlock);
    s.per_part = ((s.n + s.n_parts - 1u) / s.n_parts + aim::kIndexScanBlock - 1u) / aim::kIndexScanBlock * aim::kIndexScanBlock;
    if (kn.plan_debug)
        fprintf(stderr, "[aim plan] map_count_sec_kernel grid=%u block=%d lanes=%u reads=%u K=%u options=0x%x contigs=%u; scan parts=%u per_part=%llu; map_records_sec_kernel grid=%u block=%d\n",
                grid, aim::kSecThreads, lanes, n_reads, K, options, a.n_contigs, s.n_parts, (unsigned long long)s.per_part, grid, aim::kSecThreads);
    aim::map_count_sec_launch(a, lanes, grid, stream);
    HIP_TRY(hipGetLastError());
    aim::index_launch_scan(s, stream);
    HIP_TRY(hipGetLastError());
    aim::map_records_sec_launch(a, lanes, grid, stream);
    HIP_TRY(hipGetLastError());
    return AIM_OK;
}

}  // extern "C"
