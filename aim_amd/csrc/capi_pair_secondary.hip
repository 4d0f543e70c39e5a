// capi_pair_secondary.hip -- the stateless entry points of rule 17c (include/aim_hip.h, AIM_FEATURE_PAIR_SECONDARY):
// aim_pair_rescue_rows_secondary_device, aim_pair_select_secondary_device (apply included) and aim_map_mates_secondary_device, with the
// kernels in pair_secondary.hpp. They refuse what their rule-14c counterparts refuse (check_pair_params, capi_pair.hip), then what is
// their own. Host code only. What this unit shares with the others is in capi_common.hpp.
#include <cstdio>
#include <cstring>

#include "capi_common.hpp"
#include "pair_secondary.hpp"

using namespace aim::capi;

namespace {

// d_est may be NULL: the bounds are pp's then
bool est_ok(const char *fn, const aim_pair_estimate_t *d_est) { return aligned_ok(fn, d_est, 16, "d_est"); }

}  // namespace

extern "C" {

const char *aim_pair_secondary_kernel_names(void) { return "pair_sec_rescue_rows_kernel,pair_sec_select_kernel,map_mates_sec_kernel"; }

int aim_pair_rescue_rows_secondary_device(const aim_map_pair_params_t *pp, uint32_t K, uint32_t read_size, uint64_t ref_len, uint32_t n_contigs,
                                          const uint32_t *d_contig_start, const uint32_t *d_contig_len, uint32_t n_reads, const int32_t *d_read_len,
                                          const char *d_reads, const aim_segment_t *d_seg, const aim_sam_t *d_sam, const uint32_t *d_contig,
                                          const aim_sec_slot_t *d_sec, void *d_res_requests, uint64_t *d_res_text_pos, char *d_res_patterns,
                                          const aim_pair_estimate_t *d_est, void *hip_stream)
{
    const char *fn = "aim_pair_rescue_rows_secondary_device";
    if (const int rc = check_pair_params(fn, pp, K, read_size, n_reads, true)) return rc;
    if (!((ref_len >= 1 || refuse("%s: ref_len must be >= 1", fn)) && ref_len_ok(fn, ref_len, false) &&
          contigs_ok(fn, d_contig != nullptr, n_contigs, d_contig_start && d_contig_len) &&
          buffers_ok(fn, n_reads, d_read_len && d_reads && d_seg && d_sam && d_sec && d_res_requests && d_res_text_pos && d_res_patterns) &&
          aligned_ok(fn, d_sam, 16, "d_sam") && aligned_ok(fn, d_res_requests, 16, "d_res_requests") && aligned_ok(fn, d_reads, 8, "d_reads") &&
          aligned_ok(fn, d_res_patterns, 8, "d_res_patterns") && aligned_ok(fn, d_seg, 8, "d_seg") && aligned_ok(fn, d_res_text_pos, 8, "d_res_text_pos") &&
          aligned_ok(fn, d_sec, 8, "d_sec") && est_ok(fn, d_est)))
        return AIM_EINVAL;
    return launch_batch(n_reads, [&](const aim::Knobs &kn) {
        aim::PairSecArgs s;
        memset(&s, 0, sizeof s);
        aim::PairArgs &a = s.p;
        a.K = K; a.n_reads = n_reads; a.read_size = read_size; a.rescue_size = pp->rescue_size; a.options = pp->options; a.n_contigs = d_contig ? n_contigs : 0u;
        a.min_span = pp->min_span; a.max_span = pp->max_span; a.ref_len = (int64_t)ref_len;
        a.read_len = d_read_len; a.reads = d_reads;
        a.seg = const_cast<aim_segment_t *>(d_seg); a.sam = const_cast<aim_sam_t *>(d_sam); a.contig = const_cast<uint32_t *>(d_contig);   // (read only here)
        a.contig_start = d_contig_start; a.contig_len = d_contig_len;
        a.res_req = static_cast<aim_request_t *>(d_res_requests); a.res_text_pos = d_res_text_pos; a.res_patterns = d_res_patterns;
        s.sec = const_cast<aim_sec_slot_t *>(d_sec); s.est = d_est;
        const uint32_t lanes = aim::chain_class_lanes(K), grid = aim::pair_grid(kn, n_reads / 2u, aim::kPairThreads / lanes);
        if (kn.plan_debug)
            fprintf(stderr, "[aim plan] pair_sec_rescue_rows_kernel grid=%u block=%d lanes=%u reads=%u K=%u rescue_size=%u est=%d\n", grid, aim::kPairThreads, lanes,
                    n_reads, K, pp->rescue_size, d_est != nullptr);
        aim::pair_sec_rescue_rows_launch(s, lanes, grid, (hipStream_t)hip_stream);
    });
}

int aim_pair_select_secondary_device(const aim_map_pair_params_t *pp, uint32_t K, uint32_t read_size, uint32_t n_reads, const int32_t *d_read_len,
                                     aim_segment_t *d_seg, aim_sam_t *d_sam, aim_chain_class_t *d_class, uint32_t *d_contig, aim_sec_slot_t *d_sec,
                                     const aim_chain_t *d_chains, int32_t score_unit, const aim_sam_t *d_res_sam, uint32_t cigar_base, uint32_t md_base,
                                     aim_map_pair_t *d_pairs, aim_map_pair_mapq_t *d_pair_mapq, const aim_pair_estimate_t *d_est, void *hip_stream)
{
    const char *fn = "aim_pair_select_secondary_device";
    if (const int rc = check_pair_params(fn, pp, K, read_size, n_reads, false)) return rc;
    if (!((score_unit >= 1 || refuse("%s: score_unit %d must be >= 1", fn, score_unit)) &&
          buffers_ok(fn, n_reads, d_read_len && d_seg && d_sam && d_class && d_sec && d_chains && d_pairs && d_pair_mapq && (d_res_sam || !(pp->options & AIM_PAIR_RESCUE))) &&
          aligned_ok(fn, d_sam, 16, "d_sam") && aligned_ok(fn, d_res_sam, 16, "d_res_sam") && aligned_ok(fn, d_pairs, 16, "d_pairs") &&
          aligned_ok(fn, d_pair_mapq, 16, "d_pair_mapq") && aligned_ok(fn, d_seg, 8, "d_seg") && aligned_ok(fn, d_class, 8, "d_class") &&
          aligned_ok(fn, d_sec, 8, "d_sec") && aligned_ok(fn, d_chains, 8, "d_chains") && est_ok(fn, d_est)))
        return AIM_EINVAL;
    return launch_batch(n_reads, [&](const aim::Knobs &kn) {
        aim::PairSecArgs s;
        memset(&s, 0, sizeof s);
        aim::PairArgs &a = s.p;
        a.K = K; a.n_reads = n_reads; a.read_size = read_size; a.rescue_size = pp->rescue_size; a.options = pp->options;
        a.unpaired_penalty = pp->unpaired_penalty; a.cigar_base = cigar_base; a.md_base = md_base;
        a.min_span = pp->min_span; a.max_span = pp->max_span;
        a.read_len = d_read_len; a.seg = d_seg; a.sam = d_sam; a.cls = d_class; a.contig = d_contig; a.res_sam = d_res_sam; a.pairs = d_pairs;
        s.score_unit = score_unit; s.sec = d_sec; s.chains = d_chains; s.est = d_est; s.pair_mapq = d_pair_mapq;
        const uint32_t lanes = aim::chain_class_lanes(K), grid = aim::pair_grid(kn, n_reads / 2u, aim::kPairThreads / lanes);
        if (kn.plan_debug)
            fprintf(stderr, "[aim plan] pair_sec_select_kernel grid=%u block=%d lanes=%u reads=%u K=%u rescue=%u est=%d\n", grid, aim::kPairThreads, lanes, n_reads, K,
                    pp->options & AIM_PAIR_RESCUE, d_est != nullptr);
        aim::pair_sec_select_launch(s, lanes, grid, (hipStream_t)hip_stream);
    });
}

int aim_map_mates_secondary_device(uint32_t K, uint32_t n_reads, const aim_map_pair_t *d_pairs, const aim_segment_t *d_seg, const aim_sam_t *d_sam,
                                   const aim_sec_slot_t *d_sec, const uint32_t *d_contig, uint32_t n_contigs, const uint32_t *d_contig_start,
                                   const uint32_t *d_rec_offsets, aim_map_record_t *d_records, aim_map_mate_t *d_mates, void *hip_stream)
{
    const char *fn = "aim_map_mates_secondary_device";
    if (!((!(n_reads & 1u) || refuse("%s: n_reads %u is odd (reads 2m and 2m + 1 are mates)", fn, n_reads)) && cands_ok(fn, K) &&
          ((uint64_t)n_reads * (K + 1ull) < (1ull << 32) || refuse("%s: n_reads %u * (K %u + 1) does not fit 32 bits (split the batch)", fn, n_reads, K)) &&
          contigs_ok(fn, d_contig != nullptr, n_contigs, d_contig_start != nullptr) &&
          buffers_ok(fn, n_reads, d_pairs && d_seg && d_sam && d_sec && d_rec_offsets && d_records && d_mates) && aligned_ok(fn, d_sam, 16, "d_sam") &&
          aligned_ok(fn, d_pairs, 16, "d_pairs") && aligned_ok(fn, d_records, 16, "d_records") && aligned_ok(fn, d_mates, 16, "d_mates") &&
          aligned_ok(fn, d_seg, 8, "d_seg") && aligned_ok(fn, d_sec, 8, "d_sec")))
        return AIM_EINVAL;
    return launch_batch(n_reads, [&](const aim::Knobs &kn) {
        const aim::MatesSecArgs a = {{K, n_reads, d_contig ? n_contigs : 0u, d_pairs, d_seg, d_sam, d_contig, d_contig_start, d_rec_offsets, d_records, d_mates}, d_sec};
        // the record count is on the device: the grid covers the most there can be, n_reads * K, and is capped by what is resident
        const uint32_t grid = aim::pair_grid(kn, (uint64_t)n_reads * K, aim::kPairThreads);
        if (kn.plan_debug) fprintf(stderr, "[aim plan] map_mates_sec_kernel grid=%u block=%d reads=%u K=%u\n", grid, aim::kPairThreads, n_reads, K);
        aim::map_mates_sec_launch(a, grid, (hipStream_t)hip_stream);
    });
}

}  // extern "C"
