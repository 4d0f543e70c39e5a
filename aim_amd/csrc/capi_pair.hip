// capi_pair.hip -- the stateless entry points of rule 14c (include/aim_hip.h, AIM_FEATURE_PAIRED): aim_pair_rescue_rows_device,
// aim_pair_select_device (apply included) and aim_map_mates_device, with the kernels in pair.hpp, and the parameter check they share with
// aim_mapper_set_pairing (capi_mapper.hip); and those of rule 15c (AIM_FEATURE_PAIR_ESTIMATE): aim_pair_estimate_device, with the kernels
// in pair_estimate.hpp, and the _est twins of rule 14c's first two, which run the same bodies with the bounds read on the device. Host code only. What this unit shares with the others is in capi_common.hpp.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "capi_common.hpp"
#include "pair.hpp"
#include "pair_estimate.hpp"

using namespace aim::capi;

namespace aim {
namespace capi {

int check_pair_params(const char *fn, const aim_map_pair_params_t *pp, uint32_t K, uint32_t read_size, uint32_t n_reads, bool rescue_always)
{
    if (!pp) return fail(AIM_EINVAL, "%s: aim_map_pair_params_t is NULL", fn);
    if (!((!(pp->options & ~AIM_PAIR_RESCUE) || refuse("%s: unknown options 0x%x", fn, pp->options)) &&
          (!(n_reads & 1u) || refuse("%s: n_reads %u is odd (reads 2m and 2m + 1 are mates)", fn, n_reads)) && cands_ok(fn, K) &&
          ((uint64_t)n_reads * (K + 1ull) < (1ull << 32) || refuse("%s: n_reads %u * (K %u + 1) does not fit 32 bits (split the batch)", fn, n_reads, K)) &&
          ((pp->min_span >= 0 && pp->max_span >= pp->min_span && pp->max_span < (1ll << 62)) ||
           refuse("%s: spans must satisfy 0 <= min_span <= max_span < 2^62 (min_span %lld, max_span %lld)", fn, (long long)pp->min_span, (long long)pp->max_span)) &&
          (pp->unpaired_penalty >= 0 || refuse("%s: unpaired_penalty %d must be >= 0", fn, pp->unpaired_penalty)) && read_size_ok(fn, read_size)))
        return AIM_EINVAL;
    if (!rescue_always && !(pp->options & AIM_PAIR_RESCUE)) return AIM_OK;
    const uint32_t rz = pp->rescue_size;
    if (rz & 7u) return fail(AIM_EINVAL, "%s: rescue_size %u must be a multiple of 8", fn, rz);
    if (rz < read_size) return fail(AIM_EINVAL, "%s: rescue_size %u is below read_size %u", fn, rz, read_size);
    if (pp->max_span - pp->min_span + (int64_t)read_size > (int64_t)rz)
        return fail(AIM_EINVAL, "%s: max_span %lld - min_span %lld + read_size %u exceeds rescue_size %u (the rescue window must fit its row)", fn,
                    (long long)pp->max_span, (long long)pp->min_span, read_size, rz);
    return AIM_OK;
}

int check_pair_est_params(const char *fn, const aim_pair_est_params_t *ep)
{
    if (!ep) return fail(AIM_EINVAL, "%s: aim_pair_est_params_t is NULL", fn);
    if (ep->hist_size < 64u || ep->hist_size > AIM_PAIR_EST_MAX_HIST || (ep->hist_size & 63u))
        return fail(AIM_EINVAL, "%s: hist_size %u must be a multiple of 64 in 64..%u", fn, ep->hist_size, AIM_PAIR_EST_MAX_HIST);
    if (!ep->min_samples) return fail(AIM_EINVAL, "%s: min_samples must be >= 1", fn);
    if (ep->min_mapq > 60u) return fail(AIM_EINVAL, "%s: min_mapq %u is outside 0..60", fn, ep->min_mapq);
    return AIM_OK;
}

}  // namespace capi
}  // namespace aim

using aim::pair_grid;

extern "C" {

const char *aim_pair_kernel_names(void) { return "pair_rescue_rows_kernel,pair_select_kernel,map_mates_kernel"; }

}  // extern "C"

namespace {

// (with `est`: the d_est of the _est twins, checked behind everything their rule-14c originals check)
bool est_ok(const char *fn, bool est, uint32_t n_reads, const aim_pair_estimate_t *d_est)
{
    return !est || (buffers_ok(fn, n_reads, d_est != nullptr) && aligned_ok(fn, d_est, 16, "d_est"));
}

// aim_pair_rescue_rows_device and, with `est`, its rule-15c twin
int rescue_rows(const char *fn, bool est, const aim_map_pair_params_t *pp, uint32_t K, uint32_t read_size, uint64_t ref_len, uint32_t n_contigs,
                const uint32_t *d_contig_start, const uint32_t *d_contig_len, uint32_t n_reads, const int32_t *d_read_len, const char *d_reads,
                const aim_segment_t *d_seg, const aim_sam_t *d_sam, const uint32_t *d_contig, void *d_res_requests, uint64_t *d_res_text_pos,
                char *d_res_patterns, const aim_pair_estimate_t *d_est, void *hip_stream)
{
    if (const int rc = check_pair_params(fn, pp, K, read_size, n_reads, true)) return rc;
    if (!((ref_len >= 1 || refuse("%s: ref_len must be >= 1", fn)) && ref_len_ok(fn, ref_len, false) &&
          contigs_ok(fn, d_contig != nullptr, n_contigs, d_contig_start && d_contig_len) &&
          buffers_ok(fn, n_reads, d_read_len && d_reads && d_seg && d_sam && d_res_requests && d_res_text_pos && d_res_patterns) &&
          aligned_ok(fn, d_sam, 16, "d_sam") && aligned_ok(fn, d_res_requests, 16, "d_res_requests") && aligned_ok(fn, d_reads, 8, "d_reads") &&
          aligned_ok(fn, d_res_patterns, 8, "d_res_patterns") && aligned_ok(fn, d_seg, 8, "d_seg") && aligned_ok(fn, d_res_text_pos, 8, "d_res_text_pos") &&
          est_ok(fn, est, n_reads, d_est)))
        return AIM_EINVAL;
    return launch_batch(n_reads, [&](const aim::Knobs &kn) {
        aim::PairArgs a;
        memset(&a, 0, sizeof a);
        a.K = K; a.n_reads = n_reads; a.read_size = read_size; a.rescue_size = pp->rescue_size; a.options = pp->options; a.n_contigs = d_contig ? n_contigs : 0u;
        a.min_span = pp->min_span; a.max_span = pp->max_span; a.ref_len = (int64_t)ref_len;
        a.read_len = d_read_len; a.reads = d_reads;
        a.seg = const_cast<aim_segment_t *>(d_seg); a.sam = const_cast<aim_sam_t *>(d_sam); a.contig = const_cast<uint32_t *>(d_contig);   // (read only here)
        a.contig_start = d_contig_start; a.contig_len = d_contig_len;
        a.res_req = static_cast<aim_request_t *>(d_res_requests); a.res_text_pos = d_res_text_pos; a.res_patterns = d_res_patterns;
        const uint32_t lanes = aim::chain_class_lanes(K), grid = pair_grid(kn, n_reads / 2u, aim::kPairThreads / lanes);
        if (kn.plan_debug)
            fprintf(stderr, "[aim plan] %s grid=%u block=%d lanes=%u reads=%u K=%u rescue_size=%u\n", est ? "pair_rescue_rows_est_kernel" : "pair_rescue_rows_kernel", grid,
                    aim::kPairThreads, lanes, n_reads, K, pp->rescue_size);
        if (est) aim::pair_rescue_rows_est_launch(a, lanes, grid, d_est, (hipStream_t)hip_stream);
        else aim::pair_rescue_rows_launch(a, lanes, grid, (hipStream_t)hip_stream);
    });
}

// aim_pair_select_device and, with `est`, its rule-15c twin
int pair_select(const char *fn, bool est, const aim_map_pair_params_t *pp, uint32_t K, uint32_t read_size, uint32_t n_reads, const int32_t *d_read_len,
                aim_segment_t *d_seg, aim_sam_t *d_sam, aim_chain_class_t *d_class, uint32_t *d_contig, const aim_sam_t *d_res_sam, uint32_t cigar_base,
                uint32_t md_base, aim_map_pair_t *d_pairs, const aim_pair_estimate_t *d_est, void *hip_stream)
{
    if (const int rc = check_pair_params(fn, pp, K, read_size, n_reads, false)) return rc;
    if (!(buffers_ok(fn, n_reads, d_read_len && d_seg && d_sam && d_class && d_pairs && (d_res_sam || !(pp->options & AIM_PAIR_RESCUE))) &&
          aligned_ok(fn, d_sam, 16, "d_sam") && aligned_ok(fn, d_res_sam, 16, "d_res_sam") && aligned_ok(fn, d_pairs, 16, "d_pairs") &&
          aligned_ok(fn, d_seg, 8, "d_seg") && aligned_ok(fn, d_class, 8, "d_class") && est_ok(fn, est, n_reads, d_est)))
        return AIM_EINVAL;
    return launch_batch(n_reads, [&](const aim::Knobs &kn) {
        aim::PairArgs a;
        memset(&a, 0, sizeof a);
        a.K = K; a.n_reads = n_reads; a.read_size = read_size; a.rescue_size = pp->rescue_size; a.options = pp->options;
        a.unpaired_penalty = pp->unpaired_penalty; a.cigar_base = cigar_base; a.md_base = md_base;
        a.min_span = pp->min_span; a.max_span = pp->max_span;
        a.read_len = d_read_len; a.seg = d_seg; a.sam = d_sam; a.cls = d_class; a.contig = d_contig; a.res_sam = d_res_sam; a.pairs = d_pairs;
        const uint32_t lanes = aim::chain_class_lanes(K), grid = pair_grid(kn, n_reads / 2u, aim::kPairThreads / lanes);
        if (kn.plan_debug)
            fprintf(stderr, "[aim plan] %s grid=%u block=%d lanes=%u reads=%u K=%u rescue=%u\n", est ? "pair_select_est_kernel" : "pair_select_kernel", grid,
                    aim::kPairThreads, lanes, n_reads, K, pp->options & AIM_PAIR_RESCUE);
        if (est) aim::pair_select_est_launch(a, lanes, grid, d_est, (hipStream_t)hip_stream);
        else aim::pair_select_launch(a, lanes, grid, (hipStream_t)hip_stream);
    });
}

}  // namespace

extern "C" {

int aim_pair_rescue_rows_device(const aim_map_pair_params_t *pp, uint32_t K, uint32_t read_size, uint64_t ref_len, uint32_t n_contigs,
                                const uint32_t *d_contig_start, const uint32_t *d_contig_len, uint32_t n_reads, const int32_t *d_read_len, const char *d_reads,
                                const aim_segment_t *d_seg, const aim_sam_t *d_sam, const uint32_t *d_contig, void *d_res_requests, uint64_t *d_res_text_pos,
                                char *d_res_patterns, void *hip_stream)
{
    return rescue_rows("aim_pair_rescue_rows_device", false, pp, K, read_size, ref_len, n_contigs, d_contig_start, d_contig_len, n_reads, d_read_len, d_reads, d_seg,
                       d_sam, d_contig, d_res_requests, d_res_text_pos, d_res_patterns, nullptr, hip_stream);
}

int aim_pair_select_device(const aim_map_pair_params_t *pp, uint32_t K, uint32_t read_size, uint32_t n_reads, const int32_t *d_read_len, aim_segment_t *d_seg,
                           aim_sam_t *d_sam, aim_chain_class_t *d_class, uint32_t *d_contig, const aim_sam_t *d_res_sam, uint32_t cigar_base, uint32_t md_base,
                           aim_map_pair_t *d_pairs, void *hip_stream)
{
    return pair_select("aim_pair_select_device", false, pp, K, read_size, n_reads, d_read_len, d_seg, d_sam, d_class, d_contig, d_res_sam, cigar_base, md_base,
                       d_pairs, nullptr, hip_stream);
}

// ---------------------------------------------------------------------------
// rule 15c (AIM_FEATURE_PAIR_ESTIMATE): the bounds from the batch, and rule 14c's two kernels reading them on the device
// ---------------------------------------------------------------------------
const char *aim_pair_estimate_kernel_names(void) { return "pair_span_hist_kernel,pair_span_bounds_kernel,pair_rescue_rows_est_kernel,pair_select_est_kernel"; }

size_t aim_pair_estimate_scratch(uint32_t hist_size) { return 4u * (size_t)hist_size + 16u; }

int aim_pair_estimate_device(const aim_map_pair_params_t *pp, const aim_pair_est_params_t *ep, uint32_t K, uint32_t read_size, uint32_t n_reads,
                             const aim_segment_t *d_seg, const aim_sam_t *d_sam, const aim_chain_class_t *d_class, const uint32_t *d_contig,
                             aim_pair_estimate_t *d_est, void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
    const char *fn = "aim_pair_estimate_device";
    if (const int rc = check_pair_params(fn, pp, K, read_size, n_reads, false)) return rc;
    if (const int rc = check_pair_est_params(fn, ep)) return rc;
    const size_t need = aim_pair_estimate_scratch(ep->hist_size);
    if (!(buffers_ok(fn, n_reads, d_seg && d_sam && d_class && d_est && d_scratch) && aligned_ok(fn, d_est, 16, "d_est") && aligned_ok(fn, d_sam, 16, "d_sam") &&
          aligned_ok(fn, d_seg, 8, "d_seg") && aligned_ok(fn, d_class, 8, "d_class") && aligned_ok(fn, d_scratch, 4, "d_scratch") &&
          (!n_reads || scratch_bytes >= need || refuse("%s: scratch_bytes %zu is below the %zu aim_pair_estimate_scratch reports", fn, scratch_bytes, need))))
        return AIM_EINVAL;
    hipStream_t stream = (hipStream_t)hip_stream;
    int n_dev = 0;
    if (const int rc = aim_device_count(&n_dev)) return rc;
    if (!n_reads && !d_est) return AIM_OK;
    const aim::Knobs kn = with_chip(read_knobs());
    aim::PairEstArgs a;
    memset(&a, 0, sizeof a);
    a.K = K; a.n_reads = n_reads; a.hist_size = ep->hist_size; a.min_mapq = ep->min_mapq; a.dbg_poison_lds = poison_lds_word(kn);
    a.seg = d_seg; a.sam = d_sam; a.cls = d_class; a.contig = d_contig;
    a.min_samples = ep->min_samples; a.min_slack = ep->min_slack; a.options = pp->options; a.read_size = read_size; a.rescue_size = pp->rescue_size;
    a.min_span = pp->min_span; a.max_span = pp->max_span; a.est = d_est;
    if (n_reads) {                       // (an empty batch: the bounds kernel alone, over no histogram)
        a.hist = static_cast<uint32_t *>(d_scratch);
        // Debugging aid, as for the index scratch: results must not depend on what the scratch held before. The clear is the entry point's own.
        if (kn.poison_scratch >= 0) HIP_TRY(hipMemsetAsync(d_scratch, kn.poison_scratch & 0xff, need, stream));
        HIP_TRY(hipMemsetAsync(d_scratch, 0, need, stream));
        const uint32_t lanes = aim::chain_class_lanes(K);
        // every workgroup ends with one global add per non-zero bin of its own histogram, onto a few hundred hot addresses: a workgroup
        // walks kPairEstBlocksPerWg blocks of read pairs at least, so that there are few of those flushes (profiles/pair_estimate/README.md)
        const uint64_t per_block = aim::kPairEstThreads / lanes, n_blocks = ((uint64_t)(n_reads / 2u) + per_block - 1u) / per_block;
        const uint32_t grid = (uint32_t)std::min<uint64_t>(aim::resident_grid(kn, aim::kPairEstPerCu), (n_blocks + aim::kPairEstBlocksPerWg - 1u) / aim::kPairEstBlocksPerWg);
        if (kn.plan_debug)
            fprintf(stderr, "[aim plan] pair_span_hist_kernel grid=%u block=%d lanes=%u reads=%u K=%u hist_size=%u lds=%u; pair_span_bounds_kernel grid=1 block=%d\n", grid,
                    aim::kPairEstThreads, lanes, n_reads, K, ep->hist_size, 4u * (ep->hist_size + 1u), aim::kPairEstThreads);
        aim::pair_span_hist_launch(a, lanes, grid, stream);
        HIP_TRY(hipGetLastError());
    }
    aim::pair_span_bounds_launch(a, stream);
    HIP_TRY(hipGetLastError());
    return AIM_OK;
}

int aim_pair_rescue_rows_device_est(const aim_map_pair_params_t *pp, uint32_t K, uint32_t read_size, uint64_t ref_len, uint32_t n_contigs,
                                    const uint32_t *d_contig_start, const uint32_t *d_contig_len, uint32_t n_reads, const int32_t *d_read_len, const char *d_reads,
                                    const aim_segment_t *d_seg, const aim_sam_t *d_sam, const uint32_t *d_contig, void *d_res_requests, uint64_t *d_res_text_pos,
                                    char *d_res_patterns, const aim_pair_estimate_t *d_est, void *hip_stream)
{
    return rescue_rows("aim_pair_rescue_rows_device_est", true, pp, K, read_size, ref_len, n_contigs, d_contig_start, d_contig_len, n_reads, d_read_len, d_reads, d_seg,
                       d_sam, d_contig, d_res_requests, d_res_text_pos, d_res_patterns, d_est, hip_stream);
}

int aim_pair_select_device_est(const aim_map_pair_params_t *pp, uint32_t K, uint32_t read_size, uint32_t n_reads, const int32_t *d_read_len, aim_segment_t *d_seg,
                               aim_sam_t *d_sam, aim_chain_class_t *d_class, uint32_t *d_contig, const aim_sam_t *d_res_sam, uint32_t cigar_base, uint32_t md_base,
                               aim_map_pair_t *d_pairs, const aim_pair_estimate_t *d_est, void *hip_stream)
{
    return pair_select("aim_pair_select_device_est", true, pp, K, read_size, n_reads, d_read_len, d_seg, d_sam, d_class, d_contig, d_res_sam, cigar_base, md_base,
                       d_pairs, d_est, hip_stream);
}

int aim_map_mates_device(uint32_t K, uint32_t n_reads, const aim_map_pair_t *d_pairs, const aim_segment_t *d_seg, const aim_sam_t *d_sam, const uint32_t *d_contig,
                         uint32_t n_contigs, const uint32_t *d_contig_start, const uint32_t *d_rec_offsets, aim_map_record_t *d_records, aim_map_mate_t *d_mates,
                         void *hip_stream)
{
    const char *fn = "aim_map_mates_device";
    if (!((!(n_reads & 1u) || refuse("%s: n_reads %u is odd (reads 2m and 2m + 1 are mates)", fn, n_reads)) && cands_ok(fn, K) &&
          ((uint64_t)n_reads * (K + 1ull) < (1ull << 32) || refuse("%s: n_reads %u * (K %u + 1) does not fit 32 bits (split the batch)", fn, n_reads, K)) &&
          contigs_ok(fn, d_contig != nullptr, n_contigs, d_contig_start != nullptr) &&
          buffers_ok(fn, n_reads, d_pairs && d_seg && d_sam && d_rec_offsets && d_records && d_mates) && aligned_ok(fn, d_sam, 16, "d_sam") &&
          aligned_ok(fn, d_pairs, 16, "d_pairs") && aligned_ok(fn, d_records, 16, "d_records") && aligned_ok(fn, d_mates, 16, "d_mates") &&
          aligned_ok(fn, d_seg, 8, "d_seg")))
        return AIM_EINVAL;
    return launch_batch(n_reads, [&](const aim::Knobs &kn) {
        const aim::MatesArgs a = {K, n_reads, d_contig ? n_contigs : 0u, d_pairs, d_seg, d_sam, d_contig, d_contig_start, d_rec_offsets, d_records, d_mates};
        // the record count is on the device: the grid covers the most there can be, n_reads * K, and is capped by what is resident
        const uint32_t grid = pair_grid(kn, (uint64_t)n_reads * K, aim::kPairThreads);
        if (kn.plan_debug) fprintf(stderr, "[aim plan] map_mates_kernel grid=%u block=%d reads=%u K=%u\n", grid, aim::kPairThreads, n_reads, K);
        aim::map_mates_launch(a, grid, (hipStream_t)hip_stream);
    });
}

}  // extern "C"
