// capi_pair.hip -- the stateless entry points of rule 14c (include/aim_hip.h, AIM_FEATURE_PAIRED): aim_pair_rescue_rows_device,
// aim_pair_select_device (apply included) and aim_map_mates_device, with the kernels in pair.hpp, and the parameter check they share with
// aim_mapper_set_pairing (capi_mapper.hip). Host code only. What this unit shares with the others is in capi_common.hpp.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "capi_common.hpp"
#include "pair.hpp"

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

}  // namespace capi
}  // namespace aim

namespace {

// a buffer against its alignment; the message names it
bool aligned_ok(const char *fn, const void *p, uintptr_t align, const char *name)
{
    return !((uintptr_t)p & (align - 1u)) || refuse("%s: %s must be %u-byte aligned", fn, name, (unsigned)align);
}

bool contigs_ok(const char *fn, bool contigs, uint32_t n_contigs, bool tables)
{
    return !contigs || (((n_contigs >= 1 && n_contigs <= AIM_CONTIG_MAX) || refuse("%s: n_contigs %u is outside 1..%u", fn, n_contigs, AIM_CONTIG_MAX)) &&
                        (tables || refuse("%s: d_contig is given without its contig table", fn)));
}

uint32_t pair_grid(const aim::Knobs &kn, uint64_t units, uint32_t per_block)
{
    return (uint32_t)std::min<uint64_t>(aim::resident_grid(kn, aim::kPairPerCu), (units + per_block - 1u) / per_block);
}

}  // namespace

extern "C" {

const char *aim_pair_kernel_names(void) { return "pair_rescue_rows_kernel,pair_select_kernel,map_mates_kernel"; }

int aim_pair_rescue_rows_device(const aim_map_pair_params_t *pp, uint32_t K, uint32_t read_size, uint64_t ref_len, uint32_t n_contigs,
                                const uint32_t *d_contig_start, const uint32_t *d_contig_len, uint32_t n_reads, const int32_t *d_read_len, const char *d_reads,
                                const aim_segment_t *d_seg, const aim_sam_t *d_sam, const uint32_t *d_contig, void *d_res_requests, uint64_t *d_res_text_pos,
                                char *d_res_patterns, void *hip_stream)
{
    const char *fn = "aim_pair_rescue_rows_device";
    if (const int rc = check_pair_params(fn, pp, K, read_size, n_reads, true)) return rc;
    if (!((ref_len >= 1 || refuse("%s: ref_len must be >= 1", fn)) && ref_len_ok(fn, ref_len, false) &&
          contigs_ok(fn, d_contig != nullptr, n_contigs, d_contig_start && d_contig_len) &&
          buffers_ok(fn, n_reads, d_read_len && d_reads && d_seg && d_sam && d_res_requests && d_res_text_pos && d_res_patterns) &&
          aligned_ok(fn, d_sam, 16, "d_sam") && aligned_ok(fn, d_res_requests, 16, "d_res_requests") && aligned_ok(fn, d_reads, 8, "d_reads") &&
          aligned_ok(fn, d_res_patterns, 8, "d_res_patterns") && aligned_ok(fn, d_seg, 8, "d_seg") && aligned_ok(fn, d_res_text_pos, 8, "d_res_text_pos")))
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
            fprintf(stderr, "[aim plan] pair_rescue_rows_kernel grid=%u block=%d lanes=%u reads=%u K=%u rescue_size=%u\n", grid, aim::kPairThreads, lanes, n_reads, K,
                    pp->rescue_size);
        aim::pair_rescue_rows_launch(a, lanes, grid, (hipStream_t)hip_stream);
    });
}

int aim_pair_select_device(const aim_map_pair_params_t *pp, uint32_t K, uint32_t read_size, uint32_t n_reads, const int32_t *d_read_len, aim_segment_t *d_seg,
                           aim_sam_t *d_sam, aim_chain_class_t *d_class, uint32_t *d_contig, const aim_sam_t *d_res_sam, uint32_t cigar_base, uint32_t md_base,
                           aim_map_pair_t *d_pairs, void *hip_stream)
{
    const char *fn = "aim_pair_select_device";
    if (const int rc = check_pair_params(fn, pp, K, read_size, n_reads, false)) return rc;
    if (!(buffers_ok(fn, n_reads, d_read_len && d_seg && d_sam && d_class && d_pairs && (d_res_sam || !(pp->options & AIM_PAIR_RESCUE))) &&
          aligned_ok(fn, d_sam, 16, "d_sam") && aligned_ok(fn, d_res_sam, 16, "d_res_sam") && aligned_ok(fn, d_pairs, 16, "d_pairs") &&
          aligned_ok(fn, d_seg, 8, "d_seg") && aligned_ok(fn, d_class, 8, "d_class")))
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
            fprintf(stderr, "[aim plan] pair_select_kernel grid=%u block=%d lanes=%u reads=%u K=%u rescue=%u\n", grid, aim::kPairThreads, lanes, n_reads, K,
                    pp->options & AIM_PAIR_RESCUE);
        aim::pair_select_launch(a, lanes, grid, (hipStream_t)hip_stream);
    });
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
