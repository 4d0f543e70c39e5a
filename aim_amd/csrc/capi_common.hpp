// capi_common.hpp -- what the units of the C-ABI share: aim_capi.hip (device sets, slots, submit and wait), capi_launch.hip (a plan into
// launches, and the stateless alignment entry points), capi_groups.hip (the read-groups path: AIM_FLAG_READ_GROUPS, MATE_PAIRS and
// TOP_HITS) -- these three share the device set and launch() through capi_set.hpp --,
// capi_plan.hip (the launch planner; its types and entry points are in plan.hpp), capi_pipeline.hip (index, seeding, classes and MAPQ,
// split, extension), capi_mapper.hip (the record list and aim_mapper_t), capi_pair.hip (rule 14c's stateless entry points), capi_secondary.hip (rule 16c's), capi_pair_secondary.hip (rule 17c's) and capi_host.hip (host-side formatters and
// generators). None of
// them compiles a kernel: each kernel family's tu_*.hip does, and these units call its launchers. Internal, not installed.
// Every function declared here has ONE definition, next to the state it owns: fail() in aim_capi.hip, where it writes the thread-local
// buffer aim_last_error() returns; read_knobs(), the one reader of the AIM_* environment, with_chip(), which asks chip_cus()'s per-device
// cache, and check_align_params() in capi_plan.hip; the parameter checks of the pipeline's stages in capi_pipeline.hip; the refusals the
// pipeline's entry points share inline below.
#pragma once
#include <cstdint>
#include <cstring>

#include <hip/hip_runtime.h>

#include "aim_hip.h"
#include "aim_device.hpp"

namespace aim {
namespace capi {
#pragma GCC visibility push(hidden)
int fail(int code, const char *fmt, ...);   // sets aim_last_error() for the calling thread and returns `code`
aim::Knobs read_knobs();                    // the AIM_* environment, as it is now
aim::Knobs with_chip(aim::Knobs k);         // ... for a plan on the current device: AIM_CHIP_CUS wins, else the device's own CU count
// Every length of a batch against READ_SIZE; AIM_EINVAL names the first pair that breaks it (and *bad_pair receives it).
int check_lengths(const aim_params_t &p, uint32_t n_pairs, const void *requests, uint32_t *bad_pair = nullptr);
// AIM_FLAG_REF_TEXTS: texts gathered from a device-resident reference (batch_io.hpp); no plan depends on it.
inline bool is_ref(const aim_params_t &p) { return (p.flags & AIM_FLAG_REF_TEXTS) != 0; }
// What every alignment entry point refuses about its aim_params_t (capi_plan.hip: validate_params), before any device query.
int check_align_params(const aim_params_t &p);
// The bounds every seeding entry point sets (capi_pipeline.hip). max_read_size is AIM_SEED_MAX_READ_SIZE, or the entry point's own bound,
// and then `fn` names that entry point in the read_size message.
int check_seed_params(const aim_seed_params_t &sp, int32_t max_read_size = AIM_SEED_MAX_READ_SIZE, const char *fn = nullptr);
// aim_seed_chain_device's own bound behind check_seed_params, under the name `fn`.
int check_seed_chain_band(const aim_seed_params_t &sp, const char *fn);
// aim_seed_chain_long_device's parameter check: check_seed_params with the long read_size bound, then what is its own.
int check_seed_long_params(const aim_seed_params_t &sp, uint32_t max_hits);
// aim_extend_segments_device's refusals of its aim_extend_params_t, in the header's order, under the name `fn`.
int check_extend_params(const char *fn, const aim_extend_params_t *p);
// Rule 14c's refusals of its aim_map_pair_params_t against K, read_size and n_reads, in the header's order, under the name `fn`
// (capi_pair.hip). The rescue_size bounds are checked with AIM_PAIR_RESCUE, or always when `rescue_always`.
int check_pair_params(const char *fn, const aim_map_pair_params_t *pp, uint32_t K, uint32_t read_size, uint32_t n_reads, bool rescue_always);
// Rule 15c's refusals of its aim_pair_est_params_t, in the header's order, under the name `fn` (capi_pair.hip).
int check_pair_est_params(const char *fn, const aim_pair_est_params_t *ep);

// The refusals the pipeline's entry points share: one copy of each bound and of its message; `fn` names the entry point. Each is true when
// its bound holds and otherwise leaves its message in aim_last_error(). An entry point joins them with && in its own order -- the order its
// violations are reported in -- and answers AIM_EINVAL when the chain breaks.
template <typename... A>
inline bool refuse(const char *fmt, A... a) { return fail(AIM_EINVAL, fmt, a...) == AIM_OK; }
inline bool cands_ok(const char *fn, uint32_t K) { return (K >= 1 && K <= AIM_SEED_MAX_CANDS) || refuse("%s: K %u is outside 1..%d", fn, K, AIM_SEED_MAX_CANDS); }
inline bool read_size_ok(const char *fn, uint32_t rs)
{
    return (rs && !(rs & 7u) && rs <= AIM_SEED_LONG_MAX_READ_SIZE) || refuse("%s: read_size %u must be a positive multiple of 8, at most %d", fn, rs, AIM_SEED_LONG_MAX_READ_SIZE);
}
// (n_reads * K candidate slots are indexed with 32 bits; `what` is the name K goes by in the entry point's arguments)
inline bool slots_ok(const char *fn, uint32_t n_reads, uint32_t K, const char *what = "K")
{
    return (uint64_t)n_reads * K < (1ull << 32) || refuse("%s: n_reads %u * %s %u does not fit 32 bits (split the batch)", fn, n_reads, what, K);
}
// (the index and seeding entry points say why, the later stages name the bound)
inline bool ref_len_ok(const char *fn, uint64_t ref_len, bool say_why)
{
    if (ref_len <= AIM_SEED_MAX_REF_LEN) return true;
    return say_why ? refuse("%s: ref_len %llu is above 2^32 - 2^25 (positions and diagonal keys are 32-bit)", fn, (unsigned long long)ref_len)
                   : refuse("%s: ref_len %llu is above %llu", fn, (unsigned long long)ref_len, (unsigned long long)AIM_SEED_MAX_REF_LEN);
}
// (an empty batch may come with NULL buffers)
inline bool buffers_ok(const char *fn, uint32_t n_reads, bool all_set) { return !n_reads || all_set || refuse("%s: null device buffer", fn); }
// a buffer against its alignment; the message names it
inline bool aligned_ok(const char *fn, const void *p, uintptr_t align, const char *name)
{
    return !((uintptr_t)p & (align - 1u)) || refuse("%s: %s must be %u-byte aligned", fn, name, (unsigned)align);
}
// d_contig comes with a contig table of 1..AIM_CONTIG_MAX entries (rules 14c and 17c)
inline bool contigs_ok(const char *fn, bool contigs, uint32_t n_contigs, bool tables)
{
    return !contigs || (((n_contigs >= 1 && n_contigs <= AIM_CONTIG_MAX) || refuse("%s: n_contigs %u is outside 1..%u", fn, n_contigs, AIM_CONTIG_MAX)) &&
                        (tables || refuse("%s: d_contig is given without its contig table", fn)));
}
// AIM_DEBUG_POISON_LDS as the kernels take it (dbg_poison_lds): 0x100 | byte, or 0 for "leave LDS as it is"
inline uint32_t poison_lds_word(const aim::Knobs &kn) { return kn.poison_lds >= 0 ? (0x100u | (uint32_t)(kn.poison_lds & 0xff)) : 0u; }
// The KArgs of a batch-I/O kernel: the params, the pair count and the requests; every other member zero
inline aim::KArgs batch_args(const aim_params_t &p, uint32_t n_pairs, const void *req)
{
    aim::KArgs ka;
    memset(&ka, 0, sizeof ka);
    ka.p = p;
    ka.n_pairs = n_pairs;
    ka.req = static_cast<const aim_request_t *>(req);
    return ka;
}
#pragma GCC visibility pop
}  // namespace capi
}  // namespace aim

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return ::aim::capi::fail(e_ == hipErrorOutOfMemory ? AIM_ENOMEM : AIM_ENODEV, "%s failed: %s", #expr, \
                                     hipGetErrorString(e_));                                \
    } while (0)

namespace aim {
namespace capi {
// What every batch entry point of the pipeline ends in once its arguments are checked: the device probe, nothing to do for an empty batch,
// then launch(kn) with the knobs of the current device, and the launch's error.
template <typename Launch>
inline int launch_batch(uint32_t n_reads, Launch launch)
{
    int n = 0;
    if (const int rc = aim_device_count(&n)) return rc;
    if (!n_reads) return AIM_OK;
    launch(with_chip(read_knobs()));
    HIP_TRY(hipGetLastError());
    return AIM_OK;
}
}  // namespace capi
}  // namespace aim
