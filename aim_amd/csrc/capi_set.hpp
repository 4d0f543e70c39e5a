// capi_set.hpp -- what aim_capi.hip, capi_launch.hip and capi_groups.hip share: the device set with its slots, the launch of a plan
// over the buffers a LaunchIo names, and the functions of aim_capi.hip that a groups batch goes through (the slot's reset and row copies,
// the window and SAM checks, the SAM kernel on a slot). Internal, not installed. Every function declared here has ONE definition:
// launch(), launch_todo_stage() and aux_stream_destroy() in capi_launch.hip, submit_groups() in capi_groups.hip, the others in aim_capi.hip.
#pragma once
#include <vector>

#include "capi_common.hpp"
#include "plan.hpp"

#pragma GCC visibility push(hidden)
namespace aim {
namespace capi {
// A second stream per device for work that only has to be ordered against ONE kernel of a launch, not against the whole stream:
// wfa_group's traceback kernel of chunk c runs there while chunk c + 1 is computed on the caller's stream (the traceback is a
// latency-bound walk -- 93 % of its wavefront cycles are waits -- so it costs the compute kernel next to nothing). Events are
// re-recorded per launch; a hipStreamWaitEvent captures the record that precedes it, so re-use across launches is safe.
// OWNERSHIP: every slot of a device set has its own (created on first use, destroyed with the slot), so two host threads driving two
// sets -- or two slots -- on one device never record / wait on each other's events. The stateless aim_align_device has no slot: it
// uses one per-device instance and holds that device's mutex across its whole chunk loop.
struct AuxStream {
    hipStream_t stream = nullptr;
    hipEvent_t computed[2] = {nullptr, nullptr};   // compute kernel of the chunk that uses history buffer b has finished
    hipEvent_t walked[2] = {nullptr, nullptr};     // traceback of that chunk has finished (buffer b is free again)
};

// The fused batch I/O of a launch (Plan::pk / Plan::emits_runs): packed rows in, compact CIGAR out.
struct FusedIo {
    const uint32_t *packedP = nullptr, *packedT = nullptr;
    aim_cigar_t *cig = nullptr;
    uint32_t *runs = nullptr, *cursor = nullptr;
    uint32_t runs_cap = 0, run_slot = 0;
};

// The device buffers of the batch a launch runs over, by name (several are interchangeable by type): what a plan does not touch stays null.
struct LaunchIo {
    uint32_t n_pairs = 0;
    const void *req = nullptr;
    const char *pat = nullptr, *txt = nullptr;
    void *res = nullptr;
    char *ops = nullptr;
    void *scratch = nullptr;
    size_t scratch_bytes = 0;
};
}  // namespace capi
}  // namespace aim

// ---------------------------------------------------------------------------
// device set
// ---------------------------------------------------------------------------
// One buffer set + stream: what a batch needs from H2D to D2H. Slot 0 also serves aim_set_push / launch / pull.
struct aim_slot {
    hipStream_t stream = nullptr;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // h2d b/e, kernel b/e, d2h b/e
    void *d_req = nullptr;   // aim_request_t[] or aim_request8_t[] (AIM_FLAG_REQ8)
    char *d_pat = nullptr, *d_txt = nullptr, *d_ops = nullptr;
    void *d_res = nullptr;   // aim_result_t[] or aim_result8_t[] (AIM_FLAG_RES8)
    void *d_scratch = nullptr;
    size_t scratch_bytes = 0;
    uint32_t *d_packP = nullptr, *d_packT = nullptr;                 // packed input rows
    uint32_t *d_rawidx = nullptr;                                    // side list of raw pairs
    char *d_rawP = nullptr, *d_rawT = nullptr;
    aim_cigar_t *d_cig = nullptr;                                    // compact CIGAR
    uint32_t *d_runs = nullptr, *d_cursor = nullptr, *h_cursor = nullptr;
    void *d_rawreq = nullptr, *d_rawres = nullptr;                   // raw side pass (fused packed batches): the side list as a batch of its own
    char *d_rawops = nullptr;
    aim_cigar_t *d_rawcig = nullptr;
    uint64_t *d_tpos = nullptr;      // AIM_FLAG_REF_TEXTS: the batch's text_pos[]
    uint32_t *d_reftodo = nullptr;   // ... packed batches on the fused lane kernel: to-do list {count @0, pair ids @16..} + flag bits
    bool ref_pending = false;        // aim_set_push_ref: the texts are gathered at aim_set_launch
    // AIM_FLAG_READ_GROUPS (groups.hpp): the read-level inputs, the score-only pass's rows, the selection and the winners' batch
    char *g_readP = nullptr;         // [max_pairs][READ_SIZE] read pattern rows as they arrive
    uint32_t *g_roff = nullptr, *g_map = nullptr, *g_sel = nullptr, *g_rawslot = nullptr;
    aim_result_t *g_res1 = nullptr;
    aim_best_t *g_best = nullptr;
    aim_mate_t *g_mates = nullptr;   // AIM_FLAG_MATE_PAIRS: [max_pairs / 2]
    uint32_t *g_hoff = nullptr, *g_hit = nullptr;   // AIM_FLAG_TOP_HITS: hit_offsets [max_pairs + 1], hit_pair [max_pairs]
    // AIM_FLAG_SAM_FIELDS (aim_set_sam_capacity): records, CIGAR words, MD bytes, the two cursors and their pinned host copy
    aim_sam_t *d_sam = nullptr;
    uint32_t *d_samcig = nullptr, *d_samcur = nullptr, *h_samcur = nullptr;
    char *d_sammd = nullptr;
    uint32_t samcig_cap = 0, sammd_cap = 0;
    // ... the SAM members of the batch in flight (sam == nullptr: none)
    aim_sam_t *io_sam = nullptr;
    uint32_t *io_samcig = nullptr;
    char *io_sammd = nullptr;
    uint32_t io_samcig_cap = 0, io_sammd_cap = 0;
    void *g_req2 = nullptr;
    char *g_pat2 = nullptr, *g_txt2 = nullptr;
    uint32_t n_reads = 0;            // reads of the groups batch in flight (n_pairs then counts its output rows)
    aim::capi::Plan plan_last2;      // ... the second pass's plan
    uint32_t n_pairs = 0;
    uint32_t runs_sent = 0;  // runs of the batch in flight whose D2H copy aim_set_submit already enqueued (slotted run buffer)
    bool pushed = false, launched = false, submitted = false;
    aim::capi::AuxStream aux;   // this slot's second stream + events (chunked wfa_group launches with CIGAR); created on first use
    aim::capi::Plan plan_last;  // the plan the last launch followed (the configure-time plan re-made for the pushed pair count)
    aim_batch_io_t io;       // the batch in flight (aim_set_submit .. aim_set_wait)
    // what free_slot releases: every hipMalloc / hipHostMalloc of the slot, recorded where it is made; the SAM buffers apart, because
    // aim_set_sam_capacity re-allocates them on a live slot
    std::vector<void *> owned, owned_sam, pinned;
};

struct aim_device_ctx {
    int dev = -1;
    std::vector<aim_slot> slots;
    char *d_ref = nullptr;   // AIM_FLAG_REF_TEXTS: the reference (+ zeroed tail slack), kept across aim_set_configure
    uint64_t ref_len = 0;
    aim::capi::Plan plan;    // made at configure time for max_pairs under the set's knobs and this device's budget
    aim::capi::Plan plan2;   // AIM_FLAG_READ_GROUPS: plan is the score-only pass's, plan2 the second pass's
    uint64_t budget = 0;     // scratch bound of one slot of this device, frozen at configure time
    float h2d_ms = 0.f, kernel_ms = 0.f, d2h_ms = 0.f;   // aim_set_submit / aim_set_wait: phase times of this device's batches, summed
};

struct aim_set {
    std::vector<aim_device_ctx> devs;
    aim::capi::XParams xparams;      // the params with their extension (aim_hip.h AIM_FLAG_ENDSFREE / AIM_FLAG_AFFINE2P); xparams.base is what the plans read
    const aim_params_t &params = xparams.base;
    uint32_t max_pairs = 0, max_raw = 0, max_runs = 0;
    bool configured = false;
    aim::Knobs knobs;        // AIM_* switches as read by the last aim_set_configure; launches never re-read the environment
    float h2d_ms = 0.f, kernel_ms = 0.f, d2h_ms = 0.f;
};

namespace aim {
namespace capi {
// (the one refusal text two units use: aim_align_device[_ref] in capi_launch.hip, the stateless groups entry points in capi_groups.hip)
inline constexpr const char *kSamStateless = "AIM_FLAG_SAM_FIELDS is set: the records come from aim_set_submit (aim_batch_io_sam_t) or, after a flag-less call, from aim_sam_device";
inline size_t req_size(const aim_params_t &p) { return (p.flags & AIM_FLAG_REQ8) ? sizeof(aim_request8_t) : sizeof(aim_request_t); }
inline size_t res_size(const aim_params_t &p) { return (p.flags & AIM_FLAG_RES8) ? sizeof(aim_result8_t) : sizeof(aim_result_t); }

// Enqueue the launches of plan `pl`. AIM_FLAG_WFA_ESCALATE with two stages: the lane plan at cap esc_c over the batch, the list of the
// pairs it left at esc_c + 1 (ascending pair order), the full-cap plan over that list -- one stream, no host round trip.
int launch(const Plan &pl, const aim::Knobs &kn, const aim_params_t &p, const LaunchIo &io, hipStream_t stream, const FusedIo *fio = nullptr,
           AuxStream *slot_aux = nullptr);
// One Stage (a general kernel) over the device-side list `todo` {count @0, pair ids @16..} of the batch io, whose ASCII rows are io.pat / io.txt
int launch_todo_stage(const aim_params_t &p, const Stage &st, const LaunchIo &io, const uint32_t *todo, hipStream_t stream);
void aux_stream_destroy(AuxStream &a);
// What every submit does to its slot before it enqueues: the batch becomes the slot's, nothing of an earlier one is left (n_pairs and
// n_reads are the caller's)
void reset_slot(aim_slot &s, const aim_batch_io_t *io);
// ... and the copies back of the batch's `rows` output rows: compact CIGAR with its cursor (and the runs known by now), results, ops rows
int enqueue_rows_d2h(const aim_params_t &p, aim_slot &s, uint32_t rows);
// What a failed submit ends in: nothing of it stays in flight on the slot's stream, and aim_last_error() keeps the enqueue's message.
int fail_drained(aim_slot &s, int rc);
int check_windows(const aim_params_t &p, uint32_t n_pairs, const void *requests, const uint64_t *text_pos, uint64_t ref_len, uint32_t *bad_pair);
int check_sam_io(const aim_set *set, const aim_slot &s, const aim_batch_io_t *io, const aim_batch_io_sam_t **sio);
int enqueue_sam_on_slot(const aim_set *set, const aim_device_ctx &d, aim_slot &s, const aim_batch_io_sam_t *sio, uint32_t n_rows, const uint32_t *sel);
int enqueue_sam_d2h(aim_slot &s, uint32_t n_rows);
// aim_set_submit under AIM_FLAG_READ_GROUPS (capi_groups.hip)
int submit_groups(aim_set *set, aim_device_ctx &d, aim_slot &s, const aim_batch_io_t *io);
}  // namespace capi
}  // namespace aim
#pragma GCC visibility pop
