// plan.hpp -- what the rest of the library sees of the launch planner (capi_plan.hip): the plan types, the accessors of an
// aim_params_t's flags and extensions, and the planner's entry points. Internal, not installed. The types cross units (aim_slot and
// aim_device_ctx of aim_capi.hip embed a Plan by value), so they live in aim::capi and not in an anonymous namespace. Every function
// declared here has ONE definition, in capi_plan.hip; read_knobs(), with_chip() and check_align_params() (capi_common.hpp) are there too.
#pragma once
#include <cstring>

#include "capi_common.hpp"
#include "wfa_group.hpp"   // GroupCfg (the kernels stay in tu_wfa_group.hip)

namespace aim {
namespace capi {
#pragma GCC visibility push(hidden)
enum KernelId { K_WFA_WAVE = 0, K_WFA_LANE = 1, K_DP_LANE = 2, K_DP_WAVE = 3, K_WFA_GROUP = 4, K_GENASM = 5, K_WFA_LANE_PK = 6, K_DP_STRIP = 7, K_DP_REG = 8, K_DP_GROUP = 9, K_WFA_BIDIR = 10 };

// What a launch is asked to consume / produce besides the default ABI (ASCII rows in, result_t + ops rows out). A plan
// honours a mode bit only when its kernel can (Plan::pk / Plan::emits_runs); otherwise the caller runs the conversion
// kernels of batch_io.hpp around the launch.
enum : uint32_t { MODE_PACKED_IN = 1u, MODE_RUNS_OUT = 2u };

// One kernel launch of a plan: its main kernel, or the general kernel that drains the main kernel's to-do list.
struct Stage {
    KernelId kid;
    uint32_t grid;          // workgroups
    uint32_t block;         // threads per workgroup
    size_t lds;             // dynamic LDS bytes
    uint64_t scratch_per_wg;   // KArgs::scratch_per_wave
    size_t scratch_at;      // where the stage's scratch starts
    uint32_t pool_cap, meta_cap, ring_slots, slot_w;   // K_WFA_WAVE (wfa_wave_plan)
    bool seq_lds;           // K_WFA_WAVE: both sequences staged in LDS
    int strip_k;            // K_DP_STRIP: cells per lane
    int seq;                // K_DP_LANE: where the pattern row lives, 0 global memory, 1 LDS image, 2 registers (dp_lane_plan)
};

struct StagePlan {
    Stage main;
    Stage fb;               // the to-do pass behind the main kernel (wfa_wave, dp_lane or dp_strip); planned iff todo_bytes != 0
    // the scratch layout, offsets from its base
    size_t scratch_total;
    size_t todo_at, todo_bytes;   // to-do region {count @0, pair ids @16..} the main kernel fills and the fallback drains
    size_t hist_at, hist_bytes;   // K_WFA_GROUP + BACKTRACE: history regions (one per pair of a chunk; two alternating buffers when chunked)
    size_t flags_at, pack_p_at, pack_t_at;   // pack_first: non-ACGT flag bits, packed patterns, packed texts
    uint32_t chunk_pairs;   // K_WFA_GROUP + BACKTRACE: pairs per compute + traceback launch (their history regions fit the scratch bound)
    aim::GroupCfg gcfg;     // K_WFA_GROUP
    int group_g;
    bool pack_first;        // K_WFA_LANE_PK on a batch of ASCII rows: pack_rows_kernel first
    bool pk;                // the kernel reads the packed rows of the batch itself (no unpack pass)
    bool emits_runs;        // the kernel writes aim_cigar_t + runs itself (no ops rows, no cigar_rle_kernel)
    int bidir_t;            // K_WFA_BIDIR: the base-case threshold T (fb is wfa_wave at MAX_SCORE min(MAX_SCORE, T), run first)
};

// A plan is one StagePlan. AIM_FLAG_WFA_ESCALATE with a cap c > 0 makes it two: the base is the lane plan at MAX_SCORE c over the whole
// batch, s2 the flag-less full-cap plan over the list of pairs the first stage left at c + 1 (batch_io.hpp escalate_select_kernel).
// [stage 1 | stage 2 | list {count @0, pair ids @16..} | ballot masks | workgroup counts]; scratch_total covers all of it.
struct Plan : StagePlan {
    bool esc;               // AIM_FLAG_WFA_ESCALATE is set (the plan line ends in escalate=<esc_c>)
    int esc_c;              // the first stage's cap; 0: one stage, the flag-less plan
    StagePlan s2;
    size_t s1_scratch;      // the first stage's own scratch_total
    size_t s2_at, list_at, mask_at, count_at;
};

// AIM_FLAG_ENDSFREE / AIM_FLAG_AFFINE2P: the params are the base of an aim_endsfree_params_t / aim_affine2p_params_t (aim_hip.h).
// Every copy this library keeps of a caller's params is a whole XParams (aim_set::xparams), which holds either extension, so the
// casts are valid wherever the flags are set.
struct EndsFree { int pb = 0, pe = 0, tb = 0, te = 0; };
inline bool is_endsfree(const aim_params_t &p) { return (p.flags & AIM_FLAG_ENDSFREE) != 0; }
inline EndsFree ends_free(const aim_params_t &p)
{
    EndsFree e;
    if (!is_endsfree(p)) return e;
    const aim_endsfree_params_t &x = *reinterpret_cast<const aim_endsfree_params_t *>(&p);
    e.pb = x.pattern_begin_free; e.pe = x.pattern_end_free; e.tb = x.text_begin_free; e.te = x.text_end_free;
    return e;
}
struct Affine2p { int o2 = 0, e2 = 0; };
inline bool is_affine2p(const aim_params_t &p) { return (p.flags & AIM_FLAG_AFFINE2P) != 0; }
inline Affine2p affine2p(const aim_params_t &p)
{
    Affine2p g;
    if (!is_affine2p(p)) return g;
    const aim_affine2p_params_t &x = *reinterpret_cast<const aim_affine2p_params_t *>(&p);
    g.o2 = x.gap_o2; g.e2 = x.gap_e2;
    return g;
}
// AIM_FLAG_LINEAR: gap-linear WFA on aim_params_t itself (no extension): gap_o = 0, gap_e is the cost of one gap base.
inline bool is_linear(const aim_params_t &p) { return (p.flags & AIM_FLAG_LINEAR) != 0; }
// AIM_FLAG_WFA_W32: int32 wavefront offsets (AFFINE_WAVEFRONT_W32), wfa_wave_kernel only.
inline bool is_w32(const aim_params_t &p) { return (p.flags & AIM_FLAG_WFA_W32) != 0; }
// AIM_FLAG_WFA_BIDIR: bidirectional WFA with CIGAR (wfa_bidir.hpp).
inline bool is_bidir(const aim_params_t &p) { return (p.flags & AIM_FLAG_WFA_BIDIR) != 0; }
// aim_align_device_ref: the gathered text rows sit behind the plan's scratch, 256-B aligned, with 256 B of tail slack
inline size_t ref_rows_at(size_t plan_scratch) { return (plan_scratch + 255) & ~(size_t)255; }
inline size_t ref_rows_bytes(const aim_params_t &p, uint32_t n_pairs) { return (size_t)n_pairs * (size_t)p.read_size + 256; }
// AIM_FLAG_READ_GROUPS: reads and their candidates (groups.hpp); the plans of its two passes never see the flag.
inline bool is_groups(const aim_params_t &p) { return (p.flags & AIM_FLAG_READ_GROUPS) != 0; }
// AIM_FLAG_MATE_PAIRS: paired-end selection over a groups batch (mates.hpp); one more kernel after the independent selection.
inline bool is_mates(const aim_params_t &p) { return (p.flags & AIM_FLAG_MATE_PAIRS) != 0; }
// AIM_FLAG_WFA_ESCALATE: a lane kernel at a low cap over the batch, the flag-less plan over the pairs it left over that cap (plan_wfa).
inline bool is_escalate(const aim_params_t &p) { return (p.flags & AIM_FLAG_WFA_ESCALATE) != 0; }
// AIM_FLAG_SAM_FIELDS: SAM-ready records from the final ops rows (sam_fields.hpp); one more kernel behind the batch, no plan depends on it
// beyond keeping the ops rows on the device (no fused run output).
inline bool is_sam(const aim_params_t &p) { return (p.flags & AIM_FLAG_SAM_FIELDS) != 0; }
// AIM_FLAG_TOP_HITS: the N best candidates per read (hits.hpp); the rows behind the selection are hits, not reads.
inline bool is_hits(const aim_params_t &p) { return (p.flags & AIM_FLAG_TOP_HITS) != 0; }
// The params as this library keeps them: room for either extension, and the extension copied only when a flag says it exists.
union XParams {
    aim_params_t base;
    aim_endsfree_params_t ef;
    aim_affine2p_params_t a2p;
};
inline XParams copy_params(const aim_params_t &p)
{
    XParams x;
    memset(&x, 0, sizeof x);
    if (is_endsfree(p)) x.ef = *reinterpret_cast<const aim_endsfree_params_t *>(&p);
    else if (is_affine2p(p)) x.a2p = *reinterpret_cast<const aim_affine2p_params_t *>(&p);
    else x.base = p;
    return x;
}

inline size_t stage_bytes(const Stage &st) { return (size_t)(st.scratch_per_wg * st.grid); }

// ---- AIM_FLAG_READ_GROUPS -------------------------------------------------------------------------------------------------
// Pass 1 aligns every candidate under the configured flags minus BACKTRACE, WFA_BIDIR and RES8 (result_t rows: the selection needs
// the status); pass 2 runs the configured flags on the winners only (BACKTRACE only: without it the selected pass-1 rows are the
// answer). Both keep the params' extension (XParams), and neither carries AIM_FLAG_READ_GROUPS.
struct GroupsPlan {
    XParams x1, x2;         // the two passes' params
    Plan p1, p2;            // p2 planned iff pass2
    bool pass2;
    bool mates;             // AIM_FLAG_MATE_PAIRS: mate_select_kernel after the independent selection
    bool sam;               // AIM_FLAG_SAM_FIELDS: the reads' records after the second pass
    bool hits;              // AIM_FLAG_TOP_HITS: hit_select_kernel after the selection; the rows behind it are hits
    size_t plan_bytes;      // the larger of the two plans' scratch (both made for n_pairs)
    // aim_align_device_groups: the rest of its scratch, offsets from the base (256-B aligned)
    size_t cand_p_at, cand_t_at, res1_at, map_at, sel_at, req2_at, pat2_at, txt2_at, total;
    size_t best_at;         // aim_align_device_mates: the independent selection's rows when the caller keeps none (the last region)
    size_t hit_at;          // aim_align_device_hits: the hit list when the caller keeps none (the last region)
};

// The planner (capi_plan.hip). Pure host logic: nothing below enqueues work or reads batch data.
uint64_t budget_from_free(size_t free_b);                  // the scratch bound of a device with free_b bytes free
uint64_t stateless_budget_bytes(const aim::Knobs &kn);     // ... of the stateless entry points: read once per process and device
int validate_params(const aim_params_t &p);
int plan_wfa_wave(const aim_params_t &p, uint32_t n_pairs, const aim::Knobs &kn, uint64_t budget, Stage *st);
int describe_plan(const Plan &pl, const aim_params_t &p, uint32_t n_pairs, uint64_t budget, char *out, size_t cap);
int make_plan(const aim_params_t &p, uint32_t n_pairs, const aim::Knobs &kn, uint64_t budget, Plan *pl, uint32_t mode = 0u);
XParams groups_pass_params(const aim_params_t &p, uint32_t drop);
int describe_groups(const GroupsPlan &g, uint32_t n_pairs, uint32_t n_reads, uint64_t budget, char *out, size_t cap);
int make_groups_plan(const aim_params_t &p, uint32_t n_pairs, const aim::Knobs &kn, uint64_t budget, GroupsPlan *g);
#pragma GCC visibility pop
}  // namespace capi
}  // namespace aim
