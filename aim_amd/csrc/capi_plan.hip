// capi_plan.hip -- the launch planner of the C-ABI (plan.hpp): from an aim_params_t, a pair count, the knobs and a scratch budget to a
// Plan and the line that describes it. Pure host logic: nothing here enqueues work or reads batch data. The plan inputs that carry
// process-wide state live here with it -- the AIM_* environment (read_knobs), the CU count per device (chip_cus) and the stateless
// entry points' scratch budget per device -- and so do the three entry points that only plan: aim_scratch_bytes, aim_plan_describe
// and aim_kernel_name. Launching, device sets and the alignment entry points are in aim_capi.hip.
// The alignment-kernel headers below give their *_plan, *_supported and size functions; their kernels stay in the tu_*.hip units.
// Of the batch-I/O kernels the planner needs the region sizes (batch_sizes.hpp) and packed_row_dwords (batch_io.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "plan.hpp"
#include "wfa_wave.hpp"
#include "wfa_bidir.hpp"
#include "wfa_lane.hpp"
#include "wfa_lane_packed.hpp"
#include "wfa_group.hpp"
#include "dp_lane.hpp"
#include "dp_wave.hpp"
#include "dp_strip.hpp"
#include "dp_reg.hpp"
#include "dp_group.hpp"
#include "batch_io.hpp"
#include "genasm_wave.hpp"

using namespace aim::capi;

namespace {

// ---------------------------------------------------------------------------
// launch planning
// ---------------------------------------------------------------------------

// The AIM_* environment variables, read HERE and nowhere else (see aim::Knobs, aim_device.hpp).
int env_int(const char *name, int unset)
{
    const char *e = getenv(name);
    return (e && *e) ? atoi(e) : unset;
}
bool env_flag(const char *name)
{
    const char *e = getenv(name);
    return e && e[0] == '1';
}
}  // namespace
aim::Knobs aim::capi::read_knobs()
{
    aim::Knobs k;
    if (const char *e = getenv("AIM_SCRATCH_GB")) k.scratch_gb = std::max(0.25, atof(e));
    k.force_wave = env_flag("AIM_FORCE_WAVE");
    k.no_group = env_flag("AIM_NO_GROUP");
    k.no_lane_ext = env_flag("AIM_NO_LANE_EXT");
    k.no_lane = env_flag("AIM_NO_LANE");
    k.no_lane_pk = env_flag("AIM_NO_LANE_PK");
    k.group_overlap = env_flag("AIM_GROUP_OVERLAP");
    k.wfa_no_ring = env_flag("AIM_WFA_NO_RING");
    k.wfa_slotw = env_int("AIM_WFA_SLOTW", -1);
    k.force_dpwave = env_flag("AIM_FORCE_DPWAVE");
    k.dpw_legacy = env_flag("AIM_DPW_LEGACY");
    k.strip_k = env_int("AIM_STRIP_K", -1);
    k.dpw_nw = env_int("AIM_DPW_NW", -1);
    k.dpl_seq_lds = env_int("AIM_DPL_SEQ_LDS", -1);
    k.dpl_no_reg = env_int("AIM_DPL_NO_REG", 0);
    k.dpl_per_cu = env_int("AIM_DPL_PER_CU", -1);
    k.no_nw_reg = env_flag("AIM_NO_NW_REG");
    k.no_swg_reg = env_flag("AIM_NO_SWG_REG");
    k.no_dp_group = env_flag("AIM_NO_DP_GROUP");
    k.dpg_per_cu = env_int("AIM_DPG_PER_CU", -1);
    k.dbg_flags = env_int("AIM_DEBUG_FLAGS", 0);
#ifndef AIM_DIAG_BUILD   // bits 1 / 4 / 8 make kernels skip work (a traceback walk, the direction-bit stores, the bits themselves) and return WRONG results with status OK:
    k.dbg_flags &= 2;    // they exist in diagnostic builds only (python -m aim_amd.build --variant diag --flags "-DAIM_DIAG_BUILD=1"). Bit 2 changes the route, not the result.
#endif
    k.nw_reg_per_cu = env_int("AIM_NW_REG_PER_CU", -1);
    k.group_lds_kb = env_int("AIM_GROUP_LDS_KB", -1);
    k.group_g = env_int("AIM_GROUP_G", -1);
    k.group_per_cu = env_int("AIM_GROUP_PER_CU", -1);
    k.group_wlds = env_int("AIM_GROUP_WLDS", -1);
    k.group_unit1 = env_int("AIM_GROUP_UNIT1", 0);
    k.ga_per_cu = env_int("AIM_GA_PER_CU", 0);
    k.poison_scratch = env_int("AIM_DEBUG_POISON_SCRATCH", -1);
    k.poison_ops = env_int("AIM_DEBUG_POISON_OPS", -1);
    k.poison_lds = env_int("AIM_DEBUG_POISON_LDS", -1);
    k.sam_wave_min = env_int("AIM_SAM_WAVE_MIN", -1);
    k.class_g = env_int("AIM_CLASS_G", -1);
    k.plan_debug = getenv("AIM_PLAN_DEBUG") != nullptr;
    k.cus = (uint32_t)std::max(0, env_int("AIM_CHIP_CUS", 0));   // 0: ask the device (chip_cus)
    return k;
}
namespace {

// Compute units of the CURRENT device, read once per device (256 on a whole MI355X; a DPX / QPX / CPX partition or a CU-reduced part
// reports fewer and every persistent grid shrinks with it). Without a device (planning queries on a CPU-only host) the whole chip.
uint32_t chip_cus()
{
    static uint32_t cached[64] = {0};
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
        (void)hipGetLastError();
        return 256;
    }
    if (!cached[dev]) {
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) {
            (void)hipGetLastError();
            return 256;
        }
        cached[dev] = (uint32_t)n;
    }
    return cached[dev];
}
}  // namespace
// Knobs for a plan on the current device: AIM_CHIP_CUS wins, else the device's own count.
aim::Knobs aim::capi::with_chip(aim::Knobs k)
{
    if (k.cus == 0) k.cus = chip_cus();
    return k;
}

// Upper bound on the HBM scratch one plan may ask for (DP tables, WFA history/pools). AIM_SCRATCH_GB overrides. Plans
// are need-capped, so the bound only matters where the tables are huge: config 4 (l = 10 000, 613 MB per pair) runs 128
// pairs in 5 rounds under a 16 GB bound and in 1 round (4.4x faster) from 80 GB up; a full chip of them (256 pairs, one
// per CU) needs 157 GB, which is why the default is 3/4 of the free memory and not 1/2.
//  * device sets: the bound is taken per device inside aim_set_configure, AFTER the set's fixed buffers are allocated,
//    and frozen in the set together with the plan;
//  * stateless entry points (aim_scratch_bytes, then aim_align_device with the buffer the caller allocated in between):
//    the bound must not move between the two calls, so it is read once per process and device.
uint64_t aim::capi::budget_from_free(size_t free_b) { return std::max<uint64_t>((uint64_t)free_b / 4 * 3, (uint64_t)1 << 28); }

uint64_t aim::capi::stateless_budget_bytes(const aim::Knobs &kn)
{
    if (kn.scratch_gb >= 0) return (uint64_t)(kn.scratch_gb * (double)(1ull << 30));
    static uint64_t cached[64] = {0};
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) {
        (void)hipGetLastError();
        return (uint64_t)16 << 30;                           // no device (CPU-only host): planning queries still answer
    }
    if (!cached[dev]) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess || free_b == 0) {
            (void)hipGetLastError();
            return (uint64_t)16 << 30;
        }
        cached[dev] = budget_from_free(free_b);
    }
    return cached[dev];
}

int aim::capi::validate_params(const aim_params_t &p)
{
    if (p.algo != AIM_ALGO_NW && p.algo != AIM_ALGO_SWG && p.algo != AIM_ALGO_WFA && p.algo != AIM_ALGO_GENASM)
        return fail(AIM_EINVAL, "unknown algorithm %d", p.algo);
    // before either extension is read: the caller's struct holds at most one of them (an aim_affine2p_params_t is shorter than
    // an aim_endsfree_params_t)
    if (is_endsfree(p) && is_affine2p(p)) return fail(AIM_EINVAL, "AIM_FLAG_AFFINE2P cannot be combined with AIM_FLAG_ENDSFREE");
    if (is_mates(p)) {   // the positions it pairs by are the windows' text_pos
        if (!is_groups(p)) return fail(AIM_EINVAL, "AIM_FLAG_MATE_PAIRS needs AIM_FLAG_READ_GROUPS");
        if (!is_ref(p)) return fail(AIM_EINVAL, "AIM_FLAG_MATE_PAIRS needs AIM_FLAG_REF_TEXTS");
    }
    if (is_hits(p)) {
        if (!is_groups(p)) return fail(AIM_EINVAL, "AIM_FLAG_TOP_HITS needs AIM_FLAG_READ_GROUPS");
        if (is_mates(p)) return fail(AIM_EINVAL, "AIM_FLAG_TOP_HITS cannot be combined with AIM_FLAG_MATE_PAIRS (a follow-up)");
        if (is_sam(p))
            return fail(AIM_EINVAL, "AIM_FLAG_TOP_HITS cannot be combined with AIM_FLAG_SAM_FIELDS (a follow-up: aim_sam_device works on hit rows with d_sel = d_hit_pair)");
    }
    if (is_sam(p)) {   // the records are on the reference's coordinates and come from the ops rows
        if (p.flags & AIM_FLAG_RES8) return fail(AIM_EINVAL, "AIM_FLAG_SAM_FIELDS cannot be combined with AIM_FLAG_RES8");
        if (p.algo == AIM_ALGO_GENASM)
            return fail(AIM_EINVAL, "AIM_FLAG_SAM_FIELDS cannot be combined with AIM_ALGO_GENASM (its windowed walk is unpinned and begin_offset = 0 is another contract)");
        if (!is_ref(p)) return fail(AIM_EINVAL, "AIM_FLAG_SAM_FIELDS needs AIM_FLAG_REF_TEXTS");
        if (!(p.flags & AIM_FLAG_BACKTRACE)) return fail(AIM_EINVAL, "AIM_FLAG_SAM_FIELDS needs AIM_FLAG_BACKTRACE");
    }
    if (is_escalate(p)) {
        if (p.algo != AIM_ALGO_WFA) return fail(AIM_EINVAL, "AIM_FLAG_WFA_ESCALATE needs AIM_ALGO_WFA");
        if (is_endsfree(p)) return fail(AIM_EINVAL, "AIM_FLAG_WFA_ESCALATE cannot be combined with AIM_FLAG_ENDSFREE");
        if (is_affine2p(p)) return fail(AIM_EINVAL, "AIM_FLAG_WFA_ESCALATE cannot be combined with AIM_FLAG_AFFINE2P");
        if (is_linear(p)) return fail(AIM_EINVAL, "AIM_FLAG_WFA_ESCALATE cannot be combined with AIM_FLAG_LINEAR");
        if (is_w32(p)) return fail(AIM_EINVAL, "AIM_FLAG_WFA_ESCALATE cannot be combined with AIM_FLAG_WFA_W32");
        if (is_bidir(p)) return fail(AIM_EINVAL, "AIM_FLAG_WFA_ESCALATE cannot be combined with AIM_FLAG_WFA_BIDIR");
        if (is_groups(p)) return fail(AIM_EINVAL, "AIM_FLAG_WFA_ESCALATE cannot be combined with AIM_FLAG_READ_GROUPS (a follow-up)");
    }
    if (is_linear(p)) {
        if (p.algo != AIM_ALGO_WFA) return fail(AIM_EINVAL, "AIM_FLAG_LINEAR needs AIM_ALGO_WFA");
        if (p.flags & AIM_FLAG_REDUCE) return fail(AIM_EINVAL, "AIM_FLAG_LINEAR cannot be combined with AIM_FLAG_REDUCE");
        if (is_endsfree(p)) return fail(AIM_EINVAL, "AIM_FLAG_LINEAR cannot be combined with AIM_FLAG_ENDSFREE");
        if (is_affine2p(p)) return fail(AIM_EINVAL, "AIM_FLAG_LINEAR cannot be combined with AIM_FLAG_AFFINE2P");
    }
    if (is_w32(p) && p.algo != AIM_ALGO_WFA) return fail(AIM_EINVAL, "AIM_FLAG_WFA_W32 needs AIM_ALGO_WFA");
    if (is_bidir(p)) {
        if (p.algo != AIM_ALGO_WFA) return fail(AIM_EINVAL, "AIM_FLAG_WFA_BIDIR needs AIM_ALGO_WFA");
        if (!(p.flags & AIM_FLAG_BACKTRACE)) return fail(AIM_EINVAL, "AIM_FLAG_WFA_BIDIR needs AIM_FLAG_BACKTRACE (score-only WFA is O(s) already)");
        if (p.flags & AIM_FLAG_REDUCE) return fail(AIM_EINVAL, "AIM_FLAG_WFA_BIDIR cannot be combined with AIM_FLAG_REDUCE");
        if (is_endsfree(p)) return fail(AIM_EINVAL, "AIM_FLAG_WFA_BIDIR cannot be combined with AIM_FLAG_ENDSFREE");
        if (is_affine2p(p)) return fail(AIM_EINVAL, "AIM_FLAG_WFA_BIDIR cannot be combined with AIM_FLAG_AFFINE2P");
        if (is_linear(p)) return fail(AIM_EINVAL, "AIM_FLAG_WFA_BIDIR cannot be combined with AIM_FLAG_LINEAR");
        if (std::max(p.mismatch, p.gap_o + p.gap_e) + 1 > aim::kBidirMaxScope)
            return fail(AIM_EINVAL, "AIM_FLAG_WFA_BIDIR needs max(x, o + e) < %d", aim::kBidirMaxScope);
    }
    // The reference's recurrence starts a cell no present source covers at -10, not NULL (wfa.c:231-266), and every WFA kernel copies that.
    // Where (10 + k) * x < o + k * e for some gap length k -- o + e > 11 x, or e > x -- such a cell is a real offset before the gap that
    // leads there is paid for, and the score can lie below the minimum cost. Global WFA returns that score, as the reference does; the three
    // flags whose contract is a minimum cost are refused, whatever READ_SIZE is (short rows only make the gaps that show it rare, not absent).
    if (p.algo == AIM_ALGO_WFA && !is_linear(p) && (is_endsfree(p) || is_affine2p(p) || is_bidir(p)) &&
        (p.gap_o + p.gap_e > 11 * p.mismatch || p.gap_e > p.mismatch))
        return fail(AIM_EINVAL, "%s needs gap_o + gap_e <= 11 * mismatch and gap_e <= mismatch: beyond that the reference's -10 start value makes WFA's score "
                    "fall below the minimum cost (got x = %d, o = %d, e = %d)",
                    is_endsfree(p) ? "AIM_FLAG_ENDSFREE" : is_affine2p(p) ? "AIM_FLAG_AFFINE2P" : "AIM_FLAG_WFA_BIDIR", p.mismatch, p.gap_o, p.gap_e);
    if (p.read_size <= 0 || (p.read_size & 7)) return fail(AIM_EINVAL, "read_size must be a positive multiple of 8 (got %d)", p.read_size);
    if (p.max_score < 0) return fail(AIM_EINVAL, "max_score must be >= 0");
    if ((p.flags & AIM_FLAG_REQ8) && p.read_size >= 32760)
        return fail(AIM_EINVAL, "AIM_FLAG_REQ8 carries int16 lengths: read_size must be < 32760");
    if (p.algo == AIM_ALGO_GENASM) {   // no penalties, no score cap; lengths are int32
        if (is_endsfree(p)) return fail(AIM_EINVAL, "AIM_FLAG_ENDSFREE needs AIM_ALGO_WFA");
        if (is_affine2p(p)) return fail(AIM_EINVAL, "AIM_FLAG_AFFINE2P needs AIM_ALGO_WFA");
        if ((p.flags & AIM_FLAG_RES8) && (p.flags & AIM_FLAG_BACKTRACE))
            return fail(AIM_EINVAL, "AIM_FLAG_RES8 (idx, score results) cannot be combined with AIM_FLAG_BACKTRACE");
        if (p.read_size > (1 << 24)) return fail(AIM_EINVAL, "read_size must be <= 2^24");
        return AIM_OK;
    }
    // same admission rule as the launchers (run-wfa-pim-wram.py:41-43): m <= 0 and x, g, a > 0
    if (p.algo == AIM_ALGO_NW) {
        if (p.mismatch <= 0 || p.gap_i <= 0 || p.gap_d <= 0) return fail(AIM_EINVAL, "NW penalties must be x, g > 0");
    } else if (is_linear(p)) {
        if (p.match > 0 || p.mismatch <= 0 || p.gap_o != 0 || p.gap_e <= 0)
            return fail(AIM_EINVAL, "gap-linear penalties must be m <= 0, gap_o = 0 and x, gap_e > 0 (got %d,%d,%d,%d)", p.match, p.mismatch,
                        p.gap_o, p.gap_e);
    } else {
        if (p.match > 0 || p.mismatch <= 0 || p.gap_o <= 0 || p.gap_e <= 0)
            return fail(AIM_EINVAL, "Wrong affine gap penalties must be  m <= 0 and g, a, x > 0");
    }
    if ((p.flags & AIM_FLAG_RES8) && (p.flags & AIM_FLAG_BACKTRACE))
        return fail(AIM_EINVAL, "AIM_FLAG_RES8 (idx, score results) cannot be combined with AIM_FLAG_BACKTRACE");
    if (is_endsfree(p)) {
        if (p.algo != AIM_ALGO_WFA) return fail(AIM_EINVAL, "AIM_FLAG_ENDSFREE needs AIM_ALGO_WFA");
        if (p.flags & AIM_FLAG_REDUCE) return fail(AIM_EINVAL, "AIM_FLAG_ENDSFREE cannot be combined with AIM_FLAG_REDUCE");
        const EndsFree e = ends_free(p);
        if (e.pb < 0 || e.pe < 0 || e.tb < 0 || e.te < 0)
            return fail(AIM_EINVAL, "ends-free lengths must be >= 0 (got %d,%d,%d,%d)", e.pb, e.pe, e.tb, e.te);
    }
    if (is_affine2p(p)) {
        if (p.algo != AIM_ALGO_WFA) return fail(AIM_EINVAL, "AIM_FLAG_AFFINE2P needs AIM_ALGO_WFA");
        if (p.flags & AIM_FLAG_REDUCE) return fail(AIM_EINVAL, "AIM_FLAG_AFFINE2P cannot be combined with AIM_FLAG_REDUCE");
        const Affine2p g = affine2p(p);
        if (g.o2 <= 0 || g.e2 <= 0) return fail(AIM_EINVAL, "affine2p penalties must be gap_o2, gap_e2 > 0 (got %d,%d)", g.o2, g.e2);
    }
    // AIM_FLAG_WFA_W32: int32 offsets (AFFINE_WAVEFRONT_W32, common.h:101-104); lengths are int32 as for GenASM
    if (is_w32(p)) {
        if (p.read_size > (1 << 24)) return fail(AIM_EINVAL, "read_size must be <= 2^24");
        return AIM_OK;
    }
    // the reference's lengths, WFA offsets and NW / SWG cells are int16 (WFA/DPU-WRAM/common/common.h:98-100, 174-175): what it admits
    // is < 32 767; READ_SIZE is a multiple of 8
    if (p.read_size >= 32760)
        return fail(AIM_EINVAL, "%s are int16: read_size must be < 32760", p.algo == AIM_ALGO_WFA ? "WFA offsets (common.h:98-100)" : "NW/SWG cells");
    return AIM_OK;
}

int aim::capi::check_align_params(const aim_params_t &p) { return validate_params(p); }

namespace {

inline bool p_is_nw(const aim_params_t *p) { return p->algo == AIM_ALGO_NW; }


// GenASM: one pair per wavefront; slow-path columns in one slab per wavefront
int plan_genasm(const aim_params_t &p, uint32_t n_pairs, const aim::Knobs &kn, Plan *pl)
{
    Stage &m = pl->main;
    m.kid = K_GENASM;
    aim::genasm_plan(p, kn, n_pairs, &m.grid, &m.block, &m.lds);
    m.scratch_per_wg = aim::kGaSlabBytes;
    pl->scratch_total = stage_bytes(m);
    return AIM_OK;
}
}  // namespace

int aim::capi::plan_wfa_wave(const aim_params_t &p, uint32_t n_pairs, const aim::Knobs &kn, uint64_t budget, Stage *st)
{
    const EndsFree e = ends_free(p);
    const Affine2p g = affine2p(p);
    aim::WfaWavePlan w;
    switch (aim::wfa_wave_plan(p, n_pairs, kn, budget, e.pb, e.tb, g.o2, g.e2, &w)) {
    case aim::kWfaWaveNoPool: return fail(AIM_ENOMEM, "scratch budget too small for max_score %d", p.max_score);
    case aim::kWfaWaveNoScore0:
        return fail(AIM_ENOMEM, "scratch budget too small for the ends-free score-0 wavefront (%llu diagonals)", (unsigned long long)(w.wide + 1));
    case aim::kWfaWaveNoWindow: return fail(AIM_ENOMEM, "scratch budget too small for the live window of max_score %d", p.max_score);
    }
    st->kid = K_WFA_WAVE;
    st->grid = w.grid;
    st->block = 64;
    st->lds = w.lds;
    st->scratch_per_wg = w.scratch_per_wg;
    st->pool_cap = w.pool_cap;
    st->meta_cap = w.meta_cap;
    st->ring_slots = w.ring_slots;
    st->slot_w = w.slot_w;
    st->seq_lds = w.seq_lds;
    return AIM_OK;
}

namespace {

// wfa_group_kernel's shape; with BACKTRACE also the chunks of the batch whose history regions fit half of the scratch bound.
// False when LDS does not admit the shape or too few pairs would be in flight.
bool plan_wfa_group(const aim_params_t &p, uint32_t n_pairs, const aim::Knobs &kn, uint64_t budget, bool gpk, Plan *pl)
{
    const EndsFree e = ends_free(p);
    const Affine2p a2 = affine2p(p);
    Stage &m = pl->main;
    size_t hist_pair = 0;
    if (!aim::wfa_group_plan(p, n_pairs, kn, gpk, &pl->gcfg, &pl->group_g, &m.grid, &m.lds, &hist_pair, e.pb, e.tb, a2.o2, a2.e2))
        return false;
    m.kid = K_WFA_GROUP;
    m.block = 64;
    pl->chunk_pairs = n_pairs;
    if (!hist_pair) return true;
    // BACKTRACE: every pair of a launch keeps its history region until the traceback kernel has walked it. Launches are
    // chunks of the batch whose regions fit half of the scratch bound (one chunk whenever possible).
    // One launch when the regions fit. (AIM_GROUP_OVERLAP=1: chunks of two grid rounds, two alternating buffers of regions, the
    // traceback kernel of chunk c on a second stream while chunk c + 1 is computed. Measured and NOT adopted: cfg3 3.57 ->
    // 3.79 ms, l = 100 e = 5 % 1.62 -> 1.75 ms -- several shorter compute launches lose more to ramp-up and partial rounds than
    // the overlapped 10 % traceback gives back. Kept as a tested code path: it is also what a batch does whose regions do
    // not fit the scratch bound.)
    const uint64_t fit = (budget / 4) / hist_pair;          // per buffer
    if (fit < 4096 && fit < n_pairs) return false;   // too few pairs in flight to fill the chip: the general kernel's pools are smaller
    const uint64_t two_rounds = 2ull * m.grid * (uint64_t)(64 / pl->group_g);
    uint64_t chunk = std::min<uint64_t>(fit, std::max<uint64_t>(two_rounds, 4096));
    if (n_pairs <= 2 * fit && (chunk >= n_pairs || !kn.group_overlap)) chunk = n_pairs;   // one launch, one buffer of regions (half the bound)
    else if (!kn.group_overlap) chunk = fit;                                                  // as few launches as fit, over the two buffers
    uint32_t c = (uint32_t)chunk;
    if (c < n_pairs) c &= ~63u;
    const uint32_t nchunks = (n_pairs + c - 1) / c;
    pl->chunk_pairs = c;
    pl->hist_bytes = ((((size_t)c * hist_pair) + 255) & ~(size_t)255) * (nchunks > 1 ? 2 : 1);
    return true;
}

// WFA: a lane kernel where it takes the shape; else wfa_group, or wfa_lane_packed behind pack_rows_kernel, with wfa_wave over their
// to-do list; else wfa_wave alone. Ends-free, affine2p and gap-linear never run on the lane kernels (their wavefront shapes are fixed at compile
// time for the global case): wfa_group where LDS admits the wider rows / deeper rings, else wfa_wave.
// AIM_FLAG_WFA_BIDIR: wfa_wave_kernel at MAX_SCORE min(MAX_SCORE, T) first (every pair of score <= T gets the flag-less result and
// bytes from it), then wfa_bidir_kernel over the pairs it left over T. The two stages run one after the other on one stream and
// share one scratch region. Every READ_SIZE, both offset widths; no other stage.
int plan_wfa_bidir(const aim_params_t &p, uint32_t n_pairs, const aim::Knobs &kn, uint64_t budget, Plan *pl)
{
    const int T = aim::wfa_bidir_threshold(p);
    aim_params_t p1 = p;
    p1.flags &= ~AIM_FLAG_WFA_BIDIR;
    p1.max_score = std::min(p.max_score, T);
    int rc = plan_wfa_wave(p1, n_pairs, kn, budget, &pl->fb);
    if (rc) return rc;
    const int scope = std::max(p.mismatch, p.gap_o + p.gap_e) + 1;
    const int kw = (int)std::min<int64_t>((int64_t)p.max_score + 2 * scope + p.gap_o + p.gap_o + p.gap_e + 8, (int64_t)p.read_size + 2);
    Stage &m = pl->main;
    m.kid = K_WFA_BIDIR;
    m.block = 64;
    m.lds = aim::wfa_bidir_lds(T);
    m.scratch_per_wg = aim::wfa_bidir_wg_bytes(p, T, kw);
    m.pool_cap = (uint32_t)T;
    m.slot_w = (uint32_t)kw;
    pl->bidir_t = T;
    if (p.max_score <= T) {
        // the first stage is the whole alignment: the bidirectional kernel is not launched, needs no scratch and no grid (the plan
        // line says grid=0), and the budget is the first stage's alone
        m.scratch_per_wg = 0;
        m.grid = 0;
        pl->scratch_total = stage_bytes(pl->fb);
        return AIM_OK;
    }
    // persistent single-wave workgroups: what is resident by VGPRs (wfa_bidir_kernel's launch bound) and LDS
    const uint32_t wg_per_cu = (uint32_t)std::min<size_t>(aim::kBidirPerCu, aim::lds_workgroups_per_cu(m.lds));
    uint32_t grid = resident_grid(kn, wg_per_cu);
    const uint32_t need = ((n_pairs + 7u) / 8u) * 8u;
    if (grid > need) grid = std::max(8u, need);
    while (grid > 8 && (uint64_t)m.scratch_per_wg * grid > budget) grid -= 8;
    if ((uint64_t)m.scratch_per_wg * grid > budget) return fail(AIM_ENOMEM, "scratch budget too small for one bidirectional WFA workgroup (%llu bytes)", (unsigned long long)m.scratch_per_wg);
    m.grid = grid;
    pl->scratch_total = std::max(stage_bytes(m), stage_bytes(pl->fb));
    return AIM_OK;
}

int plan_wfa_flagless(const aim_params_t &p, uint32_t n_pairs, const aim::Knobs &kn, uint64_t budget, uint32_t mode, Plan *pl)
{
    if (is_bidir(p)) return plan_wfa_bidir(p, n_pairs, kn, budget, pl);
    if (is_w32(p)) {
        // int32 offsets exist in wfa_wave_kernel only (wfa_group / the lane kernels keep int16 rows): it runs alone at every READ_SIZE
        // and takes non-ACGT pairs itself, so there is no fallback stage. Below 32760 this costs speed and changes no result.
        int rc = plan_wfa_wave(p, n_pairs, kn, budget, &pl->main);
        pl->scratch_total = stage_bytes(pl->main);
        return rc;
    }
    const bool bt = p.flags & AIM_FLAG_BACKTRACE;
    const bool lanes = !is_endsfree(p) && !is_affine2p(p) && !is_linear(p) && !kn.force_wave && !kn.no_lane;   // a lane kernel may run
    const bool lane_pk_ok = lanes && !kn.no_lane_pk && aim::wfa_lane_packed_supported(p, !kn.no_lane_ext);
    Stage &m = pl->main;
    if ((mode & MODE_PACKED_IN) && lane_pk_ok) {
        // packed rows in; {idx, score}, compact CIGAR or result_t + ops rows out: one kernel per batch, no scratch (wfa_lane_packed.hpp)
        m.kid = K_WFA_LANE_PK;
        aim::wfa_lane_packed_plan(p, n_pairs, kn, &m.grid, &m.block, &m.lds);
        pl->scratch_total = 256;
        pl->pk = true;
        pl->emits_runs = bt && (mode & MODE_RUNS_OUT);
        return AIM_OK;
    }
    if (lanes && aim::wfa_lane_supported(p, !kn.no_lane_ext)) {
        // one pair per lane, everything in registers; no scratch, no second kernel (pairs with bytes outside A/C/G/T take
        // the kernel's own raw-byte path)
        m.kid = K_WFA_LANE;
        aim::wfa_lane_plan(p, n_pairs, kn, &m.grid, &m.block, &m.lds);
        m.scratch_per_wg = 256;
        pl->scratch_total = 256;   // unused; aim_scratch_bytes() keeps 0 for "invalid configuration"
#if AIM_LANE_STAMPS
        pl->scratch_total += (size_t)m.grid * 64;   // diagnostic builds park their s_memtime sums behind the first 256 bytes
#endif
        return AIM_OK;
    }
    const bool gpk = (mode & MODE_PACKED_IN) && !kn.no_lane_pk;   // the group kernel reads packed rows itself
    Plan grp;
    memset(&grp, 0, sizeof grp);
    const bool group_ok = !kn.force_wave && !kn.no_group && plan_wfa_group(p, n_pairs, kn, budget, gpk, &grp);
    if (!lane_pk_ok && !group_ok) {
        int rc = plan_wfa_wave(p, n_pairs, kn, budget, &m);
        pl->scratch_total = stage_bytes(m);
        return rc;
    }
    // a fast kernel, then wfa_wave over the pairs it left (its to-do list)
    if (!lane_pk_ok) *pl = grp;
    int rc = plan_wfa_wave(p, std::min<uint32_t>(n_pairs, 1024u * 64u), kn, budget, &pl->fb);
    if (rc) return rc;
    pl->todo_bytes = aim::wfa_lane_todo_bytes(n_pairs);
    if (lane_pk_ok) {
        // ASCII rows of a shape only the packed lane kernel takes (READ_SIZE other than 80 / 112: l = 150 and friends; CIGAR at
        // MAX_SCORE 6..10): pack on the device (batch_io.hpp), run the packed kernel, let the general kernel re-align the
        // non-ACGT pairs. [to-do | flag bits | packed P | packed T | general kernel]
        m.kid = K_WFA_LANE_PK;
        aim::wfa_lane_packed_plan(p, n_pairs, kn, &m.grid, &m.block, &m.lds);
        pl->pack_first = true;
        const size_t flag_b = (((size_t)n_pairs + 31) / 32 * 4 + 255) & ~(size_t)255;
        const size_t arr_b = (((size_t)n_pairs * aim::packed_row_dwords(p.read_size) * 4) + 64 + 255) & ~(size_t)255;
        pl->flags_at = pl->todo_bytes;
        pl->pack_p_at = pl->flags_at + flag_b;
        pl->pack_t_at = pl->pack_p_at + arr_b;
        pl->fb.scratch_at = pl->pack_t_at + arr_b;
    } else {
        // [to-do | history regions | general kernel]
        pl->pk = gpk;
        // (ends-free: ops rows, then cigar_rle_kernel -- the fused run output of wfa_group_tb_kernel is not used for it: one pair of
        // a host run came back with a void first run, cause not found; affine2p and gap-linear likewise)
        pl->emits_runs = bt && (mode & MODE_RUNS_OUT) && !is_endsfree(p) && !is_affine2p(p) && !is_linear(p);
        pl->hist_at = pl->todo_bytes;
        pl->fb.scratch_at = pl->hist_at + pl->hist_bytes;
    }
    pl->scratch_total = pl->fb.scratch_at + stage_bytes(pl->fb);
    return AIM_OK;
}

inline size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
inline bool is_lane_plan(const StagePlan &pl) { return pl.main.kid == K_WFA_LANE || pl.main.kid == K_WFA_LANE_PK; }

// AIM_FLAG_WFA_ESCALATE: c is the largest cap below MAX_SCORE whose flag-less plan (same params and mode otherwise) is a lane plan. Without
// one, or when the flag-less plan is a lane plan already, the plan is the flag-less one. Else stage 1 is that lane plan over the batch and
// stage 2 the flag-less plan at MAX_SCORE over the list of pairs stage 1 reports at c + 1: a pair of score <= c has the same wavefronts
// under both caps, so its stage-1 row, ops bytes included, is final. Both stages write result rows (and ops rows); the fused run output
// is not planned under escalation (the caller runs cigar_rle_kernel over the final rows, so the run total is the flag-less one).
int plan_wfa(const aim_params_t &p, uint32_t n_pairs, const aim::Knobs &kn, uint64_t budget, uint32_t mode, Plan *pl)
{
    if (!is_escalate(p)) return plan_wfa_flagless(p, n_pairs, kn, budget, mode, pl);
    aim_params_t q = p;
    q.flags &= ~AIM_FLAG_WFA_ESCALATE;
    int rc = plan_wfa_flagless(q, n_pairs, kn, budget, mode, pl);
    if (rc) return rc;
    pl->esc = true;
    if (is_lane_plan(*pl)) return AIM_OK;
    const uint32_t mode2 = mode & ~MODE_RUNS_OUT;
    // the lane test of plan_wfa_flagless alone (no group / wave planning per candidate cap); the plan is then made once, at c
    const bool lanes = !kn.force_wave && !kn.no_lane;
    auto lane_at = [&](int cap) {
        aim_params_t q1 = q;
        q1.max_score = cap;
        return lanes && ((!kn.no_lane_pk && aim::wfa_lane_packed_supported(q1, !kn.no_lane_ext)) || aim::wfa_lane_supported(q1, !kn.no_lane_ext));
    };
    int c = std::min(p.max_score - 1, 64);
    while (c > 0 && !lane_at(c)) --c;
    if (c <= 0) return AIM_OK;
    Plan s1;
    memset(&s1, 0, sizeof s1);
    {
        aim_params_t q1 = q;
        q1.max_score = c;
        if (plan_wfa_flagless(q1, n_pairs, kn, budget, mode2, &s1) != AIM_OK || !is_lane_plan(s1)) return AIM_OK;
    }
    // stage 2 gets the budget stage 1 leaves (their regions are laid out one behind the other)
    const uint64_t used = al256(s1.scratch_total);
    const uint64_t budget2 = budget > 2 * used ? budget - used : budget;
    Plan s2;
    memset(&s2, 0, sizeof s2);
    rc = plan_wfa_flagless(q, n_pairs, kn, budget2, mode2, &s2);
    if (rc) return rc;
    *pl = s1;
    pl->esc = true;
    pl->esc_c = c;
    pl->s2 = s2;
    pl->s1_scratch = s1.scratch_total;
    pl->s2_at = al256(s1.scratch_total);
    pl->list_at = pl->s2_at + al256(s2.scratch_total);
    pl->mask_at = pl->list_at + aim::wfa_lane_todo_bytes(n_pairs);
    pl->count_at = pl->mask_at + aim::escalate_mask_bytes(n_pairs);
    pl->scratch_total = pl->count_at + aim::escalate_count_bytes(n_pairs);
    return AIM_OK;
}

// dp_lane_kernel (nw_lane / swg_lane) as a stage; todo: as the to-do pass behind another kernel
bool plan_dp_lane(const aim_params_t &p, uint32_t n_pairs, uint64_t budget, const aim::Knobs &kn, bool todo, Stage *st)
{
    size_t total = 0;
    st->kid = K_DP_LANE;
    return aim::dp_lane_plan(p, n_pairs, budget, kn, todo, &st->grid, &st->block, &st->lds, &st->scratch_per_wg, &total, &st->seq);
}

bool plan_dp_strip(const aim_params_t &p, uint32_t n_pairs, uint64_t budget, const aim::Knobs &kn, Stage *st)
{
    size_t total = 0;
    st->kid = K_DP_STRIP;
    return aim::dp_strip_plan(p, n_pairs, budget, kn, &st->grid, &st->block, &st->lds, &st->scratch_per_wg, &total, &st->strip_k);
}

// NW / SWG medium reads: G lanes per pair (dp_group.hpp); pairs with an empty sequence reach nw_lane / swg_lane (READ_SIZE <= 320)
// or dp_strip_kernel (to-do mode) through the to-do list. [the pairs' direction-bit slabs OR, afterwards, the fallback kernel's scratch |
// to-do region]. False when the budget holds neither this plan nor its fallback: not an error, the plans without dp_group are tried
// next.
bool plan_dp_group(const aim_params_t &p, uint32_t n_pairs, const aim::Knobs &kn, uint64_t budget, Plan *pl)
{
    Plan g;
    memset(&g, 0, sizeof g);
    if (!(p.read_size <= 320 ? plan_dp_lane(p, n_pairs, budget / 2, kn, true, &g.fb) : plan_dp_strip(p, n_pairs, budget / 2, kn, &g.fb)))
        return false;
    Stage &m = g.main;
    aim::dp_group_plan(p, n_pairs, kn, &m.grid, &m.lds, &m.scratch_per_wg);
    while (m.grid > 8 && m.scratch_per_wg * m.grid > budget / 2) m.grid -= 8;
    if (m.scratch_per_wg * m.grid > budget / 2) return false;
    m.kid = K_DP_GROUP;
    m.block = 64;
    g.todo_bytes = aim::wfa_lane_todo_bytes(n_pairs);
    g.todo_at = (std::max(stage_bytes(g.fb), stage_bytes(m)) + 255) & ~(size_t)255;
    g.scratch_total = g.todo_at + g.todo_bytes;
    *pl = g;
    return true;
}

// NW / SWG short reads with the rows in registers (dp_reg.hpp: slab_bt bytes of direction bits per wavefront with BACKTRACE, lds bytes
// of LDS); the pairs it cannot take (tail cells, short outliers, SWG cells that wrap) reach nw_lane / swg_lane through a to-do list.
// [table slabs of max(grid) wavefronts, shared by both kernels | to-do region]
int plan_dp_reg(const aim_params_t &p, uint32_t n_pairs, const aim::Knobs &kn, uint64_t budget, uint64_t slab_bt, size_t lds, Plan *pl)
{
    Stage &m = pl->main, &fb = pl->fb;
    if (!plan_dp_lane(p, n_pairs, budget / 2, kn, true, &fb)) return fail(AIM_ENOMEM, "scratch budget too small for read_size %d", p.read_size);
    const uint64_t slab = (p.flags & AIM_FLAG_BACKTRACE) ? slab_bt : 256;
    uint32_t per_cu = kn.nw_reg_per_cu > 0 ? (uint32_t)kn.nw_reg_per_cu : 8u;   // two wavefronts per SIMD (NW: 178 - 255 VGPRs)
    per_cu = (uint32_t)std::min<size_t>(per_cu, aim::lds_workgroups_per_cu(lds));
    const uint32_t n_groups = (n_pairs + 63u) / 64u;
    uint32_t g = aim::resident_grid(kn, per_cu);
    const uint32_t need = ((n_groups + 7u) / 8u) * 8u;
    if (g > need) g = need < 8u ? 8u : need;
    const uint64_t per = std::max<uint64_t>((slab + 255) & ~255ull, fb.scratch_per_wg);
    while (g > 8 && per * g > budget / 2) g -= 8;
    if (per * std::max(g, fb.grid) > budget) return fail(AIM_ENOMEM, "scratch budget too small for read_size %d", p.read_size);
    m.kid = K_DP_REG;
    m.grid = g;
    m.block = 64;
    m.lds = lds;
    m.scratch_per_wg = fb.scratch_per_wg = per;
    pl->todo_bytes = aim::wfa_lane_todo_bytes(n_pairs);
    pl->todo_at = (size_t)(per * std::max(g, fb.grid));
    pl->scratch_total = pl->todo_at + pl->todo_bytes;
    return AIM_OK;
}

// NW / SWG
int plan_dp(const aim_params_t &p, uint32_t n_pairs, const aim::Knobs &kn, uint64_t budget, Plan *pl)
{
    if (aim::dp_group_supported(p, kn) && plan_dp_group(p, n_pairs, kn, budget, pl)) return AIM_OK;
    // NW / SWG long reads: one pair per workgroup of 1-12 wavefronts, row-scan, canonical table in per-workgroup HBM scratch
    // (SWG with int8 cells -- the launchers' MAX_SCORE < 127 -- wraps by design and is nobody's but the literal kernels': swg_lane_kernel, one pair per LANE with its M and I rows
    //  in LDS, takes it as far as 64 lanes' rows fit a CU's LDS (READ_SIZE <= 1 199; round 6: until then dp_wave_kernel's literal path, one lane per WORKGROUP, from READ_SIZE 321 on:
    //  6 - 13 GCUPS, profiles/r06/cliff_scan.txt))
    const bool cell8 = p.algo == AIM_ALGO_SWG && aim::swg_cell_bytes(p) == 1;
    bool cell8_lane = cell8 && !kn.force_dpwave && !kn.dpw_legacy && kn.dpw_nw < 0 && kn.strip_k <= 0 && (size_t)2 * (p.read_size + 1) * 64 <= 150 * 1024;
    if (cell8_lane && p.read_size > 320) {   // (with CIGAR a lane's table is READ_SIZE^2 x 4 bytes x 64 lanes per workgroup: a budget that does not hold eight of them keeps the one-table-per-workgroup path)
        Stage t;
        cell8_lane = plan_dp_lane(p, n_pairs, budget, kn, false, &t);
    }
    Stage &m = pl->main;
    if ((p.read_size > 320 && !cell8_lane) || kn.force_dpwave) {
        bool ok;
        size_t total = 0;
        if (!kn.dpw_legacy && kn.dpw_nw < 0 && aim::dp_strip_supported(p, cell8, kn))   // column-strip pipeline (dp_strip.hpp): previous row in registers, packed int16 arithmetic, mailboxes instead of barriers
            ok = plan_dp_strip(p, n_pairs, budget, kn, &m);
        else {
            m.kid = K_DP_WAVE;
            ok = aim::dp_wave_plan(p, n_pairs, budget, kn, cell8, &m.grid, &m.block, &m.lds, &m.scratch_per_wg, &total);
        }
        pl->scratch_total = stage_bytes(m);
        return ok ? AIM_OK : fail(AIM_ENOMEM, "scratch budget (AIM_SCRATCH_GB) or LDS too small for read_size %d", p.read_size);
    }
    const int rs = p.read_size;
    if (p.algo == AIM_ALGO_NW && !kn.no_nw_reg && !kn.force_dpwave && aim::nw_reg_supported(p)) {
        const int npk = aim::nw_reg_npk(rs, (p.flags & AIM_FLAG_BACKTRACE) != 0);
        return plan_dp_reg(p, n_pairs, kn, budget, aim::nw_reg_slab_bytes(npk, rs), aim::nw_reg_lds_bytes(p), pl);
    }
    if (p.algo == AIM_ALGO_SWG && !kn.no_swg_reg && !kn.force_dpwave && aim::swg_reg_supported(p)) {
        const int npk = aim::swg_reg_npk(rs);
        return plan_dp_reg(p, n_pairs, kn, budget, aim::swg_reg_slab_bytes(npk, rs), aim::swg_reg_lds_bytes(p, npk), pl);
    }
    // NW / SWG short reads: one pair per lane, flat DP table in per-wave HBM scratch
    if (!plan_dp_lane(p, n_pairs, budget, kn, false, &m)) return fail(AIM_ENOMEM, "scratch budget too small for read_size %d", p.read_size);
    pl->scratch_total = stage_bytes(m);
    return AIM_OK;
}

const char *kernel_name(const StagePlan &pl, const aim_params_t &p)
{
    switch (pl.main.kid) {
    case K_WFA_WAVE: return "wfa_wave_kernel";
    case K_WFA_BIDIR: return "wfa_bidir_kernel";
    case K_WFA_LANE: return "wfa_lane_kernel";
    case K_WFA_LANE_PK: return "wfa_lane_packed_kernel";
    case K_WFA_GROUP: return "wfa_group_kernel";
    case K_DP_LANE: return p_is_nw(&p) ? "nw_lane_kernel" : "swg_lane_kernel";
    case K_DP_REG: return p_is_nw(&p) ? "nw_reg_kernel" : "swg_reg_kernel";
    case K_DP_WAVE: return "dp_wave_kernel";
    case K_DP_STRIP: return "dp_strip_kernel";
    case K_DP_GROUP: return "dp_group_kernel";
    case K_GENASM: return "genasm_wave_kernel";
    }
    return "";
}

// One line that identifies a plan completely: kernel, lanes / wavefronts per pair, grid, block, LDS, scratch.
int describe_stage_plan(const StagePlan &pl, const aim_params_t &p, uint32_t n_pairs, uint64_t budget, char *out, size_t cap)
{
    char extra[160] = "";
    const Stage &m = pl.main, &fb = pl.fb;
    if (m.kid == K_WFA_GROUP) snprintf(extra, sizeof extra, " G=%d hist=%zu chunk=%u fb_grid=%u packed_in=%d runs_out=%d", pl.group_g, pl.hist_bytes, pl.chunk_pairs, fb.grid, (int)pl.pk, (int)pl.emits_runs);
    else if (m.kid == K_WFA_LANE_PK) snprintf(extra, sizeof extra, " pack_first=%d fb_grid=%u", (int)pl.pack_first, fb.grid);
    else if (m.kid == K_DP_WAVE) snprintf(extra, sizeof extra, " wavefronts_per_pair=%u", m.block / 64);
    else if (m.kid == K_DP_STRIP) snprintf(extra, sizeof extra, " wavefronts_per_pair=%u cells_per_lane=%d", m.block / 64, m.strip_k);
    else if (m.kid == K_WFA_WAVE) snprintf(extra, sizeof extra, " pool_cap=%u ring=%ux%u seq_lds=%d", m.pool_cap, m.ring_slots, m.slot_w, (int)m.seq_lds);
    else if (m.kid == K_DP_LANE) snprintf(extra, sizeof extra, " seq_lds=%d", (int)(m.seq == 1));
    else if (m.kid == K_DP_REG) snprintf(extra, sizeof extra, " fb_grid=%u fb_lds=%zu", fb.grid, fb.lds);
    else if (m.kid == K_DP_GROUP) snprintf(extra, sizeof extra, " lanes_per_pair=%d fb_grid=%u fb_block=%u fb_lds=%zu", aim::dp_group_lanes(p.read_size, (p.flags & AIM_FLAG_BACKTRACE) != 0, p.algo == AIM_ALGO_SWG), fb.grid, fb.block, fb.lds);
    char efs[80] = "";
    if (is_endsfree(p)) {
        const EndsFree e = ends_free(p);
        snprintf(efs, sizeof efs, " endsfree=%d,%d,%d,%d", e.pb, e.pe, e.tb, e.te);
    } else if (is_affine2p(p)) {
        const Affine2p g = affine2p(p);
        snprintf(efs, sizeof efs, " affine2p=%d,%d", g.o2, g.e2);
    } else if (is_linear(p)) {
        snprintf(efs, sizeof efs, " linear");
    }
    if (m.kid == K_WFA_BIDIR) snprintf(extra, sizeof extra, " bidir=%d", pl.bidir_t);
    return snprintf(out, cap, "%s n=%u grid=%u block=%u lds=%zu scratch=%zu budget=%llu%s%s%s%s", kernel_name(pl, p), n_pairs, pl.main.grid,
                    pl.main.block, pl.main.lds, pl.scratch_total, (unsigned long long)budget, extra, efs, is_w32(p) ? " w32" : "",
                    is_ref(p) ? " ref=1" : "");
}

// ... AIM_FLAG_WFA_ESCALATE: "<stage 1 line> | <stage 2 line> escalate=c", or the flag-less line and " escalate=0"
int describe_plan_stages(const Plan &pl, const aim_params_t &p, uint32_t n_pairs, uint64_t budget, char *out, size_t cap)
{
    if (!pl.esc) return describe_stage_plan(pl, p, n_pairs, budget, out, cap);
    char a[384], b[384];
    if (!pl.esc_c) {
        describe_stage_plan(pl, p, n_pairs, budget, a, sizeof a);
        return snprintf(out, cap, "%s escalate=0", a);
    }
    aim_params_t p1 = p;
    p1.max_score = pl.esc_c;
    StagePlan s1 = pl;
    s1.scratch_total = pl.s1_scratch;
    describe_stage_plan(s1, p1, n_pairs, budget, a, sizeof a);
    describe_stage_plan(pl.s2, p, n_pairs, budget, b, sizeof b);
    return snprintf(out, cap, "%s | %s escalate=%d", a, b, pl.esc_c);
}
}  // namespace

// ... AIM_FLAG_SAM_FIELDS: the line and " sam=1"
int aim::capi::describe_plan(const Plan &pl, const aim_params_t &p, uint32_t n_pairs, uint64_t budget, char *out, size_t cap)
{
    if (!is_sam(p)) return describe_plan_stages(pl, p, n_pairs, budget, out, cap);
    char a[800];
    describe_plan_stages(pl, p, n_pairs, budget, a, sizeof a);
    return snprintf(out, cap, "%s sam=1", a);
}

int aim::capi::make_plan(const aim_params_t &p, uint32_t n_pairs, const aim::Knobs &kn, uint64_t budget, Plan *pl, uint32_t mode)
{
    int rc = validate_params(p);
    if (rc) return rc;
    memset(pl, 0, sizeof *pl);
    const aim::Knobs kc = kn.cus ? kn : with_chip(kn);
    rc = p.algo == AIM_ALGO_GENASM ? plan_genasm(p, n_pairs, kc, pl)
         : p.algo == AIM_ALGO_WFA  ? plan_wfa(p, n_pairs, kc, budget, mode, pl)
                                   : plan_dp(p, n_pairs, kc, budget, pl);
    if (rc == AIM_OK && kn.plan_debug) {
        char line[800];
        describe_plan(*pl, p, n_pairs, budget, line, sizeof line);
        fprintf(stderr, "[aim plan] %s\n", line);
    }
    return rc;
}

XParams aim::capi::groups_pass_params(const aim_params_t &p, uint32_t drop)
{
    XParams x = copy_params(p);
    x.base.flags &= ~(AIM_FLAG_READ_GROUPS | AIM_FLAG_MATE_PAIRS | AIM_FLAG_SAM_FIELDS | AIM_FLAG_TOP_HITS | drop);
    return x;
}

int aim::capi::describe_groups(const GroupsPlan &g, uint32_t n_pairs, uint32_t n_reads, uint64_t budget, char *out, size_t cap)
{
    char a[384], b[384];
    describe_plan(g.p1, g.x1.base, n_pairs, budget, a, sizeof a);
    if (g.pass2) describe_plan(g.p2, g.x2.base, n_reads, budget, b, sizeof b);
    else snprintf(b, sizeof b, "no second pass n=%u", n_reads);
    return snprintf(out, cap, "%s | %s groups=1%s%s%s", a, b, g.mates ? " mates=1" : "", g.sam ? " sam=1" : "", g.hits ? " hits=1" : "");
}

// Both passes planned for n_pairs candidates (the worst case n_reads = n_pairs for pass 2) and the stateless scratch layout:
// [plans | candidate pattern rows | candidate text rows (REF_TEXTS) | pass-1 results | candidate -> read map | sel | pass-2 requests,
//  pattern rows, text rows (BACKTRACE) | aim_best_t rows (MATE_PAIRS) | hit list (TOP_HITS)]
int aim::capi::make_groups_plan(const aim_params_t &p, uint32_t n_pairs, const aim::Knobs &kn, uint64_t budget, GroupsPlan *g)
{
    int rc = validate_params(p);
    if (rc) return rc;
    memset(g, 0, sizeof *g);
    aim::Knobs quiet = kn;
    quiet.plan_debug = false;
    g->x1 = groups_pass_params(p, AIM_FLAG_BACKTRACE | AIM_FLAG_WFA_BIDIR | AIM_FLAG_RES8);
    g->x2 = groups_pass_params(p, 0u);
    g->pass2 = (p.flags & AIM_FLAG_BACKTRACE) != 0;
    g->mates = is_mates(p);
    g->sam = is_sam(p);
    g->hits = is_hits(p);
    rc = make_plan(g->x1.base, n_pairs, quiet, budget, &g->p1);
    if (rc) return rc;
    g->plan_bytes = g->p1.scratch_total;
    if (g->pass2) {
        rc = make_plan(g->x2.base, n_pairs, quiet, budget, &g->p2);
        if (rc) return rc;
        g->plan_bytes = std::max(g->plan_bytes, g->p2.scratch_total);
    }
    const size_t rows = (size_t)n_pairs * (size_t)p.read_size + 256;
    size_t at = al256(g->plan_bytes);
    g->cand_p_at = at; at += al256(rows);
    if (is_ref(p)) { g->cand_t_at = at; at += al256(rows); }
    g->res1_at = at; at += al256((size_t)n_pairs * sizeof(aim_result_t));
    g->map_at = at; at += al256((size_t)n_pairs * 4);
    g->sel_at = at; at += al256((size_t)n_pairs * 4);
    if (g->pass2) {
        g->req2_at = at; at += al256((size_t)n_pairs * sizeof(aim_request_t));
        g->pat2_at = at; at += al256(rows);
        g->txt2_at = at; at += al256(rows);
    }
    if (g->mates) { g->best_at = at; at += al256((size_t)n_pairs * sizeof(aim_best_t)); }
    if (g->hits) { g->hit_at = at; at += al256((size_t)n_pairs * 4); }
    g->total = at;
    if (kn.plan_debug) {
        char line[800];
        describe_groups(*g, n_pairs, n_pairs, budget, line, sizeof line);
        fprintf(stderr, "[aim plan] %s\n", line);
    }
    return AIM_OK;
}
extern "C" {

size_t aim_scratch_bytes(const aim_params_t *params, uint32_t n_pairs)
{
    Plan pl;
    const aim::Knobs kn = read_knobs();
    if (params && is_groups(*params)) {   // both passes' plans + the rows and arrays between them, for n_reads = n_pairs
        GroupsPlan g;
        aim::Knobs quiet = kn;
        quiet.plan_debug = false;
        return make_groups_plan(*params, n_pairs, quiet, stateless_budget_bytes(kn), &g) ? 0 : g.total;
    }
    if (!params || make_plan(*params, n_pairs, kn, stateless_budget_bytes(kn), &pl)) return 0;
    if (is_ref(*params)) return ref_rows_at(pl.scratch_total) + ref_rows_bytes(*params, n_pairs);   // + the gathered text rows
    return pl.scratch_total;
}

int aim_plan_describe(const aim_params_t *params, uint32_t n_pairs, char *out, size_t cap)
{
    if (!params || !out || cap == 0) return fail(AIM_EINVAL, "bad arguments");
    const aim::Knobs kn = read_knobs();
    const uint64_t budget = stateless_budget_bytes(kn);
    if (is_groups(*params)) {   // n_reads = n_pairs, as aim_scratch_bytes counts it
        GroupsPlan g;
        int rc = make_groups_plan(*params, n_pairs, kn, budget, &g);
        if (rc) return rc;
        describe_groups(g, n_pairs, n_pairs, budget, out, cap);
        return AIM_OK;
    }
    Plan pl;
    int rc = make_plan(*params, n_pairs, kn, budget, &pl);
    if (rc) return rc;
    describe_plan(pl, *params, n_pairs, budget, out, cap);
    return AIM_OK;
}

const char *aim_kernel_name(const aim_params_t *params)
{
    Plan pl;
    aim::Knobs kn = read_knobs();
    kn.plan_debug = false;
    if (!params) return "";
    if (is_groups(*params)) {   // the score-only pass's kernel (the one every candidate meets)
        const XParams x1 = groups_pass_params(*params, AIM_FLAG_BACKTRACE | AIM_FLAG_WFA_BIDIR | AIM_FLAG_RES8);
        if (validate_params(*params) || make_plan(x1.base, 1u << 20, kn, stateless_budget_bytes(kn), &pl)) return "";
        return kernel_name(pl, x1.base);
    }
    if (make_plan(*params, 1u << 20, kn, stateless_budget_bytes(kn), &pl)) return "";
    return kernel_name(pl, *params);
}

}  // extern "C"
