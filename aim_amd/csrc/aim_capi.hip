// aim_capi.hip -- C-ABI (include/aim_hip.h) over the gfx950 alignment kernels.
//
// Host side of the drop-in boundary: what host.c does with dpu_alloc /
// dpu_push_xfer / dpu_launch (WFA/DPU-WRAM/host/host.c:186-330) is done here
// with one HIP stream per device, HBM buffers planned per configuration, and
// asynchronous copies.  No CPU fallback exists: every compute entry point
// needs a HIP device.  This unit launches: device sets, slots, submits and the alignment entry points. The launch planner and the entry
// points that only plan are in capi_plan.hip (plan.hpp), the read-mapping pipeline's entry points in capi_pipeline.hip, the host-side
// helpers in capi_host.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

#include "capi_common.hpp"
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
#include "groups.hpp"
#include "hits.hpp"
#include "mates.hpp"
#include "sam_fields.hpp"
#include "genasm_wave.hpp"

using namespace aim::capi;

namespace {
thread_local char g_err[512] = "";   // what aim_last_error() returns: written by fail() alone, whichever unit calls it
}

int aim::capi::fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}

uint32_t aim::capi::packed_row_dwords(int read_size) { return aim::packed_row_dwords(read_size); }

namespace {

// KArgs of one stage: where its scratch starts, its slab and what its plan chose for wfa_wave
aim::KArgs stage_args(aim::KArgs ka, const Stage &st, void *d_scratch)
{
    ka.scratch = (char *)d_scratch + st.scratch_at;
    ka.scratch_per_wave = st.scratch_per_wg;
    ka.pool_cap = st.pool_cap;
    ka.meta_cap = st.meta_cap;
    ka.ring_slots = st.ring_slots;
    ka.slot_w = st.slot_w;
    ka.dbg_lds_bytes = (uint32_t)st.lds;
    return ka;
}

// The kernels that run alone or as the to-do pass behind another one (ka.todo set)
void launch_stage(const aim_params_t &p, const Stage &st, const aim::KArgs &ka, hipStream_t s)
{
    switch (st.kid) {
    case K_WFA_WAVE: aim::wfa_wave_launch(p.flags & AIM_FLAG_BACKTRACE, p.flags & AIM_FLAG_REDUCE, st.seq_lds, st.grid, st.lds, ka, s); break;
    case K_DP_LANE: aim::dp_lane_launch(p, st.seq, st.grid, st.lds, ka, s); break;
    case K_DP_STRIP: aim::dp_strip_launch(p, st.strip_k, st.grid, st.block, st.lds, ka, s); break;
    default: break;
    }
}

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
int aux_stream_create(AuxStream &a)
{
    if (a.stream) return AIM_OK;
    HIP_TRY(hipStreamCreateWithFlags(&a.stream, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(hipEventCreateWithFlags(&a.computed[i], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&a.walked[i], hipEventDisableTiming));
    }
    return AIM_OK;
}
void aux_stream_destroy(AuxStream &a)
{
    for (int i = 0; i < 2; ++i) {
        if (a.computed[i]) (void)hipEventDestroy(a.computed[i]);
        if (a.walked[i]) (void)hipEventDestroy(a.walked[i]);
    }
    if (a.stream) (void)hipStreamDestroy(a.stream);
    a = AuxStream();
}
struct SharedAux { std::mutex mu; AuxStream aux; };
SharedAux *shared_aux_for_current_device()
{
    static SharedAux table[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return nullptr; }
    return &table[dev];
}

// The fused batch I/O of a launch (Plan::pk / Plan::emits_runs): packed rows in, compact CIGAR out.
struct FusedIo {
    const uint32_t *packedP = nullptr, *packedT = nullptr;
    aim_cigar_t *cig = nullptr;
    uint32_t *runs = nullptr, *cursor = nullptr;
    uint32_t runs_cap = 0, run_slot = 0;
};

// Enqueue one alignment launch that follows the one-stage plan `pl` (made for >= n_pairs pairs under the caller's knobs and budget).
// list_in (AIM_FLAG_WFA_ESCALATE, second stage): the launch's pairs are those of the device-side list {count @0, pair ids @16..}, at most
// n_pairs of them; every buffer stays the batch's. Only wfa_group (+ its traceback) and wfa_wave take one.
int launch_one(const StagePlan &pl, const aim::Knobs &kn, const aim_params_t &p, uint32_t n_pairs, const void *d_req,
               const char *d_pat, const char *d_txt, void *d_res, char *d_ops, void *d_scratch, size_t scratch_bytes,
               hipStream_t stream, const FusedIo *fio = nullptr, AuxStream *slot_aux = nullptr, const uint32_t *list_in = nullptr)
{
    if (n_pairs == 0) return AIM_OK;
    const bool bt = p.flags & AIM_FLAG_BACKTRACE;
    if (list_in && pl.main.kid != K_WFA_GROUP && pl.main.kid != K_WFA_WAVE) return fail(AIM_EINVAL, "plan takes no pair list");
    if (pl.pk && !pl.pack_first && (!fio || !fio->packedP || !fio->packedT)) return fail(AIM_EINVAL, "plan reads packed rows but none were given");
    if (pl.emits_runs && (!fio || !fio->cig || !fio->runs || !fio->cursor)) return fail(AIM_EINVAL, "plan emits the compact CIGAR but no buffers were given");
    const bool reads_ascii = !(pl.main.kid == K_WFA_LANE_PK && !pl.pack_first);   // (wfa_group reads them for its to-do pairs even on packed batches)
    const bool writes_res = !(pl.main.kid == K_WFA_LANE_PK && pl.emits_runs);
    if (!d_req || (reads_ascii && (!d_pat || !d_txt)) || (writes_res && !d_res)) return fail(AIM_EINVAL, "null device buffer");
    if (bt && writes_res && !d_ops) return fail(AIM_EINVAL, "AIM_FLAG_BACKTRACE needs an ops buffer");
    if (scratch_bytes < pl.scratch_total || (!d_scratch && pl.scratch_total))
        return fail(AIM_EINVAL, "scratch too small: need %zu bytes, got %zu", pl.scratch_total, scratch_bytes);
    aim::KArgs ka0;
    ka0.p = p;
    ka0.n_pairs = n_pairs;
    ka0.req = static_cast<const aim_request_t *>(d_req);
    ka0.patterns = d_pat;
    ka0.texts = d_txt;
    ka0.res = static_cast<aim_result_t *>(d_res);
    ka0.ops = d_ops;
    ka0.todo = nullptr;
    ka0.dbg_poison_lds = kn.poison_lds >= 0 ? (0x100u | (uint32_t)(kn.poison_lds & 0xff)) : 0u;
    ka0.dbg_flags = (uint32_t)kn.dbg_flags;
    ka0.packedP = fio ? fio->packedP : nullptr;
    ka0.packedT = fio ? fio->packedT : nullptr;
    ka0.cig = fio ? fio->cig : nullptr;
    ka0.runs = fio ? fio->runs : nullptr;
    ka0.runs_cap = fio ? fio->runs_cap : 0u;
    ka0.cursor = fio ? fio->cursor : nullptr;
    ka0.pair_base = 0;
    {
        const EndsFree e = ends_free(p);
        ka0.ef_pb = e.pb; ka0.ef_pe = e.pe; ka0.ef_tb = e.tb; ka0.ef_te = e.te;
        const Affine2p g = affine2p(p);
        ka0.a2p_o2 = g.o2; ka0.a2p_e2 = g.e2;
    }
    const Stage &m = pl.main;
    aim::KArgs ka = stage_args(ka0, m, d_scratch);
    // the fallback over the to-do list the main kernel filled: its own stage, the batch's ASCII rows
    aim::KArgs kb = stage_args(ka0, pl.fb, d_scratch);
    kb.todo = reinterpret_cast<const uint32_t *>((char *)d_scratch + pl.todo_at);
    kb.packedP = kb.packedT = nullptr;
    kb.cig = nullptr;
    if (kn.poison_ops >= 0 && d_ops && bt && !list_in)   // (the second stage keeps the first stage's rows) debugging aid: results must not depend on what the ops rows held before (only ops[begin_offset, end_offset) is written)
        HIP_TRY(hipMemsetAsync(d_ops, kn.poison_ops & 0xff, (size_t)n_pairs * 2 * p.read_size, stream));
    if (pl.todo_bytes) HIP_TRY(hipMemsetAsync((char *)d_scratch + pl.todo_at, 0, 64, stream));   // the to-do count, zeroed per launch
    switch (m.kid) {
    case K_WFA_WAVE:
    case K_DP_LANE:
    case K_DP_STRIP:
        if (list_in) ka.todo = list_in;
        launch_stage(p, m, ka, stream);
        break;
    case K_WFA_LANE:
        aim::wfa_lane_launch(p, m.grid, m.block, m.lds, ka, stream);
        break;
    case K_WFA_LANE_PK:
        if (pl.pack_first) {
            // pack_rows_kernel lists the non-ACGT pairs; the packed kernel aligns the batch, wfa_wave re-aligns the listed pairs
            char *base = (char *)d_scratch;
            uint32_t *flags_d = reinterpret_cast<uint32_t *>(base + pl.flags_at);
            uint32_t *pkP = reinterpret_cast<uint32_t *>(base + pl.pack_p_at), *pkT = reinterpret_cast<uint32_t *>(base + pl.pack_t_at);
            HIP_TRY(hipMemsetAsync(flags_d, 0, pl.pack_p_at - pl.flags_at, stream));
            const uint64_t threads = (uint64_t)n_pairs * aim::packed_row_dwords(p.read_size);
            hipLaunchKernelGGL(aim::pack_rows_kernel, dim3((unsigned)((threads + 255) / 256), 2), dim3(256), 0, stream, ka, pkP, pkT, flags_d,
                               reinterpret_cast<uint32_t *>(base + pl.todo_at));
            HIP_TRY(hipGetLastError());
            aim::KArgs kp = ka;
            kp.packedP = pkP;
            kp.packedT = pkT;
            aim::wfa_lane_packed_launch(p, m.grid, m.lds, kp, 0u, stream);
            HIP_TRY(hipGetLastError());
            launch_stage(p, pl.fb, kb, stream);
            break;
        }
        aim::wfa_lane_packed_launch(p, m.grid, m.lds, ka, fio->run_slot, stream);
        break;
    case K_WFA_GROUP: {
        // fast kernel (+ traceback kernel with BACKTRACE) chunk by chunk; then the general kernel drains the to-do list
        const uint32_t chunk = (bt && pl.chunk_pairs) ? pl.chunk_pairs : n_pairs;
        const size_t rqb = (p.flags & AIM_FLAG_REQ8) ? sizeof(aim_request8_t) : sizeof(aim_request_t);
        const size_t rsb = (p.flags & AIM_FLAG_RES8) ? sizeof(aim_result8_t) : sizeof(aim_result_t);
        const size_t npw = aim::packed_row_dwords(p.read_size);
        const uint32_t nchunks = (n_pairs + chunk - 1) / chunk;
        const bool overlap = bt && nchunks > 1;
        const size_t buf_bytes = overlap ? pl.hist_bytes / 2 : 0;     // two alternating buffers of history regions
        AuxStream *aux = slot_aux;
        std::unique_lock<std::mutex> shared_lock;   // stateless callers: the device's shared instance, locked until the last wait is enqueued
        if (overlap && !aux) {
            SharedAux *sh = shared_aux_for_current_device();
            if (!sh) return fail(AIM_ENODEV, "no current HIP device");
            shared_lock = std::unique_lock<std::mutex>(sh->mu);
            aux = &sh->aux;
        }
        if (overlap) {
            int arc = aux_stream_create(*aux);
            if (arc) return arc;
        }
        uint32_t ci = 0;
        for (uint32_t first = 0; first < n_pairs; first += chunk, ++ci) {
            aim::KArgs kc = ka;
            const int b = (int)(ci & 1u);
            kc.n_pairs = std::min(chunk, n_pairs - first);
            kc.pair_base = first;
            kc.scratch_per_wave = pl.hist_at + (overlap ? (size_t)b * buf_bytes : 0);   // where this chunk's history regions start (the to-do region is in front)
            if (list_in) {   // positions [first, first + chunk) of the list; the arrays stay the batch's (indexed by the listed pair ids)
                kc.todo = list_in;
            } else {
                kc.req = reinterpret_cast<const aim_request_t *>(static_cast<const char *>(d_req) + (size_t)first * rqb);
                if (d_pat) { kc.patterns = d_pat + (size_t)first * p.read_size; kc.texts = d_txt + (size_t)first * p.read_size; }
                if (d_res) kc.res = reinterpret_cast<aim_result_t *>(static_cast<char *>(d_res) + (size_t)first * rsb);
                if (d_ops) kc.ops = d_ops + (size_t)first * 2 * p.read_size;
                if (ka.packedP) { kc.packedP = ka.packedP + (size_t)first * npw; kc.packedT = ka.packedT + (size_t)first * npw; }
                if (ka.cig) kc.cig = ka.cig + first;
            }
            // a chunk smaller than the plan's grid needs fewer workgroups (the grid stays a multiple of 8)
            uint32_t grid = m.grid;
            {
                const uint32_t ppw = 64u / (uint32_t)pl.group_g;
                const uint32_t need = ((((kc.n_pairs + ppw - 1) / ppw) + 7u) / 8u) * 8u;
                if (grid > need) grid = need < 8u ? 8u : need;
            }
            if (overlap && ci >= 2) HIP_TRY(hipStreamWaitEvent(stream, aux->walked[b], 0));   // buffer b: its previous chunk has been walked
            auto tb_launch = [&](hipStream_t ts) {
                if (list_in) aim::wfa_group_tb_todo_launch(pl.gcfg, kc.n_pairs, kc, ts);
                else aim::wfa_group_tb_launch(p, pl.gcfg, kc.n_pairs, kc, ts);
            };
            if (list_in) aim::wfa_group_todo_launch(p, pl.group_g, pl.gcfg, grid, m.lds, kc, stream);
            else aim::wfa_group_launch(p, pl.group_g, pl.gcfg, grid, m.lds, kc, stream);
            HIP_TRY(hipGetLastError());
            if (overlap) {
                HIP_TRY(hipEventRecord(aux->computed[b], stream));
                HIP_TRY(hipStreamWaitEvent(aux->stream, aux->computed[b], 0));
                tb_launch(aux->stream);
                HIP_TRY(hipGetLastError());
                HIP_TRY(hipEventRecord(aux->walked[b], aux->stream));
            } else if (bt) {
                tb_launch(stream);
                HIP_TRY(hipGetLastError());
            }
        }
        if (overlap) {   // the caller's stream continues only after both buffers' tracebacks
            HIP_TRY(hipStreamWaitEvent(stream, aux->walked[0], 0));
            HIP_TRY(hipStreamWaitEvent(stream, aux->walked[1], 0));
        }
        if (pl.pk) {   // the general kernel reads ASCII rows: expand the to-do pairs' packed rows in place first
            hipLaunchKernelGGL(aim::unpack_todo_rows_kernel, dim3(256), dim3(256), 0, stream, ka, kb.todo, ka.packedP, ka.packedT, const_cast<char *>(d_pat), const_cast<char *>(d_txt));
            HIP_TRY(hipGetLastError());
        }
        launch_stage(p, pl.fb, kb, stream);
        if (pl.emits_runs) {   // the general kernel wrote result_t + ops rows for the to-do pairs: their compact CIGAR
            hipLaunchKernelGGL(aim::cigar_rle_todo_kernel, dim3(256), dim3(64), 0, stream, kb, kb.todo, ka.cig, ka.runs, ka.runs_cap, ka.cursor);
            HIP_TRY(hipGetLastError());
        }
        break;
    }
    case K_DP_REG:
    case K_DP_GROUP:
        // the register / group kernel lists the pairs it leaves; then the literal-capable kernel over them
        ka.todo = kb.todo;
        if (m.kid == K_DP_GROUP) aim::dp_group_launch(p, m.grid, m.lds, ka, stream);
        else if (p.algo == AIM_ALGO_SWG) aim::swg_reg_launch(p, m.grid, m.lds, ka, stream);
        else aim::nw_reg_launch(p, m.grid, m.lds, ka, stream);
        HIP_TRY(hipGetLastError());
        launch_stage(p, pl.fb, kb, stream);
        break;
    case K_DP_WAVE:
        aim::dp_wave_launch(p, p.algo == AIM_ALGO_SWG && aim::swg_cell_bytes(p) == 1, m.grid, m.block, m.lds, ka, stream);
        break;
    case K_GENASM:
        aim::genasm_launch(p, m.grid, m.lds, ka, stream);
        break;
    case K_WFA_BIDIR: {
        // wfa_wave at MAX_SCORE min(MAX_SCORE, T) over the whole batch, then the bidirectional kernel over the pairs it left over T
        aim_params_t p1 = p;
        p1.flags &= ~AIM_FLAG_WFA_BIDIR;
        p1.max_score = std::min(p.max_score, pl.bidir_t);
        aim::KArgs k1 = stage_args(ka0, pl.fb, d_scratch);
        k1.p = p1;
        launch_stage(p1, pl.fb, k1, stream);
        HIP_TRY(hipGetLastError());
        if (p.max_score > pl.bidir_t) aim::wfa_bidir_launch(m.grid, m.lds, ka, stream);
        break;
    }
    }
    HIP_TRY(hipGetLastError());
    return AIM_OK;
}

// Enqueue the launches of plan `pl`. AIM_FLAG_WFA_ESCALATE with two stages: the lane plan at cap esc_c over the batch, the list of the
// pairs it left at esc_c + 1 (ascending pair order), the full-cap plan over that list -- one stream, no host round trip.
int launch(const Plan &pl, const aim::Knobs &kn, const aim_params_t &p, uint32_t n_pairs, const void *d_req,
           const char *d_pat, const char *d_txt, void *d_res, char *d_ops, void *d_scratch, size_t scratch_bytes,
           hipStream_t stream, const FusedIo *fio = nullptr, AuxStream *slot_aux = nullptr)
{
    // (without the flag p may be the base of an extension struct, which launch_one reads through its address: no copy of it here)
    if (!pl.esc) return launch_one(pl, kn, p, n_pairs, d_req, d_pat, d_txt, d_res, d_ops, d_scratch, scratch_bytes, stream, fio, slot_aux);
    if (!pl.esc_c || n_pairs == 0) {
        aim_params_t q = p;
        q.flags &= ~AIM_FLAG_WFA_ESCALATE;
        return launch_one(pl, kn, q, n_pairs, d_req, d_pat, d_txt, d_res, d_ops, d_scratch, scratch_bytes, stream, fio, slot_aux);
    }
    if (scratch_bytes < pl.scratch_total || !d_scratch) return fail(AIM_EINVAL, "scratch too small: need %zu bytes, got %zu", pl.scratch_total, scratch_bytes);
    if (!d_res) return fail(AIM_EINVAL, "null device buffer");
    aim_params_t q = p, p1 = p;
    q.flags &= ~AIM_FLAG_WFA_ESCALATE;
    p1.flags = q.flags;
    p1.max_score = pl.esc_c;
    char *base = static_cast<char *>(d_scratch);
    StagePlan s1 = pl;
    s1.scratch_total = pl.s1_scratch;
    int rc = launch_one(s1, kn, p1, n_pairs, d_req, d_pat, d_txt, d_res, d_ops, base, pl.s2_at, stream, fio, slot_aux);
    if (rc) return rc;
    uint32_t *list = reinterpret_cast<uint32_t *>(base + pl.list_at);
    uint2 *masks = reinterpret_cast<uint2 *>(base + pl.mask_at);
    uint32_t *counts = reinterpret_cast<uint32_t *>(base + pl.count_at);
    const bool res8 = p.flags & AIM_FLAG_RES8;
    const dim3 grid((n_pairs + aim::kEscTile - 1) / aim::kEscTile);
    hipLaunchKernelGGL(aim::escalate_select_kernel, grid, dim3(256), 0, stream, static_cast<const uint32_t *>(d_res), n_pairs, res8 ? 2u : 6u,
                       res8 ? 1u : 3u, (int32_t)(pl.esc_c + 1), masks, counts);
    hipLaunchKernelGGL(aim::escalate_list_kernel, grid, dim3(256), 0, stream, n_pairs, masks, counts, list);
    HIP_TRY(hipGetLastError());
    if (pl.pk && !pl.s2.pk) {   // a packed batch whose second stage reads ASCII rows: the listed pairs' rows, expanded in place
        aim::KArgs ku;
        memset(&ku, 0, sizeof ku);
        ku.p = q;
        ku.n_pairs = n_pairs;
        ku.req = static_cast<const aim_request_t *>(d_req);
        if (!d_pat || !d_txt || !fio || !fio->packedP || !fio->packedT) return fail(AIM_EINVAL, "null device buffer");
        hipLaunchKernelGGL(aim::unpack_todo_rows_kernel, dim3(256), dim3(256), 0, stream, ku, list, fio->packedP, fio->packedT, const_cast<char *>(d_pat),
                           const_cast<char *>(d_txt));
        HIP_TRY(hipGetLastError());
    }
    return launch_one(pl.s2, kn, q, n_pairs, d_req, d_pat, d_txt, d_res, d_ops, base + pl.s2_at, pl.s2.scratch_total, stream, fio, slot_aux, list);
}

// AIM_FLAG_REF_TEXTS: text rows [n_rows][READ_SIZE] of `out` gathered from the reference; row r is the window of pair idx[r]
// (idx == nullptr: pair r). ka carries the params and the requests.
int enqueue_gather(const aim::KArgs &ka, const uint64_t *d_tpos, const char *ref, uint64_t ref_len, const uint32_t *idx, uint32_t n_rows,
                   char *out, hipStream_t stream)
{
    if (!n_rows) return AIM_OK;
    const int rs = ka.p.read_size;
    const bool w16 = (rs & 15) == 0;   // 16-B stores per lane where the row stride allows them, else 8-B
    const uint64_t threads = (uint64_t)n_rows * (uint64_t)(rs / (w16 ? 16 : 8));
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (w16) hipLaunchKernelGGL(aim::gather_text_rows_kernel<4>, grid, dim3(256), 0, stream, ka, d_tpos, ref, ref_len, idx, n_rows, out);
    else hipLaunchKernelGGL(aim::gather_text_rows_kernel<2>, grid, dim3(256), 0, stream, ka, d_tpos, ref, ref_len, idx, n_rows, out);
    HIP_TRY(hipGetLastError());
    return AIM_OK;
}

// Device buffers of one groups batch (a slot's, or carved from the stateless scratch).
struct GroupsIo {
    uint32_t n_pairs, n_reads;
    const void *req;             // [n_pairs]
    const char *read_rows;       // [n_reads][READ_SIZE], or nullptr when the reads arrived packed:
    const uint32_t *packed;      // [n_reads][ceil(READ_SIZE/16)] packed read rows ...
    const uint32_t *raw_pairs;   // ... [n_raw] reads that travel raw, their rows in raw_rows [n_raw][READ_SIZE]
    const char *raw_rows;
    uint32_t n_raw;
    uint32_t *raw_slot;          // [n_reads] scratch of the expansion
    const uint32_t *roff;        // [n_reads + 1]
    char *cand_p, *cand_t;       // [n_pairs][READ_SIZE]; cand_t: the candidates' text rows (given, or gathered under REF_TEXTS)
    aim_result_t *res1;          // [n_pairs]
    uint32_t *map, *sel;         // [n_pairs], [n_reads]
    aim_best_t *best;            // [n_reads] or nullptr (never nullptr under AIM_FLAG_MATE_PAIRS)
    const uint64_t *tpos;        // AIM_FLAG_MATE_PAIRS: the candidates' text_pos [n_pairs] ...
    aim::MateArgs mate;          // ... the pairing parameters (n_mates and lanes are filled in by enqueue_groups) ...
    aim_mate_t *mates;           // ... and the read pairs' rows [n_reads / 2], or nullptr
    uint32_t n_hits, max_hits;   // AIM_FLAG_TOP_HITS: H hit rows, at most max_hits per read ...
    const uint32_t *hoff;        // ... hit_offsets [n_reads + 1] ...
    uint32_t *hit_pair;          // ... and the candidate of every hit row [n_hits]
    void *req2;                  // [rows] pass-2 requests; rows = n_reads, or n_hits under AIM_FLAG_TOP_HITS (never more than n_pairs)
    char *pat2, *txt2;           // [rows][READ_SIZE]
    void *res;                   // out [rows]
    char *ops;                   // out [rows][2 READ_SIZE] (BACKTRACE)
    void *scratch;               // the plans' region
    size_t scratch_bytes;
};

int enqueue_rows(const aim::KArgs &ka, const char *src, uint32_t n_src, const uint32_t *idx, uint32_t n_rows, int text, char *out, hipStream_t stream)
{
    if (!n_rows) return AIM_OK;
    const int rs = ka.p.read_size;
    const bool w16 = (rs & 15) == 0;
    const uint64_t threads = (uint64_t)n_rows * (uint64_t)(rs / (w16 ? 16 : 8));
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (w16) hipLaunchKernelGGL(aim::group_rows_kernel<4>, grid, dim3(256), 0, stream, ka, src, n_src, idx, n_rows, text, out);
    else hipLaunchKernelGGL(aim::group_rows_kernel<2>, grid, dim3(256), 0, stream, ka, src, n_src, idx, n_rows, text, out);
    HIP_TRY(hipGetLastError());
    return AIM_OK;
}

// Everything after the texts are candidate rows (cand_t): expand the read rows, pass 1, select, then pass 2 or the result gather.
// pl1 / pl2: the passes' plans for this batch (each fits io.scratch_bytes).
int enqueue_groups(const GroupsPlan &g, const Plan &pl1, const Plan &pl2, const aim::Knobs &kn, const GroupsIo &io, hipStream_t stream,
                   AuxStream *aux)
{
    const aim_params_t &p1 = g.x1.base, &p2 = g.x2.base;
    const uint32_t n = io.n_pairs, nr = io.n_reads;
    if (!n) return AIM_OK;
    aim::KArgs ka;
    memset(&ka, 0, sizeof ka);
    ka.p = p1;
    ka.n_pairs = n;
    ka.req = static_cast<const aim_request_t *>(io.req);
    hipLaunchKernelGGL(aim::group_map_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, io.roff, nr, n, io.map);
    HIP_TRY(hipGetLastError());
    int rc = AIM_OK;
    if (io.read_rows) {
        rc = enqueue_rows(ka, io.read_rows, nr, io.map, n, 0, io.cand_p, stream);
    } else {
        HIP_TRY(hipMemsetAsync(io.raw_slot, 0xff, (size_t)nr * 4, stream));
        if (io.n_raw)
            hipLaunchKernelGGL(aim::group_raw_slot_kernel, dim3((io.n_raw + 255) / 256), dim3(256), 0, stream, io.raw_pairs, io.n_raw, nr, io.raw_slot);
        const uint64_t threads = (uint64_t)n * (uint64_t)(p1.read_size / 8);
        hipLaunchKernelGGL(aim::group_unpack_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, ka, io.packed, io.map,
                           io.raw_slot, io.raw_rows, io.n_raw, nr, io.cand_p);
        HIP_TRY(hipGetLastError());
    }
    if (rc) return rc;
    rc = launch(pl1, kn, p1, n, io.req, io.cand_p, io.cand_t, io.res1, nullptr, io.scratch, io.scratch_bytes, stream, nullptr, aux);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(io.sel, 0, (size_t)nr * 4, stream));   // (a read the CSR check would refuse keeps a valid sel)
    const uint32_t waves = (nr + aim::kGroupReadsPerWave - 1) / aim::kGroupReadsPerWave;
    hipLaunchKernelGGL(aim::group_select_kernel, dim3((waves + 3) / 4), dim3(256), 0, stream, io.res1, n, io.roff, nr, io.best, io.sel);
    HIP_TRY(hipGetLastError());
    if (g.mates && nr >= 2) {
        // lanes per read pair: the power of two that covers an average read pair's combinations (any value gives the same rows)
        aim::MateArgs ma = io.mate;
        ma.n_mates = nr / 2;
        const uint64_t k = ((uint64_t)n + nr - 1) / nr, combos = k * k;
        ma.lanes = 1;
        while (ma.lanes < (uint32_t)aim::kWave && ma.lanes < combos) ma.lanes <<= 1;
        const uint64_t threads = (uint64_t)ma.n_mates * ma.lanes;
        hipLaunchKernelGGL(aim::mate_select_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, stream, ka, ma, io.res1, io.tpos,
                           io.roff, io.best, io.sel, io.mates);
        HIP_TRY(hipGetLastError());
    }
    // the rows behind the selection: the reads' winners, or under AIM_FLAG_TOP_HITS every read's hits in rank order
    uint32_t rows = nr;
    const uint32_t *row_cand = io.sel;
    if (g.hits) {
        rows = io.n_hits;
        row_cand = io.hit_pair;
        if (!rows) return AIM_OK;
        HIP_TRY(hipMemsetAsync(io.hit_pair, 0, (size_t)rows * 4, stream));   // (rows that wrong hit_offsets leave unwritten keep a valid candidate)
        hipLaunchKernelGGL(aim::hit_select_kernel, dim3((waves + 3) / 4), dim3(256), 0, stream, io.res1, n, io.roff, nr, io.hoff, io.max_hits,
                           rows, io.hit_pair);
        HIP_TRY(hipGetLastError());
    }
    if (!g.pass2) {
        hipLaunchKernelGGL(aim::group_results_kernel, dim3((rows + 255) / 256), dim3(256), 0, stream, io.res1, row_cand, rows,
                           (int)((p2.flags & AIM_FLAG_RES8) != 0), io.res);
        HIP_TRY(hipGetLastError());
        return AIM_OK;
    }
    // the rows as a batch of their own: requests, pattern rows (already cut to pattern_len) and text rows gathered by candidate
    const uint32_t rq_dw = (uint32_t)((p2.flags & AIM_FLAG_REQ8) ? sizeof(aim_request8_t) : sizeof(aim_request_t)) / 4;
    hipLaunchKernelGGL(aim::gather_elems_kernel, dim3((unsigned)(((uint64_t)rows * rq_dw + 255) / 256)), dim3(256), 0, stream,
                       static_cast<const uint32_t *>(io.req), row_cand, rows, rq_dw, static_cast<uint32_t *>(io.req2));
    HIP_TRY(hipGetLastError());
    aim::KArgs k2 = ka;
    k2.p = p2;
    k2.n_pairs = rows;
    k2.req = static_cast<const aim_request_t *>(io.req2);
    rc = enqueue_rows(k2, io.cand_p, n, row_cand, rows, 0, io.pat2, stream);
    if (!rc) rc = enqueue_rows(k2, io.cand_t, n, row_cand, rows, 1, io.txt2, stream);
    if (rc) return rc;
    return launch(pl2, kn, p2, rows, io.req2, io.pat2, io.txt2, io.res, io.ops, io.scratch, io.scratch_bytes, stream, nullptr, aux);
}

}  // namespace

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
    Plan plan_last2;                 // ... the second pass's plan
    uint32_t n_pairs = 0;
    uint32_t runs_sent = 0;  // runs of the batch in flight whose D2H copy aim_set_submit already enqueued (slotted run buffer)
    bool pushed = false, launched = false, submitted = false;
    AuxStream aux;           // this slot's second stream + events (chunked wfa_group launches with CIGAR); created on first use
    Plan plan_last;          // the plan the last launch followed (the configure-time plan re-made for the pushed pair count)
    aim_batch_io_t io;       // the batch in flight (aim_set_submit .. aim_set_wait)
};

struct aim_device_ctx {
    int dev = -1;
    std::vector<aim_slot> slots;
    char *d_ref = nullptr;   // AIM_FLAG_REF_TEXTS: the reference (+ zeroed tail slack), kept across aim_set_configure
    uint64_t ref_len = 0;
    Plan plan;               // made at configure time for max_pairs under the set's knobs and this device's budget
    Plan plan2;              // AIM_FLAG_READ_GROUPS: plan is the score-only pass's, plan2 the second pass's
    uint64_t budget = 0;     // scratch bound of one slot of this device, frozen at configure time
    float h2d_ms = 0.f, kernel_ms = 0.f, d2h_ms = 0.f;   // aim_set_submit / aim_set_wait: phase times of this device's batches, summed
};

struct aim_set {
    std::vector<aim_device_ctx> devs;
    XParams xparams;                 // the params with their extension (aim_hip.h AIM_FLAG_ENDSFREE / AIM_FLAG_AFFINE2P); xparams.base is what the plans read
    const aim_params_t &params = xparams.base;
    uint32_t max_pairs = 0, max_raw = 0, max_runs = 0;
    bool configured = false;
    aim::Knobs knobs;        // AIM_* switches as read by the last aim_set_configure; launches never re-read the environment
    float h2d_ms = 0.f, kernel_ms = 0.f, d2h_ms = 0.f;
};

namespace {
inline size_t req_size(const aim_params_t &p) { return (p.flags & AIM_FLAG_REQ8) ? sizeof(aim_request8_t) : sizeof(aim_request_t); }
inline size_t res_size(const aim_params_t &p) { return (p.flags & AIM_FLAG_RES8) ? sizeof(aim_result8_t) : sizeof(aim_result_t); }

void free_slot(aim_slot &s)
{
    void *bufs[] = {s.d_req, s.d_pat, s.d_txt, s.d_ops, s.d_res, s.d_scratch, s.d_packP, s.d_packT, s.d_rawidx, s.d_rawP, s.d_rawT,
                    s.d_cig, s.d_runs, s.d_cursor, s.d_rawreq, s.d_rawres, s.d_rawops, s.d_rawcig, s.d_tpos, s.d_reftodo,
                    s.g_readP, s.g_roff, s.g_map, s.g_sel, s.g_rawslot, s.g_res1, s.g_best, s.g_mates, s.g_hoff, s.g_hit, s.g_req2, s.g_pat2, s.g_txt2,
                    s.d_sam, s.d_samcig, s.d_samcur, s.d_sammd};
    for (void *b : bufs)
        if (b) (void)hipFree(b);
    if (s.h_cursor) (void)hipHostFree(s.h_cursor);
    if (s.h_samcur) (void)hipHostFree(s.h_samcur);
    for (auto &e : s.ev)
        if (e) (void)hipEventDestroy(e);
    if (s.stream) (void)hipStreamDestroy(s.stream);
    aux_stream_destroy(s.aux);
    s = aim_slot();
}

void free_device_buffers(aim_device_ctx &d)
{
    if (d.dev < 0) return;
    (void)hipSetDevice(d.dev);
    for (auto &s : d.slots) free_slot(s);
    d.slots.clear();
}

// OR of f(i) over i < n != 0, on up to 8 threads for large n (batch-sized host scans sit on the caller's critical path)
template <typename F>
bool any_nonzero(size_t n, F f)
{
    auto part = [&](size_t lo, size_t hi) { uint32_t acc = 0; for (size_t i = lo; i < hi; ++i) acc |= f(i); return acc; };
    const unsigned nt = n >= (1u << 19) ? 8u : 1u;
    if (nt == 1) return part(0, n) != 0;
    uint32_t acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::vector<std::thread> th;
    for (unsigned t = 1; t < nt; ++t) th.emplace_back([&, t] { acc[t] = part(n * t / nt, n * (t + 1) / nt); });
    acc[0] = part(0, n / nt);
    for (auto &x : th) x.join();
    uint32_t all = 0;
    for (unsigned t = 0; t < nt; ++t) all |= acc[t];
    return all != 0;
}
}  // namespace

// Every length of a batch against READ_SIZE (host.c:119-123) before anything is enqueued. A 4 M-pair batch is 32-64 MB of
// requests: scanned by one thread this was 2.5 ms of every aim_set_submit -- a fifth of the host CLI's loop at 4e8 pairs/s -- so
// large batches are scanned branch-free by a few threads and only a failing scan is repeated to name the pair.
int aim::capi::check_lengths(const aim_params_t &p, uint32_t n_pairs, const void *requests)
{
    const int rs = p.read_size;
    const bool req8 = p.flags & AIM_FLAG_REQ8;
    auto bad_in = [&](size_t lo, size_t hi) -> uint32_t {
        uint32_t bad = 0;
        if (req8) {
            const aim_request8_t *r = static_cast<const aim_request8_t *>(requests);
            for (size_t i = lo; i < hi; ++i) bad |= (uint32_t)((r[i].pattern_len < 0) | (r[i].text_len < 0) | (r[i].pattern_len > rs) | (r[i].text_len > rs));
        } else {
            const aim_request_t *r = static_cast<const aim_request_t *>(requests);
            for (size_t i = lo; i < hi; ++i) bad |= (uint32_t)((r[i].pattern_len < 0) | (r[i].text_len < 0) | (r[i].pattern_len > rs) | (r[i].text_len > rs));
        }
        return bad;
    };
    uint32_t bad = 0;
    const unsigned nt = n_pairs >= (1u << 19) ? 8u : 1u;
    if (nt == 1) bad = bad_in(0, n_pairs);
    else {
        uint32_t part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        std::vector<std::thread> th;
        for (unsigned t = 1; t < nt; ++t) th.emplace_back([&, t] { part[t] = bad_in((size_t)n_pairs * t / nt, (size_t)n_pairs * (t + 1) / nt); });
        part[0] = bad_in(0, (size_t)n_pairs / nt);
        for (auto &x : th) x.join();
        for (unsigned t = 0; t < nt; ++t) bad |= part[t];
    }
    if (!bad) return AIM_OK;
    for (uint32_t i = 0; i < n_pairs; ++i) {
        const int pl = req8 ? static_cast<const aim_request8_t *>(requests)[i].pattern_len
                            : static_cast<const aim_request_t *>(requests)[i].pattern_len;
        const int tl = req8 ? static_cast<const aim_request8_t *>(requests)[i].text_len
                            : static_cast<const aim_request_t *>(requests)[i].text_len;
        if (pl < 0 || tl < 0 || pl > rs || tl > rs)
            return fail(AIM_EINVAL, "READ LENGTH less than length of the input reads (pair %u)", i);  // host.c:119-123
    }
    return AIM_OK;
}
namespace {

// AIM_FLAG_REF_TEXTS: every window [pos, pos + text_len) inside [0, ref_len) (bit 63 is the strand; an empty window is always
// inside). Scanned branch-free like check_lengths; only a failing scan is repeated to name the pair.
int check_windows(const aim_params_t &p, uint32_t n_pairs, const void *requests, const uint64_t *text_pos, uint64_t ref_len, uint32_t *bad_pair)
{
    const bool req8 = p.flags & AIM_FLAG_REQ8;
    auto tlen = [&](size_t i) -> uint64_t {
        return (uint64_t)(req8 ? static_cast<const aim_request8_t *>(requests)[i].text_len : static_cast<const aim_request_t *>(requests)[i].text_len);
    };
    auto bad = [&](size_t i) -> uint32_t {
        const uint64_t pos = text_pos[i] & ~AIM_REF_MINUS_STRAND, len = tlen(i);   // (lengths are checked >= 0 already)
        return (uint32_t)(len != 0 && (pos > ref_len || len > ref_len - pos));
    };
    if (!n_pairs || !any_nonzero(n_pairs, bad)) return AIM_OK;
    for (uint32_t i = 0; i < n_pairs; ++i)
        if (bad(i)) {
            if (bad_pair) *bad_pair = i;
            return fail(AIM_EINVAL, "text window of pair %u is outside the reference: pos %llu + text_len %llu > ref_len %llu", i,
                        (unsigned long long)(text_pos[i] & ~AIM_REF_MINUS_STRAND), (unsigned long long)tlen(i), (unsigned long long)ref_len);
        }
    return AIM_OK;
}

// AIM_FLAG_REF_TEXTS, packed batch on the fused lane kernel: the general kernel's stage over the to-do list of windows that hold a
// byte outside A/C/G/T (the stage pack_first plans put behind the same kernel). False when it does not fit the slot's scratch.
bool ref_todo_stage(const aim_set *set, const aim_device_ctx &d, size_t scratch_bytes, uint32_t n_pairs, Stage *st)
{
    memset(st, 0, sizeof *st);
    const aim::Knobs kc = set->knobs.cus ? set->knobs : with_chip(set->knobs);
    if (plan_wfa_wave(set->params, std::min<uint32_t>(n_pairs, 1024u * 64u), kc, d.budget, st)) return false;
    return stage_bytes(*st) <= scratch_bytes;
}

int status_error(uint32_t idx, int status)
{
    return fail(AIM_EALIGN, "pair idx %u stopped with status %d (%s)", idx, status,
                status == AIM_PAIR_WFA_NO_LINK ? "Backtrace error: No link found during backtrace"
                : status == AIM_PAIR_SWG_NO_OP ? "SWG backtrace. No backtrace operation found"
                                               : "out of memory");
}

// the configure-time plan re-made for this batch's pair count (smaller grids for smaller batches) under the SAME frozen
// knobs and budget; should that ever need more scratch than configure allocated, the configure-time plan itself is
// followed (every kernel tolerates a grid larger than its work)
Plan plan_for_batch(aim_set *set, aim_device_ctx &d, aim_slot &s, uint32_t n_pairs, uint32_t mode)
{
    Plan pl;
    aim::Knobs quiet = set->knobs;
    quiet.plan_debug = false;   // the configure-time plan was printed; per-launch re-plans are not
    int rc = n_pairs ? make_plan(set->params, n_pairs, quiet, d.budget, &pl, mode) : AIM_OK;
    if (rc || !n_pairs || pl.scratch_total > s.scratch_bytes) pl = d.plan;
    return pl;
}

int launch_on_slot(aim_set *set, aim_device_ctx &d, aim_slot &s, uint32_t mode = 0u, FusedIo *fio = nullptr)
{
    const Plan pl = plan_for_batch(set, d, s, s.n_pairs, mode);
    s.plan_last = pl;
    if (fio && pl.emits_runs) {   // slotted run buffer: pair p owns runs[3p, 3p + 3), the cursor starts behind the slots (wfa_lane_packed.hpp)
        fio->run_slot = (pl.main.kid == K_WFA_LANE_PK && (uint64_t)s.n_pairs * aim::kRunSlot <= fio->runs_cap) ? aim::kRunSlot : 0u;
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)fio->cursor, (int)(s.n_pairs * fio->run_slot), 1, s.stream));
    }
    return launch(pl, set->knobs, set->params, s.n_pairs, s.d_req, s.d_pat, s.d_txt, s.d_res, s.d_ops, s.d_scratch,
                  s.scratch_bytes, s.stream, fio, &s.aux);
}

// aim_sam_t's offsets are 32-bit. CIGAR words <= op bytes and MD bytes <= 2 per op + the digits of one final count, so both cursors stay
// below 2^32 for every batch this admits. It depends on the row count and READ_SIZE only: checked before anything is enqueued.
int check_sam_rows(const aim_params_t &p, uint32_t n_rows)
{
    if ((uint64_t)n_rows * (4ull * (uint64_t)p.read_size + 10ull) >= (1ull << 32))
        return fail(AIM_EINVAL, "SAM records: %u rows of READ_SIZE %d exceed the 32-bit offsets of aim_sam_t (split the batch)", n_rows, p.read_size);
    return AIM_OK;
}
// Which of the two kernels of sam_fields.hpp a launch takes: by READ_SIZE, AIM_SAM_WAVE_MIN overriding the measured switch
inline bool sam_use_wave(const aim_params_t &p, const aim::Knobs &kn)
{
    return p.read_size >= (kn.sam_wave_min >= 0 ? kn.sam_wave_min : aim::kSamWaveMinReadSize);
}

// The SAM kernel over n_rows final rows (sam_fields.hpp), the cursors zeroed first. The caller has run check_sam_rows.
// With seg the split instantiation of the same kernel (aim_sam_device_split), the segments indexed like text_pos.
int enqueue_sam(const aim_params_t &p, const aim::Knobs &kn, aim::SamArgs a, hipStream_t stream, const aim_segment_t *seg = nullptr)
{
    if (!a.n_rows) return AIM_OK;
    a.algo = p.algo;
    a.max_score = p.max_score;
    a.read_size = p.read_size;
    HIP_TRY(hipMemsetAsync(a.cursors, 0, 8, stream));
    if (seg) aim::sam_fields_split_launch(sam_use_wave(p, kn), a, seg, stream);
    else aim::sam_fields_launch(sam_use_wave(p, kn), a, stream);
    HIP_TRY(hipGetLastError());
    return AIM_OK;
}

// AIM_FLAG_SAM_FIELDS on a slot: what aim_set_submit checks before anything is enqueued; *sio receives the struct (nullptr without the flag)
int check_sam_io(const aim_set *set, const aim_slot &s, const aim_batch_io_t *io, const aim_batch_io_sam_t **sio)
{
    *sio = nullptr;
    if (!is_sam(set->params)) return AIM_OK;
    const aim_batch_io_sam_t *x = reinterpret_cast<const aim_batch_io_sam_t *>(io);
    if (!s.d_sam) return fail(AIM_ESTATE, "AIM_FLAG_SAM_FIELDS: aim_set_sam_capacity has not been called since the set was configured");
    if (io->n_pairs && (!x->sam || !x->sam_cigar || !x->sam_md)) return fail(AIM_EINVAL, "AIM_FLAG_SAM_FIELDS: null sam, sam_cigar or sam_md");
    if (x->sam_options & ~AIM_SAM_EQX) return fail(AIM_EINVAL, "AIM_FLAG_SAM_FIELDS: unknown sam_options 0x%x", x->sam_options);
    // (rows are pairs, or reads under AIM_FLAG_READ_GROUPS: never more than n_pairs)
    if (int rc = check_sam_rows(set->params, io->n_pairs)) return rc;
    *sio = x;
    return AIM_OK;
}

// ... the kernel behind the batch's final rows (sel: the reads' candidates under AIM_FLAG_READ_GROUPS, else nullptr)
int enqueue_sam_on_slot(const aim_set *set, const aim_device_ctx &d, aim_slot &s, const aim_batch_io_sam_t *sio, uint32_t n_rows, const uint32_t *sel)
{
    aim::SamArgs a;
    memset(&a, 0, sizeof a);
    a.n_rows = n_rows;
    a.text_pos = s.d_tpos;
    a.sel = sel;
    a.res = static_cast<const aim_result_t *>(s.d_res);
    a.ops = s.d_ops;
    a.ref = d.d_ref;
    a.ref_len = d.ref_len;
    a.options = sio->sam_options;
    a.sam = s.d_sam;
    a.cigar = s.d_samcig;
    a.cigar_cap = std::min(sio->sam_cigar_cap, s.samcig_cap);
    a.md = s.d_sammd;
    a.md_cap = std::min(sio->sam_md_cap, s.sammd_cap);
    a.cursors = s.d_samcur;
    s.io_sam = sio->sam;
    s.io_samcig = sio->sam_cigar;
    s.io_sammd = sio->sam_md;
    s.io_samcig_cap = a.cigar_cap;
    s.io_sammd_cap = a.md_cap;
    return enqueue_sam(set->params, set->knobs, a, s.stream);
}
// ... and its copies back: the records and the cursors now, the words and bytes in aim_set_wait (their count is only known then)
int enqueue_sam_d2h(aim_slot &s, uint32_t n_rows)
{
    HIP_TRY(hipMemcpyAsync(s.h_samcur, s.d_samcur, 8, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipMemcpyAsync(s.io_sam, s.d_sam, (size_t)n_rows * sizeof(aim_sam_t), hipMemcpyDeviceToHost, s.stream));
    return AIM_OK;
}
}  // namespace


extern "C" {

int aim_abi_version(void) { return AIM_ABI_VERSION; }
uint32_t aim_features(void)
{
    return AIM_FEATURE_ENDSFREE | AIM_FEATURE_AFFINE2P | AIM_FEATURE_LINEAR | AIM_FEATURE_WFA_W32 | AIM_FEATURE_WFA_BIDIR | AIM_FEATURE_REF_TEXTS |
           AIM_FEATURE_READ_GROUPS | AIM_FEATURE_WFA_ESCALATE | AIM_FEATURE_MATE_PAIRS | AIM_FEATURE_SAM_FIELDS | AIM_FEATURE_TOP_HITS | AIM_FEATURE_SEED |
           AIM_FEATURE_INDEX_DEVICE | AIM_FEATURE_MINIMIZERS | AIM_FEATURE_SEED_CHAIN | AIM_FEATURE_SEED_CHAIN_LONG | AIM_FEATURE_CHAIN_CLASS | AIM_FEATURE_SPLIT | AIM_FEATURE_EXTEND |
           AIM_FEATURE_MAPPER | AIM_FEATURE_CONTIGS;
}
const char *aim_last_error(void) { return g_err; }

int aim_device_count(int *count)
{
    if (!count) return fail(AIM_EINVAL, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        *count = 0;
        return fail(AIM_ENODEV, "no HIP device: %s", e == hipSuccess ? "device count is 0" : hipGetErrorString(e));
    }
    *count = n;
    return AIM_OK;
}

int aim_set_alloc(uint32_t nr_devices, const int *device_ids, aim_set_t **out)
{
    if (!out || nr_devices == 0) return fail(AIM_EINVAL, "bad arguments");
    int have = 0;
    int rc = aim_device_count(&have);
    if (rc) return rc;
    aim_set *s = new aim_set();
    s->devs.resize(nr_devices);
    for (uint32_t i = 0; i < nr_devices; ++i) {
        const int id = device_ids ? device_ids[i] : (int)i;
        if (id < 0 || id >= have) {
            aim_set_free(s);
            return fail(AIM_ENODEV, "device %d not present (%d devices)", id, have);
        }
        s->devs[i].dev = id;
        hipError_t e = hipSetDevice(id);
        if (e != hipSuccess) {
            aim_set_free(s);
            return fail(AIM_ENODEV, "device %d setup failed: %s", id, hipGetErrorString(e));
        }
    }
    *out = s;
    return AIM_OK;
}

int aim_set_nr_devices(const aim_set_t *set, uint32_t *nr)
{
    if (!set || !nr) return fail(AIM_EINVAL, "bad arguments");
    *nr = (uint32_t)set->devs.size();
    return AIM_OK;
}

int aim_set_configure_slots(aim_set_t *set, const aim_params_t *params, uint32_t max_pairs, uint32_t slots, uint32_t max_raw,
                            uint32_t max_runs)
{
    if (!set || !params || max_pairs == 0 || slots == 0 || slots > 4) return fail(AIM_EINVAL, "bad arguments");
    int rc = validate_params(*params);
    if (rc) return rc;
    if (max_runs && !(params->flags & AIM_FLAG_BACKTRACE)) return fail(AIM_EINVAL, "compact CIGAR output needs AIM_FLAG_BACKTRACE");
    const aim::Knobs kn = read_knobs();
    // From here on the set is unconfigured until every device succeeded: a failure half-way must not leave the old
    // max_pairs / params describing buffers that were already freed or re-sized.
    set->configured = false;
    set->max_pairs = 0;
    for (auto &d : set->devs) free_device_buffers(d);
    const size_t rs = (size_t)params->read_size;
    const size_t rowdw = aim::packed_row_dwords(params->read_size);
    auto configure_slot = [&](aim_device_ctx &d, aim_slot &s) -> int {
        HIP_TRY(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
        for (auto &e : s.ev) HIP_TRY(hipEventCreate(&e));
        // the MRAM plan of host.c:215-241, in HBM (+64 B tail slack on the sequence arrays)
        HIP_TRY(hipMalloc(&s.d_req, (size_t)max_pairs * req_size(*params)));
        HIP_TRY(hipMalloc(&s.d_res, (size_t)max_pairs * res_size(*params)));
        HIP_TRY(hipMalloc((void **)&s.d_pat, (size_t)max_pairs * rs + 64));
        HIP_TRY(hipMalloc((void **)&s.d_txt, (size_t)max_pairs * rs + 64));
        if (params->flags & AIM_FLAG_BACKTRACE) HIP_TRY(hipMalloc((void **)&s.d_ops, (size_t)max_pairs * 2 * rs + 64));
        if (max_raw) {
            HIP_TRY(hipMalloc((void **)&s.d_packP, (size_t)max_pairs * rowdw * 4 + 64));
            HIP_TRY(hipMalloc((void **)&s.d_packT, (size_t)max_pairs * rowdw * 4 + 64));
            HIP_TRY(hipMalloc((void **)&s.d_rawidx, (size_t)max_raw * 4));
            HIP_TRY(hipMalloc((void **)&s.d_rawP, (size_t)max_raw * rs + 64));   // (+64 B: the raw side pass hands them to the ASCII kernels as patterns / texts, aim_hip.h tail slack)
            HIP_TRY(hipMalloc((void **)&s.d_rawT, (size_t)max_raw * rs + 64));
            HIP_TRY(hipMalloc(&s.d_rawreq, (size_t)max_raw * req_size(*params)));
            HIP_TRY(hipMalloc(&s.d_rawres, (size_t)max_raw * res_size(*params)));
            if (params->flags & AIM_FLAG_BACKTRACE) HIP_TRY(hipMalloc((void **)&s.d_rawops, (size_t)max_raw * 2 * rs + 64));
            if (max_runs) HIP_TRY(hipMalloc((void **)&s.d_rawcig, (size_t)max_raw * sizeof(aim_cigar_t)));
        }
        if (is_ref(*params)) {
            HIP_TRY(hipMalloc((void **)&s.d_tpos, (size_t)max_pairs * 8));
            if (max_raw && params->algo == AIM_ALGO_WFA)
                HIP_TRY(hipMalloc((void **)&s.d_reftodo, 64 + (size_t)max_pairs * 4 + ((size_t)max_pairs + 31) / 32 * 4));
        }
        if (is_groups(*params)) {
            HIP_TRY(hipMalloc((void **)&s.g_readP, (size_t)max_pairs * rs + 64));
            HIP_TRY(hipMalloc((void **)&s.g_roff, ((size_t)max_pairs + 1) * 4));
            HIP_TRY(hipMalloc((void **)&s.g_map, (size_t)max_pairs * 4));
            HIP_TRY(hipMalloc((void **)&s.g_sel, (size_t)max_pairs * 4));
            if (max_raw) HIP_TRY(hipMalloc((void **)&s.g_rawslot, (size_t)max_pairs * 4));
            HIP_TRY(hipMalloc((void **)&s.g_res1, (size_t)max_pairs * sizeof(aim_result_t)));
            HIP_TRY(hipMalloc((void **)&s.g_best, (size_t)max_pairs * sizeof(aim_best_t)));
            if (is_mates(*params)) HIP_TRY(hipMalloc((void **)&s.g_mates, ((size_t)max_pairs / 2 + 1) * sizeof(aim_mate_t)));
            if (is_hits(*params)) {
                HIP_TRY(hipMalloc((void **)&s.g_hoff, ((size_t)max_pairs + 1) * 4));
                HIP_TRY(hipMalloc((void **)&s.g_hit, (size_t)max_pairs * 4));
            }
            if (params->flags & AIM_FLAG_BACKTRACE) {
                HIP_TRY(hipMalloc(&s.g_req2, (size_t)max_pairs * req_size(*params)));
                HIP_TRY(hipMalloc((void **)&s.g_pat2, (size_t)max_pairs * rs + 64));
                HIP_TRY(hipMalloc((void **)&s.g_txt2, (size_t)max_pairs * rs + 64));
            }
        }
        if (max_runs) {
            HIP_TRY(hipMalloc((void **)&s.d_cig, (size_t)max_pairs * sizeof(aim_cigar_t)));
            HIP_TRY(hipMalloc((void **)&s.d_runs, (size_t)max_runs * 4));
            HIP_TRY(hipMalloc((void **)&s.d_cursor, 64));
            HIP_TRY(hipHostMalloc((void **)&s.h_cursor, 64, hipHostMallocDefault));
        }
        return AIM_OK;
    };
    auto configure_device = [&](aim_device_ctx &d) -> int {
        HIP_TRY(hipSetDevice(d.dev));
        d.slots.resize(slots);
        for (auto &s : d.slots) {
            int src = configure_slot(d, s);
            if (src) return src;
        }
        // scratch bound of one slot of THIS device, after the fixed buffers exist; halved and re-planned if the allocation
        // still fails
        if (kn.scratch_gb >= 0) {
            d.budget = (uint64_t)(kn.scratch_gb * (double)(1ull << 30)) / slots;
        } else {
            size_t free_b = 0, total_b = 0;
            HIP_TRY(hipMemGetInfo(&free_b, &total_b));
            d.budget = budget_from_free(free_b / slots);
        }
        for (int attempt = 0;; ++attempt) {
            size_t want = 0;
            if (is_groups(*params)) {   // the two passes share the slot's scratch, one after the other
                GroupsPlan g;
                int prc = make_groups_plan(*params, max_pairs, kn, d.budget, &g);
                if (prc) return prc;
                d.plan = g.p1;
                d.plan2 = g.p2;
                want = g.plan_bytes;
            } else {
                int prc = make_plan(*params, max_pairs, kn, d.budget, &d.plan);
                if (prc) return prc;
                want = d.plan.scratch_total;
            }
            if (is_ref(*params) && max_raw && params->algo == AIM_ALGO_WFA) {   // room for the to-do stage of fused packed batches
                Stage st;
                memset(&st, 0, sizeof st);
                if (!plan_wfa_wave(*params, std::min<uint32_t>(max_pairs, 1024u * 64u), kn.cus ? kn : with_chip(kn), d.budget, &st))
                    want = std::max(want, stage_bytes(st));
            }
            hipError_t e = hipSuccess;
            for (auto &s : d.slots) {
                s.scratch_bytes = want;
                if (want && (e = hipMalloc(&s.d_scratch, want)) != hipSuccess) break;
            }
            if (e == hipSuccess) break;
            (void)hipGetLastError();
            for (auto &s : d.slots) {
                if (s.d_scratch) (void)hipFree(s.d_scratch);
                s.d_scratch = nullptr;
            }
            if (e != hipErrorOutOfMemory || attempt >= 6 || d.budget <= ((uint64_t)1 << 28))
                return fail(e == hipErrorOutOfMemory ? AIM_ENOMEM : AIM_ENODEV, "hipMalloc(scratch, %zu bytes) failed: %s",
                            want, hipGetErrorString(e));
            d.budget /= 2;
        }
        for (auto &s : d.slots) {
            // Debugging aid: AIM_DEBUG_POISON_SCRATCH=<0..255> fills the scratch with that byte. Results must not depend on
            // it (every scratch byte a launch reads must have been written by that launch). On
            // the slot's own stream and completed here: launches run on non-blocking streams that do not synchronise with
            // the null stream.
            if (s.scratch_bytes && kn.poison_scratch >= 0) {
                HIP_TRY(hipMemsetAsync(s.d_scratch, kn.poison_scratch & 0xff, s.scratch_bytes, s.stream));
                HIP_TRY(hipStreamSynchronize(s.stream));
            }
            s.n_pairs = 0;
            s.pushed = s.launched = s.submitted = false;
            s.plan_last = d.plan;
            s.plan_last2 = d.plan2;
            s.n_reads = 0;
        }
        return AIM_OK;
    };
    for (auto &d : set->devs) {
        rc = configure_device(d);
        if (rc) {
            char keep[sizeof g_err];
            memcpy(keep, g_err, sizeof keep);
            for (auto &x : set->devs) free_device_buffers(x);   // nothing half-configured survives
            memcpy(g_err, keep, sizeof keep);
            return rc;
        }
    }
    set->xparams = copy_params(*params);
    set->max_pairs = max_pairs;
    set->max_raw = max_raw;
    set->max_runs = max_runs;
    set->knobs = kn;
    set->configured = true;
    return AIM_OK;
}

int aim_set_configure(aim_set_t *set, const aim_params_t *params, uint32_t max_pairs)
{
    return aim_set_configure_slots(set, params, max_pairs, 1, 0, 0);
}

namespace {
const char *const kGroupsSubmitOnly = "AIM_FLAG_READ_GROUPS is set: batches go through aim_set_submit with an aim_batch_io_groups_t";
const char *const kSamStateless = "AIM_FLAG_SAM_FIELDS is set: the records come from aim_set_submit (aim_batch_io_sam_t) or, after a flag-less call, from aim_sam_device";
const char *const kSamSubmitOnly = "AIM_FLAG_SAM_FIELDS is set: batches go through aim_set_submit with an aim_batch_io_sam_t";

// aim_set_push (texts != nullptr) and aim_set_push_ref (text_pos != nullptr)
int push_impl(aim_set_t *set, uint32_t device, uint32_t n_pairs, const void *requests, const char *patterns, const char *texts,
              const uint64_t *text_pos)
{
    if (!set || device >= set->devs.size()) return fail(AIM_EINVAL, "bad device index");
    if (!set->configured) return fail(AIM_ESTATE, "aim_set_configure has not been called");
    if (is_groups(set->params)) return fail(AIM_EINVAL, kGroupsSubmitOnly);
    if (is_sam(set->params)) return fail(AIM_EINVAL, kSamSubmitOnly);
    if (n_pairs > set->max_pairs) return fail(AIM_EINVAL, "n_pairs %u exceeds configured capacity %u", n_pairs, set->max_pairs);
    if (n_pairs && (!requests || !patterns || (!texts && !text_pos))) return fail(AIM_EINVAL, "null host buffer");
    aim_device_ctx &d = set->devs[device];
    aim_slot &s = d.slots[0];
    if (s.submitted) return fail(AIM_ESTATE, "slot 0 of device %d holds a submitted batch: aim_set_wait it first", d.dev);
    const size_t rs = (size_t)set->params.read_size;
    int rc = check_lengths(set->params, n_pairs, requests);
    if (rc) return rc;
    if (text_pos) {
        if (!d.d_ref) return fail(AIM_ESTATE, "AIM_FLAG_REF_TEXTS: no reference on device %d (aim_set_reference)", d.dev);
        rc = check_windows(set->params, n_pairs, requests, text_pos, d.ref_len, nullptr);
        if (rc) return rc;
    }
    HIP_TRY(hipSetDevice(d.dev));
    HIP_TRY(hipEventRecord(s.ev[0], s.stream));
    if (n_pairs) {
        HIP_TRY(hipMemcpyAsync(s.d_req, requests, (size_t)n_pairs * req_size(set->params), hipMemcpyHostToDevice, s.stream));
        HIP_TRY(hipMemcpyAsync(s.d_pat, patterns, (size_t)n_pairs * rs, hipMemcpyHostToDevice, s.stream));
        if (text_pos) HIP_TRY(hipMemcpyAsync(s.d_tpos, text_pos, (size_t)n_pairs * 8, hipMemcpyHostToDevice, s.stream));
        else HIP_TRY(hipMemcpyAsync(s.d_txt, texts, (size_t)n_pairs * rs, hipMemcpyHostToDevice, s.stream));
    }
    HIP_TRY(hipEventRecord(s.ev[1], s.stream));
    s.n_pairs = n_pairs;
    s.pushed = true;
    s.launched = false;
    s.ref_pending = text_pos != nullptr;
    return AIM_OK;
}
}  // namespace

int aim_set_push(aim_set_t *set, uint32_t device, uint32_t n_pairs, const void *requests, const char *patterns,
                 const char *texts)
{
    if (set && set->configured && is_ref(set->params))
        return fail(AIM_EINVAL, "AIM_FLAG_REF_TEXTS is set: the texts are named by text_pos (aim_set_push_ref)");
    return push_impl(set, device, n_pairs, requests, patterns, texts, nullptr);
}

int aim_set_push_ref(aim_set_t *set, uint32_t device, uint32_t n_pairs, const void *requests, const char *patterns,
                     const uint64_t *text_pos)
{
    if (set && set->configured && !is_ref(set->params)) return fail(AIM_EINVAL, "aim_set_push_ref needs AIM_FLAG_REF_TEXTS");
    if (n_pairs && !text_pos) return fail(AIM_EINVAL, "null text_pos");
    return push_impl(set, device, n_pairs, requests, patterns, nullptr, text_pos);
}

int aim_set_launch(aim_set_t *set)
{
    if (!set || !set->configured) return fail(AIM_ESTATE, "set is not configured");
    if (is_groups(set->params)) return fail(AIM_EINVAL, kGroupsSubmitOnly);
    if (is_sam(set->params)) return fail(AIM_EINVAL, kSamSubmitOnly);
    for (auto &d : set->devs) {
        aim_slot &s = d.slots[0];
        if (!s.pushed) return fail(AIM_ESTATE, "device %d has no pushed batch", d.dev);
        HIP_TRY(hipSetDevice(d.dev));
        HIP_TRY(hipEventRecord(s.ev[2], s.stream));
        if (s.ref_pending && s.n_pairs) {   // AIM_FLAG_REF_TEXTS: the windows into the text rows, ahead of the plan's stages
            aim::KArgs ka;
            memset(&ka, 0, sizeof ka);
            ka.p = set->params;
            ka.n_pairs = s.n_pairs;
            ka.req = static_cast<const aim_request_t *>(s.d_req);
            int grc = enqueue_gather(ka, s.d_tpos, d.d_ref, d.ref_len, nullptr, s.n_pairs, s.d_txt, s.stream);
            if (grc) return grc;
        }
        int rc = launch_on_slot(set, d, s);
        if (rc) return rc;
        HIP_TRY(hipEventRecord(s.ev[3], s.stream));
    }
    float worst_h2d = 0.f, worst_k = 0.f;
    for (auto &d : set->devs) {   // DPU_SYNCHRONOUS: wait for every device
        aim_slot &s = d.slots[0];
        HIP_TRY(hipSetDevice(d.dev));
        HIP_TRY(hipStreamSynchronize(s.stream));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, s.ev[0], s.ev[1]));
        worst_h2d = std::max(worst_h2d, ms);
        HIP_TRY(hipEventElapsedTime(&ms, s.ev[2], s.ev[3]));
        worst_k = std::max(worst_k, ms);
        s.launched = true;
    }
    set->h2d_ms += worst_h2d;
    set->kernel_ms += worst_k;
    return AIM_OK;
}

int aim_set_pull(aim_set_t *set, uint32_t device, void *results, char *ops)
{
    if (!set || device >= set->devs.size()) return fail(AIM_EINVAL, "bad device index");
    if (!set->configured) return fail(AIM_ESTATE, "aim_set_configure has not been called");
    if (is_groups(set->params)) return fail(AIM_EINVAL, kGroupsSubmitOnly);
    if (is_sam(set->params)) return fail(AIM_EINVAL, kSamSubmitOnly);
    aim_device_ctx &d = set->devs[device];
    aim_slot &s = d.slots[0];
    if (!s.launched) return fail(AIM_ESTATE, "device %d has not been launched", d.dev);
    const bool bt = set->params.flags & AIM_FLAG_BACKTRACE;
    if (s.n_pairs && (!results || (bt && !ops))) return fail(AIM_EINVAL, "null host buffer");
    const size_t rs = (size_t)set->params.read_size;
    HIP_TRY(hipSetDevice(d.dev));
    HIP_TRY(hipEventRecord(s.ev[4], s.stream));
    if (s.n_pairs) {
        HIP_TRY(hipMemcpyAsync(results, s.d_res, (size_t)s.n_pairs * res_size(set->params), hipMemcpyDeviceToHost, s.stream));
        if (bt) HIP_TRY(hipMemcpyAsync(ops, s.d_ops, (size_t)s.n_pairs * 2 * rs, hipMemcpyDeviceToHost, s.stream));
    }
    HIP_TRY(hipEventRecord(s.ev[5], s.stream));
    HIP_TRY(hipStreamSynchronize(s.stream));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s.ev[4], s.ev[5]));
    set->d2h_ms += ms;
    if (set->params.flags & AIM_FLAG_RES8) return AIM_OK;   // score-only: no status other than AIM_PAIR_OK exists
    const aim_result_t *r = static_cast<const aim_result_t *>(results);
    for (uint32_t i = 0; i < s.n_pairs; ++i)
        if (r[i].status != AIM_PAIR_OK) return status_error(r[i].idx, r[i].status);
    return AIM_OK;
}

namespace {
// aim_groups_check: the CSR of a groups batch, the first bad read named
int check_groups(uint32_t n_pairs, uint32_t n_reads, const uint32_t *roff, uint32_t *bad_read)
{
    auto bad = [&](uint32_t r, const char *what) {
        if (bad_read) *bad_read = r;
        return fail(AIM_EINVAL, "read_offsets: read %u %s", r, what);
    };
    if (!n_reads) return n_pairs ? fail(AIM_EINVAL, "read_offsets: %u candidates but no read", n_pairs) : AIM_OK;
    if (!roff) return fail(AIM_EINVAL, "read_offsets is NULL");
    if (roff[0] != 0) return bad(0, "does not start at offset 0");
    for (uint32_t r = 0; r < n_reads; ++r) {
        if (roff[r + 1] < roff[r]) return bad(r, "ends before it starts (offsets decrease)");
        if (roff[r + 1] == roff[r]) return bad(r, "has no candidate");
        if (roff[r + 1] > n_pairs) return bad(r, "runs past n_pairs");
    }
    if (roff[n_reads] != n_pairs) return bad(n_reads - 1, "is the last and does not end at n_pairs");
    return AIM_OK;
}

// A plan of one pass for this batch's size under the set's frozen knobs and budget; the configure-time plan when it would need more
// scratch than the slot holds (every kernel tolerates a grid larger than its work)
Plan pass_plan(const aim_set *set, const aim_device_ctx &d, const aim_slot &s, const aim_params_t &pp, uint32_t n, const Plan &configured)
{
    Plan pl;
    aim::Knobs quiet = set->knobs;
    quiet.plan_debug = false;
    if (make_plan(pp, n, quiet, d.budget, &pl) || pl.scratch_total > s.scratch_bytes) pl = configured;
    return pl;
}

// aim_mates_check: the read pairs and the pairing parameters of a mate-pairs batch
int check_mates(uint32_t n_reads, int64_t min_span, int64_t max_span, int32_t unpaired_penalty)
{
    if (n_reads & 1u) return fail(AIM_EINVAL, "AIM_FLAG_MATE_PAIRS: n_reads %u is odd (reads 2m and 2m + 1 are mates)", n_reads);
    if (min_span < 0 || max_span < min_span || max_span >= ((int64_t)1 << 62))
        return fail(AIM_EINVAL, "AIM_FLAG_MATE_PAIRS: bad span [%lld, %lld]: need 0 <= min_span <= max_span < 2^62", (long long)min_span,
                    (long long)max_span);
    if (unpaired_penalty < 0) return fail(AIM_EINVAL, "AIM_FLAG_MATE_PAIRS: unpaired_penalty %d is negative", unpaired_penalty);
    return AIM_OK;
}

// aim_hits_offsets: the exclusive prefix sum of min(K_r, max_hits)
int hits_offsets(uint32_t n_reads, const uint32_t *roff, uint32_t max_hits, uint32_t *hoff, uint32_t *n_hits)
{
    if (max_hits < 1 || max_hits > AIM_TOP_HITS_MAX)
        return fail(AIM_EINVAL, "AIM_FLAG_TOP_HITS: max_hits %u is outside 1..%d", max_hits, AIM_TOP_HITS_MAX);
    if (!roff || !hoff) return fail(AIM_EINVAL, "AIM_FLAG_TOP_HITS: null read_offsets or hit_offsets");
    uint32_t h = 0;
    for (uint32_t r = 0; r < n_reads; ++r) {
        hoff[r] = h;
        h += std::min(roff[r + 1] > roff[r] ? roff[r + 1] - roff[r] : 0u, max_hits);
    }
    hoff[n_reads] = h;
    if (n_hits) *n_hits = h;
    return AIM_OK;
}

// AIM_FLAG_TOP_HITS on a slot: the caller's hit_offsets against the CSR (already checked), before anything is enqueued; *n_hits receives H
int check_hits_io(const aim_batch_io_hits_t *hio, uint32_t n_reads, const uint32_t *roff, uint32_t *n_hits)
{
    if (hio->max_hits < 1 || hio->max_hits > AIM_TOP_HITS_MAX)
        return fail(AIM_EINVAL, "AIM_FLAG_TOP_HITS: max_hits %u is outside 1..%d", hio->max_hits, AIM_TOP_HITS_MAX);
    *n_hits = 0;
    if (!n_reads) return AIM_OK;
    if (!hio->hit_offsets) return fail(AIM_EINVAL, "AIM_FLAG_TOP_HITS: null hit_offsets");
    uint32_t h = 0;
    for (uint32_t r = 0; r < n_reads; ++r) {
        if (hio->hit_offsets[r] != h)
            return fail(AIM_EINVAL, "AIM_FLAG_TOP_HITS: hit_offsets[%u] = %u, but the hits of read %u start at row %u (aim_hits_offsets)", r,
                        hio->hit_offsets[r], r, h);
        h += std::min(roff[r + 1] - roff[r], hio->max_hits);
    }
    if (hio->hit_offsets[n_reads] != h)
        return fail(AIM_EINVAL, "AIM_FLAG_TOP_HITS: hit_offsets[%u] = %u, but the hits of read %u end at row %u (aim_hits_offsets)", n_reads,
                    hio->hit_offsets[n_reads], n_reads - 1, h);
    *n_hits = h;
    return AIM_OK;
}

// aim_set_submit under AIM_FLAG_READ_GROUPS
int submit_groups(aim_set *set, aim_device_ctx &d, aim_slot &s, const aim_batch_io_t *io)
{
    const aim_params_t &p = set->params;
    const aim_batch_io_groups_t *gio = reinterpret_cast<const aim_batch_io_groups_t *>(io);
    const uint32_t n = io->n_pairs, nr = gio->n_reads;
    const bool bt = p.flags & AIM_FLAG_BACKTRACE;
    const bool ref = is_ref(p);
    const bool packed = io->packed_patterns || io->packed_texts;
    // AIM_FLAG_MATE_PAIRS: io is the base of an aim_batch_io_mates_t
    const aim_batch_io_mates_t *mio = is_mates(p) ? reinterpret_cast<const aim_batch_io_mates_t *>(io) : nullptr;
    // AIM_FLAG_TOP_HITS: io is the base of an aim_batch_io_hits_t
    const aim_batch_io_hits_t *hio = is_hits(p) ? reinterpret_cast<const aim_batch_io_hits_t *>(io) : nullptr;
    if (packed && (!ref || io->packed_texts))
        return fail(AIM_EINVAL, "AIM_FLAG_READ_GROUPS: packed batches need AIM_FLAG_REF_TEXTS (packed explicit texts are a follow-up)");
    if (packed && (!s.d_packP || !s.g_rawslot)) return fail(AIM_EINVAL, "packed batch needs a set configured with max_raw_pairs > 0");
    if (packed && io->n_raw > set->max_raw) return fail(AIM_EINVAL, "n_raw %u exceeds configured capacity %u", io->n_raw, set->max_raw);
    if (packed && io->n_raw && (!io->raw_pairs || !io->raw_patterns)) return fail(AIM_EINVAL, "null raw side list");
    if (!packed && io->n_raw) return fail(AIM_EINVAL, "a raw side list needs a packed batch");
    if (ref && (io->texts || io->raw_texts)) return fail(AIM_EINVAL, "AIM_FLAG_REF_TEXTS: texts, packed_texts and raw_texts must be NULL (the texts are named by text_pos)");
    if (ref && n && !gio->text_pos) return fail(AIM_EINVAL, "AIM_FLAG_REF_TEXTS: null text_pos");
    if (!ref && gio->text_pos) return fail(AIM_EINVAL, "text_pos needs AIM_FLAG_REF_TEXTS");
    if (ref && !d.d_ref) return fail(AIM_ESTATE, "AIM_FLAG_REF_TEXTS: no reference on device %d (aim_set_reference)", d.dev);
    if (n > set->max_pairs) return fail(AIM_EINVAL, "n_pairs %u exceeds configured capacity %u", n, set->max_pairs);
    if (n && (!io->requests || (!packed && !io->patterns) || (!ref && !io->texts))) return fail(AIM_EINVAL, "null requests or sequence rows");
    if (io->cigars && (!bt || !s.d_cig || !io->runs)) return fail(AIM_EINVAL, "compact CIGAR needs AIM_FLAG_BACKTRACE, max_runs > 0 and a run buffer");
    const aim_batch_io_sam_t *sio = nullptr;
    int rc = check_sam_io(set, s, io, &sio);
    if (rc) return rc;
    if (n && !io->results && !io->cigars && !gio->best && !(mio && mio->mates) && !sio && !(hio && hio->hit_pair)) return fail(AIM_EINVAL, "no output buffer");
    if (io->ops && !bt) return fail(AIM_EINVAL, "ops requested without AIM_FLAG_BACKTRACE");
    rc = check_groups(n, nr, gio->read_offsets, nullptr);
    if (rc) return rc;
    if (mio) {
        rc = check_mates(nr, mio->min_span, mio->max_span, mio->unpaired_penalty);
        if (rc) return rc;
    }
    uint32_t rows = nr;   // the batch's output rows: reads, or hits
    if (hio) {
        rc = check_hits_io(hio, nr, gio->read_offsets, &rows);
        if (rc) return rc;
    }
    if (packed)   // the side list names reads
        for (uint32_t j = 0; j < io->n_raw; ++j)
            if (io->raw_pairs[j] >= nr) return fail(AIM_EINVAL, "raw_pairs[%u] = %u is outside the batch's %u reads", j, io->raw_pairs[j], nr);
    rc = check_lengths(p, n, io->requests);
    if (rc) return rc;
    if (ref) {
        rc = check_windows(p, n, io->requests, gio->text_pos, d.ref_len, nullptr);
        if (rc) return rc;
    }
    const size_t rs = (size_t)p.read_size;
    HIP_TRY(hipSetDevice(d.dev));
    s.io = *io;
    s.n_pairs = rows;        // aim_set_wait reads n_pairs output rows
    s.n_reads = nr;
    s.io_sam = nullptr;
    s.runs_sent = 0;
    s.pushed = s.launched = false;
    s.ref_pending = false;
    GroupsPlan g;
    memset(&g, 0, sizeof g);
    g.x1 = groups_pass_params(p, AIM_FLAG_BACKTRACE | AIM_FLAG_WFA_BIDIR | AIM_FLAG_RES8);
    g.x2 = groups_pass_params(p, 0u);
    g.pass2 = bt;
    g.mates = mio != nullptr;
    g.sam = is_sam(p);
    g.hits = hio != nullptr;
    auto enqueue = [&]() -> int {
        HIP_TRY(hipEventRecord(s.ev[0], s.stream));
        if (n) {
            HIP_TRY(hipMemcpyAsync(s.d_req, io->requests, (size_t)n * req_size(p), hipMemcpyHostToDevice, s.stream));
            HIP_TRY(hipMemcpyAsync(s.g_roff, gio->read_offsets, ((size_t)nr + 1) * 4, hipMemcpyHostToDevice, s.stream));
            if (hio) HIP_TRY(hipMemcpyAsync(s.g_hoff, hio->hit_offsets, ((size_t)nr + 1) * 4, hipMemcpyHostToDevice, s.stream));
            if (packed) {
                HIP_TRY(hipMemcpyAsync(s.d_packP, io->packed_patterns, (size_t)nr * aim::packed_row_dwords(p.read_size) * 4, hipMemcpyHostToDevice, s.stream));
                if (io->n_raw) {
                    HIP_TRY(hipMemcpyAsync(s.d_rawidx, io->raw_pairs, (size_t)io->n_raw * 4, hipMemcpyHostToDevice, s.stream));
                    HIP_TRY(hipMemcpyAsync(s.d_rawP, io->raw_patterns, (size_t)io->n_raw * rs, hipMemcpyHostToDevice, s.stream));
                }
            } else {
                HIP_TRY(hipMemcpyAsync(s.g_readP, io->patterns, (size_t)nr * rs, hipMemcpyHostToDevice, s.stream));
            }
            if (ref) HIP_TRY(hipMemcpyAsync(s.d_tpos, gio->text_pos, (size_t)n * 8, hipMemcpyHostToDevice, s.stream));
            else HIP_TRY(hipMemcpyAsync(s.d_txt, io->texts, (size_t)n * rs, hipMemcpyHostToDevice, s.stream));
        }
        HIP_TRY(hipEventRecord(s.ev[1], s.stream));
        HIP_TRY(hipEventRecord(s.ev[2], s.stream));
        if (n) {
            if (ref) {
                aim::KArgs ka;
                memset(&ka, 0, sizeof ka);
                ka.p = p;
                ka.n_pairs = n;
                ka.req = static_cast<const aim_request_t *>(s.d_req);
                int grc = enqueue_gather(ka, s.d_tpos, d.d_ref, d.ref_len, nullptr, n, s.d_txt, s.stream);
                if (grc) return grc;
            }
            const Plan pl1 = pass_plan(set, d, s, g.x1.base, n, d.plan);
            const Plan pl2 = bt ? pass_plan(set, d, s, g.x2.base, rows, d.plan2) : Plan();
            s.plan_last = pl1;
            s.plan_last2 = pl2;
            GroupsIo gi;
            gi.n_pairs = n;
            gi.n_reads = nr;
            gi.req = s.d_req;
            gi.read_rows = packed ? nullptr : s.g_readP;
            gi.packed = s.d_packP;
            gi.raw_pairs = s.d_rawidx;
            gi.raw_rows = s.d_rawP;
            gi.n_raw = packed ? io->n_raw : 0u;
            gi.raw_slot = s.g_rawslot;
            gi.roff = s.g_roff;
            gi.cand_p = s.d_pat;
            gi.cand_t = s.d_txt;
            gi.res1 = s.g_res1;
            gi.map = s.g_map;
            gi.sel = s.g_sel;
            gi.best = s.g_best;
            gi.tpos = s.d_tpos;
            memset(&gi.mate, 0, sizeof gi.mate);
            if (mio) {
                gi.mate.min_span = mio->min_span;
                gi.mate.max_span = mio->max_span;
                gi.mate.unpaired_penalty = mio->unpaired_penalty;
            }
            gi.mates = s.g_mates;
            gi.n_hits = hio ? rows : 0u;
            gi.max_hits = hio ? hio->max_hits : 0u;
            gi.hoff = s.g_hoff;
            gi.hit_pair = s.g_hit;
            gi.req2 = s.g_req2;
            gi.pat2 = s.g_pat2;
            gi.txt2 = s.g_txt2;
            gi.res = s.d_res;
            gi.ops = s.d_ops;
            gi.scratch = s.d_scratch;
            gi.scratch_bytes = s.scratch_bytes;
            int erc = enqueue_groups(g, pl1, pl2, set->knobs, gi, s.stream, &s.aux);
            if (erc) return erc;
            if (io->cigars) {
                aim::KArgs k2;
                memset(&k2, 0, sizeof k2);
                k2.p = g.x2.base;
                k2.n_pairs = rows;
                k2.req = static_cast<const aim_request_t *>(s.g_req2);
                k2.res = static_cast<aim_result_t *>(s.d_res);
                k2.ops = s.d_ops;
                HIP_TRY(hipMemsetAsync(s.d_cursor, 0, 4, s.stream));
                hipLaunchKernelGGL(aim::cigar_rle_kernel, dim3((rows + 63) / 64), dim3(64), 0, s.stream, k2, s.d_cig, s.d_runs,
                                   std::min(io->runs_cap, set->max_runs), s.d_cursor);
                HIP_TRY(hipGetLastError());
            }
            if (sio) {   // the reads' records: row r is candidate sel[r]
                int src = enqueue_sam_on_slot(set, d, s, sio, nr, s.g_sel);
                if (src) return src;
            }
        }
        HIP_TRY(hipEventRecord(s.ev[3], s.stream));
        HIP_TRY(hipEventRecord(s.ev[4], s.stream));
        if (n) {
            if (gio->best) HIP_TRY(hipMemcpyAsync(gio->best, s.g_best, (size_t)nr * sizeof(aim_best_t), hipMemcpyDeviceToHost, s.stream));
            if (mio && mio->mates && nr >= 2)
                HIP_TRY(hipMemcpyAsync(mio->mates, s.g_mates, (size_t)(nr / 2) * sizeof(aim_mate_t), hipMemcpyDeviceToHost, s.stream));
            if (io->cigars) {
                HIP_TRY(hipMemcpyAsync(s.h_cursor, s.d_cursor, 4, hipMemcpyDeviceToHost, s.stream));
                HIP_TRY(hipMemcpyAsync(io->cigars, s.d_cig, (size_t)rows * sizeof(aim_cigar_t), hipMemcpyDeviceToHost, s.stream));
            }
            if (io->results) HIP_TRY(hipMemcpyAsync(io->results, s.d_res, (size_t)rows * res_size(p), hipMemcpyDeviceToHost, s.stream));
            if (io->ops) HIP_TRY(hipMemcpyAsync(io->ops, s.d_ops, (size_t)rows * 2 * rs, hipMemcpyDeviceToHost, s.stream));
            if (hio && hio->hit_pair) HIP_TRY(hipMemcpyAsync(hio->hit_pair, s.g_hit, (size_t)rows * 4, hipMemcpyDeviceToHost, s.stream));
            if (sio) {
                int src = enqueue_sam_d2h(s, nr);
                if (src) return src;
            }
        }
        HIP_TRY(hipEventRecord(s.ev[5], s.stream));
        return AIM_OK;
    };
    rc = enqueue();
    if (rc) {   // (as aim_set_submit: nothing stays in flight on a failed submit)
        char keep[sizeof g_err];
        memcpy(keep, g_err, sizeof keep);
        (void)hipStreamSynchronize(s.stream);
        (void)hipGetLastError();
        memcpy(g_err, keep, sizeof keep);
        return rc;
    }
    s.submitted = true;
    return AIM_OK;
}
}  // namespace

int aim_set_submit(aim_set_t *set, uint32_t device, uint32_t slot, const aim_batch_io_t *io)
{
    if (!set || device >= set->devs.size() || !io) return fail(AIM_EINVAL, "bad arguments");
    if (!set->configured) return fail(AIM_ESTATE, "aim_set_configure has not been called");
    aim_device_ctx &d = set->devs[device];
    if (slot >= d.slots.size()) return fail(AIM_EINVAL, "slot %u not configured (%zu slots)", slot, d.slots.size());
    aim_slot &s = d.slots[slot];
    if (s.submitted) return fail(AIM_ESTATE, "slot %u of device %d holds a batch: aim_set_wait it first", slot, d.dev);
    if (is_groups(set->params)) return submit_groups(set, d, s, io);
    const aim_params_t &p = set->params;
    const uint32_t n = io->n_pairs;
    const bool bt = p.flags & AIM_FLAG_BACKTRACE;
    // AIM_FLAG_REF_TEXTS: io is the base of an aim_batch_io_ref_t and the texts are windows of the device's reference
    const bool ref = is_ref(p);
    const uint64_t *text_pos = ref ? reinterpret_cast<const aim_batch_io_ref_t *>(io)->text_pos : nullptr;
    if (ref && (io->texts || io->packed_texts || io->raw_texts))
        return fail(AIM_EINVAL, "AIM_FLAG_REF_TEXTS: texts, packed_texts and raw_texts must be NULL (the texts are named by text_pos)");
    if (ref && n && !text_pos) return fail(AIM_EINVAL, "AIM_FLAG_REF_TEXTS: null text_pos");
    if (ref && !d.d_ref) return fail(AIM_ESTATE, "AIM_FLAG_REF_TEXTS: no reference on device %d (aim_set_reference)", d.dev);
    const bool packed = io->packed_patterns || io->packed_texts;
    if (n > set->max_pairs) return fail(AIM_EINVAL, "n_pairs %u exceeds configured capacity %u", n, set->max_pairs);
    if (n && !io->requests) return fail(AIM_EINVAL, "null requests");
    if (n && packed && (!io->packed_patterns || (!ref && !io->packed_texts) || !s.d_packP))
        return fail(AIM_EINVAL, "packed batch needs both packed arrays and a set configured with max_raw_pairs > 0");
    if (n && !packed && (!io->patterns || (!ref && !io->texts))) return fail(AIM_EINVAL, "null sequence rows");
    if (packed && io->n_raw > set->max_raw) return fail(AIM_EINVAL, "n_raw %u exceeds configured capacity %u", io->n_raw, set->max_raw);
    if (packed && io->n_raw && (!io->raw_pairs || !io->raw_patterns || (!ref && !io->raw_texts))) return fail(AIM_EINVAL, "null raw side list");
    if (io->cigars && (!bt || !s.d_cig || !io->runs)) return fail(AIM_EINVAL, "compact CIGAR needs AIM_FLAG_BACKTRACE, max_runs > 0 and a run buffer");
    const aim_batch_io_sam_t *sio = nullptr;
    int rc = check_sam_io(set, s, io, &sio);
    if (rc) return rc;
    if (n && !io->results && !io->cigars && !sio) return fail(AIM_EINVAL, "no output buffer");
    if (io->ops && !bt) return fail(AIM_EINVAL, "ops requested without AIM_FLAG_BACKTRACE");
    rc = check_lengths(p, n, io->requests);
    if (rc) return rc;
    if (ref) {
        rc = check_windows(p, n, io->requests, text_pos, d.ref_len, nullptr);
        if (rc) return rc;
    }
    if (packed)
        for (uint32_t j = 0; j < io->n_raw; ++j)
            if (io->raw_pairs[j] >= n) return fail(AIM_EINVAL, "raw_pairs[%u] = %u is outside the batch", j, io->raw_pairs[j]);
    const size_t rs = (size_t)p.read_size;
    const size_t rowb = (size_t)aim::packed_row_dwords(p.read_size) * 4;
    HIP_TRY(hipSetDevice(d.dev));
    s.io = *io;
    s.n_pairs = n;
    s.io_sam = nullptr;
    s.runs_sent = 0;
    s.pushed = s.launched = false;
    s.ref_pending = false;
    // Everything below only enqueues work on the slot's stream. Should an enqueue fail half-way, the copies already queued
    // still reference the caller's buffers: the stream is drained before the error is returned, so that a failed submit
    // never leaves the slot (or the caller's memory) in flight.
    auto enqueue = [&]() -> int {
        HIP_TRY(hipEventRecord(s.ev[0], s.stream));
        if (n) {
            HIP_TRY(hipMemcpyAsync(s.d_req, io->requests, (size_t)n * req_size(p), hipMemcpyHostToDevice, s.stream));
            if (ref) HIP_TRY(hipMemcpyAsync(s.d_tpos, text_pos, (size_t)n * 8, hipMemcpyHostToDevice, s.stream));
            if (packed) {
                HIP_TRY(hipMemcpyAsync(s.d_packP, io->packed_patterns, (size_t)n * rowb, hipMemcpyHostToDevice, s.stream));
                if (!ref) HIP_TRY(hipMemcpyAsync(s.d_packT, io->packed_texts, (size_t)n * rowb, hipMemcpyHostToDevice, s.stream));
                if (io->n_raw) {
                    HIP_TRY(hipMemcpyAsync(s.d_rawidx, io->raw_pairs, (size_t)io->n_raw * 4, hipMemcpyHostToDevice, s.stream));
                    HIP_TRY(hipMemcpyAsync(s.d_rawP, io->raw_patterns, (size_t)io->n_raw * rs, hipMemcpyHostToDevice, s.stream));
                    if (!ref) HIP_TRY(hipMemcpyAsync(s.d_rawT, io->raw_texts, (size_t)io->n_raw * rs, hipMemcpyHostToDevice, s.stream));
                }
            } else {
                HIP_TRY(hipMemcpyAsync(s.d_pat, io->patterns, (size_t)n * rs, hipMemcpyHostToDevice, s.stream));
                if (!ref) HIP_TRY(hipMemcpyAsync(s.d_txt, io->texts, (size_t)n * rs, hipMemcpyHostToDevice, s.stream));
            }
        }
        HIP_TRY(hipEventRecord(s.ev[1], s.stream));
        HIP_TRY(hipEventRecord(s.ev[2], s.stream));
        if (n) {
            aim::KArgs ka;
            memset(&ka, 0, sizeof ka);
            ka.p = p;
            ka.n_pairs = n;
            ka.req = static_cast<const aim_request_t *>(s.d_req);
            ka.res = static_cast<aim_result_t *>(s.d_res);
            ka.ops = s.d_ops;
            // Does the alignment kernel of this configuration take the batch as it arrived and deliver what was asked for?
            // (wfa_lane_packed_kernel: packed rows in, {idx, score} or compact CIGAR out.) Then this batch is ONE kernel;
            // otherwise the conversion kernels of batch_io.hpp run around the default-ABI kernel.
            uint32_t mode = (packed ? MODE_PACKED_IN : 0u) | ((io->cigars && !io->results && !io->ops && !sio) ? MODE_RUNS_OUT : 0u);   // (the SAM kernel reads ops rows)
            Plan pl = plan_for_batch(set, d, s, n, mode);
            // AIM_FLAG_REF_TEXTS: a packed batch keeps the fused packed lane kernel (its texts gathered as packed rows, the windows
            // holding a byte outside A/C/G/T re-aligned by the general kernel over a to-do list); every other plan runs as for an
            // ASCII batch after the gather
            Stage ref_fb;
            const bool ref_fused = ref && packed && pl.pk && pl.main.kid == K_WFA_LANE_PK && !pl.pack_first && s.d_reftodo && !pl.esc_c &&
                                   ref_todo_stage(set, d, s.scratch_bytes, n, &ref_fb);
            if (ref && packed && !ref_fused && pl.pk) {
                mode &= ~MODE_PACKED_IN;
                pl = plan_for_batch(set, d, s, n, mode);
            }
            const uint32_t runs_cap = std::min(io->runs_cap, set->max_runs);
            if (packed && !pl.pk) {   // expand into the reference's char[n][READ_SIZE] layout (batch_io.hpp), then run as usual
                const uint64_t threads = (uint64_t)n * (rs / 8);
                const unsigned rows = ref ? 1u : 2u;   // (grid.y 0: patterns; the texts of a reference batch are gathered below)
                hipLaunchKernelGGL(aim::unpack_rows_kernel, dim3((unsigned)((threads + 255) / 256), rows), dim3(256), 0, s.stream, ka, s.d_packP,
                                   s.d_packT, s.d_pat, s.d_txt);
                if (io->n_raw) {
                    const uint64_t rt = (uint64_t)io->n_raw * (rs / 8);
                    hipLaunchKernelGGL(aim::scatter_raw_rows_kernel, dim3((unsigned)((rt + 255) / 256), rows), dim3(256), 0, s.stream, p.read_size,
                                       io->n_raw, s.d_rawidx, s.d_rawP, s.d_rawT, s.d_pat, s.d_txt);
                }
                HIP_TRY(hipGetLastError());
            }
            uint32_t *ref_todo = s.d_reftodo;
            if (ref_fused) {
                // packed text rows + to-do list; the side list's (non-ACGT patterns) text rows as ASCII for the raw side pass
                uint32_t *flag_bits = ref_todo + 16 + set->max_pairs;
                HIP_TRY(hipMemsetAsync(ref_todo, 0, 64, s.stream));
                HIP_TRY(hipMemsetAsync(flag_bits, 0, ((size_t)n + 31) / 32 * 4, s.stream));
                const uint64_t threads = (uint64_t)n * aim::packed_row_dwords(p.read_size);
                hipLaunchKernelGGL(aim::gather_text_packed_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, s.stream, ka, s.d_tpos,
                                   d.d_ref, d.ref_len, s.d_packT, flag_bits, ref_todo);
                HIP_TRY(hipGetLastError());
                rc = enqueue_gather(ka, s.d_tpos, d.d_ref, d.ref_len, s.d_rawidx, io->n_raw, s.d_rawT, s.stream);
                if (rc) return rc;
            } else if (ref) {
                rc = enqueue_gather(ka, s.d_tpos, d.d_ref, d.ref_len, nullptr, n, s.d_txt, s.stream);
                if (rc) return rc;
            }
            FusedIo fio;
            if (pl.pk) { fio.packedP = s.d_packP; fio.packedT = s.d_packT; }
            if (pl.emits_runs) { fio.cig = s.d_cig; fio.runs = s.d_runs; fio.cursor = s.d_cursor; fio.runs_cap = runs_cap; }
            rc = launch_on_slot(set, d, s, mode, &fio);
            if (rc) return rc;
            if (ref_fused) {
                // the to-do windows: ASCII rows (pattern unpacked, text gathered), the general kernel over them, their compact CIGAR
                hipLaunchKernelGGL(aim::gather_todo_rows_kernel, dim3(256), dim3(256), 0, s.stream, ka, ref_todo, s.d_tpos, d.d_ref, d.ref_len,
                                   s.d_packP, s.d_pat, s.d_txt);
                HIP_TRY(hipGetLastError());
                aim::KArgs kb = stage_args(ka, ref_fb, s.d_scratch);
                kb.patterns = s.d_pat;
                kb.texts = s.d_txt;
                kb.todo = ref_todo;
                launch_stage(p, ref_fb, kb, s.stream);
                HIP_TRY(hipGetLastError());
                if (pl.emits_runs) {
                    hipLaunchKernelGGL(aim::cigar_rle_todo_kernel, dim3(256), dim3(64), 0, s.stream, kb, ref_todo, s.d_cig, s.d_runs, runs_cap, s.d_cursor);
                    HIP_TRY(hipGetLastError());
                }
            }
            s.runs_sent = pl.emits_runs ? n * fio.run_slot : 0u;   // 0 when the run buffer is bump-allocated: nothing is known before the kernel ran
            if (io->cigars && !pl.emits_runs) {
                HIP_TRY(hipMemsetAsync(s.d_cursor, 0, 4, s.stream));
                hipLaunchKernelGGL(aim::cigar_rle_kernel, dim3((n + 63) / 64), dim3(64), 0, s.stream, ka, s.d_cig, s.d_runs, runs_cap, s.d_cursor);
                HIP_TRY(hipGetLastError());
            }
            if (pl.pk && io->n_raw) {
                // Raw side pass: the pairs of the side list hold a byte outside A/C/G/T (the reference compares raw bytes,
                // host.c:126-127); what the packed kernel computed for them is void. They are aligned as a batch of their own by
                // the ASCII kernels -- requests gathered, the side list's rows are its patterns / texts -- and their results
                // replace the void ones (with the compact CIGAR: their runs are appended to the run buffer).
                const uint32_t nr = io->n_raw;
                const uint32_t rq_dw = (uint32_t)req_size(p) / 4, rs_dw = (uint32_t)res_size(p) / 4;
                auto blocks = [](uint64_t t) { return dim3((unsigned)((t + 255) / 256)); };
                hipLaunchKernelGGL(aim::gather_elems_kernel, blocks((uint64_t)nr * rq_dw), dim3(256), 0, s.stream, (const uint32_t *)s.d_req,
                                   s.d_rawidx, nr, rq_dw, (uint32_t *)s.d_rawreq);
                HIP_TRY(hipGetLastError());
                const Plan rp = plan_for_batch(set, d, s, nr, 0u);
                rc = launch(rp, set->knobs, p, nr, s.d_rawreq, s.d_rawP, s.d_rawT, s.d_rawres, s.d_rawops, s.d_scratch, s.scratch_bytes, s.stream, nullptr, &s.aux);
                if (rc) return rc;
                // (both outputs may be asked for at once -- aim_cigar_t + runs AND result_t [+ ops rows]: each gets its own scatter)
                if (io->cigars) {
                    aim::KArgs kr = ka;
                    kr.n_pairs = nr;
                    kr.res = static_cast<aim_result_t *>(s.d_rawres);
                    kr.ops = s.d_rawops;
                    hipLaunchKernelGGL(aim::cigar_rle_kernel, dim3((nr + 63) / 64), dim3(64), 0, s.stream, kr, s.d_rawcig, s.d_runs, runs_cap, s.d_cursor);
                    hipLaunchKernelGGL(aim::scatter_elems_kernel, blocks((uint64_t)nr * 4), dim3(256), 0, s.stream, (const uint32_t *)s.d_rawcig,
                                       s.d_rawidx, nr, 4u, (uint32_t *)s.d_cig);
                }
                if (!io->cigars || io->results || io->ops || sio) {
                    hipLaunchKernelGGL(aim::scatter_elems_kernel, blocks((uint64_t)nr * rs_dw), dim3(256), 0, s.stream, (const uint32_t *)s.d_rawres,
                                       s.d_rawidx, nr, rs_dw, (uint32_t *)s.d_res);
                    if (bt) {   // default output (result_t + ops rows): the side list's ops rows go home too
                        const uint32_t op_dw = (uint32_t)(2 * rs / 4);
                        hipLaunchKernelGGL(aim::scatter_elems_kernel, blocks((uint64_t)nr * op_dw), dim3(256), 0, s.stream, (const uint32_t *)s.d_rawops,
                                           s.d_rawidx, nr, op_dw, (uint32_t *)s.d_ops);
                    }
                }
                HIP_TRY(hipGetLastError());
            }
            if (sio) {   // the records of the final rows (the raw side pass's rows are home)
                rc = enqueue_sam_on_slot(set, d, s, sio, n, nullptr);
                if (rc) return rc;
            }
        }
        HIP_TRY(hipEventRecord(s.ev[3], s.stream));
        HIP_TRY(hipEventRecord(s.ev[4], s.stream));
        if (n) {
            if (sio) {
                rc = enqueue_sam_d2h(s, n);
                if (rc) return rc;
            }
            if (io->cigars) {
                HIP_TRY(hipMemcpyAsync(s.h_cursor, s.d_cursor, 4, hipMemcpyDeviceToHost, s.stream));
                HIP_TRY(hipMemcpyAsync(io->cigars, s.d_cig, (size_t)n * sizeof(aim_cigar_t), hipMemcpyDeviceToHost, s.stream));
                // slotted run buffer (wfa_lane_packed.hpp): the first 3 n runs are the pairs' own slots, known now -- their copy
                // overlaps the next batch instead of waiting in aim_set_wait for the cursor; only runs behind the slots follow there
                if (s.runs_sent) HIP_TRY(hipMemcpyAsync(io->runs, s.d_runs, (size_t)s.runs_sent * 4, hipMemcpyDeviceToHost, s.stream));
            }
            if (io->results) HIP_TRY(hipMemcpyAsync(io->results, s.d_res, (size_t)n * res_size(p), hipMemcpyDeviceToHost, s.stream));
            if (io->ops) HIP_TRY(hipMemcpyAsync(io->ops, s.d_ops, (size_t)n * 2 * rs, hipMemcpyDeviceToHost, s.stream));
        }
        HIP_TRY(hipEventRecord(s.ev[5], s.stream));
        return AIM_OK;
    };
    rc = enqueue();
    if (rc) {
        char keep[sizeof g_err];
        memcpy(keep, g_err, sizeof keep);
        (void)hipStreamSynchronize(s.stream);
        (void)hipGetLastError();
        memcpy(g_err, keep, sizeof keep);
        return rc;
    }
    s.submitted = true;
    return AIM_OK;
}

int aim_set_wait(aim_set_t *set, uint32_t device, uint32_t slot, uint32_t *n_runs)
{
    if (!set || device >= set->devs.size()) return fail(AIM_EINVAL, "bad arguments");
    if (!set->configured) return fail(AIM_ESTATE, "aim_set_configure has not been called");
    aim_device_ctx &d = set->devs[device];
    if (slot >= d.slots.size()) return fail(AIM_EINVAL, "slot %u not configured", slot);
    aim_slot &s = d.slots[slot];
    if (!s.submitted) return fail(AIM_ESTATE, "slot %u of device %d holds no batch", slot, d.dev);
    HIP_TRY(hipSetDevice(d.dev));
    if (getenv("AIM_WAIT_POLL")) {   // A/B (host lanes sharing a device): poll the stream instead of blocking inside the runtime
        hipError_t q;
        while ((q = hipStreamQuery(s.stream)) == hipErrorNotReady) std::this_thread::sleep_for(std::chrono::microseconds(50));
        if (q != hipSuccess) return fail(AIM_ENODEV, "hipStreamQuery failed: %s", hipGetErrorString(q));
    } else
    HIP_TRY(hipStreamSynchronize(s.stream));
    s.submitted = false;
    const aim_batch_io_t &io = s.io;
    uint32_t runs = 0;
    if (io.cigars && s.n_pairs) {   // the run count is only known now: fetch exactly that many
        runs = std::min(std::min(*s.h_cursor, io.runs_cap), set->max_runs);
        if (runs > s.runs_sent) {
            HIP_TRY(hipMemcpyAsync(io.runs + s.runs_sent, s.d_runs + s.runs_sent, (size_t)(runs - s.runs_sent) * 4, hipMemcpyDeviceToHost, s.stream));
            HIP_TRY(hipStreamSynchronize(s.stream));
        }
        s.runs_sent = 0;
    }
    if (n_runs) *n_runs = runs;
    const aim_sam_t *sam_rows = s.io_sam;
    if (sam_rows && s.n_pairs) {   // AIM_FLAG_SAM_FIELDS: exactly the words and bytes that were written (rows that did not fit reserved theirs too)
        const uint32_t words = std::min(s.h_samcur[0], s.io_samcig_cap), bytes = std::min(s.h_samcur[1], s.io_sammd_cap);
        if (words) HIP_TRY(hipMemcpyAsync(s.io_samcig, s.d_samcig, (size_t)words * 4, hipMemcpyDeviceToHost, s.stream));
        if (bytes) HIP_TRY(hipMemcpyAsync(s.io_sammd, s.d_sammd, bytes, hipMemcpyDeviceToHost, s.stream));
        if (words || bytes) HIP_TRY(hipStreamSynchronize(s.stream));
    }
    s.io_sam = nullptr;
    // per DEVICE (devices run concurrently: aim_set_timers reports the slowest device, like aim_set_launch does)
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, s.ev[0], s.ev[1]));
    d.h2d_ms += ms;
    HIP_TRY(hipEventElapsedTime(&ms, s.ev[2], s.ev[3]));
    d.kernel_ms += ms;
    HIP_TRY(hipEventElapsedTime(&ms, s.ev[4], s.ev[5]));
    d.d2h_ms += ms;
    // Every pair's status (the reference stops at the first DPU fault). 4 M compact CIGARs are 64 MB: one thread scanning them took as
    // long as the batch's transfers (the e2e rate with CIGAR was bound by THIS loop, not by PCIe), so the scan is an OR over a few
    // threads and only a batch that holds a fault is walked to name it.
    if (io.cigars) {
        const aim_cigar_t *cg = io.cigars;
        if (any_nonzero(s.n_pairs, [cg](size_t i) { return (uint32_t)cg[i].status; }))
            for (uint32_t i = 0; i < s.n_pairs; ++i) {
                if (io.cigars[i].status & AIM_CIGAR_OVERFLOW) return fail(AIM_ENOMEM, "run buffer too small (pair idx %u)", io.cigars[i].idx);
                if (io.cigars[i].status != AIM_PAIR_OK) return status_error(io.cigars[i].idx, io.cigars[i].status);
            }
    } else if (io.results && !(set->params.flags & AIM_FLAG_RES8)) {
        const aim_result_t *r = static_cast<const aim_result_t *>(io.results);
        if (any_nonzero(s.n_pairs, [r](size_t i) { return (uint32_t)r[i].status; }))
            for (uint32_t i = 0; i < s.n_pairs; ++i)
                if (r[i].status != AIM_PAIR_OK) return status_error(r[i].idx, r[i].status);
    } else if (sam_rows) {   // the records are the batch's only per-row output
        if (any_nonzero(s.n_pairs, [sam_rows](size_t i) { return (uint32_t)(sam_rows[i].status & 0xffu); }))
            for (uint32_t i = 0; i < s.n_pairs; ++i)
                if ((sam_rows[i].status & 0xffu) != AIM_PAIR_OK) return status_error(sam_rows[i].idx, sam_rows[i].status & 0xffu);
    }
    return AIM_OK;
}

int aim_set_sam_capacity(aim_set_t *set, uint32_t max_cigar_words, uint32_t max_md_bytes)
{
    if (!set) return fail(AIM_EINVAL, "set is NULL");
    if (!set->configured) return fail(AIM_ESTATE, "aim_set_configure_slots has not been called");
    if (!is_sam(set->params)) return fail(AIM_EINVAL, "aim_set_sam_capacity needs a set configured with AIM_FLAG_SAM_FIELDS");
    if (!max_cigar_words || !max_md_bytes) return fail(AIM_EINVAL, "aim_set_sam_capacity: capacities must be > 0");
    for (auto &d : set->devs) {
        HIP_TRY(hipSetDevice(d.dev));
        for (auto &s : d.slots) {
            if (s.submitted) return fail(AIM_ESTATE, "a slot of device %d holds a batch: aim_set_wait it first", d.dev);
            void *old[] = {s.d_sam, s.d_samcig, s.d_sammd, s.d_samcur};
            for (void *b : old)
                if (b) (void)hipFree(b);
            s.d_sam = nullptr; s.d_samcig = nullptr; s.d_sammd = nullptr; s.d_samcur = nullptr;
            s.samcig_cap = s.sammd_cap = 0;
            HIP_TRY(hipMalloc((void **)&s.d_samcig, (size_t)max_cigar_words * 4));
            HIP_TRY(hipMalloc((void **)&s.d_sammd, (size_t)max_md_bytes));
            HIP_TRY(hipMalloc((void **)&s.d_samcur, 64));
            if (!s.h_samcur) HIP_TRY(hipHostMalloc((void **)&s.h_samcur, 64, hipHostMallocDefault));
            HIP_TRY(hipMalloc((void **)&s.d_sam, (size_t)set->max_pairs * sizeof(aim_sam_t)));   // last: a slot with d_sam is complete
            s.samcig_cap = max_cigar_words;
            s.sammd_cap = max_md_bytes;
        }
    }
    return AIM_OK;
}

int aim_set_timers(const aim_set_t *set, float *h2d_ms, float *kernel_ms, float *d2h_ms)
{
    if (!set) return fail(AIM_EINVAL, "set is NULL");
    float dh = 0.f, dk = 0.f, dd = 0.f;   // submit / wait path: the slowest device
    for (const auto &d : set->devs) { dh = std::max(dh, d.h2d_ms); dk = std::max(dk, d.kernel_ms); dd = std::max(dd, d.d2h_ms); }
    if (h2d_ms) *h2d_ms = set->h2d_ms + dh;
    if (kernel_ms) *kernel_ms = set->kernel_ms + dk;
    if (d2h_ms) *d2h_ms = set->d2h_ms + dd;
    return AIM_OK;
}

int aim_set_fallback_pairs(aim_set_t *set, uint32_t device, uint32_t *n_fallback)
{
    if (!set || device >= set->devs.size() || !n_fallback) return fail(AIM_EINVAL, "bad arguments");
    if (!set->configured) return fail(AIM_ESTATE, "aim_set_configure has not been called");
    aim_device_ctx &d = set->devs[device];
    aim_slot &s = d.slots[0];
    if (!s.launched) return fail(AIM_ESTATE, "device %d has not been launched", d.dev);
    *n_fallback = 0;
    const Plan &pl = s.plan_last;   // the plan the launch actually followed, not a re-plan
    if (!pl.todo_bytes || s.n_pairs == 0) return AIM_OK;   // no to-do list: the kernel aligns every pair itself
    HIP_TRY(hipSetDevice(d.dev));
    HIP_TRY(hipMemcpy(n_fallback, static_cast<const char *>(s.d_scratch) + pl.todo_at, sizeof(uint32_t), hipMemcpyDeviceToHost));   // the to-do count
    return AIM_OK;
}

int aim_set_plan_describe(const aim_set_t *set, uint32_t device, char *out, size_t cap)
{
    if (!set || device >= set->devs.size() || !out || cap == 0) return fail(AIM_EINVAL, "bad arguments");
    if (!set->configured) return fail(AIM_ESTATE, "aim_set_configure has not been called");
    const aim_device_ctx &d = set->devs[device];
    const aim_slot &s = d.slots[0];
    if (is_groups(set->params)) {   // the last groups batch submitted on slot 0 (before the first: the configure-time plans)
        GroupsPlan g;
        memset(&g, 0, sizeof g);
        g.x1 = groups_pass_params(set->params, AIM_FLAG_BACKTRACE | AIM_FLAG_WFA_BIDIR | AIM_FLAG_RES8);
        g.x2 = groups_pass_params(set->params, 0u);
        g.pass2 = (set->params.flags & AIM_FLAG_BACKTRACE) != 0;
        g.mates = is_mates(set->params);
        g.sam = is_sam(set->params);
        g.hits = is_hits(set->params);
        g.p1 = s.plan_last;
        g.p2 = s.plan_last2;
        const bool any = s.n_reads != 0;
        describe_groups(g, any ? s.io.n_pairs : set->max_pairs, any ? s.n_pairs : set->max_pairs, d.budget, out, cap);   // (n_pairs: the output rows)
        return AIM_OK;
    }
    describe_plan(s.plan_last, set->params, s.launched ? s.n_pairs : set->max_pairs, d.budget, out, cap);
    return AIM_OK;
}

int aim_set_free(aim_set_t *set)
{
    if (!set) return AIM_OK;
    for (auto &d : set->devs) {
        free_device_buffers(d);
        if (d.d_ref) {
            (void)hipSetDevice(d.dev);
            (void)hipFree(d.d_ref);
            d.d_ref = nullptr;
        }
    }
    delete set;
    return AIM_OK;
}

int aim_set_reference(aim_set_t *set, const char *seq, uint64_t len)
{
    if (!set || (len && !seq)) return fail(AIM_EINVAL, "bad arguments");
    if (len > (1ull << 62)) return fail(AIM_EINVAL, "reference length %llu does not fit text_pos", (unsigned long long)len);
    // every device's copy first; the old references are released only once all of them exist (AIM_ENOMEM keeps the old one)
    std::vector<char *> fresh(set->devs.size(), nullptr);
    auto drop = [&]() {
        for (size_t i = 0; i < fresh.size(); ++i)
            if (fresh[i]) { (void)hipSetDevice(set->devs[i].dev); (void)hipFree(fresh[i]); }
    };
    const size_t slack = 64;   // zeroed; the gather reads at most aim::kRefSlack bytes past the end
    for (size_t i = 0; i < set->devs.size(); ++i) {
        hipError_t e = hipSetDevice(set->devs[i].dev);
        if (e == hipSuccess) e = hipMalloc((void **)&fresh[i], (size_t)len + slack);
        if (e == hipSuccess) e = hipMemset(fresh[i] + len, 0, slack);
        if (e == hipSuccess && len) e = hipMemcpy(fresh[i], seq, (size_t)len, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            if (e == hipErrorOutOfMemory) fresh[i] = nullptr;
            drop();
            return fail(e == hipErrorOutOfMemory ? AIM_ENOMEM : AIM_ENODEV, "reference of %llu bytes on device %d: %s (the previous reference stays)",
                        (unsigned long long)len, set->devs[i].dev, hipGetErrorString(e));
        }
    }
    for (size_t i = 0; i < set->devs.size(); ++i) {
        aim_device_ctx &d = set->devs[i];
        HIP_TRY(hipSetDevice(d.dev));
        if (d.d_ref) {
            for (auto &s : d.slots) HIP_TRY(hipStreamSynchronize(s.stream));   // batches in flight still read the old reference
            HIP_TRY(hipFree(d.d_ref));
        }
        d.d_ref = fresh[i];
        d.ref_len = len;
        fresh[i] = nullptr;
    }
    return AIM_OK;
}

int aim_host_alloc(void **ptr, size_t bytes)
{
    if (!ptr) return fail(AIM_EINVAL, "ptr is NULL");
    HIP_TRY(hipHostMalloc(ptr, bytes ? bytes : 1, hipHostMallocDefault));
    return AIM_OK;
}

int aim_host_free(void *ptr)
{
    if (ptr) HIP_TRY(hipHostFree(ptr));
    return AIM_OK;
}


int aim_align_device_ref(const aim_params_t *params, uint32_t n_pairs, const void *d_requests, const char *d_patterns,
                         const uint64_t *d_text_pos, const char *d_reference, uint64_t ref_len, void *d_results, char *d_ops,
                         void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
    if (!params) return fail(AIM_EINVAL, "params is NULL");
    if (is_sam(*params)) return fail(AIM_EINVAL, kSamStateless);
    if (!is_ref(*params)) return fail(AIM_EINVAL, "aim_align_device_ref needs AIM_FLAG_REF_TEXTS");
    if (is_groups(*params)) return fail(AIM_EINVAL, "AIM_FLAG_READ_GROUPS is set: use aim_align_device_groups");
    if (is_mates(*params)) return fail(AIM_EINVAL, "AIM_FLAG_MATE_PAIRS is set: use aim_align_device_mates");
    if (n_pairs && (!d_text_pos || !d_reference || !d_requests)) return fail(AIM_EINVAL, "null device buffer");
    int n = 0;
    int rc = aim_device_count(&n);
    if (rc) return rc;
    const aim::Knobs kn = read_knobs();
    Plan pl;
    rc = make_plan(*params, n_pairs, kn, stateless_budget_bytes(kn), &pl);
    if (rc) return rc;
    const size_t at = ref_rows_at(pl.scratch_total), need = at + ref_rows_bytes(*params, n_pairs);
    if (!d_scratch || scratch_bytes < need) return fail(AIM_EINVAL, "scratch too small: need %zu bytes, got %zu", need, scratch_bytes);
    if (n_pairs == 0) return AIM_OK;
    char *rows = static_cast<char *>(d_scratch) + at;
    aim::KArgs ka;
    memset(&ka, 0, sizeof ka);
    ka.p = *params;
    ka.n_pairs = n_pairs;
    ka.req = static_cast<const aim_request_t *>(d_requests);
    rc = enqueue_gather(ka, d_text_pos, d_reference, ref_len, nullptr, n_pairs, rows, (hipStream_t)hip_stream);
    if (rc) return rc;
    return launch(pl, kn, *params, n_pairs, d_requests, d_patterns, rows, d_results, d_ops, d_scratch, at, (hipStream_t)hip_stream);
}

int aim_ref_windows_check(const aim_params_t *params, uint32_t n_pairs, const void *requests, const uint64_t *text_pos, uint64_t ref_len,
                          uint32_t *bad_pair)
{
    if (!params || (n_pairs && (!requests || !text_pos))) return fail(AIM_EINVAL, "bad arguments");
    int rc = check_lengths(*params, n_pairs, requests);
    if (rc) {
        if (bad_pair)   // name the pair check_lengths refused
            for (uint32_t i = 0; i < n_pairs; ++i) {
                const bool r8 = params->flags & AIM_FLAG_REQ8;
                const int tl = r8 ? static_cast<const aim_request8_t *>(requests)[i].text_len : static_cast<const aim_request_t *>(requests)[i].text_len;
                const int pl = r8 ? static_cast<const aim_request8_t *>(requests)[i].pattern_len : static_cast<const aim_request_t *>(requests)[i].pattern_len;
                if (pl < 0 || tl < 0 || pl > params->read_size || tl > params->read_size) { *bad_pair = i; break; }
            }
        return rc;
    }
    return check_windows(*params, n_pairs, requests, text_pos, ref_len, bad_pair);
}

int aim_align_device(const aim_params_t *params, uint32_t n_pairs, const void *d_requests,
                     const char *d_patterns, const char *d_texts, void *d_results, char *d_ops,
                     void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
    if (!params) return fail(AIM_EINVAL, "params is NULL");
    if (is_sam(*params)) return fail(AIM_EINVAL, kSamStateless);
    if (is_groups(*params)) return fail(AIM_EINVAL, "AIM_FLAG_READ_GROUPS is set: use aim_align_device_groups");
    if (is_mates(*params)) return fail(AIM_EINVAL, "AIM_FLAG_MATE_PAIRS is set: use aim_align_device_mates");
    int n = 0;
    int rc = aim_device_count(&n);
    if (rc) return rc;
    const aim::Knobs kn = read_knobs();
    Plan pl;
    rc = make_plan(*params, n_pairs, kn, stateless_budget_bytes(kn), &pl);
    if (rc) return rc;
    return launch(pl, kn, *params, n_pairs, d_requests, d_patterns, d_texts, d_results, d_ops, d_scratch, scratch_bytes,
                  (hipStream_t)hip_stream);
}

// aim_sam_device (split = false) and aim_sam_device_split under the name fn: the same checks in the same order, then one launch.
static int sam_device_entry(const char *fn, bool split, const aim_params_t *params, uint32_t n_rows, const void *d_requests, const uint64_t *d_text_pos,
                            const uint32_t *d_sel_or_null, const void *d_results, const char *d_ops, const char *d_reference, uint64_t ref_len,
                            uint32_t options, aim_sam_t *d_sam, uint32_t *d_cigar, uint32_t cigar_cap, char *d_md, uint32_t md_cap,
                            uint32_t *d_cursors, const aim_segment_t *d_seg, void *hip_stream)
{
    if (!params) return fail(AIM_EINVAL, "params is NULL");
    if (params->algo == AIM_ALGO_GENASM)
        return fail(AIM_EINVAL, "%s cannot take AIM_ALGO_GENASM rows (its windowed walk is unpinned and begin_offset = 0 is another contract)", fn);
    if (!(params->flags & AIM_FLAG_BACKTRACE)) return fail(AIM_EINVAL, "%s needs AIM_FLAG_BACKTRACE (the records come from the ops rows)", fn);
    if (params->flags & AIM_FLAG_RES8) return fail(AIM_EINVAL, "%s cannot be combined with AIM_FLAG_RES8", fn);
    if (params->read_size <= 0 || (params->read_size & 7)) return fail(AIM_EINVAL, "read_size must be a positive multiple of 8 (got %d)", params->read_size);
    if (options & ~AIM_SAM_EQX) return fail(AIM_EINVAL, "%s: unknown options 0x%x", fn, options);
    int rc = check_sam_rows(*params, n_rows);
    if (rc) return rc;
    if (!d_cursors) return fail(AIM_EINVAL, "null device buffer");
    if (n_rows && (!d_requests || !d_text_pos || !d_results || !d_ops || !d_reference || !d_sam || !d_cigar || !d_md || (split && !d_seg)))
        return fail(AIM_EINVAL, "null device buffer");
    int n = 0;
    rc = aim_device_count(&n);
    if (rc) return rc;
    aim::SamArgs a;
    memset(&a, 0, sizeof a);
    a.n_rows = n_rows;
    a.text_pos = d_text_pos;
    a.sel = d_sel_or_null;
    a.res = static_cast<const aim_result_t *>(d_results);
    a.ops = d_ops;
    a.ref = d_reference;
    a.ref_len = ref_len;
    a.options = options;
    a.sam = d_sam;
    a.cigar = d_cigar;
    a.cigar_cap = cigar_cap;
    a.md = d_md;
    a.md_cap = md_cap;
    a.cursors = d_cursors;
    if (!n_rows) {
        HIP_TRY(hipMemsetAsync(d_cursors, 0, 8, (hipStream_t)hip_stream));
        return AIM_OK;
    }
    return enqueue_sam(*params, read_knobs(), a, (hipStream_t)hip_stream, split ? d_seg : nullptr);
}

int aim_sam_device(const aim_params_t *params, uint32_t n_rows, const void *d_requests, const uint64_t *d_text_pos,
                   const uint32_t *d_sel_or_null, const void *d_results, const char *d_ops, const char *d_reference, uint64_t ref_len,
                   uint32_t options, aim_sam_t *d_sam, uint32_t *d_cigar, uint32_t cigar_cap, char *d_md, uint32_t md_cap,
                   uint32_t *d_cursors, void *hip_stream)
{
    return sam_device_entry("aim_sam_device", false, params, n_rows, d_requests, d_text_pos, d_sel_or_null, d_results, d_ops, d_reference, ref_len, options, d_sam,
                            d_cigar, cigar_cap, d_md, md_cap, d_cursors, nullptr, hip_stream);
}

int aim_sam_device_split(const aim_params_t *params, uint32_t n_rows, const void *d_requests, const uint64_t *d_text_pos,
                         const uint32_t *d_sel_or_null, const void *d_results, const char *d_ops, const char *d_reference, uint64_t ref_len,
                         uint32_t options, aim_sam_t *d_sam, uint32_t *d_cigar, uint32_t cigar_cap, char *d_md, uint32_t md_cap,
                         uint32_t *d_cursors, const aim_segment_t *d_seg, void *hip_stream)
{
    return sam_device_entry("aim_sam_device_split", true, params, n_rows, d_requests, d_text_pos, d_sel_or_null, d_results, d_ops, d_reference, ref_len, options,
                            d_sam, d_cigar, cigar_cap, d_md, md_cap, d_cursors, d_seg, hip_stream);
}

const char *aim_sam_kernel_name(const aim_params_t *params)
{
    if (!params) return "";
    return sam_use_wave(*params, read_knobs()) ? "sam_wave_kernel" : "sam_lane_kernel";
}


int aim_groups_check(uint32_t n_pairs, uint32_t n_reads, const uint32_t *read_offsets, uint32_t *bad_read)
{
    return check_groups(n_pairs, n_reads, read_offsets, bad_read);
}

int aim_mates_check(uint32_t n_reads, int64_t min_span, int64_t max_span, int32_t unpaired_penalty)
{
    return check_mates(n_reads, min_span, max_span, unpaired_penalty);
}

namespace {
// AIM_FLAG_TOP_HITS: the hit rows of a stateless call
struct HitArgs {
    uint32_t max_hits, n_hits;
    const uint32_t *hoff;
    uint32_t *hit_pair;      // or nullptr: the hit list lives in the scratch
};

// aim_align_device_groups (mate == nullptr, hit == nullptr), aim_align_device_mates and aim_align_device_hits
int align_device_groups(const aim_params_t *params, uint32_t n_pairs, uint32_t n_reads, const void *d_requests, const char *d_patterns,
                        const char *d_texts_or_null, const uint64_t *d_text_pos_or_null, const char *d_reference, uint64_t ref_len,
                        const uint32_t *d_read_offsets, void *d_results, char *d_ops, aim_best_t *d_best, const aim::MateArgs *mate,
                        aim_mate_t *d_mates, const HitArgs *hit, void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
    const bool ref = is_ref(*params), bt = params->flags & AIM_FLAG_BACKTRACE;
    if (is_sam(*params)) return fail(AIM_EINVAL, kSamStateless);
    if (n_reads > n_pairs || (n_pairs && !n_reads)) return fail(AIM_EINVAL, "n_reads %u does not fit n_pairs %u", n_reads, n_pairs);
    if (n_pairs && (!d_requests || !d_patterns || !d_read_offsets || !d_results || (bt && !d_ops) ||
                    (ref ? (!d_text_pos_or_null || !d_reference) : !d_texts_or_null)))
        return fail(AIM_EINVAL, "null device buffer");
    int n = 0;
    int rc = aim_device_count(&n);
    if (rc) return rc;
    const aim::Knobs kn = read_knobs();
    const uint64_t budget = stateless_budget_bytes(kn);
    GroupsPlan g;
    rc = make_groups_plan(*params, n_pairs, kn, budget, &g);
    if (rc) return rc;
    if (!d_scratch || scratch_bytes < g.total) return fail(AIM_EINVAL, "scratch too small: need %zu bytes, got %zu", g.total, scratch_bytes);
    if (n_pairs == 0) return AIM_OK;
    char *base = static_cast<char *>(d_scratch);
    const hipStream_t stream = (hipStream_t)hip_stream;
    GroupsIo gi;
    gi.n_pairs = n_pairs;
    gi.n_reads = n_reads;
    gi.req = d_requests;
    gi.read_rows = d_patterns;
    gi.packed = nullptr;
    gi.raw_pairs = nullptr;
    gi.raw_rows = nullptr;
    gi.n_raw = 0;
    gi.raw_slot = nullptr;
    gi.roff = d_read_offsets;
    gi.cand_p = base + g.cand_p_at;
    gi.cand_t = ref ? base + g.cand_t_at : const_cast<char *>(d_texts_or_null);
    gi.res1 = reinterpret_cast<aim_result_t *>(base + g.res1_at);
    gi.map = reinterpret_cast<uint32_t *>(base + g.map_at);
    gi.sel = reinterpret_cast<uint32_t *>(base + g.sel_at);
    gi.best = d_best ? d_best : (mate ? reinterpret_cast<aim_best_t *>(base + g.best_at) : nullptr);
    gi.tpos = d_text_pos_or_null;
    memset(&gi.mate, 0, sizeof gi.mate);
    if (mate) gi.mate = *mate;
    gi.mates = d_mates;
    gi.n_hits = hit ? hit->n_hits : 0u;
    gi.max_hits = hit ? hit->max_hits : 0u;
    gi.hoff = hit ? hit->hoff : nullptr;
    gi.hit_pair = !hit ? nullptr : hit->hit_pair ? hit->hit_pair : reinterpret_cast<uint32_t *>(base + g.hit_at);
    gi.req2 = bt ? base + g.req2_at : nullptr;
    gi.pat2 = bt ? base + g.pat2_at : nullptr;
    gi.txt2 = bt ? base + g.txt2_at : nullptr;
    gi.res = d_results;
    gi.ops = d_ops;
    gi.scratch = d_scratch;
    gi.scratch_bytes = g.plan_bytes;
    if (ref) {
        aim::KArgs ka;
        memset(&ka, 0, sizeof ka);
        ka.p = *params;
        ka.n_pairs = n_pairs;
        ka.req = static_cast<const aim_request_t *>(d_requests);
        rc = enqueue_gather(ka, d_text_pos_or_null, d_reference, ref_len, nullptr, n_pairs, gi.cand_t, stream);
        if (rc) return rc;
    }
    // pass 2 re-planned for its rows (smaller grids); the n_pairs plan where that would not fit the plans' region
    Plan pl2 = g.p2;
    if (bt) {
        Plan q;
        aim::Knobs quiet = kn;
        quiet.plan_debug = false;
        if (!make_plan(g.x2.base, hit ? hit->n_hits : n_reads, quiet, budget, &q) && q.scratch_total <= g.plan_bytes) pl2 = q;
    }
    return enqueue_groups(g, g.p1, pl2, kn, gi, stream, nullptr);
}
}  // namespace

int aim_align_device_groups(const aim_params_t *params, uint32_t n_pairs, uint32_t n_reads, const void *d_requests, const char *d_patterns,
                            const char *d_texts_or_null, const uint64_t *d_text_pos_or_null, const char *d_reference, uint64_t ref_len,
                            const uint32_t *d_read_offsets, void *d_results, char *d_ops, aim_best_t *d_best, void *d_scratch,
                            size_t scratch_bytes, void *hip_stream)
{
    if (!params) return fail(AIM_EINVAL, "params is NULL");
    if (!is_groups(*params)) return fail(AIM_EINVAL, "aim_align_device_groups needs AIM_FLAG_READ_GROUPS");
    if (is_mates(*params)) return fail(AIM_EINVAL, "AIM_FLAG_MATE_PAIRS is set: use aim_align_device_mates");
    if (is_hits(*params)) return fail(AIM_EINVAL, "AIM_FLAG_TOP_HITS is set: use aim_align_device_hits");
    return align_device_groups(params, n_pairs, n_reads, d_requests, d_patterns, d_texts_or_null, d_text_pos_or_null, d_reference, ref_len,
                               d_read_offsets, d_results, d_ops, d_best, nullptr, nullptr, nullptr, d_scratch, scratch_bytes, hip_stream);
}

int aim_hits_offsets(uint32_t n_reads, const uint32_t *read_offsets, uint32_t max_hits, uint32_t *hit_offsets, uint32_t *n_hits)
{
    return hits_offsets(n_reads, read_offsets, max_hits, hit_offsets, n_hits);
}

int aim_align_device_hits(const aim_params_t *params, uint32_t n_pairs, uint32_t n_reads, const void *d_requests, const char *d_patterns,
                          const char *d_texts_or_null, const uint64_t *d_text_pos_or_null, const char *d_reference, uint64_t ref_len,
                          const uint32_t *d_read_offsets, void *d_results, char *d_ops, aim_best_t *d_best, uint32_t max_hits,
                          const uint32_t *d_hit_offsets, uint32_t n_hits, uint32_t *d_hit_pair, void *d_scratch, size_t scratch_bytes,
                          void *hip_stream)
{
    if (!params) return fail(AIM_EINVAL, "params is NULL");
    if (!is_hits(*params)) return fail(AIM_EINVAL, "aim_align_device_hits needs AIM_FLAG_TOP_HITS");
    int rc = validate_params(*params);   // (names a missing AIM_FLAG_READ_GROUPS, or AIM_FLAG_MATE_PAIRS / AIM_FLAG_SAM_FIELDS)
    if (rc) return rc;
    if (max_hits < 1 || max_hits > AIM_TOP_HITS_MAX)
        return fail(AIM_EINVAL, "AIM_FLAG_TOP_HITS: max_hits %u is outside 1..%d", max_hits, AIM_TOP_HITS_MAX);
    if (n_hits > n_pairs || n_hits < n_reads)
        return fail(AIM_EINVAL, "AIM_FLAG_TOP_HITS: n_hits %u does not fit n_reads %u and n_pairs %u (aim_hits_offsets)", n_hits, n_reads, n_pairs);
    if (n_pairs && !d_hit_offsets) return fail(AIM_EINVAL, "AIM_FLAG_TOP_HITS: null d_hit_offsets");
    const HitArgs ha{max_hits, n_hits, d_hit_offsets, d_hit_pair};
    return align_device_groups(params, n_pairs, n_reads, d_requests, d_patterns, d_texts_or_null, d_text_pos_or_null, d_reference, ref_len,
                               d_read_offsets, d_results, d_ops, d_best, nullptr, nullptr, &ha, d_scratch, scratch_bytes, hip_stream);
}

int aim_align_device_mates(const aim_params_t *params, uint32_t n_pairs, uint32_t n_reads, const void *d_requests, const char *d_patterns,
                           const char *d_texts_or_null, const uint64_t *d_text_pos_or_null, const char *d_reference, uint64_t ref_len,
                           const uint32_t *d_read_offsets, void *d_results, char *d_ops, aim_best_t *d_best, int64_t min_span,
                           int64_t max_span, int32_t unpaired_penalty, aim_mate_t *d_mates, void *d_scratch, size_t scratch_bytes,
                           void *hip_stream)
{
    if (!params) return fail(AIM_EINVAL, "params is NULL");
    if (!is_mates(*params)) return fail(AIM_EINVAL, "aim_align_device_mates needs AIM_FLAG_MATE_PAIRS");
    int rc = validate_params(*params);   // (names a missing AIM_FLAG_READ_GROUPS / AIM_FLAG_REF_TEXTS)
    if (rc) return rc;
    if (d_texts_or_null) return fail(AIM_EINVAL, "AIM_FLAG_MATE_PAIRS: d_texts must be NULL (the texts are named by d_text_pos)");
    rc = check_mates(n_reads, min_span, max_span, unpaired_penalty);
    if (rc) return rc;
    aim::MateArgs ma;
    memset(&ma, 0, sizeof ma);
    ma.min_span = min_span;
    ma.max_span = max_span;
    ma.unpaired_penalty = unpaired_penalty;
    return align_device_groups(params, n_pairs, n_reads, d_requests, d_patterns, nullptr, d_text_pos_or_null, d_reference, ref_len,
                               d_read_offsets, d_results, d_ops, d_best, &ma, d_mates, nullptr, d_scratch, scratch_bytes, hip_stream);
}

}  // extern "C"
