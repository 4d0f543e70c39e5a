// capi_launch.hip -- the launcher of the C-ABI (include/aim_hip.h): what turns a Plan of capi_plan.hip into kernel launches on one stream.
// launch() follows a plan over the buffers a LaunchIo names (capi_set.hpp); aim_capi.hip's slots and capi_groups.hip's two passes go
// through it, and so do the two stateless entry points that are thin wrappers over it, aim_align_device and aim_align_device_ref, which
// are here. The aux stream of chunked wfa_group launches (a slot's own, or the device's shared one for stateless callers) is created
// here. Host code only: the kernels are launched through the launchers their headers declare.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>

#include "capi_set.hpp"
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
struct SharedAux { std::mutex mu; AuxStream aux; };
SharedAux *shared_aux_for_current_device()
{
    static SharedAux table[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) { (void)hipGetLastError(); return nullptr; }
    return &table[dev];
}

// Enqueue one alignment launch that follows the one-stage plan `pl` (made for >= io.n_pairs pairs under the caller's knobs and budget).
// list_in (AIM_FLAG_WFA_ESCALATE, second stage): the launch's pairs are those of the device-side list {count @0, pair ids @16..}, at most
// n_pairs of them; every buffer stays the batch's. Only wfa_group (+ its traceback) and wfa_wave take one.
int launch_one(const StagePlan &pl, const aim::Knobs &kn, const aim_params_t &p, const LaunchIo &io, hipStream_t stream,
               const FusedIo *fio = nullptr, AuxStream *slot_aux = nullptr, const uint32_t *list_in = nullptr)
{
    const uint32_t n_pairs = io.n_pairs;
    if (n_pairs == 0) return AIM_OK;
    const bool bt = p.flags & AIM_FLAG_BACKTRACE;
    if (list_in && pl.main.kid != K_WFA_GROUP && pl.main.kid != K_WFA_WAVE) return fail(AIM_EINVAL, "plan takes no pair list");
    if (pl.pk && !pl.pack_first && (!fio || !fio->packedP || !fio->packedT)) return fail(AIM_EINVAL, "plan reads packed rows but none were given");
    if (pl.emits_runs && (!fio || !fio->cig || !fio->runs || !fio->cursor)) return fail(AIM_EINVAL, "plan emits the compact CIGAR but no buffers were given");
    const bool reads_ascii = !(pl.main.kid == K_WFA_LANE_PK && !pl.pack_first);   // (wfa_group reads them for its to-do pairs even on packed batches)
    const bool writes_res = !(pl.main.kid == K_WFA_LANE_PK && pl.emits_runs);
    if (!io.req || (reads_ascii && (!io.pat || !io.txt)) || (writes_res && !io.res)) return fail(AIM_EINVAL, "null device buffer");
    if (bt && writes_res && !io.ops) return fail(AIM_EINVAL, "AIM_FLAG_BACKTRACE needs an ops buffer");
    if (io.scratch_bytes < pl.scratch_total || (!io.scratch && pl.scratch_total))
        return fail(AIM_EINVAL, "scratch too small: need %zu bytes, got %zu", pl.scratch_total, io.scratch_bytes);
    aim::KArgs ka0;
    ka0.p = p;
    ka0.n_pairs = n_pairs;
    ka0.req = static_cast<const aim_request_t *>(io.req);
    ka0.patterns = io.pat;
    ka0.texts = io.txt;
    ka0.res = static_cast<aim_result_t *>(io.res);
    ka0.ops = io.ops;
    ka0.todo = nullptr;
    ka0.dbg_poison_lds = poison_lds_word(kn);
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
    aim::KArgs ka = stage_args(ka0, m, io.scratch);
    // the fallback over the to-do list the main kernel filled: its own stage, the batch's ASCII rows
    aim::KArgs kb = stage_args(ka0, pl.fb, io.scratch);
    kb.todo = reinterpret_cast<const uint32_t *>((char *)io.scratch + pl.todo_at);
    kb.packedP = kb.packedT = nullptr;
    kb.cig = nullptr;
    if (kn.poison_ops >= 0 && io.ops && bt && !list_in)   // (the second stage keeps the first stage's rows) debugging aid: results must not depend on what the ops rows held before (only ops[begin_offset, end_offset) is written)
        HIP_TRY(hipMemsetAsync(io.ops, kn.poison_ops & 0xff, (size_t)n_pairs * 2 * p.read_size, stream));
    if (pl.todo_bytes) HIP_TRY(hipMemsetAsync((char *)io.scratch + pl.todo_at, 0, 64, stream));   // the to-do count, zeroed per launch
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
            char *base = (char *)io.scratch;
            uint32_t *flags_d = reinterpret_cast<uint32_t *>(base + pl.flags_at);
            uint32_t *pkP = reinterpret_cast<uint32_t *>(base + pl.pack_p_at), *pkT = reinterpret_cast<uint32_t *>(base + pl.pack_t_at);
            HIP_TRY(hipMemsetAsync(flags_d, 0, pl.pack_p_at - pl.flags_at, stream));
            aim::pack_rows_launch(ka, pkP, pkT, flags_d, reinterpret_cast<uint32_t *>(base + pl.todo_at), stream);
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
        const size_t rqb = req_size(p), rsb = res_size(p);
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
                kc.req = reinterpret_cast<const aim_request_t *>(static_cast<const char *>(io.req) + (size_t)first * rqb);
                if (io.pat) { kc.patterns = io.pat + (size_t)first * p.read_size; kc.texts = io.txt + (size_t)first * p.read_size; }
                if (io.res) kc.res = reinterpret_cast<aim_result_t *>(static_cast<char *>(io.res) + (size_t)first * rsb);
                if (io.ops) kc.ops = io.ops + (size_t)first * 2 * p.read_size;
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
            aim::unpack_todo_rows_launch(ka, kb.todo, ka.packedP, ka.packedT, const_cast<char *>(io.pat), const_cast<char *>(io.txt), stream);
            HIP_TRY(hipGetLastError());
        }
        launch_stage(p, pl.fb, kb, stream);
        if (pl.emits_runs) {   // the general kernel wrote result_t + ops rows for the to-do pairs: their compact CIGAR
            aim::cigar_rle_todo_launch(kb, kb.todo, ka.cig, ka.runs, ka.runs_cap, ka.cursor, stream);
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
        aim::KArgs k1 = stage_args(ka0, pl.fb, io.scratch);
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

}  // namespace

void aim::capi::aux_stream_destroy(AuxStream &a)
{
    for (int i = 0; i < 2; ++i) {
        if (a.computed[i]) (void)hipEventDestroy(a.computed[i]);
        if (a.walked[i]) (void)hipEventDestroy(a.walked[i]);
    }
    if (a.stream) (void)hipStreamDestroy(a.stream);
    a = AuxStream();
}

int aim::capi::launch(const Plan &pl, const aim::Knobs &kn, const aim_params_t &p, const LaunchIo &io, hipStream_t stream, const FusedIo *fio,
                      AuxStream *slot_aux)
{
    // (without the flag p may be the base of an extension struct, which launch_one reads through its address: no copy of it here)
    if (!pl.esc) return launch_one(pl, kn, p, io, stream, fio, slot_aux);
    aim_params_t q = p, p1 = p;
    q.flags &= ~AIM_FLAG_WFA_ESCALATE;
    if (!pl.esc_c || io.n_pairs == 0) return launch_one(pl, kn, q, io, stream, fio, slot_aux);
    if (io.scratch_bytes < pl.scratch_total || !io.scratch) return fail(AIM_EINVAL, "scratch too small: need %zu bytes, got %zu", pl.scratch_total, io.scratch_bytes);
    if (!io.res) return fail(AIM_EINVAL, "null device buffer");
    p1.flags = q.flags;
    p1.max_score = pl.esc_c;
    char *base = static_cast<char *>(io.scratch);
    StagePlan s1 = pl;
    s1.scratch_total = pl.s1_scratch;
    LaunchIo io1 = io, io2 = io;   // the two stages: the batch's buffers, each stage's own part of the scratch
    io1.scratch_bytes = pl.s2_at;
    io2.scratch = base + pl.s2_at;
    io2.scratch_bytes = pl.s2.scratch_total;
    int rc = launch_one(s1, kn, p1, io1, stream, fio, slot_aux);
    if (rc) return rc;
    uint32_t *list = reinterpret_cast<uint32_t *>(base + pl.list_at);
    uint2 *masks = reinterpret_cast<uint2 *>(base + pl.mask_at);
    uint32_t *counts = reinterpret_cast<uint32_t *>(base + pl.count_at);
    const bool res8 = p.flags & AIM_FLAG_RES8;
    aim::escalate_list_launch(static_cast<const uint32_t *>(io.res), io.n_pairs, res8 ? 2u : 6u, res8 ? 1u : 3u, (int32_t)(pl.esc_c + 1), masks, counts, list,
                              stream);
    HIP_TRY(hipGetLastError());
    if (pl.pk && !pl.s2.pk) {   // a packed batch whose second stage reads ASCII rows: the listed pairs' rows, expanded in place
        if (!io.pat || !io.txt || !fio || !fio->packedP || !fio->packedT) return fail(AIM_EINVAL, "null device buffer");
        aim::unpack_todo_rows_launch(batch_args(q, io.n_pairs, io.req), list, fio->packedP, fio->packedT, const_cast<char *>(io.pat), const_cast<char *>(io.txt),
                                     stream);
        HIP_TRY(hipGetLastError());
    }
    return launch_one(pl.s2, kn, q, io2, stream, fio, slot_aux, list);
}

int aim::capi::launch_todo_stage(const aim_params_t &p, const Stage &st, const LaunchIo &io, const uint32_t *todo, hipStream_t stream)
{
    aim::KArgs kb = batch_args(p, io.n_pairs, io.req);
    kb.res = static_cast<aim_result_t *>(io.res);
    kb.ops = io.ops;
    kb = stage_args(kb, st, io.scratch);
    kb.patterns = io.pat;
    kb.texts = io.txt;
    kb.todo = todo;
    launch_stage(p, st, kb, stream);
    HIP_TRY(hipGetLastError());
    return AIM_OK;
}

extern "C" {

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
    aim::gather_text_rows_launch(batch_args(*params, n_pairs, d_requests), d_text_pos, d_reference, ref_len, nullptr, n_pairs, rows, (hipStream_t)hip_stream);
    HIP_TRY(hipGetLastError());
    LaunchIo io;
    io.n_pairs = n_pairs; io.req = d_requests; io.pat = d_patterns; io.txt = rows;
    io.res = d_results; io.ops = d_ops; io.scratch = d_scratch; io.scratch_bytes = at;
    return launch(pl, kn, *params, io, (hipStream_t)hip_stream);
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
    LaunchIo io;
    io.n_pairs = n_pairs; io.req = d_requests; io.pat = d_patterns; io.txt = d_texts;
    io.res = d_results; io.ops = d_ops; io.scratch = d_scratch; io.scratch_bytes = scratch_bytes;
    return launch(pl, kn, *params, io, (hipStream_t)hip_stream);
}

}  // extern "C"
