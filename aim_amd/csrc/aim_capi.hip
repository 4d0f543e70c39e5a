// aim_capi.hip -- C-ABI (include/aim_hip.h) over the gfx950 alignment kernels.
//
// Host side of the drop-in boundary: what host.c does with dpu_alloc /
// dpu_push_xfer / dpu_launch (WFA/DPU-WRAM/host/host.c:186-330) is done here
// with one HIP stream per device, HBM buffers planned per configuration, and
// asynchronous copies.  No CPU fallback exists: every compute entry point
// needs a HIP device.  This unit is the device set: its slots and their buffers, push / launch / pull, aim_set_submit as a sequence of
// steps, aim_set_wait, the SAM entry points and the host-side checks of a batch. It compiles no kernel and launches no alignment kernel:
// a plan becomes launches in capi_launch.hip (launch(), with aim_align_device[_ref]), reached through capi_set.hpp like the read-groups
// path (AIM_FLAG_READ_GROUPS, MATE_PAIRS, TOP_HITS) of capi_groups.hip; the launch planner and the entry points that only plan are in
// capi_plan.hip (plan.hpp), the read-mapping pipeline's entry points in capi_pipeline.hip, the host-side helpers in capi_host.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "capi_set.hpp"
#include "wfa_lane_packed.hpp"   // kRunSlot
#include "batch_io.hpp"
#include "sam_fields.hpp"

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

int aim::capi::fail_drained(aim_slot &s, int rc)
{
    char keep[sizeof g_err];
    memcpy(keep, g_err, sizeof keep);
    (void)hipStreamSynchronize(s.stream);
    (void)hipGetLastError();
    memcpy(g_err, keep, sizeof keep);
    return rc;
}

void aim::capi::reset_slot(aim_slot &s, const aim_batch_io_t *io)
{
    s.io = *io;
    s.io_sam = nullptr;
    s.runs_sent = 0;
    s.pushed = s.launched = false;
    s.ref_pending = false;
}

int aim::capi::enqueue_rows_d2h(const aim_params_t &p, aim_slot &s, uint32_t rows)
{
    const aim_batch_io_t &io = s.io;
    if (io.cigars) {
        HIP_TRY(hipMemcpyAsync(s.h_cursor, s.d_cursor, 4, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipMemcpyAsync(io.cigars, s.d_cig, (size_t)rows * sizeof(aim_cigar_t), hipMemcpyDeviceToHost, s.stream));
        // slotted run buffer (wfa_lane_packed.hpp): the first 3 n runs are the pairs' own slots, known now -- their copy
        // overlaps the next batch instead of waiting in aim_set_wait for the cursor; only runs behind the slots follow there
        if (s.runs_sent) HIP_TRY(hipMemcpyAsync(io.runs, s.d_runs, (size_t)s.runs_sent * 4, hipMemcpyDeviceToHost, s.stream));
    }
    if (io.results) HIP_TRY(hipMemcpyAsync(io.results, s.d_res, (size_t)rows * res_size(p), hipMemcpyDeviceToHost, s.stream));
    if (io.ops) HIP_TRY(hipMemcpyAsync(io.ops, s.d_ops, (size_t)rows * 2 * (size_t)p.read_size, hipMemcpyDeviceToHost, s.stream));
    return AIM_OK;
}

namespace {

// A slot's allocations: made into a typed member and recorded in one of the slot's lists, which is all that releasing them reads
template <typename T>
hipError_t slot_alloc(std::vector<void *> &list, T *&member, size_t bytes)
{
    void *b = nullptr;
    const hipError_t e = hipMalloc(&b, bytes);
    if (e == hipSuccess) list.push_back(member = static_cast<T *>(b));
    return e;
}
// ... and the two pinned ones
hipError_t slot_alloc_pinned(aim_slot &s, uint32_t *&member, size_t bytes)
{
    const hipError_t e = hipHostMalloc((void **)&member, bytes, hipHostMallocDefault);
    if (e == hipSuccess) s.pinned.push_back(member);
    return e;
}

// The SAM buffers (aim_set_sam_capacity re-allocates them on a live slot). d_sam is what says that a slot has them.
void free_sam_buffers(aim_slot &s)
{
    for (void *b : s.owned_sam) (void)hipFree(b);
    s.owned_sam.clear();
    s.d_sam = nullptr;
    s.samcig_cap = s.sammd_cap = 0;
}

void free_slot(aim_slot &s)
{
    free_sam_buffers(s);
    for (void *b : s.owned) (void)hipFree(b);
    for (void *b : s.pinned) (void)hipHostFree(b);
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
// large batches are scanned branch-free by a few threads (any_nonzero) and only a failing scan is repeated to name the pair.
int aim::capi::check_lengths(const aim_params_t &p, uint32_t n_pairs, const void *requests, uint32_t *bad_pair)
{
    auto scan = [&](auto *r) -> int {   // (r: the requests in their own type, aim_request_t or aim_request8_t)
        const int rs = p.read_size;
        auto bad = [r, rs](size_t i) { return (uint32_t)((r[i].pattern_len < 0) | (r[i].text_len < 0) | (r[i].pattern_len > rs) | (r[i].text_len > rs)); };
        if (!any_nonzero(n_pairs, bad)) return AIM_OK;
        uint32_t i = 0;
        while (!bad(i)) ++i;
        if (bad_pair) *bad_pair = i;
        return fail(AIM_EINVAL, "READ LENGTH less than length of the input reads (pair %u)", i);  // host.c:119-123
    };
    return (p.flags & AIM_FLAG_REQ8) ? scan(static_cast<const aim_request8_t *>(requests)) : scan(static_cast<const aim_request_t *>(requests));
}

// AIM_FLAG_REF_TEXTS: every window [pos, pos + text_len) inside [0, ref_len) (bit 63 is the strand; an empty window is always
// inside). Scanned branch-free like check_lengths; only a failing scan is repeated to name the pair.
int aim::capi::check_windows(const aim_params_t &p, uint32_t n_pairs, const void *requests, const uint64_t *text_pos, uint64_t ref_len, uint32_t *bad_pair)
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

namespace {

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

// The slot's batch as a launch takes it: n_pairs pairs in the slot's own buffers
LaunchIo slot_launch_io(const aim_slot &s)
{
    LaunchIo io;
    io.n_pairs = s.n_pairs; io.req = s.d_req; io.pat = s.d_pat; io.txt = s.d_txt;
    io.res = s.d_res; io.ops = s.d_ops; io.scratch = s.d_scratch; io.scratch_bytes = s.scratch_bytes;
    return io;
}

int launch_on_slot(aim_set *set, aim_device_ctx &d, aim_slot &s, uint32_t mode = 0u, FusedIo *fio = nullptr)
{
    const Plan pl = plan_for_batch(set, d, s, s.n_pairs, mode);
    s.plan_last = pl;
    if (fio && pl.emits_runs) {   // slotted run buffer: pair p owns runs[3p, 3p + 3), the cursor starts behind the slots (wfa_lane_packed.hpp)
        fio->run_slot = (pl.main.kid == K_WFA_LANE_PK && (uint64_t)s.n_pairs * aim::kRunSlot <= fio->runs_cap) ? aim::kRunSlot : 0u;
        HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)fio->cursor, (int)(s.n_pairs * fio->run_slot), 1, s.stream));
    }
    return launch(pl, set->knobs, set->params, slot_launch_io(s), s.stream, fio, &s.aux);
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
}  // namespace

// AIM_FLAG_SAM_FIELDS on a slot: what aim_set_submit checks before anything is enqueued; *sio receives the struct (nullptr without the flag)
int aim::capi::check_sam_io(const aim_set *set, const aim_slot &s, const aim_batch_io_t *io, const aim_batch_io_sam_t **sio)
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
int aim::capi::enqueue_sam_on_slot(const aim_set *set, const aim_device_ctx &d, aim_slot &s, const aim_batch_io_sam_t *sio, uint32_t n_rows, const uint32_t *sel)
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
int aim::capi::enqueue_sam_d2h(aim_slot &s, uint32_t n_rows)
{
    HIP_TRY(hipMemcpyAsync(s.h_samcur, s.d_samcur, 8, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipMemcpyAsync(s.io_sam, s.d_sam, (size_t)n_rows * sizeof(aim_sam_t), hipMemcpyDeviceToHost, s.stream));
    return AIM_OK;
}


namespace {

// What the steps of one aim_set_submit share: the batch as check_submit_io read it, then what choose_plan decided for it
struct Batch {
    uint32_t n = 0;
    bool ref = false, packed = false;             // AIM_FLAG_REF_TEXTS; packed rows in
    const uint64_t *text_pos = nullptr;           // ref: io is the base of an aim_batch_io_ref_t and the texts are windows of the device's reference
    const aim_batch_io_sam_t *sio = nullptr;      // AIM_FLAG_SAM_FIELDS: io is the base of one
    uint32_t mode = 0;
    Plan pl;
    uint32_t runs_cap = 0;
    bool ref_fused = false;                       // a packed REF_TEXTS batch that keeps the fused packed lane kernel ...
    Stage ref_fb;                                 // ... and the general kernel's stage over its to-do windows
};

// Every refusal of a batch, before anything is enqueued
int check_submit_io(const aim_set *set, const aim_device_ctx &d, const aim_slot &s, const aim_batch_io_t *io, Batch *b)
{
    const aim_params_t &p = set->params;
    const uint32_t n = b->n = io->n_pairs;
    const bool bt = p.flags & AIM_FLAG_BACKTRACE;
    const bool ref = b->ref = is_ref(p);
    const uint64_t *text_pos = b->text_pos = ref ? reinterpret_cast<const aim_batch_io_ref_t *>(io)->text_pos : nullptr;
    if (ref && (io->texts || io->packed_texts || io->raw_texts))
        return fail(AIM_EINVAL, "AIM_FLAG_REF_TEXTS: texts, packed_texts and raw_texts must be NULL (the texts are named by text_pos)");
    if (ref && n && !text_pos) return fail(AIM_EINVAL, "AIM_FLAG_REF_TEXTS: null text_pos");
    if (ref && !d.d_ref) return fail(AIM_ESTATE, "AIM_FLAG_REF_TEXTS: no reference on device %d (aim_set_reference)", d.dev);
    const bool packed = b->packed = io->packed_patterns || io->packed_texts;
    if (n > set->max_pairs) return fail(AIM_EINVAL, "n_pairs %u exceeds configured capacity %u", n, set->max_pairs);
    if (n && !io->requests) return fail(AIM_EINVAL, "null requests");
    if (n && packed && (!io->packed_patterns || (!ref && !io->packed_texts) || !s.d_packP))
        return fail(AIM_EINVAL, "packed batch needs both packed arrays and a set configured with max_raw_pairs > 0");
    if (n && !packed && (!io->patterns || (!ref && !io->texts))) return fail(AIM_EINVAL, "null sequence rows");
    if (packed && io->n_raw > set->max_raw) return fail(AIM_EINVAL, "n_raw %u exceeds configured capacity %u", io->n_raw, set->max_raw);
    if (packed && io->n_raw && (!io->raw_pairs || !io->raw_patterns || (!ref && !io->raw_texts))) return fail(AIM_EINVAL, "null raw side list");
    if (io->cigars && (!bt || !s.d_cig || !io->runs)) return fail(AIM_EINVAL, "compact CIGAR needs AIM_FLAG_BACKTRACE, max_runs > 0 and a run buffer");
    if (int rc = check_sam_io(set, s, io, &b->sio)) return rc;
    if (n && !io->results && !io->cigars && !b->sio) return fail(AIM_EINVAL, "no output buffer");
    if (io->ops && !bt) return fail(AIM_EINVAL, "ops requested without AIM_FLAG_BACKTRACE");
    if (int rc = check_lengths(p, n, io->requests)) return rc;
    if (ref)
        if (int rc = check_windows(p, n, io->requests, text_pos, d.ref_len, nullptr)) return rc;
    if (packed)
        for (uint32_t j = 0; j < io->n_raw; ++j)
            if (io->raw_pairs[j] >= n) return fail(AIM_EINVAL, "raw_pairs[%u] = %u is outside the batch", j, io->raw_pairs[j]);
    return AIM_OK;
}

// Does the alignment kernel of this configuration take the batch as it arrived and deliver what was asked for?
// (wfa_lane_packed_kernel: packed rows in, {idx, score} or compact CIGAR out.) Then this batch is ONE kernel;
// otherwise the conversion kernels of batch_io.hpp run around the default-ABI kernel.
void choose_plan(aim_set *set, aim_device_ctx &d, aim_slot &s, Batch &b)
{
    const aim_batch_io_t &io = s.io;
    b.runs_cap = std::min(io.runs_cap, set->max_runs);
    b.mode = (b.packed ? MODE_PACKED_IN : 0u) | ((io.cigars && !io.results && !io.ops && !b.sio) ? MODE_RUNS_OUT : 0u);   // (the SAM kernel reads ops rows)
    b.pl = plan_for_batch(set, d, s, b.n, b.mode);
    // AIM_FLAG_REF_TEXTS: a packed batch keeps the fused packed lane kernel (its texts gathered as packed rows, the windows
    // holding a byte outside A/C/G/T re-aligned by the general kernel over a to-do list); every other plan runs as for an
    // ASCII batch after the gather
    b.ref_fused = b.ref && b.packed && b.pl.pk && b.pl.main.kid == K_WFA_LANE_PK && !b.pl.pack_first && s.d_reftodo && !b.pl.esc_c &&
                  ref_todo_stage(set, d, s.scratch_bytes, b.n, &b.ref_fb);
    if (b.ref && b.packed && !b.ref_fused && b.pl.pk) {
        b.mode &= ~MODE_PACKED_IN;
        b.pl = plan_for_batch(set, d, s, b.n, b.mode);
    }
}

// The KArgs of the batch-I/O kernels around the slot's alignment: the batch's requests and its result and ops rows
aim::KArgs slot_args(const aim_params_t &p, const aim_slot &s)
{
    aim::KArgs ka = batch_args(p, s.n_pairs, s.d_req);
    ka.res = static_cast<aim_result_t *>(s.d_res);
    ka.ops = s.d_ops;
    return ka;
}

// The H2D copies of a batch
int enqueue_inputs(const aim_params_t &p, aim_slot &s, const Batch &b)
{
    const aim_batch_io_t &io = s.io;
    const size_t n = b.n, rs = (size_t)p.read_size, rowb = (size_t)aim::packed_row_dwords(p.read_size) * 4;
    HIP_TRY(hipMemcpyAsync(s.d_req, io.requests, n * req_size(p), hipMemcpyHostToDevice, s.stream));
    if (b.ref) HIP_TRY(hipMemcpyAsync(s.d_tpos, b.text_pos, n * 8, hipMemcpyHostToDevice, s.stream));
    if (!b.packed) {
        HIP_TRY(hipMemcpyAsync(s.d_pat, io.patterns, n * rs, hipMemcpyHostToDevice, s.stream));
        if (!b.ref) HIP_TRY(hipMemcpyAsync(s.d_txt, io.texts, n * rs, hipMemcpyHostToDevice, s.stream));
        return AIM_OK;
    }
    HIP_TRY(hipMemcpyAsync(s.d_packP, io.packed_patterns, n * rowb, hipMemcpyHostToDevice, s.stream));
    if (!b.ref) HIP_TRY(hipMemcpyAsync(s.d_packT, io.packed_texts, n * rowb, hipMemcpyHostToDevice, s.stream));
    if (io.n_raw) {
        HIP_TRY(hipMemcpyAsync(s.d_rawidx, io.raw_pairs, (size_t)io.n_raw * 4, hipMemcpyHostToDevice, s.stream));
        HIP_TRY(hipMemcpyAsync(s.d_rawP, io.raw_patterns, (size_t)io.n_raw * rs, hipMemcpyHostToDevice, s.stream));
        if (!b.ref) HIP_TRY(hipMemcpyAsync(s.d_rawT, io.raw_texts, (size_t)io.n_raw * rs, hipMemcpyHostToDevice, s.stream));
    }
    return AIM_OK;
}

// The rows as the plan's kernel reads them: packed rows expanded where it reads ASCII, REF_TEXTS windows gathered
int enqueue_text_rows(const aim_set *set, const aim_device_ctx &d, aim_slot &s, const Batch &b)
{
    const aim_batch_io_t &io = s.io;
    const aim::KArgs ka = slot_args(set->params, s);
    if (b.packed && !b.pl.pk) {   // expand into the reference's char[n][READ_SIZE] layout (batch_io.hpp), then run as usual
        const unsigned rows = b.ref ? 1u : 2u;   // (grid.y 0: patterns; the texts of a reference batch are gathered below)
        aim::unpack_rows_launch(ka, s.d_packP, s.d_packT, s.d_pat, s.d_txt, rows, s.stream);
        if (io.n_raw) aim::scatter_raw_rows_launch(set->params.read_size, io.n_raw, s.d_rawidx, s.d_rawP, s.d_rawT, s.d_pat, s.d_txt, rows, s.stream);
        HIP_TRY(hipGetLastError());
    }
    if (b.ref_fused) {
        // packed text rows + to-do list; the side list's (non-ACGT patterns) text rows as ASCII for the raw side pass
        uint32_t *flag_bits = s.d_reftodo + 16 + set->max_pairs;
        HIP_TRY(hipMemsetAsync(s.d_reftodo, 0, 64, s.stream));
        HIP_TRY(hipMemsetAsync(flag_bits, 0, ((size_t)b.n + 31) / 32 * 4, s.stream));
        aim::gather_text_packed_launch(ka, s.d_tpos, d.d_ref, d.ref_len, s.d_packT, flag_bits, s.d_reftodo, s.stream);
        HIP_TRY(hipGetLastError());
        if (io.n_raw) {
            aim::gather_text_rows_launch(ka, s.d_tpos, d.d_ref, d.ref_len, s.d_rawidx, io.n_raw, s.d_rawT, s.stream);
            HIP_TRY(hipGetLastError());
        }
    } else if (b.ref) {
        aim::gather_text_rows_launch(ka, s.d_tpos, d.d_ref, d.ref_len, nullptr, b.n, s.d_txt, s.stream);
        HIP_TRY(hipGetLastError());
    }
    return AIM_OK;
}

// The plan's launches over the slot's batch, then what completes its rows: the to-do windows of a fused REF_TEXTS batch, and the
// compact CIGAR as a pass of its own when the plan's kernel does not emit runs
int enqueue_alignment(aim_set *set, aim_device_ctx &d, aim_slot &s, const Batch &b)
{
    const aim_params_t &p = set->params;
    const aim::KArgs ka = slot_args(p, s);
    FusedIo fio;
    if (b.pl.pk) { fio.packedP = s.d_packP; fio.packedT = s.d_packT; }
    if (b.pl.emits_runs) { fio.cig = s.d_cig; fio.runs = s.d_runs; fio.cursor = s.d_cursor; fio.runs_cap = b.runs_cap; }
    if (int rc = launch_on_slot(set, d, s, b.mode, &fio)) return rc;
    if (b.ref_fused) {
        // the to-do windows: ASCII rows (pattern unpacked, text gathered), the general kernel over them, their compact CIGAR
        aim::gather_todo_rows_launch(ka, s.d_reftodo, s.d_tpos, d.d_ref, d.ref_len, s.d_packP, s.d_pat, s.d_txt, s.stream);
        HIP_TRY(hipGetLastError());
        if (int rc = launch_todo_stage(p, b.ref_fb, slot_launch_io(s), s.d_reftodo, s.stream)) return rc;
        if (b.pl.emits_runs) {
            aim::cigar_rle_todo_launch(ka, s.d_reftodo, s.d_cig, s.d_runs, b.runs_cap, s.d_cursor, s.stream);
            HIP_TRY(hipGetLastError());
        }
    }
    s.runs_sent = b.pl.emits_runs ? b.n * fio.run_slot : 0u;   // 0 when the run buffer is bump-allocated: nothing is known before the kernel ran
    if (s.io.cigars && !b.pl.emits_runs) {
        HIP_TRY(hipMemsetAsync(s.d_cursor, 0, 4, s.stream));
        aim::cigar_rle_launch(ka, s.d_cig, s.d_runs, b.runs_cap, s.d_cursor, s.stream);
        HIP_TRY(hipGetLastError());
    }
    return AIM_OK;
}

// Raw side pass: the pairs of the side list hold a byte outside A/C/G/T (the reference compares raw bytes,
// host.c:126-127); what the packed kernel computed for them is void. They are aligned as a batch of their own by
// the ASCII kernels -- requests gathered, the side list's rows are its patterns / texts -- and their results
// replace the void ones (with the compact CIGAR: their runs are appended to the run buffer).
int enqueue_raw_side_pass(aim_set *set, aim_device_ctx &d, aim_slot &s, const Batch &b)
{
    const aim_params_t &p = set->params;
    const aim_batch_io_t &io = s.io;
    const uint32_t nr = io.n_raw;
    if (!b.pl.pk || !nr) return AIM_OK;
    const uint32_t rq_dw = (uint32_t)req_size(p) / 4, rs_dw = (uint32_t)res_size(p) / 4;
    aim::gather_elems_launch((const uint32_t *)s.d_req, s.d_rawidx, nr, rq_dw, (uint32_t *)s.d_rawreq, s.stream);
    HIP_TRY(hipGetLastError());
    LaunchIo raw;
    raw.n_pairs = nr; raw.req = s.d_rawreq; raw.pat = s.d_rawP; raw.txt = s.d_rawT;
    raw.res = s.d_rawres; raw.ops = s.d_rawops; raw.scratch = s.d_scratch; raw.scratch_bytes = s.scratch_bytes;
    if (int rc = launch(plan_for_batch(set, d, s, nr, 0u), set->knobs, p, raw, s.stream, nullptr, &s.aux)) return rc;
    // (both outputs may be asked for at once -- aim_cigar_t + runs AND result_t [+ ops rows]: each gets its own scatter)
    if (io.cigars) {
        aim::KArgs kr = slot_args(p, s);
        kr.n_pairs = nr;
        kr.res = static_cast<aim_result_t *>(s.d_rawres);
        kr.ops = s.d_rawops;
        aim::cigar_rle_launch(kr, s.d_rawcig, s.d_runs, b.runs_cap, s.d_cursor, s.stream);
        aim::scatter_elems_launch((const uint32_t *)s.d_rawcig, s.d_rawidx, nr, 4u, (uint32_t *)s.d_cig, s.stream);
    }
    if (!io.cigars || io.results || io.ops || b.sio) {
        aim::scatter_elems_launch((const uint32_t *)s.d_rawres, s.d_rawidx, nr, rs_dw, (uint32_t *)s.d_res, s.stream);
        if (p.flags & AIM_FLAG_BACKTRACE)   // default output (result_t + ops rows): the side list's ops rows go home too
            aim::scatter_elems_launch((const uint32_t *)s.d_rawops, s.d_rawidx, nr, (uint32_t)(2 * p.read_size / 4), (uint32_t *)s.d_ops, s.stream);
    }
    HIP_TRY(hipGetLastError());
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
           AIM_FEATURE_MAPPER | AIM_FEATURE_CONTIGS | AIM_FEATURE_PAIRED | AIM_FEATURE_PAIR_ESTIMATE | AIM_FEATURE_SECONDARY | AIM_FEATURE_PAIR_SECONDARY;
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
        HIP_TRY(slot_alloc(s.owned, s.d_req, (size_t)max_pairs * req_size(*params)));
        HIP_TRY(slot_alloc(s.owned, s.d_res, (size_t)max_pairs * res_size(*params)));
        HIP_TRY(slot_alloc(s.owned, s.d_pat, (size_t)max_pairs * rs + 64));
        HIP_TRY(slot_alloc(s.owned, s.d_txt, (size_t)max_pairs * rs + 64));
        if (params->flags & AIM_FLAG_BACKTRACE) HIP_TRY(slot_alloc(s.owned, s.d_ops, (size_t)max_pairs * 2 * rs + 64));
        if (max_raw) {
            HIP_TRY(slot_alloc(s.owned, s.d_packP, (size_t)max_pairs * rowdw * 4 + 64));
            HIP_TRY(slot_alloc(s.owned, s.d_packT, (size_t)max_pairs * rowdw * 4 + 64));
            HIP_TRY(slot_alloc(s.owned, s.d_rawidx, (size_t)max_raw * 4));
            HIP_TRY(slot_alloc(s.owned, s.d_rawP, (size_t)max_raw * rs + 64));   // (+64 B: the raw side pass hands them to the ASCII kernels as patterns / texts, aim_hip.h tail slack)
            HIP_TRY(slot_alloc(s.owned, s.d_rawT, (size_t)max_raw * rs + 64));
            HIP_TRY(slot_alloc(s.owned, s.d_rawreq, (size_t)max_raw * req_size(*params)));
            HIP_TRY(slot_alloc(s.owned, s.d_rawres, (size_t)max_raw * res_size(*params)));
            if (params->flags & AIM_FLAG_BACKTRACE) HIP_TRY(slot_alloc(s.owned, s.d_rawops, (size_t)max_raw * 2 * rs + 64));
            if (max_runs) HIP_TRY(slot_alloc(s.owned, s.d_rawcig, (size_t)max_raw * sizeof(aim_cigar_t)));
        }
        if (is_ref(*params)) {
            HIP_TRY(slot_alloc(s.owned, s.d_tpos, (size_t)max_pairs * 8));
            if (max_raw && params->algo == AIM_ALGO_WFA)
                HIP_TRY(slot_alloc(s.owned, s.d_reftodo, 64 + (size_t)max_pairs * 4 + ((size_t)max_pairs + 31) / 32 * 4));
        }
        if (is_groups(*params)) {
            HIP_TRY(slot_alloc(s.owned, s.g_readP, (size_t)max_pairs * rs + 64));
            HIP_TRY(slot_alloc(s.owned, s.g_roff, ((size_t)max_pairs + 1) * 4));
            HIP_TRY(slot_alloc(s.owned, s.g_map, (size_t)max_pairs * 4));
            HIP_TRY(slot_alloc(s.owned, s.g_sel, (size_t)max_pairs * 4));
            if (max_raw) HIP_TRY(slot_alloc(s.owned, s.g_rawslot, (size_t)max_pairs * 4));
            HIP_TRY(slot_alloc(s.owned, s.g_res1, (size_t)max_pairs * sizeof(aim_result_t)));
            HIP_TRY(slot_alloc(s.owned, s.g_best, (size_t)max_pairs * sizeof(aim_best_t)));
            if (is_mates(*params)) HIP_TRY(slot_alloc(s.owned, s.g_mates, ((size_t)max_pairs / 2 + 1) * sizeof(aim_mate_t)));
            if (is_hits(*params)) {
                HIP_TRY(slot_alloc(s.owned, s.g_hoff, ((size_t)max_pairs + 1) * 4));
                HIP_TRY(slot_alloc(s.owned, s.g_hit, (size_t)max_pairs * 4));
            }
            if (params->flags & AIM_FLAG_BACKTRACE) {
                HIP_TRY(slot_alloc(s.owned, s.g_req2, (size_t)max_pairs * req_size(*params)));
                HIP_TRY(slot_alloc(s.owned, s.g_pat2, (size_t)max_pairs * rs + 64));
                HIP_TRY(slot_alloc(s.owned, s.g_txt2, (size_t)max_pairs * rs + 64));
            }
        }
        if (max_runs) {
            HIP_TRY(slot_alloc(s.owned, s.d_cig, (size_t)max_pairs * sizeof(aim_cigar_t)));
            HIP_TRY(slot_alloc(s.owned, s.d_runs, (size_t)max_runs * 4));
            HIP_TRY(slot_alloc(s.owned, s.d_cursor, 64));
            HIP_TRY(slot_alloc_pinned(s, s.h_cursor, 64));
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
                if (want && (e = slot_alloc(s.owned, s.d_scratch, want)) != hipSuccess) break;
            }
            if (e == hipSuccess) break;
            (void)hipGetLastError();
            for (auto &s : d.slots) {
                if (s.d_scratch) { (void)hipFree(s.d_scratch); s.owned.pop_back(); }   // (the scratch is the last the slot recorded)
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
            aim::gather_text_rows_launch(batch_args(set->params, s.n_pairs, s.d_req), s.d_tpos, d.d_ref, d.ref_len, nullptr, s.n_pairs, s.d_txt, s.stream);
            HIP_TRY(hipGetLastError());
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

int aim_set_submit(aim_set_t *set, uint32_t device, uint32_t slot, const aim_batch_io_t *io)
{
    if (!set || device >= set->devs.size() || !io) return fail(AIM_EINVAL, "bad arguments");
    if (!set->configured) return fail(AIM_ESTATE, "aim_set_configure has not been called");
    aim_device_ctx &d = set->devs[device];
    if (slot >= d.slots.size()) return fail(AIM_EINVAL, "slot %u not configured (%zu slots)", slot, d.slots.size());
    aim_slot &s = d.slots[slot];
    if (s.submitted) return fail(AIM_ESTATE, "slot %u of device %d holds a batch: aim_set_wait it first", slot, d.dev);
    if (is_groups(set->params)) return submit_groups(set, d, s, io);
    Batch b;
    if (int rc = check_submit_io(set, d, s, io, &b)) return rc;
    HIP_TRY(hipSetDevice(d.dev));
    reset_slot(s, io);
    s.n_pairs = b.n;
    // Everything below only enqueues work on the slot's stream. Should an enqueue fail half-way, the copies already queued
    // still reference the caller's buffers: the stream is drained before the error is returned, so that a failed submit
    // never leaves the slot (or the caller's memory) in flight.
    auto enqueue = [&]() -> int {
        int rc = AIM_OK;
        HIP_TRY(hipEventRecord(s.ev[0], s.stream));
        if (b.n && (rc = enqueue_inputs(set->params, s, b))) return rc;
        HIP_TRY(hipEventRecord(s.ev[1], s.stream));
        HIP_TRY(hipEventRecord(s.ev[2], s.stream));
        if (b.n) choose_plan(set, d, s, b);
        if (b.n && (rc = enqueue_text_rows(set, d, s, b))) return rc;
        if (b.n && (rc = enqueue_alignment(set, d, s, b))) return rc;
        if (b.n && (rc = enqueue_raw_side_pass(set, d, s, b))) return rc;
        if (b.n && b.sio && (rc = enqueue_sam_on_slot(set, d, s, b.sio, b.n, nullptr))) return rc;   // the records of the final rows (the raw side pass's rows are home)
        HIP_TRY(hipEventRecord(s.ev[3], s.stream));
        HIP_TRY(hipEventRecord(s.ev[4], s.stream));
        if (b.n && b.sio && (rc = enqueue_sam_d2h(s, b.n))) return rc;
        if (b.n && (rc = enqueue_rows_d2h(set->params, s, b.n))) return rc;
        HIP_TRY(hipEventRecord(s.ev[5], s.stream));
        return AIM_OK;
    };
    if (int rc = enqueue()) return fail_drained(s, rc);
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
            free_sam_buffers(s);
            HIP_TRY(slot_alloc(s.owned_sam, s.d_samcig, (size_t)max_cigar_words * 4));
            HIP_TRY(slot_alloc(s.owned_sam, s.d_sammd, (size_t)max_md_bytes));
            HIP_TRY(slot_alloc(s.owned_sam, s.d_samcur, 64));
            if (!s.h_samcur) HIP_TRY(slot_alloc_pinned(s, s.h_samcur, 64));
            HIP_TRY(slot_alloc(s.owned_sam, s.d_sam, (size_t)set->max_pairs * sizeof(aim_sam_t)));   // last: a slot with d_sam is complete
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


int aim_ref_windows_check(const aim_params_t *params, uint32_t n_pairs, const void *requests, const uint64_t *text_pos, uint64_t ref_len,
                          uint32_t *bad_pair)
{
    if (!params || (n_pairs && (!requests || !text_pos))) return fail(AIM_EINVAL, "bad arguments");
    if (int rc = check_lengths(*params, n_pairs, requests, bad_pair)) return rc;
    return check_windows(*params, n_pairs, requests, text_pos, ref_len, bad_pair);
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

}  // extern "C"
