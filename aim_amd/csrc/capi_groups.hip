// capi_groups.hip -- the read-groups path of the C-ABI (include/aim_hip.h): AIM_FLAG_READ_GROUPS, AIM_FLAG_MATE_PAIRS and
// AIM_FLAG_TOP_HITS. A groups batch on a slot (submit_groups, which aim_set_submit hands such a batch to), the stateless entry points
// and the host-side checks of their inputs. Host code only: the kernels are launched through groups.hpp, hits.hpp, mates.hpp and
// batch_io.hpp, the two alignment passes through launch() of capi_launch.hip; that and what a groups batch shares with aim_set_submit
// of aim_capi.hip (the slot's reset, the copies of its output rows, the checks) are declared in capi_set.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>

#include "capi_set.hpp"
#include "batch_io.hpp"
#include "groups.hpp"
#include "hits.hpp"
#include "mates.hpp"

using namespace aim::capi;

namespace {

// Device buffers of one groups batch (a slot's, or carved from the stateless scratch). What a batch does not have stays zero.
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
    aim::MateArgs mate;          // ... the pairing parameters (n_mates and lanes are filled in by mate_select_launch) ...
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

// Everything after the texts are candidate rows (cand_t): expand the read rows, pass 1, select, then pass 2 or the result gather.
// pl1 / pl2: the passes' plans for this batch (each fits io.scratch_bytes).
int enqueue_groups(const GroupsPlan &g, const Plan &pl1, const Plan &pl2, const aim::Knobs &kn, const GroupsIo &io, hipStream_t stream,
                   AuxStream *aux)
{
    const aim_params_t &p1 = g.x1.base, &p2 = g.x2.base;
    const uint32_t n = io.n_pairs, nr = io.n_reads;
    if (!n) return AIM_OK;
    const aim::KArgs ka = batch_args(p1, n, io.req);
    aim::group_map_launch(io.roff, nr, n, io.map, stream);
    HIP_TRY(hipGetLastError());
    if (io.read_rows) {
        aim::group_rows_launch(ka, io.read_rows, nr, io.map, n, 0, io.cand_p, stream);
        HIP_TRY(hipGetLastError());
    } else {
        HIP_TRY(hipMemsetAsync(io.raw_slot, 0xff, (size_t)nr * 4, stream));
        if (io.n_raw) aim::group_raw_slot_launch(io.raw_pairs, io.n_raw, nr, io.raw_slot, stream);
        aim::group_unpack_launch(ka, io.packed, io.map, io.raw_slot, io.raw_rows, io.n_raw, nr, io.cand_p, stream);
        HIP_TRY(hipGetLastError());
    }
    LaunchIo pass;   // pass 1: every candidate, score rows only
    pass.n_pairs = n; pass.req = io.req; pass.pat = io.cand_p; pass.txt = io.cand_t;
    pass.res = io.res1; pass.scratch = io.scratch; pass.scratch_bytes = io.scratch_bytes;
    int rc = launch(pl1, kn, p1, pass, stream, nullptr, aux);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(io.sel, 0, (size_t)nr * 4, stream));   // (a read the CSR check would refuse keeps a valid sel)
    aim::group_select_launch(io.res1, n, io.roff, nr, io.best, io.sel, stream);
    HIP_TRY(hipGetLastError());
    if (g.mates && nr >= 2) {
        aim::mate_select_launch(ka, io.mate, nr, io.res1, io.tpos, io.roff, io.best, io.sel, io.mates, stream);
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
        aim::hit_select_launch(io.res1, n, io.roff, nr, io.hoff, io.max_hits, rows, io.hit_pair, stream);
        HIP_TRY(hipGetLastError());
    }
    if (!g.pass2) {
        aim::group_results_launch(io.res1, row_cand, rows, (int)((p2.flags & AIM_FLAG_RES8) != 0), io.res, stream);
        HIP_TRY(hipGetLastError());
        return AIM_OK;
    }
    // the rows as a batch of their own: requests, pattern rows (already cut to pattern_len) and text rows gathered by candidate
    aim::gather_elems_launch(static_cast<const uint32_t *>(io.req), row_cand, rows, (uint32_t)req_size(p2) / 4, static_cast<uint32_t *>(io.req2), stream);
    HIP_TRY(hipGetLastError());
    aim::KArgs k2 = ka;
    k2.p = p2;
    k2.n_pairs = rows;
    k2.req = static_cast<const aim_request_t *>(io.req2);
    aim::group_rows_launch(k2, io.cand_p, n, row_cand, rows, 0, io.pat2, stream);
    HIP_TRY(hipGetLastError());
    aim::group_rows_launch(k2, io.cand_t, n, row_cand, rows, 1, io.txt2, stream);
    HIP_TRY(hipGetLastError());
    pass.n_pairs = rows; pass.req = io.req2; pass.pat = io.pat2; pass.txt = io.txt2;   // pass 2: the rows behind the selection
    pass.res = io.res; pass.ops = io.ops;
    return launch(pl2, kn, p2, pass, stream, nullptr, aux);
}

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

}  // namespace

// aim_set_submit under AIM_FLAG_READ_GROUPS
int aim::capi::submit_groups(aim_set *set, aim_device_ctx &d, aim_slot &s, const aim_batch_io_t *io)
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
    reset_slot(s, io);
    s.n_pairs = rows;        // aim_set_wait reads n_pairs output rows
    s.n_reads = nr;
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
                aim::gather_text_rows_launch(batch_args(p, n, s.d_req), s.d_tpos, d.d_ref, d.ref_len, nullptr, n, s.d_txt, s.stream);
                HIP_TRY(hipGetLastError());
            }
            const Plan pl1 = pass_plan(set, d, s, g.x1.base, n, d.plan);
            const Plan pl2 = bt ? pass_plan(set, d, s, g.x2.base, rows, d.plan2) : Plan();
            s.plan_last = pl1;
            s.plan_last2 = pl2;
            GroupsIo gi{};
            gi.n_pairs = n;
            gi.n_reads = nr;
            gi.req = s.d_req;
            if (packed) {
                gi.packed = s.d_packP;
                gi.raw_pairs = s.d_rawidx;
                gi.raw_rows = s.d_rawP;
                gi.n_raw = io->n_raw;
                gi.raw_slot = s.g_rawslot;
            } else {
                gi.read_rows = s.g_readP;
            }
            gi.roff = s.g_roff;
            gi.cand_p = s.d_pat;
            gi.cand_t = s.d_txt;
            gi.res1 = s.g_res1;
            gi.map = s.g_map;
            gi.sel = s.g_sel;
            gi.best = s.g_best;
            gi.tpos = s.d_tpos;
            if (mio) {
                gi.mate.min_span = mio->min_span;
                gi.mate.max_span = mio->max_span;
                gi.mate.unpaired_penalty = mio->unpaired_penalty;
            }
            gi.mates = s.g_mates;
            if (hio) {
                gi.n_hits = rows;
                gi.max_hits = hio->max_hits;
            }
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
                aim::KArgs k2 = batch_args(g.x2.base, rows, s.g_req2);
                k2.res = static_cast<aim_result_t *>(s.d_res);
                k2.ops = s.d_ops;
                HIP_TRY(hipMemsetAsync(s.d_cursor, 0, 4, s.stream));
                aim::cigar_rle_launch(k2, s.d_cig, s.d_runs, std::min(io->runs_cap, set->max_runs), s.d_cursor, s.stream);
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
            if (int crc = enqueue_rows_d2h(p, s, rows)) return crc;   // (runs_sent is 0: a groups batch's runs all follow in aim_set_wait)
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
    if (rc) return fail_drained(s, rc);   // (as aim_set_submit: nothing stays in flight on a failed submit)
    s.submitted = true;
    return AIM_OK;
}

extern "C" {

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
    GroupsIo gi{};
    gi.n_pairs = n_pairs;
    gi.n_reads = n_reads;
    gi.req = d_requests;
    gi.read_rows = d_patterns;
    gi.roff = d_read_offsets;
    gi.cand_p = base + g.cand_p_at;
    gi.cand_t = ref ? base + g.cand_t_at : const_cast<char *>(d_texts_or_null);
    gi.res1 = reinterpret_cast<aim_result_t *>(base + g.res1_at);
    gi.map = reinterpret_cast<uint32_t *>(base + g.map_at);
    gi.sel = reinterpret_cast<uint32_t *>(base + g.sel_at);
    gi.best = d_best ? d_best : (mate ? reinterpret_cast<aim_best_t *>(base + g.best_at) : nullptr);
    gi.tpos = d_text_pos_or_null;
    if (mate) gi.mate = *mate;
    gi.mates = d_mates;
    if (hit) {
        gi.n_hits = hit->n_hits;
        gi.max_hits = hit->max_hits;
        gi.hoff = hit->hoff;
        gi.hit_pair = hit->hit_pair ? hit->hit_pair : reinterpret_cast<uint32_t *>(base + g.hit_at);
    }
    if (bt) {
        gi.req2 = base + g.req2_at;
        gi.pat2 = base + g.pat2_at;
        gi.txt2 = base + g.txt2_at;
    }
    gi.res = d_results;
    gi.ops = d_ops;
    gi.scratch = d_scratch;
    gi.scratch_bytes = g.plan_bytes;
    if (ref) {
        aim::gather_text_rows_launch(batch_args(*params, n_pairs, d_requests), d_text_pos_or_null, d_reference, ref_len, nullptr, n_pairs, gi.cand_t, stream);
        HIP_TRY(hipGetLastError());
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
