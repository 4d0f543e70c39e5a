// capi_pipeline.hip -- the read-mapping pipeline's entry points of the C-ABI (include/aim_hip.h): the k-mer / minimizer index on host and
// device, seeding and chaining, chain classes and MAPQ, split segments and their extension. Host code only: every kernel lives in its
// family's tu_*.hip and is reached through the launcher its header declares. What this unit shares with aim_capi.hip is in capi_common.hpp.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <thread>
#include <vector>

#include "capi_common.hpp"
#include "seed.hpp"
#include "seed_chain.hpp"
#include "seed_chain_long.hpp"
#include "chain_class.hpp"
#include "split.hpp"
#include "extend.hpp"
#include "index.hpp"

using namespace aim::capi;

namespace {

// ---------------------------------------------------------------------------
// device-side seeding (AIM_FEATURE_SEED; the rule is stated in aim_hip.h, the kernel in seed.hpp)
// ---------------------------------------------------------------------------
int check_index_args(int32_t k, uint64_t ref_len)
{
    if (k < 8 || k > 14) return fail(AIM_EINVAL, "seed index: k %d is outside 8..14", k);
    return ref_len_ok("seed index", ref_len, true) ? AIM_OK : AIM_EINVAL;
}

}  // namespace

// The bounds every seeding entry point sets (declared in capi_common.hpp).
int aim::capi::check_seed_params(const aim_seed_params_t &sp, int32_t max_read_size, const char *fn)
{
    if (sp.k < 8 || sp.k > 14) return fail(AIM_EINVAL, "aim_seed_params_t: k %d is outside 8..14", sp.k);
    if (sp.stride < 1) return fail(AIM_EINVAL, "aim_seed_params_t: stride %d must be >= 1", sp.stride);
    if (sp.max_occ < 1) return fail(AIM_EINVAL, "aim_seed_params_t: max_occ %d must be >= 1", sp.max_occ);
    if (sp.band < 0) return fail(AIM_EINVAL, "aim_seed_params_t: band %d must be >= 0", sp.band);
    if (sp.flank < 0) return fail(AIM_EINVAL, "aim_seed_params_t: flank %d must be >= 0", sp.flank);
    if (sp.min_votes < 1) return fail(AIM_EINVAL, "aim_seed_params_t: min_votes %d must be >= 1", sp.min_votes);
    if (sp.max_cands < 1 || sp.max_cands > AIM_SEED_MAX_CANDS)
        return fail(AIM_EINVAL, "aim_seed_params_t: max_cands %d is outside 1..%d", sp.max_cands, AIM_SEED_MAX_CANDS);
    if (sp.read_size <= 0 || (sp.read_size & 7) || sp.read_size > max_read_size)
        return fail(AIM_EINVAL, "aim_seed_params_t: read_size %d must be a positive multiple of 8, at most %d%s%s%s", sp.read_size, max_read_size,
                    fn ? " (" : "", fn ? fn : "", fn ? ")" : "");
    if (sp.options) {   // AIM_SEED_OPT_MINIMIZERS(w) and nothing else
        const uint32_t w = sp.options >> 8;
        if ((sp.options & 0xffu) || w < 1 || w > AIM_SEED_MAX_W) return fail(AIM_EINVAL, "aim_seed_params_t: unknown options 0x%x", sp.options);
        if (sp.stride != 1) return fail(AIM_EINVAL, "aim_seed_params_t: stride %d must be 1 with AIM_SEED_OPT_MINIMIZERS", sp.stride);
    }
    return AIM_OK;
}

int aim::capi::check_seed_chain_band(const aim_seed_params_t &sp, const char *fn)
{
    return sp.band > AIM_SEED_CHAIN_MAX_BAND ? fail(AIM_EINVAL, "aim_seed_params_t: band %d is above %d (%s)", sp.band, AIM_SEED_CHAIN_MAX_BAND, fn) : AIM_OK;
}

namespace {

int check_window(int32_t w) { return w < 1 || w > AIM_SEED_MAX_W ? fail(AIM_EINVAL, "seed index: w %d is outside 1..%d", w, AIM_SEED_MAX_W) : AIM_OK; }

// The rolling code of both scans takes in base c: it keeps the last k bases (top = 2 (k - 1)); `good` counts how many in a row were upper-case A C G T.
inline void roll_code(unsigned char c, int top, uint32_t &code, uint32_t &good)
{
    if (c == 'A' || c == 'C' || c == 'G' || c == 'T') code = (code >> 2) | ((uint32_t)((c >> 1) & 3) << top), ++good;
    else code = 0, good = 0;
}

// One pass of the index build over the whole sequence for the codes [c_lo, c_hi): `visit(code, p)` for every indexed k-mer of the range, p ascending.
template <typename F>
void index_scan(const char *seq, uint64_t len, int k, uint32_t c_lo, uint32_t c_hi, F visit)
{
    uint32_t code = 0, good = 0;
    const int top = 2 * (k - 1);
    for (uint64_t i = 0; i < len; ++i) {
        roll_code((unsigned char)seq[i], top, code, good);
        if (good >= (uint32_t)k && code >= c_lo && code < c_hi) visit(code, (uint32_t)(i + 1 - (uint64_t)k));
    }
}

// index_scan over the (w, k) minimizers alone (the rule in aim_hip.h, by its window definition): the windows slide with the scan, and a
// monotone queue of at most w candidates -- keys strictly ascending from its front, so the front is the window's leftmost smallest --
// names each window's minimizer. Those are ascending in p from window to window, so a position is visited once, when it first wins.
template <typename F>
void minimizer_scan(const char *seq, uint64_t len, int k, int w, uint32_t c_lo, uint32_t c_hi, F visit)
{
    if (len < (uint64_t)k) return;
    const uint64_t n = len - (uint64_t)k + 1u, full = std::min<uint64_t>((uint64_t)w, n);   // positions; positions in a window
    constexpr uint64_t invalid = 1ull << 32;                 // above every min_hash
    uint64_t q_key[AIM_SEED_MAX_W], q_pos[AIM_SEED_MAX_W];   // a ring: head, size
    uint32_t q_code[AIM_SEED_MAX_W];
    uint32_t head = 0, size = 0, code = 0, good = 0;
    uint64_t last = UINT64_MAX;
    const int top = 2 * (k - 1);
    for (uint64_t i = 0; i < len; ++i) {
        roll_code((unsigned char)seq[i], top, code, good);
        if (i + 1 < (uint64_t)k) continue;
        const uint64_t p = i + 1 - (uint64_t)k;              // the k-mer that ends here
        const uint64_t key = good >= (uint32_t)k ? aim::min_hash(code) : invalid;
        while (size && q_pos[head] + full <= p) head = (head + 1) % AIM_SEED_MAX_W, --size;   // the window is [p + 1 - full, p]: < w others remain
        while (size && q_key[(head + size - 1) % AIM_SEED_MAX_W] > key) --size;
        const uint32_t at = (head + size) % AIM_SEED_MAX_W;
        q_key[at] = key, q_pos[at] = p, q_code[at] = code;
        ++size;
        if (p + 1 < full) continue;                          // the first window is not complete yet
        if (q_key[head] != invalid && q_pos[head] != last) {
            last = q_pos[head];
            if (q_code[head] >= c_lo && q_code[head] < c_hi) visit(q_code[head], (uint32_t)last);
        }
    }
}

// The body of aim_index_build and aim_index_build_minimizers: a counting sort in two passes of `scan(lo, hi, visit)` per worker.
template <typename S>
int index_build_with(const char *seq, uint64_t ref_len, int32_t k, uint32_t *bucket, uint32_t *pos, uint64_t *n_pos, int threads, S scan)
{
    const bool any = ref_len >= (uint64_t)k;
    if (!bucket || (ref_len && !seq) || (any && !pos)) return fail(AIM_EINVAL, "seed index: NULL seq, bucket or pos");
    const uint64_t n_codes = 1ull << (2 * k);
    const int T = std::max(1, std::min(threads, 64));
    // every worker owns the codes [n_codes * t / T, n_codes * (t + 1) / T): its counts and, later, its runs of pos[] are its own
    auto range = [&](int t) { return (uint32_t)(n_codes * (uint64_t)t / (uint64_t)T); };
    auto run = [&](auto body) {
        std::vector<std::thread> th;
        for (int t = 1; t < T; ++t) th.emplace_back(body, t);
        body(0);
        for (auto &x : th) x.join();
    };
    // pass 1: counts, shifted by one so that the prefix sum below leaves bucket[c] = first entry of code c
    run([&](int t) {
        const uint32_t lo = range(t), hi = t + 1 == T ? (uint32_t)n_codes : range(t + 1);
        memset(bucket + (size_t)lo + 1, 0, (size_t)(hi - lo) * sizeof(uint32_t));
        if (any) scan(lo, hi, [&](uint32_t c, uint32_t) { ++bucket[(size_t)c + 1]; });
    });
    bucket[0] = 0;
    for (uint64_t c = 0; c < n_codes; ++c) bucket[c + 1] += bucket[c];
    const uint64_t total = bucket[n_codes];
    // pass 2: bucket[c] is code c's cursor; afterwards it holds bucket[c + 1], and one shift restores the prefix sums
    if (total) {
        run([&](int t) {
            const uint32_t lo = range(t), hi = t + 1 == T ? (uint32_t)n_codes : range(t + 1);
            scan(lo, hi, [&](uint32_t c, uint32_t p) { pos[bucket[c]++] = p; });
        });
        for (uint64_t c = n_codes; c > 0; --c) bucket[c] = bucket[c - 1];
        bucket[0] = 0;
    }
    if (n_pos) *n_pos = total;
    return AIM_OK;
}

// What the seeding entry points share once their parameters are checked: the checks on ref_len, the batch size and the device pointers,
// the device probe, the SeedArgs `a` (inside the entry point's zeroed argument struct) with the poison knobs, the persistent grid and the
// plan line, which ends in plan_tail. launch(grid) starts `kernel`, whose workgroups take `lds` bytes each.
template <typename Launch>
int seed_submit(const char *fn, const char *kernel, const char *plan_tail, aim::SeedArgs &a, size_t lds, const aim_seed_params_t *sp, uint32_t n_reads,
                const int32_t *d_read_len, const char *d_reads, const uint32_t *d_bucket, const uint32_t *d_pos, uint64_t ref_len, void *d_requests,
                uint64_t *d_text_pos, uint32_t *d_votes, aim_seed_t *d_seed, Launch launch)
{
    if (!(ref_len_ok(fn, ref_len, true) && slots_ok(fn, n_reads, (uint32_t)sp->max_cands, "max_cands") &&
          buffers_ok(fn, n_reads, d_read_len && d_reads && d_bucket && (d_pos || ref_len < (uint64_t)sp->k) && d_requests && d_text_pos && d_votes && d_seed)))
        return AIM_EINVAL;
    return launch_batch(n_reads, [&](const aim::Knobs &kn) {
        a.sp = *sp; a.n_reads = n_reads; a.read_len = d_read_len; a.reads = d_reads;
        a.bucket = d_bucket; a.pos = d_pos; a.ref_len = ref_len;
        a.req = static_cast<aim_request_t *>(d_requests); a.text_pos = d_text_pos; a.votes = d_votes; a.seed = d_seed;
        a.dbg_poison_lds = poison_lds_word(kn); a.dbg_lds_bytes = (uint32_t)lds;
        // persistent grid: what LDS lets one CU hold (at most 16 wavefronts), on every CU, capped at the reads rounded up to the multiple of 8
        // xcd_unit needs (below 8 reads the surplus workgroups find no work and leave)
        const uint32_t per_cu = (uint32_t)std::min<size_t>(16, aim::lds_workgroups_per_cu(lds));
        const uint32_t grid = std::min(aim::resident_grid(kn, per_cu), (uint32_t)std::min<uint64_t>(((uint64_t)n_reads + 7u) & ~7ull, 1u << 20));
        if (kn.plan_debug) fprintf(stderr, "[aim plan] %s grid=%u block=64 lds=%zu per_cu=%u reads=%u%s\n", kernel, grid, lds, per_cu, n_reads, plan_tail);
        launch(grid);
    });
}

// aim_seed_device (chain = false) and aim_seed_chain_device (chain = true: the chaining kernels, the band bound and d_chains)
int seed_device(const char *fn, bool chain, const aim_seed_params_t *sp, uint32_t n_reads, const int32_t *d_read_len, const char *d_reads,
                const uint32_t *d_bucket, const uint32_t *d_pos, uint64_t ref_len, void *d_requests, uint64_t *d_text_pos, uint32_t *d_votes,
                aim_seed_t *d_seed, aim_chain_t *d_chains, void *hip_stream)
{
    if (!sp) return fail(AIM_EINVAL, "%s: sp is NULL", fn);
    if (const int rc = check_seed_params(*sp)) return rc;
    if (chain)
        if (const int rc = check_seed_chain_band(*sp, fn)) return rc;
    aim::SeedChainArgs ca;
    memset(&ca, 0, sizeof ca);
    ca.chains = d_chains;
    const bool minimizers = sp->options != 0;
    const size_t lds = chain ? (minimizers ? aim::seed_chain_minimizer_lds_bytes(sp->read_size) : aim::seed_chain_lds_bytes(sp->read_size))
                             : (minimizers ? aim::seed_minimizer_lds_bytes(sp->read_size) : aim::seed_lds_bytes(sp->read_size));
    const char *kernel = chain ? (minimizers ? "seed_chain_minimizer_kernel" : "seed_chain_kernel") : (minimizers ? "seed_minimizer_kernel" : "seed_candidates_kernel");
    return seed_submit(fn, kernel, "", ca.s, lds, sp, n_reads, d_read_len, d_reads, d_bucket, d_pos, ref_len, d_requests, d_text_pos, d_votes, d_seed,
                       [&](uint32_t grid) {
                           if (chain)
                               aim::seed_chain_launch(ca, minimizers, grid, lds, (hipStream_t)hip_stream);
                           else if (minimizers)
                               aim::seed_minimizer_launch(ca.s, grid, lds, (hipStream_t)hip_stream);
                           else
                               aim::seed_launch(ca.s, grid, lds, (hipStream_t)hip_stream);
                       });
}

}  // namespace

// aim_seed_chain_long_device's parameter check: check_seed_params with the long read_size bound, then what is its own -- minimizers
// required, the band bound and the hit cap.
int aim::capi::check_seed_long_params(const aim_seed_params_t &sp, uint32_t max_hits)
{
    if (const int rc = check_seed_params(sp, AIM_SEED_LONG_MAX_READ_SIZE, "aim_seed_chain_long_device")) return rc;
    if (!sp.options)
        return fail(AIM_EINVAL, "aim_seed_params_t: options 0x0 must be AIM_SEED_OPT_MINIMIZERS(w) (aim_seed_chain_long_device takes minimizer seeds only)");
    if (sp.band > AIM_SEED_CHAIN_MAX_BAND)
        return fail(AIM_EINVAL, "aim_seed_params_t: band %d is above %d (aim_seed_chain_long_device)", sp.band, AIM_SEED_CHAIN_MAX_BAND);
    if (max_hits < AIM_SEED_MAX_HITS || max_hits > AIM_SEED_LONG_MAX_HITS || (max_hits & (max_hits - 1u)))
        return fail(AIM_EINVAL, "aim_seed_chain_long_device: max_hits %u must be a power of two in %d..%d", max_hits, AIM_SEED_MAX_HITS, AIM_SEED_LONG_MAX_HITS);
    return AIM_OK;
}

int aim::capi::check_extend_params(const char *fn, const aim_extend_params_t *p)
{
    if (!p) return fail(AIM_EINVAL, "%s: NULL parameters", fn);
    if (p->match < 1) return fail(AIM_EINVAL, "%s: match %d must be >= 1", fn, p->match);
    if (p->mismatch < 1) return fail(AIM_EINVAL, "%s: mismatch %d must be >= 1", fn, p->mismatch);
    if (p->gap_o < 0) return fail(AIM_EINVAL, "%s: gap_o %d must be >= 0", fn, p->gap_o);
    if (p->gap_e < 1) return fail(AIM_EINVAL, "%s: gap_e %d must be >= 1", fn, p->gap_e);
    if (p->xdrop < 0) return fail(AIM_EINVAL, "%s: xdrop %d must be >= 0", fn, p->xdrop);
    if (p->max_cost < 1 || p->max_cost > AIM_EXTEND_MAX_COST) return fail(AIM_EINVAL, "%s: max_cost %d is outside 1..%d", fn, p->max_cost, AIM_EXTEND_MAX_COST);
    if (p->band < 1 || p->band > AIM_EXTEND_MAX_BAND) return fail(AIM_EINVAL, "%s: band %d is outside 1..%d", fn, p->band, AIM_EXTEND_MAX_BAND);
    if (p->max_ext < 8 || p->max_ext > AIM_EXTEND_MAX_EXT) return fail(AIM_EINVAL, "%s: max_ext %d is outside 8..%d", fn, p->max_ext, AIM_EXTEND_MAX_EXT);
    const int64_t unit = std::max<int64_t>(2 * ((int64_t)p->match + p->mismatch), 2 * (int64_t)p->gap_o + 2 * (int64_t)p->gap_e + p->match);   // (64-bit: the sums of any accepted fields fit)
    if (unit > AIM_EXTEND_MAX_UNIT)
        return fail(AIM_EINVAL, "%s: max(x', o' + e') = %lld is above %d (x' = 2 (match + mismatch), o' + e' = 2 gap_o + 2 gap_e + match)", fn, (long long)unit, AIM_EXTEND_MAX_UNIT);
    return AIM_OK;
}

namespace {

// aim_index_build_device (w = 0: index_code_kernel) and aim_index_build_device_minimizers (w >= 1: index_minimizer_kernel in its place)
int index_build_device(const char *d_reference, uint64_t ref_len, int32_t k, int32_t w, uint32_t *d_bucket, uint32_t *d_pos, void *d_scratch,
                       uint64_t scratch_bytes, void *hip_stream)
{
    if (const int rc = check_index_args(k, ref_len)) return rc;
    const aim::IndexLayout L = aim::index_layout(k, ref_len);
    if (!d_bucket) return fail(AIM_EINVAL, "aim_index_build_device: d_bucket is NULL");
    if (L.n) {
        if (!d_reference) return fail(AIM_EINVAL, "aim_index_build_device: d_reference is NULL");
        if ((uintptr_t)d_reference & 15u) return fail(AIM_EINVAL, "aim_index_build_device: d_reference is not 16-byte aligned");
        if (!d_pos) return fail(AIM_EINVAL, "aim_index_build_device: d_pos is NULL (ref_len %llu >= k %d)", (unsigned long long)ref_len, k);
        if (!d_scratch) return fail(AIM_EINVAL, "aim_index_build_device: d_scratch is NULL (%llu bytes are needed)", (unsigned long long)L.total);
        if ((uintptr_t)d_scratch & 255u) return fail(AIM_EINVAL, "aim_index_build_device: d_scratch is not 256-byte aligned");
        if (scratch_bytes < L.total)
            return fail(AIM_EINVAL, "aim_index_build_device: scratch_bytes %llu is below the %llu aim_index_device_scratch reports",
                        (unsigned long long)scratch_bytes, (unsigned long long)L.total);
    }
    int n_dev = 0;
    if (const int rc = aim_device_count(&n_dev)) return rc;
    hipStream_t stream = (hipStream_t)hip_stream;
    const aim::Knobs kn = with_chip(read_knobs());
    const uint64_t n_codes = 1ull << (2 * k);
    if (kn.plan_debug) fprintf(stderr, "[aim plan] index memset bucket bytes=%llu\n", (unsigned long long)((n_codes + 1u) * 4u));
    HIP_TRY(hipMemsetAsync(d_bucket, 0, (size_t)(n_codes + 1u) * sizeof(uint32_t), stream));
    if (!L.n) return AIM_OK;
    char *scr = static_cast<char *>(d_scratch);
    // Debugging aid, as for the alignment scratch: results must not depend on what the scratch held before.
    if (kn.poison_scratch >= 0) HIP_TRY(hipMemsetAsync(scr, kn.poison_scratch & 0xff, (size_t)L.total, stream));
    uint32_t *keys[2] = {reinterpret_cast<uint32_t *>(scr + L.key_a), reinterpret_cast<uint32_t *>(scr + L.key_b)};
    uint32_t *pos_s = reinterpret_cast<uint32_t *>(scr + L.pos_s);
    const uint32_t poison_lds = poison_lds_word(kn);
    // persistent grids: 8 workgroups of 256 threads per CU (index.hpp OCCUPANCY), never more than there are tiles / scan parts
    const uint32_t resident = aim::resident_grid(kn, 8);
    const uint32_t grid = std::min(resident, L.n_tiles);
    auto scan = [&](uint32_t *data, uint64_t n, const char *what) {
        aim::IndexScanArgs s;
        memset(&s, 0, sizeof s);
        s.data = data; s.n = n; s.dbg_poison_lds = poison_lds; s.part = reinterpret_cast<uint32_t *>(scr + L.parts);
        s.n_parts = (uint32_t)std::min<uint64_t>(std::min(resident, aim::kIndexScanParts), (n + aim::kIndexScanBlock - 1u) / aim::kIndexScanBlock);
        s.per_part = ((n + s.n_parts - 1u) / s.n_parts + aim::kIndexScanBlock - 1u) / aim::kIndexScanBlock * aim::kIndexScanBlock;
        if (kn.plan_debug) {
            fprintf(stderr, "[aim plan] index_scan_sums_kernel grid=%u block=%d %s entries=%llu per_part=%llu\n", s.n_parts, aim::kIndexThreads, what,
                    (unsigned long long)n, (unsigned long long)s.per_part);
            fprintf(stderr, "[aim plan] index_scan_top_kernel grid=1 block=%d %s parts=%u\n", aim::kIndexThreads, what, s.n_parts);
            fprintf(stderr, "[aim plan] index_scan_apply_kernel grid=%u block=%d %s entries=%llu per_part=%llu\n", s.n_parts, aim::kIndexThreads, what,
                    (unsigned long long)n, (unsigned long long)s.per_part);
        }
        aim::index_launch_scan(s, stream);
    };
    aim::IndexArgs a;
    memset(&a, 0, sizeof a);
    a.ref = d_reference; a.ref_len = ref_len; a.k = k; a.w = w; a.n = L.n; a.n_tiles = L.n_tiles;
    a.table = reinterpret_cast<uint32_t *>(scr + L.table); a.bucket = d_bucket; a.key_out = keys[0];
    a.dbg_poison_lds = poison_lds;
    if (w) {   // 7 workgroups per CU: what its LDS allows (index.hpp)
        const uint32_t grid_m = std::min(aim::resident_grid(kn, 7), L.n_tiles);
        if (kn.plan_debug)
            fprintf(stderr, "[aim plan] index_minimizer_kernel grid=%u block=%d k=%d w=%d positions=%llu tiles=%u\n", grid_m, aim::kIndexThreads, k, w,
                    (unsigned long long)L.n, L.n_tiles);
        aim::index_launch_minimizer(a, grid_m, stream);
    } else {
        if (kn.plan_debug)
            fprintf(stderr, "[aim plan] index_code_kernel grid=%u block=%d k=%d positions=%llu tiles=%u\n", grid, aim::kIndexThreads, k, (unsigned long long)L.n, L.n_tiles);
        aim::index_launch_code(a, grid, stream);
    }
    HIP_TRY(hipGetLastError());
    scan(d_bucket, n_codes + 1u, "bucket");
    HIP_TRY(hipGetLastError());
    // pass p reads what pass p - 1 wrote; the positions alternate between d_pos and the scratch array so that the last pass lands in d_pos
    const int passes = aim::index_passes(k);
    for (int p = 0; p < passes; ++p) {
        const bool last = p + 1 == passes;
        auto pos_of = [&](int q) { return ((passes - 1 - q) & 1) ? pos_s : d_pos; };
        a.shift = (uint32_t)(8 * p);
        a.key_in = keys[p & 1];
        a.key_out = last ? nullptr : keys[(p + 1) & 1];
        a.pos_in = p ? pos_of(p - 1) : nullptr;
        a.pos_out = pos_of(p);
        if (kn.plan_debug) fprintf(stderr, "[aim plan] index_hist_kernel grid=%u block=%d pass=%d/%d shift=%u\n", grid, aim::kIndexThreads, p + 1, passes, a.shift);
        aim::index_launch_hist(a, grid, stream);
        HIP_TRY(hipGetLastError());
        scan(a.table, (uint64_t)aim::kIndexDigits * L.n_tiles, "table");
        HIP_TRY(hipGetLastError());
        if (kn.plan_debug)
            fprintf(stderr, "[aim plan] index_scatter_kernel grid=%u block=%d pass=%d/%d shift=%u keys_out=%d\n", grid, aim::kIndexThreads, p + 1, passes, a.shift, last ? 0 : 1);
        aim::index_launch_scatter(a, grid, stream);
        HIP_TRY(hipGetLastError());
    }
    return AIM_OK;
}

}  // namespace

extern "C" {

int aim_index_sizes(int32_t k, uint64_t ref_len, uint64_t *bucket_entries, uint64_t *pos_capacity)
{
    if (const int rc = check_index_args(k, ref_len)) return rc;
    if (!bucket_entries || !pos_capacity) return fail(AIM_EINVAL, "seed index: NULL output pointer");
    *bucket_entries = (1ull << (2 * k)) + 1u;
    *pos_capacity = ref_len >= (uint64_t)k ? ref_len - (uint64_t)k + 1u : 0u;
    return AIM_OK;
}

int aim_index_build(const char *seq, uint64_t ref_len, int32_t k, uint32_t *bucket, uint32_t *pos, uint64_t *n_pos, int threads)
{
    if (const int rc = check_index_args(k, ref_len)) return rc;
    return index_build_with(seq, ref_len, k, bucket, pos, n_pos, threads,
                            [&](uint32_t lo, uint32_t hi, auto visit) { index_scan(seq, ref_len, k, lo, hi, visit); });
}

int aim_index_build_minimizers(const char *seq, uint64_t ref_len, int32_t k, int32_t w, uint32_t *bucket, uint32_t *pos, uint64_t *n_pos, int threads)
{
    int rc = check_index_args(k, ref_len);
    if (!rc) rc = check_window(w);
    if (rc) return rc;
    return index_build_with(seq, ref_len, k, bucket, pos, n_pos, threads,
                            [&](uint32_t lo, uint32_t hi, auto visit) { minimizer_scan(seq, ref_len, k, w, lo, hi, visit); });
}

int aim_seed_groups_offsets(uint32_t n_reads, uint32_t K, uint32_t *read_offsets)
{
    if (!cands_ok("aim_seed_groups_offsets", K)) return AIM_EINVAL;
    if (!read_offsets) return fail(AIM_EINVAL, "aim_seed_groups_offsets: NULL read_offsets");
    if ((uint64_t)n_reads * K >= (1ull << 32)) return fail(AIM_EINVAL, "aim_seed_groups_offsets: n_reads %u * K %u does not fit 32 bits", n_reads, K);
    for (uint64_t r = 0; r <= n_reads; ++r) read_offsets[r] = (uint32_t)(r * K);
    return AIM_OK;
}

const char *aim_seed_kernel_name(void) { return "seed_candidates_kernel"; }

int aim_seed_device(const aim_seed_params_t *sp, uint32_t n_reads, const int32_t *d_read_len, const char *d_reads, const uint32_t *d_bucket,
                    const uint32_t *d_pos, uint64_t ref_len, void *d_requests, uint64_t *d_text_pos, uint32_t *d_votes, aim_seed_t *d_seed,
                    void *hip_stream)
{
    return seed_device("aim_seed_device", false, sp, n_reads, d_read_len, d_reads, d_bucket, d_pos, ref_len, d_requests, d_text_pos, d_votes, d_seed,
                       nullptr, hip_stream);
}

const char *aim_seed_chain_kernel_names(void) { return "seed_chain_kernel,seed_chain_minimizer_kernel"; }

int aim_seed_chain_device(const aim_seed_params_t *sp, uint32_t n_reads, const int32_t *d_read_len, const char *d_reads, const uint32_t *d_bucket,
                          const uint32_t *d_pos, uint64_t ref_len, void *d_requests, uint64_t *d_text_pos, uint32_t *d_votes, aim_seed_t *d_seed,
                          aim_chain_t *d_chains_or_null, void *hip_stream)
{
    return seed_device("aim_seed_chain_device", true, sp, n_reads, d_read_len, d_reads, d_bucket, d_pos, ref_len, d_requests, d_text_pos, d_votes,
                       d_seed, d_chains_or_null, hip_stream);
}

const char *aim_seed_chain_long_kernel_name(void) { return "seed_chain_long_kernel"; }

// aim_seed_chain_device for long reads (AIM_FEATURE_SEED_CHAIN_LONG; the kernel in seed_chain_long.hpp): seed_device()'s order of checks
// and its grid, with the hit cap H deciding the LDS and with it the workgroups per CU.
int aim_seed_chain_long_device(const aim_seed_params_t *sp, uint32_t max_hits, uint32_t n_reads, const int32_t *d_read_len, const char *d_reads,
                               const uint32_t *d_bucket, const uint32_t *d_pos, uint64_t ref_len, void *d_requests, uint64_t *d_text_pos, uint32_t *d_votes,
                               aim_seed_t *d_seed, aim_chain_t *d_chains_or_null, void *hip_stream)
{
    const char *fn = "aim_seed_chain_long_device";
    if (!sp) return fail(AIM_EINVAL, "%s: sp is NULL", fn);
    if (const int rc = check_seed_long_params(*sp, max_hits)) return rc;
    aim::SeedChainLongArgs la;
    memset(&la, 0, sizeof la);
    la.c.chains = d_chains_or_null;
    la.max_hits = max_hits;
    const size_t lds = aim::seed_chain_long_lds_bytes(max_hits);
    char plan_tail[48];
    snprintf(plan_tail, sizeof plan_tail, " max_hits=%u tile=%u", max_hits, aim::kSeedLongTile);
    return seed_submit(fn, "seed_chain_long_kernel", plan_tail, la.c.s, lds, sp, n_reads, d_read_len, d_reads, d_bucket, d_pos, ref_len, d_requests,
                       d_text_pos, d_votes, d_seed, [&](uint32_t grid) { aim::seed_chain_long_launch(la, grid, lds, (hipStream_t)hip_stream); });
}

// ---------------------------------------------------------------------------
// primary / secondary chains and MAPQ (AIM_FEATURE_CHAIN_CLASS; rules 8c and 9c in aim_hip.h, the kernels in chain_class.hpp)
// ---------------------------------------------------------------------------
const char *aim_chain_class_kernel_names(void) { return "chain_class_kernel,read_mapq_kernel"; }

int aim_chain_classify_device(uint32_t K, uint32_t read_size, uint32_t mask_q8, uint32_t n_reads, const int32_t *d_read_len, const uint64_t *d_text_pos,
                              const aim_seed_t *d_seed, const aim_chain_t *d_chains, aim_chain_class_t *d_class, void *hip_stream)
{
    const char *fn = "aim_chain_classify_device";
    if (!(cands_ok(fn, K) && ((mask_q8 >= 1 && mask_q8 <= 256) || refuse("%s: mask_q8 %u is outside 1..256", fn, mask_q8)) && read_size_ok(fn, read_size) &&
          slots_ok(fn, n_reads, K) && buffers_ok(fn, n_reads, d_read_len && d_text_pos && d_seed && d_chains && d_class)))
        return AIM_EINVAL;
    return launch_batch(n_reads, [&](const aim::Knobs &kn) {
        const aim::ChainClassArgs a = {K, read_size, mask_q8, n_reads, d_read_len, d_text_pos, d_seed, d_chains, d_class};
        // lanes per read: the smallest group that holds K; AIM_CLASS_G widens it for A/B runs (the rows do not depend on it)
        uint32_t lanes = aim::chain_class_lanes(K);
        if ((kn.class_g == 8 || kn.class_g == 16) && (uint32_t)kn.class_g > lanes) lanes = (uint32_t)kn.class_g;
        const uint32_t per_block = aim::kChainClassThreads / lanes;
        const uint32_t grid = (uint32_t)std::min<uint64_t>(aim::resident_grid(kn, aim::kChainClassPerCu), ((uint64_t)n_reads + per_block - 1u) / per_block);
        if (kn.plan_debug) fprintf(stderr, "[aim plan] chain_class_kernel grid=%u block=%d lanes=%u reads=%u K=%u mask_q8=%u\n", grid, aim::kChainClassThreads, lanes, n_reads, K, mask_q8);
        aim::chain_class_launch(a, lanes, grid, (hipStream_t)hip_stream);
    });
}

int aim_read_mapq_device(uint32_t K, uint32_t n_reads, int32_t score_unit, const aim_best_t *d_best, const aim_mate_t *d_mates_or_null,
                         const aim_chain_class_t *d_class, aim_read_mapq_t *d_mapq, void *hip_stream)
{
    const char *fn = "aim_read_mapq_device";
    if (!(cands_ok(fn, K) && slots_ok(fn, n_reads, K) && (score_unit >= 1 || refuse("%s: score_unit %d must be >= 1", fn, score_unit)) &&
          (!d_mates_or_null || !(n_reads & 1u) || refuse("%s: n_reads %u is odd with d_mates (reads 2m and 2m + 1 are mates)", fn, n_reads)) &&
          buffers_ok(fn, n_reads, d_best && d_class && d_mapq)))
        return AIM_EINVAL;
    return launch_batch(n_reads, [&](const aim::Knobs &kn) {
        const aim::ReadMapqArgs a = {K, n_reads, score_unit, d_best, d_mates_or_null, d_class, d_mapq};
        const uint32_t grid =
            (uint32_t)std::min<uint64_t>(aim::resident_grid(kn, aim::kChainClassPerCu), ((uint64_t)n_reads + aim::kChainClassThreads - 1u) / aim::kChainClassThreads);
        if (kn.plan_debug)
            fprintf(stderr, "[aim plan] read_mapq_kernel grid=%u block=%d reads=%u K=%u score_unit=%d mates=%d\n", grid, aim::kChainClassThreads, n_reads, K, score_unit,
                    d_mates_or_null ? 1 : 0);
        aim::read_mapq_launch(a, grid, (hipStream_t)hip_stream);
    });
}

// ---------------------------------------------------------------------------
// split reads (AIM_FEATURE_SPLIT; rule 10c in aim_hip.h, the kernel in split.hpp; aim_sam_device_split stands next to aim_sam_device)
// ---------------------------------------------------------------------------
const char *aim_split_kernel_names(void) { return "split_segments_kernel,sam_lane_split_kernel,sam_wave_split_kernel"; }

int aim_split_segments_device(uint32_t K, uint32_t read_size, int32_t flank, uint64_t ref_len, uint32_t n_reads, const int32_t *d_read_len, const char *d_reads,
                              const void *d_requests, const uint64_t *d_text_pos, const aim_seed_t *d_seed, const aim_chain_t *d_chains,
                              const aim_chain_class_t *d_class, void *d_seg_requests, uint64_t *d_seg_text_pos, char *d_seg_patterns, aim_segment_t *d_seg,
                              void *hip_stream)
{
    const char *fn = "aim_split_segments_device";
    if (!(cands_ok(fn, K) && read_size_ok(fn, read_size) && slots_ok(fn, n_reads, K) && (flank >= 0 || refuse("%s: flank %d must be >= 0", fn, flank)) &&
          ref_len_ok(fn, ref_len, false) &&
          buffers_ok(fn, n_reads, d_read_len && d_reads && d_requests && d_text_pos && d_seed && d_chains && d_class && d_seg_requests && d_seg_text_pos && d_seg_patterns && d_seg)))
        return AIM_EINVAL;
    return launch_batch(n_reads, [&](const aim::Knobs &kn) {
        aim::SplitArgs a;
        memset(&a, 0, sizeof a);
        a.K = K; a.read_size = read_size; a.n_reads = n_reads; a.parts_log2 = aim::split_parts_log2(K, read_size);
        a.flank = flank; a.ref_len = (int64_t)ref_len;
        a.read_len = d_read_len; a.reads = d_reads; a.requests = static_cast<const aim_request_t *>(d_requests); a.text_pos = d_text_pos;
        a.seed = d_seed; a.chains = d_chains; a.cls = d_class;
        a.seg_requests = static_cast<aim_request_t *>(d_seg_requests); a.seg_text_pos = d_seg_text_pos; a.seg_patterns = d_seg_patterns; a.seg = d_seg;
        // lanes per read and shares per read come from K and read_size alone; only the grid is the device's
        const uint32_t lanes = aim::split_lanes(read_size);
        const uint32_t per_block = aim::kSplitThreads / lanes;
        const uint64_t items = (uint64_t)n_reads << a.parts_log2;
        const uint32_t grid = (uint32_t)std::min<uint64_t>(aim::resident_grid(kn, aim::kSplitPerCu), (items + per_block - 1u) / per_block);
        if (kn.plan_debug)
            fprintf(stderr, "[aim plan] split_segments_kernel grid=%u block=%d lanes=%u parts=%u reads=%u K=%u read_size=%u\n", grid, aim::kSplitThreads, lanes,
                    1u << a.parts_log2, n_reads, K, read_size);
        aim::split_segments_launch(a, lanes, grid, (hipStream_t)hip_stream);
    });
}

// ---------------------------------------------------------------------------
// segment extension (AIM_FEATURE_EXTEND; rule 11c in aim_hip.h, the kernels in extend.hpp)
// ---------------------------------------------------------------------------
const char *aim_extend_kernel_names(void) { return "extend_sides_kernel,extend_apply_kernel"; }

int aim_extend_segments_device(const aim_extend_params_t *p, uint32_t K, uint32_t read_size, uint64_t ref_len, uint32_t n_reads, const int32_t *d_read_len,
                               const char *d_reads, const char *d_reference, void *d_seg_requests, uint64_t *d_seg_text_pos, char *d_seg_patterns,
                               aim_segment_t *d_seg, aim_extend_t *d_ext, void *hip_stream)
{
    const char *fn = "aim_extend_segments_device";
    if (!(cands_ok(fn, K) && read_size_ok(fn, read_size) && slots_ok(fn, n_reads, K))) return AIM_EINVAL;
    if (const int rc = check_extend_params(fn, p)) return rc;
    if (!(ref_len_ok(fn, ref_len, false) && buffers_ok(fn, n_reads, d_read_len && d_reads && d_reference && d_seg_requests && d_seg_text_pos && d_seg_patterns && d_seg && d_ext)))
        return AIM_EINVAL;
    return launch_batch(n_reads, [&](const aim::Knobs &kn) {
        aim::ExtendArgs a;
        memset(&a, 0, sizeof a);
        aim::extend_plan(*p, a);
        a.K = K; a.read_size = read_size; a.n_reads = n_reads; a.ref_len = (int64_t)ref_len;
        a.dbg_poison_lds = poison_lds_word(kn);
        a.read_len = d_read_len; a.reads = d_reads; a.ref = d_reference;
        a.seg_requests = static_cast<aim_request_t *>(d_seg_requests); a.seg_text_pos = d_seg_text_pos; a.seg_patterns = d_seg_patterns; a.seg = d_seg;
        a.ext = d_ext;
        // the items of a wavefront and the LDS of a side come from the parameters alone; only the grids are the device's
        const uint64_t slots = (uint64_t)n_reads * K;
        const uint32_t per_cu = std::min<uint32_t>(32u, std::max<uint32_t>(1u, aim::kExtendLdsPerCu / a.lds_bytes));
        const uint32_t grid_sides = (uint32_t)std::min<uint64_t>(aim::resident_grid(kn, per_cu), (2u * slots + 63u) / 64u);
        const uint32_t per_block = 64u * (aim::kExtendApplyThreads / 64u);
        const uint32_t grid_apply = (uint32_t)std::min<uint64_t>(aim::resident_grid(kn, aim::kExtendApplyPerCu), (slots + per_block - 1u) / per_block);
        if (kn.plan_debug)
            fprintf(stderr, "[aim plan] extend_sides_kernel grid=%u block=%d lds=%u step=%d rings=%u+2*%u reads=%u K=%u read_size=%u; extend_apply_kernel grid=%u block=%d\n",
                    grid_sides, aim::kExtendThreads, a.lds_bytes, a.g, a.dm, a.di, n_reads, K, read_size, grid_apply, aim::kExtendApplyThreads);
        aim::extend_launch(a, grid_sides, grid_apply, (hipStream_t)hip_stream);
    });
}

// ---------------------------------------------------------------------------
// the index built on the device (AIM_FEATURE_INDEX_DEVICE; the kernels and the scratch layout in index.hpp)
// ---------------------------------------------------------------------------
int aim_index_device_scratch(int32_t k, uint64_t ref_len, uint64_t *scratch_bytes)
{
    if (const int rc = check_index_args(k, ref_len)) return rc;
    if (!scratch_bytes) return fail(AIM_EINVAL, "seed index: NULL output pointer");
    *scratch_bytes = aim::index_layout(k, ref_len).total;
    return AIM_OK;
}

const char *aim_index_kernel_names(void) { return "index_code_kernel,index_scan_sums_kernel,index_scan_top_kernel,index_scan_apply_kernel,index_hist_kernel,index_scatter_kernel"; }

const char *aim_minimizer_kernel_names(void) { return "index_minimizer_kernel,seed_minimizer_kernel"; }

int aim_index_build_device(const char *d_reference, uint64_t ref_len, int32_t k, uint32_t *d_bucket, uint32_t *d_pos, void *d_scratch,
                           uint64_t scratch_bytes, void *hip_stream)
{
    return index_build_device(d_reference, ref_len, k, 0, d_bucket, d_pos, d_scratch, scratch_bytes, hip_stream);
}

int aim_index_build_device_minimizers(const char *d_reference, uint64_t ref_len, int32_t k, int32_t w, uint32_t *d_bucket, uint32_t *d_pos,
                                      void *d_scratch, uint64_t scratch_bytes, void *hip_stream)
{
    if (const int rc = check_window(w)) return rc;
    return index_build_device(d_reference, ref_len, k, w, d_bucket, d_pos, d_scratch, scratch_bytes, hip_stream);
}

}  // extern "C"
