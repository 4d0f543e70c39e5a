// capi_mapper.hip -- the top layer of the read-mapping pipeline (include/aim_hip.h, AIM_FEATURE_MAPPER): rule 12c's entry point
// aim_map_records_device (kernels in mapper.hpp, the prefix sums by index.hpp's scan) and aim_mapper_t, which owns the reference, the
// index and per-slot buffers and streams and runs the stages of capi_pipeline.hip and aim_capi.hip through their public entry points.
// Rule 13c (AIM_FEATURE_CONTIGS) lives here too: the contig layout, aim_contig_clip_device (kernel in contig.hpp),
// aim_map_records_contigs_device and the mapper of a reference of several sequences.
// Rule 16c's mapper side (AIM_FEATURE_SECONDARY: aim_mapper_set_secondary, aim_mapper_secondary) is here as well; its stateless entry points
// are in capi_secondary.hip.
// Host code only. What this unit shares with the others is in capi_common.hpp.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "capi_common.hpp"
#include "contig.hpp"
#include "index.hpp"
#include "mapper.hpp"
#include "secondary.hpp"

using namespace aim::capi;

namespace {

constexpr size_t kMapScratch = 4u * aim::kIndexScanParts;   // the scan's part sums

// The message a stage's own check left, under the mapper entry point's name.
int under(const char *fn, int rc)
{
    const std::string was = aim_last_error();
    return fail(rc, "%s: %s", fn, was.c_str());
}

// The segment alignment of the mapper: global-in-the-read, free text ends of 2 * flank, CIGAR, windows of the resident reference.
aim_endsfree_params_t align_params(const aim_mapper_params_t &p)
{
    aim_endsfree_params_t e;
    memset(&e, 0, sizeof e);
    e.base.algo = AIM_ALGO_WFA;
    e.base.match = p.match; e.base.mismatch = p.mismatch; e.base.gap_o = p.gap_o; e.base.gap_e = p.gap_e;
    e.base.max_score = p.max_score;
    e.base.read_size = p.seed.read_size;
    e.base.flags = AIM_FLAG_BACKTRACE | AIM_FLAG_ENDSFREE | AIM_FLAG_REF_TEXTS;
    e.text_begin_free = e.text_end_free = 2 * p.seed.flank;
    return e;
}

// Rule 14c's rescue alignment: the segment alignment at read_size = rescue_size, with the whole window free at either end.
aim_endsfree_params_t rescue_params(const aim_mapper_params_t &p, const aim_map_pair_params_t &pp)
{
    aim_endsfree_params_t e = align_params(p);
    e.base.read_size = (int32_t)pp.rescue_size;
    e.text_begin_free = e.text_end_free = (int32_t)pp.rescue_size;
    return e;
}

// Every refusal of aim_mapper_pairing_device_bytes and aim_mapper_set_pairing behind the NULL checks; no device is asked anything.
int check_pairing(const char *fn, const aim_mapper_params_t &p, const aim_map_pair_params_t *pp)
{
    if (const int rc = check_pair_params(fn, pp, (uint32_t)p.seed.max_cands, (uint32_t)p.seed.read_size, 0, false)) return rc;
    if ((uint64_t)p.max_reads * ((uint64_t)p.seed.max_cands + 1u) >= (1ull << 32))
        return fail(AIM_EINVAL, "%s: max_reads %u * (K %d + 1) does not fit 32 bits", fn, p.max_reads, p.seed.max_cands);
    if (pp->options & AIM_PAIR_RESCUE) {
        if (pp->rescue_size > (uint32_t)INT32_MAX) return fail(AIM_EINVAL, "%s: rescue_size %u is above INT32_MAX", fn, pp->rescue_size);
        const aim_endsfree_params_t rap = rescue_params(p, *pp);
        if (check_align_params(rap.base)) return under(fn, AIM_EINVAL);
        if ((uint64_t)p.max_reads * (4ull * pp->rescue_size + 10ull) >= (1ull << 32))
            return fail(AIM_EINVAL, "%s: max_reads %u rows of rescue_size %u exceed the 32-bit offsets of aim_sam_t (max_reads * (4 * rescue_size + 10) must stay below 2^32)",
                        fn, p.max_reads, pp->rescue_size);
    }
    if ((uint64_t)p.cigar_cap + pp->rescue_cigar_cap >= (1ull << 32) || (uint64_t)p.md_cap + pp->rescue_md_cap >= (1ull << 32))
        return fail(AIM_EINVAL, "%s: cigar_cap + rescue_cigar_cap and md_cap + rescue_md_cap must stay below 2^32", fn);
    return AIM_OK;
}

// The refusals of rule 16c's aim_map_sec_params_t, under the name `fn`; no device is asked anything.
int check_secondary(const char *fn, const aim_map_sec_params_t *sp)
{
    if (!sp) return fail(AIM_EINVAL, "%s: params is NULL", fn);
    if (sp->max_sec < 1 || sp->max_sec > AIM_SEC_MAX) return fail(AIM_EINVAL, "%s: max_sec %u is outside 1..%u", fn, sp->max_sec, AIM_SEC_MAX);
    if (sp->options & ~AIM_SEC_RECORDS) return fail(AIM_EINVAL, "%s: unknown options 0x%x", fn, sp->options);
    return AIM_OK;
}

// Every refusal of aim_mapper_device_bytes and aim_mapper_create, in stage order; no device is asked anything.
int check_mapper_params(const char *fn, const aim_mapper_params_t *p, uint64_t ref_len)
{
    if (!p) return fail(AIM_EINVAL, "%s: params is NULL", fn);
    const aim_seed_params_t &sp = p->seed;
    if (p->max_hits) {
        if (check_seed_long_params(sp, p->max_hits)) return under(fn, AIM_EINVAL);
    } else {
        if (check_seed_params(sp, AIM_SEED_MAX_READ_SIZE, "aim_seed_chain_device") || check_seed_chain_band(sp, "aim_seed_chain_device")) return under(fn, AIM_EINVAL);
        if (!sp.options) return fail(AIM_EINVAL, "%s: aim_seed_params_t: options 0x0 must be AIM_SEED_OPT_MINIMIZERS(w) (the mapper builds a minimizer index)", fn);
    }
    const uint32_t K = (uint32_t)sp.max_cands, rs = (uint32_t)sp.read_size;
    if (p->mask_q8 < 1 || p->mask_q8 > 256) return fail(AIM_EINVAL, "%s: mask_q8 %u is outside 1..256", fn, p->mask_q8);
    if (!(slots_ok(fn, p->max_reads, K, "max_cands") && ref_len_ok(fn, ref_len, false))) return AIM_EINVAL;
    if (p->options & AIM_MAP_EXTEND)
        if (const int rc = check_extend_params(fn, &p->extend)) return rc;
    const aim_endsfree_params_t ap = align_params(*p);
    if (check_align_params(ap.base)) return under(fn, AIM_EINVAL);
    if (p->sam_options & ~AIM_SAM_EQX) return fail(AIM_EINVAL, "%s: unknown sam_options 0x%x", fn, p->sam_options);
    if ((uint64_t)p->max_reads * K * (4ull * rs + 10ull) >= (1ull << 32))
        return fail(AIM_EINVAL, "%s: max_reads %u * K %u rows of read_size %u exceed the 32-bit offsets of aim_sam_t (max_reads * K * (4 * read_size + 10) must stay below 2^32)",
                    fn, p->max_reads, K, rs);
    if (p->options & ~AIM_MAP_EXTEND) return fail(AIM_EINVAL, "%s: unknown options 0x%x", fn, p->options);
    if (!p->max_reads) return fail(AIM_EINVAL, "%s: max_reads must be >= 1", fn);
    if (p->slots < 1 || p->slots > AIM_MAPPER_MAX_SLOTS) return fail(AIM_EINVAL, "%s: slots %u is outside 1..%d", fn, p->slots, AIM_MAPPER_MAX_SLOTS);
    return AIM_OK;
}

// Rule 13c's layout and its bounds, under the name `fn`: starts (when asked for) and ref_len.
int contigs_layout(const char *fn, uint32_t n, const uint32_t *lens, uint32_t spacer, uint32_t *starts, uint64_t *ref_len)
{
    if (n < 1 || n > AIM_CONTIG_MAX) return fail(AIM_EINVAL, "%s: n_contigs %u is outside 1..%u", fn, n, AIM_CONTIG_MAX);
    if (!lens) return fail(AIM_EINVAL, "%s: lens is NULL", fn);
    if (spacer < 1) return fail(AIM_EINVAL, "%s: spacer %u must be >= 1", fn, spacer);
    uint64_t at = 0;
    for (uint32_t c = 0; c < n; ++c) {
        if (!lens[c]) return fail(AIM_EINVAL, "%s: lens[%u] is 0 (a contig holds at least one base)", fn, c);
        if (c) at += spacer;
        if (at + lens[c] > AIM_SEED_MAX_REF_LEN)
            return fail(AIM_EINVAL, "%s: contig %u ends at %llu: ref_len is above %llu", fn, c, (unsigned long long)(at + lens[c]), (unsigned long long)AIM_SEED_MAX_REF_LEN);
        if (starts) starts[c] = (uint32_t)at;
        at += lens[c];
    }
    if (ref_len) *ref_len = at;
    return AIM_OK;
}

void contigs_concat(uint32_t n, const char *const *seqs, const uint32_t *lens, const uint32_t *starts, uint64_t ref_len, char *out)
{
    memset(out, 'N', (size_t)ref_len);
    for (uint32_t c = 0; c < n; ++c) memcpy(out + starts[c], seqs[c], lens[c]);
}

// The spacer of the mapper: the band as far as any chain kernel takes one (a band outside its bounds is refused by the mapper's checks).
uint32_t mapper_spacer(const aim_mapper_params_t &p) { return AIM_CONTIG_SPACER(std::min(std::max(p.seed.band, 0), AIM_SEED_CHAIN_MAX_BAND)); }

// The device buffers of one slot, in allocation order: `bytes` each, carved out of one allocation at multiples of 256.
enum Buf { B_READS, B_READ_LEN, B_REQ, B_TEXT_POS, B_VOTES, B_SEED, B_CHAINS, B_CLASS, B_SEG_REQ, B_SEG_TEXT_POS, B_SEG_PATTERNS, B_SEG, B_EXT,
           B_RESULTS, B_OPS, B_SCRATCH, B_SAM, B_CIGAR, B_MD, B_OFFSETS, B_RECORDS, B_MAP_SCRATCH, B_CONTIG,
           // rule 14c, after aim_mapper_set_pairing alone (the B_RES_* only with AIM_PAIR_RESCUE): a mapper without it keeps its layout
           B_PAIRS, B_MATES, B_RES_CURSORS, B_RES_REQ, B_RES_TEXT_POS, B_RES_PATTERNS, B_RES_RESULTS, B_RES_OPS, B_RES_SCRATCH, B_RES_SAM,
           // rule 15c, after aim_mapper_set_pairing_estimated alone: the estimate and its histogram
           B_EST, B_EST_SCRATCH,
           // rule 16c, after aim_mapper_set_secondary alone: aim_sec_slot_t per slot and aim_map_sec_t per record
           B_SEC, B_SEC_RECORDS,
           // rule 17c, after aim_mapper_set_pairing_secondary alone: aim_map_pair_mapq_t per read pair
           B_PAIR_MAPQ, B_COUNT };

struct SlotLayout {
    uint64_t at[B_COUNT], bytes[B_COUNT], total;
};

inline uint64_t up256(uint64_t x) { return (x + 255u) & ~255ull; }

SlotLayout slot_layout(const aim_mapper_params_t &p, size_t align_scratch, bool contigs, const aim_map_pair_params_t *pp = nullptr, size_t rescue_scratch = 0,
                       const aim_pair_est_params_t *ep = nullptr, bool secondary = false)
{
    const uint64_t N = p.max_reads, K = (uint64_t)p.seed.max_cands, rs = (uint64_t)p.seed.read_size, S = N * K;
    SlotLayout L;
    memset(&L, 0, sizeof L);
    uint64_t *b = L.bytes;
    b[B_READS] = N * rs + 64; b[B_READ_LEN] = 4 * N;
    b[B_REQ] = 16 * S; b[B_TEXT_POS] = 8 * S; b[B_VOTES] = 4 * S; b[B_SEED] = 16 * N; b[B_CHAINS] = 16 * S; b[B_CLASS] = 8 * S;
    b[B_SEG_REQ] = 16 * S; b[B_SEG_TEXT_POS] = 8 * S; b[B_SEG_PATTERNS] = S * rs + 64; b[B_SEG] = 8 * S;
    b[B_EXT] = (p.options & AIM_MAP_EXTEND) ? 24 * S : 0;
    b[B_RESULTS] = sizeof(aim_result_t) * S; b[B_OPS] = S * 2 * rs + 64; b[B_SCRATCH] = align_scratch;
    b[B_SAM] = sizeof(aim_sam_t) * S; b[B_CIGAR] = 4ull * p.cigar_cap; b[B_MD] = p.md_cap;
    b[B_OFFSETS] = 4 * (N + 3);          // rec_offsets[n_reads + 1], then the two cursors of the SAM kernel: one copy fetches the three dwords
    b[B_RECORDS] = sizeof(aim_map_record_t) * S; b[B_MAP_SCRATCH] = kMapScratch;
    b[B_CONTIG] = contigs ? 4 * S : 0;   // d_contig of rule 13c: a mapper of one sequence has none and keeps its size
    if (pp) {                            // rule 14c: the rescue regions behind the main ones, and the buffers of the new stages
        b[B_CIGAR] += 4ull * pp->rescue_cigar_cap; b[B_MD] += pp->rescue_md_cap;
        b[B_PAIRS] = sizeof(aim_map_pair_t) * ((N + 1) / 2); b[B_MATES] = sizeof(aim_map_mate_t) * S; b[B_RES_CURSORS] = 8;
        if (pp->options & AIM_PAIR_RESCUE) {
            const uint64_t rz = pp->rescue_size;
            b[B_RES_REQ] = 16 * N; b[B_RES_TEXT_POS] = 8 * N; b[B_RES_PATTERNS] = N * rz + 64; b[B_RES_RESULTS] = sizeof(aim_result_t) * N;
            b[B_RES_OPS] = N * 2 * rz + 64; b[B_RES_SCRATCH] = rescue_scratch; b[B_RES_SAM] = sizeof(aim_sam_t) * N;
        }
    }
    if (pp && ep) {                      // rule 15c
        b[B_EST] = sizeof(aim_pair_estimate_t); b[B_EST_SCRATCH] = aim_pair_estimate_scratch(ep->hist_size);
    }
    if (secondary) {                     // rule 16c
        b[B_SEC] = sizeof(aim_sec_slot_t) * S; b[B_SEC_RECORDS] = sizeof(aim_map_sec_t) * S;
    }
    if (pp && secondary) b[B_PAIR_MAPQ] = sizeof(aim_map_pair_mapq_t) * ((N + 1) / 2);   // rule 17c
    uint64_t at = 0;
    for (int i = 0; i < B_COUNT; ++i) {
        L.at[i] = at;
        if (i >= B_CONTIG && !b[i]) continue;   // the buffers of rules 13c to 17c exist only where the rule runs
        at += up256(std::max<uint64_t>(b[i], 4));
    }
    L.total = at;
    return L;
}

struct MapperSlot {
    hipStream_t stream = nullptr;
    char *dev = nullptr;                 // SlotLayout
    char *h_reads = nullptr;             // pinned
    int32_t *h_read_len = nullptr;
    aim_map_record_t *h_records = nullptr;
    uint32_t *h_offsets = nullptr;
    uint32_t *h_cigar = nullptr;
    char *h_md = nullptr;
    uint32_t *h_head = nullptr;          // {record count, CIGAR words, MD bytes}
    bool in_flight = false;
    uint32_t n_reads = 0;
    // rule 14c (aim_mapper_set_pairing): the views of aim_mapper_pairs and what the last wait found
    aim_map_mate_t *h_mates = nullptr;   // pinned
    aim_map_pair_t *h_pairs = nullptr;
    uint32_t *h_res_head = nullptr;      // {rescue CIGAR words, rescue MD bytes}
    bool waited = false;
    aim_mapper_pairs_out_t po = {};
    aim_pair_estimate_t *h_est = nullptr;   // rule 15c (aim_mapper_set_pairing_estimated): pinned; the last batch waited for
    aim_map_sec_t *h_sec = nullptr;      // rule 16c (aim_mapper_set_secondary): pinned; the view of aim_mapper_secondary
    uint32_t n_records = 0;              // ... and how many of them the last wait copied
    aim_map_pair_mapq_t *h_pair_mapq = nullptr;   // rule 17c (aim_mapper_set_pairing_secondary): pinned; the view of aim_mapper_pair_mapq
};

}  // namespace

struct aim_mapper {
    aim_mapper_params_t p;
    aim_endsfree_params_t ap;
    int device = 0;
    uint64_t ref_len = 0;
    char *d_ref = nullptr;
    uint32_t *d_bucket = nullptr, *d_pos = nullptr;
    std::vector<uint32_t> starts, lens;  // rule 13c's layout; empty for a reference of one sequence
    uint32_t *d_contig_start = nullptr, *d_contig_len = nullptr;
    size_t align_scratch = 0;
    SlotLayout L;
    MapperSlot slot[AIM_MAPPER_MAX_SLOTS];
    bool paired = false;                 // rule 14c: aim_mapper_set_pairing was called
    aim_map_pair_params_t pp = {};
    aim_endsfree_params_t rap = {};      // the rescue alignment
    size_t rescue_scratch = 0;
    bool estimated = false;              // rule 15c: ... through aim_mapper_set_pairing_estimated
    aim_pair_est_params_t ep = {};
    bool secondary = false;              // rule 16c: aim_mapper_set_secondary was called
    aim_map_sec_params_t sc = {};
    bool combined = false;               // rule 17c: paired and secondary through aim_mapper_set_pairing_secondary
};

namespace {

template <typename T>
T *at(const aim_mapper *m, const MapperSlot &s, Buf b) { return reinterpret_cast<T *>(s.dev + m->L.at[b]); }

void release(aim_mapper *m)
{
    for (MapperSlot &s : m->slot) {
        if (s.stream) (void)hipStreamSynchronize(s.stream);
        if (s.dev) (void)hipFree(s.dev);
        for (void *h : {(void *)s.h_reads, (void *)s.h_read_len, (void *)s.h_records, (void *)s.h_offsets, (void *)s.h_cigar, (void *)s.h_md, (void *)s.h_head,
                        (void *)s.h_mates, (void *)s.h_pairs, (void *)s.h_res_head, (void *)s.h_est, (void *)s.h_sec, (void *)s.h_pair_mapq})
            if (h) (void)hipHostFree(h);
        if (s.stream) (void)hipStreamDestroy(s.stream);
    }
    if (m->d_ref) (void)hipFree(m->d_ref);
    if (m->d_bucket) (void)hipFree(m->d_bucket);
    if (m->d_pos) (void)hipFree(m->d_pos);
    if (m->d_contig_start) (void)hipFree(m->d_contig_start);
    delete m;
}

template <typename T>
int pinned(T **p, uint64_t bytes) { HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(p), (size_t)std::max<uint64_t>(bytes, 16), hipHostMallocDefault)); return AIM_OK; }

int create(aim_mapper *m, const char *seq)
{
    const aim_mapper_params_t &p = m->p;
    const uint64_t N = p.max_reads, K = (uint64_t)p.seed.max_cands, rs = (uint64_t)p.seed.read_size;
    const int32_t k = p.seed.k, w = (int32_t)(p.seed.options >> 8);
    HIP_TRY(hipSetDevice(m->device));
    // the reference with its 16 bytes of slack, then the minimizer index on the device; the build's scratch goes before the slots come
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&m->d_ref), (size_t)up256(m->ref_len + 16)));
    HIP_TRY(hipMemset(m->d_ref, 0, (size_t)up256(m->ref_len + 16)));
    if (m->ref_len) HIP_TRY(hipMemcpy(m->d_ref, seq, (size_t)m->ref_len, hipMemcpyHostToDevice));
    uint64_t be = 0, pc = 0, isb = 0;
    if (const int rc = aim_index_sizes(k, m->ref_len, &be, &pc)) return rc;
    if (const int rc = aim_index_device_scratch(k, m->ref_len, &isb)) return rc;
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&m->d_bucket), (size_t)(be * 4)));
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&m->d_pos), (size_t)std::max<uint64_t>(pc * 4, 256)));
    void *iscr = nullptr;
    HIP_TRY(hipMalloc(&iscr, (size_t)std::max<uint64_t>(isb, 256)));
    int rc = aim_index_build_device_minimizers(m->d_ref, m->ref_len, k, w, m->d_bucket, m->d_pos, iscr, isb, nullptr);
    const hipError_t e = hipDeviceSynchronize();
    (void)hipFree(iscr);
    if (rc) return rc;
    HIP_TRY(e);
    if (const size_t nc = m->starts.size()) {   // one allocation: starts, then lens
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&m->d_contig_start), 8 * nc));
        m->d_contig_len = m->d_contig_start + nc;
        HIP_TRY(hipMemcpy(m->d_contig_start, m->starts.data(), 4 * nc, hipMemcpyHostToDevice));
        HIP_TRY(hipMemcpy(m->d_contig_len, m->lens.data(), 4 * nc, hipMemcpyHostToDevice));
    }
    m->align_scratch = aim_scratch_bytes(&m->ap.base, (uint32_t)(N * K));
    if (!m->align_scratch) return under("aim_mapper_create", AIM_ENOMEM);
    m->L = slot_layout(p, m->align_scratch, !m->starts.empty());
    for (uint32_t i = 0; i < p.slots; ++i) {
        MapperSlot &s = m->slot[i];
        HIP_TRY(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&s.dev), (size_t)m->L.total));
        HIP_TRY(hipMemset(s.dev, 0, (size_t)m->L.total));
        if ((rc = pinned(&s.h_reads, N * rs)) || (rc = pinned(&s.h_read_len, 4 * N)) || (rc = pinned(&s.h_records, sizeof(aim_map_record_t) * N * K)) ||
            (rc = pinned(&s.h_offsets, 4 * (N + 1))) || (rc = pinned(&s.h_cigar, 4ull * p.cigar_cap)) || (rc = pinned(&s.h_md, p.md_cap)) || (rc = pinned(&s.h_head, 16)))
            return rc;
    }
    HIP_TRY(hipDeviceSynchronize());
    return AIM_OK;
}

}  // namespace

extern "C" {

// ---------------------------------------------------------------------------
// the record list (rule 12c in aim_hip.h, the kernels in mapper.hpp)
// ---------------------------------------------------------------------------
const char *aim_mapper_kernel_names(void) { return "map_count_kernel,map_records_kernel"; }

size_t aim_map_records_scratch(uint32_t) { return kMapScratch; }

}  // extern "C"

namespace {

// Rule 12c's three steps; with d_contig rule 13c's record kernel takes map_records_kernel's place.
int map_records(const char *fn, bool contigs, uint32_t K, uint32_t n_reads, const aim_segment_t *d_seg, const aim_sam_t *d_sam, const aim_chain_class_t *d_class,
                const uint32_t *d_contig, uint32_t n_contigs, const uint32_t *d_contig_start, uint32_t *d_rec_offsets, aim_map_record_t *d_records,
                void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
    if (!(cands_ok(fn, K) && slots_ok(fn, n_reads, K) && (d_rec_offsets || refuse("%s: d_rec_offsets is NULL", fn)) &&
          (!contigs || (n_contigs >= 1 && n_contigs <= AIM_CONTIG_MAX) || refuse("%s: n_contigs %u is outside 1..%u", fn, n_contigs, AIM_CONTIG_MAX)) &&
          buffers_ok(fn, n_reads, d_seg && d_sam && d_class && d_records && d_scratch && (!contigs || (d_contig && d_contig_start))) &&
          (!(((uintptr_t)d_sam | (uintptr_t)d_records) & 15u) || refuse("%s: d_sam and d_records must be 16-byte aligned", fn)) &&
          (!n_reads || scratch_bytes >= kMapScratch ||
           refuse("%s: scratch_bytes %zu is below the %zu aim_map_records_scratch reports", fn, scratch_bytes, kMapScratch))))
        return AIM_EINVAL;
    hipStream_t stream = (hipStream_t)hip_stream;
    int n_dev = 0;
    if (const int rc = aim_device_count(&n_dev)) return rc;
    if (!n_reads) {
        HIP_TRY(hipMemsetAsync(d_rec_offsets, 0, 4, stream));
        return AIM_OK;
    }
    const aim::Knobs kn = with_chip(read_knobs());
    // Debugging aid, as for the index scratch: results must not depend on what the scratch held before.
    if (kn.poison_scratch >= 0) HIP_TRY(hipMemsetAsync(d_scratch, kn.poison_scratch & 0xff, kMapScratch, stream));
    const aim::MapArgs a = {K, n_reads, d_seg, d_sam, d_class, d_rec_offsets, d_records};
    const uint32_t lanes = aim::chain_class_lanes(K), per_block = aim::kMapThreads / lanes;
    const uint32_t resident = aim::resident_grid(kn, aim::kMapPerCu);
    const uint32_t grid = (uint32_t)std::min<uint64_t>(resident, ((uint64_t)n_reads + per_block - 1u) / per_block);
    aim::IndexScanArgs s;
    memset(&s, 0, sizeof s);
    s.data = d_rec_offsets; s.n = (uint64_t)n_reads + 1u; s.dbg_poison_lds = poison_lds_word(kn); s.part = static_cast<uint32_t *>(d_scratch);
    s.n_parts = (uint32_t)std::min<uint64_t>(std::min(resident, aim::kIndexScanParts), (s.n + aim::kIndexScanBlock - 1u) / aim::kIndexScanBlock);
    s.per_part = ((s.n + s.n_parts - 1u) / s.n_parts + aim::kIndexScanBlock - 1u) / aim::kIndexScanBlock * aim::kIndexScanBlock;
    if (kn.plan_debug)
        fprintf(stderr, "[aim plan] map_count_kernel grid=%u block=%d lanes=%u reads=%u K=%u; scan parts=%u per_part=%llu; %s grid=%u block=%d\n", grid,
                aim::kMapThreads, lanes, n_reads, K, s.n_parts, (unsigned long long)s.per_part, contigs ? "map_records_contig_kernel" : "map_records_kernel", grid,
                aim::kMapThreads);
    aim::map_count_launch(a, lanes, grid, stream);
    HIP_TRY(hipGetLastError());
    aim::index_launch_scan(s, stream);
    HIP_TRY(hipGetLastError());
    if (contigs) aim::map_records_contig_launch(a, lanes, grid, d_contig, n_contigs, d_contig_start, stream);
    else aim::map_records_launch(a, lanes, grid, stream);
    HIP_TRY(hipGetLastError());
    return AIM_OK;
}

// Rule 14c's stages between aim_sam_device_split and the record kernel, on the slot's buffers: the rescue rows, their alignment and
// their records behind the main CIGAR / MD regions (the three with AIM_PAIR_RESCUE alone), then select / apply. With rule 15c the
// estimate comes first, and the two kernels of rule 14c read their bounds from it.
int submit_pairing(aim_mapper *m, MapperSlot &s, uint32_t n_reads, hipStream_t st)
{
    const aim_mapper_params_t &p = m->p;
    const aim_map_pair_params_t &pp = m->pp;
    const uint32_t K = (uint32_t)p.seed.max_cands, rs = (uint32_t)p.seed.read_size, n_contigs = (uint32_t)m->starts.size();
    const bool rescue = (pp.options & AIM_PAIR_RESCUE) != 0;
    int32_t *d_rl = at<int32_t>(m, s, B_READ_LEN);
    aim_segment_t *d_seg = at<aim_segment_t>(m, s, B_SEG);
    aim_sam_t *d_sam = at<aim_sam_t>(m, s, B_SAM), *d_res_sam = rescue ? at<aim_sam_t>(m, s, B_RES_SAM) : nullptr;
    uint32_t *d_contig = n_contigs ? at<uint32_t>(m, s, B_CONTIG) : nullptr, *d_res_cursors = at<uint32_t>(m, s, B_RES_CURSORS);
    aim_chain_class_t *d_cls = at<aim_chain_class_t>(m, s, B_CLASS);
    aim_pair_estimate_t *d_est = m->estimated ? at<aim_pair_estimate_t>(m, s, B_EST) : nullptr;
    aim_sec_slot_t *d_sec = m->combined ? at<aim_sec_slot_t>(m, s, B_SEC) : nullptr;   // rule 17c
    int rc = AIM_OK;
    if (m->estimated)
        rc = aim_pair_estimate_device(&pp, &m->ep, K, rs, n_reads, d_seg, d_sam, d_cls, d_contig, d_est, at<void>(m, s, B_EST_SCRATCH), (size_t)m->L.bytes[B_EST_SCRATCH], st);
    if (rc) return rc;
    if (rescue) {
        void *d_req = at<void>(m, s, B_RES_REQ), *d_res = at<void>(m, s, B_RES_RESULTS);
        uint64_t *d_tp = at<uint64_t>(m, s, B_RES_TEXT_POS);
        char *d_pat = at<char>(m, s, B_RES_PATTERNS), *d_ops = at<char>(m, s, B_RES_OPS);
        // (rule 17c: the slots d_sec gave a role, anchored at the representative; its d_est may be NULL)
        rc = m->combined    ? aim_pair_rescue_rows_secondary_device(&pp, K, rs, m->ref_len, n_contigs, m->d_contig_start, m->d_contig_len, n_reads, d_rl,
                                                                    at<char>(m, s, B_READS), d_seg, d_sam, d_contig, d_sec, d_req, d_tp, d_pat, d_est, st)
             : m->estimated ? aim_pair_rescue_rows_device_est(&pp, K, rs, m->ref_len, n_contigs, m->d_contig_start, m->d_contig_len, n_reads, d_rl, at<char>(m, s, B_READS),
                                                              d_seg, d_sam, d_contig, d_req, d_tp, d_pat, d_est, st)
                            : aim_pair_rescue_rows_device(&pp, K, rs, m->ref_len, n_contigs, m->d_contig_start, m->d_contig_len, n_reads, d_rl, at<char>(m, s, B_READS), d_seg,
                                                          d_sam, d_contig, d_req, d_tp, d_pat, st);
        if (!rc) rc = aim_align_device_ref(&m->rap.base, n_reads, d_req, d_pat, d_tp, m->d_ref, m->ref_len, d_res, d_ops, at<void>(m, s, B_RES_SCRATCH), m->rescue_scratch, st);
        if (!rc)
            rc = aim_sam_device(&m->rap.base, n_reads, d_req, d_tp, nullptr, d_res, d_ops, m->d_ref, m->ref_len, p.sam_options, d_res_sam,
                                at<uint32_t>(m, s, B_CIGAR) + p.cigar_cap, pp.rescue_cigar_cap, at<char>(m, s, B_MD) + p.md_cap, pp.rescue_md_cap, d_res_cursors, st);
    } else {
        HIP_TRY(hipMemsetAsync(d_res_cursors, 0, 8, st));
    }
    aim_map_pair_t *d_pairs = at<aim_map_pair_t>(m, s, B_PAIRS);
    if (!rc)
        rc = m->combined    ? aim_pair_select_secondary_device(&pp, K, rs, n_reads, d_rl, d_seg, d_sam, d_cls, d_contig, d_sec, at<aim_chain_t>(m, s, B_CHAINS), p.mismatch,
                                                               d_res_sam, p.cigar_cap, p.md_cap, d_pairs, at<aim_map_pair_mapq_t>(m, s, B_PAIR_MAPQ), d_est, st)
             : m->estimated ? aim_pair_select_device_est(&pp, K, rs, n_reads, d_rl, d_seg, d_sam, d_cls, d_contig, d_res_sam, p.cigar_cap, p.md_cap, d_pairs, d_est, st)
                            : aim_pair_select_device(&pp, K, rs, n_reads, d_rl, d_seg, d_sam, d_cls, d_contig, d_res_sam, p.cigar_cap, p.md_cap, d_pairs, st);
    return rc;
}

// What aim_mapper_device_bytes and its contig twin report, behind their checks.
int mapper_bytes(const char *fn, const aim_mapper_params_t *params, uint64_t ref_len, uint32_t n_contigs, uint64_t *bytes)
{
    if (!bytes) return fail(AIM_EINVAL, "%s: bytes is NULL", fn);
    const aim_endsfree_params_t ap = align_params(*params);
    const size_t as = aim_scratch_bytes(&ap.base, (uint32_t)((uint64_t)params->max_reads * (uint64_t)params->seed.max_cands));
    if (!as) return under(fn, AIM_ENOMEM);
    uint64_t be = 0, pc = 0, isb = 0;
    if (aim_index_sizes(params->seed.k, ref_len, &be, &pc) || aim_index_device_scratch(params->seed.k, ref_len, &isb)) return under(fn, AIM_EINVAL);
    *bytes = up256(ref_len + 16) + be * 4 + std::max<uint64_t>(pc * 4, 256) + 8ull * n_contigs +
             std::max<uint64_t>(std::max<uint64_t>(isb, 256), (uint64_t)params->slots * slot_layout(*params, as, n_contigs != 0).total);
    return AIM_OK;
}

// The device probe and the object, behind the checks of aim_mapper_create and its contig twin (which filled m's layout first).
int mapper_make(const char *fn, aim_mapper *m, const aim_mapper_params_t *params, int device, const char *seq, uint64_t ref_len, aim_mapper_t **mapper)
{
    int n_dev = 0;
    int rc = aim_device_count(&n_dev);
    if (!rc && (device < 0 || device >= n_dev)) rc = fail(AIM_EINVAL, "%s: device %d is outside 0..%d", fn, device, n_dev - 1);
    if (rc) {
        delete m;
        return rc;
    }
    m->p = *params;
    m->ap = align_params(*params);
    m->device = device;
    m->ref_len = ref_len;
    if ((rc = create(m, seq))) {
        const std::string was = aim_last_error();   // (release() must not lose the message)
        release(m);
        return fail(rc, "%s", was.c_str());
    }
    *mapper = m;
    return AIM_OK;
}

}  // namespace

extern "C" {

int aim_map_records_device(uint32_t K, uint32_t n_reads, const aim_segment_t *d_seg, const aim_sam_t *d_sam, const aim_chain_class_t *d_class,
                           uint32_t *d_rec_offsets, aim_map_record_t *d_records, void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
    return map_records("aim_map_records_device", false, K, n_reads, d_seg, d_sam, d_class, nullptr, 0, nullptr, d_rec_offsets, d_records, d_scratch, scratch_bytes,
                       hip_stream);
}

// ---------------------------------------------------------------------------
// several sequences (AIM_FEATURE_CONTIGS; rule 13c in aim_hip.h, the clip kernel in contig.hpp, the record kernel in mapper.hpp)
// ---------------------------------------------------------------------------
const char *aim_contig_kernel_names(void) { return "contig_clip_kernel,map_records_contig_kernel"; }

int aim_contigs_layout(uint32_t n_contigs, const uint32_t *lens, uint32_t spacer, uint32_t *starts, uint64_t *ref_len)
{
    const char *fn = "aim_contigs_layout";
    if (const int rc = contigs_layout(fn, n_contigs, lens, spacer, nullptr, nullptr)) return rc;
    if (!starts || !ref_len) return fail(AIM_EINVAL, "%s: %s is NULL", fn, starts ? "ref_len" : "starts");
    return contigs_layout(fn, n_contigs, lens, spacer, starts, ref_len);
}

int aim_contigs_concat(uint32_t n_contigs, const char *const *seqs, const uint32_t *lens, uint32_t spacer, char *out)
{
    const char *fn = "aim_contigs_concat";
    uint64_t ref_len = 0;
    if (const int rc = contigs_layout(fn, n_contigs, lens, spacer, nullptr, &ref_len)) return rc;
    if (!seqs || !out) return fail(AIM_EINVAL, "%s: %s is NULL", fn, seqs ? "out" : "seqs");
    for (uint32_t c = 0; c < n_contigs; ++c)
        if (!seqs[c]) return fail(AIM_EINVAL, "%s: seqs[%u] is NULL", fn, c);
    std::vector<uint32_t> starts(n_contigs);
    (void)contigs_layout(fn, n_contigs, lens, spacer, starts.data(), nullptr);
    contigs_concat(n_contigs, seqs, lens, starts.data(), ref_len, out);
    return AIM_OK;
}

int aim_contig_clip_device(uint32_t K, uint32_t read_size, int32_t flank, uint64_t ref_len, uint32_t n_contigs, const uint32_t *d_contig_start,
                           const uint32_t *d_contig_len, uint32_t n_reads, const int32_t *d_read_len, const void *d_requests, const uint64_t *d_text_pos,
                           const aim_chain_t *d_chains, void *d_seg_requests, uint64_t *d_seg_text_pos, aim_segment_t *d_seg, uint32_t *d_contig, void *hip_stream)
{
    const char *fn = "aim_contig_clip_device";
    if (!(cands_ok(fn, K) && read_size_ok(fn, read_size) && slots_ok(fn, n_reads, K) && (flank >= 0 || refuse("%s: flank %d must be >= 0", fn, flank)) &&
          (ref_len >= 1 || refuse("%s: ref_len must be >= 1", fn)) && ref_len_ok(fn, ref_len, false) &&
          ((n_contigs >= 1 && n_contigs <= AIM_CONTIG_MAX) || refuse("%s: n_contigs %u is outside 1..%u", fn, n_contigs, AIM_CONTIG_MAX)) &&
          ((d_contig_start && d_contig_len) || refuse("%s: d_contig_start or d_contig_len is NULL", fn)) &&
          buffers_ok(fn, n_reads, d_read_len && d_requests && d_text_pos && d_chains && d_seg_requests && d_seg_text_pos && d_seg && d_contig)))
        return AIM_EINVAL;
    return launch_batch(n_reads, [&](const aim::Knobs &kn) {
        aim::ContigArgs a;
        memset(&a, 0, sizeof a);
        a.K = K; a.read_size = read_size; a.n_slots = n_reads * K; a.n_contigs = n_contigs; a.step_log2 = aim::contig_step_log2(n_contigs);
        a.dbg_poison_lds = poison_lds_word(kn);
        a.flank = flank; a.ref_len = (int64_t)ref_len;
        a.start = d_contig_start; a.len = d_contig_len;
        a.read_len = d_read_len; a.requests = static_cast<const aim_request_t *>(d_requests); a.text_pos = d_text_pos; a.chains = d_chains;
        a.seg_requests = static_cast<aim_request_t *>(d_seg_requests); a.seg_text_pos = d_seg_text_pos; a.seg = d_seg; a.contig = d_contig;
        // the step comes from n_contigs alone; only the grid is the device's
        const uint32_t grid = (uint32_t)std::min<uint64_t>(aim::resident_grid(kn, aim::kContigPerCu), ((uint64_t)a.n_slots + aim::kContigThreads - 1u) / aim::kContigThreads);
        if (kn.plan_debug)
            fprintf(stderr, "[aim plan] contig_clip_kernel grid=%u block=%d contigs=%u step=%u slots=%u\n", grid, aim::kContigThreads, n_contigs, 1u << a.step_log2,
                    a.n_slots);
        aim::contig_clip_launch(a, grid, (hipStream_t)hip_stream);
    });
}

int aim_map_records_contigs_device(uint32_t K, uint32_t n_reads, const aim_segment_t *d_seg, const aim_sam_t *d_sam, const aim_chain_class_t *d_class,
                                   const uint32_t *d_contig, uint32_t n_contigs, const uint32_t *d_contig_start, uint32_t *d_rec_offsets,
                                   aim_map_record_t *d_records, void *d_scratch, size_t scratch_bytes, void *hip_stream)
{
    return map_records("aim_map_records_contigs_device", true, K, n_reads, d_seg, d_sam, d_class, d_contig, n_contigs, d_contig_start, d_rec_offsets, d_records,
                       d_scratch, scratch_bytes, hip_stream);
}

// ---------------------------------------------------------------------------
// aim_mapper_t
// ---------------------------------------------------------------------------
int aim_mapper_device_bytes(const aim_mapper_params_t *params, uint64_t ref_len, uint64_t *bytes)
{
    const char *fn = "aim_mapper_device_bytes";
    if (const int rc = check_mapper_params(fn, params, ref_len)) return rc;
    return mapper_bytes(fn, params, ref_len, 0, bytes);
}

int aim_mapper_device_bytes_contigs(const aim_mapper_params_t *params, uint32_t n_contigs, const uint32_t *lens, uint64_t *bytes)
{
    const char *fn = "aim_mapper_device_bytes_contigs";
    if (!params) return fail(AIM_EINVAL, "%s: params is NULL", fn);
    uint64_t ref_len = 0;
    if (const int rc = contigs_layout(fn, n_contigs, lens, mapper_spacer(*params), nullptr, &ref_len)) return rc;
    if (const int rc = check_mapper_params(fn, params, ref_len)) return rc;
    return mapper_bytes(fn, params, ref_len, n_contigs, bytes);
}

int aim_mapper_create(const aim_mapper_params_t *params, int device, const char *seq, uint64_t ref_len, aim_mapper_t **mapper)
{
    const char *fn = "aim_mapper_create";
    if (const int rc = check_mapper_params(fn, params, ref_len)) return rc;
    if (!mapper) return fail(AIM_EINVAL, "%s: mapper is NULL", fn);
    if (ref_len && !seq) return fail(AIM_EINVAL, "%s: seq is NULL", fn);
    return mapper_make(fn, new aim_mapper(), params, device, seq, ref_len, mapper);
}

int aim_mapper_create_contigs(const aim_mapper_params_t *params, int device, uint32_t n_contigs, const char *const *seqs, const uint32_t *lens, aim_mapper_t **mapper)
{
    const char *fn = "aim_mapper_create_contigs";
    if (!params) return fail(AIM_EINVAL, "%s: params is NULL", fn);
    uint64_t ref_len = 0;
    const uint32_t spacer = mapper_spacer(*params);
    if (const int rc = contigs_layout(fn, n_contigs, lens, spacer, nullptr, &ref_len)) return rc;
    if (const int rc = check_mapper_params(fn, params, ref_len)) return rc;
    if (!mapper) return fail(AIM_EINVAL, "%s: mapper is NULL", fn);
    if (!seqs) return fail(AIM_EINVAL, "%s: seqs is NULL", fn);
    for (uint32_t c = 0; c < n_contigs; ++c)
        if (!seqs[c]) return fail(AIM_EINVAL, "%s: seqs[%u] is NULL", fn, c);
    aim_mapper *m = new aim_mapper();
    m->starts.resize(n_contigs);
    m->lens.assign(lens, lens + n_contigs);
    (void)contigs_layout(fn, n_contigs, lens, spacer, m->starts.data(), nullptr);
    std::vector<char> cat((size_t)ref_len);
    contigs_concat(n_contigs, seqs, lens, m->starts.data(), ref_len, cat.data());
    return mapper_make(fn, m, params, device, cat.data(), ref_len, mapper);
}

int aim_mapper_contigs(const aim_mapper_t *m, uint32_t *n_contigs, const uint32_t **starts, const uint32_t **lens)
{
    const char *fn = "aim_mapper_contigs";
    if (!m) return fail(AIM_EINVAL, "%s: mapper is NULL", fn);
    if (!n_contigs || !starts || !lens) return fail(AIM_EINVAL, "%s: NULL output", fn);
    *n_contigs = (uint32_t)m->starts.size();
    *starts = m->starts.empty() ? nullptr : m->starts.data();
    *lens = m->lens.empty() ? nullptr : m->lens.data();
    return AIM_OK;
}

int aim_mapper_submit(aim_mapper_t *m, uint32_t slot, uint32_t n_reads, const int32_t *read_len, const char *reads)
{
    const char *fn = "aim_mapper_submit";
    if (!m) return fail(AIM_EINVAL, "%s: mapper is NULL", fn);
    if (slot >= m->p.slots) return fail(AIM_EINVAL, "%s: slot %u is outside 0..%u", fn, slot, m->p.slots - 1);
    if (n_reads > m->p.max_reads) return fail(AIM_EINVAL, "%s: n_reads %u is above max_reads %u", fn, n_reads, m->p.max_reads);
    if (n_reads && (!read_len || !reads)) return fail(AIM_EINVAL, "%s: NULL read_len or reads", fn);
    if (m->paired && (n_reads & 1u)) return fail(AIM_EINVAL, "%s: n_reads %u is odd (after aim_mapper_set_pairing reads 2m and 2m + 1 are mates)", fn, n_reads);
    MapperSlot &s = m->slot[slot];
    if (s.in_flight) return fail(AIM_ESTATE, "%s: slot %u is in flight (aim_mapper_wait first)", fn, slot);
    HIP_TRY(hipSetDevice(m->device));
    s.n_reads = n_reads;
    s.waited = false;                    // the views of aim_mapper_pairs end here
    if (!n_reads) {                      // a valid batch with nothing to enqueue
        s.in_flight = true;
        return AIM_OK;
    }
    const aim_mapper_params_t &p = m->p;
    const uint32_t K = (uint32_t)p.seed.max_cands, rs = (uint32_t)p.seed.read_size, rows = n_reads * K;
    const int32_t flank = p.seed.flank;
    hipStream_t st = s.stream;
    memcpy(s.h_read_len, read_len, 4ull * n_reads);
    memcpy(s.h_reads, reads, (size_t)n_reads * rs);
    char *d_reads = at<char>(m, s, B_READS), *d_seg_pat = at<char>(m, s, B_SEG_PATTERNS), *d_ops = at<char>(m, s, B_OPS);
    int32_t *d_rl = at<int32_t>(m, s, B_READ_LEN);
    void *d_req = at<void>(m, s, B_REQ), *d_seg_req = at<void>(m, s, B_SEG_REQ), *d_res = at<void>(m, s, B_RESULTS);
    uint64_t *d_tp = at<uint64_t>(m, s, B_TEXT_POS), *d_seg_tp = at<uint64_t>(m, s, B_SEG_TEXT_POS);
    aim_seed_t *d_seed = at<aim_seed_t>(m, s, B_SEED);
    aim_chain_t *d_chains = at<aim_chain_t>(m, s, B_CHAINS);
    aim_chain_class_t *d_cls = at<aim_chain_class_t>(m, s, B_CLASS);
    aim_segment_t *d_seg = at<aim_segment_t>(m, s, B_SEG);
    aim_sam_t *d_sam = at<aim_sam_t>(m, s, B_SAM);
    uint32_t *d_off = at<uint32_t>(m, s, B_OFFSETS), *d_cursors = d_off + n_reads + 1u;
    HIP_TRY(hipMemcpyAsync(d_rl, s.h_read_len, 4ull * n_reads, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_reads, s.h_reads, (size_t)n_reads * rs, hipMemcpyHostToDevice, st));
    int rc = p.max_hits ? aim_seed_chain_long_device(&p.seed, p.max_hits, n_reads, d_rl, d_reads, m->d_bucket, m->d_pos, m->ref_len, d_req, d_tp,
                                                     at<uint32_t>(m, s, B_VOTES), d_seed, d_chains, st)
                        : aim_seed_chain_device(&p.seed, n_reads, d_rl, d_reads, m->d_bucket, m->d_pos, m->ref_len, d_req, d_tp, at<uint32_t>(m, s, B_VOTES),
                                                d_seed, d_chains, st);
    if (!rc) rc = aim_chain_classify_device(K, rs, p.mask_q8, n_reads, d_rl, d_tp, d_seed, d_chains, d_cls, st);
    if (!rc) rc = aim_split_segments_device(K, rs, flank, m->ref_len, n_reads, d_rl, d_reads, d_req, d_tp, d_seed, d_chains, d_cls, d_seg_req, d_seg_tp, d_seg_pat, d_seg, st);
    if (!rc && (p.options & AIM_MAP_EXTEND))
        rc = aim_extend_segments_device(&p.extend, K, rs, m->ref_len, n_reads, d_rl, d_reads, m->d_ref, d_seg_req, d_seg_tp, d_seg_pat, d_seg,
                                        at<aim_extend_t>(m, s, B_EXT), st);
    if (!rc && m->secondary)             // rule 16c, part 1: rows for the secondaries, where the split left empty slots
        rc = aim_secondary_rows_device(K, rs, flank, m->ref_len, n_reads, d_rl, d_reads, d_req, d_tp, d_seed, d_chains, d_cls, d_seg_req, d_seg_tp, d_seg_pat, d_seg,
                                       m->sc.max_sec, st);
    const uint32_t n_contigs = (uint32_t)m->starts.size();
    uint32_t *d_contig = at<uint32_t>(m, s, B_CONTIG);
    if (!rc && n_contigs)
        rc = aim_contig_clip_device(K, rs, flank, m->ref_len, n_contigs, m->d_contig_start, m->d_contig_len, n_reads, d_rl, d_req, d_tp, d_chains, d_seg_req, d_seg_tp,
                                    d_seg, d_contig, st);
    if (!rc) rc = aim_align_device_ref(&m->ap.base, rows, d_seg_req, d_seg_pat, d_seg_tp, m->d_ref, m->ref_len, d_res, d_ops, at<void>(m, s, B_SCRATCH), m->align_scratch, st);
    if (!rc)
        rc = aim_sam_device_split(&m->ap.base, rows, d_seg_req, d_seg_tp, nullptr, d_res, d_ops, m->d_ref, m->ref_len, p.sam_options, d_sam, at<uint32_t>(m, s, B_CIGAR),
                                  p.cigar_cap, at<char>(m, s, B_MD), p.md_cap, d_cursors, d_seg, st);
    if (!rc && m->combined)              // rule 17c: part 2 of rule 16c moves in front of the pairing, which reads and rewrites its d_sec
        rc = aim_secondary_select_device(K, n_reads, d_seg, d_sam, d_cls, d_chains, p.max_score, p.mismatch, at<aim_sec_slot_t>(m, s, B_SEC), st);
    if (!rc && m->paired) rc = submit_pairing(m, s, n_reads, st);   // rule 14c in front of the record kernel: rescue, select / apply
    if (!rc && m->secondary) {           // ... part 2: one winner per locus; part 3: the records over loci
        if (!m->combined)
            rc = aim_secondary_select_device(K, n_reads, d_seg, d_sam, d_cls, d_chains, p.max_score, p.mismatch, at<aim_sec_slot_t>(m, s, B_SEC), st);
        if (!rc)
            rc = aim_map_records_secondary_device(K, n_reads, m->sc.options, d_seg, d_sam, d_cls, at<aim_sec_slot_t>(m, s, B_SEC), n_contigs ? d_contig : nullptr, n_contigs,
                                                  n_contigs ? m->d_contig_start : nullptr, d_off, at<aim_map_record_t>(m, s, B_RECORDS),
                                                  at<aim_map_sec_t>(m, s, B_SEC_RECORDS), at<void>(m, s, B_MAP_SCRATCH), kMapScratch, st);
    } else if (!rc)
        rc = n_contigs ? aim_map_records_contigs_device(K, n_reads, d_seg, d_sam, d_cls, d_contig, n_contigs, m->d_contig_start, d_off,
                                                        at<aim_map_record_t>(m, s, B_RECORDS), at<void>(m, s, B_MAP_SCRATCH), kMapScratch, st)
                       : aim_map_records_device(K, n_reads, d_seg, d_sam, d_cls, d_off, at<aim_map_record_t>(m, s, B_RECORDS), at<void>(m, s, B_MAP_SCRATCH), kMapScratch, st);
    if (!rc && m->combined)              // ... and behind it: the mate fields, the representative from d_sec
        rc = aim_map_mates_secondary_device(K, n_reads, at<aim_map_pair_t>(m, s, B_PAIRS), d_seg, d_sam, at<aim_sec_slot_t>(m, s, B_SEC), n_contigs ? d_contig : nullptr,
                                            n_contigs, m->d_contig_start, d_off, at<aim_map_record_t>(m, s, B_RECORDS), at<aim_map_mate_t>(m, s, B_MATES), st);
    else if (!rc && m->paired)           // ... and behind it: the mate fields
        rc = aim_map_mates_device(K, n_reads, at<aim_map_pair_t>(m, s, B_PAIRS), d_seg, d_sam, n_contigs ? d_contig : nullptr, n_contigs, m->d_contig_start, d_off,
                                  at<aim_map_record_t>(m, s, B_RECORDS), at<aim_map_mate_t>(m, s, B_MATES), st);
    if (rc) {
        (void)hipStreamSynchronize(st);  // what was enqueued reads the pinned buffers
        return under(fn, rc);
    }
    s.in_flight = true;
    return AIM_OK;
}

int aim_mapper_wait(aim_mapper_t *m, uint32_t slot, aim_mapper_out_t *out)
{
    const char *fn = "aim_mapper_wait";
    if (!m) return fail(AIM_EINVAL, "%s: mapper is NULL", fn);
    if (slot >= m->p.slots) return fail(AIM_EINVAL, "%s: slot %u is outside 0..%u", fn, slot, m->p.slots - 1);
    if (!out) return fail(AIM_EINVAL, "%s: out is NULL", fn);
    MapperSlot &s = m->slot[slot];
    if (!s.in_flight) return fail(AIM_ESTATE, "%s: nothing is in flight on slot %u", fn, slot);
    s.in_flight = false;
    s.waited = true;
    memset(&s.po, 0, sizeof s.po);
    s.po.mates = s.h_mates; s.po.pairs = s.h_pairs;
    memset(out, 0, sizeof *out);
    out->n_reads = s.n_reads;
    out->records = s.h_records; out->rec_offsets = s.h_offsets; out->cigar = s.h_cigar; out->md = s.h_md;
    s.h_offsets[0] = 0;
    s.n_records = 0;
    if (m->estimated) {                  // an empty batch: the fallback, every count 0
        memset(s.h_est, 0, sizeof *s.h_est);
        s.h_est->min_span = m->pp.min_span; s.h_est->max_span = m->pp.max_span; s.h_est->flags = AIM_PAIR_EST_FALLBACK;
    }
    if (!s.n_reads) return AIM_OK;
    HIP_TRY(hipSetDevice(m->device));
    const uint32_t *d_off = at<uint32_t>(m, s, B_OFFSETS);
    // one small copy first: rec_offsets[n_reads] and the two cursors behind it; it says how much of everything else is in use
    HIP_TRY(hipMemcpyAsync(s.h_head, d_off + s.n_reads, 12, hipMemcpyDeviceToHost, s.stream));
    if (m->paired) HIP_TRY(hipMemcpyAsync(s.h_res_head, at<char>(m, s, B_RES_CURSORS), 8, hipMemcpyDeviceToHost, s.stream));   // the rescue regions' own cursor pair
    if (m->estimated) HIP_TRY(hipMemcpyAsync(s.h_est, at<char>(m, s, B_EST), sizeof(aim_pair_estimate_t), hipMemcpyDeviceToHost, s.stream));   // rule 15c's 48 bytes
    HIP_TRY(hipStreamSynchronize(s.stream));
    out->n_records = s.h_head[0];
    out->cigar_needed = s.h_head[1]; out->md_needed = s.h_head[2];
    out->cigar_words = std::min(out->cigar_needed, m->p.cigar_cap); out->md_bytes = std::min(out->md_needed, m->p.md_cap);
    HIP_TRY(hipMemcpyAsync(s.h_records, at<char>(m, s, B_RECORDS), sizeof(aim_map_record_t) * (size_t)out->n_records, hipMemcpyDeviceToHost, s.stream));
    HIP_TRY(hipMemcpyAsync(s.h_offsets, d_off, 4ull * (s.n_reads + 1u), hipMemcpyDeviceToHost, s.stream));
    if (out->cigar_words) HIP_TRY(hipMemcpyAsync(s.h_cigar, at<char>(m, s, B_CIGAR), 4ull * out->cigar_words, hipMemcpyDeviceToHost, s.stream));
    if (out->md_bytes) HIP_TRY(hipMemcpyAsync(s.h_md, at<char>(m, s, B_MD), out->md_bytes, hipMemcpyDeviceToHost, s.stream));
    if (m->secondary) {                  // rule 16c: the array parallel to the records
        s.n_records = out->n_records;
        HIP_TRY(hipMemcpyAsync(s.h_sec, at<char>(m, s, B_SEC_RECORDS), sizeof(aim_map_sec_t) * (size_t)out->n_records, hipMemcpyDeviceToHost, s.stream));
    }
    if (m->paired) {                     // rule 14c: the second range of either buffer, the mate fields and the pairs
        aim_mapper_pairs_out_t &po = s.po;
        po.n_pairs = s.n_reads / 2u; po.n_records = out->n_records;
        po.rescue_cigar_needed = s.h_res_head[0]; po.rescue_md_needed = s.h_res_head[1];
        po.rescue_cigar_words = std::min(po.rescue_cigar_needed, m->pp.rescue_cigar_cap); po.rescue_md_bytes = std::min(po.rescue_md_needed, m->pp.rescue_md_cap);
        if (po.rescue_cigar_words)
            HIP_TRY(hipMemcpyAsync(s.h_cigar + m->p.cigar_cap, at<uint32_t>(m, s, B_CIGAR) + m->p.cigar_cap, 4ull * po.rescue_cigar_words, hipMemcpyDeviceToHost, s.stream));
        if (po.rescue_md_bytes) HIP_TRY(hipMemcpyAsync(s.h_md + m->p.md_cap, at<char>(m, s, B_MD) + m->p.md_cap, po.rescue_md_bytes, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipMemcpyAsync(s.h_mates, at<char>(m, s, B_MATES), sizeof(aim_map_mate_t) * (size_t)po.n_records, hipMemcpyDeviceToHost, s.stream));
        HIP_TRY(hipMemcpyAsync(s.h_pairs, at<char>(m, s, B_PAIRS), sizeof(aim_map_pair_t) * (size_t)po.n_pairs, hipMemcpyDeviceToHost, s.stream));
        if (m->combined)                 // rule 17c: one aim_map_pair_mapq_t per pair
            HIP_TRY(hipMemcpyAsync(s.h_pair_mapq, at<char>(m, s, B_PAIR_MAPQ), sizeof(aim_map_pair_mapq_t) * (size_t)po.n_pairs, hipMemcpyDeviceToHost, s.stream));
    }
    HIP_TRY(hipStreamSynchronize(s.stream));
    return AIM_OK;
}

// ---------------------------------------------------------------------------
// paired-end reads (AIM_FEATURE_PAIRED; rule 14c in aim_hip.h, the kernels in pair.hpp, the stateless entry points in capi_pair.hip)
// ---------------------------------------------------------------------------
int aim_mapper_pairing_device_bytes(const aim_mapper_params_t *params, const aim_map_pair_params_t *pp, uint64_t *bytes)
{
    const char *fn = "aim_mapper_pairing_device_bytes";
    if (const int rc = check_mapper_params(fn, params, 0)) return rc;
    if (const int rc = check_pairing(fn, *params, pp)) return rc;
    if (!bytes) return fail(AIM_EINVAL, "%s: bytes is NULL", fn);
    const aim_endsfree_params_t ap = align_params(*params), rap = rescue_params(*params, *pp);
    const size_t as = aim_scratch_bytes(&ap.base, (uint32_t)((uint64_t)params->max_reads * (uint64_t)params->seed.max_cands));
    const size_t rsb = (pp->options & AIM_PAIR_RESCUE) ? aim_scratch_bytes(&rap.base, params->max_reads) : 0;
    if (!as || ((pp->options & AIM_PAIR_RESCUE) && !rsb)) return under(fn, AIM_ENOMEM);
    // (the difference is the same for either kind of mapper)
    *bytes = (uint64_t)params->slots * (slot_layout(*params, as, false, pp, rsb).total - slot_layout(*params, as, false).total);
    return AIM_OK;
}

// rule 17c: what aim_mapper_set_pairing_secondary adds over all slots (without the estimate's buffers, as aim_mapper_pairing_device_bytes)
int aim_mapper_pairing_secondary_device_bytes(const aim_mapper_params_t *params, const aim_map_pair_params_t *pp, const aim_map_sec_params_t *sp, uint64_t *bytes)
{
    const char *fn = "aim_mapper_pairing_secondary_device_bytes";
    if (const int rc = check_mapper_params(fn, params, 0)) return rc;
    if (const int rc = check_pairing(fn, *params, pp)) return rc;
    if (const int rc = check_secondary(fn, sp)) return rc;
    if (!bytes) return fail(AIM_EINVAL, "%s: bytes is NULL", fn);
    const aim_endsfree_params_t ap = align_params(*params), rap = rescue_params(*params, *pp);
    const size_t as = aim_scratch_bytes(&ap.base, (uint32_t)((uint64_t)params->max_reads * (uint64_t)params->seed.max_cands));
    const size_t rsb = (pp->options & AIM_PAIR_RESCUE) ? aim_scratch_bytes(&rap.base, params->max_reads) : 0;
    if (!as || ((pp->options & AIM_PAIR_RESCUE) && !rsb)) return under(fn, AIM_ENOMEM);
    *bytes = (uint64_t)params->slots * (slot_layout(*params, as, false, pp, rsb, nullptr, true).total - slot_layout(*params, as, false).total);
    return AIM_OK;
}

}  // extern "C"

namespace {

// What the two setters of rules 14c / 15c refuse of the mapper's state: one the new setter has touched, one with secondaries, a second call.
int state_for_pairing(const char *fn, const aim_mapper *m)
{
    if (m->combined) return fail(AIM_EINVAL, "%s: the mapper pairs over secondaries (aim_mapper_set_pairing_secondary): it is paired already", fn);
    if (m->secondary) return fail(AIM_EINVAL, "%s: the mapper aligns secondaries (aim_mapper_set_secondary): aim_mapper_set_pairing_secondary switches both on, in one call on a fresh mapper", fn);
    if (m->paired) return fail(AIM_ESTATE, "%s: pairing is already set", fn);
    return AIM_OK;
}

// ... and the setter of rule 17c: a second call of its own, and a mapper any of the three earlier setters has touched.
int state_for_pairing_secondary(const char *fn, const aim_mapper *m)
{
    if (m->combined) return fail(AIM_ESTATE, "%s: pairing over secondaries is already set", fn);
    if (m->paired) return fail(AIM_EINVAL, "%s: the mapper is paired (aim_mapper_set_pairing): call this setter on a mapper no other setter has touched", fn);
    if (m->secondary) return fail(AIM_EINVAL, "%s: the mapper aligns secondaries (aim_mapper_set_secondary): call this setter on a mapper no other setter has touched", fn);
    return AIM_OK;
}

// aim_mapper_set_pairing and, with `estimate`, aim_mapper_set_pairing_estimated: the first's refusals, then ep's; with `sp`,
// aim_mapper_set_pairing_secondary (rule 17c): check_pairing, ep's rules where ep is given, check_secondary, then the mapper's state
int set_pairing(const char *fn, aim_mapper *m, const aim_map_pair_params_t *pp, bool estimate, const aim_pair_est_params_t *ep, const aim_map_sec_params_t *sp = nullptr,
                bool combined = false)
{
    if (!m) return fail(AIM_EINVAL, "%s: mapper is NULL", fn);
    if (const int rc = check_pairing(fn, m->p, pp)) return rc;
    if (estimate)
        if (const int rc = check_pair_est_params(fn, ep)) return rc;
    if (combined)
        if (const int rc = check_secondary(fn, sp)) return rc;
    if (const int rc = combined ? state_for_pairing_secondary(fn, m) : state_for_pairing(fn, m)) return rc;
    for (uint32_t i = 0; i < m->p.slots; ++i)
        if (m->slot[i].in_flight) return fail(AIM_ESTATE, "%s: slot %u is in flight (aim_mapper_wait first)", fn, i);
    HIP_TRY(hipSetDevice(m->device));
    const aim_mapper_params_t &p = m->p;
    const uint64_t N = p.max_reads, K = (uint64_t)p.seed.max_cands;
    const aim_endsfree_params_t rap = rescue_params(p, *pp);
    size_t rsb = 0;
    if (pp->options & AIM_PAIR_RESCUE) {
        rsb = aim_scratch_bytes(&rap.base, p.max_reads);
        if (!rsb) return under(fn, AIM_ENOMEM);
    }
    const SlotLayout L = slot_layout(p, m->align_scratch, !m->starts.empty(), pp, rsb, estimate ? ep : nullptr, combined);
    // Each slot moves to buffers of the new layout; nothing is in flight and no slot keeps state between batches. The new buffers come
    // first, so a failure leaves the mapper as it was.
    char *dev[AIM_MAPPER_MAX_SLOTS] = {};
    void *host[AIM_MAPPER_MAX_SLOTS][8] = {};
    int rc = AIM_OK;
    auto make = [&]() -> int {
        for (uint32_t i = 0; i < p.slots; ++i) {
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&dev[i]), (size_t)L.total));
            HIP_TRY(hipMemset(dev[i], 0, (size_t)L.total));
            const uint64_t sizes[5] = {4ull * ((uint64_t)p.cigar_cap + pp->rescue_cigar_cap), (uint64_t)p.md_cap + pp->rescue_md_cap, sizeof(aim_map_mate_t) * N * K,
                                       sizeof(aim_map_pair_t) * ((N + 1) / 2), 16};
            for (int j = 0; j < 5; ++j)
                if (const int r = pinned(&host[i][j], sizes[j])) return r;
            if (estimate)
                if (const int r = pinned(&host[i][5], sizeof(aim_pair_estimate_t))) return r;
            if (combined) {
                if (const int r = pinned(&host[i][6], sizeof(aim_map_sec_t) * N * K)) return r;
                if (const int r = pinned(&host[i][7], sizeof(aim_map_pair_mapq_t) * ((N + 1) / 2))) return r;
            }
        }
        HIP_TRY(hipDeviceSynchronize());
        return AIM_OK;
    };
    if ((rc = make())) {
        const std::string was = aim_last_error();
        for (uint32_t i = 0; i < p.slots; ++i) {
            if (dev[i]) (void)hipFree(dev[i]);
            for (void *h : host[i])
                if (h) (void)hipHostFree(h);
        }
        return fail(rc, "%s: %s", fn, was.c_str());
    }
    for (uint32_t i = 0; i < p.slots; ++i) {
        MapperSlot &s = m->slot[i];
        (void)hipFree(s.dev);
        (void)hipHostFree(s.h_cigar);
        (void)hipHostFree(s.h_md);
        s.dev = dev[i];
        s.h_cigar = static_cast<uint32_t *>(host[i][0]); s.h_md = static_cast<char *>(host[i][1]);
        s.h_mates = static_cast<aim_map_mate_t *>(host[i][2]); s.h_pairs = static_cast<aim_map_pair_t *>(host[i][3]); s.h_res_head = static_cast<uint32_t *>(host[i][4]);
        s.h_est = static_cast<aim_pair_estimate_t *>(host[i][5]);
        if (combined) {
            s.h_sec = static_cast<aim_map_sec_t *>(host[i][6]);
            s.h_pair_mapq = static_cast<aim_map_pair_mapq_t *>(host[i][7]);
        }
        s.waited = false;
    }
    m->L = L;
    if (estimate) {
        m->estimated = true;
        m->ep = *ep;
    }
    m->pp = *pp;
    m->rap = rap;
    m->rescue_scratch = rsb;
    m->paired = true;
    if (combined) {
        m->sc = *sp;
        m->secondary = true;
        m->combined = true;
    }
    return AIM_OK;
}

}  // namespace

extern "C" {

int aim_mapper_set_pairing(aim_mapper_t *m, const aim_map_pair_params_t *pp) { return set_pairing("aim_mapper_set_pairing", m, pp, false, nullptr); }

// rule 15c (AIM_FEATURE_PAIR_ESTIMATE): pairing with the span bounds estimated per batch on the device
int aim_mapper_set_pairing_estimated(aim_mapper_t *m, const aim_map_pair_params_t *pp, const aim_pair_est_params_t *ep)
{
    return set_pairing("aim_mapper_set_pairing_estimated", m, pp, true, ep);
}

// rule 17c (AIM_FEATURE_PAIR_SECONDARY): pairing, the estimate when ep is given, and secondaries in one call
int aim_mapper_set_pairing_secondary(aim_mapper_t *m, const aim_map_pair_params_t *pp, const aim_pair_est_params_t *ep, const aim_map_sec_params_t *sp)
{
    return set_pairing("aim_mapper_set_pairing_secondary", m, pp, ep != nullptr, ep, sp, true);
}

int aim_mapper_pair_mapq(aim_mapper_t *m, uint32_t slot, const aim_map_pair_mapq_t **out)
{
    const char *fn = "aim_mapper_pair_mapq";
    if (!m) return fail(AIM_EINVAL, "%s: mapper is NULL", fn);
    if (slot >= m->p.slots) return fail(AIM_EINVAL, "%s: slot %u is outside 0..%u", fn, slot, m->p.slots - 1);
    if (!out) return fail(AIM_EINVAL, "%s: out is NULL", fn);
    if (!m->combined) return fail(AIM_ESTATE, "%s: aim_mapper_set_pairing_secondary was not called", fn);
    const MapperSlot &s = m->slot[slot];
    if (s.in_flight || !s.waited) return fail(AIM_ESTATE, "%s: slot %u has no batch waited for (aim_mapper_wait first)", fn, slot);
    *out = s.h_pair_mapq;                // [aim_mapper_pairs' n_pairs]
    return AIM_OK;
}

int aim_mapper_pair_estimate(aim_mapper_t *m, uint32_t slot, aim_pair_estimate_t *out)
{
    const char *fn = "aim_mapper_pair_estimate";
    if (!m) return fail(AIM_EINVAL, "%s: mapper is NULL", fn);
    if (slot >= m->p.slots) return fail(AIM_EINVAL, "%s: slot %u is outside 0..%u", fn, slot, m->p.slots - 1);
    if (!out) return fail(AIM_EINVAL, "%s: out is NULL", fn);
    if (!m->estimated) return fail(AIM_ESTATE, "%s: aim_mapper_set_pairing_estimated was not called", fn);
    const MapperSlot &s = m->slot[slot];
    if (s.in_flight || !s.waited) return fail(AIM_ESTATE, "%s: slot %u has no batch waited for (aim_mapper_wait first)", fn, slot);
    *out = *s.h_est;
    return AIM_OK;
}

int aim_mapper_pairs(aim_mapper_t *m, uint32_t slot, aim_mapper_pairs_out_t *out)
{
    const char *fn = "aim_mapper_pairs";
    if (!m) return fail(AIM_EINVAL, "%s: mapper is NULL", fn);
    if (slot >= m->p.slots) return fail(AIM_EINVAL, "%s: slot %u is outside 0..%u", fn, slot, m->p.slots - 1);
    if (!out) return fail(AIM_EINVAL, "%s: out is NULL", fn);
    if (!m->paired) return fail(AIM_ESTATE, "%s: aim_mapper_set_pairing was not called", fn);
    const MapperSlot &s = m->slot[slot];
    if (s.in_flight || !s.waited) return fail(AIM_ESTATE, "%s: slot %u has no batch waited for (aim_mapper_wait first)", fn, slot);
    *out = s.po;
    return AIM_OK;
}

// ---------------------------------------------------------------------------
// aligned secondaries (AIM_FEATURE_SECONDARY; rule 16c in aim_hip.h, the kernels in secondary.hpp, the stateless entry points in
// capi_secondary.hip)
// ---------------------------------------------------------------------------
int aim_mapper_secondary_device_bytes(const aim_mapper_params_t *params, const aim_map_sec_params_t *sp, uint64_t *bytes)
{
    const char *fn = "aim_mapper_secondary_device_bytes";
    if (const int rc = check_mapper_params(fn, params, 0)) return rc;
    if (const int rc = check_secondary(fn, sp)) return rc;
    if (!bytes) return fail(AIM_EINVAL, "%s: bytes is NULL", fn);
    // (the difference does not depend on the alignment's scratch, nor on the kind of mapper)
    *bytes = (uint64_t)params->slots * (slot_layout(*params, 0, false, nullptr, 0, nullptr, true).total - slot_layout(*params, 0, false).total);
    return AIM_OK;
}

int aim_mapper_set_secondary(aim_mapper_t *m, const aim_map_sec_params_t *sp)
{
    const char *fn = "aim_mapper_set_secondary";
    if (const int rc = check_secondary(fn, sp)) return rc;
    if (!m) return fail(AIM_EINVAL, "%s: mapper is NULL", fn);
    if (m->secondary) return fail(AIM_EINVAL, "%s: secondaries are already set", fn);
    for (uint32_t i = 0; i < m->p.slots; ++i)
        if (m->slot[i].in_flight) return fail(AIM_EINVAL, "%s: slot %u is in flight (aim_mapper_wait first)", fn, i);
    if (m->paired) return fail(AIM_EINVAL, "%s: the mapper is paired (aim_mapper_set_pairing): aim_mapper_set_pairing_secondary switches both on, in one call on a fresh mapper", fn);
    HIP_TRY(hipSetDevice(m->device));
    const aim_mapper_params_t &p = m->p;
    const SlotLayout L = slot_layout(p, m->align_scratch, !m->starts.empty(), nullptr, 0, nullptr, true);
    // As in aim_mapper_set_pairing: each slot moves to buffers of the new layout, the new buffers come first, a failure leaves the mapper as it was.
    char *dev[AIM_MAPPER_MAX_SLOTS] = {};
    aim_map_sec_t *host[AIM_MAPPER_MAX_SLOTS] = {};
    auto make = [&]() -> int {
        for (uint32_t i = 0; i < p.slots; ++i) {
            HIP_TRY(hipMalloc(reinterpret_cast<void **>(&dev[i]), (size_t)L.total));
            HIP_TRY(hipMemset(dev[i], 0, (size_t)L.total));
            if (const int r = pinned(&host[i], sizeof(aim_map_sec_t) * (uint64_t)p.max_reads * (uint64_t)p.seed.max_cands)) return r;
        }
        HIP_TRY(hipDeviceSynchronize());
        return AIM_OK;
    };
    if (const int rc = make()) {
        const std::string was = aim_last_error();
        for (uint32_t i = 0; i < p.slots; ++i) {
            if (dev[i]) (void)hipFree(dev[i]);
            if (host[i]) (void)hipHostFree(host[i]);
        }
        return fail(rc, "%s: %s", fn, was.c_str());
    }
    for (uint32_t i = 0; i < p.slots; ++i) {
        MapperSlot &s = m->slot[i];
        (void)hipFree(s.dev);
        s.dev = dev[i];
        s.h_sec = host[i];
        s.waited = false;
    }
    m->L = L;
    m->sc = *sp;
    m->secondary = true;
    return AIM_OK;
}

int aim_mapper_secondary(aim_mapper_t *m, uint32_t slot, aim_mapper_secondary_out_t *out)
{
    const char *fn = "aim_mapper_secondary";
    if (!m) return fail(AIM_EINVAL, "%s: mapper is NULL", fn);
    if (slot >= m->p.slots) return fail(AIM_EINVAL, "%s: slot %u is outside 0..%u", fn, slot, m->p.slots - 1);
    if (!out) return fail(AIM_EINVAL, "%s: out is NULL", fn);
    if (!m->secondary) return fail(AIM_ESTATE, "%s: aim_mapper_set_secondary was not called", fn);
    const MapperSlot &s = m->slot[slot];
    if (s.in_flight || !s.waited) return fail(AIM_ESTATE, "%s: slot %u has no batch waited for (aim_mapper_wait first)", fn, slot);
    out->n_records = s.n_records;
    out->pad = 0;
    out->sec = s.h_sec;
    return AIM_OK;
}

int aim_mapper_free(aim_mapper_t *m)
{
    if (!m) return AIM_OK;
    (void)hipSetDevice(m->device);
    release(m);
    return AIM_OK;
}

}  // extern "C"
