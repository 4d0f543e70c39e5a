// secondary.hpp -- the device side of AIM_FEATURE_SECONDARY (aim_hip.h, rule 16c): the secondaries of a locus aligned next to their
// primary, one winner per locus by alignment score with a MAPQ from the runner-up, and the record list over loci.
//
//   * secondary_rows_kernel (part 1), behind split_segments_kernel / the extension, in place on the four segment buffers: per read,
//     which secondaries get a row (their index among their parent's secondaries, the parent's segment, the recovered p_lo), the
//     window of each along its own chain's end diagonals over the parent's read interval, and the pattern rows of those slots.
//   * secondary_select_kernel (part 2), behind the SAM kernel: per read, the families (a primary and its valid secondaries), the
//     winner of each by (score, i), the runner-up, the ties and the MAPQ -> aim_sec_slot_t per slot.
//   * map_count_sec_kernel / map_records_sec_kernel (part 3): mapper.hpp's pair keyed on aim_sec_slot_t.role instead of "mapped":
//     c_r -> rec_offsets, the scan (index.hpp), then every record at rec_offsets[r] + rank as four 16-byte stores and its
//     aim_map_sec_t as one. The record kernel takes rule 13c's contig table as an optional argument.
//
// Every kernel gives a read G = 4, 8 or 16 consecutive lanes by K (chain_class_lanes), candidate i in lane i of the group; what a
// candidate needs of another comes from shuffles inside the group, and sets of candidates are the group's bits of one wave ballot. A
// group never leaves a 16-lane row. Every loop that holds a shuffle or a ballot has a workgroup-uniform bound (K, the block walk), and
// every branch around one is uniform over the group, so the lanes a shuffle reads are active with it.
//   secondary_rows_kernel reaches the parent's segment by one shuffle from the parent's lane. Its pattern rows are gathered as
//   split_segments_kernel gathers them -- byte-shifted 8-byte units, three aligned dword loads and two alignbyte's each -- but row by
//   row: only the rows of secondaries are written, so the group walks the K slots, and a slot with a row is a flat walk of its
//   read_size / 8 units by the group's lanes. Long rows are cut into `parts` interleaved shares (a power of two from K's group width
//   and read_size alone), each walked by a group of its own, which repeats the cheap decision and leaves the per-slot records to
//   share 0. A wavefront none of whose reads has such a row -- a batch without repeats -- skips the walk. The kernel writes the slots
//   of secondaries only and reads d_seg of primaries only, so no share reads what another writes.
// Measured (profiles/secondary/README.md, 1 Mi reads of 100 bases, K = 4): 96 / 81 / 11 / 89 us for the four kernels on a batch without
// repeats, 318 / 85 / 11 / 134 us where every read has a secondary; 0.06 - 0.34 of the 8 TB/s roofline in algorithmic bytes. No LDS, no scratch, no atomics, vector stores only; an output byte has exactly one writer.
#pragma once

#include <climits>

#include "aim_device.hpp"
#include "chain_class.hpp"

namespace aim {

constexpr int kSecMaxVgpr = 64;             // 8 wavefronts per SIMD; the bound tests/test_secondary_cpu.py checks in the code object
constexpr int kSecThreads = 256;
constexpr uint32_t kSecPerCu = 8;           // workgroups per compute unit of the resident grid: 32 wavefronts
constexpr uint32_t kSecShareSteps = 16;     // steps of a group over one share of a row

struct SecRowsArgs {
    uint32_t K, read_size, n_reads, parts_log2, max_sec;
    int64_t flank, ref_len;
    const int32_t *read_len;
    const char *reads;
    const aim_request_t *requests;
    const uint64_t *text_pos;
    const aim_seed_t *seed;
    const aim_chain_t *chains;
    const aim_chain_class_t *cls;
    aim_request_t *seg_requests;
    uint64_t *seg_text_pos;
    char *seg_patterns;
    aim_segment_t *seg;
};

struct SecSelectArgs {
    uint32_t K, n_reads;
    int32_t max_score, score_unit;
    const aim_segment_t *seg;
    const aim_sam_t *sam;
    const aim_chain_class_t *cls;
    const aim_chain_t *chains;
    aim_sec_slot_t *sec;
};

struct MapSecArgs {
    uint32_t K, n_reads, options, n_contigs;
    const aim_segment_t *seg;
    const aim_sam_t *sam;
    const aim_chain_class_t *cls;
    const aim_sec_slot_t *sec;
    const uint32_t *contig;              // or nullptr: a reference of one sequence
    const uint32_t *contig_start;
    uint32_t *rec_offsets;               // [n_reads + 1]: counts after map_count_sec_kernel, offsets after the scan
    aim_map_record_t *records;
    aim_map_sec_t *sec_records;
};

// Shares per row: a function of the group width and read_size alone, never of the grid.
inline uint32_t sec_parts_log2(uint32_t lanes, uint32_t read_size)
{
    const uint32_t units = read_size / 8u;
    uint32_t lg = 0;
    while (lg < 6u && (units >> lg) > kSecShareSteps * lanes) ++lg;
    return lg;
}

#ifdef AIM_TU_SECONDARY   // the kernels live in tu_secondary.hip alone; capi_secondary.hip sees the arguments and the launchers

static_assert(sizeof(aim_sec_slot_t) == 8 && sizeof(aim_map_sec_t) == 16 && sizeof(aim_segment_t) == 8 && sizeof(aim_chain_class_t) == 8 &&
              sizeof(aim_sam_t) == 48 && sizeof(aim_map_record_t) == 64 && sizeof(aim_request_t) == 16 && sizeof(aim_chain_t) == 16,
              "rows as rule 16c lays them out");

constexpr uint32_t kSecKind = AIM_CHAIN_PRIMARY | AIM_CHAIN_SECONDARY;

// G: lanes per read, 4, 8 or 16 and at least K (workgroup-uniform).
__global__ __launch_bounds__(kSecThreads) void secondary_rows_kernel(SecRowsArgs a, uint32_t G)
{
    const uint32_t kGroups = kSecThreads / G;                     // (read, share) items per workgroup
    const uint32_t sub = threadIdx.x & (G - 1u);
    const uint32_t parts = 1u << a.parts_log2;
    const uint64_t n_items = (uint64_t)a.n_reads << a.parts_log2;
    const uint64_t n_blocks = (n_items + kGroups - 1u) / kGroups;
    const uint32_t U = a.read_size >> 3;                          // units per row
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t item = blk * kGroups + threadIdx.x / G;
        const bool item_live = item < n_items;
        const uint64_t r = item_live ? item >> a.parts_log2 : 0;
        const uint32_t part = (uint32_t)item & (parts - 1u);
        const bool live = item_live && sub < a.K;
        const uint64_t slot = r * a.K + sub;

        // ---- the decision: lane i < K of the group holds slot i ----
        int32_t L = 0;
        uint32_t kind = 0, parent = 0, sg0 = 0, sg1 = 0;
        aim_chain_t c = {0u, 0, 0, 0, 0, 0u};
        aim_request_t rq = {0, 0, 0, 0u};
        uint64_t tp = 0;
        if (live) {
            const uint32_t n = min(a.seed[r].n_cands, a.K);
            L = min(max(a.read_len[r], 0), (int32_t)a.read_size);
            const uint32_t c1 = reinterpret_cast<const uint32_t *>(a.cls)[slot * 2u + 1u];   // parent | flags << 8 | mapq << 16 | n_sub << 24
            parent = c1 & 0xffu;
            kind = sub < n ? (c1 >> 8) & kSecKind : 0u;           // 0 beyond the kept candidates
            if (kind == AIM_CHAIN_PRIMARY) {                      // (only a primary's segment is ever read: no share reads what share 0 writes)
                const uint2 sg = reinterpret_cast<const uint2 *>(a.seg)[slot];
                sg0 = sg.x;
                sg1 = sg.y;
            } else if (kind == AIM_CHAIN_SECONDARY) {
                c = a.chains[slot];
                tp = a.text_pos[slot];
                rq = a.requests[slot];
            }
        }
        const bool secondary = kind == AIM_CHAIN_SECONDARY;
        uint32_t t = 0;                                           // my index among my parent's secondaries
        const uint32_t mine = secondary ? parent : 0x100u + sub;  // (a key no other lane's parent equals)
        for (uint32_t j = 0; j < a.K; ++j) {
            const uint32_t key_j = (uint32_t)__shfl((int)mine, (int)j, (int)G);
            t += (j < sub && key_j == mine) ? 1u : 0u;
        }
        const int src = (int)(parent & (G - 1u));
        const uint32_t p0 = (uint32_t)__shfl((int)sg0, src, (int)G), p1 = (uint32_t)__shfl((int)sg1, src, (int)G);
        const uint32_t pkind = (uint32_t)__shfl((int)kind, src, (int)G);
        const int32_t qa = (int32_t)(p0 & 0xffffu), qb = (int32_t)(p0 >> 16);
        const uint32_t pflags = (p1 >> 16) & 0xffu;
        const bool minus = (tp >> 63) != 0;
        const int64_t start = (int64_t)(tp & ~AIM_REF_MINUS_STRAND), E = start + (int64_t)rq.text_len;
        int64_t p_lo = 0;
        bool recoverable = true;
        if (start > 0) p_lo = start + (int64_t)c.q_lo + a.flank;
        else if (rq.text_len > 0 && rq.text_len < (int32_t)a.read_size && E < a.ref_len)
            p_lo = E - ((int64_t)L - (int64_t)c.q_hi) - a.flank - (int64_t)c.ref_span;
        else recoverable = false;
        const bool row = secondary && parent < a.K && t < a.max_sec && pkind == AIM_CHAIN_PRIMARY && (pflags & AIM_SEG_VALID) != 0 && qa <= qb && qb <= L &&
                         recoverable;
        if (row && part == 0) {
            const int64_t u = minus ? (int64_t)L - qb : (int64_t)qa, v = minus ? (int64_t)L - qa : (int64_t)qb;
            const int64_t lo = p_lo + (u - (int64_t)c.q_lo) - a.flank;
            const int64_t hi = p_lo + (int64_t)c.ref_span + (v - (int64_t)c.q_hi) + a.flank;
            const int64_t seg_start = min(max(lo, (int64_t)0), a.ref_len);
            const int64_t seg_end = max(seg_start, min(max(hi, (int64_t)0), a.ref_len));
            const aim_request_t o = {qb - qa, (int32_t)min(seg_end - seg_start, (int64_t)a.read_size), 0, rq.idx};
            const uint32_t flags = pflags & (AIM_SEG_VALID | AIM_SEG_SUPPLEMENTARY | AIM_SEG_LEFT_OPEN | AIM_SEG_RIGHT_OPEN);
            a.seg_requests[slot] = o;
            a.seg_text_pos[slot] = (uint64_t)seg_start | (minus ? AIM_REF_MINUS_STRAND : 0ull);
            reinterpret_cast<uint2 *>(a.seg)[slot] = make_uint2(p0, (uint32_t)L | flags << 16 | sub << 24);   // (one dwordx2 store per row)
        }

        // ---- the rows of the slots that got one: bytes [8t, 8t + 8) of read[qa, qb), zero behind it ----
        if (!__ballot(row)) continue;                             // (uniform over the wavefront: no read of it has such a row)
        const uint32_t span = row ? ((uint32_t)qa | (uint32_t)(qb - qa) << 16) : 0xffffffffu;   // (both at most 65 528; all ones: no row)
        const uint32_t *srcw = reinterpret_cast<const uint32_t *>(a.reads + r * a.read_size);
        for (uint32_t i = 0; i < a.K; ++i) {
            const uint32_t sp = (uint32_t)__shfl((int)span, (int)i, (int)G);
            if (sp == 0xffffffffu) continue;                      // (uniform over the group)
            const uint32_t off = sp & 0xffffu, len = sp >> 16;
            const uint32_t end = off + len;                       // one past the interval's last source byte, at most L <= read_size
            uint2 *dst = reinterpret_cast<uint2 *>(a.seg_patterns + (r * a.K + i) * a.read_size);
            for (uint32_t tt = part * G + sub; tt < U; tt += parts * G) {
                const uint32_t at = off + 8u * tt;                // first source byte of the unit
                const uint32_t w = at >> 2, sh = at & 3u;
                // only dwords that hold a byte of [off, end) are loaded, and those lie inside the row
                const uint32_t d0 = 4u * w < end ? srcw[w] : 0u;
                const uint32_t d1 = 4u * (w + 1u) < end ? srcw[w + 1u] : 0u;
                const uint32_t d2 = (sh && 4u * (w + 2u) < end) ? srcw[w + 2u] : 0u;
                uint2 val;
                val.x = __builtin_amdgcn_alignbyte(d1, d0, sh);
                val.y = __builtin_amdgcn_alignbyte(d2, d1, sh);
                const int32_t keep = (int32_t)len - 8 * (int32_t)tt;   // bytes of the unit inside the interval; zero behind it
                if (keep < 8) {
                    val.y = keep <= 4 ? 0u : (val.y & (0xffffffffu >> (8 * (8 - keep))));
                    val.x = keep <= 0 ? 0u : keep >= 4 ? val.x : (val.x & (0xffffffffu >> (8 * (4 - keep))));
                }
                dst[tt] = val;
            }
        }
    }
}

__global__ __launch_bounds__(kSecThreads) void secondary_select_kernel(SecSelectArgs a, uint32_t G)
{
    const uint32_t kReads = kSecThreads / G;
    const uint32_t cand = threadIdx.x & (G - 1u);
    const uint64_t n_blocks = ((uint64_t)a.n_reads + kReads - 1u) / kReads;
    constexpr uint32_t kNone = 0xffu;
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t r = blk * kReads + threadIdx.x / G;
        const bool live = r < a.n_reads && cand < a.K;
        const uint64_t slot = r * a.K + cand;
        uint32_t c1 = 0, kind = 0, cap = 0;
        int32_t score = 0;
        bool valid = false, mapped = false, ok = false;
        if (live) {
            c1 = reinterpret_cast<const uint32_t *>(a.cls)[slot * 2u + 1u];
            kind = (c1 >> 8) & kSecKind;
            const uint32_t s1 = reinterpret_cast<const uint32_t *>(a.seg)[slot * 2u + 1u];
            const uint32_t *row = reinterpret_cast<const uint32_t *>(a.sam) + slot * 12u;
            const uint32_t fs = row[10];                          // flags | status << 16
            score = (int32_t)row[1];
            valid = ((s1 >> 16) & AIM_SEG_VALID) != 0;
            mapped = valid && !(fs & AIM_SAM_UNMAPPED);
            ok = ((fs >> 16) & ~AIM_SAM_OVERFLOW & 0xffffu) == AIM_PAIR_OK;
            const uint32_t *ch = reinterpret_cast<const uint32_t *>(a.chains) + slot * 4u;   // score, n_anchors | reserved << 16
            cap = ch[0] ? 6u * min(ch[1] & 0xffffu, 10u) : 0u;
        }
        const uint32_t parent = c1 & 0xffu;
        const uint32_t pkind = (uint32_t)__shfl((int)kind, (int)(parent & (G - 1u)), (int)G);
        uint32_t fam = kNone;                                     // the primary my family hangs on
        if (kind == AIM_CHAIN_PRIMARY) fam = cand;
        else if (kind == AIM_CHAIN_SECONDARY && valid && parent < a.K && pkind == AIM_CHAIN_PRIMARY) fam = parent;
        const int32_t e = mapped ? score : a.max_score + 1;       // the counted score (max_score is below INT32_MAX)
        const uint32_t st = fam | (mapped ? 0x100u : 0u) | ((valid && ok) ? 0x200u : 0u);
        // the winner of my family: its mapped member of lowest (score, i); and the members
        int64_t b = 0;
        uint32_t w = kNone, n_members = 0, wcap = 0;
        for (uint32_t j = 0; j < a.K; ++j) {
            const uint32_t st_j = (uint32_t)__shfl((int)st, (int)j, (int)G);
            const int32_t sc_j = __shfl(score, (int)j, (int)G);
            const uint32_t cap_j = (uint32_t)__shfl((int)cap, (int)j, (int)G);
            if (fam == kNone || (st_j & 0xffu) != fam) continue;
            ++n_members;
            if ((st_j & 0x100u) && (w == kNone || (int64_t)sc_j < b)) {   // (ascending j: the first of equal scores stays)
                w = j;
                b = sc_j;
                wcap = cap_j;
            }
        }
        // the runner-up and the ties among the other valid and OK members
        int64_t s2 = INT_MAX;
        uint32_t n_tied = 1;
        bool runner = false;
        for (uint32_t j = 0; j < a.K; ++j) {
            const uint32_t st_j = (uint32_t)__shfl((int)st, (int)j, (int)G);
            const int64_t e_j = __shfl(e, (int)j, (int)G);
            if (w == kNone || (st_j & 0xffu) != fam || j == w || !(st_j & 0x200u)) continue;
            runner = true;
            s2 = min(s2, e_j);
            n_tied += e_j == b ? 1u : 0u;
        }
        const uint32_t fc1 = (uint32_t)__shfl((int)c1, (int)(fam & (G - 1u)), (int)G);   // d_class of the family's primary
        uint2 out = make_uint2(0u, 0u);
        if (w != kNone && mapped) {                               // (w != kNone implies a family)
            const uint64_t gap = (uint64_t)max(s2 - b, (int64_t)0);
            const uint32_t aln = n_tied > 1u ? 0u : !runner ? 60u : quot60(6ull * gap, (uint64_t)a.score_unit);
            const bool complete = n_members - 1u == (fc1 >> 24);
            uint32_t mapq = min(aln, wcap);
            if (!complete) mapq = min(mapq, (fc1 >> 16) & 0xffu);
            const uint32_t flags = (w != fam ? AIM_SEC_SWAPPED : 0u) | (complete ? AIM_SEC_COMPLETE : 0u) | (n_members - 1u) << 4;
            const uint32_t role = cand == w ? 1u : 2u;
            out.x = role | fam << 8 | (role == 1u ? mapq : 0u) << 16 | aln << 24;
            out.y = n_tied | flags << 8 | (runner ? (uint32_t)min(gap, (uint64_t)65534u) : 65535u) << 16;
        }
        if (live) reinterpret_cast<uint2 *>(a.sec)[slot] = out;
    }
}

// What part 3 reads of a slot, and the read's records as the group's bits of two ballots.
struct SecSlot {
    uint32_t s0, s1;                     // aim_sec_slot_t as its two dwords: role | family << 8 | mapq << 16 | aln_mapq << 24, n_tied | flags << 8 | gap << 16
    uint32_t locus, second;              // bit i: candidate i gives a locus record / a secondary record
};

__device__ __forceinline__ SecSlot sec_slot(const MapSecArgs &a, bool live, uint64_t slot, uint32_t base, uint32_t G)
{
    SecSlot s = {0u, 0u, 0u, 0u};
    if (live) {
        const uint2 v = reinterpret_cast<const uint2 *>(a.sec)[slot];
        s.s0 = v.x;
        s.s1 = v.y;
    }
    const uint32_t role = s.s0 & 0xffu;
    s.locus = (uint32_t)(__ballot(role == 1u) >> base) & ((1u << G) - 1u);
    s.second = (uint32_t)(__ballot(role == 2u && (a.options & AIM_SEC_RECORDS)) >> base) & ((1u << G) - 1u);
    if (!s.locus) s.second = 0u;         // (part 2 never writes a secondary record without its locus record; nor does a record land outside c_r)
    return s;
}

__global__ __launch_bounds__(kSecThreads) void map_count_sec_kernel(MapSecArgs a, uint32_t G)
{
    const uint32_t kReads = kSecThreads / G;
    const uint32_t cand = threadIdx.x & (G - 1u);
    const uint32_t base = (threadIdx.x & (uint32_t)(kWave - 1)) & ~(G - 1u);
    const uint64_t n_blocks = ((uint64_t)a.n_reads + kReads - 1u) / kReads;
    if (blockIdx.x == 0 && threadIdx.x == 0) a.rec_offsets[a.n_reads] = 0u;     // the scan's last entry: the total lands here
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t r = blk * kReads + threadIdx.x / G;
        const bool live = r < a.n_reads && cand < a.K;
        const SecSlot s = sec_slot(a, live, r * a.K + cand, base, G);
        if (r < a.n_reads && cand == 0) a.rec_offsets[r] = s.locus ? (uint32_t)__popc(s.locus) + (uint32_t)__popc(s.second) : 1u;
    }
}

__global__ __launch_bounds__(kSecThreads) void map_records_sec_kernel(MapSecArgs a, uint32_t G)
{
    const uint32_t kReads = kSecThreads / G;
    const uint32_t cand = threadIdx.x & (G - 1u);
    const uint32_t base = (threadIdx.x & (uint32_t)(kWave - 1)) & ~(G - 1u);
    const uint64_t n_blocks = ((uint64_t)a.n_reads + kReads - 1u) / kReads;
    for (uint64_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint64_t r = blk * kReads + threadIdx.x / G;
        const bool live = r < a.n_reads && cand < a.K;
        const uint64_t slot = r * a.K + cand;
        const SecSlot s = sec_slot(a, live, slot, base, G);
        const bool is1 = (s.locus >> cand) & 1u, is2 = (s.second >> cand) & 1u;
        const uint32_t fam = min((s.s0 >> 8) & 0xffu, a.K - 1u);              // (part 2's j is below K: no load outside the read's slots)
        uint32_t seg0 = 0, seg1 = 0;
        int32_t score = 0;
        if (is1 || is2) {
            const uint2 sg = reinterpret_cast<const uint2 *>(a.seg)[slot];
            seg0 = sg.x;
            seg1 = sg.y;
            score = (int32_t)reinterpret_cast<const uint32_t *>(a.sam)[slot * 12u + 1u];
        }
        const uint32_t q = seg0 & 0xffffu;
        // the locus records by (q_begin, j); every lane learns the rank and the score of its family's locus record
        uint32_t rank = 0, fam_rank = 0, rep = 0xffu;
        int32_t b = 0;
        for (uint32_t j = 0; j < a.K; ++j) {                                  // rank of candidate j: the locus keys below its own
            const uint32_t q_j = (uint32_t)__shfl((int)q, (int)j, (int)G), fam_j = (uint32_t)__shfl((int)fam, (int)j, (int)G);
            const int32_t sc_j = __shfl(score, (int)j, (int)G);
            const bool below = is1 && (q < q_j || (q == q_j && fam < fam_j));
            const uint32_t rank_j = (uint32_t)__popc((uint32_t)(__ballot(below) >> base) & ((1u << G) - 1u));
            if (!((s.locus >> j) & 1u)) continue;                             // (uniform over the group)
            rep = min(rep, fam_j);                                            // the family of lowest j with a winner: the one non-supplementary line
            if (fam_j == fam) {
                fam_rank = rank_j;
                b = sc_j;
            }
            if (cand == j) rank = rank_j;
        }
        // the secondary records behind them by (rank of the family, score, i)
        const uint32_t n_locus = (uint32_t)__popc(s.locus);
        for (uint32_t j = 0; j < a.K; ++j) {
            const uint32_t fr_j = (uint32_t)__shfl((int)fam_rank, (int)j, (int)G);
            const int32_t sc_j = __shfl(score, (int)j, (int)G);
            const bool below = is2 && (fam_rank < fr_j || (fam_rank == fr_j && (score < sc_j || (score == sc_j && cand < j))));
            const uint32_t bits = (uint32_t)(__ballot(below) >> base) & ((1u << G) - 1u);
            if (cand == j && is2) rank = n_locus + (uint32_t)__popc(bits);
        }
        const bool unmapped_read = live && cand == 0 && !s.locus;             // its one record comes from candidate 0's row
        if (is1 || is2 || unmapped_read) {                                    // (an if, not a continue: every lane reaches the next round's ballots)
            const uint4 *row = reinterpret_cast<const uint4 *>(a.sam) + slot * 3u;
            uint4 w0 = row[0], w1 = row[1], w2 = row[2], w3, x;
            if (!unmapped_read) {
                const uint32_t fs = w2.z;
                const uint32_t flags = is2 ? ((fs & ~AIM_SAM_SUPPLEMENTARY) | AIM_SAM_SECONDARY) : fam == rep ? (fs & ~AIM_SAM_SUPPLEMENTARY) : (fs | AIM_SAM_SUPPLEMENTARY);
                const uint32_t n_rec = n_locus + (uint32_t)__popc(s.second);
                w2.z = flags;
                w3.x = (uint32_t)r;
                w3.y = seg0;
                w3.z = (is1 ? (s.s0 >> 16) & 0xffu : 0u) | ((seg1 >> 16) & 0xffu) << 8 | rank << 16 | n_rec << 24;
                if (a.contig) {                                                         // rule 13c: the contig-local position and the contig
                    const uint32_t c = a.contig[slot];
                    const uint64_t pos = ((uint64_t)w0.w << 32 | w0.z) - (c < a.n_contigs ? a.contig_start[c] : 0u);   // (no load outside the table)
                    w0.z = (uint32_t)pos;
                    w0.w = (uint32_t)(pos >> 32);
                    w2.w = c;                                                           // pad
                }
                const uint32_t fslot = (uint32_t)(r * a.K) + fam;
                const uint32_t fc1 = reinterpret_cast<const uint32_t *>(a.cls)[(uint64_t)fslot * 2u + 1u];
                const uint32_t gap = s.s1 >> 16, sflags = (s.s1 >> 8) & 0xffu;
                const int64_t second = gap == 65535u ? (int64_t)INT_MAX : min((int64_t)b + (int64_t)gap, (int64_t)INT_MAX - 1);
                x = make_uint4(fslot, (uint32_t)(int32_t)second, (s.s0 >> 24) | ((fc1 >> 16) & 0xffu) << 8 | ((sflags >> 4) + 1u) << 16 | (s.s1 & 0xffu) << 24,
                               sflags & (AIM_SEC_SWAPPED | AIM_SEC_COMPLETE));
            } else {
                w0.z = w0.w = 0u;                                                       // pos
                w1 = make_uint4(0u, 0u, 0u, 0u);                                        // ref_span, nm, cigar_offset, n_cigar
                w2.x = w2.y = 0u;                                                       // md_offset, md_len
                w2.z = AIM_SAM_UNMAPPED | (w2.z & 0xffff0000u);                         // status is kept
                if (a.contig) w2.w = AIM_CONTIG_NONE;                                   // rule 13c: pad of an unmapped read
                w3.x = (uint32_t)r;
                w3.y = 0u;
                w3.z = 1u << 24;
                x = make_uint4((uint32_t)slot, (uint32_t)INT_MAX, 0u, 0u);
            }
            w3.w = (uint32_t)slot;                                                      // (n_reads * K fits 32 bits)
            const uint64_t at = (uint64_t)a.rec_offsets[r] + (unmapped_read ? 0u : rank);
            uint4 *out = reinterpret_cast<uint4 *>(a.records) + at * 4u;
            out[0] = w0;
            out[1] = w1;
            out[2] = w2;
            out[3] = w3;
            reinterpret_cast<uint4 *>(a.sec_records)[at] = x;
        }
    }
}

void secondary_rows_launch(const SecRowsArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s)
{
    hipLaunchKernelGGL(secondary_rows_kernel, dim3(grid), dim3(kSecThreads), 0, s, a, lanes);
}

void secondary_select_launch(const SecSelectArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s)
{
    hipLaunchKernelGGL(secondary_select_kernel, dim3(grid), dim3(kSecThreads), 0, s, a, lanes);
}

void map_count_sec_launch(const MapSecArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s)
{
    hipLaunchKernelGGL(map_count_sec_kernel, dim3(grid), dim3(kSecThreads), 0, s, a, lanes);
}

void map_records_sec_launch(const MapSecArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s)
{
    hipLaunchKernelGGL(map_records_sec_kernel, dim3(grid), dim3(kSecThreads), 0, s, a, lanes);
}
#else
void secondary_rows_launch(const SecRowsArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s);
void secondary_select_launch(const SecSelectArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s);
void map_count_sec_launch(const MapSecArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s);
void map_records_sec_launch(const MapSecArgs &a, uint32_t lanes, uint32_t grid, hipStream_t s);
#endif

}  // namespace aim
