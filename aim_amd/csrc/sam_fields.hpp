// sam_fields.hpp -- AIM_FLAG_SAM_FIELDS / aim_sam_device: SAM-ready records from the final ops rows and the resident reference.
//
// One pass turns each row's ops[begin_offset, end_offset) -- AIM's wire format, in the orientation of the text row -- into an aim_sam_t
// (forward-strand POS, reference span, NM) plus BAM CIGAR words and MD bytes; the conventions are stated at the flag in aim_hip.h.
// The text is the reference, so AIM 'I' (a text base) is SAM 'D' and AIM 'D' (a pattern base) is SAM 'I'. A strand-1 row is walked from
// the top: walk index k is row byte begin + k on strand 0 and end - 1 - k on strand 1, and along the walk the forward reference position
// only ever grows, so neither the read nor a complement is needed. Every byte other than 'M', 'X' and 'I' counts as 'D'.
//
// Structure (cigar_rle_wave, batch_io.hpp, is the model): count, reserve once per wavefront, write.
//   pass 1  finds the peeled range (terminal non-M/X ops) and counts CIGAR words and MD bytes, decimal digits included;
//   reserve one vector atomicAdd per buffer per wavefront on the two cursors {CIGAR words @0, MD bytes @1};
//   pass 2  writes. A row that does not fit either buffer writes nothing and reports AIM_SAM_OVERFLOW.
// Placement in the buffers depends on scheduling; content and every record field other than the two offsets do not.
//
// Two mappings:
//   sam_lane_kernel  one row per lane (short rows): a byte walk over word loads, whole words of 'M' taken four at a time;
//   sam_wave_kernel  one row per wavefront (long rows): each lane takes 4 consecutive walk positions of a 256-op tile; run boundaries,
//                    reference positions, MD match counts and output offsets come from wave scans with uniform carries between
//                    tiles, and every lane reads the reference bytes of its own mismatches / deleted bases.
// No LDS (the scans are cross-lane shuffles), plain vector stores only.
//
// aim_sam_device_split (AIM_FEATURE_SPLIT) is a second instantiation of both mappings, sam_lane_split_kernel and sam_wave_split_kernel:
// the bodies below take SPLIT as a compile-time constant, and with it a row also reads its aim_segment_t, adds the rest of the read to the two soft
// clips before anything is counted, and carries 0x800 into the record. SPLIT = false compiles to the kernels as they were.
#pragma once

#include "aim_device.hpp"

namespace aim {

// READ_SIZE from which one row gets a whole wavefront (AIM_SAM_WAVE_MIN overrides). Measured on 256 MB of ops rows at e = 1 %, the two
// mappings alternating over five rounds (profiles/sam/kernel_rounds.jsonl; spread below 1 %): one row per lane is 1.13x faster at
// READ_SIZE 2 536, one row per wavefront 1.11x faster at 3 040; the times cross near 2 800.
constexpr int kSamWaveMinReadSize = 2816;
constexpr uint64_t kSamPosMask = ~(1ull << 63);

struct SamArgs {
    int32_t algo, max_score, read_size;
    uint32_t n_rows;
    const uint64_t *text_pos;      // [candidates] window start | strand << 63
    const uint32_t *sel;           // [n_rows] candidate of row r, or nullptr (candidate r); UINT32_MAX: no candidate
    const aim_result_t *res;       // [n_rows]
    const char *ops;               // [n_rows][2 READ_SIZE]
    const char *ref;
    uint64_t ref_len;
    uint32_t options;              // AIM_SAM_EQX
    aim_sam_t *sam;                // out [n_rows]
    uint32_t *cigar;               // out, BAM words
    uint32_t cigar_cap;
    char *md;                      // out, no terminator
    uint32_t md_cap;
    uint32_t *cursors;             // {next free CIGAR word, next free MD byte}
};

#ifdef AIM_TU_SAM_FIELDS   // the kernels live in tu_sam_fields.hip alone; aim_capi.hip sees SamArgs and the launcher

// AIM op classes: 0 'M', 1 'X', 2 'I' (a reference base: SAM D), 3 everything else ('D', a read base: SAM I)
__device__ __forceinline__ uint32_t sam_class(uint32_t op) { return op == 'M' ? 0u : (op == 'X' ? 1u : (op == 'I' ? 2u : 3u)); }
// BAM op of a class: M 0, I 1, D 2, = 7, X 8
__device__ __forceinline__ uint32_t sam_bam_op(uint32_t cls, bool eqx) { return cls == 0 ? (eqx ? 7u : 0u) : (cls == 1 ? (eqx ? 8u : 0u) : (cls == 2 ? 2u : 1u)); }
__device__ __forceinline__ uint32_t sam_ndig(uint32_t x)
{
    return x < 10u ? 1u : x < 100u ? 2u : x < 1000u ? 3u : x < 10000u ? 4u : x < 100000u ? 5u : x < 1000000u ? 6u : x < 10000000u ? 7u : x < 100000000u ? 8u : x < 1000000000u ? 9u : 10u;
}
__device__ __forceinline__ void sam_put_dec(char *dst, uint32_t x, uint32_t nd)
{
    for (int i = (int)nd - 1; i >= 0; --i) { dst[i] = (char)('0' + x % 10u); x /= 10u; }
}
// the reference byte at forward position pos, the read clamped to [0, ref_len)
__device__ __forceinline__ char sam_ref_byte(const SamArgs &a, uint64_t pos)
{
    if (!a.ref_len) return 'N';
    return a.ref[pos < a.ref_len ? pos : a.ref_len - 1];
}

// What every mapping first learns about its row.
struct SamRow {
    aim_result_t r;
    uint64_t ws;        // window start
    int b, e;           // ops range, clamped to the row
    bool rev, walk;     // strand 1; the row has ops to walk (else: unmapped)
};
__device__ __forceinline__ SamRow sam_row(const SamArgs &a, uint32_t row, bool active)
{
    SamRow s;
    s.r.max_operations = 0; s.r.begin_offset = 0; s.r.end_offset = 0; s.r.score = 0; s.r.status = AIM_PAIR_OK; s.r.idx = 0;
    s.ws = 0; s.b = 0; s.e = 0; s.rev = false; s.walk = false;
    if (!active) return s;
    s.r = a.res[row];
    const uint32_t c = a.sel ? a.sel[row] : row;
    const bool has = c != 0xffffffffu;
    const uint64_t tp = has ? a.text_pos[c] : 0ull;
    s.ws = tp & kSamPosMask;
    s.rev = (tp >> 63) != 0;
    s.b = s.r.begin_offset < 0 ? 0 : s.r.begin_offset;
    s.e = s.r.end_offset > 2 * a.read_size ? 2 * a.read_size : s.r.end_offset;
    const bool over = a.algo == AIM_ALGO_WFA && (int64_t)s.r.score == (int64_t)a.max_score + 1;   // a WFA row over the cap
    s.walk = has && s.r.status == AIM_PAIR_OK && s.e > s.b && !over;
    return s;
}

// The record of a row: counts from pass 1, the offsets the wavefront reserved.
struct SamCount {
    uint32_t n_cigar, md_len, nm, ref_span, lead_ref;
    bool mapped;
};
__device__ __forceinline__ void sam_store_record(const SamArgs &a, uint32_t row, const SamRow &s, const SamCount &c, uint32_t coff, uint32_t moff, bool fits,
                                                 uint32_t more_flags = 0u)
{
    aim_sam_t o;
    o.idx = s.r.idx;
    o.score = s.r.score;
    o.pos = s.ws + (c.mapped ? c.lead_ref : 0u);
    o.ref_span = c.mapped ? c.ref_span : 0u;
    o.nm = c.mapped ? c.nm : 0u;
    o.cigar_offset = coff;
    o.n_cigar = (c.mapped && fits) ? c.n_cigar : 0u;
    o.md_offset = moff;
    o.md_len = (c.mapped && fits) ? c.md_len : 0u;
    o.flags = (uint16_t)(c.mapped ? ((s.rev ? 0x10u : 0u) | more_flags) : 0x4u);
    o.status = (uint16_t)(((uint32_t)s.r.status & 0xffu) | ((c.mapped && !fits) ? 0x100u : 0u));
    o.pad = 0;
    a.sam[row] = o;
}

// SPLIT: what the row's segment adds. A segment without flags turns the row into one without a candidate.
struct SamSplit {
    uint32_t lead, trail;   // read bases in front of / behind the segment, in the record's orientation
    uint32_t flags;         // AIM_SAM_SUPPLEMENTARY or 0
};
__device__ __forceinline__ SamSplit sam_split_row(const SamArgs &a, const aim_segment_t *seg, uint32_t row, bool active, SamRow *s)
{
    SamSplit x = {0u, 0u, 0u};
    if (!active) return x;
    const uint32_t c = a.sel ? a.sel[row] : row;
    if (c == 0xffffffffu) return x;
    const uint2 w = reinterpret_cast<const uint2 *>(seg)[c];      // {q_begin | q_end << 16, read_len | flags << 16 | cand << 24}
    const uint32_t flags = (w.y >> 16) & 0xffu;
    if (!flags) { s->ws = 0; s->rev = false; s->walk = false; return x; }
    const uint32_t before = w.x & 0xffffu, q_end = w.x >> 16, len = w.y & 0xffffu;
    const uint32_t behind = len > q_end ? len - q_end : 0u;
    x.lead = s->rev ? behind : before;
    x.trail = s->rev ? before : behind;
    x.flags = (flags & AIM_SEG_SUPPLEMENTARY) ? AIM_SAM_SUPPLEMENTARY : 0u;
    return x;
}

__device__ __forceinline__ uint32_t sam_wave_excl_sum(uint32_t v, int lane, uint32_t *total)
{
    uint32_t incl = v;
    for (int o = 1; o < kWave; o <<= 1) { const uint32_t t = __shfl_up(incl, o); if (lane >= o) incl += t; }
    *total = (uint32_t)__builtin_amdgcn_readlane((int)incl, kWave - 1);
    return incl - v;
}
// exclusive running maximum (-1 before lane 0); *top receives the maximum over the wavefront
__device__ __forceinline__ int sam_wave_excl_max(int v, int lane, int *top)
{
    int incl = v;
    for (int o = 1; o < kWave; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl = max(incl, t); }
    *top = __builtin_amdgcn_readlane(incl, kWave - 1);
    const int prev = __shfl_up(incl, 1);
    return lane ? prev : -1;
}

// ---- one row per lane ---------------------------------------------------------------------------------------------------------------
// The core [k0, k1) of the walk, counted (WRITE = false) or written. The same statement order in both, so the counts are the bytes.
template <bool WRITE>
__device__ __forceinline__ void sam_lane_core(const SamArgs &a, const SamRow &s, const uint32_t *rowp, int k0, int k1, uint32_t lead_clip, uint32_t trail_clip,
                                              uint32_t lead_ref, SamCount *c, uint32_t *cg, char *md)
{
    const bool eqx = (a.options & AIM_SAM_EQX) != 0;
    uint32_t nc = 0, nmd = 0, nm = 0, span = 0, cnt = 0;
    uint32_t run_op = 0xffu, run_len = 0, prev_cls = 0;
    int cw = -1;
    uint32_t word = 0;
    if (lead_clip) { if (WRITE) cg[nc] = (lead_clip << 4) | 4u; ++nc; }
    int k = k0;
    while (k < k1) {
        const int i = s.rev ? s.e - 1 - k : s.b + k;
        if ((i >> 2) != cw) { cw = i >> 2; word = rowp[cw]; }
        // four matches at once: the walk sits at the word's first byte in walk order and the whole word lies inside the core
        const bool whole = k + 4 <= k1 && (i & 3) == (s.rev ? 3 : 0) && word == 0x4D4D4D4Du;
        const uint32_t cls = whole ? 0u : sam_class((word >> (8 * (i & 3))) & 0xffu);
        const uint32_t step = whole ? 4u : 1u;
        const uint32_t bop = sam_bam_op(cls, eqx);
        if (bop != run_op) {
            if (run_len) { if (WRITE) cg[nc] = (run_len << 4) | run_op; ++nc; }
            run_op = bop;
            run_len = 0;
        }
        run_len += step;
        if (cls == 0) {
            cnt += step;
            span += step;
        } else if (cls == 1) {
            const uint32_t nd = sam_ndig(cnt);
            if (WRITE) { sam_put_dec(md + nmd, cnt, nd); md[nmd + nd] = sam_ref_byte(a, s.ws + lead_ref + span); }
            nmd += nd + 1;
            cnt = 0; ++span; ++nm;
        } else if (cls == 2) {
            if (prev_cls != 2) {
                const uint32_t nd = sam_ndig(cnt);
                if (WRITE) { sam_put_dec(md + nmd, cnt, nd); md[nmd + nd] = '^'; }
                nmd += nd + 1;
                cnt = 0;
            }
            if (WRITE) md[nmd] = sam_ref_byte(a, s.ws + lead_ref + span);
            ++nmd; ++span; ++nm;
        } else {
            ++nm;
        }
        prev_cls = cls;
        k += (int)step;
    }
    if (run_len) { if (WRITE) cg[nc] = (run_len << 4) | run_op; ++nc; }
    if (trail_clip) { if (WRITE) cg[nc] = (trail_clip << 4) | 4u; ++nc; }
    const uint32_t nd = sam_ndig(cnt);
    if (WRITE) sam_put_dec(md + nmd, cnt, nd);
    nmd += nd;
    if (!WRITE) { c->n_cigar = nc; c->md_len = nmd; c->nm = nm; c->ref_span = span; }
}

// one wavefront of 64 rows; all 64 lanes must call
template <bool SPLIT>
__device__ __forceinline__ void sam_lane_wave(const SamArgs &a, const aim_segment_t *seg, uint32_t row, bool active, int lane)
{
    SamRow s = sam_row(a, row, active);
    SamSplit x = {0u, 0u, 0u};
    if (SPLIT) x = sam_split_row(a, seg, row, active, &s);
    const uint32_t *rowp = reinterpret_cast<const uint32_t *>(a.ops + (uint64_t)row * 2u * (uint32_t)a.read_size);
    const int n = s.walk ? s.e - s.b : 0;
    auto op_at = [&](int k) -> uint32_t {
        const int i = s.rev ? s.e - 1 - k : s.b + k;
        return (rowp[i >> 2] >> (8 * (i & 3))) & 0xffu;
    };
    // peel both ends: every op that is not M or X; 'I' moves the position, the rest is the soft clip
    int k0 = 0, k1 = n;
    uint32_t lead_ref = 0, trail_ref = 0;
    while (k0 < n) {
        const uint32_t cls = sam_class(op_at(k0));
        if (cls < 2) break;
        lead_ref += cls == 2;
        ++k0;
    }
    while (k1 > k0) {
        const uint32_t cls = sam_class(op_at(k1 - 1));
        if (cls < 2) break;
        trail_ref += cls == 2;
        --k1;
    }
    const uint32_t lead_clip = (uint32_t)k0 - lead_ref + (SPLIT ? x.lead : 0u), trail_clip = (uint32_t)(n - k1) - trail_ref + (SPLIT ? x.trail : 0u);
    SamCount c;
    c.n_cigar = 0; c.md_len = 0; c.nm = 0; c.ref_span = 0; c.lead_ref = lead_ref;
    c.mapped = k1 > k0;
    if (c.mapped) sam_lane_core<false>(a, s, rowp, k0, k1, lead_clip, trail_clip, lead_ref, &c, nullptr, nullptr);
    // one reservation per buffer for the wavefront
    uint32_t tot_c = 0, tot_m = 0;
    const uint32_t ex_c = sam_wave_excl_sum(c.n_cigar, lane, &tot_c), ex_m = sam_wave_excl_sum(c.md_len, lane, &tot_m);
    uint32_t base_c = 0, base_m = 0;
    if (lane == 0 && tot_c) base_c = atomicAdd(&a.cursors[0], tot_c);
    if (lane == 0 && tot_m) base_m = atomicAdd(&a.cursors[1], tot_m);
    base_c = (uint32_t)__builtin_amdgcn_readfirstlane((int)base_c);
    base_m = (uint32_t)__builtin_amdgcn_readfirstlane((int)base_m);
    const uint64_t off_c = (uint64_t)base_c + ex_c, off_m = (uint64_t)base_m + ex_m;
    const bool fits = off_c + c.n_cigar <= a.cigar_cap && off_m + c.md_len <= a.md_cap;
    if (c.mapped && fits) sam_lane_core<true>(a, s, rowp, k0, k1, lead_clip, trail_clip, lead_ref, &c, a.cigar + off_c, a.md + off_m);
    if (active) sam_store_record(a, row, s, c, (uint32_t)off_c, (uint32_t)off_m, fits, SPLIT ? x.flags : 0u);
}

__global__ __launch_bounds__(64) void sam_lane_kernel(SamArgs a)
{
    const int lane = threadIdx.x;
    const uint32_t row = blockIdx.x * kWave + lane;
    sam_lane_wave<false>(a, nullptr, row, row < a.n_rows, lane);
}

__global__ __launch_bounds__(64) void sam_lane_split_kernel(SamArgs a, const aim_segment_t *seg)
{
    const int lane = threadIdx.x;
    const uint32_t row = blockIdx.x * kWave + lane;
    sam_lane_wave<true>(a, seg, row, row < a.n_rows, lane);
}

// ---- one row per wavefront ----------------------------------------------------------------------------------------------------------
// The 4 ops at walk positions k .. k + 3 of a row, byte j = position k + j; 0 at and past n. Only words that hold a byte of [b, e) are
// loaded, and those lie inside the row.
__device__ __forceinline__ uint32_t sam_walk4(const uint32_t *rowp, const SamRow &s, int n, int k)
{
    const int valid = n - k;
    if (valid <= 0) return 0u;
    const int o = s.rev ? s.e - k - 4 : s.b + k;           // first row byte of the four (strand 1: may lie below the range, even below 0)
    const int w0 = o >> 2;                                 // (arithmetic shift: floor)
    const uint32_t sh = (uint32_t)(o & 3);
    const uint32_t lo = (w0 >= 0 && 4 * w0 < s.e) ? rowp[w0] : 0u;
    const uint32_t hi = (sh && w0 + 1 >= 0 && 4 * (w0 + 1) < s.e) ? rowp[w0 + 1] : 0u;
    uint32_t q = __builtin_amdgcn_alignbyte(hi, lo, sh);
    if (s.rev) q = __builtin_amdgcn_perm(0u, q, 0x00010203u);   // the walk runs down the row
    return valid >= 4 ? q : (q & ((1u << (8 * valid)) - 1u));
}

struct SamWaveState {          // uniform over the wavefront
    int first, last;           // walk positions of the first and the last M / X
    uint32_t lead_clip, trail_clip;
};

// One sweep over the tiles of a row. WRITE = false counts (c), WRITE = true stores at cg / md (the bases the wavefront reserved).
template <bool WRITE>
__device__ __forceinline__ void sam_wave_sweep(const SamArgs &a, const SamRow &s, const uint32_t *rowp, int n, int lane, SamWaveState &st, SamCount *c,
                                               uint32_t *cg, char *md)
{
    const bool eqx = (a.options & AIM_SAM_EQX) != 0;
    const int first = st.first, last = st.last;
    // carries between tiles
    uint32_t prev_q = 0;                 // the previous tile's lane 63
    uint32_t mp_c = 0, rp_c = 0, nb_c = 0, md_c = 0;   // core M's, reference-consuming ops, run boundaries, MD bytes so far
    int start_c = first, base_c = 0;     // where the open run started; the M count at the last mismatch / deleted base
    uint32_t my_nm = 0, my_lead = 0, my_trail = 0, my_md = 0, my_span = 0;   // per-lane sums, reduced after the sweep
    const uint32_t lead_s = st.lead_clip ? 1u : 0u;
    for (int t0 = 0; t0 <= last; t0 += 4 * kWave) {
        const int k = t0 + 4 * lane;
        const uint32_t q = sam_walk4(rowp, s, n, k);
        const uint32_t up = __shfl_up(q, 1);
        uint32_t pcls = sam_class((lane ? up : prev_q) >> 24);   // class of position k - 1
        uint32_t cls[4];
        uint32_t nM = 0, nR = 0, nB = 0;
        int my_start = -1;
        bool bnd[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int kk = k + j;
            cls[j] = kk < n ? sam_class((q >> (8 * j)) & 0xffu) : 3u;
            const bool core = kk >= first && kk <= last;
            nM += core && cls[j] == 0;
            nR += kk < n && cls[j] < 3;
            const uint32_t before = j ? cls[j - 1] : pcls;
            bnd[j] = kk > first && kk <= last && sam_bam_op(cls[j], eqx) != sam_bam_op(before, eqx);
            if (bnd[j]) { ++nB; my_start = kk; }
            if (!WRITE) {
                my_nm += core && cls[j] != 0;
                my_span += core && cls[j] != 3;
                my_lead += kk < first && cls[j] == 3;
                my_trail += kk > last && kk < n && cls[j] == 3;
            }
        }
        uint32_t tot = 0;
        const uint32_t ex = sam_wave_excl_sum(nM | (nR << 10) | (nB << 20), lane, &tot);
        uint32_t mp = mp_c + (ex & 0x3ffu);
        const uint32_t rp0 = rp_c + ((ex >> 10) & 0x3ffu);
        // the M count at this lane's last mismatch / deleted base
        int my_base = -1;
        {
            uint32_t m = mp;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kk = k + j;
                const bool core = kk >= first && kk <= last;
                if (core && cls[j] == 0) ++m;
                if (core && (cls[j] == 1 || cls[j] == 2)) my_base = (int)m;
            }
        }
        int top_base = -1;
        const int ex_base = sam_wave_excl_max(my_base, lane, &top_base);
        int base = max(base_c, ex_base);
        // MD bytes of this lane's ops
        uint32_t bytes = 0, nd[4];
        uint32_t cnt[4];
        {
            uint32_t m = mp;
            int bs = base;
            uint32_t before = pcls;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kk = k + j;
                const bool core = kk >= first && kk <= last;
                nd[j] = 0; cnt[j] = 0;
                if (core && cls[j] == 0) ++m;
                if (core && (cls[j] == 1 || (cls[j] == 2 && before != 2))) { cnt[j] = m - (uint32_t)bs; nd[j] = sam_ndig(cnt[j]); bytes += nd[j] + 1; }
                if (core && cls[j] == 2) ++bytes;
                if (core && (cls[j] == 1 || cls[j] == 2)) bs = (int)m;
                before = cls[j];
            }
        }
        if (!WRITE) {
            my_md += bytes;
        } else {
            uint32_t tot_md = 0;
            const uint32_t ex_md = sam_wave_excl_sum(bytes, lane, &tot_md);
            int top_start = -1;
            const int ex_start = sam_wave_excl_max(my_start, lane, &top_start);
            // CIGAR: a boundary at kk closes the run that started at the latest boundary (or `first`) before it
            int cur = max(start_c, ex_start);
            uint32_t at = lead_s + nb_c + ((ex >> 20) & 0x3ffu);
            char *m = md + md_c + ex_md;
            uint32_t rp = rp0, before = pcls;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int kk = k + j;
                const bool core = kk >= first && kk <= last;
                if (bnd[j]) { cg[at++] = ((uint32_t)(kk - cur) << 4) | sam_bam_op(before, eqx); cur = kk; }
                if (core && cls[j] == 1) {
                    sam_put_dec(m, cnt[j], nd[j]);
                    m[nd[j]] = sam_ref_byte(a, s.ws + rp);
                    m += nd[j] + 1;
                } else if (core && cls[j] == 2) {
                    if (before != 2) { sam_put_dec(m, cnt[j], nd[j]); m[nd[j]] = '^'; m += nd[j] + 1; }
                    *m++ = sam_ref_byte(a, s.ws + rp);
                }
                rp += kk < n && cls[j] < 3;
                before = cls[j];
            }
            md_c += tot_md;
            start_c = max(start_c, top_start);
        }
        mp_c += tot & 0x3ffu;
        rp_c += (tot >> 10) & 0x3ffu;
        nb_c += (tot >> 20) & 0x3ffu;
        base_c = max(base_c, top_base);
        prev_q = (uint32_t)__builtin_amdgcn_readlane((int)q, kWave - 1);
    }
    const uint32_t tail = mp_c - (uint32_t)base_c;       // the final match count
    if (!WRITE) {
        uint32_t t_nm = 0, t_md = 0, t_lead = 0, t_span = 0;
        (void)sam_wave_excl_sum(my_span, lane, &t_span);
        (void)sam_wave_excl_sum(my_nm, lane, &t_nm);
        (void)sam_wave_excl_sum(my_md, lane, &t_md);
        (void)sam_wave_excl_sum(my_lead, lane, &t_lead);
        // the ops behind the last tile of the core (a long trailing peel) are counted here
        for (int t0 = ((last >> 8) + 1) << 8; t0 < n; t0 += 4 * kWave) {
            const int k = t0 + 4 * lane;
            const uint32_t q = sam_walk4(rowp, s, n, k);
#pragma unroll
            for (int j = 0; j < 4; ++j) my_trail += k + j < n && sam_class((q >> (8 * j)) & 0xffu) == 3;
        }
        uint32_t t_trail = 0;
        (void)sam_wave_excl_sum(my_trail, lane, &t_trail);
        st.lead_clip = t_lead;
        st.trail_clip = t_trail;
        c->n_cigar = nb_c + 1u + (t_lead ? 1u : 0u) + (t_trail ? 1u : 0u);
        c->md_len = t_md + sam_ndig(tail);
        c->nm = t_nm;
        c->ref_span = t_span;                       // the core's M, X and I ops
        c->lead_ref = (uint32_t)first - t_lead;     // what precedes `first` is dropped reference bases and the clip
    } else if (lane == 0) {
        if (st.lead_clip) cg[0] = (st.lead_clip << 4) | 4u;
        const int il = s.rev ? s.e - 1 - last : s.b + last;
        const uint32_t last_cls = sam_class((rowp[il >> 2] >> (8 * (il & 3))) & 0xffu);
        uint32_t at = lead_s + nb_c;
        cg[at++] = ((uint32_t)(last + 1 - start_c) << 4) | sam_bam_op(last_cls, eqx);
        if (st.trail_clip) cg[at] = (st.trail_clip << 4) | 4u;
        sam_put_dec(md + md_c, tail, sam_ndig(tail));
    }
}

// blockDim.x = 256: four rows per workgroup, one per wavefront (no LDS, no barrier). The body is a macro, not a function template like
// sam_lane_wave: expanded inside the kernel, SPLIT = false gives sam_wave_kernel instruction for instruction as it was before there was a
// second instantiation; inlined from a function it came out with two scalar instructions in another place.
// Should a later compiler give the same instructions for a function template (compare the disassembly of sam_wave_kernel before and
// after), make this a template like sam_lane_wave again.
#define AIM_SAM_WAVE_ROWS(SPLIT, seg)                                                                                              \
    const int lane = threadIdx.x & (kWave - 1);                                                                                    \
    const uint32_t row = blockIdx.x * 4u + (threadIdx.x >> 6);                                                                     \
    if (row >= a.n_rows) return; /* (wave-uniform) */                                                                              \
    SamRow s = sam_row(a, row, true);                                                                                              \
    SamSplit x = {0u, 0u, 0u};                                                                                                     \
    if (SPLIT) x = sam_split_row(a, seg, row, true, &s);                                                                           \
    const uint32_t *rowp = reinterpret_cast<const uint32_t *>(a.ops + (uint64_t)row * 2u * (uint32_t)a.read_size);                 \
    const int n = s.walk ? s.e - s.b : 0;                                                                                          \
    /* the first and the last M / X of the walk */                                                                                 \
    int fmin = 0x7fffffff, lneg = 0x7fffffff; /* lneg = -(last position) */                                                        \
    for (int t0 = 0; t0 < n; t0 += 4 * kWave) {                                                                                    \
        const int k = t0 + 4 * lane;                                                                                               \
        const uint32_t q = sam_walk4(rowp, s, n, k);                                                                               \
        _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                                              \
            if (k + j < n && sam_class((q >> (8 * j)) & 0xffu) < 2) { fmin = min(fmin, k + j); lneg = min(lneg, -(k + j)); }       \
    }                                                                                                                              \
    SamWaveState st;                                                                                                               \
    st.first = wave_min_i32(fmin);                                                                                                 \
    const int ln = wave_min_i32(lneg);                                                                                             \
    st.last = -ln;                                                                                                                 \
    st.lead_clip = st.trail_clip = 0;                                                                                              \
    SamCount c;                                                                                                                    \
    c.n_cigar = 0; c.md_len = 0; c.nm = 0; c.ref_span = 0; c.lead_ref = 0;                                                         \
    c.mapped = st.first != 0x7fffffff;                                                                                             \
    if (c.mapped) sam_wave_sweep<false>(a, s, rowp, n, lane, st, &c, nullptr, nullptr);                                            \
    if (SPLIT && c.mapped) { /* the rest of the read joins the clips the sweep counted */                                          \
        c.n_cigar += (uint32_t)(!st.lead_clip && x.lead) + (uint32_t)(!st.trail_clip && x.trail);                                  \
        st.lead_clip += x.lead;                                                                                                    \
        st.trail_clip += x.trail;                                                                                                  \
    }                                                                                                                              \
    uint32_t base_c = 0, base_m = 0;                                                                                               \
    if (lane == 0 && c.n_cigar) base_c = atomicAdd(&a.cursors[0], c.n_cigar);                                                      \
    if (lane == 0 && c.md_len) base_m = atomicAdd(&a.cursors[1], c.md_len);                                                        \
    base_c = (uint32_t)__builtin_amdgcn_readfirstlane((int)base_c);                                                                \
    base_m = (uint32_t)__builtin_amdgcn_readfirstlane((int)base_m);                                                                \
    const bool fits = (uint64_t)base_c + c.n_cigar <= a.cigar_cap && (uint64_t)base_m + c.md_len <= a.md_cap;                      \
    if (c.mapped && fits) sam_wave_sweep<true>(a, s, rowp, n, lane, st, &c, a.cigar + base_c, a.md + base_m);                      \
    if (lane == 0) sam_store_record(a, row, s, c, base_c, base_m, fits, SPLIT ? x.flags : 0u);

__global__ __launch_bounds__(256) void sam_wave_kernel(SamArgs a) { AIM_SAM_WAVE_ROWS(false, nullptr) }
__global__ __launch_bounds__(256) void sam_wave_split_kernel(SamArgs a, const aim_segment_t *seg) { AIM_SAM_WAVE_ROWS(true, seg) }
#undef AIM_SAM_WAVE_ROWS

void sam_fields_launch(bool wave, const SamArgs &a, hipStream_t s)
{
    if (!a.n_rows) return;
    if (wave) hipLaunchKernelGGL(sam_wave_kernel, dim3((a.n_rows + 3u) / 4u), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(sam_lane_kernel, dim3((a.n_rows + 63u) / 64u), dim3(64), 0, s, a);
}

void sam_fields_split_launch(bool wave, const SamArgs &a, const aim_segment_t *seg, hipStream_t s)
{
    if (!a.n_rows) return;
    if (wave) hipLaunchKernelGGL(sam_wave_split_kernel, dim3((a.n_rows + 3u) / 4u), dim3(256), 0, s, a, seg);
    else hipLaunchKernelGGL(sam_lane_split_kernel, dim3((a.n_rows + 63u) / 64u), dim3(64), 0, s, a, seg);
}
#else
void sam_fields_launch(bool wave, const SamArgs &a, hipStream_t s);
void sam_fields_split_launch(bool wave, const SamArgs &a, const aim_segment_t *seg, hipStream_t s);
#endif

}  // namespace aim
