// wfa_wave.hpp -- general WFA / WFA-adaptive kernel: ONE PAIR PER 64-LANE WAVEFRONT.
//
// Replaces the tasklet loop + affine_wfa_compute of the reference
// (WFA/DPU-WRAM/dpu/wfa.c:342-503) and affine_wavefronts_backtrace
// (WFA/DPU-WRAM/dpu/wfa_backtracing.c:210-351).
//
// Mapping: lanes run along the diagonals k of the current wavefront (64 per
// step, looping for wider wavefronts).  Sequences are staged once per pair in
// LDS (the DPU's WRAM copy, wfa.c:417-459); the descriptors of the last 64
// scores live in an LDS ring; the offset vectors (M/I/D) of the live window --
// the max(x, o+e)+1 most recent scores, all that affine_wfa_compute_next ever
// reads -- live in a second LDS ring (one slot per score, slot_w diagonals), so a
// score step costs LDS round trips, not L2 ones.  With BACKTRACE every
// wavefront is also streamed to a per-wave HBM pool (the DPU's WRAM arena /
// MRAM spill, allocate_new_score wfa.c:143-183) that the traceback walks; a
// wavefront wider than a slot lives in that pool only (slower, same results).
// Handles any MAX_SCORE / READ_SIZE / penalties; the short-read fast path is
// wfa_lane.hpp.
//
// EF (AIM_FLAG_ENDSFREE, aim_hip.h): ends-free alignment.  Three changes, all
// compiled out of the global instantiations: the score-0 wavefront spans
// diagonals [-PB, TB] with offsets max(k, 0); after each extend the run ends as
// soon as any diagonal's M offset sits on an end border (one wave reduction);
// the traceback writes the trailing free run, walks, writes the score-0 match
// stroke and then the leading free run.
//
// A2P (AIM_FLAG_AFFINE2P, never with REDUCE or EF): dual-cost gap-affine.  Two
// more components, I2 and D2 (M at s - (o2+e2), themselves at s - e2); M takes
// the best of X, I1, D1, I2 and D2.  An LDS slot holds five rows, and a score's
// pool region always holds all five (M, I1, D1, I2, D2 at off_m + comp * len),
// so WfMeta keeps its 32 bytes and the I2 / D2 offsets are derived.  An absent
// piece-2 component reads as NULL.  The walk tests piece 1 before piece 2.
//
// LIN (AIM_FLAG_LINEAR, never with REDUCE, EF or A2P): gap-linear.  M only:
// M[s][k] = max(M[s-x][k] + 1, M[s-g][k-1] + 1, M[s-g][k+1]), then extend; an
// LDS slot and a score's pool region hold the M row alone, and every NULL
// reads as NULL.  The walk tests D, then I, then X (wfa_group.hpp's
// group_tb_walk_lin, same CIGAR bytes).
//
// OFF (AIM_FLAG_WFA_W32): the offset type.  int16_t is the reference as built
// (AFFINE_WAVEFRONT_W16, common.h:92-100: NULL = INT16_MIN/2, every (awf_t)
// cast a deliberate int16 wrap); int32_t is its AFFINE_WAVEFRONT_W32 branch
// (common.h:101-104: NULL = INT32_MIN/2), which lifts the READ_SIZE < 32760 cap.
// The LDS ring, the HBM pool, the wrap casts, the NULL tests and the traceback
// all take OFF; nothing else changes.
#pragma once

#include "aim_device.hpp"

namespace aim {

// AFFINE_WAVEFRONT_OFFSET_NULL of each offset type: INT16_MIN/2 (W16, common.h:98) / INT32_MIN/2 (W32, common.h:102)
template <typename OFF>
constexpr int awf_null() { return sizeof(OFF) == 2 ? -16384 : INT32_MIN / 2; }

// wfa_component (common.h:126-138) with pool offsets instead of pointers.
struct __attribute__((aligned(16))) WfMeta {
    int klo, khi;   // current (possibly reduced) bounds
    int lo, hi;     // allocation bounds (lo_base / hi_base)
    int off_m;      // pool index of M[lo]
    int off_i;      // pool index of I[lo] (iwavefront != NULL <=> WF_HASI)
    int off_d;      // pool index of D[lo] (dwavefront != NULL <=> WF_HASD)
    int flags;
};
enum { WF_PRESENT = 1, WF_MNULL = 2, WF_INULL = 4, WF_DNULL = 8, WF_INLDS = 16, WF_HASI = 32, WF_HASD = 64, WF_HASI2 = 128, WF_HASD2 = 256 };

constexpr int kMetaRing = 64;        // scores kept in the LDS descriptor ring

struct WfaWaveCtx {
    WfMeta *ring;        // LDS, kMetaRing entries
    WfMeta *gmeta;       // HBM, meta_cap entries
    int cur_score;
};

__device__ __forceinline__ WfMeta wf_get_meta(const WfaWaveCtx &c, int s)
{
    if (c.cur_score - s < kMetaRing) return c.ring[s & (kMetaRing - 1)];
    return c.gmeta[s];
}

__device__ __forceinline__ void wf_put_meta(const WfaWaveCtx &c, int s, const WfMeta &m, int lane)
{
    if (lane == 0) {
        c.ring[s & (kMetaRing - 1)] = m;
        c.gmeta[s] = m;
    }
}

// affine_wfa_extend inner loop (wfa.c:198-206) on 4-byte words.
template <typename PtrT>
__device__ __forceinline__ int wf_extend_count(PtrT P, PtrT T, int v, int h, int plen, int tlen, int last_word)
{
    if (v < 0 || h < 0) return 0;
    int rem = min(plen - v, tlen - h);
    if (rem <= 0) return 0;
    int count = 0;
    for (;;) {
        const uint32_t x = load4_unaligned(P, v + count, last_word) ^ load4_unaligned(T, h + count, last_word);
        const int m = x ? (__builtin_ctz(x) >> 3) : 4;
        const int r = rem - count;
        if (m < 4) { count += min(m, r); break; }
        if (r <= 4) { count += r; break; }
        count += 4;
    }
    return count;
}

template <bool BT, bool REDUCE, bool SEQ_LDS, bool EF = false, bool A2P = false, bool LIN = false, typename OFF = int16_t>
__global__ __launch_bounds__(64) void wfa_wave_kernel(KArgs a)
{
    static_assert(sizeof(OFF) == 2 || sizeof(OFF) == 4, "offsets are int16_t or int32_t");
    typedef OFF awf_t;
    constexpr int kAwfNull = awf_null<OFF>();
    // pool index sums that may pass 2^31 before they are compared with pool_cap (W32 pools can hold up to 2^31 - 1 entries)
    typedef typename std::conditional<sizeof(OFF) == 4, int64_t, int>::type pidx_t;
    constexpr int NC = A2P ? 5 : LIN ? 1 : 3;   // components per wavefront: M, I, D (A2P: + I2, D2; LIN: M alone)
    extern __shared__ __attribute__((aligned(16))) char smem[];
    debug_poison_lds(a, smem);
    const int lane = threadIdx.x;
    const int rs = a.p.read_size;
    const int rsw = rs >> 2;                 // dwords per sequence row (read_size % 8 == 0)
    WfMeta *ring = reinterpret_cast<WfMeta *>(smem);
    awf_t *oring = reinterpret_cast<awf_t *>(smem + kMetaRing * sizeof(WfMeta));
    const int ring_slots = (int)a.ring_slots, slot_w = (int)a.slot_w;
    uint32_t *ldsP = reinterpret_cast<uint32_t *>(smem + kMetaRing * sizeof(WfMeta) + (((size_t)ring_slots * NC * slot_w * sizeof(awf_t) + 15) & ~(size_t)15));
    uint32_t *ldsT = ldsP + rsw + 2;

    char *wscr = a.scratch + (uint64_t)blockIdx.x * a.scratch_per_wave;
    WfaWaveCtx ctx;
    ctx.ring = ring;
    ctx.gmeta = reinterpret_cast<WfMeta *>(wscr);
    awf_t *pool = reinterpret_cast<awf_t *>(wscr + (uint64_t)a.meta_cap * sizeof(WfMeta));
    const int pool_cap = (int)a.pool_cap;

    const int X = a.p.mismatch, OE = a.p.gap_o + a.p.gap_e, E = a.p.gap_e;
    const int MS = a.p.max_score;
    const int OE2 = A2P ? a.a2p_o2 + a.a2p_e2 : 0, E2 = A2P ? a.a2p_e2 : 0;
    // component comp (0 M, 1 I, 2 D; A2P: 3 I2, 4 D2) of the wavefront of score sc: LDS slot or HBM pool
    auto slot = [&](int sc, int comp) -> awf_t * { return oring + ((sc % ring_slots) * NC + comp) * slot_w; };
    // row pointer (biased so that row[k] is diagonal k) -- computed once per score step, never per element
    auto rowp = [&](const WfMeta &m, int sc, int comp) -> const awf_t * {
        const awf_t *b = (m.flags & WF_INLDS) ? slot(sc, comp)
                         : A2P ? pool + m.off_m + comp * (m.hi - m.lo + 1)
                               : pool + (comp == 0 ? m.off_m : (comp == 1 ? m.off_i : m.off_d));
        return b - m.lo;
    };

    // Single-wave workgroup: LDS operations of one wave execute in issue order, so data exchanged through LDS
    // needs no hardware wait, only a compiler fence.  __syncthreads() would add s_waitcnt vmcnt(0), i.e. a full
    // round trip for the history / descriptor stores still in flight -- only paid when a row lives in the HBM pool.
    const bool meta_in_lds = max(max(X, OE), OE2) < kMetaRing;
    auto sync = [&](bool rows_in_lds) {
        if (rows_in_lds && meta_in_lds) asm volatile("" ::: "memory");
        else __syncthreads();
    };
    // direct mode: every pair of the batch; indirect mode: the pairs the lane kernel could not pack
    const uint32_t n_units = a.todo ? min(a.todo[0], a.n_pairs) : a.n_pairs;

    for (uint32_t it = 0;; ++it) {
        uint32_t pair;
        if (!xcd_unit(n_units, it, &pair)) break;   // past this block's slice: done
        if (a.todo) pair = a.todo[16 + pair];
        const aim_request_t rq = load_request(a, pair);
        const int plen = rq.pattern_len, tlen = rq.text_len;
        const uint32_t *gP = reinterpret_cast<const uint32_t *>(a.patterns + (uint64_t)pair * rs);
        const uint32_t *gT = reinterpret_cast<const uint32_t *>(a.texts + (uint64_t)pair * rs);
        char *ops = BT ? a.ops + (uint64_t)pair * 2 * rs : nullptr;

        __syncthreads();  // previous pair's LDS reads are done
        if (SEQ_LDS) {
            const int pw = (plen + 3) >> 2, tw = (tlen + 3) >> 2;
            for (int w = lane; w < pw; w += kWave) ldsP[w] = gP[w];
            for (int w = lane; w < tw; w += kWave) ldsT[w] = gT[w];
        }
        if (BT) {  // memset(cigar->operations, 'M', 2*READ_SIZE), wfa.c:465
            uint32_t *o4 = reinterpret_cast<uint32_t *>(ops);
            for (int w = lane; w < (rs >> 1); w += kWave) o4[w] = 0x4D4D4D4Du;
        }
        const int last_word = SEQ_LDS ? rsw + 1 : rsw - 1;

        // edit_cigar_allocate, wfa.c:57-67
        const int max_ops = plen + tlen;
        int begin_offset = max_ops - 1;
        const int end_offset = max_ops;
        int status = AIM_PAIR_OK;
        int final_score;
        const int ak = tlen - plen;   // alignment_k
        // EF: the pair's free lengths, clamped to its lengths
        const int pb = EF ? min(a.ef_pb, plen) : 0, pe = EF ? min(a.ef_pe, plen) : 0;
        const int tb = EF ? min(a.ef_tb, tlen) : 0, te = EF ? min(a.ef_te, tlen) : 0;
        const int w0 = pb + tb + 1;                       // diagonals of the score-0 wavefront
        const bool w0_lds = ring_slots > 0 && (!EF || w0 <= slot_w);
        const bool w0_fits = !EF || w0 <= pool_cap;       // (a BACKTRACE pool shrunk by the scratch bound may not hold it)
        int end_k = ak;                                   // EF: the end cell's diagonal

        // wavefronts[0] = allocate_new_score(0,0,0,0); M[0] = 0   (wfa.c:347-348)
        int pool_used = EF ? w0 : 1;
        WfMeta cur;
        cur.klo = cur.lo = -pb;
        cur.khi = cur.hi = tb;
        cur.off_m = 0; cur.off_i = -1; cur.off_d = -1;
        cur.flags = WF_PRESENT | WF_INULL | WF_DNULL | (w0_lds ? WF_INLDS : 0);
        ctx.cur_score = 0;
        if (EF) {   // M[k] = max(k, 0): (v = -k, h = 0) below the main diagonal, (v = 0, h = k) above it
            if (w0_fits)
                for (int i = lane; i < w0; i += kWave) {
                    const awf_t o = (awf_t)max(i - pb, 0);
                    pool[i] = o;
                    if (w0_lds) slot(0, 0)[i] = o;
                }
        } else if (lane == 0) {
            pool[0] = 0;
            if (ring_slots > 0) slot(0, 0)[0] = 0;
        }
        wf_put_meta(ctx, 0, cur, lane);
        __syncthreads();

        int score = 0;
        for (;;) {
            if (EF && !w0_fits) {   // allocate_new(): "out of memory", dpu_allocator_wram.c:19-23 (the plan never admits it: a guard)
                status = AIM_PAIR_NOMEM;
                final_score = MS + 1;   // no score was reached: not a 0 that would read like a perfect alignment
                break;
            }
            const bool live = (cur.flags & WF_PRESENT) && !(cur.flags & WF_MNULL);
            int hit_k = 0x7fffffff;   // EF: smallest diagonal whose extended M offset sits on an end border
            // ---- affine_wfa_extend, wfa.c:186-208 -------------------------------
            if (live) {
                const bool inlds = cur.flags & WF_INLDS;
                // one body, two call sites: after inlining the LDS call site compiles to ds_read/ds_write and the
                // pool call site to global loads/stores (a merged pointer would force flat accesses)
                auto extend_row = [&](awf_t *mrow) {
                    for (int k = cur.klo + lane; k <= cur.khi; k += kWave) {
                        const int moff = mrow[k - cur.lo];
                        if (moff >= 0) {
                            const int cnt = SEQ_LDS
                                ? wf_extend_count((const uint32_t *)ldsP, (const uint32_t *)ldsT, moff - k, moff, plen, tlen, last_word)
                                : wf_extend_count(gP, gT, moff - k, moff, plen, tlen, last_word);
                            if (cnt) mrow[k - cur.lo] = (awf_t)(moff + cnt);
                            if (BT && inlds) pool[cur.off_m + (k - cur.lo)] = (awf_t)(moff + cnt);   // HBM history for the traceback
                            if (EF) {
                                // end borders: (plen, h >= tlen - TE) and (v >= plen - PE, tlen); with PE = TE = 0 also
                                // global WFA's own test (alignment_k, offset >= tlen), so that zero free lengths end alike
                                const int h = moff + cnt, v = h - k;
                                const bool end = (v == plen && h >= tlen - te && h <= tlen) || (h == tlen && v >= plen - pe && v <= plen) ||
                                                 (pe == 0 && te == 0 && k == ak && h >= tlen);
                                if (end) hit_k = min(hit_k, k);
                            }
                        } else if (BT && inlds) {
                            pool[cur.off_m + (k - cur.lo)] = (awf_t)moff;
                        }
                    }
                };
                if (inlds) extend_row(slot(score, 0));
                else extend_row(pool + cur.off_m);
                sync(inlds);
            }
            // ---- affine_wfa_reduce_wvs (WFA-adaptive), wfa.c:69-140 --------------
            if (REDUCE && live && (cur.khi - cur.klo + 1) >= 10) {
                auto reduce_row = [&](const awf_t *mk) {
                int mind = max(plen, tlen);
                {
                    int d = 0x7fffffff;   // per-lane minimum over its diagonals, then ONE wave reduction
                    for (int k = cur.klo + lane; k <= cur.khi; k += kWave) {
                        const int off = mk[k];
                        d = min(d, max(plen - (off - k), tlen - off));
                    }
                    mind = min(mind, wave_min_i32(d));
                }
                int nklo = cur.klo, nkhi = cur.khi;
                const int top_limit = min(ak - 1, cur.khi);
                if (cur.klo < top_limit) {
                    bool found = false;
                    for (int base = cur.klo; base < top_limit && !found; base += kWave) {
                        const int k = base + lane;
                        bool ok = false;
                        if (k < top_limit) {
                            const int off = mk[k];
                            ok = (max(plen - (off - k), tlen - off) - mind) <= 50;
                        }
                        const unsigned long long mask = __ballot(ok);
                        if (mask) { nklo = base + __builtin_ctzll(mask); found = true; }
                    }
                    if (!found) nklo = top_limit;
                }
                const int bottom_limit = max(ak + 1, nklo);
                if (cur.khi > bottom_limit) {
                    bool found = false;
                    for (int top = cur.khi; top > bottom_limit && !found; top -= kWave) {
                        const int k = top - lane;
                        bool ok = false;
                        if (k > bottom_limit) {
                            const int off = mk[k];
                            ok = (max(plen - (off - k), tlen - off) - mind) <= 50;
                        }
                        const unsigned long long mask = __ballot(ok);
                        if (mask) { nkhi = top - __builtin_ctzll(mask); found = true; }
                    }
                    if (!found) nkhi = bottom_limit;
                }
                if (nklo > nkhi) {
                    cur.flags |= WF_MNULL | WF_INULL | WF_DNULL;   // wfa.c:131-139
                } else {
                    cur.klo = nklo;
                    cur.khi = nkhi;
                }
                wf_put_meta(ctx, score, cur, lane);
                sync(true);
                };
                if (cur.flags & WF_INLDS) reduce_row(slot(score, 0) - cur.lo);
                else reduce_row(pool + cur.off_m - cur.lo);
            }
            // ---- affine_wfa_end_reached, wfa.c:210-230 ---------------------------
            bool done = false;
            if (EF) {
                if (live) {
                    end_k = wave_min_i32(hit_k);
                    done = end_k != 0x7fffffff;
                }
            } else if ((cur.flags & WF_PRESENT) && !(cur.flags & WF_MNULL) && cur.klo <= ak && cur.khi >= ak) {
                const int off = (cur.flags & WF_INLDS) ? (int)slot(score, 0)[ak - cur.lo] : (int)pool[cur.off_m + (ak - cur.lo)];
                done = off >= tlen;
            }
            if (done) { final_score = score; break; }
            ++score;
            if (score > MS) { final_score = score; break; }   // wfa.c:368-376
            ctx.cur_score = score;

            // ---- affine_wfa_compute_next, wfa.c:268-340 --------------------------
            const int s_sub = score - X, s_o = score - OE, s_e = score - E;
            WfMeta ms, mo, me;
            ms.flags = mo.flags = me.flags = 0;
            if (s_sub >= 0) ms = wf_get_meta(ctx, s_sub);
            if (s_o >= 0) mo = wf_get_meta(ctx, s_o);
            if (!LIN && s_e >= 0) me = wf_get_meta(ctx, s_e);
            const bool m_sub_null = (s_sub < 0) || !(ms.flags & WF_PRESENT) || (ms.flags & WF_MNULL);
            const bool m_o_null = (s_o < 0) || !(mo.flags & WF_PRESENT) || (mo.flags & WF_MNULL);
            // (LIN: no I / D components; I and D of a cell come from M at s - g, the "open" source, with o = 0)
            const bool i_e_null = LIN || (s_e < 0) || !(me.flags & WF_PRESENT) || !(me.flags & WF_HASI) || (me.flags & WF_INULL);
            const bool d_e_null = LIN || (s_e < 0) || !(me.flags & WF_PRESENT) || !(me.flags & WF_HASD) || (me.flags & WF_DNULL);
            const bool i_out_null = m_o_null && i_e_null;
            const bool d_out_null = m_o_null && d_e_null;
            // A2P: piece 2's sources
            const int s_o2 = score - OE2, s_e2 = score - E2;
            WfMeta mo2, me2;
            mo2.flags = me2.flags = 0;
            bool m_o2_null = true, i2_e_null = true, d2_e_null = true;
            if constexpr (A2P) {
                if (s_o2 >= 0) mo2 = wf_get_meta(ctx, s_o2);
                if (s_e2 >= 0) me2 = wf_get_meta(ctx, s_e2);
                m_o2_null = (s_o2 < 0) || !(mo2.flags & WF_PRESENT) || (mo2.flags & WF_MNULL);
                i2_e_null = (s_e2 < 0) || !(me2.flags & WF_PRESENT) || !(me2.flags & WF_HASI2);
                d2_e_null = (s_e2 < 0) || !(me2.flags & WF_PRESENT) || !(me2.flags & WF_HASD2);
            }
            const bool i2_out_null = m_o2_null && i2_e_null, d2_out_null = m_o2_null && d2_e_null;
            if (m_sub_null && i_out_null && d_out_null && i2_out_null && d2_out_null) {
                cur.flags = 0;   // wavefronts[score] = NULL
                cur.klo = cur.lo = 0; cur.khi = cur.hi = -1;
                cur.off_m = cur.off_i = cur.off_d = -1;
                wf_put_meta(ctx, score, cur, lane);
                sync(true);
                continue;
            }
            const int sub_lo = m_sub_null ? 1 : ms.klo, sub_hi = m_sub_null ? -1 : ms.khi;
            const int o_lo = m_o_null ? 1 : mo.klo, o_hi = m_o_null ? -1 : mo.khi;
            const bool e_none = i_e_null && d_e_null;
            const int e_lo = e_none ? 1 : me.klo, e_hi = e_none ? -1 : me.khi;
            const int o2_lo = m_o2_null ? 1 : mo2.klo, o2_hi = m_o2_null ? -1 : mo2.khi;
            const bool e2_none = i2_e_null && d2_e_null;
            const int e2_lo = e2_none ? 1 : me2.klo, e2_hi = e2_none ? -1 : me2.khi;
            const int lo = A2P ? min(min(min(sub_lo, o_lo), e_lo), min(o2_lo, e2_lo)) - 1 : min(min(sub_lo, o_lo), e_lo) - 1;
            const int hi = A2P ? max(max(max(sub_hi, o_hi), e_hi), max(o2_hi, e2_hi)) + 1 : max(max(sub_hi, o_hi), e_hi) + 1;
            const int len = hi - lo + 1;
            const int narr = A2P ? 5 : LIN ? 1 : 1 + (d_out_null ? 0 : 1) + (i_out_null ? 0 : 1);   // (A2P: all five rows, at fixed places)
            // allocate_new_score, wfa.c:143-183: an LDS slot when the wavefront fits one; an HBM pool
            // region when it does not, and always with BACKTRACE (history)
            const bool inlds = ring_slots > 0 && len <= slot_w;
            const bool in_pool = BT || !inlds;
            if (in_pool && (pidx_t)pool_used + (pidx_t)len * narr > pool_cap) {
                if (BT) {   // allocate_new(): "out of memory" + exit(1), dpu_allocator_wram.c:19-23
                    status = AIM_PAIR_NOMEM;
                    final_score = score;
                    break;
                }
                pool_used = 0;   // score-only: the pool is a ring sized for the live window
                // The plan never hands a score-only wavefront less than the live window ((R+2) * 3 * (2*MAX_SCORE+3)
                // entries, make_plan); a wavefront that still does not fit after the wrap would run over the next
                // workgroup's scratch, so it is reported like the DPU arena's "out of memory" instead.
                if (sizeof(OFF) == 2 ? (uint32_t)(len * narr) > (uint32_t)pool_cap : (pidx_t)len * narr > pool_cap) {
                    status = AIM_PAIR_NOMEM;
                    final_score = score;
                    break;
                }
            }
            cur.flags = WF_PRESENT | (i_out_null ? WF_INULL : WF_HASI) | (d_out_null ? WF_DNULL : WF_HASD) | (inlds ? WF_INLDS : 0);
            cur.klo = cur.lo = lo;
            cur.khi = cur.hi = hi;
            cur.off_m = in_pool ? pool_used : -1;
            if constexpr (A2P) {
                cur.flags |= (i2_out_null ? 0 : WF_HASI2) | (d2_out_null ? 0 : WF_HASD2);
                cur.off_i = in_pool ? pool_used + len : -1;
                cur.off_d = in_pool ? pool_used + 2 * len : -1;
            } else if constexpr (LIN) {
                cur.off_i = cur.off_d = -1;
            } else {
                cur.off_d = (d_out_null || !in_pool) ? -1 : pool_used + len;
                cur.off_i = (i_out_null || !in_pool) ? -1 : pool_used + len * (d_out_null ? 1 : 2);
            }
            if (in_pool) pool_used += len * narr;
            wf_put_meta(ctx, score, cur, lane);
            // affine_wfa_compute_offsets, wfa.c:231-266 -- one body, LDS-typed and generic call sites (see extend)
            auto compute_row = [&](const awf_t *r_mo, const awf_t *r_ie, const awf_t *r_de, const awf_t *r_ms, awf_t *om, awf_t *oi,
                                   awf_t *od, const awf_t *r_mo2, const awf_t *r_ie2, const awf_t *r_de2, awf_t *oi2, awf_t *od2) {
                for (int k = lo + lane; k <= hi; k += kWave) {
                    if constexpr (LIN) {   // M only; out of range: NULL (wfa_group_kernel computes the same offsets)
                        const int ins_g = (!m_o_null && o_lo <= k - 1 && k - 1 <= o_hi) ? (int)r_mo[k - 1] : kAwfNull;
                        const int ins_l = ins_g == kAwfNull ? kAwfNull : (int)(awf_t)(ins_g + 1);
                        const int del_l = (!m_o_null && o_lo <= k + 1 && k + 1 <= o_hi) ? (int)r_mo[k + 1] : kAwfNull;
                        const int sub_l = (!m_sub_null && sub_lo <= k && k <= sub_hi) ? (int)(awf_t)(r_ms[k] + 1) : kAwfNull;
                        om[k - lo] = (awf_t)max(del_l, max(sub_l, ins_l));
                        continue;
                    }
                    int ins = -10;
                    if (!i_out_null) {
                        const int ins_g = (!m_o_null && o_lo <= k - 1 && k - 1 <= o_hi) ? (int)r_mo[k - 1] : kAwfNull;
                        const int ins_i = (!i_e_null && e_lo <= k - 1 && k - 1 <= e_hi) ? (int)r_ie[k - 1] : kAwfNull;
                        ins = (ins_g == kAwfNull && ins_i == kAwfNull) ? kAwfNull : (int)(awf_t)(max(ins_g, ins_i) + 1);
                        oi[k - lo] = (awf_t)ins;
                        if (BT && inlds) pool[cur.off_i + (k - lo)] = (awf_t)ins;
                    }
                    int del = -10;
                    if (!d_out_null) {
                        const int del_g = (!m_o_null && o_lo <= k + 1 && k + 1 <= o_hi) ? (int)r_mo[k + 1] : kAwfNull;
                        const int del_d = (!d_e_null && e_lo <= k + 1 && k + 1 <= e_hi) ? (int)r_de[k + 1] : kAwfNull;
                        del = max(del_g, del_d);
                        od[k - lo] = (awf_t)del;
                        if (BT && inlds) pool[cur.off_d + (k - lo)] = (awf_t)del;
                    }
                    int sub = -10;
                    if (!m_sub_null) sub = (sub_lo <= k && k <= sub_hi) ? (int)(awf_t)(r_ms[k] + 1) : kAwfNull;
                    int best = max(del, max(sub, ins));
                    if constexpr (A2P) {   // absent or out of range: NULL (a piece 2 that never fires changes no M offset)
                        int ins2 = kAwfNull, del2 = kAwfNull;
                        if (!i2_out_null) {
                            const int g_ = (!m_o2_null && o2_lo <= k - 1 && k - 1 <= o2_hi) ? (int)r_mo2[k - 1] : kAwfNull;
                            const int i_ = (!i2_e_null && e2_lo <= k - 1 && k - 1 <= e2_hi) ? (int)r_ie2[k - 1] : kAwfNull;
                            ins2 = (g_ == kAwfNull && i_ == kAwfNull) ? kAwfNull : (int)(awf_t)(max(g_, i_) + 1);
                            oi2[k - lo] = (awf_t)ins2;
                            if (BT && inlds) pool[cur.off_m + 3 * len + (k - lo)] = (awf_t)ins2;
                        }
                        if (!d2_out_null) {
                            const int g_ = (!m_o2_null && o2_lo <= k + 1 && k + 1 <= o2_hi) ? (int)r_mo2[k + 1] : kAwfNull;
                            const int d_ = (!d2_e_null && e2_lo <= k + 1 && k + 1 <= e2_hi) ? (int)r_de2[k + 1] : kAwfNull;
                            del2 = max(g_, d_);
                            od2[k - lo] = (awf_t)del2;
                            if (BT && inlds) pool[cur.off_m + 4 * len + (k - lo)] = (awf_t)del2;
                        }
                        best = max(best, max(ins2, del2));
                    }
                    om[k - lo] = (awf_t)best;
                }
            };
            const bool all_lds = inlds && (m_o_null || (mo.flags & WF_INLDS)) && (e_none || (me.flags & WF_INLDS)) &&
                                 (m_sub_null || (ms.flags & WF_INLDS)) &&
                                 (!A2P || ((m_o2_null || (mo2.flags & WF_INLDS)) && (e2_none || (me2.flags & WF_INLDS))));
            if (all_lds) {
                compute_row(slot(s_o < 0 ? 0 : s_o, 0) - mo.lo, slot(s_e < 0 ? 0 : s_e, 1) - me.lo, slot(s_e < 0 ? 0 : s_e, 2) - me.lo,
                            slot(s_sub < 0 ? 0 : s_sub, 0) - ms.lo, slot(score, 0), slot(score, 1), slot(score, 2),
                            A2P ? slot(s_o2 < 0 ? 0 : s_o2, 0) - mo2.lo : nullptr, A2P ? slot(s_e2 < 0 ? 0 : s_e2, 3) - me2.lo : nullptr,
                            A2P ? slot(s_e2 < 0 ? 0 : s_e2, 4) - me2.lo : nullptr, A2P ? slot(score, 3) : nullptr, A2P ? slot(score, 4) : nullptr);
            } else {
                compute_row(m_o_null ? nullptr : rowp(mo, s_o, 0), i_e_null ? nullptr : rowp(me, s_e, 1),
                            d_e_null ? nullptr : rowp(me, s_e, 2), m_sub_null ? nullptr : rowp(ms, s_sub, 0),
                            inlds ? slot(score, 0) : pool + cur.off_m, inlds ? slot(score, 1) : pool + cur.off_i,
                            inlds ? slot(score, 2) : pool + cur.off_d,
                            (!A2P || m_o2_null) ? nullptr : rowp(mo2, s_o2, 0), (!A2P || i2_e_null) ? nullptr : rowp(me2, s_e2, 3),
                            (!A2P || d2_e_null) ? nullptr : rowp(me2, s_e2, 4), !A2P ? nullptr : inlds ? slot(score, 3) : pool + cur.off_m + 3 * len,
                            !A2P ? nullptr : inlds ? slot(score, 4) : pool + cur.off_m + 4 * len);
            }
            sync(inlds);
        }
        __syncthreads();   // history and descriptors in HBM are complete before the traceback reads them

        // ---- affine_wavefronts_backtrace, wfa_backtracing.c:210-351 ---------------
        // Wave-uniform scalar walk; the ops row is pre-filled with 'M' so match
        // runs only move begin_offset, and gap runs are filled by all lanes.
        if (BT && status == AIM_PAIR_OK && final_score <= MS) {
            enum { BT_M = 0, BT_I = 1, BT_D = 2, BT_I2 = 3, BT_D2 = 4 };
            const int ops_cap = 2 * rs;
            int sc = final_score, k = EF ? end_k : ak;
            WfMeta m0 = ctx.gmeta[sc];
            int offset = pool[m0.off_m + (k - m0.lo)];
            auto valid_loc = [&](int kk, int off) {
                const int v = off - kk, h = off;
                return v > 0 && v <= plen && h > 0 && h <= tlen;
            };
            auto put_run = [&](char ch, int count) {   // ops[begin--] = ch, count times
                for (int i = lane; i < count; i += kWave) {
                    const int at = begin_offset - i;
                    if (at >= 0 && at < ops_cap) ops[at] = ch;
                }
                if (count > 0) begin_offset -= count;
            };
            bool valid = valid_loc(k, offset);
            int bt = BT_M;
            int v = offset - k, h = offset;
            if (EF) {   // the trailing free run: the end cell sits on the bottom or the right border
                if (v == plen && h < tlen) put_run('I', tlen - h);
                else if (h == tlen && v < plen) put_run('D', plen - v);
            }
            while (v > 0 && h > 0 && sc > 0) {
                if (!valid) {
                    valid = valid_loc(k, offset);
                    if (valid) {   // add_trailing_gap, wfa_backtracing.c:48-69
                        if (k < ak) put_run('I', ak - k);
                        else if (k > ak) put_run('D', k - ak);
                    }
                }
                const int s_o = sc - OE, s_e = sc - E, s_x = sc - X;
                WfMeta mo, me, mx;
                mo.flags = me.flags = mx.flags = 0;
                if (s_o >= 0) mo = ctx.gmeta[s_o];
                if (!LIN && s_e >= 0) me = ctx.gmeta[s_e];   // (LIN: no I / D components: D, then I, then X, all from M)
                if (s_x >= 0 && bt == BT_M) mx = ctx.gmeta[s_x];
                int del_ext = kAwfNull, del_open = kAwfNull, ins_ext = kAwfNull, ins_open = kAwfNull, misms = kAwfNull;
                if (A2P ? (bt == BT_M || bt == BT_D) : bt != BT_I) {   // (A2P: not in the piece-2 states)
                    if ((me.flags & WF_PRESENT) && !(me.flags & WF_DNULL) && me.klo <= k + 1 && k + 1 <= me.khi)
                        del_ext = pool[me.off_d + (k + 1 - me.lo)];
                    if ((mo.flags & WF_PRESENT) && mo.klo <= k + 1 && k + 1 <= mo.khi)
                        del_open = pool[mo.off_m + (k + 1 - mo.lo)];
                }
                if (A2P ? (bt == BT_M || bt == BT_I) : bt != BT_D) {
                    if ((me.flags & WF_PRESENT) && (me.flags & WF_HASI) && me.klo <= k - 1 && k - 1 <= me.khi)
                        ins_ext = (awf_t)(pool[me.off_i + (k - 1 - me.lo)] + 1);
                    if ((mo.flags & WF_PRESENT) && mo.klo <= k - 1 && k - 1 <= mo.khi)
                        ins_open = (awf_t)(pool[mo.off_m + (k - 1 - mo.lo)] + 1);
                }
                if (bt == BT_M) {
                    if ((mx.flags & WF_PRESENT) && mx.klo <= k && k <= mx.khi)
                        misms = (awf_t)(pool[mx.off_m + (k - mx.lo)] + 1);
                }
                int del2_ext = kAwfNull, del2_open = kAwfNull, ins2_ext = kAwfNull, ins2_open = kAwfNull;
                if constexpr (A2P) {   // piece 2: M at s - (o2+e2), I2 / D2 at s - e2 (rows at off_m + 3 / 4 * len)
                    const int s_o2 = sc - OE2, s_e2 = sc - E2;
                    WfMeta mo2, me2;
                    mo2.flags = me2.flags = 0;
                    if (s_o2 >= 0) mo2 = ctx.gmeta[s_o2];
                    if (s_e2 >= 0) me2 = ctx.gmeta[s_e2];
                    const int len2 = me2.hi - me2.lo + 1;
                    if (bt == BT_M || bt == BT_D2) {
                        if ((me2.flags & WF_PRESENT) && (me2.flags & WF_HASD2) && me2.klo <= k + 1 && k + 1 <= me2.khi)
                            del2_ext = pool[me2.off_m + 4 * len2 + (k + 1 - me2.lo)];
                        if ((mo2.flags & WF_PRESENT) && mo2.klo <= k + 1 && k + 1 <= mo2.khi)
                            del2_open = pool[mo2.off_m + (k + 1 - mo2.lo)];
                    }
                    if (bt == BT_M || bt == BT_I2) {
                        if ((me2.flags & WF_PRESENT) && (me2.flags & WF_HASI2) && me2.klo <= k - 1 && k - 1 <= me2.khi)
                            ins2_ext = (awf_t)(pool[me2.off_m + 3 * len2 + (k - 1 - me2.lo)] + 1);
                        if ((mo2.flags & WF_PRESENT) && mo2.klo <= k - 1 && k - 1 <= mo2.khi)
                            ins2_open = (awf_t)(pool[mo2.off_m + (k - 1 - mo2.lo)] + 1);
                    }
                }
                const int max_del = max(del_ext, del_open);
                const int max_ins = max(ins_ext, ins_open);
                const int max_all = A2P ? max(max(misms, max(max_ins, max_del)), max(max(del2_ext, del2_open), max(ins2_ext, ins2_open)))
                                        : max(misms, max(max_ins, max_del));
                if (bt == BT_M) {
                    const int num_matches = offset - max_all;
                    if (num_matches > 0) begin_offset -= num_matches;   // 'M' already in place
                    offset = max_all;
                    v = offset - k;
                    h = offset;
                    if (v <= 0 || h <= 0) break;
                }
                char op;
                if (max_all == del_ext) { op = 'D'; sc = s_e; ++k; bt = BT_D; }
                else if (max_all == del_open) { op = 'D'; sc = s_o; ++k; bt = BT_M; }
                else if (max_all == ins_ext) { op = 'I'; sc = s_e; --k; offset = (awf_t)(offset - 1); bt = BT_I; }
                else if (max_all == ins_open) { op = 'I'; sc = s_o; --k; offset = (awf_t)(offset - 1); bt = BT_M; }
                else if (A2P && max_all == del2_ext) { op = 'D'; sc = sc - E2; ++k; bt = BT_D2; }
                else if (A2P && max_all == del2_open) { op = 'D'; sc = sc - OE2; ++k; bt = BT_M; }
                else if (A2P && max_all == ins2_ext) { op = 'I'; sc = sc - E2; --k; offset = (awf_t)(offset - 1); bt = BT_I2; }
                else if (A2P && max_all == ins2_open) { op = 'I'; sc = sc - OE2; --k; offset = (awf_t)(offset - 1); bt = BT_M; }
                else if (max_all == misms) { op = 'X'; sc = s_x; offset = (awf_t)(offset - 1); }
                else { status = AIM_PAIR_WFA_NO_LINK; break; }
                if (valid) {
                    if (lane == 0 && begin_offset >= 0 && begin_offset < ops_cap) ops[begin_offset] = op;
                    --begin_offset;
                }
                v = offset - k;
                h = offset;
            }
            if (status == AIM_PAIR_OK) {
                if (sc == 0) {
                    if (EF) {   // the score-0 match stroke from (max(-k, 0), max(k, 0)), then the leading free run
                        const int h0 = max(k, 0);
                        if (offset > h0) begin_offset -= offset - h0;
                        if (k > 0) put_run('I', k);
                        else if (k < 0) put_run('D', -k);
                    } else if (offset > 0) begin_offset -= offset;
                } else {
                    if (v > 0) put_run('D', v);
                    if (h > 0) put_run('I', h);
                }
                ++begin_offset;
            }
        }

        if (EF && status == AIM_PAIR_OK && final_score > MS) begin_offset = end_offset;   // over the cap: empty CIGAR
        if (lane == 0) {
            aim_result_t r;
            r.max_operations = max_ops;
            r.begin_offset = begin_offset;
            r.end_offset = end_offset;
            r.score = final_score;
            r.status = status;
            r.idx = rq.idx;
            store_result(a, pair, r);
        }
    }
}

// What make_plan (capi_plan.hip) launches wfa_wave_kernel with, alone or over a lane / group kernel's to-do list.
struct WfaWavePlan {
    uint32_t grid;
    size_t lds;
    uint64_t scratch_per_wg;   // WfMeta array + pool of one wave
    uint32_t pool_cap, meta_cap, ring_slots, slot_w;
    bool seq_lds;
    uint64_t wide;             // ends-free: diagonals every wavefront is wider by
};
enum { kWfaWaveOk = 0, kWfaWaveNoPool, kWfaWaveNoScore0, kWfaWaveNoWindow };   // wfa_wave_plan: what does not fit the budget

// pb / tb: the ends-free begin lengths (0 without AIM_FLAG_ENDSFREE); o2 / e2: the second gap piece of AIM_FLAG_AFFINE2P.
inline int wfa_wave_plan(const aim_params_t &p, uint32_t n_pairs, const Knobs &kn, uint64_t budget, int pb, int tb, int o2, int e2,
                         WfaWavePlan *w)
{
    const bool bt = p.flags & AIM_FLAG_BACKTRACE;
    const bool a2p = p.flags & AIM_FLAG_AFFINE2P;
    const bool lin = p.flags & AIM_FLAG_LINEAR;
    const uint64_t off_b = (p.flags & AIM_FLAG_WFA_W32) ? sizeof(int32_t) : sizeof(int16_t);   // bytes per offset (AIM_FLAG_WFA_W32)
    const uint64_t ms = (uint64_t)p.max_score;
    // ends-free: every wavefront is up to PB + TB diagonals wider (the free lengths clamp to the pairs' lengths <= READ_SIZE)
    const uint64_t wide = (uint64_t)std::min(pb, p.read_size) + (uint64_t)std::min(tb, p.read_size);
    w->wide = wide;
    // affine2p: five rows per wavefront (M, I1, D1, I2, D2) and a live window of max(x, o1+e1, o2+e2) + 1 scores; gap-linear: M alone
    const uint64_t nc = a2p ? 5 : lin ? 1 : 3;
    const int Rw = std::max(std::max(p.mismatch, p.gap_o + p.gap_e), a2p ? o2 + e2 : 0);
    const uint64_t full = nc * (ms + 2) * (ms + 2 + wide) + 64;
    uint64_t cap;
    if (bt) {
        cap = full;
    } else {   // score-only: the pool is a ring that must hold the live window (scores s-R .. s) plus the one being built
        const uint64_t R = (uint64_t)Rw;
        cap = std::min(full, (R + 2) * nc * (2 * ms + 3 + wide));
    }
    const uint64_t cap_min = bt ? 0 : cap;   // below this a score-only ring would overwrite wavefronts still in use
    w->meta_cap = (uint32_t)(ms + 2);
    // LDS ring for the live window of wavefronts: max(x, o+e)+1 slots of slot_w diagonals (M, I, D)
    {
        const uint32_t R = (uint32_t)Rw;
        uint32_t sw = 16;
        while (sw < 2 * (uint32_t)ms + 3 + (uint32_t)wide && sw < 128) sw *= 2;   // 128: keeps 16 workgroups resident per CU at l = 1000 (measured +9 % over 256)
        if (kn.wfa_slotw >= 0) sw = (uint32_t)std::max(16, kn.wfa_slotw) & ~15u;
        while (sw > 16 && (uint64_t)(R + 1) * nc * sw * off_b > 24 * 1024) sw /= 2;
        const bool ring_ok = (uint64_t)(R + 1) * nc * sw * off_b <= 24 * 1024 && !kn.wfa_no_ring;
        w->ring_slots = ring_ok ? R + 1 : 0;
        w->slot_w = ring_ok ? sw : 0;
    }
    const size_t seq_bytes = 2 * ((size_t)p.read_size + 8);
    w->seq_lds = seq_bytes <= 40 * 1024;
    const size_t ring_bytes = ((size_t)w->ring_slots * nc * w->slot_w * off_b + 15) & ~(size_t)15;
    w->lds = kMetaRing * sizeof(WfMeta) + ring_bytes + (w->seq_lds ? seq_bytes : 0);
    // persistent single-wave workgroups: exactly what is resident (4 waves/SIMD by VGPRs, 160 KiB LDS per CU);
    // a larger grid runs in uneven rounds
    // (affine2p with BACKTRACE: 142-148 VGPRs, 3 waves per SIMD)
    const uint32_t wg_per_cu = (uint32_t)std::min<size_t>(a2p && bt ? 12 : 16, lds_workgroups_per_cu(w->lds));
    uint32_t grid = resident_grid(kn, wg_per_cu);
    const uint32_t need = ((n_pairs + 7u) / 8u) * 8u;
    if (grid > need) grid = std::max(8u, need);
    uint64_t per = (uint64_t)w->meta_cap * sizeof(WfMeta) + cap * off_b;
    per = (per + 255) & ~255ull;
    while (grid > 2 * kn.cus && grid > 16 && per * grid > budget) grid = ((grid / 2) + 7u) & ~7u;
    if (per * grid > budget) {
        const uint64_t meta_b = (uint64_t)w->meta_cap * sizeof(WfMeta);
        if (bt) {
            // With BACKTRACE the pool is a bump arena like the DPU's (allocate_new_score, wfa.c:143-183): a smaller one
            // is legal and a pair that outgrows it reports AIM_PAIR_NOMEM (dpu_allocator_wram.c:19-23 "out of memory").
            uint64_t avail = budget / grid;
            if (avail < meta_b + 4096) return kWfaWaveNoPool;
            cap = (avail - meta_b - 256) / off_b;
            if (cap < wide + 1) return kWfaWaveNoScore0;
            per = (meta_b + cap * off_b + 255) & ~255ull;
        } else {
            // Score-only: the pool is a ring and must keep its full live window (a shrunken ring silently overwrites
            // wavefronts score-x / score-o-e / score-e still read). Fewer workgroups instead, down to one per XCD.
            while (grid > 8 && per * grid > budget) grid -= 8;
            if (per * grid > budget || cap < cap_min) return kWfaWaveNoWindow;
        }
    }
    w->grid = grid;
    w->pool_cap = (uint32_t)std::min<uint64_t>(cap, 0x7fffffffu);
    w->scratch_per_wg = per;
    return kWfaWaveOk;
}

// Kernels are instantiated in ONE translation unit (tu_*.hip defines AIM_TU_WFA_WAVE); every other includer sees the declaration only.
#ifdef AIM_TU_WFA_WAVE
template <typename OFF>
void wfa_wave_launch_off(bool bt, bool red, bool seq_lds, uint32_t grid, size_t lds, const KArgs &ka, hipStream_t s)
{
#define AIM_WFW(BTV, REDV)                                                                                              \
    do {                                                                                                                \
        if (seq_lds) hipLaunchKernelGGL((wfa_wave_kernel<BTV, REDV, true, false, false, false, OFF>), dim3(grid), dim3(kWave), lds, s, ka);  \
        else hipLaunchKernelGGL((wfa_wave_kernel<BTV, REDV, false, false, false, false, OFF>), dim3(grid), dim3(kWave), lds, s, ka);         \
    } while (0)
#define AIM_WFW_EF(BTV)                                                                                                 \
    do {                                                                                                                \
        if (seq_lds) hipLaunchKernelGGL((wfa_wave_kernel<BTV, false, true, true, false, false, OFF>), dim3(grid), dim3(kWave), lds, s, ka);  \
        else hipLaunchKernelGGL((wfa_wave_kernel<BTV, false, false, true, false, false, OFF>), dim3(grid), dim3(kWave), lds, s, ka);         \
    } while (0)
#define AIM_WFW_A2P(BTV)                                                                                                \
    do {                                                                                                                \
        if (seq_lds) hipLaunchKernelGGL((wfa_wave_kernel<BTV, false, true, false, true, false, OFF>), dim3(grid), dim3(kWave), lds, s, ka);  \
        else hipLaunchKernelGGL((wfa_wave_kernel<BTV, false, false, false, true, false, OFF>), dim3(grid), dim3(kWave), lds, s, ka);         \
    } while (0)
#define AIM_WFW_LIN(BTV)                                                                                                \
    do {                                                                                                                \
        if (seq_lds) hipLaunchKernelGGL((wfa_wave_kernel<BTV, false, true, false, false, true, OFF>), dim3(grid), dim3(kWave), lds, s, ka);  \
        else hipLaunchKernelGGL((wfa_wave_kernel<BTV, false, false, false, false, true, OFF>), dim3(grid), dim3(kWave), lds, s, ka);         \
    } while (0)
    if (ka.p.flags & AIM_FLAG_AFFINE2P) {   // (validate_params: never with REDUCE or ENDSFREE)
        if (bt) AIM_WFW_A2P(true);
        else AIM_WFW_A2P(false);
    } else if (ka.p.flags & AIM_FLAG_LINEAR) {   // (validate_params: never with REDUCE, ENDSFREE or AFFINE2P)
        if (bt) AIM_WFW_LIN(true);
        else AIM_WFW_LIN(false);
    } else if (ka.p.flags & AIM_FLAG_ENDSFREE) {   // (validate_params: never with REDUCE)
        if (bt) AIM_WFW_EF(true);
        else AIM_WFW_EF(false);
    } else if (bt && red) AIM_WFW(true, true);
    else if (bt) AIM_WFW(true, false);
    else if (red) AIM_WFW(false, true);
    else AIM_WFW(false, false);
#undef AIM_WFW
#undef AIM_WFW_EF
#undef AIM_WFW_A2P
#undef AIM_WFW_LIN
}

void wfa_wave_launch(bool bt, bool red, bool seq_lds, uint32_t grid, size_t lds, const KArgs &ka, hipStream_t s)
{
    if (ka.p.flags & AIM_FLAG_WFA_W32) wfa_wave_launch_off<int32_t>(bt, red, seq_lds, grid, lds, ka, s);
    else wfa_wave_launch_off<int16_t>(bt, red, seq_lds, grid, lds, ka, s);
}
#else
void wfa_wave_launch(bool bt, bool red, bool seq_lds, uint32_t grid, size_t lds, const KArgs &ka, hipStream_t s);
#endif

}  // namespace aim
