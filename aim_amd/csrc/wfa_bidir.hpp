// wfa_bidir.hpp -- bidirectional gap-affine WFA with CIGAR (AIM_FLAG_WFA_BIDIR): ONE PAIR PER 64-LANE WAVEFRONT, O(MAX_SCORE)
// memory per workgroup (Marco-Sola, Eizenga, Guarracino, Paten, Garrison, Moreto, "Optimal gap-affine alignment in O(s) space",
// Bioinformatics 2023). tests/bidir_model.py is the same algorithm in Python, checked against a brute-force Gotoh DP.
//
// The plan runs wfa_wave_kernel first with MAX_SCORE = min(MAX_SCORE, T): every pair whose score is <= T gets the flag-less
// result and CIGAR bytes from the reference's own WFA and walk. This kernel then takes the pairs that came back over T:
//
// - breakpoint: forward WFA from the start and reverse WFA (on the reversed sequences) from the end, score-only, each in a window
//   of max(x, o+e) + 2 scores in the workgroup's HBM scratch, every cell clipped to the matrix. A collision phase on
//   anti-diagonals, then the overlap phase: each new wavefront against the other direction's last max(x, o+e) + 1 scores;
//   forward diagonal k meets reverse diagonal (tlen - plen) - k, M-M when f + r >= tlen, I-I / D-D likewise at one gap-open
//   less. Tie rule: the first strictly better candidate in the order (newer check first; within a check the other direction's
//   scores from the newest down, then M, I, D, then the forward diagonals upward: one ballot per 64 diagonals, its lowest lane).
//   The search stops by the paper's rule: no later overlap can beat the best one found.
// - recursion: an explicit stack of sub-problems (v0, v1, h0, h1, start component, end component, score estimate) in LDS,
//   right half first, so the ops row is written backwards from end_offset like the reference's walk writes it.
// - base case: a sub-problem whose estimate is <= T is first tried with forward WFA with a history of up to T scores in a
//   per-workgroup arena (fixed stride, (T + 1) * 3 rows of 2T + 5 diagonals), walked in the reference's order (W7: deletion
//   extend, deletion open, insertion extend, insertion open, mismatch), from the end component back to the start component. A
//   sub-problem over T gets a breakpoint of its own; one of score <= T after all goes to the base case.
//   An empty side is one gap run, written directly; a short non-empty side with a score over T takes further breakpoints
//   (the arena holds T scores, not a long gap), which stay correct and end.
//
// Components: a sub-problem that starts inside a gap has it open already (score 0 holds that component at offset 0 next to
// M); one that ends inside a gap must end with it and pays its open (the reverse direction's first wavefront is that open,
// at score o + e). With these two rules a gap-gap overlap costs o less than the sum in every case.
#pragma once

#include "aim_device.hpp"

namespace aim {

constexpr int kBidirStack = 64;      // sub-problems on the LDS stack (depth O(log MAX_SCORE))
constexpr int kBidirMaxScope = 62;   // max(x, o + e) + 1 the window ring admits (the plan refuses more)
// Resident workgroups per CU the plan assumes: 4 single-wave workgroups per SIMD. The kernel's launch bound pins it (at most 128
// VGPRs); tests/test_bidir_cpu.py checks the code object (VGPRs, no scratch) against it.
constexpr int kBidirWavesPerSimd = 4;
constexpr int kBidirPerCu = 4 * kBidirWavesPerSimd;

struct BidirSub {
    int v0, v1, h0, h1;
    int cs, ce, est, pad;
};

// KArgs from the plan: pool_cap = T (the base-case threshold), slot_w = kw (window rows cover diagonals [-kw, kw]).
template <typename OFF>
__global__ __launch_bounds__(64, kBidirWavesPerSimd) void wfa_bidir_kernel(KArgs a)
{
    typedef OFF awf_t;
    constexpr int kNull = sizeof(OFF) == 2 ? -16384 : INT32_MIN / 2;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    debug_poison_lds(a, smem);
    const int lane = threadIdx.x;
    const int rs = a.p.read_size;
    const int X = a.p.mismatch, O = a.p.gap_o, E = a.p.gap_e, OE = O + E;
    const int MS = a.p.max_score;
    const int scope = max(X, OE) + 1;
    const int NS = scope + 1;                  // window slots per direction
    const int TB = (int)a.pool_cap;            // base-case threshold T
    const int KW = (int)a.slot_w;              // window rows cover diagonals [-KW, KW]
    const int WW = 2 * KW + 1;
    const int WB = 2 * TB + 5;                 // arena rows cover diagonals [-(TB + 2), TB + 2]

    // LDS: window metas {lo, hi} (2 x NS), arena metas {lo, hi} (TB + 1), the stack
    int *fmeta = reinterpret_cast<int *>(smem);
    int *rmeta = fmeta + 2 * kBidirMaxScope + 4;
    int *bmeta = rmeta + 2 * kBidirMaxScope + 4;
    BidirSub *stack = reinterpret_cast<BidirSub *>(smem + (((size_t)(4 * kBidirMaxScope + 8 + 2 * (TB + 1)) * 4 + 15) & ~(size_t)15));

    char *wscr = a.scratch + (uint64_t)blockIdx.x * a.scratch_per_wave;
    awf_t *frows = reinterpret_cast<awf_t *>(wscr);
    awf_t *rrows = frows + (size_t)NS * 3 * WW;
    awf_t *arena = rrows + (size_t)NS * 3 * WW;

    for (uint32_t it = 0;; ++it) {
        uint32_t pair;
        if (!xcd_unit(a.n_pairs, it, &pair)) break;
        // the first stage's result: a pair of score <= T (or any pair when MAX_SCORE <= T, never planned here) is final
        const aim_result_t r0 = a.res[pair];
        if (r0.status != AIM_PAIR_OK || r0.score <= min(TB, MS)) continue;
        const aim_request_t rq = load_request(a, pair);
        const int plen = rq.pattern_len, tlen = rq.text_len;
        const unsigned char *gP = reinterpret_cast<const unsigned char *>(a.patterns + (uint64_t)pair * rs);
        const unsigned char *gT = reinterpret_cast<const unsigned char *>(a.texts + (uint64_t)pair * rs);
        const uint32_t *gP4 = reinterpret_cast<const uint32_t *>(gP), *gT4 = reinterpret_cast<const uint32_t *>(gT);
        const int last_word = (rs >> 2) - 1;
        char *ops = a.ops + (uint64_t)pair * 2 * rs;
        const int ops_cap = 2 * rs;
        const int max_ops = plen + tlen;
        int begin_offset = max_ops - 1;
        int status = AIM_PAIR_OK;
        int final_score = MS + 1;
        __syncthreads();   // the previous pair's LDS and scratch reads are done

        auto put_run = [&](char ch, int count) {   // ops[begin--] = ch, count times (vector stores from lanes)
            for (int i = lane; i < count; i += kWave) {
                const int at = begin_offset - i;
                if (at >= 0 && at < ops_cap) ops[at] = ch;
            }
            if (count > 0) begin_offset -= count;
        };

        // ---- one direction's score-only window -------------------------------------------------------------------------
        // dir 0 forward over P[v0 ..), T[h0 ..); dir 1 reverse over P[.. v1), T[.. h1) read backwards. Offsets are h.
        struct Dir {
            awf_t *rows;
            int *meta;
            int score;     // newest score computed
            int first;     // first score with a wavefront
            int maxad;     // furthest anti-diagonal reached
        };
        int sv0 = 0, sv1 = 0, sh0 = 0, sh1 = 0, splen = 0, stlen = 0;   // the sub-problem of the running search
        auto row = [&](const Dir &d, int s, int c) -> awf_t * { return d.rows + ((size_t)((s % NS) * 3 + c)) * WW + KW; };
        // the match run from offset off of diagonal k, four bytes per compare (wf_extend_count's loop; the reverse direction reads the
        // words that end at its first byte and counts matching bytes from the top)
        auto extend = [&](int dir, int off, int k) -> int {
            const int h = off, v = off - k;
            const int rem = min(splen - v, stlen - h);
            if (rem <= 0) return h;
            int cnt = 0;
            if (dir == 0) {
                const int pi = sv0 + v, ti = sh0 + h;
                for (;;) {
                    const uint32_t x = load4_unaligned(gP4, pi + cnt, last_word) ^ load4_unaligned(gT4, ti + cnt, last_word);
                    const int m = x ? (__builtin_ctz(x) >> 3) : 4;
                    const int r = rem - cnt;
                    if (m < 4) { cnt += min(m, r); break; }
                    if (r <= 4) { cnt += r; break; }
                    cnt += 4;
                }
            } else {
                const int pi = sv1 - 1 - v, ti = sh1 - 1 - h;   // the first bytes compared; then downwards
                for (;;) {
                    const int r = rem - cnt;
                    if (pi - cnt < 3 || ti - cnt < 3) {   // the first bytes of a row: one at a time
                        while (cnt < rem && gP[pi - cnt] == gT[ti - cnt]) ++cnt;
                        break;
                    }
                    const uint32_t x = load4_unaligned(gP4, pi - cnt - 3, last_word) ^ load4_unaligned(gT4, ti - cnt - 3, last_word);
                    const int m = x ? (__builtin_clz(x) >> 3) : 4;
                    if (m < 4) { cnt += min(m, r); break; }
                    if (r <= 4) { cnt += r; break; }
                    cnt += 4;
                }
            }
            return h + cnt;
        };
        auto clip = [&](int off, int k, int pl, int tl) -> int {
            return (off < 0 || off > tl || off - k < 0 || off - k > pl) ? kNull : off;
        };
        auto in_window = [&](const Dir &d, int s) { return s >= d.first && s <= d.score && d.score - s < NS - 1; };
        // source cell (score s, component c, diagonal k) of a window, NULL when absent
        auto wget = [&](const Dir &d, int s, int c, int k) -> int {
            if (!in_window(d, s)) return kNull;
            const int lo = d.meta[2 * (s % NS)], hi = d.meta[2 * (s % NS) + 1];
            if (k < lo || k > hi) return kNull;
            return (int)row(d, s, c)[k];
        };
        // initial wavefront: forward starting in component cs (open gap: that component at offset 0 next to M); reverse ending in
        // ce (the gap's open is its first wavefront, at score o + e)
        auto init_dir = [&](int dir, Dir &d, int comp) {
            d.maxad = -1;
            if (dir == 1 && comp != 0) {
                const int k = comp == 1 ? 1 : -1, off = comp == 1 ? 1 : 0;
                d.first = d.score = OE;
                const bool ok = clip(off, k, splen, stlen) >= 0;
                if (lane == 0) {
                    d.meta[2 * (OE % NS)] = ok ? k : 1;
                    d.meta[2 * (OE % NS) + 1] = ok ? k : 0;
                }
                if (ok && lane == 0) {
                    const int m = extend(dir, off, k);
                    row(d, OE, 0)[k] = (awf_t)m;
                    row(d, OE, 1)[k] = (awf_t)(comp == 1 ? off : kNull);
                    row(d, OE, 2)[k] = (awf_t)(comp == 2 ? off : kNull);
                    d.maxad = 2 * m - k;
                }
            } else {
                d.first = d.score = 0;
                if (lane == 0) {
                    d.meta[0] = 0;
                    d.meta[1] = 0;
                    const int m = extend(dir, 0, 0);
                    row(d, 0, 0)[0] = (awf_t)m;
                    row(d, 0, 1)[0] = (awf_t)(comp == 1 ? 0 : kNull);
                    row(d, 0, 2)[0] = (awf_t)(comp == 2 ? 0 : kNull);
                    d.maxad = 2 * m;
                }
            }
            d.maxad = __shfl(d.maxad, 0);
            __syncthreads();
        };
        // compute + extend the next score of a window
        auto step = [&](int dir, Dir &d) {
            const int s = d.score + 1;
            int lo = 0x7fffffff, hi = -0x7fffffff;
            const int srcs[3] = {s - X, s - OE, s - E};
            for (int j = 0; j < 3; ++j)
                if (in_window(d, srcs[j])) {
                    const int l = d.meta[2 * (srcs[j] % NS)], h = d.meta[2 * (srcs[j] % NS) + 1];
                    if (l <= h) { lo = min(lo, l - 1); hi = max(hi, h + 1); }
                }
            lo = max(lo, max(-splen, -KW));
            hi = min(hi, min(stlen, KW));
            int ad = -1;
            awf_t *om = row(d, s, 0), *oi = row(d, s, 1), *od = row(d, s, 2);
            for (int k = lo + lane; k <= hi; k += kWave) {
                // every candidate clipped on its own (the walk tests them one by one): a diagonal's in-matrix offsets are an interval
                const int ins = max(clip(wget(d, s - OE, 0, k - 1) + 1, k, splen, stlen), clip(wget(d, s - E, 1, k - 1) + 1, k, splen, stlen));
                const int dd = max(clip(wget(d, s - OE, 0, k + 1), k, splen, stlen), clip(wget(d, s - E, 2, k + 1), k, splen, stlen));
                const int sub = clip(wget(d, s - X, 0, k) + 1, k, splen, stlen);
                const int best = max(max(ins, dd), sub);
                int m = kNull;
                if (best >= 0) {
                    m = extend(dir, best, k);
                    ad = max(ad, 2 * m - k);
                }
                om[k] = (awf_t)m;
                oi[k] = (awf_t)ins;
                od[k] = (awf_t)dd;
            }
            __syncthreads();   // the rows are in HBM: stores complete before the next step reads them
            if (lane == 0) {
                d.meta[2 * (s % NS)] = lo;
                d.meta[2 * (s % NS) + 1] = hi;
            }
            d.score = s;
            d.maxad = max(d.maxad, -wave_min_i32(-ad));
            __syncthreads();
        };
        // Breakpoint state
        int bp_score, bp_v = 0, bp_h = 0, bp_comp = 0, bp_sf = 0, bp_sr = 0;
        // the newest wavefront of one direction against the other's last `scope` scores
        auto overlap = [&](const Dir &fw, const Dir &rv, bool new_fwd) {
            const Dir &nw = new_fwd ? fw : rv;
            const Dir &od = new_fwd ? rv : fw;
            const int kend = stlen - splen;
            for (int i = 0; i < scope; ++i) {
                const int so = od.score - i;
                if (so < od.first) break;
                for (int c = 0; c < 3; ++c) {
                    const int cand = nw.score + so - (c ? O : 0);
                    if (cand >= bp_score) continue;
                    const int sfw = new_fwd ? nw.score : so, srv = new_fwd ? so : nw.score;
                    const int flo = fw.meta[2 * (sfw % NS)], fhi = fw.meta[2 * (sfw % NS) + 1];
                    const int rlo = rv.meta[2 * (srv % NS)], rhi = rv.meta[2 * (srv % NS) + 1];
                    const int lo = max(flo, kend - rhi), hi = min(fhi, kend - rlo);
                    const awf_t *fr = row(fw, sfw, c);
                    const awf_t *rr = row(rv, srv, c);
                    for (int base = lo; base <= hi; base += kWave) {
                        const int k = base + lane;
                        bool ok = false;
                        int f = 0;
                        if (k <= hi) {
                            f = fr[k];
                            const int r = rr[kend - k];
                            ok = f >= 0 && r >= 0 && f + r >= stlen;
                        }
                        const unsigned long long mask = __ballot(ok);
                        if (mask) {
                            const int src = __builtin_ctzll(mask);
                            const int kf = base + src;
                            const int fo = __shfl(f, src);
                            bp_score = cand;
                            bp_comp = c;
                            bp_v = fo - kf;
                            bp_h = fo;
                            bp_sf = sfw;
                            bp_sr = srv - (c ? O : 0);
                            break;
                        }
                    }
                }
            }
        };
        // The breakpoint of sub-problem (v0, v1, h0, h1, cs, ce) at a score <= bound; bp_score = bound + 1 when there is none.
        auto breakpoint = [&](int v0, int v1, int h0, int h1, int cs, int ce, int bound) {
            sv0 = v0; sv1 = v1; sh0 = h0; sh1 = h1; splen = v1 - v0; stlen = h1 - h0;
            Dir fw, rv;
            fw.rows = frows; fw.meta = fmeta;
            rv.rows = rrows; rv.meta = rmeta;
            init_dir(0, fw, cs);
            init_dir(1, rv, ce);
            bp_score = bound + 1;
            const int max_ad = splen + stlen - 1;
            bool last_fwd = false;
            while (fw.maxad + rv.maxad < max_ad) {   // collision phase
                if (fw.score + max(rv.score - scope + 1, 0) - O > bound + scope) return;
                step(0, fw);
                last_fwd = true;
                if (fw.maxad + rv.maxad >= max_ad) break;
                step(1, rv);
                last_fwd = false;
            }
            for (;;) {   // overlap phase
                if (last_fwd) {
                    if (fw.score + max(rv.score - (scope - 1), 0) - O >= bp_score) break;
                    overlap(fw, rv, true);
                    step(1, rv);
                }
                if (max(fw.score - (scope - 1), 0) + rv.score - O >= bp_score) break;
                overlap(fw, rv, false);
                step(0, fw);
                last_fwd = true;
            }
        };

        // ---- base case: forward WFA with a history of up to TB scores, clipped, then the walk ---------------------------------
        // Returns the score, or -1 over TB. Writes the ops backwards from begin_offset.
        auto base_case = [&](int v0, int v1, int h0, int h1, int cs, int ce) -> int {
            sv0 = v0; sh0 = h0; splen = v1 - v0; stlen = h1 - h0;
            const int C = TB + 2;
            auto arow = [&](int s, int c) -> awf_t * { return arena + ((size_t)s * 3 + c) * WB + C; };
            auto aget = [&](int s, int c, int k) -> int {
                if (s < 0) return kNull;
                const int lo = bmeta[2 * s], hi = bmeta[2 * s + 1];
                if (k < lo || k > hi) return kNull;
                return (int)arow(s, c)[k];
            };
            const int kend = stlen - splen;
            if (lane == 0) {
                bmeta[0] = 0; bmeta[1] = 0;
                arow(0, 0)[0] = (awf_t)extend(0, 0, 0);
                arow(0, 1)[0] = (awf_t)(cs == 1 ? 0 : kNull);
                arow(0, 2)[0] = (awf_t)(cs == 2 ? 0 : kNull);
            }
            __syncthreads();
            int s = 0;
            auto reached = [&](int sc) {
                return kend >= bmeta[2 * sc] && kend <= bmeta[2 * sc + 1] && (int)arow(sc, ce)[kend] == stlen;
            };
            while (!reached(s)) {
                if (s >= TB) return -1;
                ++s;
                int lo = 0x7fffffff, hi = -0x7fffffff;
                const int srcs[3] = {s - X, s - OE, s - E};
                for (int j = 0; j < 3; ++j)
                    if (srcs[j] >= 0) {
                        const int l = bmeta[2 * srcs[j]], h = bmeta[2 * srcs[j] + 1];
                        if (l <= h) { lo = min(lo, l - 1); hi = max(hi, h + 1); }
                    }
                lo = max(lo, max(-splen, -C));
                hi = min(hi, min(stlen, C));
                awf_t *om = arow(s, 0), *oi = arow(s, 1), *od = arow(s, 2);
                for (int k = lo + lane; k <= hi; k += kWave) {
                    const int ins = max(clip(aget(s - OE, 0, k - 1) + 1, k, splen, stlen), clip(aget(s - E, 1, k - 1) + 1, k, splen, stlen));
                    const int dd = max(clip(aget(s - OE, 0, k + 1), k, splen, stlen), clip(aget(s - E, 2, k + 1), k, splen, stlen));
                    const int sub = clip(aget(s - X, 0, k) + 1, k, splen, stlen);
                    const int best = max(max(ins, dd), sub);
                    om[k] = (awf_t)(best >= 0 ? extend(0, best, k) : kNull);
                    oi[k] = (awf_t)ins;
                    od[k] = (awf_t)dd;
                }
                if (lane == 0) { bmeta[2 * s] = lo; bmeta[2 * s + 1] = hi; }
                __syncthreads();
            }
            // the walk (wave-uniform), the reference's W7 order, clipped like the compute
            const int score = s;
            int k = kend, off = stlen, bt = ce;
            for (;;) {
                if (s == 0) {
                    if (bt == 0) begin_offset -= off;   // the leading match run ('M' already in place)
                    break;
                }
                int del_ext = kNull, del_open = kNull, ins_ext = kNull, ins_open = kNull, mis = kNull;
                if (bt != 1) {
                    del_ext = clip(aget(s - E, 2, k + 1), k, splen, stlen);
                    del_open = clip(aget(s - OE, 0, k + 1), k, splen, stlen);
                }
                if (bt != 2) {
                    ins_ext = clip(aget(s - E, 1, k - 1) + 1, k, splen, stlen);
                    ins_open = clip(aget(s - OE, 0, k - 1) + 1, k, splen, stlen);
                }
                if (bt == 0) mis = clip(aget(s - X, 0, k) + 1, k, splen, stlen);
                const int best = max(max(max(del_ext, del_open), max(ins_ext, ins_open)), mis);
                if (best < 0) { status = AIM_PAIR_WFA_NO_LINK; break; }
                if (bt == 0) {
                    begin_offset -= off - best;   // matches ('M' already in place)
                    off = best;
                }
                char op;
                if (best == del_ext) { op = 'D'; s -= E; ++k; bt = 2; }
                else if (best == del_open) { op = 'D'; s -= OE; ++k; bt = 0; }
                else if (best == ins_ext) { op = 'I'; s -= E; --k; --off; bt = 1; }
                else if (best == ins_open) { op = 'I'; s -= OE; --k; --off; bt = 0; }
                else { op = 'X'; s -= X; --off; }
                if (lane == 0 && begin_offset >= 0 && begin_offset < ops_cap) ops[begin_offset] = op;
                --begin_offset;
            }
            __syncthreads();
            return score;
        };

        // the 'M' fill of the pair's range: the walks only move begin_offset over match runs
        {
            uint32_t *o4 = reinterpret_cast<uint32_t *>(ops);
            for (int w = lane; w < (rs >> 1); w += kWave) o4[w] = 0x4D4D4D4Du;
        }
        breakpoint(0, plen, 0, tlen, 0, 0, MS);
        if (bp_score <= MS) {
            final_score = bp_score;
            int sp = 0;
            auto push = [&](int v0, int v1, int h0, int h1, int cs, int ce, int est) {
                if (lane == 0) {
                    BidirSub b;
                    b.v0 = v0; b.v1 = v1; b.h0 = h0; b.h1 = h1; b.cs = cs; b.ce = ce; b.est = est; b.pad = 0;
                    stack[sp] = b;
                }
                ++sp;
            };
            push(0, bp_v, 0, bp_h, 0, bp_comp, bp_sf);
            push(bp_v, plen, bp_h, tlen, bp_comp, 0, bp_sr);
            __syncthreads();
            while (sp > 0 && status == AIM_PAIR_OK) {
                --sp;
                const BidirSub b = stack[sp];
                __syncthreads();
                const int pl = b.v1 - b.v0, tl = b.h1 - b.h0;
                if (pl == 0 || tl == 0) {   // one gap run (or nothing)
                    put_run('D', pl);
                    put_run('I', tl);
                    continue;
                }
                if (b.est <= TB && base_case(b.v0, b.v1, b.h0, b.h1, b.cs, b.ce) >= 0) continue;
                breakpoint(b.v0, b.v1, b.h0, b.h1, b.cs, b.ce, final_score);
                if (bp_score > final_score) { status = AIM_PAIR_WFA_NO_LINK; break; }   // (a guard: the model never meets it)
                if (bp_score <= TB) {
                    if (base_case(b.v0, b.v1, b.h0, b.h1, b.cs, b.ce) < 0) status = AIM_PAIR_WFA_NO_LINK;
                    continue;
                }
                if ((bp_v == 0 && bp_h == 0) || (bp_v == pl && bp_h == tl) || sp + 2 > kBidirStack) { status = AIM_PAIR_WFA_NO_LINK; break; }
                push(b.v0, b.v0 + bp_v, b.h0, b.h0 + bp_h, b.cs, bp_comp, bp_sf);
                push(b.v0 + bp_v, b.v1, b.h0 + bp_h, b.h1, bp_comp, b.ce, bp_sr);
                __syncthreads();
            }
            ++begin_offset;
        }
        if (lane == 0) {
            aim_result_t r;
            r.max_operations = max_ops;
            r.begin_offset = (status == AIM_PAIR_OK && final_score <= MS) ? begin_offset : max_ops - 1;
            r.end_offset = max_ops;
            r.score = final_score;
            r.status = status;
            r.idx = rq.idx;
            store_result(a, pair, r);
        }
    }
}

// The shape of the second stage (make_plan: plan_wfa_bidir).
struct WfaBidirPlan {
    uint32_t grid;
    size_t lds;
    uint64_t scratch_per_wg;
    int T;        // base-case threshold
    int kw;       // window rows cover diagonals [-kw, kw]
};

// The base-case threshold T: at least 250 (the launchers' MAX_SCORE at l = 1 000, e = 5 %), and at least 2 * scope + o, the score
// above which both halves of a breakpoint score > 0 (the two directions' scores differ by less than a scope), so the recursion ends.
inline int wfa_bidir_threshold(const aim_params_t &p)
{
    const int scope = std::max(p.mismatch, p.gap_o + p.gap_e) + 1;
    return std::max(250, 2 * scope + p.gap_o);
}

inline size_t wfa_bidir_lds(int T)
{
    return ((((size_t)(4 * kBidirMaxScope + 8 + 2 * (T + 1)) * 4 + 15) & ~(size_t)15)) + kBidirStack * sizeof(BidirSub);
}

// Per-workgroup scratch: two windows of (scope + 1) x 3 rows of 2 kw + 1 offsets, and the arena of (T + 1) x 3 rows of 2T + 5.
inline uint64_t wfa_bidir_wg_bytes(const aim_params_t &p, int T, int kw)
{
    const uint64_t off_b = (p.flags & AIM_FLAG_WFA_W32) ? 4 : 2;
    const uint64_t scope = (uint64_t)std::max(p.mismatch, p.gap_o + p.gap_e) + 1;
    const uint64_t win = (scope + 1) * 3 * (2 * (uint64_t)kw + 1);
    const uint64_t arena = ((uint64_t)T + 1) * 3 * (2 * (uint64_t)T + 5);
    return ((2 * win + arena) * off_b + 255) & ~255ull;
}

#ifdef AIM_TU_WFA_BIDIR
void wfa_bidir_launch(uint32_t grid, size_t lds, const KArgs &ka, hipStream_t s)
{
    if (ka.p.flags & AIM_FLAG_WFA_W32) hipLaunchKernelGGL((wfa_bidir_kernel<int32_t>), dim3(grid), dim3(kWave), lds, s, ka);
    else hipLaunchKernelGGL((wfa_bidir_kernel<int16_t>), dim3(grid), dim3(kWave), lds, s, ka);
}
#else
void wfa_bidir_launch(uint32_t grid, size_t lds, const KArgs &ka, hipStream_t s);
#endif

}  // namespace aim
