// pair_select_body.inc -- the body of pair_select_kernel and of pair_select_est_kernel (pair.hpp includes it inside either kernel): `a` is
// the kernel's PairArgs, G its lanes per read pair. The two kernels differ in where a.min_span and a.max_span come from alone.
    const uint32_t kPairs = kPairThreads / G;
    const uint32_t cand = threadIdx.x & (G - 1u);
    const uint32_t base = (threadIdx.x & (uint32_t)(kWave - 1)) & ~(G - 1u);
    const uint32_t gm = (1u << G) - 1u, K = a.K;
    const uint32_t n_mates = a.n_reads / 2u, n_blocks = (n_mates + kPairs - 1u) / kPairs;
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint32_t m = blk * kPairs + threadIdx.x / G;
        const bool pair_live = m < n_mates, live = pair_live && cand < K;
        const uint32_t ra = 2u * m, rb = ra + 1u;
        const PairCand A = pair_load_slot(a, live, ra * K + cand), B = pair_load_slot(a, live, rb * K + cand);
        const uint32_t mask_a = (uint32_t)(__ballot(A.fl & 1u) >> base) & gm, mask_b = (uint32_t)(__ballot(B.fl & 1u) >> base) & gm;
        const uint32_t rep_a = mask_a ? (uint32_t)__ffs(mask_a) - 1u : 0u, rep_b = mask_b ? (uint32_t)__ffs(mask_b) - 1u : 0u;
        PairSel v = pair_mapped_row(a, A, B, cand, G);
        // of the two representatives -- the anchors of the rescue -- what the choice needs: the contig and the score
        const uint32_t contig_a = (uint32_t)__shfl((int)A.contig, (int)rep_a, (int)G), contig_b = (uint32_t)__shfl((int)B.contig, (int)rep_b, (int)G);
        const int score_a = __shfl(A.score, (int)rep_a, (int)G), score_b = __shfl(B.score, (int)rep_b, (int)G);
        // the rescue rows: tried as pair_rescue_rows_kernel decides it, usable when the row came back mapped; its contig is its anchor's
        const bool rescue = (a.options & AIM_PAIR_RESCUE) && !((uint32_t)(__ballot(v.cnt != 0u) >> base) & gm);
        const bool tried_a = rescue && mask_b && pair_read_len(a, pair_live, ra), tried_b = rescue && mask_a && pair_read_len(a, pair_live, rb);
#pragma unroll 1   // (one copy of the 64-bit arithmetic: unrolled, the kernel needs 68 VGPRs)
        for (uint32_t side = 0; side < 2u; ++side) {                           // (i, K) with read 2m + 1's row, then (K, j) with read 2m's; (K, K) is excluded
            const PairCand R = pair_load(a.res_sam, side ? tried_a : tried_b, side ? ra : rb, true, side ? contig_b : contig_a);
            v = pair_add(a, v, side ? B : A, R, side ? K : cand, side ? cand : K);
        }
        v = pair_butterfly(v, G);
        const uint32_t vi = v.ij >> 8, vj = v.ij & 0xffu;
        const bool both = mask_a && mask_b;
        const int unpaired = pair_clamp((int64_t)score_a + score_b + a.unpaired_penalty);
        const bool take = v.cnt && (!both || v.cost <= unpaired);              // (a tie goes to the proper combination)
        if (pair_live && cand == 0) {
            uint4 lo = make_uint4(mask_a ? ra * K + rep_a : UINT_MAX, mask_b ? rb * K + rep_b : UINT_MAX, (uint32_t)INT_MAX, (uint32_t)INT_MAX);
            uint4 hi = make_uint4(0u, (tried_a ? AIM_PAIR_RESCUE_TRIED_A : 0u) | (tried_b ? AIM_PAIR_RESCUE_TRIED_B : 0u), 0u, 0u);
            if (take) {
                lo = make_uint4(ra * K + vi, rb * K + vj, (uint32_t)v.cost, (uint32_t)v.sec);
                hi.x = v.cnt;
                hi.y |= AIM_PAIR_PROPER | (vi == K ? AIM_PAIR_RESCUED_A : 0u) | (vj == K ? AIM_PAIR_RESCUED_B : 0u);
                hi.z = v.span_lo;
                hi.w = v.span_hi;
            } else if (both) {
                lo.z = (uint32_t)unpaired;
                lo.w = (uint32_t)(v.cnt ? v.cost : INT_MAX);
            }
            uint4 *out = reinterpret_cast<uint4 *>(a.pairs + m);
            out[0] = lo;
            out[1] = hi;
        }
        // apply: the rescue row of the winning combination becomes slot 0 of its read, the read's other slots lose AIM_SEG_VALID
        if (take && live && (vi == K || vj == K)) {
            const bool b_side = vj == K;
            const uint32_t r = b_side ? rb : ra;
            const uint64_t slot = (uint64_t)r * K + cand;
            if (cand == 0) {
                const uint4 *row = reinterpret_cast<const uint4 *>(a.res_sam) + (uint64_t)r * 3u;
                const uint4 w0 = row[0], w1 = row[1], w2 = row[2];
                uint4 *dst = reinterpret_cast<uint4 *>(a.sam) + slot * 3u;
                dst[0] = w0;
                dst[1] = make_uint4(w1.x, w1.y, w1.z + a.cigar_base, w1.w);    // cigar_offset
                dst[2] = make_uint4(w2.x + a.md_base, w2.y, w2.z, w2.w);       // md_offset
                const uint32_t L = pair_read_len(a, true, r);
                reinterpret_cast<uint2 *>(a.seg)[slot] = make_uint2(L << 16, L | (AIM_SEG_VALID | AIM_SEG_LEFT_OPEN | AIM_SEG_RIGHT_OPEN) << 16);
                const uint64_t anchor_slot = b_side ? ra * K + rep_a : rb * K + rep_b;
                if (a.contig) a.contig[slot] = b_side ? contig_a : contig_b;
                uint32_t *c1 = reinterpret_cast<uint32_t *>(a.cls) + slot * 2u + 1u;
                *c1 = (*c1 & ~0x00ff0000u) | (reinterpret_cast<const uint32_t *>(a.cls)[anchor_slot * 2u + 1u] & 0x00ff0000u);   // the mapq byte
            } else {
                uint32_t *s1 = reinterpret_cast<uint32_t *>(a.seg) + slot * 2u + 1u;
                *s1 &= ~(AIM_SEG_VALID << 16);
            }
        }
    }
