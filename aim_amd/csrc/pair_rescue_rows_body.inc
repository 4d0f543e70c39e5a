// pair_rescue_rows_body.inc -- the body of pair_rescue_rows_kernel and of pair_rescue_rows_est_kernel (pair.hpp includes it inside either
// kernel): `a` is the kernel's PairArgs, G its lanes per read pair. The two kernels differ in where a.min_span and a.max_span come from alone.
// One text, compiled twice: the first kernel's instructions are what they were when the body stood in it.
    const uint32_t kPairs = kPairThreads / G;
    const uint32_t cand = threadIdx.x & (G - 1u);
    const uint32_t base = (threadIdx.x & (uint32_t)(kWave - 1)) & ~(G - 1u);
    const uint32_t gm = (1u << G) - 1u;
    const uint32_t n_mates = a.n_reads / 2u, n_blocks = (n_mates + kPairs - 1u) / kPairs;   // (slots, reads and pairs are 32-bit: n_reads * (K + 1) < 2^32)
    for (uint32_t blk = blockIdx.x; blk < n_blocks; blk += gridDim.x) {
        const uint32_t m = blk * kPairs + threadIdx.x / G;
        const bool pair_live = m < n_mates, live = pair_live && cand < a.K;
        const PairCand A = pair_load_slot(a, live, 2u * m * a.K + cand), B = pair_load_slot(a, live, (2u * m + 1u) * a.K + cand);
        const uint32_t mask_a = (uint32_t)(__ballot(A.fl & 1u) >> base) & gm, mask_b = (uint32_t)(__ballot(B.fl & 1u) >> base) & gm;
        const bool none_proper = !((uint32_t)(__ballot(pair_mapped_row(a, A, B, cand, G).cnt != 0u) >> base) & gm);
        // (`side ? A : B` selects a six-register candidate. The compiler unrolls these two rounds, so each is a plain use of A or of B and
        // the kernel stays at 36 VGPRs; nothing in the language promises that. tests/test_pairs_cpu.py holds the code object to kPairMaxVgpr
        // and to no scratch: if a compiler keeps the loop and the count moves, write the two rounds out.)
        for (uint32_t side = 0; side < 2u; ++side) {                        // side: the read b of the row; its mate is the anchor's read
            const uint32_t b = 2u * m + side;
            const uint32_t mask = side ? mask_a : mask_b;                    // the mate's mapped slots
            const PairCand anchor = pair_bcast(side ? A : B, mask ? (uint32_t)__ffs(mask) - 1u : 0u, G);
            const uint32_t L = pair_read_len(a, pair_live, b);
            int64_t lo = 0, hi = 0;
            if ((a.options & AIM_PAIR_RESCUE) && mask && none_proper && L) {   // the rescue is tried
                int64_t c_lo = 0, c_hi = a.ref_len;
                if (a.contig && anchor.contig < a.n_contigs) {               // (no load outside the table)
                    c_lo = a.contig_start[anchor.contig];
                    c_hi = c_lo + a.contig_len[anchor.contig];
                }
                const int64_t P = (int64_t)((uint64_t)anchor.pos_hi << 32 | anchor.pos_lo);
                if (anchor.fl & 2u) {
                    const int64_t E = P + anchor.span;
                    lo = max(E - a.max_span, c_lo);
                    hi = min(E - a.min_span + L, c_hi);
                } else {
                    lo = max(P + a.min_span - L, c_lo);
                    hi = min(P + a.max_span, c_hi);
                }
            }
            const bool row = hi - lo >= (int64_t)L && L;                     // else the empty row: lengths 0, text_pos 0
            if (pair_live && cand == 0) {
                const uint64_t tp = row ? ((uint64_t)lo | ((anchor.fl & 2u) ? 0ull : AIM_REF_MINUS_STRAND)) : 0ull;
                reinterpret_cast<uint4 *>(a.res_req)[b] = make_uint4(row ? L : 0u, row ? (uint32_t)(hi - lo) : 0u, 0u, b);
                reinterpret_cast<uint2 *>(a.res_text_pos)[b] = make_uint2((uint32_t)tp, (uint32_t)(tp >> 32));
            }
            if (row) {                                                       // the read as given, at the stride of the rescue alignment
                const uint2 *src = reinterpret_cast<const uint2 *>(a.reads + (uint64_t)b * a.read_size);
                uint2 *dst = reinterpret_cast<uint2 *>(a.res_patterns + (uint64_t)b * a.rescue_size);
                for (uint32_t w = cand; w < a.read_size / 8u; w += G) dst[w] = src[w];
            }
        }
    }
