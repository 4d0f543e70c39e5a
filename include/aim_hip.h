/*
 * aim_hip.h -- C-ABI of the MI355X alignment engine (libaim_hip.so).
 *
 * This is the drop-in boundary for AIM's per-pair alignment path.  The
 * reference host program (safaad/aim, e.g. WFA/DPU-WRAM/host/host.c) talks to
 * the UPMEM SDK through nine calls and a byte-layout ABI in MRAM; every entry
 * point below names the reference call site it replaces.  Plain C: pointers,
 * sizes, POD structs; no C++ or torch types cross this boundary.
 *
 * All functions return AIM_OK (0) or a negative AIM_E* code; aim_last_error()
 * returns a thread-local human readable message for the last failure.
 * There is no CPU fallback: without a usable HIP device every compute entry
 * point fails with AIM_ENODEV.
 */
#ifndef AIM_HIP_H
#define AIM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AIM_ABI_VERSION 2

/* ---- error codes ------------------------------------------------------- */
#define AIM_OK 0
#define AIM_EINVAL (-1)  /* bad argument / unsupported configuration          */
#define AIM_ENODEV (-2)  /* no HIP device / HIP runtime failure                */
#define AIM_ENOMEM (-3)  /* host or device allocation failed                  */
#define AIM_ESTATE (-4)  /* call sequence violated (e.g. launch before push)  */
#define AIM_EALIGN (-5)  /* at least one pair hit a reference abort condition;
                            see aim_result_t.status                           */

/* ---- algorithm selection (one per reference sub-project) ---------------- */
#define AIM_ALGO_NW 0  /* NW/DPU-{WRAM,MRAM}   nw_compute      nw.c:109-153   */
#define AIM_ALGO_SWG 1 /* SWG/DPU-{WRAM,MRAM}  swg_compute     swg.c:121-171  */
#define AIM_ALGO_WFA 2 /* WFA/DPU-{WRAM,MRAM}  affine_wfa_compute wfa.c:342-379 */
#define AIM_ALGO_GENASM 3 /* aim-genasm (BASELINE config 5): bit-vector edit distance + windowed traceback for long reads.
                             PARITY UNPINNED: the reference tree holds only an un-pinned, empty submodule
                             (.gitmodules:1-3); this implements the published GenASM algorithm (MICRO 2020) as restated
                             in oracle/genasm_oracle.c.  score = edit distance of the reported alignment; penalties and
                             max_score are ignored; ops are written forward (begin_offset = 0). */

/* ---- flags: the reference's compile-time -D switches, now run time ------ */
#define AIM_FLAG_BACKTRACE 0x1u /* -DBACKTRACE (run-*-pim-*.py -b)            */
#define AIM_FLAG_REDUCE 0x2u    /* -DREDUCE = WFA-adaptive (run-wfa-*.py -r)  */
#define AIM_FLAG_SWG_W16 0x4u   /* force int16 SWG cells (= SWG/DPU-MRAM,
                                   SWG/DPU-MRAM/common/common.h:91); default is
                                   the WRAM rule: int8 iff MAX_SCORE < 127
                                   (SWG/DPU-WRAM/common/common.h:71-75)       */

/* Opt-in compact I/O layouts (round 2; the 16-B / 24-B structs below stay the default ABI):
 *  AIM_FLAG_REQ8  requests[] are aim_request8_t = the reference's own WFA request_t, 8 B
 *                 (WFA/DPU-WRAM/common/common.h:172-177: int16 pattern_len, int16 text_len, uint32 idx);
 *  AIM_FLAG_RES8  results[] are aim_result8_t {idx, score}, 8 B -- exactly what the reference host prints in
 *                 score-only mode (host.c:339-341).  Not valid with AIM_FLAG_BACKTRACE (the CIGAR needs the offsets).
 *                 There is no status field: without BACKTRACE the only per-pair failure that exists is AIM_PAIR_NOMEM, which
 *                 the launch plans rule out (a score-only launch is refused with AIM_ENOMEM rather than given a window that
 *                 could overflow); should a kernel ever report one all the same, its score reads AIM_SCORE_FAILED.
 * Both apply to every entry point that takes requests / results (aim_set_push / aim_set_pull / aim_align_device). */
#define AIM_FLAG_REQ8 0x8u
#define AIM_FLAG_RES8 0x10u
#define AIM_SCORE_FAILED ((int32_t)0x80000000) /* aim_result8_t.score of a pair that stopped with a status (see above) */


/* Replaces the -D macro set the launchers pass to make
 * (WFA/DPU-WRAM/run-wfa-pim-wram.py:128-131; common.h:63-89). */
typedef struct aim_params {
    int32_t algo;      /* AIM_ALGO_*                                          */
    int32_t match;     /* MATCH     (SWG only; NW/WFA ignore it like the ref) */
    int32_t mismatch;  /* MISMATCH                                            */
    int32_t gap_o;     /* GAP_O     (SWG, WFA)                                */
    int32_t gap_e;     /* GAP_E     (SWG, WFA)                                */
    int32_t gap_i;     /* GAP_I     (NW)                                      */
    int32_t gap_d;     /* GAP_D     (NW)                                      */
    int32_t max_score; /* MAX_SCORE (WFA: score cap; SWG: "+infinity" value)  */
    int32_t read_size; /* READ_SIZE: row stride of patterns/texts, multiple of 8 */
    uint32_t flags;    /* AIM_FLAG_*                                          */
} aim_params_t;

/* WFA scores and the reference's -10.  The reference's recurrence (the reference's dpu/wfa.c, affine_wfa_compute_offsets) starts a cell
 * that no present source wavefront covers at -10, not at NULL, and every WFA kernel here copies that rule byte for byte.  On a
 * penalty set with gap_o + gap_e > 11 * mismatch or gap_e > mismatch such a cell can become a real offset before the gap that
 * leads to it is paid for ((10 + k) * mismatch < gap_o + k * gap_e for a gap of k bases), and global WFA then returns the
 * reference's score, which can lie below the minimum cost and below the cost of the CIGAR printed next to it (the CIGAR stays a
 * valid alignment of the two sequences).  On every other penalty set the score is the minimum cost.  AIM_FLAG_ENDSFREE,
 * AIM_FLAG_AFFINE2P and AIM_FLAG_WFA_BIDIR promise a minimum cost and are refused (AIM_EINVAL) on those penalty sets, whatever
 * read_size is (for AIM_FLAG_AFFINE2P the rule reads piece 1); AIM_FLAG_LINEAR has no such start value to inherit and is not. */
/* AIM_FLAG_ENDSFREE (WFA only, not with AIM_FLAG_REDUCE): ends-free (semi-global) alignment.  The params are then the
 * `base` of an aim_endsfree_params_t and every entry point taking `const aim_params_t *` also reads its four free lengths
 * (it never reads past `base` without the flag).  Leading / trailing gaps inside the free lengths cost 0: the alignment
 * starts at any (v = 0, h <= text_begin_free) or (v <= pattern_begin_free, h = 0) and ends at any (v = plen,
 * h >= tlen - text_end_free) or (v >= plen - pattern_end_free, h = tlen); every other cost is WFA's.  Each free length is
 * clamped per pair to that pair's length.  The CIGAR still covers both whole sequences: free runs print as 'I' (a text
 * base) / 'D' (a pattern base).  A pair whose score exceeds max_score reports max_score + 1, status AIM_PAIR_OK and an
 * empty CIGAR (begin_offset == end_offset; n_runs == 0).  With all four lengths 0 the results are global WFA's (but for
 * that empty CIGAR of a pair over max_score, where global WFA reports a range of one byte).  Needs gap_o + gap_e <= 11 * mismatch
 * and gap_e <= mismatch (above).
 * Check aim_features() & AIM_FEATURE_ENDSFREE first: older libraries ignore unknown flags. */
#define AIM_FLAG_ENDSFREE 0x20u
typedef struct aim_endsfree_params {
    aim_params_t base;
    int32_t pattern_begin_free, pattern_end_free, text_begin_free, text_end_free;   /* each >= 0 */
} aim_endsfree_params_t;

/* AIM_FLAG_AFFINE2P (WFA only; not with AIM_FLAG_REDUCE or AIM_FLAG_ENDSFREE): dual-cost (two-piece) gap-affine penalties.
 * The params are then the `base` of an aim_affine2p_params_t and every entry point taking `const aim_params_t *` also reads
 * gap_o2 / gap_e2 (it never reads past `base` without the flag).  A maximal run of L insertions or of L deletions costs
 * min(gap_o + L*gap_e, gap_o2 + L*gap_e2): base.gap_o / base.gap_e are piece 1; match costs 0, mismatch costs `mismatch`.
 * The score is the minimum cost of a global alignment; MAX_SCORE, the over-cap result and the ops-row contract are global
 * WFA's.  A dual-affine cost never exceeds the piece-1 cost of the same alignment, so a max_score sized for piece 1 is
 * never too small.  With (gap_o2, gap_e2) == (gap_o, gap_e), or gap_o2 + gap_e2 > max_score, the results (CIGAR bytes
 * included) are global WFA's.  Needs gap_o + gap_e <= 11 * mismatch and gap_e <= mismatch (above).
 * Check aim_features() & AIM_FEATURE_AFFINE2P first: older libraries ignore unknown flags. */
#define AIM_FLAG_AFFINE2P 0x40u
typedef struct aim_affine2p_params {
    aim_params_t base;
    int32_t gap_o2, gap_e2;   /* piece 2: each > 0 */
} aim_affine2p_params_t;

/* AIM_FLAG_LINEAR (WFA only; not with AIM_FLAG_REDUCE, AIM_FLAG_ENDSFREE or AIM_FLAG_AFFINE2P): gap-linear penalties, read
 * from aim_params_t itself (no extension struct).  A match costs 0, a mismatch `mismatch` (x > 0) and every inserted or deleted
 * base `gap_e` (g > 0); gap_o must be 0 and match <= 0.  The score is the minimum cost of a global alignment; x = g = 1 is the
 * edit distance.  MAX_SCORE, the over-cap result and the ops-row contract are global WFA's.  Without this flag gap_o = 0 is
 * rejected as before.  Check aim_features() & AIM_FEATURE_LINEAR first: older libraries ignore unknown flags. */
#define AIM_FLAG_LINEAR 0x80u

/* AIM_FLAG_WFA_W32 (WFA only): 32-bit wavefront offsets, the reference's WFA built with -DAFFINE_WAVEFRONT_W32 (offsets int32,
 * NULL = INT32_MIN / 2) instead of its default AFFINE_WAVEFRONT_W16.  It lifts WFA's read_size < 32760 bound to read_size <= 2^24
 * (GenASM's); AIM_FLAG_REQ8 still carries int16 lengths and keeps read_size < 32760.  It combines with AIM_FLAG_REDUCE,
 * AIM_FLAG_ENDSFREE, AIM_FLAG_AFFINE2P, AIM_FLAG_LINEAR, AIM_FLAG_BACKTRACE and AIM_FLAG_RES8 under their own rules.  MAX_SCORE,
 * the over-cap result, the ops-row contract, the statuses and the CIGAR bytes are unchanged.  Every batch runs on the general
 * one-pair-per-wavefront kernel: below read_size 32760 the results equal those without the flag and the flag only costs speed.
 * Check aim_features() & AIM_FEATURE_WFA_W32 first: older libraries ignore unknown flags. */
#define AIM_FLAG_WFA_W32 0x100u
/* AIM_FLAG_WFA_BIDIR (global gap-affine WFA with AIM_FLAG_BACKTRACE only): bidirectional WFA (Marco-Sola et al., Bioinformatics
 * 2023), CIGAR in O(MAX_SCORE) scratch per workgroup instead of the O(MAX_SCORE^2) history, so no pair reports AIM_PAIR_NOMEM
 * because of its score. Score and status are exactly the flag-less ones (MAX_SCORE + 1 over the cap, with the over-cap row
 * begin_offset = end_offset - 1). The CIGAR is an optimal global alignment of the same cost in the same ops-row layout; it
 * equals the flag-less bytes for every pair whose score is <= T, the base-case threshold the plan line prints as "bidir=T"
 * (T >= 250). Results do not depend on the offset width, the grid, the slots or the batch size. Combines with
 * AIM_FLAG_WFA_W32, AIM_FLAG_REQ8, packed input, compact runs and every entry point; rejected (AIM_EINVAL) with NW / SWG / GenASM,
 * without AIM_FLAG_BACKTRACE, with AIM_FLAG_REDUCE, AIM_FLAG_ENDSFREE, AIM_FLAG_AFFINE2P or AIM_FLAG_LINEAR (follow-ups), and on a
 * penalty set with gap_o + gap_e > 11 * mismatch or gap_e > mismatch (above: its second stage has no -10).  Caveat: the flag is
 * accepted up to max(mismatch, gap_o + gap_e) = 61, but it is verified on a GPU only up to 5; the one run at 61 ((61,50,11),
 * read_size 1024, max_score 610) ended in an illegal memory access whose cause is not found yet ("Penalty sets").
 * Check aim_features() & AIM_FEATURE_WFA_BIDIR first: older libraries ignore unknown flags. */
#define AIM_FLAG_WFA_BIDIR 0x200u
/* AIM_FLAG_REF_TEXTS (every algorithm, combines with every other flag): the texts of a batch are windows of a reference sequence
 * that lives on each device of the set (aim_set_reference), named per pair by a uint64_t text_pos instead of being carried as rows.
 * Bits 0..62 of text_pos hold the window's start, bit 63 its strand: strand 0 is ref[pos, pos + text_len), strand 1 the reverse
 * complement of that window (A<->T, C<->G, a<->t, c<->g; every other byte unchanged). text_len <= read_size as always; the
 * request arrays are unchanged. The device gathers the windows into the char[n][READ_SIZE] text rows (zero past text_len) before
 * any alignment kernel runs: results, statuses, ops rows and compact CIGARs equal those of the same batch sent with explicit texts.
 * Entry points: aim_set_push_ref (aim_set_push is refused with the flag), aim_set_submit with an aim_batch_io_ref_t (texts,
 * packed_texts and raw_texts NULL; a packed pair is raw only when its PATTERN holds a byte outside A/C/G/T) and
 * aim_align_device_ref. aim_set_push_ref / aim_set_submit check every window with aim_ref_windows_check before anything is
 * enqueued. Check aim_features() & AIM_FEATURE_REF_TEXTS first: older libraries ignore unknown flags. */
#define AIM_FLAG_REF_TEXTS 0x400u
#define AIM_REF_MINUS_STRAND (1ull << 63) /* text_pos bit 63: the reverse complement of the window */
/* AIM_FLAG_READ_GROUPS (every algorithm, combines with every other flag under that flag's own rules): the verification stage of a
 * read mapper. A batch holds n_reads reads and n_pairs candidates; read_offsets[n_reads + 1] (CSR, read_offsets[0] = 0,
 * read_offsets[n_reads] = n_pairs, every read >= 1 candidate) gives read r the candidates [read_offsets[r], read_offsets[r+1]).
 * Requests and texts (or text_pos) stay one per candidate; patterns are one row per READ, and candidate i's pattern is the first
 * pattern_len[i] bytes of its read's row. The device aligns every candidate score-only (the configured flags minus BACKTRACE,
 * WFA_BIDIR and RES8), picks per read the AIM_PAIR_OK candidate of lowest score (lowest batch index on a tie; a WFA pair over the cap
 * counts with its MAX_SCORE + 1) into an aim_best_t, and runs the configured plan again on the winners only. Read r's result row,
 * ops row [begin_offset, end_offset), compact header and runs are exactly those of candidate sel[r] -- best_pair, or
 * read_offsets[r] when the read has no OK candidate -- run without this flag under the configured flags (its idx and status
 * included). Entry points: aim_set_submit with an aim_batch_io_groups_t (ASCII read rows, or with AIM_FLAG_REF_TEXTS packed read rows
 * whose raw_pairs list READ indices and raw_patterns their rows; packed explicit texts are refused) and aim_align_device_groups (ASCII); aim_set_push, aim_set_push_ref, aim_set_launch, aim_set_pull, aim_align_device and aim_align_device_ref
 * refuse the flag. Check aim_features() & AIM_FEATURE_READ_GROUPS first: older libraries ignore unknown flags. */
#define AIM_FLAG_READ_GROUPS 0x800u
/* AIM_FLAG_WFA_ESCALATE (global gap-affine WFA): a generous MAX_SCORE without losing the one-pair-per-lane kernels. The batch runs at
 * a low cap c on a lane kernel -- c is the largest cap below MAX_SCORE whose flag-less plan is wfa_lane_kernel or wfa_lane_packed_kernel
 * (5 or 10 today, by penalties, BACKTRACE, READ_SIZE and packed input) -- and only the pairs that come back over c are run again under
 * the flag-less plan at MAX_SCORE, from a device-side list, on the same stream. EVERY per-pair output is exactly that of the same
 * call without the flag: the result row, status and ops[begin_offset, end_offset); the {idx, score} row; the compact header's idx, score,
 * n_runs and status and the pair's runs (run_offset may differ, the batch's run total does not). Results do not depend on the grid, the
 * slots, the batch size or the AIM_DEBUG_POISON_* knobs. The plan line ends in " escalate=c": with c > 0 it is
 * "<stage 1 line> | <stage 2 line> escalate=c"; where no lane kernel takes the shape, or the flag-less plan is a lane plan already, it
 * is the flag-less line and " escalate=0". Combines with AIM_FLAG_REDUCE, AIM_FLAG_BACKTRACE, AIM_FLAG_REQ8, AIM_FLAG_RES8, packed
 * input, compact runs and AIM_FLAG_REF_TEXTS on every entry point that takes them (aim_kernel_name names the first stage). Rejected
 * (AIM_EINVAL) with NW / SWG / GenASM, with AIM_FLAG_ENDSFREE, AIM_FLAG_AFFINE2P, AIM_FLAG_LINEAR, AIM_FLAG_WFA_W32 or
 * AIM_FLAG_WFA_BIDIR (no lane kernel takes them) and with AIM_FLAG_READ_GROUPS (a follow-up).
 * Check aim_features() & AIM_FEATURE_WFA_ESCALATE first: older libraries ignore unknown flags. */
#define AIM_FLAG_WFA_ESCALATE 0x1000u
/* AIM_FLAG_MATE_PAIRS (needs AIM_FLAG_READ_GROUPS and AIM_FLAG_REF_TEXTS; combines with whatever AIM_FLAG_READ_GROUPS combines with,
 * under those flags' own rules): paired-end candidate selection on the device. Reads 2m and 2m + 1 of a batch are mates (n_reads must
 * be even). After the score-only pass and the independent selection of AIM_FLAG_READ_GROUPS, the device picks for every read pair the
 * best consistent pair of candidates and falls back to the independent winners only when no consistent pair is good enough.
 * THE SELECTION RULE (deterministic; it does not depend on the grid):
 *   Candidate windows. Candidate c has a window [start_c, end_c) with start_c = text_pos[c] & ~AIM_REF_MINUS_STRAND and
 *   end_c = start_c + text_len[c]. It has a strand bit, a score and a status from the score-only pass. A WFA pair over the cap counts
 *   with MAX_SCORE + 1, as under AIM_FLAG_READ_GROUPS.
 *   Proper combination. A combination (i, j) takes candidate i of read 2m and candidate j of read 2m+1. It is proper when all of the
 *   following hold: both candidates are AIM_PAIR_OK; their strands differ; start_f <= start_r, with f the strand-0 candidate and r the
 *   strand-1 candidate; min_span <= end_r - start_f <= max_span.
 *   The spans are window coordinates. They are not refined by the CIGAR: a caller widens the bounds by the flanks of its windows.
 *   Costs. A proper combination costs score_i + score_j. The unpaired choice costs best_a + best_b + unpaired_penalty, where best_a
 *   and best_b are the independent AIM_FLAG_READ_GROUPS winners' scores. The unpaired choice exists only when both reads have an OK
 *   candidate. Sums are formed in 64 bits and clamped to INT32_MAX - 1.
 *   Choice. The proper combination of lowest cost wins, with ties broken by lowest i and then lowest j. It is taken if its cost is
 *   at most the unpaired cost, so a tie goes to proper. Otherwise the independent winners are taken and flags = 0. If one mate has no
 *   OK candidate, the other keeps its independent winner and score_sum = INT32_MAX.
 *   Outputs. sel[2m] and sel[2m+1] are the chosen candidates, or read_offsets[r] when a read has none. Everything downstream is
 *   AIM_FLAG_READ_GROUPS' contract unchanged: read r's result row, its ops row [begin_offset, end_offset), its compact header and its
 *   runs are those of candidate sel[r] run without these flags. groups.best still reports each read's INDEPENDENT selection.
 * The selection enumerates a read pair's combinations: its cost is O(K1 * K2) for reads of K1 and K2 candidates.
 * Entry points: aim_set_submit with an aim_batch_io_mates_t and aim_align_device_mates; every entry point that refuses
 * AIM_FLAG_READ_GROUPS refuses this flag too, and so does aim_align_device_groups. Without AIM_FLAG_READ_GROUPS or AIM_FLAG_REF_TEXTS
 * the flag is AIM_EINVAL, the message naming the missing flag.
 * Check aim_features() & AIM_FEATURE_MATE_PAIRS first: older libraries ignore unknown flags. */
#define AIM_FLAG_MATE_PAIRS 0x2000u
/* AIM_FLAG_SAM_FIELDS (needs AIM_FLAG_REF_TEXTS and AIM_FLAG_BACKTRACE; not with AIM_ALGO_GENASM or AIM_FLAG_RES8): the device turns every
 * final ops row into a SAM-ready record -- an aim_sam_t plus BAM CIGAR words and MD bytes -- in one pass over the rows and the resident
 * reference (aim_set_submit with an aim_batch_io_sam_t; aim_sam_device is the same kernel without the flag, on rows already on a device).
 * THE CONVENTIONS:
 *   Ops mapping. AIM ops are 'M' (match), 'X' (mismatch), 'I' (consumes a text base) and 'D' (consumes a pattern base). The text is the
 *   reference: AIM 'I' is SAM 'D' and AIM 'D' is SAM 'I'.
 *   Orientation. Records are on the forward strand of the reference. A strand-0 window's ops are taken in row order, a strand-1 window's
 *   (text_pos bit 63) in reverse order. Reference bases are read from the forward reference at their forward position: no complement, and
 *   the read's bases are never needed ('M' / 'X' already say match / mismatch).
 *   Terminal runs. At each end of ops[begin_offset, end_offset) every op that is not 'M' or 'X' is peeled (terminal 'I' and 'D' runs may
 *   alternate). Peeled 'D' bases (read only) become ONE soft clip at that end; peeled 'I' bases (reference only) are dropped and move the
 *   position. The rule is the same with and without AIM_FLAG_ENDSFREE: a record neither starts nor ends with SAM I or D.
 *   Fields. pos is the 0-based forward position of the first reference base the remaining ops consume: the window start plus the
 *   reference bases dropped at the row's beginning (strand 0) or at the row's END (strand 1). ref_span counts the reference bases the
 *   remaining ops consume, nm their 'X' bases plus their inner 'I' and 'D' bases.
 *   CIGAR. BAM words (len << 4) | op with M 0, I 1, D 2, S 4, = 7, X 8; adjacent equal ops are merged. 'M' and 'X' both give M unless
 *   AIM_SAM_EQX is set in sam_options (then = and X).
 *   MD. samtools' rule: a decimal match count (possibly 0) before every mismatch and before every deletion; a mismatch writes the
 *   reference byte verbatim, a deletion '^' plus its reference bytes; a final count ends the string; read insertions and clips neither
 *   appear nor reset the count. No terminating NUL.
 *   Unmapped rows. A row whose status is not AIM_PAIR_OK, whose ops range is empty, which is a WFA row over the cap (score
 *   MAX_SCORE + 1), of which nothing remains after peeling, or whose candidate is UINT32_MAX gets flags = AIM_SAM_UNMAPPED, n_cigar = 0,
 *   md_len = 0, ref_span = 0, nm = 0 and pos = the window start (0 without a candidate).
 *   Capacity. A row whose words or bytes do not fit gets AIM_SAM_OVERFLOW in status, n_cigar = md_len = 0 and every other field
 *   intact; nothing of it is written. Placement in the two buffers depends on scheduling: each record carries its own offsets, and the
 *   content they address and every other field do not depend on the grid or on the AIM_DEBUG_POISON_* knobs.
 * Every other output of the call (result rows, ops ranges, compact headers and runs, best, mates) equals that of the same call without the
 * flag. Combines with AIM_FLAG_READ_GROUPS / AIM_FLAG_MATE_PAIRS (rows are reads, record r follows sel[r]) and with ENDSFREE, AFFINE2P,
 * LINEAR, WFA_W32, WFA_BIDIR, REDUCE, WFA_ESCALATE, REQ8, packed read rows and compact runs. Under the flag the ops rows stay on the
 * device, so a plan that would fuse the run output is not used; the plan line gains " sam=1". aim_set_push_ref, aim_set_launch and
 * aim_set_pull refuse the flag (the records need the submit struct), and so do aim_align_device, aim_align_device_ref,
 * aim_align_device_groups and aim_align_device_mates (AIM_EINVAL: run them without the flag, then aim_sam_device over their rows).
 * aim_plan_describe, aim_scratch_bytes and aim_kernel_name accept it and describe the plan aim_set_submit follows.
 * Check aim_features() & AIM_FEATURE_SAM_FIELDS first: older libraries ignore unknown flags. */
#define AIM_FLAG_SAM_FIELDS 0x4000u
/* AIM_FLAG_TOP_HITS (needs AIM_FLAG_READ_GROUPS; combines with whatever that flag combines with, under those flags' own rules): the
 * max_hits best candidates of every read, each a full row -- secondary alignments, repeats, a mate-rescue list -- without sending the
 * runners-up again as a second batch. Rows are hits, not reads, and their number is fixed by the batch's shape, so the host knows every
 * size before it submits: nothing is compacted, scanned or counted on the device.
 * RANKING. For read r with K_r candidates, after the score-only pass of AIM_FLAG_READ_GROUPS: the AIM_PAIR_OK candidates come first,
 *   ordered by (score, batch index) ascending (a WFA pair over the cap counts with its MAX_SCORE + 1, as under AIM_FLAG_READ_GROUPS); the
 *   candidates that are not OK follow, ordered by batch index. Rank 0 is therefore always sel[r] of AIM_FLAG_READ_GROUPS.
 * ROWS. Read r gets exactly min(K_r, max_hits) hit rows, at [hit_offsets[r], hit_offsets[r + 1]) in rank order; hit_offsets is the
 *   exclusive prefix sum of those counts (aim_hits_offsets) and H = hit_offsets[n_reads] <= n_pairs. hit_pair[h] is the candidate of
 *   row h. Row h's result row (its idx and status included), ops range [begin_offset, end_offset), compact header and runs are exactly
 *   those of candidate hit_pair[h] run without AIM_FLAG_READ_GROUPS and AIM_FLAG_TOP_HITS under the configured flags: the contract of
 *   AIM_FLAG_READ_GROUPS applied per hit. Without AIM_FLAG_BACKTRACE there is no second pass and the rows are the score-only rows
 *   (aim_result_t, or {idx, score} under AIM_FLAG_RES8). best[] is unchanged, and with max_hits = 1 every output equals that of the same
 *   call without the flag. Nothing depends on the grid, the slots, the batch split or the AIM_DEBUG_POISON_* knobs.
 * Entry points: aim_set_submit with an aim_batch_io_hits_t and aim_align_device_hits; every entry point that refuses
 * AIM_FLAG_READ_GROUPS refuses this flag too, and so does aim_align_device_groups. The plan line ends in " groups=1 hits=1".
 * AIM_EINVAL, the message naming the flag: without AIM_FLAG_READ_GROUPS, and with AIM_FLAG_MATE_PAIRS or AIM_FLAG_SAM_FIELDS (follow-ups;
 * aim_sam_device already works on hit rows: pass d_sel = d_hit_pair and n_rows = H).
 * Check aim_features() & AIM_FEATURE_TOP_HITS first: older libraries ignore unknown flags. */
#define AIM_FLAG_TOP_HITS 0x8000u
#define AIM_TOP_HITS_MAX 8          /* max_hits is 1..AIM_TOP_HITS_MAX */
#define AIM_SAM_EQX 0x1u            /* sam_options / options: '=' and 'X' instead of 'M' */
#define AIM_SAM_REVERSE 0x10u       /* aim_sam_t.flags: SAM's own FLAG bits */
#define AIM_SAM_UNMAPPED 0x4u
#define AIM_SAM_OVERFLOW 0x100u     /* aim_sam_t.status bit: the CIGAR or the MD buffer was too small for this row */
typedef struct aim_sam {            /* 48 B per row */
    uint32_t idx; int32_t score;    /* the row's */
    uint64_t pos;
    uint32_t ref_span, nm;
    uint32_t cigar_offset, n_cigar; /* words in the CIGAR buffer */
    uint32_t md_offset, md_len;     /* bytes in the MD buffer */
    uint16_t flags;                 /* AIM_SAM_REVERSE | AIM_SAM_UNMAPPED; from aim_sam_device_split also AIM_SAM_SUPPLEMENTARY */
    uint16_t status;                /* AIM_PAIR_* | AIM_SAM_OVERFLOW */
    uint32_t pad;                   /* 0 */
} aim_sam_t;

/* Per-pair descriptor: byte-compatible with the NW/SWG request_t
 * (NW/DPU-WRAM/common/common.h:114-120).  The WFA variant of the reference
 * uses int16 lengths (WFA/DPU-WRAM/common/common.h:172-177); a binding widens
 * them when filling this struct. */
typedef struct aim_request {
    int32_t pattern_len;
    int32_t text_len;
    int32_t padding;
    uint32_t idx; /* global pair index, echoed into the result */
} aim_request_t;

/* AIM_FLAG_REQ8: byte-compatible with the WFA request_t (WFA/DPU-WRAM/common/common.h:172-177). */
typedef struct aim_request8 {
    int16_t pattern_len;
    int16_t text_len;
    uint32_t idx;
} aim_request8_t;

/* Per-pair result: byte-compatible with the NW/SWG result_t
 * (NW/DPU-WRAM/common/common.h:122-130); the reference's unused `padding`
 * word carries the per-pair status. */
#define AIM_PAIR_OK 0
#define AIM_PAIR_WFA_NO_LINK 1 /* wfa_backtracing.c:321-325: ref prints + exit(1) */
#define AIM_PAIR_SWG_NO_OP 2   /* swg.c:99-104: ref prints + exit(1)             */
#define AIM_PAIR_NOMEM 3       /* dpu_allocator_wram.c:19-23: ref prints + exit(1) */
typedef struct aim_result {
    int32_t max_operations; /* plen + tlen                                    */
    int32_t begin_offset;   /* CIGAR ops live in ops[begin_offset,end_offset) */
    int32_t end_offset;
    int32_t score;
    int32_t status; /* AIM_PAIR_* */
    uint32_t idx;
} aim_result_t;

/* AIM_FLAG_RES8: the two numbers the reference prints per pair without BACKTRACE (host.c:339-341). */
typedef struct aim_result8 {
    uint32_t idx;
    int32_t score;
} aim_result8_t;

/* ---- library / device discovery ----------------------------------------- */
int aim_abi_version(void);
/* Capabilities added without an ABI version change: a binding tests a bit before it sets the matching flag. */
#define AIM_FEATURE_ENDSFREE 0x1u /* AIM_FLAG_ENDSFREE is honoured */
#define AIM_FEATURE_AFFINE2P 0x2u /* AIM_FLAG_AFFINE2P is honoured */
#define AIM_FEATURE_LINEAR 0x4u   /* AIM_FLAG_LINEAR is honoured */
#define AIM_FEATURE_WFA_W32 0x8u  /* AIM_FLAG_WFA_W32 is honoured */
#define AIM_FEATURE_WFA_BIDIR 0x10u /* AIM_FLAG_WFA_BIDIR is honoured */
#define AIM_FEATURE_REF_TEXTS 0x20u /* AIM_FLAG_REF_TEXTS is honoured */
#define AIM_FEATURE_READ_GROUPS 0x40u /* AIM_FLAG_READ_GROUPS is honoured */
#define AIM_FEATURE_WFA_ESCALATE 0x80u /* AIM_FLAG_WFA_ESCALATE is honoured */
#define AIM_FEATURE_MATE_PAIRS 0x100u /* AIM_FLAG_MATE_PAIRS is honoured */
#define AIM_FEATURE_SAM_FIELDS 0x200u /* AIM_FLAG_SAM_FIELDS is honoured; aim_sam_device and aim_sam_format_cigar exist */
#define AIM_FEATURE_TOP_HITS 0x400u /* AIM_FLAG_TOP_HITS is honoured; aim_hits_offsets and aim_align_device_hits exist */
#define AIM_FEATURE_SEED 0x800u /* device-side seeding: aim_index_sizes / aim_index_build / aim_seed_device / aim_seed_groups_offsets exist */
#define AIM_FEATURE_INDEX_DEVICE 0x1000u /* aim_index_device_scratch / aim_index_build_device / aim_index_kernel_names exist */
#define AIM_FEATURE_MINIMIZERS 0x2000u /* (w, k) minimizers: aim_index_build_minimizers / aim_index_build_device_minimizers / AIM_SEED_OPT_MINIMIZERS exist */
#define AIM_FEATURE_SEED_CHAIN 0x4000u /* colinear chaining of the seed hits: aim_seed_chain_device / aim_chain_t / aim_seed_chain_kernel_names exist */
#define AIM_FEATURE_SEED_CHAIN_LONG 0x8000u /* chaining for long reads: aim_seed_chain_long_device / aim_seed_chain_long_kernel_name exist */
#define AIM_FEATURE_CHAIN_CLASS 0x10000u /* primary / secondary chains and MAPQ: aim_chain_classify_device / aim_read_mapq_device / aim_chain_class_kernel_names exist */
#define AIM_FEATURE_SPLIT 0x20000u /* split reads: aim_split_segments_device / aim_sam_device_split / aim_split_kernel_names exist */
#define AIM_FEATURE_EXTEND 0x40000u /* segment extension: aim_extend_segments_device / aim_extend_kernel_names exist */
#define AIM_FEATURE_MAPPER 0x80000u /* rule 12c and the mapper object: aim_map_records_device / aim_mapper_create / aim_mapper_submit / aim_mapper_wait exist */
#define AIM_FEATURE_CONTIGS 0x100000u /* rule 13c, references of several sequences: aim_contigs_layout / aim_contig_clip_device / aim_map_records_contigs_device / aim_mapper_create_contigs exist */
#define AIM_FEATURE_PAIRED 0x200000u /* rule 14c, paired-end reads: aim_pair_rescue_rows_device / aim_pair_select_device / aim_map_mates_device / aim_mapper_set_pairing / aim_mapper_pairs exist */
#define AIM_FEATURE_PAIR_ESTIMATE 0x400000u /* rule 15c, the span bounds of rule 14c estimated from the batch: aim_pair_estimate_device / aim_pair_rescue_rows_device_est / aim_pair_select_device_est / aim_mapper_set_pairing_estimated / aim_mapper_pair_estimate exist */
uint32_t aim_features(void);
const char *aim_last_error(void);
/* Number of usable gfx950 devices (0 and AIM_ENODEV when there is none). */
int aim_device_count(int *count);

/* ---- device set: replaces struct dpu_set_t and the nine SDK calls -------- */
typedef struct aim_set aim_set_t;

/* dpu_alloc(NR_DPUS, NULL, &set) + dpu_load(set, DPU_BINARY, NULL)
 * (host.c:186-187).  device_ids may be NULL (= 0..nr_devices-1). */
int aim_set_alloc(uint32_t nr_devices, const int *device_ids, aim_set_t **set);
/* dpu_get_nr_dpus (host.c:188) */
int aim_set_nr_devices(const aim_set_t *set, uint32_t *nr_devices);
/* The compile-time configuration plus the MRAM plan of host.c:215-241
 * (mram_heap_alloc of params/requests/results/patterns/texts/operations):
 * sizes every device-side buffer for up to max_pairs_per_device pairs. */
int aim_set_configure(aim_set_t *set, const aim_params_t *params, uint32_t max_pairs_per_device);
/* The four host->device scatters of host.c:246-268 (DPUParams, requests,
 * patterns, texts) for ONE device of the set.  patterns/texts are
 * [n_pairs][read_size] byte rows.  Asynchronous when the host buffers come
 * from aim_host_alloc; the copy is ordered before the next launch. */
int aim_set_push(aim_set_t *set, uint32_t device, uint32_t n_pairs, const void *requests /* aim_request_t[] or, with
                 AIM_FLAG_REQ8, aim_request8_t[] */, const char *patterns, const char *texts);
/* dpu_launch(set, DPU_SYNCHRONOUS) (host.c:289): runs the alignment kernel on
 * every device of the set and waits for all of them. */
int aim_set_launch(aim_set_t *set);
/* The device->host gathers of host.c:316-326: results[n_pairs] and, with
 * AIM_FLAG_BACKTRACE, ops[n_pairs][2*read_size] (may be NULL otherwise).
 * CONTRACT OF AN OPS ROW: ops[i][begin_offset, end_offset) holds pair i's edit operations -- the bytes edit_cigar_print reads
 * (host.c:347-349). The REST of the row is unspecified: the reference's memset(operations, 'M', 2*READ_SIZE) (wfa.c:465,
 * swg.c:261) is only performed where an operation can be printed, so a caller that compares or copies whole rows sees
 * whatever its buffer held before (tests run with AIM_DEBUG_POISON_OPS to keep every kernel honest about that). */
int aim_set_pull(aim_set_t *set, uint32_t device, void *results /* aim_result_t[] or, with AIM_FLAG_RES8,
                 aim_result8_t[] */, char *ops);
/* The three phase timers host.c prints ("CPU-DPU", "DPU Kernel", "DPU-CPU",
 * host.c:270-272, 297-299, 328-330), in milliseconds, accumulated. Devices of a set work concurrently: each figure is the
 * SLOWEST device's (aim_set_launch: per launch; aim_set_submit / aim_set_wait: each device's batches summed, then the
 * maximum over devices). With several slots the phases of one device's batches overlap each other, so the three figures are
 * device-time per phase, not a partition of the wall time. */
int aim_set_timers(const aim_set_t *set, float *h2d_ms, float *kernel_ms, float *d2h_ms);
/* How many pairs of the last launch on `device` left the short-read fast path
 * (sequences with bytes other than A/C/G/T) and were aligned by the general
 * kernel instead.  Diagnostic only; 0 when the configuration has no fast path. */
int aim_set_fallback_pairs(aim_set_t *set, uint32_t device, uint32_t *n_fallback);
/* One line naming the plan the last launch on `device` followed (before the first launch: the configure-time plan):
 * kernel, lanes / wavefronts per pair, grid, block, LDS, scratch, scratch bound.  The AIM_* environment switches
 * (experiment / debugging knobs; none changes results) are read once per aim_set_configure and frozen in the set, so
 * this line cannot change between a configure and its launches. */
int aim_set_plan_describe(const aim_set_t *set, uint32_t device, char *out, size_t cap);
/* dpu_free (host.c:371); also releases the set's reference */
int aim_set_free(aim_set_t *set);

/* ---- device-resident reference (AIM_FLAG_REF_TEXTS) ------------------------------------------------------------------
 * Upload len bytes (taken verbatim: any byte value) to every device of the set; a second call replaces the reference. It does not
 * count against AIM_SCRATCH_GB. AIM_ENOMEM when it does not fit a device: the previous reference then stays. Batches in flight on
 * the set are completed before the old reference is released. */
int aim_set_reference(aim_set_t *set, const char *seq, uint64_t len);
/* aim_set_push of a batch whose texts are windows of the reference (needs AIM_FLAG_REF_TEXTS): text_pos[n_pairs] as above. */
int aim_set_push_ref(aim_set_t *set, uint32_t device, uint32_t n_pairs, const void *requests, const char *patterns,
                     const uint64_t *text_pos);
/* Host-side window check: AIM_OK when every pair's window [pos, pos + text_len) lies inside [0, ref_len) (bit 63 is the strand,
 * never part of the position; text_len 0 is always inside); else AIM_EINVAL naming the first bad pair, which *bad_pair (may be
 * NULL) receives. Lengths are checked against read_size like every entry point does. */
int aim_ref_windows_check(const aim_params_t *params, uint32_t n_pairs, const void *requests, const uint64_t *text_pos,
                          uint64_t ref_len, uint32_t *bad_pair);

/* ---- pipelined batches: packed input, compact CIGAR output, double buffering -----------------
 * The reference's host loop is strictly serial (host.c:246-330: scatter, launch, gather, print).  These entry points
 * keep its data (same pairs, same results) and overlap its phases: a set configured with aim_set_configure_slots owns
 * `slots` independent buffer sets and streams per device, aim_set_submit enqueues H2D + kernel(s) + D2H of one batch on a
 * slot and returns, aim_set_wait blocks until that slot's results are in the caller's buffers.  With two slots
 * pack(k+1) || H2D(k+1) || kernel(k) || D2H(k-1) || format(k-1).  aim_set_push / launch / pull keep working (slot 0).
 *
 * Packed input (opt-in): 2 bits per base, code = (ascii >> 1) & 3 (A 0, C 1, T 2, G 3); base i of a sequence sits at bits
 * [2*(i%16), 2*(i%16)+1] of dword i/16 of its row; a row is ceil(read_size/16) dwords.  The reference compares raw bytes
 * and accepts any character (host.c:126-127), so a pair with a byte outside A/C/G/T inside either sequence cannot be
 * packed: it is listed in raw_pairs[] (batch indices, ascending) and its two ASCII rows travel in raw_patterns /
 * raw_texts ([n_raw][read_size]); its packed rows are ignored.  The device expands the batch into the reference's own
 * char[n][READ_SIZE] layout before any alignment kernel runs, so results are bit-identical to the ASCII path.
 *
 * Compact CIGAR (opt-in, needs AIM_FLAG_BACKTRACE): instead of ops[n][2*read_size], the device run-length encodes
 * ops[begin_offset, end_offset) -- the loop of edit_cigar_print, host.c:69-89 -- and returns one aim_cigar_t per pair plus
 * a shared run buffer; run = (length << 8) | op character.  aim_cigar_format_runs prints it exactly like the reference. */
#define AIM_CIGAR_OVERFLOW 0x100u /* aim_cigar_t.status bit: the run buffer was too small for this pair's runs */
typedef struct aim_cigar {
    uint32_t idx;
    int32_t score;
    uint32_t run_offset; /* first run of this pair in the run buffer */
    uint16_t n_runs;     /* 0 when status != AIM_PAIR_OK */
    uint16_t status;     /* AIM_PAIR_* | AIM_CIGAR_OVERFLOW */
} aim_cigar_t;

typedef struct aim_batch_io {
    uint32_t n_pairs;
    const void *requests;            /* aim_request_t[n] or aim_request8_t[n] (AIM_FLAG_REQ8) */
    const char *patterns, *texts;    /* ASCII rows [n][read_size], or NULL when the batch is packed */
    const uint32_t *packed_patterns; /* packed rows [n][ceil(read_size/16)] dwords, or NULL */
    const uint32_t *packed_texts;
    uint32_t n_raw;                  /* packed batches: pairs that travel as raw rows */
    const uint32_t *raw_pairs;       /* [n_raw] batch indices */
    const char *raw_patterns, *raw_texts; /* [n_raw][read_size] */
    void *results;                   /* out: aim_result_t[n] / aim_result8_t[n]; may be NULL when cigars is given */
    char *ops;                       /* out: ops[n][2*read_size] (AIM_FLAG_BACKTRACE), or NULL */
    aim_cigar_t *cigars;             /* out: compact CIGAR headers [n], or NULL */
    uint32_t *runs;                  /* out: run buffer */
    uint32_t runs_cap;               /* capacity of runs[], in runs */
} aim_batch_io_t;

/* AIM_FLAG_REF_TEXTS: aim_set_submit reads past `base` (only with the flag). */
typedef struct aim_batch_io_ref {
    aim_batch_io_t base;             /* texts, packed_texts and raw_texts must be NULL */
    const uint64_t *text_pos;        /* [n_pairs] window start | strand << 63 */
} aim_batch_io_ref_t;

/* AIM_FLAG_READ_GROUPS: what each read's candidates scored in the score-only pass. second_score is the lowest score among the
 * read's OTHER OK candidates (= best_score on a tie; INT32_MAX with fewer than two OK candidates); n_best counts the OK candidates
 * of best_score. A read without an OK candidate: best_pair = UINT32_MAX, best_score = INT32_MAX, n_best = 0. */
typedef struct aim_best {
    uint32_t best_pair;              /* batch (candidate) index */
    int32_t best_score;
    int32_t second_score;
    uint32_t n_best;
} aim_best_t;

/* AIM_FLAG_READ_GROUPS: aim_set_submit reads past `base` (only with the flag). The first two members are laid out exactly like
 * aim_batch_io_ref_t. base.n_pairs, base.requests and the texts (or text_pos) are per candidate; base.patterns holds n_reads rows;
 * base.results, ops, cigars and runs receive one row per read. Packed input only with AIM_FLAG_REF_TEXTS: packed_patterns holds n_reads
 * rows and raw_pairs lists reads (AIM_EINVAL otherwise). */
typedef struct aim_batch_io_groups {
    aim_batch_io_t base;
    const uint64_t *text_pos;        /* AIM_FLAG_REF_TEXTS: [n_pairs]; else NULL */
    uint32_t n_reads;
    const uint32_t *read_offsets;    /* [n_reads + 1] */
    aim_best_t *best;                /* out: [n_reads], or NULL */
} aim_batch_io_groups_t;
/* Host-side CSR check: AIM_OK when read_offsets[0] == 0, the offsets never decrease, every read has a candidate and
 * read_offsets[n_reads] == n_pairs; else AIM_EINVAL naming the first bad read, which *bad_read (may be NULL) receives (a wrong
 * last offset names read n_reads - 1). n_reads 0 is valid only with n_pairs 0. aim_set_submit runs it before anything is enqueued. */
int aim_groups_check(uint32_t n_pairs, uint32_t n_reads, const uint32_t *read_offsets, uint32_t *bad_read);

/* AIM_FLAG_MATE_PAIRS: what the device chose for read pair m (reads 2m and 2m + 1); the rule is stated at the flag. */
#define AIM_MATE_PROPER 0x1u
typedef struct aim_mate {          /* 32 B, one per read pair m */
    uint32_t best_pair[2];         /* chosen candidate (batch index) of read 2m / 2m+1; UINT32_MAX: that read has no OK candidate */
    int32_t  score_sum;            /* cost of the choice; INT32_MAX when a mate has no OK candidate */
    int32_t  second_sum;           /* lowest cost among the OTHER proper combinations; INT32_MAX when there is none */
    uint32_t n_best;               /* proper combinations of cost score_sum (0 when the choice is not proper) */
    uint32_t flags;                /* AIM_MATE_PROPER */
    uint32_t pad[2];               /* 0 */
} aim_mate_t;

/* AIM_FLAG_MATE_PAIRS: aim_set_submit reads past `groups` (only with the flag). */
typedef struct aim_batch_io_mates {
    aim_batch_io_groups_t groups;  /* unchanged meaning; groups.best still reports each read's INDEPENDENT selection */
    int64_t  min_span, max_span;   /* 0 <= min_span <= max_span < 2^62 */
    int32_t  unpaired_penalty;     /* >= 0 */
    uint32_t pad;
    aim_mate_t *mates;             /* out: [n_reads / 2], or NULL */
} aim_batch_io_mates_t;
/* Host-side check of a mate-pairs batch: AIM_OK, or AIM_EINVAL with a message for an odd n_reads, a span outside
 * 0 <= min_span <= max_span < 2^62, or a negative penalty. aim_set_submit runs it after aim_groups_check, before anything is enqueued. */
int aim_mates_check(uint32_t n_reads, int64_t min_span, int64_t max_span, int32_t unpaired_penalty);

/* AIM_FLAG_SAM_FIELDS: aim_set_submit reads past `mates` (only with the flag; the groups and mates members are read only under their own
 * flags). base.results, ops and cigars may each be NULL when sam is given. aim_set_wait copies back the n records and exactly the words
 * and bytes that were written. */
typedef struct aim_batch_io_sam {
    aim_batch_io_mates_t mates;    /* @0, 184 B: unchanged meaning */
    aim_sam_t *sam;                /* out: [n_pairs], or [n_reads] under AIM_FLAG_READ_GROUPS */
    uint32_t *sam_cigar;           /* out: BAM CIGAR words */
    uint32_t sam_cigar_cap;        /* capacity of sam_cigar[], in words */
    char *sam_md;                  /* out: MD bytes */
    uint32_t sam_md_cap;           /* capacity of sam_md[], in bytes */
    uint32_t sam_options;          /* AIM_SAM_EQX */
} aim_batch_io_sam_t;
/* Sizes the per-slot device buffers of the records: call after aim_set_configure_slots (a re-configure drops them). A submit with the
 * flag before this call returns AIM_ESTATE. A batch may use less (sam_cigar_cap / sam_md_cap), never more. */
int aim_set_sam_capacity(aim_set_t *set, uint32_t max_cigar_words, uint32_t max_md_bytes);

/* AIM_FLAG_TOP_HITS: aim_set_submit reads past `sam` (only with the flag). Of `sam` the groups members are read; its mates and sam
 * members are ignored. base.results, ops, cigars and runs receive H = hit_offsets[n_reads] rows, groups.best n_reads rows. */
typedef struct aim_batch_io_hits {
    aim_batch_io_sam_t sam;        /* @0, 224 B */
    uint32_t max_hits, pad;        /* 1..AIM_TOP_HITS_MAX; 0 */
    const uint32_t *hit_offsets;   /* in: [n_reads + 1], as aim_hits_offsets gives it */
    uint32_t *hit_pair;            /* out: [H] candidate (batch index) of every hit row, or NULL */
} aim_batch_io_hits_t;
/* Host helper: hit_offsets[r] = the sum of min(K_q, max_hits) over the reads q < r, for r = 0..n_reads, K_q = read_offsets[q + 1] -
 * read_offsets[q]; *n_hits (may be NULL) receives hit_offsets[n_reads]. AIM_EINVAL when max_hits is outside 1..AIM_TOP_HITS_MAX or a
 * pointer is NULL. The CSR itself is aim_groups_check's business (a decreasing pair of offsets counts as an empty read here).
 * aim_set_submit recomputes the offsets before anything is enqueued: a mismatch is AIM_EINVAL naming the first bad read. */
int aim_hits_offsets(uint32_t n_reads, const uint32_t *read_offsets, uint32_t max_hits, uint32_t *hit_offsets /* [n_reads + 1] */,
                     uint32_t *n_hits);

/* aim_set_configure with `slots` (1..4) buffer sets per device; max_raw_pairs bounds n_raw of a packed batch
 * (0 = packed input not used), max_runs the run buffer of a compact-CIGAR batch (0 = not used). */
int aim_set_configure_slots(aim_set_t *set, const aim_params_t *params, uint32_t max_pairs_per_device, uint32_t slots,
                            uint32_t max_raw_pairs, uint32_t max_runs);
/* Enqueue one batch on (device, slot): H2D, [unpack], alignment kernel(s), [CIGAR run-length encoding], D2H into the
 * buffers named in *io (which must stay valid, and should be pinned -- aim_host_alloc -- for the copies to overlap).
 * Returns immediately.  A slot holds one batch at a time: aim_set_wait it before submitting to it again. */
int aim_set_submit(aim_set_t *set, uint32_t device, uint32_t slot, const aim_batch_io_t *io /* with AIM_FLAG_REF_TEXTS: the base
                   of an aim_batch_io_ref_t */);
/* Block until the batch on (device, slot) is complete.  n_runs (may be NULL) receives the number of runs written.
 * Returns AIM_EALIGN like aim_set_pull when a pair stopped with a status other than AIM_PAIR_OK. */
int aim_set_wait(aim_set_t *set, uint32_t device, uint32_t slot, uint32_t *n_runs);
/* Host-side packer used by the CLI and the tests: packs one sequence (len bytes) into row[ceil(read_size/16)]; returns 1
 * when every byte is A/C/G/T, 0 when the pair must travel raw (the row content is then unspecified). */
int aim_pack_sequence(const char *seq, int32_t len, int32_t read_size, uint32_t *row);
/* Whole-batch packer (host threads): ASCII rows -> packed rows + raw side list, exactly what aim_batch_io_t takes.
 * *n_raw receives the number of pairs that must travel raw; AIM_ENOMEM when it exceeds max_raw (ship the batch as ASCII).
 * With AIM_FLAG_REF_TEXTS texts and packed_texts may be NULL (and raw_texts is then not written): a pair is raw when its pattern
 * holds a byte outside A/C/G/T. */
int aim_pack_batch(const aim_params_t *params, uint32_t n_pairs, const void *requests, const char *patterns, const char *texts,
                   uint32_t *packed_patterns, uint32_t *packed_texts, uint32_t *raw_pairs, char *raw_patterns,
                   char *raw_texts, uint32_t max_raw, uint32_t *n_raw, int threads);
/* edit_cigar_print (host.c:69-89) from runs: adjacent runs of the same op are merged; returns bytes written incl. '\n'. */
int aim_cigar_format_runs(const uint32_t *runs, uint32_t n_runs, char *out, int32_t cap);

/* Pinned host staging for aim_set_push / aim_set_pull / aim_set_submit. */
int aim_host_alloc(void **ptr, size_t bytes);
int aim_host_free(void *ptr);

/* ---- device-resident entry point ----------------------------------------
 * One alignment launch over buffers that already live in HBM (same layouts as
 * above).  Used by the benchmark and by callers that manage device memory
 * themselves.  hip_stream is a hipStream_t (NULL = default stream); the call
 * only enqueues work.  d_scratch must hold aim_scratch_bytes() bytes.  Scratch is need-capped; for table-heavy
 * configurations (full-DP CIGAR at long reads) it is bounded by AIM_SCRATCH_GB, default 3/4 of the device's free
 * memory read once per process, and a smaller bound only means fewer pairs in flight (more rounds), never an error
 * unless not even one workgroup's table fits (AIM_ENOMEM).
 * d_patterns / d_texts must be 16-byte aligned and carry >= 16 bytes of
 * addressable slack after the last row (the kernels read whole 16-byte chunks).
 * A sequence may fill its row (pattern_len, text_len <= READ_SIZE): the bytes of a row behind its length, and the slack's,
 * are never interpreted, whatever they hold; a pair of 2 * READ_SIZE operations fills its ops row from begin_offset 0.
 * The host arrays of aim_set_push / aim_set_submit need no slack. */
size_t aim_scratch_bytes(const aim_params_t *params, uint32_t n_pairs);
int aim_align_device(const aim_params_t *params, uint32_t n_pairs, const void *d_requests,
                     const char *d_patterns, const char *d_texts, void *d_results,
                     char *d_ops, void *d_scratch, size_t scratch_bytes, void *hip_stream);
/* AIM_FLAG_REF_TEXTS: aim_align_device with the texts gathered from d_reference (ref_len bytes, 16-byte aligned, >= 16 bytes of
 * addressable slack after the last byte) at d_text_pos[n_pairs] (uint64_t, device memory). aim_scratch_bytes then includes the text
 * rows: the flag-less figure rounded up to 256 B, plus n_pairs * read_size + 256 B. The caller is responsible for the windows
 * (aim_ref_windows_check); the gather never reads outside [0, ref_len + 16), so a bad window yields an unspecified result for its
 * pair, never a fault. */
int aim_align_device_ref(const aim_params_t *params, uint32_t n_pairs, const void *d_requests, const char *d_patterns,
                         const uint64_t *d_text_pos, const char *d_reference, uint64_t ref_len, void *d_results, char *d_ops,
                         void *d_scratch, size_t scratch_bytes, void *hip_stream);
/* AIM_FLAG_READ_GROUPS: the stateless form. d_patterns holds n_reads rows, d_texts_or_null n_pairs rows (NULL with
 * AIM_FLAG_REF_TEXTS, which reads d_text_pos_or_null / d_reference / ref_len like aim_align_device_ref; otherwise those are ignored),
 * d_read_offsets the CSR (device memory, checked by the caller: aim_groups_check). d_results / d_ops / d_best receive n_reads rows
 * (d_ops only with AIM_FLAG_BACKTRACE; d_best may be NULL). aim_scratch_bytes(params, n_pairs) under the flag covers n_reads = n_pairs.
 * A CSR the check would refuse yields unspecified rows, never an access outside the buffers. */
int aim_align_device_groups(const aim_params_t *params, uint32_t n_pairs, uint32_t n_reads, const void *d_requests, const char *d_patterns,
                            const char *d_texts_or_null, const uint64_t *d_text_pos_or_null, const char *d_reference, uint64_t ref_len,
                            const uint32_t *d_read_offsets, void *d_results, char *d_ops, aim_best_t *d_best, void *d_scratch,
                            size_t scratch_bytes, void *hip_stream);
/* AIM_FLAG_MATE_PAIRS: aim_align_device_groups' arguments (d_texts_or_null must be NULL: the flag needs AIM_FLAG_REF_TEXTS), then the
 * pairing parameters and d_mates[n_reads / 2] (device memory; may be NULL). n_reads must be even (aim_mates_check). d_best still
 * receives the independent selection (may be NULL: aim_scratch_bytes under the flag includes a copy for the kernel). */
int aim_align_device_mates(const aim_params_t *params, uint32_t n_pairs, uint32_t n_reads, const void *d_requests, const char *d_patterns,
                           const char *d_texts_or_null, const uint64_t *d_text_pos_or_null, const char *d_reference, uint64_t ref_len,
                           const uint32_t *d_read_offsets, void *d_results, char *d_ops, aim_best_t *d_best, int64_t min_span,
                           int64_t max_span, int32_t unpaired_penalty, aim_mate_t *d_mates, void *d_scratch, size_t scratch_bytes,
                           void *hip_stream);
/* AIM_FLAG_TOP_HITS: aim_align_device_groups' arguments, then max_hits, d_hit_offsets[n_reads + 1] (device memory; unchecked like the
 * CSR: a wrong one yields unspecified rows, never an access outside the buffers), n_hits = H as aim_hits_offsets gave it (<= n_pairs) and
 * d_hit_pair[H] (device memory; may be NULL). d_results and d_ops hold H rows, d_best n_reads rows. aim_scratch_bytes under the flag is
 * the figure without it plus the hit list: n_pairs * 4 bytes rounded up to 256 B. */
int aim_align_device_hits(const aim_params_t *params, uint32_t n_pairs, uint32_t n_reads, const void *d_requests, const char *d_patterns,
                          const char *d_texts_or_null, const uint64_t *d_text_pos_or_null, const char *d_reference, uint64_t ref_len,
                          const uint32_t *d_read_offsets, void *d_results, char *d_ops, aim_best_t *d_best, uint32_t max_hits,
                          const uint32_t *d_hit_offsets, uint32_t n_hits, uint32_t *d_hit_pair, void *d_scratch, size_t scratch_bytes,
                          void *hip_stream);
/* The kernel of AIM_FLAG_SAM_FIELDS on rows that already live on the device, after any aim_align_device* call with AIM_FLAG_BACKTRACE
 * (params are that call's; the flag itself is not needed). Row r uses text_pos entry d_sel[r] -- entry r when d_sel is NULL; UINT32_MAX
 * gives an unmapped record -- while d_results[n_rows] and d_ops[n_rows][2 * read_size] are indexed by row. d_requests (aim_request_t[] or,
 * with AIM_FLAG_REQ8, aim_request8_t[]) is taken for symmetry with the other entry points: the records derive from the ops ranges alone.
 * d_cursors holds 2 dwords, zeroed by the call: afterwards {CIGAR words, MD bytes} the batch needed (which may exceed the capacities).
 * AIM_EINVAL (with a message) for AIM_ALGO_GENASM (its windowed walk is unpinned and begin_offset = 0 is another contract), without
 * AIM_FLAG_BACKTRACE, with AIM_FLAG_RES8, and when n_rows * (4 * read_size + 10) >= 2^32 (offsets are 32-bit: split the batch; aim_set_submit applies the
 * same bound to n_pairs before anything is enqueued). Every reference
 * read is clamped to [0, ref_len) and every ops read to the row: rows that disagree with their lengths give an unspecified record,
 * never a fault. The call only enqueues work on hip_stream. */
int aim_sam_device(const aim_params_t *params, uint32_t n_rows, const void *d_requests, const uint64_t *d_text_pos,
                   const uint32_t *d_sel_or_null, const void *d_results, const char *d_ops, const char *d_reference, uint64_t ref_len,
                   uint32_t options, aim_sam_t *d_sam, uint32_t *d_cigar, uint32_t cigar_cap, char *d_md, uint32_t md_cap,
                   uint32_t *d_cursors, void *hip_stream);
/* Which of the two record kernels (sam_fields.hpp) a launch with these params takes in this process right now: "sam_lane_kernel" (one row
 * per lane) or "sam_wave_kernel" (one row per wavefront), by read_size; the names match the rocprofv3 kernel-trace prefixes. A set freezes
 * the choice at aim_set_configure like every other AIM_* switch. */
const char *aim_sam_kernel_name(const aim_params_t *params);

/* ---- device-side seeding (AIM_FEATURE_SEED): candidate windows from a k-mer index -----------------------------------------
 * The step in front of AIM_FLAG_REF_TEXTS | AIM_FLAG_READ_GROUPS: reads go in, and requests[] / text_pos[] for K candidate windows per
 * read come out in device memory, in the fixed shape slot = r * K + i, so that aim_align_device_groups / _mates / _hits consume them
 * without a trip through the host. Empty slots are marked, nothing is compacted, scanned or counted across reads, and the host knows
 * every size before it launches. No flag of aim_params_t is involved.
 * INDEX. The k-mer at reference position p is seq[p, p + k); base i of it sits at bits [2i, 2i + 1] of its code, with the packed
 *   rows' code (ascii >> 1) & 3 (A 0, C 1, T 2, G 3). A k-mer that covers any byte other than upper-case A C G T is not indexed.
 *   bucket[4^k + 1] is the exclusive prefix sum of the codes' counts and pos[bucket[c] .. bucket[c + 1]) holds the positions of code c
 *   in ascending order: 4^k * 4 B + 4 B per position. Positions and diagonal keys are 32-bit: ref_len <= AIM_SEED_MAX_REF_LEN.
 * RULE, for read r of length L = read_len[r] (0..read_size) and strand s in {0, 1}; deterministic and independent of the grid:
 *   1. The query is the read (s = 0) or its reverse complement (s = 1). Only A C G T are complemented; any other byte stays, and a
 *      k-mer that covers one is skipped.
 *   2. Seeds sit at query offsets j = 0, stride, 2 * stride, ... with j + k <= L. A seed whose code has n reference positions is
 *      skipped when n = 0 or n > max_occ; otherwise every position p, in ascending order, yields the hit key a = p + read_size - j
 *      (uint32_t: the diagonal, biased to stay non-negative).
 *   3. Hits are kept in (j, p) order up to AIM_SEED_MAX_HITS per strand; later ones are dropped and AIM_SEED_TRUNCATED is set.
 *      n_hits[s] counts the kept ones.
 *   4. The strand's keys are sorted. A cluster is a maximal run whose consecutive differences are <= band; it has votes (its
 *      length), a_lo (its first key) and a_hi (its last).
 *   5. The clusters of both strands with votes >= min_votes are ranked by (votes descending, strand ascending, a_lo ascending); the
 *      first K = max_cands become the candidates, n_cands is their number.
 *   6. Candidate i fills slot r * K + i. With lo = a_lo - read_size - flank (signed 64-bit) and
 *      hi = lo + L + 2 * flank + min(a_hi - a_lo, read_size): start = max(lo, 0), end = max(start, min(hi, ref_len));
 *      requests[slot] = {pattern_len L, text_len min(end - start, read_size), 0, idx_base + slot}, text_pos[slot] = start | s << 63,
 *      votes[slot] = votes.
 *   7. Slots from n_cands on are empty: {L, 0, 0, idx_base + slot}, text_pos 0, votes 0. An empty window is always inside the
 *      reference; under AIM_FLAG_READ_GROUPS such a candidate scores a pure gap of L bases, and callers read n_cands.
 * The window is on the forward reference and strand 1 sets bit 63: exactly what AIM_FLAG_REF_TEXTS reverse-complements. Flanked
 * windows are usually aligned with AIM_FLAG_ENDSFREE (text_begin_free = text_end_free = 2 * flank).
 * MINIMIZERS (AIM_FEATURE_MINIMIZERS). With a window w the index holds, and a query looks up, only the (w, k) minimizers: the same
 *   positions are chosen in the reference and in the query, every exact match of w + k - 1 bases shares at least one seed, and on random
 *   sequence about 2 / (w + 1) of the positions are kept.
 *   Order. A valid k-mer of code c has the order key h(c), in uint32_t arithmetic:
 *       x = c;  x ^= x >> 16;  x *= 0x85ebca6b;  x ^= x >> 13;  x *= 0xc2b2ae35;  x ^= x >> 16
 *     h is a bijection on 32 bits, so two k-mers tie only when they are the same k-mer. A k-mer that covers a byte other than
 *     upper-case A C G T is invalid and compares greater than every valid key, 0xFFFFFFFF included.
 *   Windows. A sequence of len bytes has n = len - k + 1 k-mer start positions. For n >= w the windows are [s, s + w) for
 *     s = 0 .. n - w; for 0 < n < w there is the one window [0, n).
 *   Selection. The minimizer of a window is its leftmost position of smallest key; a window whose k-mers are all invalid has none. A
 *     position is selected when it is the minimizer of at least one window. Equivalently, a valid position i is selected iff
 *     L + R + 1 >= min(w, n), where L counts the consecutive positions immediately left of i whose key is strictly greater (it stops at
 *     the sequence start) and R the consecutive positions immediately right of i whose key is greater or equal (it stops at the
 *     sequence end); both may be capped at w - 1.
 *   Index. bucket[] / pos[] as above, except that only the selected reference positions are counted and stored; bucket[4^k] is their
 *     number. w = 1 selects every valid k-mer: the bytes of aim_index_build.
 *   Seeding. Only rule 2 changes: the seeds of a strand's query (the read, or its reverse complement) are its selected positions j in
 *     ascending order, computed on the query itself, left to right; stride must be 1. max_occ, the key a = p + read_size - j, rules 3-7
 *     are untouched. The index must have been built with the same (k, w): nothing in the arrays records w, so the library cannot check
 *     that, and a mismatch only loses seeds.
 * Follow-ups, not in this version: packed read rows, spaced seeds, a seeding stage inside aim_set_submit, compacting the selected
 * positions before the device build's sort; for chaining (below) also a lookback other than 64, and beyond
 * aim_seed_chain_long_device more than 8 192 anchors per strand and reads above 65 528 bases. Check
 * aim_features() & AIM_FEATURE_SEED first. */
#define AIM_SEED_MAX_CANDS 16
#define AIM_SEED_MAX_HITS 1024      /* hits kept per (read, strand) */
#define AIM_SEED_TRUNCATED 0x1u     /* aim_seed_t.flags: a strand dropped hits beyond AIM_SEED_MAX_HITS */
#define AIM_SEED_MAX_READ_SIZE 4096 /* the read row is staged in LDS next to the key arrays */
#define AIM_SEED_MAX_REF_LEN 0xFE000000ull /* 2^32 - 2^25 */
#define AIM_SEED_MAX_W 32           /* minimizer window, 1..AIM_SEED_MAX_W */
#define AIM_SEED_OPT_MINIMIZERS(w) ((uint32_t)(w) << 8) /* aim_seed_params_t.options: seeds are the query's (w, k) minimizers */
typedef struct aim_seed_params {
    int32_t k;          /* 8..14 */
    int32_t stride;     /* >= 1: seeds start at read offsets 0, stride, 2*stride, ... */
    int32_t max_occ;    /* >= 1: a k-mer with more reference positions than this is skipped */
    int32_t band;       /* >= 0: consecutive sorted diagonals at most this far apart share a cluster */
    int32_t flank;      /* >= 0: reference bases added on each side of a cluster's window */
    int32_t min_votes;  /* >= 1 */
    int32_t max_cands;  /* K, 1..AIM_SEED_MAX_CANDS */
    int32_t read_size;  /* row stride of the read rows, multiple of 8, <= AIM_SEED_MAX_READ_SIZE; also the cap on text_len */
    uint32_t idx_base;  /* requests[r*K+i].idx = idx_base + r*K + i */
    uint32_t options;   /* 0, or AIM_SEED_OPT_MINIMIZERS(w) with stride 1; every other bit must be 0 */
} aim_seed_params_t;
typedef struct aim_seed { uint32_t n_cands, n_hits[2], flags; } aim_seed_t;   /* 16 B per read */
/* Sizes of the index arrays, in entries: *bucket_entries = 4^k + 1, *pos_capacity = ref_len - k + 1 (0 below k). AIM_EINVAL for a k
 * outside 8..14 or a ref_len above AIM_SEED_MAX_REF_LEN. */
int aim_index_sizes(int32_t k, uint64_t ref_len, uint64_t *bucket_entries, uint64_t *pos_capacity);
/* Builds the index on the host (no device is needed): a counting sort in two passes with `threads` workers (< 1 counts as 1), each of
 * which owns a range of codes, so the result does not depend on `threads`. bucket and pos hold what aim_index_sizes reports (pos may
 * be NULL when its capacity is 0); *n_pos (may be NULL) receives bucket[4^k], the number of positions written. */
int aim_index_build(const char *seq, uint64_t ref_len, int32_t k, uint32_t *bucket, uint32_t *pos, uint64_t *n_pos, int threads);
/* aim_index_build over the (w, k) minimizers of seq alone (AIM_FEATURE_MINIMIZERS, the rule above): same arrays, same sizes, same
 * meaning of threads and n_pos. pos_capacity is an upper bound -- about 2 / (w + 1) of it is used on random sequence -- and a caller
 * may keep only pos[0, *n_pos). AIM_EINVAL as aim_index_build, and for a w outside 1..AIM_SEED_MAX_W. */
int aim_index_build_minimizers(const char *seq, uint64_t ref_len, int32_t k, int32_t w, uint32_t *bucket, uint32_t *pos, uint64_t *n_pos,
                               int threads);
/* ---- the same index, built on the device (AIM_FEATURE_INDEX_DEVICE) ----
 * Bytes of device scratch aim_index_build_device needs for (k, ref_len); 0 is a legal answer (ref_len < k). With P = ref_len - k + 1
 * positions and A(x) = x rounded up to 256:  scratch = 3 * A(4 * P) + A(1024 * ceil(P / 4096)) + 8192  -- two key arrays and one
 * position array of a dword per position, 256 dwords of digit table per tile of 4096 positions, and the scan's 2048 part sums: about
 * 12.25 B per position, 52 GB at AIM_SEED_MAX_REF_LEN. AIM_EINVAL as aim_index_sizes, and for a NULL scratch_bytes. */
int aim_index_device_scratch(int32_t k, uint64_t ref_len, uint64_t *scratch_bytes);
/* The index of aim_index_build, built on the device from ASCII reference bytes already there (d_reference as for
 * aim_align_device_ref: 16-byte aligned, >= 16 bytes of slack). d_bucket / d_pos hold what aim_index_sizes reports. Only enqueues
 * work on hip_stream; allocates nothing; d_scratch (256-byte aligned) may be reused once the stream has passed. Afterwards d_bucket
 * equals aim_index_build's bucket and d_pos[0, d_bucket[4^k]) its pos, byte for byte; entries of d_pos from d_bucket[4^k] on are
 * unspecified (the call uses all of d_pos as a sort buffer). The result does not depend on the grid, on what the scratch held, or on
 * the order in which workgroups run: a stable radix sort of the positions by code, with the counts of bucket[] the only atomics
 * (csrc/index.hpp). AIM_EINVAL with a message naming the cause for a k outside 8..14, a ref_len above AIM_SEED_MAX_REF_LEN, a NULL
 * buffer that the sizes make necessary (d_bucket always; d_reference, d_pos and d_scratch from ref_len >= k), a d_reference or
 * d_scratch that is misaligned and a scratch_bytes below aim_index_device_scratch. ref_len < k is legal: an all-zero bucket and
 * nothing else is written. */
int aim_index_build_device(const char *d_reference, uint64_t ref_len, int32_t k, uint32_t *d_bucket, uint32_t *d_pos,
                           void *d_scratch, uint64_t scratch_bytes, void *hip_stream);
/* Comma-separated rocprofv3 kernel-trace name prefixes of aim_index_build_device's kernels, in launch order. */
const char *aim_index_kernel_names(void);
/* aim_index_build_minimizers on the device (AIM_FEATURE_MINIMIZERS): the contract, the scratch (aim_index_device_scratch) and the
 * refusals of aim_index_build_device, and AIM_EINVAL with a message naming w for a w outside 1..AIM_SEED_MAX_W. Afterwards d_bucket and
 * d_pos[0, d_bucket[4^k]) equal aim_index_build_minimizers', byte for byte. index_minimizer_kernel takes the place of
 * index_code_kernel; the sort behind it is the same launches over all ref_len - k + 1 positions, selected or not. */
int aim_index_build_device_minimizers(const char *d_reference, uint64_t ref_len, int32_t k, int32_t w, uint32_t *d_bucket,
                                      uint32_t *d_pos, void *d_scratch, uint64_t scratch_bytes, void *hip_stream);
/* "index_minimizer_kernel,seed_minimizer_kernel": comma-separated rocprofv3 kernel-trace name prefixes of the kernels
 * AIM_FEATURE_MINIMIZERS adds, the code pass of aim_index_build_device_minimizers and aim_seed_device's kernel under
 * AIM_SEED_OPT_MINIMIZERS. */
const char *aim_minimizer_kernel_names(void);
/* The seeding kernel over device buffers: ASCII read rows d_reads[n_reads][read_size] (aligned and with slack like d_patterns),
 * d_read_len[n_reads], the index of a reference of ref_len bytes, and the outputs of the rule above: d_requests
 * (aim_request_t[n_reads * K]), d_text_pos, d_votes (each [n_reads * K]) and d_seed[n_reads]. The call only enqueues work on
 * hip_stream and needs no scratch: everything per read lives in LDS. A read_len outside 0..read_size is clamped; index entries that
 * point outside the arrays aim_index_sizes describes make a seed count as absent, never a fault: a code c whose entries fail
 * bucket[c] <= bucket[c + 1] <= pos_capacity has no positions, and every other code has pos[bucket[c] .. bucket[c + 1]) as it
 * stands, in the array's order. AIM_EINVAL with a message naming the
 * field for every bound of aim_seed_params_t, for ref_len, and for n_reads * K >= 2^32. With options = AIM_SEED_OPT_MINIMIZERS(w) the
 * kernel is seed_minimizer_kernel and d_bucket / d_pos must be a minimizer index of the same (k, w). */
int aim_seed_device(const aim_seed_params_t *sp, uint32_t n_reads, const int32_t *d_read_len, const char *d_reads,
                    const uint32_t *d_bucket, const uint32_t *d_pos, uint64_t ref_len, void *d_requests /* aim_request_t[n_reads*K] */,
                    uint64_t *d_text_pos, uint32_t *d_votes, aim_seed_t *d_seed, void *hip_stream);
/* Host helper: read_offsets[r] = r * K for r = 0..n_reads, the CSR AIM_FLAG_READ_GROUPS wants for the slots above. AIM_EINVAL for a
 * K outside 1..AIM_SEED_MAX_CANDS, a NULL pointer or n_reads * K >= 2^32. */
int aim_seed_groups_offsets(uint32_t n_reads, uint32_t K, uint32_t *read_offsets /* [n_reads + 1] */);
/* "seed_candidates_kernel": the rocprofv3 kernel-trace name prefix of aim_seed_device's kernel. */
const char *aim_seed_kernel_name(void);

/* ---- colinear chaining of the seed hits (AIM_FEATURE_SEED_CHAIN): chain-scored candidates with exact windows ----------------
 * aim_seed_chain_device is aim_seed_device with rules 4-6 replaced: instead of sorting diagonals and cutting them into clusters by
 * band, it chains the hits (p, j) with a gap cost, so a candidate's window follows the chain's net indel instead of its diagonal
 * spread, and each candidate says which part of the read supports it. Rules 1-3 and 7, n_hits, AIM_SEED_TRUNCATED, the idx and slot
 * layout, aim_seed_params_t and both seed sources (stride over the full index, or AIM_SEED_OPT_MINIMIZERS(w) over a minimizer index)
 * are those of the seeding section above. For read r of length L and strand s, with k = aim_seed_params_t.k:
 *   4c. Anchors. A kept hit of strand s is the pair (p, j): reference position and query offset; at most AIM_SEED_MAX_HITS per
 *       strand, truncated in (j, p) order by rule 3. They are sorted ascending by (p, j); the pairs are distinct.
 *       Lookback. The candidate predecessors of anchor i are the AIM_SEED_CHAIN_LOOKBACK anchors immediately before it in sorted
 *       order (fewer at the start).
 *       Admissible. With dp = p_i - p_j and dq = j_i - j_j (compared in 64 bits), predecessor j is admissible iff dp > 0, dq > 0 and
 *       |dp - dq| <= band. band is 0..AIM_SEED_CHAIN_MAX_BAND here.
 *       Score. gain = min(dp, dq, k); g = |dp - dq|; cost(0) = 0 and cost(g) = ((g * k) >> 7) + ((floor(log2 g) + 1) >> 1) otherwise;
 *       f(i) = max(k, max over admissible j of f(j) + gain - cost). Anchor i takes a predecessor only when the best candidate score is
 *       strictly greater than k; among equal best scores it takes the one of largest sorted index (the nearest). Otherwise i is a
 *       root. k <= f <= AIM_SEED_MAX_HITS * 14, and no f is negative.
 *       Chains. The predecessor links form trees, and each tree yields one chain: its end is the tree's anchor of greatest f (the
 *       lowest sorted index on a tie) and the chain is the path from that end to the root. score = f(end), n_anchors = the path's
 *       length, (p_lo, q_lo) = the root, p_hi = p_end + k, q_hi = j_end + k. Chains with n_anchors < min_votes are dropped.
 *   5c. The chains of both strands are ranked by (score descending, strand ascending, p_lo ascending, q_lo ascending); the first
 *       K = max_cands become the candidates, n_cands is their number.
 *   6c. Candidate i fills slot r * K + i. In signed 64 bits: lo = p_lo - q_lo - flank, hi = p_hi + (L - q_hi) + flank,
 *       start = max(lo, 0), end = max(start, min(hi, ref_len)); requests[slot] = {L, min(end - start, read_size), 0, idx_base + slot},
 *       text_pos[slot] = start | s << 63, votes[slot] = score.
 * aim_chain_t (optional, one per slot): score and n_anchors as above, q_lo, q_hi, and ref_span = p_hi - p_lo. [q_lo, q_hi) is the
 * query interval the chain covers; for strand 1 the query is the read's reverse complement, so the interval of the read as given is
 * [L - q_hi, L - q_lo). A caller clips with it, or takes it as the read interval of one part of a split read. Empty slots (rule 7)
 * are all zero. */
#define AIM_SEED_CHAIN_LOOKBACK 64
#define AIM_SEED_CHAIN_MAX_BAND 4096
typedef struct aim_chain {
    uint32_t score;
    uint16_t n_anchors, reserved;
    uint16_t q_lo, q_hi;
    uint32_t ref_span;
} aim_chain_t;   /* 16 B per slot */
/* aim_seed_device's arguments, checks and messages (under the name aim_seed_chain_device), AIM_EINVAL with a message naming band for
 * a band above AIM_SEED_CHAIN_MAX_BAND, and d_chains: aim_chain_t[n_reads * K], or NULL when they are not wanted -- the other outputs
 * do not depend on it. The kernel is seed_chain_kernel, or seed_chain_minimizer_kernel under AIM_SEED_OPT_MINIMIZERS; like
 * aim_seed_device the call only enqueues work on hip_stream and needs no scratch. Check aim_features() & AIM_FEATURE_SEED_CHAIN. */
int aim_seed_chain_device(const aim_seed_params_t *sp, uint32_t n_reads, const int32_t *d_read_len, const char *d_reads,
                          const uint32_t *d_bucket, const uint32_t *d_pos, uint64_t ref_len, void *d_requests /* aim_request_t[n_reads*K] */,
                          uint64_t *d_text_pos, uint32_t *d_votes, aim_seed_t *d_seed, aim_chain_t *d_chains_or_null, void *hip_stream);
/* "seed_chain_kernel,seed_chain_minimizer_kernel": comma-separated rocprofv3 kernel-trace name prefixes of aim_seed_chain_device's
 * kernels. */
const char *aim_seed_chain_kernel_names(void);

/* ---- chaining for long reads (AIM_FEATURE_SEED_CHAIN_LONG): the aligner's read lengths, a caller-chosen hit cap ----------------
 * aim_seed_chain_long_device is aim_seed_chain_device -- rules 1-3, 4c-6c and 7, aim_chain_t, the slot and idx layout, d_chains or
 * NULL -- for read rows of up to AIM_SEED_LONG_MAX_READ_SIZE bases and up to AIM_SEED_LONG_MAX_HITS anchors per strand, with exactly
 * these differences:
 *   Seeds. Minimizers only: options must be AIM_SEED_OPT_MINIMIZERS(w), w = 1..AIM_SEED_MAX_W, over a minimizer index of the same
 *     (k, w); w = 1 selects every valid k-mer, which is aim_index_build's index. options = 0 is refused. stride must be 1.
 *   Hit cap. max_hits = H takes the place of AIM_SEED_MAX_HITS in rule 3, in rule 4c and in n_hits / AIM_SEED_TRUNCATED: hits are kept
 *     in (j, p) order up to H per strand. H is a power of two in 1024..AIM_SEED_LONG_MAX_HITS. It is part of the rule -- it decides
 *     which hits are dropped -- and k <= f <= H * 14.
 *   Read size. read_size is a positive multiple of 8, at most AIM_SEED_LONG_MAX_READ_SIZE: the largest multiple of 8 for which q_hi
 *     fits aim_chain_t's uint16_t. text_len = min(end - start, read_size) as before; a read_len outside 0..read_size is clamped.
 * Everything else is identical: band <= AIM_SEED_CHAIN_MAX_BAND, the lookback of AIM_SEED_CHAIN_LOOKBACK, gain, cost and the tie
 * rules, the ranking by (score descending, strand, p_lo, q_lo), the windows, the empty slots, and the tolerance of index entries that
 * point outside the arrays. So for read_size <= AIM_SEED_MAX_READ_SIZE and H = AIM_SEED_MAX_HITS every output byte equals
 * aim_seed_chain_device's under the same AIM_SEED_OPT_MINIMIZERS(w). The result is deterministic and independent of the grid.
 * The kernel is seed_chain_long_kernel (csrc/seed_chain_long.hpp): it walks the read in tiles from global memory, so its LDS is
 * 14 * H bytes plus a fixed tile buffer whatever read_size is, and H decides how many reads one compute unit chains at a time
 * (9, 5, 2, 1 for H = 1024, 2048, 4096, 8192). The call only enqueues work on hip_stream and needs no scratch.
 * AIM_EINVAL with a message naming the field: the refusals of aim_seed_chain_device under the name aim_seed_chain_long_device, with
 * the read_size bound above, and for a max_hits that is no power of two in 1024..AIM_SEED_LONG_MAX_HITS and for options = 0. The
 * parameter checks come before any device query. aim_seed_device and aim_seed_chain_device keep their bounds. */
#define AIM_SEED_LONG_MAX_READ_SIZE 65528
#define AIM_SEED_LONG_MAX_HITS 8192
int aim_seed_chain_long_device(const aim_seed_params_t *sp, uint32_t max_hits, uint32_t n_reads, const int32_t *d_read_len, const char *d_reads,
                               const uint32_t *d_bucket, const uint32_t *d_pos, uint64_t ref_len, void *d_requests /* aim_request_t[n_reads*K] */,
                               uint64_t *d_text_pos, uint32_t *d_votes, aim_seed_t *d_seed, aim_chain_t *d_chains_or_null, void *hip_stream);
/* "seed_chain_long_kernel": the rocprofv3 kernel-trace name prefix of aim_seed_chain_long_device's kernel. */
const char *aim_seed_chain_long_kernel_name(void);

/* ---- primary and secondary chains, MAPQ (AIM_FEATURE_CHAIN_CLASS): what a read's K candidates are to each other ------------------
 * After aim_seed_chain_device or aim_seed_chain_long_device the candidates of a read are a list ranked by score. Rule 8c says which of
 * them cover the same part of the read at another locus (secondaries: repeat copies) and which cover a part no better chain covers
 * (primaries; beyond candidate 0 supplementary: the other part of a split or chimeric read), and gives each primary a MAPQ from the
 * chains alone. Rule 9c, after verification, turns that and aim_best_t / aim_mate_t into one MAPQ per read. All arithmetic is signed
 * and in at least 32 bits unless 64 is stated; both results are deterministic and independent of the grid.
 *   8c. Classification (aim_chain_classify_device). For read r: n = min(d_seed[r].n_cands, K), L = d_read_len[r] clamped to
 *       0..read_size (the clamp of the chain kernels), and candidate i (0 <= i < n) is slot r * K + i, in the order the chain kernel
 *       wrote it.
 *       Read interval. With c = d_chains[slot] and s = d_text_pos[slot] >> 63: [a_i, b_i) = [c.q_lo, c.q_hi) for s = 0 and
 *       [L - c.q_hi, L - c.q_lo) for s = 1 -- the interval of the read as given (see aim_chain_t above). len_i = b_i - a_i.
 *       Overlap. ov(i, j) = min(b_i, b_j) - max(a_i, a_j). i and j overlap iff ov > 0 and 256 * ov >= mask_q8 * min(len_i, len_j);
 *       equality counts as overlap. mask_q8 is 1..256; AIM_CHAIN_MASK_DEFAULT = 128 is minimap2's mask level of 0.5. A candidate
 *       with len <= 0 (malformed input) overlaps nothing.
 *       Parent. Candidate 0 is primary and parent(0) = 0. For i = 1 .. n - 1 in order, parent(i) is the lowest j < i that is primary
 *       and overlaps i; if there is none, i is primary and parent(i) = i. A secondary is never a parent.
 *       Flags. A primary gets AIM_CHAIN_PRIMARY, a primary with i > 0 also AIM_CHAIN_SUPPLEMENTARY, every other candidate
 *       AIM_CHAIN_SECONDARY.
 *       Sub-score. For a primary j, n_sub is the number of i != j with parent(i) = j and sub_score the greatest c.score among them
 *       (0 if there are none). For a secondary both are 0.
 *       Chain MAPQ of a primary. f1 = c.score, f2 = sub_score, m = min(c.n_anchors, 10): mapq = min(60, (6 * m * (f1 - f2)) / f1) in
 *       64 bits, integer division; 0 when f1 = 0 or f2 > f1. A secondary has mapq 0. The formula is this project's own: minimap2's
 *       (1 - f2 / f1) factor and its penalty for few anchors, without the log factor, so that the rule is exact in integers.
 *       Empty slots (i >= n) are 8 zero bytes.
 *       Parents only rank higher, so the classification of the kept candidates equals what classifying every chain of the read and
 *       keeping the first K would give. sub_score and n_sub see the kept candidates only; they are exact when n_cands < K.
 *   9c. MAPQ of a read (aim_read_mapq_device), after aim_align_device_groups or aim_align_device_mates over the chain kernel's slots
 *       with read_offsets[r] = r * K (aim_seed_groups_offsets), so that best_pair is a slot.
 *       Selection. sel = d_best[r].best_pair; with d_mates and m = r / 2, sel = d_mates[m].best_pair[r & 1].
 *       Unmapped. sel == UINT32_MAX, sel - r * K >= K (unsigned) or d_class[sel].flags == 0 (an empty slot) gives
 *       {slot = sel, mapq = chain_mapq = aln_mapq = 0, flags = AIM_MAPQ_UNMAPPED}. No entry of d_class outside the read's own K slots
 *       is ever read.
 *       Chain evidence. p = r * K + d_class[sel].parent and chain_mapq = d_class[p].mapq: the ambiguity of a locus is that of its
 *       primary, also when verification preferred the secondary. (A parent >= K, which rule 8c never writes, gives chain_mapq 0.)
 *       Alignment evidence (b, s2, nb) = d_best[r].(best_score, second_score, n_best); with d_mates and
 *       d_mates[m].flags & AIM_MATE_PROPER it is d_mates[m].(score_sum, second_sum, n_best) instead. aln_mapq = 0 when nb > 1, 60 when
 *       s2 == INT32_MAX, otherwise min(60, 6 * max(s2 - b, 0) / score_unit) in 64 bits. score_unit >= 1 is the caller's cost of one
 *       mismatch; only the difference is used, so negative scores (SWG with a match bonus) are fine.
 *       A WFA candidate over the cap counts with MAX_SCORE + 1 (AIM_FLAG_READ_GROUPS), a lower bound of its cost: aln_mapq reaches 60
 *       only where MAX_SCORE + 1 >= b + 10 * score_unit.
 *       Result. mapq = min(chain_mapq, aln_mapq). For a proper pair mapq = min(aln_mapq, max(chain_mapq, the mate's chain_mapq)): a
 *       pair is as well anchored as its better mate; a mate that is unmapped by the rule above counts as 0.
 *       Flags. AIM_MAPQ_UNMAPPED; AIM_MAPQ_SECONDARY: the chosen candidate is a secondary chain; AIM_MAPQ_SUPPLEMENTARY: it is a
 *       primary of index > 0; AIM_MAPQ_PROPER.
 * Both calls only enqueue work on hip_stream, allocate nothing and need no scratch; d_class and d_mapq are 8 bytes per row and must be
 * 4-byte aligned. AIM_EINVAL with a message under the entry point's name, before any device query: K outside 1..AIM_SEED_MAX_CANDS,
 * mask_q8 outside 1..256, a read_size that is 0, no multiple of 8 or above AIM_SEED_LONG_MAX_READ_SIZE, n_reads * K >= 2^32,
 * score_unit < 1, an odd n_reads with d_mates and, last of all, a NULL device buffer.
 * Not in this version: MAPQ inside aim_sam_t (a caller joins d_mapq[r] with record r; the supplementary parts of a split read are
 * aligned through rule 10c below), AIM_FLAG_TOP_HITS rows, the clusters of aim_seed_device (they have no read interval) and a classification stage inside
 * aim_set_submit. */
#define AIM_CHAIN_MASK_DEFAULT 128
#define AIM_CHAIN_PRIMARY 0x1u
#define AIM_CHAIN_SECONDARY 0x2u
#define AIM_CHAIN_SUPPLEMENTARY 0x4u
typedef struct aim_chain_class {
    uint32_t sub_score;
    uint8_t parent;                /* 0..K-1, index within the read */
    uint8_t flags;                 /* AIM_CHAIN_*; 0: an empty slot */
    uint8_t mapq;
    uint8_t n_sub;
} aim_chain_class_t;   /* 8 B per slot */
int aim_chain_classify_device(uint32_t K, uint32_t read_size, uint32_t mask_q8, uint32_t n_reads, const int32_t *d_read_len,
                              const uint64_t *d_text_pos, const aim_seed_t *d_seed, const aim_chain_t *d_chains,
                              aim_chain_class_t *d_class /* [n_reads * K] */, void *hip_stream);
#define AIM_MAPQ_UNMAPPED 0x1u
#define AIM_MAPQ_SECONDARY 0x2u
#define AIM_MAPQ_SUPPLEMENTARY 0x4u
#define AIM_MAPQ_PROPER 0x8u
typedef struct aim_read_mapq {
    uint32_t slot;                 /* the chosen candidate: best_pair as rule 9c selects it */
    uint8_t mapq, chain_mapq, aln_mapq;
    uint8_t flags;                 /* AIM_MAPQ_* */
} aim_read_mapq_t;     /* 8 B per read */
int aim_read_mapq_device(uint32_t K, uint32_t n_reads, int32_t score_unit, const aim_best_t *d_best, const aim_mate_t *d_mates_or_null,
                         const aim_chain_class_t *d_class, aim_read_mapq_t *d_mapq /* [n_reads] */, void *hip_stream);
/* "chain_class_kernel,read_mapq_kernel": comma-separated rocprofv3 kernel-trace name prefixes of the two entry points' kernels. */
const char *aim_chain_class_kernel_names(void);

/* ---- split reads (AIM_FEATURE_SPLIT): one alignable segment row per primary chain, supplementary SAM records -------------------
 * Rule 8c marks the other parts of a split or chimeric read as supplementary primaries. Rule 10c turns every primary into a row an
 * alignment kernel takes: the part of the read that is the primary's, and the window that fits that part. aim_sam_device_split then
 * gives each aligned segment the clips for the rest of its read and SAM's supplementary flag. The sequence is
 *     aim_seed_chain_device | aim_seed_chain_long_device -> aim_chain_classify_device -> aim_split_segments_device ->
 *     aim_align_device_ref over all n_reads * K segment rows (AIM_FLAG_BACKTRACE | AIM_FLAG_ENDSFREE | AIM_FLAG_REF_TEXTS, text free
 *     ends 2 * flank) -> aim_sam_device_split,
 * through device buffers only. Nothing is compacted or counted: segment rows keep the slot layout slot = r * K + i, and the host knows
 * every size before it launches. Arithmetic is signed 64-bit unless stated; the result is deterministic and independent of the grid.
 *   10c. Segments (aim_split_segments_device). For read r: n = min(d_seed[r].n_cands, K), L = d_read_len[r] clamped to 0..read_size,
 *       and [a_i, b_i) and the strand s of candidate i are those of rule 8c. Candidate i is a primary when i < n and
 *       d_class[slot].flags & AIM_CHAIN_PRIMARY.
 *       Open sides. A primary i is left-open when no other primary j of the read has a_j < a_i, and right-open when none has
 *       b_j > b_i. A read with one primary is open on both sides.
 *       Read interval. a' = left-open ? 0 : a_i and b' = right-open ? L : b_i. An open side runs to the end of the read; an inner side
 *       stops exactly where the chain stops, at an exact k-mer match. (Extending an inner side to the true breakpoint is a stage of
 *       its own behind this one: rule 11c, aim_extend_segments_device.) A malformed chain cannot move the interval outside the read: a' is
 *       clamped to 0..L and b' to a'..L. A chain kernel's own chains are never clamped.
 *       Window. In chain-query coordinates low-open = s ? right-open : left-open and high-open = s ? left-open : right-open. With
 *       c = d_chains[slot], start = d_text_pos[slot] & ~AIM_REF_MINUS_STRAND and E = start + d_requests[slot].text_len, rule 6c's
 *       p_lo is recovered: if start > 0, p_lo = start + c.q_lo + flank (the left clamp did not act); otherwise, if
 *       0 < text_len < read_size and E < ref_len, p_lo = E - (L - c.q_hi) - flank - c.ref_span (the right side was not clamped, so E
 *       is rule 6c's hi); otherwise p_lo is not recoverable: the segment gets AIM_SEG_LOOSE and both of its window bounds are the
 *       candidate's (start, E). p_hi = p_lo + c.ref_span. seg_start = low-open ? start : min(max(p_lo, 0), ref_len);
 *       seg_end = max(seg_start, high-open ? E : min(max(p_hi, 0), ref_len)); text_len = min(seg_end - seg_start, read_size).
 *       An open side keeps the candidate's flank; an inner side has none, since it ends on matching bases.
 *       Outputs for a primary. d_seg_requests[slot] = {b' - a', text_len, 0, d_requests[slot].idx};
 *       d_seg_text_pos[slot] = seg_start | s << 63; d_seg_patterns[slot] holds read[a', b') as given (no complement:
 *       AIM_FLAG_REF_TEXTS turns the text), then zero bytes up to read_size; d_seg[slot] = {q_begin = a', q_end = b', read_len = L,
 *       flags, cand = i} with flags = AIM_SEG_VALID, plus AIM_SEG_SUPPLEMENTARY when i > 0, AIM_SEG_LEFT_OPEN, AIM_SEG_RIGHT_OPEN and
 *       AIM_SEG_LOOSE as they apply.
 *       Every other slot (a secondary, an empty slot, i >= n) is rule 7's empty slot, which every alignment kernel already takes:
 *       request {L, 0, 0, d_requests[slot].idx}, text_pos 0, the whole read row (all read_size bytes) as pattern, and a segment record
 *       of 8 zero bytes.
 *       Identity. For a read with a single primary (a' = 0, b' = L, both sides open) the segment's request and text_pos equal the
 *       chain kernel's slot byte for byte, and so does its pattern row wherever the read row is zero behind L.
 *   aim_sam_device_split. aim_sam_device's arguments plus d_seg, indexed like d_text_pos (entry d_sel[r], or r when d_sel is NULL;
 *       no entry is read for UINT32_MAX). Record r is exactly aim_sam_device's record for the row, with two changes.
 *       Clips. lead = q_begin and trail = read_len - q_end for a strand-0 window, swapped for strand 1 (the record shows the read
 *       reverse-complemented). Each is added to the soft clip at that end of the CIGAR, merged with the peeled 'D' bases into the one
 *       S word; a clip of 0 emits no word; n_cigar grows by at most 2.
 *       Flag. flags gains AIM_SAM_SUPPLEMENTARY when the segment has AIM_SEG_SUPPLEMENTARY.
 *       pos, ref_span, nm and MD are untouched. A row whose segment has flags == 0 gets aim_sam_device's record for a row without a
 *       candidate (unmapped, pos 0). Capacity, overflow, the cursors and the 2^32 bound follow aim_sam_device's rules.
 *       Invariant. For a mapped record the CIGAR's read-consuming lengths (M, I, S, =, X) sum to read_len.
 * aim_split_segments_device only enqueues work on hip_stream, allocates nothing and needs no scratch. d_reads and d_seg_patterns are
 * rows of read_size bytes, aligned like d_patterns (8 bytes suffice); d_seg and d_seg_text_pos are 8-byte aligned. The kernel is
 * split_segments_kernel (csrc/split.hpp). AIM_EINVAL with a message under the entry point's name, before any device query: the
 * refusals of aim_chain_classify_device (K outside 1..AIM_SEED_MAX_CANDS, a read_size that is 0, no multiple of 8 or above
 * AIM_SEED_LONG_MAX_READ_SIZE, n_reads * K >= 2^32), flank < 0, a ref_len above AIM_SEED_MAX_REF_LEN and, last of all, a NULL device
 * buffer. aim_sam_device_split refuses what aim_sam_device refuses, and a NULL d_seg with n_rows > 0.
 * Not in this version: a split stage inside aim_set_submit or the host CLI, the SA tag and hard clips, packed read rows, segments
 * from the voting kernel's clusters, MAPQ per segment in aim_sam_t (rule 12c's record carries d_class[slot].mapq); overlap between
 * neighbouring extended segments (rule 11c) is not trimmed. aim_mapper_t (below) runs these stages in order. Check aim_features() & AIM_FEATURE_SPLIT first. */
#define AIM_SEG_VALID 0x1u
#define AIM_SEG_SUPPLEMENTARY 0x2u
#define AIM_SEG_LEFT_OPEN 0x4u
#define AIM_SEG_RIGHT_OPEN 0x8u
#define AIM_SEG_LOOSE 0x10u
#define AIM_SAM_SUPPLEMENTARY 0x800u /* aim_sam_t.flags, from aim_sam_device_split alone */
typedef struct aim_segment {
    uint16_t q_begin, q_end;       /* [a', b'): the segment's interval of the read as given */
    uint16_t read_len;             /* L */
    uint8_t flags;                 /* AIM_SEG_*; 0: no segment in this slot */
    uint8_t cand;                  /* i, the candidate within the read */
} aim_segment_t;       /* 8 B per slot */
int aim_split_segments_device(uint32_t K, uint32_t read_size, int32_t flank, uint64_t ref_len, uint32_t n_reads, const int32_t *d_read_len,
                              const char *d_reads, const void *d_requests /* aim_request_t[n_reads * K] */, const uint64_t *d_text_pos,
                              const aim_seed_t *d_seed, const aim_chain_t *d_chains, const aim_chain_class_t *d_class,
                              void *d_seg_requests /* aim_request_t[n_reads * K] */, uint64_t *d_seg_text_pos,
                              char *d_seg_patterns /* [n_reads * K][read_size] */, aim_segment_t *d_seg /* [n_reads * K] */,
                              void *hip_stream);
int aim_sam_device_split(const aim_params_t *params, uint32_t n_rows, const void *d_requests, const uint64_t *d_text_pos,
                         const uint32_t *d_sel_or_null, const void *d_results, const char *d_ops, const char *d_reference, uint64_t ref_len,
                         uint32_t options, aim_sam_t *d_sam, uint32_t *d_cigar, uint32_t cigar_cap, char *d_md, uint32_t md_cap,
                         uint32_t *d_cursors, const aim_segment_t *d_seg, void *hip_stream);
/* "split_segments_kernel,sam_lane_split_kernel,sam_wave_split_kernel": comma-separated rocprofv3 kernel-trace name prefixes of the
 * kernels the two entry points launch; aim_sam_device_split takes the lane or the wave kernel where aim_sam_kernel_name names
 * aim_sam_device's. */
const char *aim_split_kernel_names(void);

/* ---- segment extension (AIM_FEATURE_EXTEND): the inner sides of split-read segments extended to the breakpoint ------------------
 * Rule 10c stops an inner side at the chain's last exact k-mer, so the read bases between that k-mer and the junction are clipped in
 * both records of a split read. aim_extend_segments_device stands between aim_split_segments_device and aim_align_device_ref: a
 * score-only x-drop alignment moves each inner side outward, and the touched slots are rewritten in place. CIGAR and records stay
 * with the AIM_FLAG_ENDSFREE alignment and aim_sam_device_split, which reads the new q_begin / q_end: the clips shrink by themselves
 * and the CIGAR's read-consuming lengths still sum to read_len. Arithmetic is signed 64-bit unless stated; the result is deterministic
 * and independent of the grid.
 *   11c, part 1: one side. Parameters (aim_extend_params_t): match a >= 1, mismatch x >= 1, gap_o o >= 0, gap_e e >= 1, xdrop Z >= 0,
 *       max_cost in 1..AIM_EXTEND_MAX_COST, band in 1..AIM_EXTEND_MAX_BAND, max_ext in 8..AIM_EXTEND_MAX_EXT. The transformed
 *       penalties (Eizenga and Paten) are x' = 2 (a + x), o' = 2 o, e' = 2 e + a, and max(x', o' + e') <= AIM_EXTEND_MAX_UNIT.
 *       Sides. q_begin, q_end are the slot's aim_segment_t, seg_start = d_seg_text_pos[slot] & ~AIM_REF_MINUS_STRAND, minus is its
 *       bit 63, text_len = d_seg_requests[slot].text_len, L = d_read_len[r] clamped to 0..read_size. Side 0 is the read's left, side
 *       1 its right. A side is run when the segment has AIM_SEG_VALID and not AIM_SEG_LOOSE, the side is not open, the record is
 *       well-formed (q_begin <= q_end <= L, 0 <= text_len <= read_size, seg_start + text_len <= ref_len) and n > 0 and m > 0 below;
 *       the outputs of every other side are zero.
 *       Right: Q = read[q_end, min(L, q_end + max_ext)). Left: Q = reverse(read[max(0, q_begin - max_ext), q_begin)). n = |Q|.
 *       The reference side runs up when (side is right) != minus. m = min(n + band, room, (read_size - text_len) / inner) with
 *       room = ref_len - (seg_start + text_len) up and seg_start down, and inner the number of sides of the segment that are not
 *       open (1 or 2; the division rounds down). Up: T = ref[seg_start + text_len, ... + m). Down: T = reverse(ref[seg_start - m,
 *       seg_start)). T is complemented with AIM_FLAG_REF_TEXTS' table when minus. Bases match when their bytes are equal.
 *       Cost. D(v, h) is the minimum gap-affine cost (match 0, mismatch x', a gap of g bases o' + g e'; a gap in the read next to
 *       one in the reference opens twice) of aligning Q[0, v) with T[0, h) through cells with |h - v| <= band only; D(0, 0) = 0.
 *       S(v, h) = (a (v + h) - D(v, h)) / 2, always an integer, is the best score of that prefix pair with match +a, mismatch -x and
 *       a gap of g bases -(o + g e).
 *       Stop level. For s = 0, 1, 2, ...: R(s) = max{v + h : D <= s} and B(s) = max{a (v + h) - D : D <= s}. s* is the first s with
 *       a R(s) - s < B(s) - 2 Z, or max_cost if there is none up to max_cost. (No cell of a cost above s can score within Z of the
 *       best any more.)
 *       Result. The cell with D <= s* of the greatest a (v + h) - D; among equals the smallest D, then the smallest h - v; (0, 0)
 *       when no cell is positive. dq = v, dr = h, score = S(v, h), stop = s* (stop is also written when the result is (0, 0)).
 *   11c, part 2: apply. For a slot with a non-zero (dq, dr) on either side: q_begin -= dq[0], q_end += dq[1]; the reference bound of
 *       the side that ran up moves up by that side's dr (seg_end), the other one down (seg_start); pattern_len = q_end - q_begin,
 *       text_len = seg_end - seg_start (part 1's budget keeps it <= read_size), d_seg_text_pos = seg_start | minus << 63;
 *       aim_segment_t.flags gains AIM_SEG_EXT_LEFT / AIM_SEG_EXT_RIGHT for the sides that moved; the pattern row becomes
 *       read[q_begin, q_end) as given, read from d_reads, then zero bytes up to read_size. Every other slot keeps every byte: a
 *       single-primary read, a secondary, an empty slot. An extended inner side gets no flank: it ends on a match.
 *   d_ext[slot] holds both sides' (dq, dr, stop, score), zero for a side that was not run; pad is zero.
 * aim_extend_segments_device only enqueues work on hip_stream (extend_sides_kernel, then extend_apply_kernel; csrc/extend.hpp),
 * allocates nothing and needs no scratch. Alignment of the buffers as for aim_split_segments_device; d_ext is 8-byte aligned;
 * d_reference holds ref_len bytes. AIM_EINVAL with a message under the entry point's name, before any device query, in this order:
 * the K, read_size and n_reads * K refusals of aim_split_segments_device, a NULL p and each parameter bound in the order above, a
 * ref_len above AIM_SEED_MAX_REF_LEN and, last of all, a NULL device buffer.
 * Not in this version: a stage inside aim_set_submit or host.c (aim_mapper_t below runs it), trimming the overlap of neighbouring
 * extended segments, a band above 31, max_ext above 1024, extending open sides, Z-drop. Check aim_features() & AIM_FEATURE_EXTEND first. */
#define AIM_SEG_EXT_LEFT 0x20u
#define AIM_SEG_EXT_RIGHT 0x40u
#define AIM_EXTEND_MAX_UNIT 64
#define AIM_EXTEND_MAX_COST 4095
#define AIM_EXTEND_MAX_BAND 31
#define AIM_EXTEND_MAX_EXT 1024
typedef struct aim_extend_params {
    int32_t match, mismatch, gap_o, gap_e;   /* a, x, o, e of the score S */
    int32_t xdrop;                           /* Z */
    int32_t max_cost, band, max_ext;
} aim_extend_params_t; /* 32 B */
typedef struct aim_extend {
    uint16_t dq[2], dr[2], stop[2], pad[2];  /* index 0: read-left side, 1: read-right side */
    int32_t score[2];
} aim_extend_t;        /* 24 B per slot */
int aim_extend_segments_device(const aim_extend_params_t *p, uint32_t K, uint32_t read_size, uint64_t ref_len, uint32_t n_reads,
                               const int32_t *d_read_len, const char *d_reads, const char *d_reference,
                               void *d_seg_requests /* in/out */, uint64_t *d_seg_text_pos /* in/out */,
                               char *d_seg_patterns /* in/out */, aim_segment_t *d_seg /* in/out */,
                               aim_extend_t *d_ext /* [n_reads * K] */, void *hip_stream);
/* "extend_sides_kernel,extend_apply_kernel": comma-separated rocprofv3 kernel-trace name prefixes of the entry point's kernels. */
const char *aim_extend_kernel_names(void);

/* ---- the mapper (AIM_FEATURE_MAPPER): reads in, a dense list of SAM-ready records per read out -------------------------------
 * The split path above ends in n_reads * K slot-shaped rows, most of them empty or secondary, without MAPQ and without a word on
 * which rows belong to one read. Rule 12c turns them into the list a SAM writer walks, and aim_mapper_t runs the whole sequence
 *     chain -> aim_chain_classify_device -> aim_split_segments_device -> [aim_extend_segments_device] -> aim_align_device_ref ->
 *     aim_sam_device_split -> aim_map_records_device
 * on buffers it owns, one stream per slot, and sends back exactly the records, their offsets and the CIGAR words and MD bytes in use.
 *   12c. Records (aim_map_records_device). d_seg, d_sam (the rows of aim_sam_device_split with d_sel = NULL) and d_class are indexed by
 *       slot = r * K + i. Everything is deterministic and independent of the grid and of the AIM_DEBUG_POISON_* knobs.
 *       Mapped slot. Slot r * K + i is mapped when d_seg[slot].flags & AIM_SEG_VALID is set and d_sam[slot].flags & AIM_SAM_UNMAPPED
 *       is not. A row with AIM_SAM_OVERFLOW in its status counts as mapped: the status says why it has no words.
 *       Count. c_r is the number of mapped slots of read r, or 1 if there are none. d_rec_offsets[n_reads + 1] is the exclusive prefix
 *       sum of c_r, so d_rec_offsets[n_reads] is the number of records; the records of read r are
 *       d_records[d_rec_offsets[r], d_rec_offsets[r + 1]). There are at most n_reads * K records.
 *       Order. The mapped slots of a read are sorted by (q_begin, i) ascending -- the order of the segments along the read as given;
 *       rank is a slot's position in that order, and its record is d_records[d_rec_offsets[r] + rank].
 *       Representative. The mapped slot of lowest i loses AIM_SAM_SUPPLEMENTARY if it has it, every other mapped slot gains it: a
 *       mapped read has exactly one non-supplementary line, also when candidate 0 came back over the cap.
 *       Record. aim_map_record_t, 64 bytes: sam is the slot's aim_sam_t verbatim except for the flag change above (cigar_offset and
 *       md_offset still address the buffers aim_sam_device_split wrote); read = r; q_begin, q_end and seg_flags are d_seg[slot]'s;
 *       mapq = d_class[slot].mapq; rank as above; n_records = c_r; slot = r * K + i.
 *       MAPQ. The record's mapq is rule 8c's chain MAPQ of that primary. That is this project's own rule: it comes from the chains
 *       alone, not from the alignment scores, and it is not minimap2's or BWA's figure.
 *       Unmapped read. A read without a mapped slot gets one record: d_sam[r * K] with flags = AIM_SAM_UNMAPPED and pos, ref_span, nm,
 *       n_cigar, md_len, cigar_offset and md_offset zero; idx, score, status and pad are kept; read = r, slot = r * K, n_records = 1
 *       and q_begin, q_end, mapq, seg_flags and rank zero.
 *   aim_map_records_device only enqueues work on hip_stream: map_count_kernel, the three launches of the index's scan over
 *       d_rec_offsets, map_records_kernel (csrc/mapper.hpp). It allocates nothing; d_scratch holds aim_map_records_scratch(n_reads)
 *       bytes (the scan's part sums) and may be reused once the stream has passed. Where a record lands depends on the prefix sums
 *       alone: no atomic is involved and no workgroup waits for another. d_sam and d_records are 16-byte aligned, d_seg and d_class
 *       8-byte, d_rec_offsets and d_scratch 4-byte. n_reads = 0 writes d_rec_offsets[0] = 0 and nothing else.
 *       AIM_EINVAL with a message under the entry point's name, before any device query: K outside 1..AIM_SEED_MAX_CANDS,
 *       n_reads * K >= 2^32, a NULL d_rec_offsets, a NULL device buffer with n_reads > 0, a d_sam or d_records that is not 16-byte
 *       aligned and a scratch_bytes below aim_map_records_scratch.
 *   aim_mapper_t. aim_mapper_params_t carries every stage's parameters: seed (options must be AIM_SEED_OPT_MINIMIZERS(w); K is
 *       max_cands and read_size its read_size), max_hits (0: aim_seed_chain_device, which needs read_size <= AIM_SEED_MAX_READ_SIZE;
 *       otherwise the H of aim_seed_chain_long_device), mask_q8, extend and the option bit AIM_MAP_EXTEND that runs rule 11c, the WFA
 *       penalties and max_score of the segment alignment (the mapper sets AIM_FLAG_BACKTRACE | AIM_FLAG_ENDSFREE | AIM_FLAG_REF_TEXTS
 *       itself, with text free ends of 2 * flank), sam_options, and the sizes: max_reads per batch, slots (1..AIM_MAPPER_MAX_SLOTS),
 *       cigar_cap words and md_cap bytes per slot.
 *       aim_mapper_device_bytes reports the device memory aim_mapper_create takes at its peak (the index build's scratch included,
 *       which is released before create returns). It and aim_mapper_create refuse, with a message under their own name and before any
 *       device query, in this order: a NULL argument; the seed parameters (aim_seed_chain_device's bounds, or
 *       aim_seed_chain_long_device's with max_hits != 0; minimizers are required); mask_q8 outside 1..256; max_reads * K >= 2^32; a
 *       ref_len above AIM_SEED_MAX_REF_LEN; with AIM_MAP_EXTEND the bounds of aim_extend_params_t; the alignment's parameter rules
 *       (the penalty rule of AIM_FLAG_ENDSFREE among them); sam_options other than AIM_SAM_EQX;
 *       max_reads * K * (4 * read_size + 10) >= 2^32; unknown option bits, max_reads = 0, slots outside 1..AIM_MAPPER_MAX_SLOTS.
 *       aim_mapper_create(params, device, seq, ref_len, &m) uploads the reference with its 16-byte slack, builds the minimizer index
 *       with aim_index_build_device_minimizers, allocates every per-slot device buffer and pinned host buffer once and creates one
 *       stream per slot. aim_mapper_submit(m, slot, n_reads, read_len, reads) copies read_len[n_reads] and the ASCII rows
 *       reads[n_reads][read_size] into the slot's pinned buffers and then only enqueues work: the copies and the stages in the order
 *       above (rule 11c only with AIM_MAP_EXTEND). AIM_EINVAL for n_reads > max_reads or a NULL array with n_reads > 0, AIM_ESTATE for
 *       a slot that is still in flight. aim_mapper_wait(m, slot, &out) first makes one small copy -- the record count and the two
 *       cursors -- and then copies exactly records[n_records], rec_offsets[n_reads + 1], cigar[cigar_words] and md[md_bytes]; out's
 *       pointers are views of the slot's pinned buffers and stay valid until the slot's next submit. AIM_ESTATE when nothing is in
 *       flight on the slot.
 *       Capacity. A batch that needed more than cigar_cap words or md_cap bytes still succeeds: cigar_needed / md_needed carry what
 *       it needed, cigar_words / md_bytes what was copied (the smaller of need and capacity), and the affected records carry
 *       AIM_SAM_OVERFLOW. n_reads = 0 is a valid batch: no records, rec_offsets = {0}.
 *       The slots are independent: batches on different slots overlap, and a slot's result does not depend on what ran before it.
 * aim_mapper_kernel_names: "map_count_kernel,map_records_kernel".
 * Not in this version: a mapper stage inside aim_set_submit or host.c, more than one device per mapper
 * (references of more than one sequence: rule 13c and aim_mapper_create_contigs below; paired-end reads: rule 14c and
 * aim_mapper_set_pairing below), hard clips, trimming the overlap of neighbouring segments, packed
 * read rows (MAPQ from alignment runner-ups and secondary records: rule 16c and aim_mapper_set_secondary below). The SA tag is text and is written on the host (aim_amd/samout.py) from the records of a
 * read. Check aim_features() & AIM_FEATURE_MAPPER first. */
typedef struct aim_map_record {
    aim_sam_t sam;                 /* the slot's row; flags with rule 12c's supplementary bit */
    uint32_t read;                 /* r */
    uint16_t q_begin, q_end;       /* the segment's interval of the read as given */
    uint8_t mapq;                  /* the chain MAPQ of this primary (rule 8c) */
    uint8_t seg_flags;             /* AIM_SEG_* */
    uint8_t rank;                  /* position among the read's records */
    uint8_t n_records;             /* c_r */
    uint32_t slot;                 /* r * K + i */
} aim_map_record_t;    /* 64 B per record */
size_t aim_map_records_scratch(uint32_t n_reads);
int aim_map_records_device(uint32_t K, uint32_t n_reads, const aim_segment_t *d_seg, const aim_sam_t *d_sam, const aim_chain_class_t *d_class,
                           uint32_t *d_rec_offsets /* [n_reads + 1] */, aim_map_record_t *d_records /* [n_reads * K] */, void *d_scratch,
                           size_t scratch_bytes, void *hip_stream);
/* Comma-separated rocprofv3 kernel-trace name prefixes of the two kernels rule 12c adds. */
const char *aim_mapper_kernel_names(void);
#define AIM_MAP_EXTEND 0x1u        /* aim_mapper_params_t.options: run aim_extend_segments_device between split and alignment */
#define AIM_MAPPER_MAX_SLOTS 4
typedef struct aim_mapper_params {
    aim_seed_params_t seed;
    uint32_t max_hits;             /* 0: aim_seed_chain_device; otherwise the H of aim_seed_chain_long_device */
    uint32_t mask_q8;              /* rule 8c; AIM_CHAIN_MASK_DEFAULT */
    aim_extend_params_t extend;    /* read with AIM_MAP_EXTEND only */
    uint32_t options;              /* AIM_MAP_EXTEND */
    int32_t match, mismatch, gap_o, gap_e, max_score;   /* the WFA segment alignment */
    uint32_t sam_options;          /* AIM_SAM_EQX */
    uint32_t max_reads;            /* reads per batch */
    uint32_t slots;                /* 1..AIM_MAPPER_MAX_SLOTS */
    uint32_t cigar_cap, md_cap;    /* CIGAR words and MD bytes per slot */
} aim_mapper_params_t; /* 124 B */
typedef struct aim_mapper aim_mapper_t;
typedef struct aim_mapper_out {
    uint32_t n_reads, n_records;
    uint32_t cigar_words, md_bytes;      /* copied: min(needed, capacity) */
    uint32_t cigar_needed, md_needed;    /* what the batch needed */
    const aim_map_record_t *records;     /* [n_records] */
    const uint32_t *rec_offsets;         /* [n_reads + 1] */
    const uint32_t *cigar;               /* [cigar_words] */
    const char *md;                      /* [md_bytes] */
} aim_mapper_out_t;
int aim_mapper_device_bytes(const aim_mapper_params_t *params, uint64_t ref_len, uint64_t *bytes);
int aim_mapper_create(const aim_mapper_params_t *params, int device, const char *seq, uint64_t ref_len, aim_mapper_t **mapper);
int aim_mapper_submit(aim_mapper_t *mapper, uint32_t slot, uint32_t n_reads, const int32_t *read_len, const char *reads);
int aim_mapper_wait(aim_mapper_t *mapper, uint32_t slot, aim_mapper_out_t *out);
int aim_mapper_free(aim_mapper_t *mapper);

/* ---- references of several sequences (AIM_FEATURE_CONTIGS): contig table, edge clipping, the contig in the record ---------------
 * The index, the chains and the alignment work on one sequence of positions. A reference of several sequences (contigs) becomes one
 * by concatenation, and rule 13c says what the concatenation looks like, how a segment's window is kept inside the contig it belongs
 * to, and how a record names its contig. No other stage changes.
 *   13c. Layout (aim_contigs_layout, aim_contigs_concat; host only). Contig c of lens[c] bases starts at starts[c]: starts[0] = 0,
 *       starts[c + 1] = starts[c] + lens[c] + spacer, and ref_len = starts[n - 1] + lens[n - 1]. The spacer bases between two
 *       contigs are 'N': an 'N' is not A, C, G or T, so no k-mer and no minimizer spans two contigs. AIM_CONTIG_SPACER(band) =
 *       band + 64 is the spacer aim_mapper_create_contigs uses: two anchors on either side of a true junction between neighbouring
 *       contigs (the read continues from the end of one into the start of the next) then differ in diagonal by more than band, so
 *       rule 4c does not link them and each side becomes a chain of its own.
 *       AIM_EINVAL names the field or the contig: n_contigs outside 1..AIM_CONTIG_MAX, a NULL array, spacer < 1, a lens[c] of 0,
 *       a ref_len above AIM_SEED_MAX_REF_LEN (the contig at which the sum passed it is named).
 *       Clip (aim_contig_clip_device). Runs behind aim_split_segments_device, and behind aim_extend_segments_device where that
 *       runs, in front of aim_align_device_ref, on every slot r * K + i whose d_seg[slot].flags has AIM_SEG_VALID:
 *         Anchor. A is rule 10c's recovered p_lo of the candidate, from d_requests[slot], d_text_pos[slot], d_chains[slot], flank
 *         and L = min(max(d_read_len[r], 0), read_size) -- the candidate's window, not the segment's --, clamped to
 *         [0, ref_len - 1]. Where the segment has AIM_SEG_LOOSE, or p_lo is not recoverable, A is the segment's start.
 *         Contig. c = max{ j : starts[j] <= A }. An anchor inside a spacer belongs to the contig in front of it.
 *         Window. With seg_start = d_seg_text_pos[slot] without the strand bit and seg_end = seg_start + d_seg_requests[slot].text_len:
 *         s' = max(seg_start, starts[c]) and e' = max(s', min(seg_end, starts[c] + lens[c])). If either bound moved,
 *         d_seg_text_pos[slot] = s' | strand bit, text_len = e' - s' and d_seg[slot].flags gains AIM_SEG_CONTIG_CLIPPED; a window
 *         wholly outside its contig ends with text_len 0. d_contig[slot] = c.
 *         Every slot without AIM_SEG_VALID keeps every byte and gets d_contig[slot] = AIM_CONTIG_NONE; a slot that is not clipped
 *         keeps every byte of the three segment buffers. The pattern rows, q_begin and q_end are never touched: read bases that lost
 *         their reference come back from the alignment as a terminal read-only run, which aim_sam_device_split folds into the soft
 *         clip, so the CIGAR's read-consuming lengths still sum to read_len and pos + ref_span stays inside the contig.
 *         Deterministic, independent of the grid and of the AIM_DEBUG_POISON_* knobs. d_contig_start and d_contig_len are
 *         uint32_t[n_contigs] on the device, as aim_contigs_layout gave them, and ref_len is its ref_len.
 *         contig_clip_kernel (csrc/contig.hpp): a slot per lane; a workgroup stages every step-th start in LDS (step = the smallest
 *         power of two with ceil(n_contigs / step) <= 1024), searches that table and finishes with at most log2(step) loads from
 *         d_contig_start. No atomics, no scratch memory; only enqueues work on hip_stream.
 *         AIM_EINVAL under the entry point's name, before any device query: K outside 1..AIM_SEED_MAX_CANDS, a read_size that is not
 *         a positive multiple of 8 up to AIM_SEED_LONG_MAX_READ_SIZE, n_reads * K >= 2^32, flank < 0, ref_len 0 or above
 *         AIM_SEED_MAX_REF_LEN, n_contigs outside 1..AIM_CONTIG_MAX, a NULL d_contig_start or d_contig_len, a NULL device buffer with
 *         n_reads > 0.
 *       Records (aim_map_records_contigs_device). Rule 12c exactly -- the same d_rec_offsets, ranks, representative, flags and MAPQ
 *       -- with two changes to a mapped record: sam.pos -= starts[c] with c = d_contig[slot], so the position is contig-local, and
 *       sam.pad = c. (A d_contig[slot] outside 0..n_contigs - 1 on a mapped slot leaves pos as it is; pad still carries it.) The one
 *       record of an unmapped read gets sam.pad = AIM_CONTIG_NONE. map_records_contig_kernel takes map_records_kernel's place;
 *       map_count_kernel and the scan are rule 12c's.
 *   Mapper. aim_mapper_create_contigs(params, device, n_contigs, seqs, lens, &m) lays the contigs out with
 *       AIM_CONTIG_SPACER(params->seed.band), concatenates them, uploads the concatenation, builds the index as aim_mapper_create
 *       does and uploads starts and lens (8 B per contig); aim_mapper_submit then runs the clip in front of the alignment and the
 *       contig record kernel at the end. aim_mapper_submit, aim_mapper_wait, aim_mapper_out_t and aim_mapper_params_t are unchanged,
 *       and a mapper made by aim_mapper_create gives the bytes it always gave (pad 0, global pos).
 *       aim_mapper_device_bytes_contigs is aim_mapper_device_bytes for such a mapper; aim_mapper_contigs returns the layout (views
 *       that live as long as the mapper; n = 0 and NULL for a mapper of one sequence).
 *       Refusals of the two, under their own name and before any device query: a NULL params, then the layout's bounds above, then
 *       every check of aim_mapper_device_bytes / aim_mapper_create on the laid-out ref_len, then a NULL seqs or seqs[c].
 * aim_contig_kernel_names: "contig_clip_kernel,map_records_contig_kernel".
 * Not in this version: an extension (rule 11c) that stops at a contig's edge -- it may claim a few read bases against the spacer,
 * which come back as soft clip --, chains confined to one contig inside the chain kernels, a contig stage inside
 * aim_set_submit or host.c (paired-end reads: rule 14c below). Check aim_features() & AIM_FEATURE_CONTIGS first. */
#define AIM_CONTIG_MAX (1u << 20)
#define AIM_CONTIG_NONE 0xFFFFFFFFu
#define AIM_CONTIG_SPACER(band) ((uint32_t)(band) + 64u)
#define AIM_SEG_CONTIG_CLIPPED 0x80u /* aim_segment_t.flags, from aim_contig_clip_device */
int aim_contigs_layout(uint32_t n_contigs, const uint32_t *lens, uint32_t spacer, uint32_t *starts /* [n_contigs] */, uint64_t *ref_len);
int aim_contigs_concat(uint32_t n_contigs, const char *const *seqs, const uint32_t *lens, uint32_t spacer, char *out /* [ref_len] */);
int aim_contig_clip_device(uint32_t K, uint32_t read_size, int32_t flank, uint64_t ref_len, uint32_t n_contigs, const uint32_t *d_contig_start,
                           const uint32_t *d_contig_len, uint32_t n_reads, const int32_t *d_read_len, const void *d_requests, const uint64_t *d_text_pos,
                           const aim_chain_t *d_chains, void *d_seg_requests, uint64_t *d_seg_text_pos, aim_segment_t *d_seg,
                           uint32_t *d_contig /* [n_reads * K] */, void *hip_stream);
int aim_map_records_contigs_device(uint32_t K, uint32_t n_reads, const aim_segment_t *d_seg, const aim_sam_t *d_sam, const aim_chain_class_t *d_class,
                                   const uint32_t *d_contig /* [n_reads * K] */, uint32_t n_contigs, const uint32_t *d_contig_start,
                                   uint32_t *d_rec_offsets /* [n_reads + 1] */, aim_map_record_t *d_records /* [n_reads * K] */, void *d_scratch,
                                   size_t scratch_bytes, void *hip_stream);
/* Comma-separated rocprofv3 kernel-trace name prefixes of the two kernels rule 13c adds. */
const char *aim_contig_kernel_names(void);
int aim_mapper_device_bytes_contigs(const aim_mapper_params_t *params, uint32_t n_contigs, const uint32_t *lens, uint64_t *bytes);
int aim_mapper_create_contigs(const aim_mapper_params_t *params, int device, uint32_t n_contigs, const char *const *seqs, const uint32_t *lens,
                              aim_mapper_t **mapper);
int aim_mapper_contigs(const aim_mapper_t *mapper, uint32_t *n_contigs, const uint32_t **starts, const uint32_t **lens);

/* ---- paired-end reads (AIM_FEATURE_PAIRED): pairing from aligned coordinates, mate rescue, the mate fields of a record -----------
 * Reads 2m and 2m + 1 of a batch are mates, so n_reads is even. Rule 14c works on the slot arrays as they stand after
 * aim_sam_device_split -- d_seg, d_sam, d_class, d_read_len, and d_contig (NULL for one sequence) -- between that stage and the record
 * kernel, and once more behind the record kernel. Mapped slot and representative are rule 12c's. Positions are the global ones of
 * d_sam; the record kernel still makes them contig-local. All arithmetic is signed 64-bit; everything is deterministic and
 * independent of the grid and of the AIM_DEBUG_POISON_* knobs.
 *   14c. Proper combination (i, j). Slot i of read 2m and slot j of read 2m + 1 are both mapped, lie on the same contig (d_contig
 *       equal, when given) and differ in AIM_SAM_REVERSE; with f the forward and r the reverse of the two records, pos_f <= pos_r and
 *       min_span <= pos_r + ref_span_r - pos_f <= max_span. That figure is the combination's span. Its cost is score_i + score_j,
 *       summed in 64 bits and clamped to INT32_MAX - 1.
 *       Rescue rows (aim_pair_rescue_rows_device). One row per read b, with mate a = b ^ 1. The rescue is TRIED when options has
 *       AIM_PAIR_RESCUE, read a has a mapped slot, no proper combination exists among the mapped slots of the two reads and
 *       L = min(max(d_read_len[b], 0), read_size) > 0. The anchor A is a's representative with P = pos, S = ref_span and the bounds
 *       [c_lo, c_hi) of its contig d_contig[A] (for one sequence, or a d_contig[A] outside the table, [0, ref_len)).
 *         A forward: lo = max(P + min_span - L, c_lo), hi = min(P + max_span, c_hi), and the window's strand bit is set.
 *         A reverse: with E = P + S, lo = max(E - max_span, c_lo), hi = min(E - min_span + L, c_hi), strand 0.
 *       If hi - lo >= L the row is d_res_requests[b] = {pattern_len L, text_len hi - lo, 0, idx b} with d_res_text_pos[b] =
 *       lo | strand bit, and the first read_size bytes of pattern row b (d_res_patterns + b * rescue_size) become read b's row; the
 *       bytes behind them are never written and never interpreted. Otherwise, and for every read that is not tried, the row is
 *       the EMPTY ROW {0, 0, 0, b} with text_pos 0, and its pattern row is not written. An empty row aligns to an empty ops range, so
 *       aim_sam_device gives it AIM_SAM_UNMAPPED with pos 0 (the unmapped rule of AIM_FLAG_SAM_FIELDS): rows that were not tried
 *       need no mark of their own. hi - lo <= max_span - min_span + read_size <= rescue_size.
 *       The rows are aligned by aim_align_device_ref with AIM_FLAG_BACKTRACE | AIM_FLAG_ENDSFREE | AIM_FLAG_REF_TEXTS, read_size =
 *       rescue_size, pattern free ends 0 / 0 and text free ends rescue_size / rescue_size, and aim_sam_device turns them into
 *       d_res_sam[n_reads] with CIGAR / MD buffers of their own. No alignment kernel is added.
 *       Choice (aim_pair_select_device). The combinations run over the mapped slots plus index K for a read's rescue row where that
 *       row was tried and d_res_sam[b] is not AIM_SAM_UNMAPPED (AIM_SAM_OVERFLOW counts as mapped, as in rule 12c). The rescue row's
 *       contig is its anchor's. (K, K) is excluded. The proper combination of lowest cost wins, ties going to the lowest i and then
 *       the lowest j; n_best counts the proper combinations of that cost and second_sum is the lowest cost among the other
 *       proper combinations (with a tie the cost itself; INT32_MAX: none), as in aim_mate_t. The unpaired cost is score(rep_a) + score(rep_b) + unpaired_penalty, clamped alike;
 *       it exists only when both reads have a mapped slot. The proper combination is taken if there is no unpaired cost or its
 *       cost <= the unpaired cost.
 *       aim_map_pair_t. Taken: slot[] = the two chosen slots, 2m * K + i and (2m + 1) * K + j, so r * K + K names read r's rescue
 *       row; score_sum, second_sum and n_best as above; span; flags has AIM_PAIR_PROPER, plus AIM_PAIR_RESCUED_A / _B where index
 *       K was chosen for read 2m / 2m + 1. Not taken: slot[] = the representatives (UINT32_MAX: the read has no mapped slot), n_best
 *       0, span 0, score_sum = the unpaired cost and second_sum = the best proper cost or INT32_MAX; without an unpaired cost both
 *       are INT32_MAX. AIM_PAIR_RESCUE_TRIED_A / _B say for which read the rescue was tried, taken or not.
 *       Apply (inside aim_pair_select_device). Where read b's rescue row is in the combination taken, it is folded into the slot
 *       arrays in place, so rules 12c / 13c run unchanged behind it: d_sam[b * K] = d_res_sam[b] with cigar_offset += cigar_base and
 *       md_offset += md_base; d_seg[b * K] = {0, L, L, AIM_SEG_VALID | AIM_SEG_LEFT_OPEN | AIM_SEG_RIGHT_OPEN, 0}; b's other slots
 *       lose AIM_SEG_VALID and keep every other bit; d_contig[b * K] = the anchor's contig (when d_contig is given); the mapq byte
 *       of d_class[b * K] becomes that of the anchor's slot. The placement a rescued read had before -- a discordant one, by the
 *       condition for trying -- is dropped: it gives no record. Every other byte of the slot arrays stays.
 *       Mate fields (aim_map_mates_device). Runs behind aim_map_records_device / aim_map_records_contigs_device on the same slot
 *       arrays, one record per lane. A record of read r takes its mate's REFERENCE RECORD: the mate's chosen slot if the pair is
 *       proper (a chosen rescue row lies in slot r * K since apply), else the mate's representative. d_records[..].sam.flags gains
 *       0x1 always, 0x40 for even r and 0x80 for odd r, 0x8 when the mate has no mapped slot, 0x20 when the mate's reference
 *       record has AIM_SAM_REVERSE, and 0x2 on the records of the two chosen slots of a proper pair. aim_map_mate_t[rec]:
 *       mate_pos and mate_contig are the reference record's pos and contig, in the record's own convention (with d_contig:
 *       pos - starts[c] and c; for one sequence the global pos and 0); tlen is +min(span, INT32_MAX) on the forward chosen record of a
 *       proper pair, minus that on the reverse one and 0 everywhere else. With an unmapped mate, mate_pos / mate_contig are the
 *       record's own sam.pos / sam.pad (0 for one sequence); with both reads unmapped they are 0 / AIM_CONTIG_NONE (0 / 0 for one
 *       sequence). No other byte of a record changes.
 *   The three entry points only enqueue work on hip_stream and allocate nothing: pair_rescue_rows_kernel, pair_select_kernel and
 *       map_mates_kernel (csrc/pair.hpp); the first two give a read pair 4, 8 or 16 lanes by K. No LDS, no scratch memory, no atomics.
 *       d_sam, d_res_sam, d_res_requests, d_pairs, d_records and d_mates are 16-byte aligned, d_reads, d_res_patterns, d_seg, d_class
 *       and d_res_text_pos 8-byte. d_res_sam may be NULL without AIM_PAIR_RESCUE. n_reads = 0 enqueues nothing.
 *       AIM_EINVAL under the entry point's name, before any device query: a NULL params; unknown option bits; an odd n_reads; K
 *       outside 1..AIM_SEED_MAX_CANDS; n_reads * (K + 1) >= 2^32; min_span < 0, max_span < min_span or max_span >= 2^62; a negative
 *       unpaired_penalty; a read_size that is not a positive multiple of 8 up to AIM_SEED_LONG_MAX_READ_SIZE; with AIM_PAIR_RESCUE (and
 *       always from aim_pair_rescue_rows_device) a rescue_size that is not a multiple of 8, rescue_size < read_size or
 *       max_span - min_span + read_size > rescue_size; ref_len 0 or above AIM_SEED_MAX_REF_LEN and, with d_contig, n_contigs outside
 *       1..AIM_CONTIG_MAX or a NULL table; a NULL buffer with n_reads > 0; a buffer that breaks its alignment (the message names it).
 *   Mapper. aim_mapper_set_pairing(m, &pp) switches rule 14c on for a mapper of either kind. It is legal once and only while no
 *       slot is in flight (AIM_ESTATE otherwise); it allocates the extra per-slot buffers -- aim_mapper_pairing_device_bytes says how
 *       much device memory that is, for all slots -- and moves each slot's CIGAR and MD buffers to ones that hold the rescue regions
 *       behind the main ones: cigar_base = cigar_cap, md_base = md_cap, rescue_cigar_cap words and rescue_md_cap bytes, in the same
 *       device and pinned buffers, so out->cigar[cigar_offset] and out->md[md_offset] address a rescued record like any other.
 *       Its refusals are the ones above with K and read_size the mapper's, then the alignment's parameter rules at read_size =
 *       rescue_size, then (cigar_cap + rescue_cigar_cap) or (md_cap + rescue_md_cap) >= 2^32.
 *       aim_mapper_submit then refuses an odd n_reads and enqueues, behind aim_sam_device_split: the rescue rows, their alignment
 *       and their records (the three only with AIM_PAIR_RESCUE), select / apply, the record kernel, the mate fields.
 *       aim_mapper_wait copies the rescue regions by a cursor pair of their own, and mates[n_records] and pairs[n_reads / 2];
 *       aim_mapper_out_t is unchanged (cigar_words / md_bytes / *_needed speak of the main regions). aim_mapper_pairs(m, slot, &po)
 *       gives the views of the last batch waited for on the slot, valid until the slot's next submit; AIM_ESTATE without
 *       aim_mapper_set_pairing, before the first wait and while the slot is in flight. A rescue region that was too small leaves
 *       AIM_SAM_OVERFLOW on the rescued records and rescue_*_needed above rescue_*_words / _bytes.
 *       A mapper on which aim_mapper_set_pairing was never called gives the bytes it always gave.
 * aim_pair_kernel_names: "pair_rescue_rows_kernel,pair_select_kernel,map_mates_kernel".
 * Not in this version (a pair MAPQ: rule 17c below; the span bounds estimated from the data: rule 15c below): rescue against anchors other than the representative,
 * keeping a rescued read's discordant placement as a secondary line, mates that overlap so far that pos_r < pos_f, pairing inside
 * aim_set_submit or host.c, AIM_FLAG_TOP_HITS rows. Check aim_features() & AIM_FEATURE_PAIRED first. */
#define AIM_PAIR_RESCUE 0x1u            /* aim_map_pair_params_t.options: try the mate rescue */
#define AIM_PAIR_PROPER 0x1u            /* aim_map_pair_t.flags */
#define AIM_PAIR_RESCUE_TRIED_A 0x2u
#define AIM_PAIR_RESCUE_TRIED_B 0x4u
#define AIM_PAIR_RESCUED_A 0x8u
#define AIM_PAIR_RESCUED_B 0x10u
typedef struct aim_map_pair_params {
    int64_t min_span, max_span;    /* 0 <= min_span <= max_span < 2^62, in aligned coordinates */
    int32_t unpaired_penalty;      /* >= 0 */
    uint32_t options;              /* AIM_PAIR_RESCUE */
    uint32_t rescue_size;          /* read_size of the rescue alignment: a multiple of 8, >= max_span - min_span + read_size */
    uint32_t rescue_cigar_cap, rescue_md_cap;   /* the mapper's rescue regions, words and bytes per slot; the entry points ignore them */
    uint32_t pad;                  /* 0 */
} aim_map_pair_params_t; /* 40 B */
typedef struct aim_map_pair {      /* 32 B, one per read pair m */
    uint32_t slot[2];              /* the chosen slot of read 2m / 2m + 1; r * K + K: its rescue row; UINT32_MAX: no mapped slot */
    int32_t score_sum;             /* cost of the choice; INT32_MAX when a read has no mapped slot and the choice is not proper */
    int32_t second_sum;            /* lowest cost among the OTHER proper combinations; INT32_MAX when there is none */
    uint32_t n_best;               /* proper combinations of cost score_sum (0 when the choice is not proper) */
    uint32_t flags;                /* AIM_PAIR_* */
    int64_t span;                  /* pos_r + ref_span_r - pos_f of the choice; 0 when it is not proper */
} aim_map_pair_t;
typedef struct aim_map_mate {      /* 16 B, one per record */
    uint64_t mate_pos;
    int32_t tlen;
    uint32_t mate_contig;
} aim_map_mate_t;
typedef struct aim_mapper_pairs_out {
    uint32_t n_pairs, n_records;
    uint32_t rescue_cigar_words, rescue_md_bytes;     /* copied: min(needed, capacity); they start at cigar[cigar_cap] / md[md_cap] */
    uint32_t rescue_cigar_needed, rescue_md_needed;
    const aim_map_mate_t *mates;         /* [n_records], record by record */
    const aim_map_pair_t *pairs;         /* [n_pairs] */
} aim_mapper_pairs_out_t;
int aim_pair_rescue_rows_device(const aim_map_pair_params_t *pp, uint32_t K, uint32_t read_size, uint64_t ref_len, uint32_t n_contigs,
                                const uint32_t *d_contig_start, const uint32_t *d_contig_len, uint32_t n_reads, const int32_t *d_read_len,
                                const char *d_reads, const aim_segment_t *d_seg, const aim_sam_t *d_sam, const uint32_t *d_contig_or_null,
                                void *d_res_requests /* aim_request_t[n_reads] */, uint64_t *d_res_text_pos /* [n_reads] */,
                                char *d_res_patterns /* [n_reads][rescue_size] */, void *hip_stream);
int aim_pair_select_device(const aim_map_pair_params_t *pp, uint32_t K, uint32_t read_size, uint32_t n_reads, const int32_t *d_read_len,
                           aim_segment_t *d_seg, aim_sam_t *d_sam, aim_chain_class_t *d_class, uint32_t *d_contig_or_null,
                           const aim_sam_t *d_res_sam /* [n_reads]; may be NULL without AIM_PAIR_RESCUE */, uint32_t cigar_base, uint32_t md_base,
                           aim_map_pair_t *d_pairs /* [n_reads / 2] */, void *hip_stream);
int aim_map_mates_device(uint32_t K, uint32_t n_reads, const aim_map_pair_t *d_pairs, const aim_segment_t *d_seg, const aim_sam_t *d_sam,
                         const uint32_t *d_contig_or_null, uint32_t n_contigs, const uint32_t *d_contig_start, const uint32_t *d_rec_offsets,
                         aim_map_record_t *d_records, aim_map_mate_t *d_mates /* [n_reads * K] */, void *hip_stream);
/* Comma-separated rocprofv3 kernel-trace name prefixes of the three kernels rule 14c adds. */
const char *aim_pair_kernel_names(void);
int aim_mapper_pairing_device_bytes(const aim_mapper_params_t *params, const aim_map_pair_params_t *pp, uint64_t *bytes);
int aim_mapper_set_pairing(aim_mapper_t *mapper, const aim_map_pair_params_t *pp);
int aim_mapper_pairs(aim_mapper_t *mapper, uint32_t slot, aim_mapper_pairs_out_t *out);

/* ---- the span bounds of rule 14c estimated from the batch (AIM_FEATURE_PAIR_ESTIMATE) ---------------------------------------------
 * min_span and max_span decide what rule 14c calls proper, which mates it rescues and where; a caller who does not know the library's
 * fragment lengths has to guess them. Most read pairs of a batch place both mates uniquely, and their spans are the fragment lengths.
 * Rule 15c reads them off the slot arrays as they stand after aim_sam_device_split -- d_seg, d_sam, d_class and d_contig (NULL for one
 * sequence), in front of aim_pair_rescue_rows_device -- and leaves the bounds in device memory, where the two kernels of rule 14c read
 * them: no round trip through the host, and nothing is carried from one batch to the next. All arithmetic is signed 64-bit and
 * integer only; the result is deterministic and independent of the grid and of the AIM_DEBUG_POISON_* knobs.
 *   15c. Sample. Read pair m = (2m, 2m + 1) is a SAMPLE when each of the two reads has exactly one mapped slot (rule 12c's: the read
 *       is neither unmapped nor split), d_class[slot].mapq >= min_mapq for both, the two slots lie on the same contig (d_contig equal,
 *       when given), they differ in AIM_SAM_REVERSE and, with f the forward and r the reverse record, pos_f <= pos_r. Its value is
 *       rule 14c's span, pos_r + ref_span_r - pos_f. A sample with span < hist_size is binned at its span and n_samples counts these;
 *       a sample with span >= hist_size counts in n_beyond and is otherwise ignored.
 *       Quartiles. cum(s) is the number of binned samples with span <= s. p_q is the smallest s with 4 * cum(s) >= q * n_samples, for
 *       q = 1, 2, 3: p25, p50, p75. All three are 0 when n_samples == 0.
 *       Bounds. IQR = p75 - p25, slack = max(3 * IQR, min_slack), lo = max(p25 - slack, 0), hi = p75 + slack.
 *         AIM_PAIR_EST_FLOORED: the max(.., 0) in lo = max(p25 - slack, 0) changed lo.
 *         AIM_PAIR_EST_CLAMPED: with AIM_PAIR_RESCUE and W = rescue_size - read_size, when hi - lo > W: lo = max(p50 - W / 2, 0) and
 *           hi = lo + W. This keeps rule 14c's invariant hi - lo + read_size <= rescue_size for bounds the host never sees.
 *         AIM_PAIR_EST_FALLBACK: when n_samples < min_samples, lo = pp->min_span and hi = pp->max_span, and no other flag is set.
 *       Output. aim_pair_estimate_t in device memory, 48 bytes, 16-byte aligned: min_span = lo, max_span = hi, the counts, the
 *       quartiles, the flags, and two pad words of 0.
 *       Use. aim_pair_rescue_rows_device_est and aim_pair_select_device_est are aim_pair_rescue_rows_device and aim_pair_select_device
 *       of rule 14c word for word, with min_span and max_span read from d_est by the kernel. pp's own bounds are the fallback alone and
 *       still have to pass rule 14c's checks; d_est is 16-byte aligned and may be NULL only with n_reads = 0.
 *   aim_pair_estimate_device enqueues on hip_stream, allocating nothing: the clear of d_scratch (so the scratch may hold anything),
 *       pair_span_hist_kernel and pair_span_bounds_kernel (csrc/pair_estimate.hpp). The first gives a read pair 4, 8 or 16 lanes by K
 *       like rule 14c's kernels and counts into a histogram in LDS of its workgroup (4 * (hist_size + 1) bytes), whose non-zero bins
 *       it adds to the one in d_scratch; those integer adds are the only atomics, and a sum does not depend on the order of its terms.
 *       The second is one workgroup. aim_pair_estimate_scratch(hist_size) = 4 * hist_size + 16 bytes. n_reads = 0 writes the fallback
 *       estimate with every count 0 (into a d_est that is not NULL; the other buffers may be NULL then).
 *       AIM_EINVAL under the entry point's name, before any device query: every check of rule 14c on pp, K, read_size and n_reads; a
 *       NULL aim_pair_est_params_t; hist_size outside 64..AIM_PAIR_EST_MAX_HIST or not a multiple of 64; min_samples 0; min_mapq above
 *       60; a NULL buffer with n_reads > 0; a d_est that is not 16-byte aligned (d_sam 16, d_seg and d_class 8, d_scratch 4);
 *       scratch_bytes below aim_pair_estimate_scratch(hist_size).
 *   Mapper. aim_mapper_set_pairing_estimated(m, &pp, &ep) is aim_mapper_set_pairing plus the estimate: the same state rules, its
 *       refusals followed by ep's. Per slot it allocates, on the device, up256(48) + up256(aim_pair_estimate_scratch(hist_size)) bytes
 *       more than aim_mapper_pairing_device_bytes reports per slot (up256: rounded up to a multiple of 256); that function is unchanged.
 *       aim_mapper_submit enqueues the estimate behind aim_sam_device_split and calls the _est variants in place of rule 14c's two;
 *       aim_mapper_wait copies the 48 bytes together with its first small copy. aim_mapper_pair_estimate(m, slot, &e) gives the
 *       estimate of the last batch waited for on the slot (for an empty batch: the fallback with every count 0); AIM_ESTATE before the
 *       first wait, while the slot is in flight, and on a mapper without estimation. A mapper paired with aim_mapper_set_pairing, or not
 *       paired at all, keeps its buffers and every byte it gave before.
 * aim_pair_estimate_kernel_names: "pair_span_hist_kernel,pair_span_bounds_kernel,pair_rescue_rows_est_kernel,pair_select_est_kernel".
 * Not in this version: a pair MAPQ, orientations other than forward / reverse, bins wider than one base or spans of
 * AIM_PAIR_EST_MAX_HIST and more, an estimate carried across batches, compaction of the rescue rows. Check aim_features() &
 * AIM_FEATURE_PAIR_ESTIMATE first. */
#define AIM_PAIR_EST_MAX_HIST 8192u
#define AIM_PAIR_EST_FALLBACK 0x1u      /* aim_pair_estimate_t.flags */
#define AIM_PAIR_EST_CLAMPED 0x2u
#define AIM_PAIR_EST_FLOORED 0x4u
typedef struct aim_pair_est_params {
    uint32_t hist_size;            /* bins of one base: 64..AIM_PAIR_EST_MAX_HIST, a multiple of 64 */
    uint32_t min_samples;          /* >= 1: fewer binned samples give the fallback */
    uint32_t min_mapq;             /* 0..60 */
    uint32_t min_slack;            /* a floor for the spread 3 * IQR */
} aim_pair_est_params_t; /* 16 B */
typedef struct aim_pair_estimate {
    int64_t min_span, max_span;    /* lo and hi */
    uint32_t n_samples, n_beyond, p25, p50, p75;
    uint32_t flags;                /* AIM_PAIR_EST_* */
    uint32_t pad[2];               /* 0 */
} aim_pair_estimate_t; /* 48 B, 16-byte aligned in device memory */
size_t aim_pair_estimate_scratch(uint32_t hist_size);   /* 4 * hist_size + 16 */
int aim_pair_estimate_device(const aim_map_pair_params_t *pp, const aim_pair_est_params_t *ep, uint32_t K, uint32_t read_size, uint32_t n_reads,
                             const aim_segment_t *d_seg, const aim_sam_t *d_sam, const aim_chain_class_t *d_class, const uint32_t *d_contig_or_null,
                             aim_pair_estimate_t *d_est, void *d_scratch, size_t scratch_bytes, void *hip_stream);
int aim_pair_rescue_rows_device_est(const aim_map_pair_params_t *pp, uint32_t K, uint32_t read_size, uint64_t ref_len, uint32_t n_contigs,
                                    const uint32_t *d_contig_start, const uint32_t *d_contig_len, uint32_t n_reads, const int32_t *d_read_len,
                                    const char *d_reads, const aim_segment_t *d_seg, const aim_sam_t *d_sam, const uint32_t *d_contig_or_null,
                                    void *d_res_requests, uint64_t *d_res_text_pos, char *d_res_patterns, const aim_pair_estimate_t *d_est,
                                    void *hip_stream);
int aim_pair_select_device_est(const aim_map_pair_params_t *pp, uint32_t K, uint32_t read_size, uint32_t n_reads, const int32_t *d_read_len,
                               aim_segment_t *d_seg, aim_sam_t *d_sam, aim_chain_class_t *d_class, uint32_t *d_contig_or_null,
                               const aim_sam_t *d_res_sam, uint32_t cigar_base, uint32_t md_base, aim_map_pair_t *d_pairs,
                               const aim_pair_estimate_t *d_est, void *hip_stream);
/* Comma-separated rocprofv3 kernel-trace name prefixes of the four kernels rule 15c adds. */
const char *aim_pair_estimate_kernel_names(void);
int aim_mapper_set_pairing_estimated(aim_mapper_t *mapper, const aim_map_pair_params_t *pp, const aim_pair_est_params_t *ep);
int aim_mapper_pair_estimate(aim_mapper_t *mapper, uint32_t slot, aim_pair_estimate_t *out);

/* ---- aligned secondaries (AIM_FEATURE_SECONDARY): the best copy of a repeat by alignment, MAPQ from the runner-up, 0x100 records ----
 * Rules 8c, 10c and 12c decide from the chains alone which copy of a repeat a read belongs to: the primary of a locus is the chain of
 * highest score (the lowest position among equals), only primaries get a row, and the record carries the chain MAPQ. A read from a
 * diverged repeat whose chains tie therefore comes back on whichever copy lies first, with MAPQ 0. Rule 16c aligns the secondaries of
 * a locus over the same read interval as their primary, lets the alignment scores choose the locus' one record, derives its MAPQ from
 * the runner-up, and can report the other copies as SAM secondary records. The sequence is
 *     chain -> aim_chain_classify_device -> aim_split_segments_device -> [aim_extend_segments_device] -> aim_secondary_rows_device ->
 *     [aim_contig_clip_device] -> aim_align_device_ref -> aim_sam_device_split -> aim_secondary_select_device ->
 *     aim_map_records_secondary_device.
 * All n_reads * K slot rows go through the alignment anyway, so there is no new alignment launch and no new row buffer: a secondary's
 * row takes the place of rule 7's empty slot. Arithmetic is signed 64-bit unless stated; every byte is deterministic and independent of
 * the grid and of the AIM_DEBUG_POISON_* knobs. A mapper that does not switch the rule on gives the bytes it always gave.
 *   16c, part 1: rows for secondaries (aim_secondary_rows_device). Works in place on the four segment buffers, behind
 *       aim_split_segments_device and, where it runs, aim_extend_segments_device. For read r: n = min(d_seed[r].n_cands, K), L =
 *       d_read_len[r] clamped to 0..read_size. Candidate i < n is a secondary when d_class[slot].flags & (AIM_CHAIN_PRIMARY |
 *       AIM_CHAIN_SECONDARY) is AIM_CHAIN_SECONDARY alone, its parent is j = d_class[slot].parent (rule 8c), and t is its index among
 *       the secondaries of the read with the same parent, in candidate order. It gets a row when all of these hold: t < max_sec;
 *       j < n and candidate j carries AIM_CHAIN_PRIMARY alone of the two flags; d_seg[r * K + j] has AIM_SEG_VALID and is well-formed
 *       (q_begin <= q_end <= L); rule 10c's p_lo of candidate i is recoverable -- the same recovery, from the candidate's own
 *       d_requests / d_text_pos / d_chains. Every other slot keeps every byte of the four buffers.
 *       Interval. [qa, qb) = the parent segment's (q_begin, q_end) as they stand: an extension has already acted.
 *       Window. The interval projected along the secondary chain's end diagonals, the flank on both sides. With c = d_chains[slot],
 *       s = d_text_pos[slot] >> 63, p_hi = p_lo + c.ref_span and [u, v) = s ? [L - qb, L - qa) : [qa, qb):
 *       lo = p_lo + (u - c.q_lo) - flank, hi = p_hi + (v - c.q_hi) + flank, seg_start = min(max(lo, 0), ref_len),
 *       seg_end = max(seg_start, min(max(hi, 0), ref_len)), text_len = min(seg_end - seg_start, read_size).
 *       Outputs. d_seg_requests[slot] = {qb - qa, text_len, 0, d_requests[slot].idx}; d_seg_text_pos[slot] = seg_start | s << 63; the
 *       pattern row is read[qa, qb) as given, then zero bytes up to read_size; d_seg[slot] = {qa, qb, L, the parent's flags &
 *       (AIM_SEG_VALID | AIM_SEG_SUPPLEMENTARY | AIM_SEG_LEFT_OPEN | AIM_SEG_RIGHT_OPEN), cand = i}. A secondary segment needs no flag
 *       of its own: it is a VALID slot whose d_class entry says SECONDARY.
 *       Identity. Where the parent's interval is the whole read ([0, L): one primary, no extension) the row's request and text_pos
 *       equal the chain kernel's own slot byte for byte: lo and hi above are rule 6c's.
 *   16c, part 2: one winner per locus (aim_secondary_select_device), behind aim_sam_device_split. Slot r * K + i is valid when
 *       d_seg[slot].flags has AIM_SEG_VALID, mapped as in rule 12c, and OK when d_sam[slot].status without AIM_SAM_OVERFLOW is
 *       AIM_PAIR_OK. Primary and secondary are read from d_class as in part 1 (an empty slot is neither).
 *       Family of primary j: j itself and the valid secondaries whose parent is j. n_members is their number.
 *       Counted score. e_i = d_sam[slot].score for a mapped slot and max_score + 1 otherwise: a WFA row over the cap counts with
 *       MAX_SCORE + 1, a lower bound of its cost, as in rule 9c.
 *       Winner. The mapped member of lowest (score, i); b is its score. A family without a mapped member has no winner, and all its
 *       slots get 8 zero bytes.
 *       Runner-up. s2 = the lowest e among the other members that are valid and OK; INT32_MAX when there is none.
 *       n_tied = 1 + the number of those members with e == b.
 *       aln_mapq: rule 9c's formula -- 0 when n_tied > 1, 60 without a runner-up, otherwise min(60, 6 * max(s2 - b, 0) / score_unit).
 *       anchor_cap = 6 * min(the winner's d_chains n_anchors, 10), and 0 where that chain's score is 0 (rule 8c's f1 = 0).
 *       complete: n_members - 1 == d_class[r * K + j].n_sub -- every secondary the classification counted got a row.
 *       mapq = min(aln_mapq, anchor_cap) when complete, min(aln_mapq, anchor_cap, d_class[r * K + j].mapq) otherwise. A primary
 *       without secondaries thereby keeps exactly the byte rule 12c gives it: 6 * m with f2 = 0.
 *       aim_sec_slot_t of a family with a winner: role = 1 (the locus record) in the winner's slot, 2 (a secondary record) in the slot
 *       of every other mapped member; family = j; mapq in the winner's slot and 0 in the others; aln_mapq and n_tied; flags =
 *       AIM_SEC_SWAPPED (the winner is not j) | AIM_SEC_COMPLETE | (n_members - 1) << 4; gap = min(max(s2 - b, 0), 65534), or 65535
 *       without a runner-up: the second score relative to b in 16 bits, which saturates far above anything aln_mapq tells apart.
 *       Every other slot is 8 zero bytes.
 *   16c, part 3: records (aim_map_records_secondary_device). Rule 12c over loci instead of slots.
 *       Locus records. A family with a winner contributes the winner's row. The locus records of a read are sorted by (q_begin of the
 *       winner's segment, j); rank is the position in that order. The family of lowest j that has a winner is the line without
 *       AIM_SAM_SUPPLEMENTARY, the others gain it. The record's mapq is part 2's.
 *       Secondary records, with AIM_SEC_RECORDS in options: every slot of role 2 (a primary that lost among them) follows behind the
 *       read's locus records, ordered by (the rank of its family's locus record, score, i); such a record carries AIM_SAM_SECONDARY,
 *       has AIM_SAM_SUPPLEMENTARY cleared and mapq 0. Without the option they are dropped.
 *       c_r is the number of records of read r, or 1 when it has none: that read gets rule 12c's single unmapped record.
 *       d_rec_offsets (the same three-launch scan), read, q_begin, q_end, seg_flags, n_records and slot are rule 12c's.
 *       aim_map_sec_t, one per record, parallel to d_records: family_slot = r * K + j; second_score = b + gap saturated at
 *       INT32_MAX - 1, or INT32_MAX without a runner-up; aln_mapq; chain_mapq = d_class[family_slot].mapq; n_members; n_tied; flags =
 *       AIM_SEC_SWAPPED | AIM_SEC_COMPLETE as in part 2. The unmapped record's is {r * K, INT32_MAX, zeros}.
 *       Contigs. With d_contig (NULL: a reference of one sequence) every mapped record gets rule 13c's change -- sam.pos local to
 *       d_contig[slot], sam.pad the contig -- and the unmapped record sam.pad = AIM_CONTIG_NONE. One record kernel serves both.
 *   Kernels (csrc/secondary.hpp): secondary_rows_kernel, secondary_select_kernel, map_count_sec_kernel, map_records_sec_kernel. A read
 *       gets 4, 8 or 16 lanes by K as in chain_class_kernel; no LDS, no scratch memory, no atomics, vector stores only. The calls only
 *       enqueue work on hip_stream. d_sec is 8-byte aligned, d_sec_records, d_sam and d_records 16-byte.
 *   AIM_EINVAL with a message under the entry point's name, before any device query: aim_secondary_rows_device refuses what
 *       aim_split_segments_device refuses and, behind those bounds and before the NULL-buffer check, a max_sec outside 1..AIM_SEC_MAX;
 *       aim_secondary_select_device a K outside 1..AIM_SEED_MAX_CANDS, n_reads * K >= 2^32, max_score outside 0..INT32_MAX - 1,
 *       score_unit < 1 and a NULL device buffer with n_reads > 0; aim_map_records_secondary_device what aim_map_records_device
 *       refuses (d_sec_records aligned like d_records), unknown option bits, and with d_contig an n_contigs outside 1..AIM_CONTIG_MAX
 *       or a NULL d_contig_start.
 *   Mapper. aim_mapper_set_secondary(m, params) is called once, while no slot is in flight (like aim_mapper_set_pairing: before the first
 *       submit, or after every submitted batch was waited for); it allocates d_sec and the per-record array
 *       in every slot (aim_mapper_secondary_device_bytes says how much over all slots). aim_mapper_submit then runs the three stages
 *       at the places named above with score_unit = mismatch and the mapper's max_score, aim_mapper_wait copies the extra array, and
 *       aim_mapper_secondary(m, slot, &out) returns a view of the aim_map_sec_t[n_records] of the last wait on the slot (AIM_ESTATE
 *       before the first wait, while the slot is in flight and on a mapper without secondaries). Refusals, AIM_EINVAL under the entry
 *       point's name before any device query, in this order: a NULL params, max_sec outside 1..AIM_SEC_MAX, unknown option bits, a
 *       NULL mapper, a second call, a slot in flight, a paired mapper -- and likewise the two pairing setters on a mapper with
 *       secondaries: rule 14c rewrites the slot arrays; aim_mapper_set_pairing_secondary (rule 17c) switches both on in one call.
 * aim_secondary_kernel_names: "secondary_rows_kernel,secondary_select_kernel,map_count_sec_kernel,map_records_sec_kernel".
 * Not in this version (pairing together with secondaries and a pair MAPQ: rule 17c below): secondaries beyond the kept K, AIM_FLAG_TOP_HITS rows, the
 * voting kernel's clusters, hard clips, trimming overlapping neighbour segments, a stage inside aim_set_submit or host.c. Check
 * aim_features() & AIM_FEATURE_SECONDARY first. */
#define AIM_FEATURE_SECONDARY 0x800000u /* rule 16c: aim_secondary_rows_device / aim_secondary_select_device / aim_map_records_secondary_device / aim_mapper_set_secondary / aim_mapper_secondary exist */
#define AIM_SEC_MAX 15u                 /* max_sec is 1..AIM_SEC_MAX */
#define AIM_SEC_RECORDS 0x1u            /* options: the other mapped members of a locus as AIM_SAM_SECONDARY records */
#define AIM_SAM_SECONDARY 0x100u        /* aim_sam_t.flags, from aim_map_records_secondary_device alone */
#define AIM_SEC_SWAPPED 0x1u            /* aim_sec_slot_t.flags / aim_map_sec_t.flags: the winner is not the chain's primary */
#define AIM_SEC_COMPLETE 0x2u           /* ... every secondary rule 8c counted under the primary was aligned */
#define AIM_SEC_MEMBERS(flags) ((((uint32_t)(flags)) >> 4) + 1u) /* n_members from aim_sec_slot_t.flags */
typedef struct aim_sec_slot {
    uint8_t role;                  /* 0: none, 1: the locus record, 2: a secondary record */
    uint8_t family;                /* j */
    uint8_t mapq, aln_mapq, n_tied;
    uint8_t flags;                 /* AIM_SEC_SWAPPED | AIM_SEC_COMPLETE | (n_members - 1) << 4 */
    uint16_t gap;                  /* min(max(s2 - b, 0), 65534); 65535: no runner-up */
} aim_sec_slot_t;      /* 8 B per slot */
typedef struct aim_map_sec {
    uint32_t family_slot;          /* r * K + j */
    int32_t second_score;          /* INT32_MAX: none */
    uint8_t aln_mapq, chain_mapq, n_members, n_tied;
    uint32_t flags;                /* AIM_SEC_SWAPPED | AIM_SEC_COMPLETE */
} aim_map_sec_t;       /* 16 B per record */
typedef struct aim_map_sec_params {
    uint32_t max_sec;              /* 1..AIM_SEC_MAX */
    uint32_t options;              /* AIM_SEC_RECORDS */
} aim_map_sec_params_t;
typedef struct aim_mapper_secondary_out {
    uint32_t n_records, pad;
    const aim_map_sec_t *sec;      /* [n_records], parallel to aim_mapper_out_t.records */
} aim_mapper_secondary_out_t;
int aim_secondary_rows_device(uint32_t K, uint32_t read_size, int32_t flank, uint64_t ref_len, uint32_t n_reads, const int32_t *d_read_len,
                              const char *d_reads, const void *d_requests /* aim_request_t[n_reads * K] */, const uint64_t *d_text_pos,
                              const aim_seed_t *d_seed, const aim_chain_t *d_chains, const aim_chain_class_t *d_class,
                              void *d_seg_requests /* in/out */, uint64_t *d_seg_text_pos /* in/out */, char *d_seg_patterns /* in/out */,
                              aim_segment_t *d_seg /* in/out */, uint32_t max_sec, void *hip_stream);
int aim_secondary_select_device(uint32_t K, uint32_t n_reads, const aim_segment_t *d_seg, const aim_sam_t *d_sam, const aim_chain_class_t *d_class,
                                const aim_chain_t *d_chains, int32_t max_score, int32_t score_unit, aim_sec_slot_t *d_sec /* [n_reads * K] */,
                                void *hip_stream);
int aim_map_records_secondary_device(uint32_t K, uint32_t n_reads, uint32_t options, const aim_segment_t *d_seg, const aim_sam_t *d_sam,
                                     const aim_chain_class_t *d_class, const aim_sec_slot_t *d_sec, const uint32_t *d_contig_or_null,
                                     uint32_t n_contigs, const uint32_t *d_contig_start_or_null, uint32_t *d_rec_offsets /* [n_reads + 1] */,
                                     aim_map_record_t *d_records /* [n_reads * K] */, aim_map_sec_t *d_sec_records /* [n_reads * K] */,
                                     void *d_scratch, size_t scratch_bytes, void *hip_stream);
/* Comma-separated rocprofv3 kernel-trace name prefixes of the four kernels rule 16c adds. */
const char *aim_secondary_kernel_names(void);
int aim_mapper_secondary_device_bytes(const aim_mapper_params_t *params, const aim_map_sec_params_t *sp, uint64_t *bytes);
int aim_mapper_set_secondary(aim_mapper_t *mapper, const aim_map_sec_params_t *sp);
int aim_mapper_secondary(aim_mapper_t *mapper, uint32_t slot, aim_mapper_secondary_out_t *out);

/* ---- pairing over aligned secondaries, a MAPQ per read from the pair's runner-up (AIM_FEATURE_PAIR_SECONDARY) ----------------------
 * Rule 16c lets the alignment choose the copy of a repeat a read belongs to, rule 14c lets the mate choose -- but over the primaries
 * alone, so it reaches the right copy only through a rescue alignment, and almost never sees a second proper combination. Rule 17c is
 * rule 14c over every slot rule 16c aligned: the copy next to the mate is already a slot, and the runner-up among the combinations is
 * what a paired-end MAPQ is made from. The sequence is rule 16c's up to aim_secondary_select_device, which now runs in front of the
 * pairing; then [aim_pair_estimate_device, unchanged] -> aim_pair_rescue_rows_secondary_device -> the alignment and the records of the
 * rescue rows (rule 14c's calls, unchanged) -> aim_pair_select_secondary_device -> aim_map_records_secondary_device (unchanged) ->
 * aim_map_mates_secondary_device. Rule 17c reads d_sec as part 2 of rule 16c wrote it and rewrites it. Arithmetic is signed 64-bit;
 * everything is deterministic and independent of the grid and of the AIM_DEBUG_POISON_* knobs.
 *   17c. A slot TAKES PART when it is mapped (rule 12c) and d_sec[slot].role is not 0; part 2 of rule 16c gives a role to every mapped
 *       slot the pipeline produces, a secondary that got a row under part 1 included. The REPRESENTATIVE of read r is the slot of role 1
 *       in the family of lowest j that has a winner: the record part 3 leaves without AIM_SAM_SUPPLEMENTARY. (Not rule 12c's lowest
 *       mapped slot: a family's winner may be a secondary.) Where rule 14c says "read r has a mapped slot", rule 17c says "read r has
 *       a representative". Proper combination, span and cost are rule 14c's, over the slots that take part plus index K for a usable
 *       rescue row; primaries, supplementary primaries and secondaries count alike; (K, K) is excluded.
 *       Bounds. min_span and max_span are pp's, or those of the aim_pair_estimate_t at d_est when d_est is not NULL (rule 15c; pp's
 *       own still have to pass rule 14c's checks). One kernel serves both cases.
 *       Rescue rows (aim_pair_rescue_rows_secondary_device). Rule 14c's text with the representative as the anchor: tried when options
 *       has AIM_PAIR_RESCUE, the mate has a representative, no proper combination exists among the slots that take part -- a copy
 *       that already fits the mate costs no rescue -- and L > 0. Windows, empty rows, pattern rows and the contig clip are rule 14c's.
 *       Choice (aim_pair_select_secondary_device). Rule 14c's: lowest cost, ties to the lowest i and then the lowest j; n_best and
 *       second_sum as there. The unpaired cost is score(rep_a) + score(rep_b) + unpaired_penalty, clamped alike, and exists when both
 *       reads have a representative. The proper combination is taken when there is no unpaired cost or its cost is no higher.
 *       aim_map_pair_t keeps its layout and its meaning (not taken: slot[] = the representatives). On slot arrays in which no secondary
 *       has a row every aim_map_pair_t equals rule 14c's byte for byte.
 *       Pair MAPQ, for a taken combination (vi, vj) of cost c, for read a = 2m (read b alike with j, vj): alt_a is the lower of the
 *       lowest cost among the proper combinations with i != vi and, where it exists and a's representative is not slot vi, the
 *       unpaired cost; INT32_MAX with neither. tied_a is the number of proper combinations with i != vi and cost c. pair_mapq_a is 0
 *       when tied_a > 0, 60 when alt_a is INT32_MAX, otherwise min(60, 6 * max(alt_a - c, 0) / score_unit). own_a is
 *       d_sec[slot].mapq when the chosen slot has role 1 (before apply), 0 for a role-2 slot and for a rescue row.
 *       mapq_a = min(max(own_a, min(pair_mapq_a, own_a + 40)), cap_a), where cap_a is rule 16c's anchor_cap of the chosen slot's own
 *       chain (d_chains) and, for a rescue row, the mate's mapq, computed first. So a unique mate keeps its 60 while its partner in a
 *       tied repeat gets 0, and a read that pairing moved off its alignment winner gets 6 * (unpaired_penalty - score difference) /
 *       score_unit. aim_map_pair_mapq_t[m] holds alt, mapq, pair_mapq, own_mapq and tied (saturating at 255) of both reads; for a
 *       combination that is not taken, zeros with alt_sum INT32_MAX.
 *       Apply (inside aim_pair_select_secondary_device). Not taken: no byte of d_sec or of the slot arrays changes. A chosen slot of
 *       role 1: its d_sec.mapq becomes mapq_a. A chosen slot of role 2: it and its family's role-1 slot exchange roles -- the promoted
 *       slot gets role 1, mapq_a, aln_mapq 0, gap 0 and AIM_SEC_SWAPPED exactly when it is not the family's j; the demoted slot gets
 *       role 2 and mapq 0, and thereby becomes the 0x100 record under AIM_SEC_RECORDS; every other byte of the family stays. A chosen
 *       rescue row of read b: rule 14c's apply to d_sam, d_seg and d_contig; the mapq byte of d_class[b * K] becomes that of
 *       d_class[the anchor's family slot], which is what part 3 reports as chain_mapq; d_sec[b * K] becomes {role 1, family 0, mapq_b,
 *       aln_mapq 0, n_tied 1, AIM_SEC_COMPLETE, gap 65535} and the read's other d_sec entries 8 zero bytes.
 *       Mate fields (aim_map_mates_secondary_device), behind aim_map_records_secondary_device. Rule 14c's, with the mate's reference
 *       record its chosen slot if the pair is proper, else its representative, read from d_sec as apply left it; "the mate has no
 *       mapped slot" reads "the mate has no slot of role 1". AIM_SAM_SECONDARY records get 0x1, 0x40 / 0x80, 0x8 / 0x20 and the mate's
 *       position like any record; they never get 0x2, and their tlen is 0.
 *   Kernels (csrc/pair_secondary.hpp): pair_sec_rescue_rows_kernel, pair_sec_select_kernel, map_mates_sec_kernel. A read pair gets 4, 8
 *       or 16 lanes by K as in rule 14c, candidate i of both reads with its d_sec entries in lane i; the per-read alternatives come from
 *       a second pass of K broadcasts. No LDS, no scratch memory, no atomics. The calls only enqueue work on hip_stream.
 *       AIM_EINVAL under the entry point's name, before any device query: everything the rule-14c counterpart refuses, in its order;
 *       aim_pair_select_secondary_device a score_unit < 1, in front of the NULL-buffer check; a NULL d_sec, d_chains or d_pair_mapq
 *       with n_reads > 0; d_sec or d_chains not 8-byte aligned, d_pair_mapq or a given d_est not 16-byte aligned.
 * aim_pair_secondary_kernel_names: "pair_sec_rescue_rows_kernel,pair_sec_select_kernel,map_mates_sec_kernel".
 *   Precondition. d_sec is what aim_secondary_select_device wrote for these slot arrays: a slot with a role is mapped, and a role-2 slot
 *       has a role-1 slot in its family. The kernels stay inside the read's slots for any d_sec, but their bytes are defined for such a one only.
 *   Mapper. aim_mapper_set_pairing_secondary(m, &pp, ep_or_null, &sp) switches on pairing, the estimate when ep is given, and
 *       secondaries in one call, with the state rules of aim_mapper_set_pairing. Refusals, AIM_EINVAL under its name before any device
 *       query, in this order: a NULL mapper, aim_mapper_set_pairing's of pp, ep's rules (rule 15c) when ep is given, rule 16c's of sp;
 *       then a mapper any of the three earlier setters has touched (AIM_ESTATE for a second call of its own, and for a slot in flight).
 *       The earlier setters refuse a mapper this one has touched. It allocates what aim_mapper_set_pairing[_estimated] and
 *       aim_mapper_set_secondary allocate plus one aim_map_pair_mapq_t per read pair and slot;
 *       aim_mapper_pairing_secondary_device_bytes reports the sum without the estimate's buffers. aim_mapper_submit runs the
 *       sequence above with score_unit = mismatch; aim_mapper_wait copies aim_map_pair_mapq_t[n_reads / 2] as well. aim_mapper_pairs,
 *       aim_mapper_secondary and aim_mapper_pair_estimate work as on the mappers of their own setters; aim_mapper_pair_mapq(m, slot,
 *       &view) gives the aim_map_pair_mapq_t[n_pairs] of the last batch waited for on the slot, with aim_mapper_pairs' state rules.
 *       A mapper set up by an earlier setter, or by none, keeps its buffers and every byte it gave.
 * Not in this version: rescue against anchors other than the representative; a
 * rescued read's discordant placement as a secondary line; a pair MAPQ on a mapper paired without secondaries; compaction of the rescue
 * rows; pairing inside aim_set_submit or host.c. Check aim_features() & AIM_FEATURE_PAIR_SECONDARY first. */
#define AIM_FEATURE_PAIR_SECONDARY 0x1000000u /* rule 17c: aim_pair_rescue_rows_secondary_device / aim_pair_select_secondary_device / aim_map_mates_secondary_device / aim_mapper_set_pairing_secondary / aim_mapper_pair_mapq exist */
typedef struct aim_map_pair_mapq {  /* 16 B, one per read pair m; [0]: read 2m, [1]: read 2m + 1 */
    int32_t alt_sum[2];            /* lowest cost of what places the read elsewhere; INT32_MAX: nothing does, or not taken */
    uint8_t mapq[2];               /* what apply wrote into d_sec of the chosen slot */
    uint8_t pair_mapq[2];          /* from alt_sum and tied alone */
    uint8_t own_mapq[2];           /* the chosen slot's MAPQ before apply; 0 for a role-2 slot and a rescue row */
    uint8_t tied[2];               /* combinations that place the read elsewhere at the taken cost, saturating at 255 */
} aim_map_pair_mapq_t;
int aim_pair_rescue_rows_secondary_device(const aim_map_pair_params_t *pp, uint32_t K, uint32_t read_size, uint64_t ref_len, uint32_t n_contigs,
                                          const uint32_t *d_contig_start, const uint32_t *d_contig_len, uint32_t n_reads, const int32_t *d_read_len,
                                          const char *d_reads, const aim_segment_t *d_seg, const aim_sam_t *d_sam, const uint32_t *d_contig_or_null,
                                          const aim_sec_slot_t *d_sec, void *d_res_requests, uint64_t *d_res_text_pos, char *d_res_patterns,
                                          const aim_pair_estimate_t *d_est_or_null, void *hip_stream);
int aim_pair_select_secondary_device(const aim_map_pair_params_t *pp, uint32_t K, uint32_t read_size, uint32_t n_reads, const int32_t *d_read_len,
                                     aim_segment_t *d_seg, aim_sam_t *d_sam, aim_chain_class_t *d_class, uint32_t *d_contig_or_null,
                                     aim_sec_slot_t *d_sec /* in/out */, const aim_chain_t *d_chains, int32_t score_unit,
                                     const aim_sam_t *d_res_sam /* [n_reads]; may be NULL without AIM_PAIR_RESCUE */, uint32_t cigar_base, uint32_t md_base,
                                     aim_map_pair_t *d_pairs /* [n_reads / 2] */, aim_map_pair_mapq_t *d_pair_mapq /* [n_reads / 2] */,
                                     const aim_pair_estimate_t *d_est_or_null, void *hip_stream);
int aim_map_mates_secondary_device(uint32_t K, uint32_t n_reads, const aim_map_pair_t *d_pairs, const aim_segment_t *d_seg, const aim_sam_t *d_sam,
                                   const aim_sec_slot_t *d_sec, const uint32_t *d_contig_or_null, uint32_t n_contigs, const uint32_t *d_contig_start,
                                   const uint32_t *d_rec_offsets, aim_map_record_t *d_records, aim_map_mate_t *d_mates /* [n_reads * K] */,
                                   void *hip_stream);
/* Comma-separated rocprofv3 kernel-trace name prefixes of the three kernels rule 17c adds. */
const char *aim_pair_secondary_kernel_names(void);
int aim_mapper_pairing_secondary_device_bytes(const aim_mapper_params_t *params, const aim_map_pair_params_t *pp, const aim_map_sec_params_t *sp, uint64_t *bytes);
int aim_mapper_set_pairing_secondary(aim_mapper_t *mapper, const aim_map_pair_params_t *pp, const aim_pair_est_params_t *ep_or_null, const aim_map_sec_params_t *sp);
int aim_mapper_pair_mapq(aim_mapper_t *mapper, uint32_t slot, const aim_map_pair_mapq_t **out /* [n_pairs of aim_mapper_pairs] */);
/* The plan aim_align_device would follow for (params, n_pairs) in this process right now, as one line (see
 * aim_set_plan_describe).  The stateless entry points read the AIM_* switches at every call. */
int aim_plan_describe(const aim_params_t *params, uint32_t n_pairs, char *out, size_t cap);
/* Name of the kernel aim_align_device would launch for this configuration
 * (matches the rocprofv3 kernel-trace name prefix). */
const char *aim_kernel_name(const aim_params_t *params);

/* ---- host-side helpers shared by the CLI and the Python binding ---------- */
/* MAX_SCORE / READ_SIZE heuristics of the launchers (run-wfa-pim-wram.py:57-68,
 * run-nw-pim-wram.py:50-57 [gap instead of gap_o+gap_e], run-swg-pim-wram.py:52-62). */
int aim_launcher_sizes(int32_t algo, int32_t read_length, double error, int32_t mismatch, int32_t gap_o,
                       int32_t gap_e, int32_t gap, int32_t *max_score, int32_t *read_size);
/* edit_cigar_print (host.c:69-89): RLE of ops[begin,end) + '\n' into out;
 * returns bytes written or AIM_EINVAL if cap is too small. */
int aim_cigar_format(const char *ops, int32_t begin_offset, int32_t end_offset, char *out, int32_t cap);
/* BAM CIGAR words (aim_sam_t) as a SAM CIGAR string, NUL-terminated: "*" for n = 0. Returns the bytes written (without the NUL) or
 * AIM_EINVAL when cap is too small or a word holds an op outside MIDNSHP=X. */
int aim_sam_format_cigar(const uint32_t *words, uint32_t n, char *out, int32_t cap);
/* Seeded synthetic pairs (DESIGN.md "Synthetic data"): pattern = len uniform
 * ACGT bases; text = pattern after ceil(len*error) sequential uniform
 * substitute/insert/delete edits.  Pair i depends only on (seed, first_idx+i). */
int aim_gen_pairs(uint64_t seed, uint64_t first_idx, uint32_t n_pairs, int32_t len, double error,
                  int32_t read_size, aim_request_t *requests, char *patterns, char *texts);

#ifdef __cplusplus
}
#endif
#endif /* AIM_HIP_H */
