"""ctypes binding of the C-ABI in include/aim_hip.h (libaim_hip.so).

This is the Python twin of the cgo/ctypes stub shown in INTEGRATION.md: plain
pointers and sizes only.  The library is built in-tree by aim_amd.build (hipcc,
gfx950); importing this module never compiles anything and never falls back to
a CPU implementation -- a missing library is an ImportError-like RuntimeError.
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("AIM_LIB") or os.path.join(_HERE, "libaim_hip.so")   # AIM_LIB: A/B builds of the same ABI

AIM_OK, AIM_EINVAL, AIM_ENODEV, AIM_ENOMEM, AIM_ESTATE, AIM_EALIGN = 0, -1, -2, -3, -4, -5
ALGO_NW, ALGO_SWG, ALGO_WFA, ALGO_GENASM = 0, 1, 2, 3
ALGO_BY_NAME = {"nw": ALGO_NW, "swg": ALGO_SWG, "wfa": ALGO_WFA, "genasm": ALGO_GENASM}
FLAG_BACKTRACE, FLAG_REDUCE, FLAG_SWG_W16, FLAG_REQ8, FLAG_RES8, FLAG_ENDSFREE, FLAG_AFFINE2P = 1, 2, 4, 8, 16, 32, 64
FLAG_LINEAR = 128      # gap-linear WFA on Params itself (gap_o = 0, gap_e per gap base)
FEATURE_ENDSFREE = 1   # aim_features(): AIM_FLAG_ENDSFREE is honoured
FEATURE_AFFINE2P = 2   # aim_features(): AIM_FLAG_AFFINE2P is honoured
FEATURE_LINEAR = 4     # aim_features(): AIM_FLAG_LINEAR is honoured
FLAG_WFA_W32 = 256     # WFA with int32 wavefront offsets (AFFINE_WAVEFRONT_W32): read_size up to 2^24
FEATURE_WFA_W32 = 8    # aim_features(): AIM_FLAG_WFA_W32 is honoured
FLAG_WFA_BIDIR = 512   # bidirectional WFA with CIGAR: O(MAX_SCORE) scratch per workgroup (global gap-affine, BACKTRACE)
FEATURE_WFA_BIDIR = 16 # aim_features(): AIM_FLAG_WFA_BIDIR is honoured
FLAG_REF_TEXTS = 0x400 # texts named as (position, strand) windows of the device-resident reference (aim_set_reference)
FEATURE_REF_TEXTS = 0x20  # aim_features(): AIM_FLAG_REF_TEXTS is honoured
REF_MINUS_STRAND = 1 << 63   # text_pos bit 63: the reverse complement of the window
FLAG_READ_GROUPS = 0x800     # reads and their candidates: score-only pass, best candidate per read, the configured run on the winners
FEATURE_READ_GROUPS = 0x40   # aim_features(): AIM_FLAG_READ_GROUPS is honoured
FLAG_WFA_ESCALATE = 0x1000   # WFA: a lane kernel at a low cap over the batch, the flag-less plan over the pairs it left over that cap
FEATURE_WFA_ESCALATE = 0x80  # aim_features(): AIM_FLAG_WFA_ESCALATE is honoured
FLAG_MATE_PAIRS = 0x2000     # paired-end selection over a read-groups batch of reference windows: reads 2m and 2m + 1 are mates
FEATURE_MATE_PAIRS = 0x100   # aim_features(): AIM_FLAG_MATE_PAIRS is honoured
FLAG_SAM_FIELDS = 0x4000     # SAM-ready records (POS, CIGAR, NM, MD) from the final ops rows and the resident reference
FEATURE_SAM_FIELDS = 0x200   # aim_features(): AIM_FLAG_SAM_FIELDS is honoured
FLAG_TOP_HITS = 0x8000       # the max_hits best candidates of every read of a read-groups batch, each a full row
FEATURE_TOP_HITS = 0x400     # aim_features(): AIM_FLAG_TOP_HITS is honoured
TOP_HITS_MAX = 8             # max_hits is 1..TOP_HITS_MAX
FEATURE_SEED = 0x800         # aim_features(): device-side seeding (aim_index_* / aim_seed_*) exists
SEED_MAX_CANDS, SEED_MAX_HITS, SEED_TRUNCATED, SEED_MAX_READ_SIZE = 16, 1024, 1, 4096
SEED_MAX_REF_LEN = (1 << 32) - (1 << 25)
FEATURE_INDEX_DEVICE = 0x1000   # aim_features(): aim_index_device_scratch / aim_index_build_device / aim_index_kernel_names exist
FEATURE_MINIMIZERS = 0x2000     # aim_features(): aim_index_build_minimizers / aim_index_build_device_minimizers / SEED_OPT_MINIMIZERS exist
SEED_MAX_W = 32                 # AIM_SEED_MAX_W: the minimizer window is 1..32
FEATURE_SEED_CHAIN = 0x4000     # aim_features(): aim_seed_chain_device / aim_chain_t / aim_seed_chain_kernel_names exist
SEED_CHAIN_LOOKBACK, SEED_CHAIN_MAX_BAND = 64, 4096
FEATURE_SEED_CHAIN_LONG = 0x8000  # aim_features(): aim_seed_chain_long_device / aim_seed_chain_long_kernel_name exist
SEED_LONG_MAX_READ_SIZE, SEED_LONG_MAX_HITS = 65528, 8192
FEATURE_CHAIN_CLASS = 0x10000     # aim_features(): aim_chain_classify_device / aim_read_mapq_device / aim_chain_class_kernel_names exist
FEATURE_SPLIT = 0x20000           # aim_features(): aim_split_segments_device / aim_sam_device_split / aim_split_kernel_names exist
FEATURE_EXTEND = 0x40000          # aim_features(): aim_extend_segments_device / aim_extend_kernel_names exist
CHAIN_MASK_DEFAULT = 128          # AIM_CHAIN_MASK_DEFAULT: mask_q8 of minimap2's mask level 0.5
CHAIN_PRIMARY, CHAIN_SECONDARY, CHAIN_SUPPLEMENTARY = 0x1, 0x2, 0x4            # aim_chain_class_t.flags
MAPQ_UNMAPPED, MAPQ_SECONDARY, MAPQ_SUPPLEMENTARY, MAPQ_PROPER = 0x1, 0x2, 0x4, 0x8   # aim_read_mapq_t.flags
SEG_VALID, SEG_SUPPLEMENTARY, SEG_LEFT_OPEN, SEG_RIGHT_OPEN, SEG_LOOSE = 0x1, 0x2, 0x4, 0x8, 0x10   # aim_segment_t.flags
SAM_SUPPLEMENTARY = 0x800         # aim_sam_t.flags, from aim_sam_device_split
SEG_EXT_LEFT, SEG_EXT_RIGHT = 0x20, 0x40   # aim_segment_t.flags, from aim_extend_segments_device
EXTEND_MAX_UNIT, EXTEND_MAX_COST, EXTEND_MAX_BAND, EXTEND_MAX_EXT = 64, 4095, 31, 1024
FEATURE_MAPPER = 0x80000          # aim_features(): aim_map_records_device / aim_mapper_* exist
MAP_EXTEND = 0x1                  # aim_mapper_params_t.options: run the segment extension (rule 11c)
MAPPER_MAX_SLOTS = 4
FEATURE_CONTIGS = 0x100000        # aim_features(): aim_contigs_* / aim_contig_clip_device / aim_map_records_contigs_device / aim_mapper_create_contigs exist
CONTIG_MAX, CONTIG_NONE = 1 << 20, 0xFFFFFFFF
SEG_CONTIG_CLIPPED = 0x80         # aim_segment_t.flags, from aim_contig_clip_device
FEATURE_PAIRED = 0x200000         # aim_features(): aim_pair_rescue_rows_device / aim_pair_select_device / aim_map_mates_device / aim_mapper_set_pairing exist
PAIR_RESCUE = 0x1                 # aim_map_pair_params_t.options: try the mate rescue
PAIR_PROPER, PAIR_RESCUE_TRIED_A, PAIR_RESCUE_TRIED_B, PAIR_RESCUED_A, PAIR_RESCUED_B = 0x1, 0x2, 0x4, 0x8, 0x10   # aim_map_pair_t.flags
FEATURE_PAIR_ESTIMATE = 0x400000  # aim_features(): aim_pair_estimate_device / the _est entry points / aim_mapper_set_pairing_estimated exist (rule 15c)
PAIR_EST_MAX_HIST = 8192          # aim_pair_est_params_t.hist_size: 64..this, a multiple of 64
PAIR_EST_FALLBACK, PAIR_EST_CLAMPED, PAIR_EST_FLOORED = 0x1, 0x2, 0x4   # aim_pair_estimate_t.flags
FEATURE_SECONDARY = 0x800000      # aim_features(): aim_secondary_rows_device / aim_secondary_select_device / aim_map_records_secondary_device / aim_mapper_set_secondary exist (rule 16c)
SEC_MAX = 15                      # max_sec is 1..SEC_MAX
SEC_RECORDS = 0x1                 # aim_map_sec_params_t.options: the other mapped members of a locus as SAM_SECONDARY records
SAM_SECONDARY = 0x100             # aim_sam_t.flags, from aim_map_records_secondary_device
SEC_SWAPPED, SEC_COMPLETE = 0x1, 0x2   # aim_sec_slot_t.flags / aim_map_sec_t.flags; aim_sec_slot_t.flags >> 4 is n_members - 1
FEATURE_PAIR_SECONDARY = 0x1000000  # aim_features(): aim_pair_rescue_rows_secondary_device / aim_pair_select_secondary_device / aim_map_mates_secondary_device exist (rule 17c)


def CONTIG_SPACER(band):
    """AIM_CONTIG_SPACER(band): the 'N' bases aim_mapper_create_contigs puts between two contigs."""
    return int(band) + 64


def SEED_OPT_MINIMIZERS(w):
    """AIM_SEED_OPT_MINIMIZERS(w), for aim_seed_params_t.options."""
    return (int(w) << 8) & 0xFFFFFFFF
SAM_EQX, SAM_REVERSE, SAM_UNMAPPED, SAM_OVERFLOW = 0x1, 0x10, 0x4, 0x100   # sam_options; aim_sam_t.flags (SAM's own bits); aim_sam_t.status bit
MATE_PROPER = 1              # aim_mate_t.flags: the chosen candidates are a proper combination
PAIR_OK, PAIR_WFA_NO_LINK, PAIR_SWG_NO_OP, PAIR_NOMEM = 0, 1, 2, 3


class Params(C.Structure):
    """aim_params_t"""
    _fields_ = [("algo", C.c_int32), ("match", C.c_int32), ("mismatch", C.c_int32), ("gap_o", C.c_int32),
                ("gap_e", C.c_int32), ("gap_i", C.c_int32), ("gap_d", C.c_int32), ("max_score", C.c_int32),
                ("read_size", C.c_int32), ("flags", C.c_uint32)]


class EndsFreeParams(C.Structure):
    """aim_endsfree_params_t: aim_params_t + the four free lengths of AIM_FLAG_ENDSFREE (include/aim_hip.h). The entry points
    receive a pointer to `base` (params_ref); fields of the base read through, e.g. p.read_size."""
    _fields_ = [("base", Params), ("pattern_begin_free", C.c_int32), ("pattern_end_free", C.c_int32),
                ("text_begin_free", C.c_int32), ("text_end_free", C.c_int32)]

    _own = ("base", "pattern_begin_free", "pattern_end_free", "text_begin_free", "text_end_free")

    def __getattr__(self, name):   # only reached for names that are not fields of this structure
        return getattr(self.base, name)

    def __setattr__(self, name, value):   # fields of the base are written through: ef.flags |= FLAG_BACKTRACE reaches the library
        if name not in self._own and hasattr(Params, name):
            setattr(self.base, name, value)
        else:
            super().__setattr__(name, value)


class Affine2pParams(C.Structure):
    """aim_affine2p_params_t: aim_params_t + the second gap piece of AIM_FLAG_AFFINE2P (include/aim_hip.h). Like EndsFreeParams,
    the entry points receive a pointer to `base` (params_ref) and fields of the base read and write through."""
    _fields_ = [("base", Params), ("gap_o2", C.c_int32), ("gap_e2", C.c_int32)]

    _own = ("base", "gap_o2", "gap_e2")

    def __getattr__(self, name):
        return getattr(self.base, name)

    def __setattr__(self, name, value):
        if name not in self._own and hasattr(Params, name):
            setattr(self.base, name, value)
        else:
            super().__setattr__(name, value)


def params_ref(params):
    """The `const aim_params_t *` argument for Params, EndsFreeParams or Affine2pParams (a pointer to the base of the extended struct)."""
    return C.byref(params.base) if isinstance(params, (EndsFreeParams, Affine2pParams)) else C.byref(params)


REQUEST_DTYPE = np.dtype([("pattern_len", "<i4"), ("text_len", "<i4"), ("padding", "<i4"), ("idx", "<u4")])
RESULT_DTYPE = np.dtype([("max_operations", "<i4"), ("begin_offset", "<i4"), ("end_offset", "<i4"),
                         ("score", "<i4"), ("status", "<i4"), ("idx", "<u4")])
REQUEST8_DTYPE = np.dtype([("pattern_len", "<i2"), ("text_len", "<i2"), ("idx", "<u4")])     # AIM_FLAG_REQ8
RESULT8_DTYPE = np.dtype([("idx", "<u4"), ("score", "<i4")])                                 # AIM_FLAG_RES8
assert REQUEST_DTYPE.itemsize == 16 and RESULT_DTYPE.itemsize == 24
assert REQUEST8_DTYPE.itemsize == 8 and RESULT8_DTYPE.itemsize == 8

CIGAR_DTYPE = np.dtype([("idx", "<u4"), ("score", "<i4"), ("run_offset", "<u4"), ("n_runs", "<u2"), ("status", "<u2")])   # aim_cigar_t
assert CIGAR_DTYPE.itemsize == 16
CIGAR_OVERFLOW = 0x100
BEST_DTYPE = np.dtype([("best_pair", "<u4"), ("best_score", "<i4"), ("second_score", "<i4"), ("n_best", "<u4")])   # aim_best_t
assert BEST_DTYPE.itemsize == 16
MATE_DTYPE = np.dtype([("best_pair", "<u4", (2,)), ("score_sum", "<i4"), ("second_sum", "<i4"), ("n_best", "<u4"), ("flags", "<u4"),
                       ("pad", "<u4", (2,))])   # aim_mate_t
assert MATE_DTYPE.itemsize == 32
SAM_DTYPE = np.dtype([("idx", "<u4"), ("score", "<i4"), ("pos", "<u8"), ("ref_span", "<u4"), ("nm", "<u4"), ("cigar_offset", "<u4"),
                      ("n_cigar", "<u4"), ("md_offset", "<u4"), ("md_len", "<u4"), ("flags", "<u2"), ("status", "<u2"), ("pad", "<u4")])   # aim_sam_t
assert SAM_DTYPE.itemsize == 48


class SeedParams(C.Structure):
    """aim_seed_params_t"""
    _fields_ = [("k", C.c_int32), ("stride", C.c_int32), ("max_occ", C.c_int32), ("band", C.c_int32), ("flank", C.c_int32),
                ("min_votes", C.c_int32), ("max_cands", C.c_int32), ("read_size", C.c_int32), ("idx_base", C.c_uint32), ("options", C.c_uint32)]


SEED_DTYPE = np.dtype([("n_cands", "<u4"), ("n_hits", "<u4", (2,)), ("flags", "<u4")])   # aim_seed_t
assert SEED_DTYPE.itemsize == 16 and C.sizeof(SeedParams) == 40
CHAIN_DTYPE = np.dtype([("score", "<u4"), ("n_anchors", "<u2"), ("reserved", "<u2"), ("q_lo", "<u2"), ("q_hi", "<u2"), ("ref_span", "<u4")])   # aim_chain_t
assert CHAIN_DTYPE.itemsize == 16
CHAIN_CLASS_DTYPE = np.dtype([("sub_score", "<u4"), ("parent", "u1"), ("flags", "u1"), ("mapq", "u1"), ("n_sub", "u1")])   # aim_chain_class_t
READ_MAPQ_DTYPE = np.dtype([("slot", "<u4"), ("mapq", "u1"), ("chain_mapq", "u1"), ("aln_mapq", "u1"), ("flags", "u1")])   # aim_read_mapq_t
SEGMENT_DTYPE = np.dtype([("q_begin", "<u2"), ("q_end", "<u2"), ("read_len", "<u2"), ("flags", "u1"), ("cand", "u1")])   # aim_segment_t
assert CHAIN_CLASS_DTYPE.itemsize == 8 and READ_MAPQ_DTYPE.itemsize == 8
EXTEND_DTYPE = np.dtype([("dq", "<u2", (2,)), ("dr", "<u2", (2,)), ("stop", "<u2", (2,)), ("pad", "<u2", (2,)), ("score", "<i4", (2,))])   # aim_extend_t
assert EXTEND_DTYPE.itemsize == 24


class ExtendParams(C.Structure):
    """aim_extend_params_t"""
    _fields_ = [("match", C.c_int32), ("mismatch", C.c_int32), ("gap_o", C.c_int32), ("gap_e", C.c_int32), ("xdrop", C.c_int32),
                ("max_cost", C.c_int32), ("band", C.c_int32), ("max_ext", C.c_int32)]


MAP_RECORD_DTYPE = np.dtype([("sam", SAM_DTYPE), ("read", "<u4"), ("q_begin", "<u2"), ("q_end", "<u2"), ("mapq", "u1"), ("seg_flags", "u1"), ("rank", "u1"),
                             ("n_records", "u1"), ("slot", "<u4")])   # aim_map_record_t
assert MAP_RECORD_DTYPE.itemsize == 64


class MapperParams(C.Structure):
    """aim_mapper_params_t"""
    _fields_ = [("seed", SeedParams), ("max_hits", C.c_uint32), ("mask_q8", C.c_uint32), ("extend", ExtendParams), ("options", C.c_uint32),
                ("match", C.c_int32), ("mismatch", C.c_int32), ("gap_o", C.c_int32), ("gap_e", C.c_int32), ("max_score", C.c_int32),
                ("sam_options", C.c_uint32), ("max_reads", C.c_uint32), ("slots", C.c_uint32), ("cigar_cap", C.c_uint32), ("md_cap", C.c_uint32)]


class MapperOut(C.Structure):
    """aim_mapper_out_t"""
    _fields_ = [("n_reads", C.c_uint32), ("n_records", C.c_uint32), ("cigar_words", C.c_uint32), ("md_bytes", C.c_uint32),
                ("cigar_needed", C.c_uint32), ("md_needed", C.c_uint32), ("records", C.c_void_p), ("rec_offsets", C.c_void_p),
                ("cigar", C.c_void_p), ("md", C.c_void_p)]


assert C.sizeof(MapperParams) == 124 and C.sizeof(MapperOut) == 56


class MapPairParams(C.Structure):
    """aim_map_pair_params_t"""
    _fields_ = [("min_span", C.c_int64), ("max_span", C.c_int64), ("unpaired_penalty", C.c_int32), ("options", C.c_uint32), ("rescue_size", C.c_uint32),
                ("rescue_cigar_cap", C.c_uint32), ("rescue_md_cap", C.c_uint32), ("pad", C.c_uint32)]


class MapperPairsOut(C.Structure):
    """aim_mapper_pairs_out_t"""
    _fields_ = [("n_pairs", C.c_uint32), ("n_records", C.c_uint32), ("rescue_cigar_words", C.c_uint32), ("rescue_md_bytes", C.c_uint32),
                ("rescue_cigar_needed", C.c_uint32), ("rescue_md_needed", C.c_uint32), ("mates", C.c_void_p), ("pairs", C.c_void_p)]


MAP_PAIR_DTYPE = np.dtype([("slot", "<u4", (2,)), ("score_sum", "<i4"), ("second_sum", "<i4"), ("n_best", "<u4"), ("flags", "<u4"), ("span", "<i8")])   # aim_map_pair_t
MAP_MATE_DTYPE = np.dtype([("mate_pos", "<u8"), ("tlen", "<i4"), ("mate_contig", "<u4")])   # aim_map_mate_t
assert C.sizeof(MapPairParams) == 40 and C.sizeof(MapperPairsOut) == 40 and MAP_PAIR_DTYPE.itemsize == 32 and MAP_MATE_DTYPE.itemsize == 16


class PairEstParams(C.Structure):
    """aim_pair_est_params_t"""
    _fields_ = [("hist_size", C.c_uint32), ("min_samples", C.c_uint32), ("min_mapq", C.c_uint32), ("min_slack", C.c_uint32)]


class PairEstimate(C.Structure):
    """aim_pair_estimate_t"""
    _fields_ = [("min_span", C.c_int64), ("max_span", C.c_int64), ("n_samples", C.c_uint32), ("n_beyond", C.c_uint32), ("p25", C.c_uint32), ("p50", C.c_uint32),
                ("p75", C.c_uint32), ("flags", C.c_uint32), ("pad", C.c_uint32 * 2)]


PAIR_ESTIMATE_DTYPE = np.dtype([("min_span", "<i8"), ("max_span", "<i8"), ("n_samples", "<u4"), ("n_beyond", "<u4"), ("p25", "<u4"), ("p50", "<u4"), ("p75", "<u4"),
                                ("flags", "<u4"), ("pad", "<u4", (2,))])   # aim_pair_estimate_t
assert C.sizeof(PairEstParams) == 16 and C.sizeof(PairEstimate) == 48 and PAIR_ESTIMATE_DTYPE.itemsize == 48


class MapSecParams(C.Structure):
    """aim_map_sec_params_t"""
    _fields_ = [("max_sec", C.c_uint32), ("options", C.c_uint32)]


class MapperSecondaryOut(C.Structure):
    """aim_mapper_secondary_out_t"""
    _fields_ = [("n_records", C.c_uint32), ("pad", C.c_uint32), ("sec", C.c_void_p)]


SEC_SLOT_DTYPE = np.dtype([("role", "u1"), ("family", "u1"), ("mapq", "u1"), ("aln_mapq", "u1"), ("n_tied", "u1"), ("flags", "u1"), ("gap", "<u2")])   # aim_sec_slot_t
MAP_SEC_DTYPE = np.dtype([("family_slot", "<u4"), ("second_score", "<i4"), ("aln_mapq", "u1"), ("chain_mapq", "u1"), ("n_members", "u1"), ("n_tied", "u1"),
                          ("flags", "<u4")])   # aim_map_sec_t
assert C.sizeof(MapSecParams) == 8 and C.sizeof(MapperSecondaryOut) == 16 and SEC_SLOT_DTYPE.itemsize == 8 and MAP_SEC_DTYPE.itemsize == 16
MAP_PAIR_MAPQ_DTYPE = np.dtype([("alt_sum", "<i4", (2,)), ("mapq", "u1", (2,)), ("pair_mapq", "u1", (2,)), ("own_mapq", "u1", (2,)), ("tied", "u1", (2,))])   # aim_map_pair_mapq_t
assert MAP_PAIR_MAPQ_DTYPE.itemsize == 16


class BatchIO(C.Structure):
    """aim_batch_io_t"""
    _fields_ = [("n_pairs", C.c_uint32), ("requests", C.c_void_p), ("patterns", C.c_void_p), ("texts", C.c_void_p),
                ("packed_patterns", C.c_void_p), ("packed_texts", C.c_void_p), ("n_raw", C.c_uint32), ("raw_pairs", C.c_void_p),
                ("raw_patterns", C.c_void_p), ("raw_texts", C.c_void_p), ("results", C.c_void_p), ("ops", C.c_void_p),
                ("cigars", C.c_void_p), ("runs", C.c_void_p), ("runs_cap", C.c_uint32)]


class BatchIORef(C.Structure):
    """aim_batch_io_ref_t: aim_batch_io_t + text_pos (AIM_FLAG_REF_TEXTS); aim_set_submit receives a pointer to `base`."""
    _fields_ = [("base", BatchIO), ("text_pos", C.c_void_p)]


class BatchIOGroups(C.Structure):
    """aim_batch_io_groups_t: laid out like BatchIORef, then the reads (AIM_FLAG_READ_GROUPS); aim_set_submit receives a pointer to
    `base`."""
    _fields_ = [("base", BatchIO), ("text_pos", C.c_void_p), ("n_reads", C.c_uint32), ("read_offsets", C.c_void_p), ("best", C.c_void_p)]


class BatchIOMates(C.Structure):
    """aim_batch_io_mates_t: BatchIOGroups, then the pairing parameters and the read pairs' rows (AIM_FLAG_MATE_PAIRS); aim_set_submit
    receives a pointer to `groups.base`."""
    _fields_ = [("groups", BatchIOGroups), ("min_span", C.c_int64), ("max_span", C.c_int64), ("unpaired_penalty", C.c_int32),
                ("pad", C.c_uint32), ("mates", C.c_void_p)]


class BatchIOSam(C.Structure):
    """aim_batch_io_sam_t: BatchIOMates at offset 0 (its groups / mates members are read only under their own flags), then the record
    buffers (AIM_FLAG_SAM_FIELDS); aim_set_submit receives a pointer to `mates.groups.base`."""
    _fields_ = [("mates", BatchIOMates), ("sam", C.c_void_p), ("sam_cigar", C.c_void_p), ("sam_cigar_cap", C.c_uint32), ("sam_md", C.c_void_p),
                ("sam_md_cap", C.c_uint32), ("sam_options", C.c_uint32)]


class BatchIOHits(C.Structure):
    """aim_batch_io_hits_t: BatchIOSam at offset 0 (its groups members are read, its mates and sam members ignored), then the hit rows
    (AIM_FLAG_TOP_HITS); aim_set_submit receives a pointer to `sam.mates.groups.base`."""
    _fields_ = [("sam", BatchIOSam), ("max_hits", C.c_uint32), ("pad", C.c_uint32), ("hit_offsets", C.c_void_p), ("hit_pair", C.c_void_p)]


# every symbol include/aim_hip.h declares: name -> (restype, argtypes)
_VP, _U32, _I32 = C.c_void_p, C.c_uint32, C.c_int32
SYMBOLS = {
    "aim_abi_version": (C.c_int, []),
    "aim_features": (C.c_uint32, []),
    "aim_last_error": (C.c_char_p, []),
    "aim_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "aim_set_alloc": (C.c_int, [_U32, C.POINTER(C.c_int), C.POINTER(_VP)]),
    "aim_set_nr_devices": (C.c_int, [_VP, C.POINTER(_U32)]),
    "aim_set_configure": (C.c_int, [_VP, C.POINTER(Params), _U32]),
    "aim_set_push": (C.c_int, [_VP, _U32, _U32, _VP, _VP, _VP]),
    "aim_set_launch": (C.c_int, [_VP]),
    "aim_set_pull": (C.c_int, [_VP, _U32, _VP, _VP]),
    "aim_set_configure_slots": (C.c_int, [_VP, C.POINTER(Params), _U32, _U32, _U32, _U32]),
    "aim_set_submit": (C.c_int, [_VP, _U32, _U32, C.POINTER(BatchIO)]),
    "aim_set_wait": (C.c_int, [_VP, _U32, _U32, C.POINTER(_U32)]),
    "aim_pack_sequence": (C.c_int, [_VP, _I32, _I32, _VP]),
    "aim_pack_batch": (C.c_int, [C.POINTER(Params), _U32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _U32, C.POINTER(_U32), C.c_int]),
    "aim_cigar_format_runs": (C.c_int, [_VP, _U32, _VP, _I32]),
    "aim_set_timers": (C.c_int, [_VP, C.POINTER(C.c_float), C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "aim_set_fallback_pairs": (C.c_int, [_VP, _U32, C.POINTER(_U32)]),
    "aim_set_plan_describe": (C.c_int, [_VP, _U32, C.c_char_p, C.c_size_t]),
    "aim_set_free": (C.c_int, [_VP]),
    "aim_host_alloc": (C.c_int, [C.POINTER(_VP), C.c_size_t]),
    "aim_host_free": (C.c_int, [_VP]),
    "aim_scratch_bytes": (C.c_size_t, [C.POINTER(Params), _U32]),
    "aim_align_device": (C.c_int, [C.POINTER(Params), _U32, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "aim_plan_describe": (C.c_int, [C.POINTER(Params), _U32, C.c_char_p, C.c_size_t]),
    "aim_kernel_name": (C.c_char_p, [C.POINTER(Params)]),
    "aim_launcher_sizes": (C.c_int, [_I32, _I32, C.c_double, _I32, _I32, _I32, _I32, C.POINTER(_I32), C.POINTER(_I32)]),
    "aim_cigar_format": (C.c_int, [_VP, _I32, _I32, _VP, _I32]),
    "aim_gen_pairs": (C.c_int, [C.c_uint64, C.c_uint64, _U32, _I32, C.c_double, _I32, _VP, _VP, _VP]),
    "aim_set_reference": (C.c_int, [_VP, _VP, C.c_uint64]),
    "aim_set_push_ref": (C.c_int, [_VP, _U32, _U32, _VP, _VP, _VP]),
    "aim_ref_windows_check": (C.c_int, [C.POINTER(Params), _U32, _VP, _VP, C.c_uint64, C.POINTER(_U32)]),
    "aim_align_device_ref": (C.c_int, [C.POINTER(Params), _U32, _VP, _VP, _VP, _VP, C.c_uint64, _VP, _VP, _VP, C.c_size_t, _VP]),
    "aim_groups_check": (C.c_int, [_U32, _U32, _VP, C.POINTER(_U32)]),
    "aim_align_device_groups": (C.c_int, [C.POINTER(Params), _U32, _U32, _VP, _VP, _VP, _VP, _VP, C.c_uint64, _VP, _VP, _VP, _VP, _VP,
                                          C.c_size_t, _VP]),
    "aim_mates_check": (C.c_int, [_U32, C.c_int64, C.c_int64, _I32]),
    "aim_align_device_mates": (C.c_int, [C.POINTER(Params), _U32, _U32, _VP, _VP, _VP, _VP, _VP, C.c_uint64, _VP, _VP, _VP, _VP, C.c_int64,
                                         C.c_int64, _I32, _VP, _VP, C.c_size_t, _VP]),
    "aim_hits_offsets": (C.c_int, [_U32, _VP, _U32, _VP, C.POINTER(_U32)]),
    "aim_align_device_hits": (C.c_int, [C.POINTER(Params), _U32, _U32, _VP, _VP, _VP, _VP, _VP, C.c_uint64, _VP, _VP, _VP, _VP, _U32, _VP, _U32,
                                        _VP, _VP, C.c_size_t, _VP]),
    "aim_set_sam_capacity": (C.c_int, [_VP, _U32, _U32]),
    "aim_sam_device": (C.c_int, [C.POINTER(Params), _U32, _VP, _VP, _VP, _VP, _VP, _VP, C.c_uint64, _U32, _VP, _VP, _U32, _VP, _U32, _VP, _VP]),
    "aim_sam_format_cigar": (C.c_int, [_VP, _U32, _VP, _I32]),
    "aim_sam_kernel_name": (C.c_char_p, [C.POINTER(Params)]),
    "aim_index_sizes": (C.c_int, [_I32, C.c_uint64, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "aim_index_build": (C.c_int, [_VP, C.c_uint64, _I32, _VP, _VP, C.POINTER(C.c_uint64), C.c_int]),
    "aim_seed_device": (C.c_int, [C.POINTER(SeedParams), _U32, _VP, _VP, _VP, _VP, C.c_uint64, _VP, _VP, _VP, _VP, _VP]),
    "aim_seed_chain_device": (C.c_int, [C.POINTER(SeedParams), _U32, _VP, _VP, _VP, _VP, C.c_uint64, _VP, _VP, _VP, _VP, _VP, _VP]),
    "aim_seed_chain_kernel_names": (C.c_char_p, []),
    "aim_seed_chain_long_device": (C.c_int, [C.POINTER(SeedParams), _U32, _U32, _VP, _VP, _VP, _VP, C.c_uint64, _VP, _VP, _VP, _VP, _VP, _VP]),
    "aim_seed_chain_long_kernel_name": (C.c_char_p, []),
    "aim_chain_classify_device": (C.c_int, [_U32, _U32, _U32, _U32, _VP, _VP, _VP, _VP, _VP, _VP]),
    "aim_read_mapq_device": (C.c_int, [_U32, _U32, _I32, _VP, _VP, _VP, _VP, _VP]),
    "aim_chain_class_kernel_names": (C.c_char_p, []),
    "aim_split_segments_device": (C.c_int, [_U32, _U32, _I32, C.c_uint64, _U32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "aim_sam_device_split": (C.c_int, [C.POINTER(Params), _U32, _VP, _VP, _VP, _VP, _VP, _VP, C.c_uint64, _U32, _VP, _VP, _U32, _VP, _U32, _VP, _VP, _VP]),
    "aim_split_kernel_names": (C.c_char_p, []),
    "aim_extend_segments_device": (C.c_int, [C.POINTER(ExtendParams), _U32, _U32, C.c_uint64, _U32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "aim_extend_kernel_names": (C.c_char_p, []),
    "aim_seed_groups_offsets": (C.c_int, [_U32, _U32, _VP]),
    "aim_seed_kernel_name": (C.c_char_p, []),
    "aim_index_device_scratch": (C.c_int, [_I32, C.c_uint64, C.POINTER(C.c_uint64)]),
    "aim_index_build_device": (C.c_int, [_VP, C.c_uint64, _I32, _VP, _VP, _VP, C.c_uint64, _VP]),
    "aim_index_kernel_names": (C.c_char_p, []),
    "aim_index_build_minimizers": (C.c_int, [_VP, C.c_uint64, _I32, _I32, _VP, _VP, C.POINTER(C.c_uint64), C.c_int]),
    "aim_index_build_device_minimizers": (C.c_int, [_VP, C.c_uint64, _I32, _I32, _VP, _VP, _VP, C.c_uint64, _VP]),
    "aim_minimizer_kernel_names": (C.c_char_p, []),
    "aim_map_records_scratch": (C.c_size_t, [_U32]),
    "aim_map_records_device": (C.c_int, [_U32, _U32, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "aim_mapper_kernel_names": (C.c_char_p, []),
    "aim_mapper_device_bytes": (C.c_int, [C.POINTER(MapperParams), C.c_uint64, C.POINTER(C.c_uint64)]),
    "aim_mapper_create": (C.c_int, [C.POINTER(MapperParams), C.c_int, _VP, C.c_uint64, C.POINTER(_VP)]),
    "aim_mapper_submit": (C.c_int, [_VP, _U32, _U32, _VP, _VP]),
    "aim_mapper_wait": (C.c_int, [_VP, _U32, C.POINTER(MapperOut)]),
    "aim_mapper_free": (C.c_int, [_VP]),
    "aim_contigs_layout": (C.c_int, [_U32, _VP, _U32, _VP, C.POINTER(C.c_uint64)]),
    "aim_contigs_concat": (C.c_int, [_U32, _VP, _VP, _U32, _VP]),
    "aim_contig_clip_device": (C.c_int, [_U32, _U32, _I32, C.c_uint64, _U32, _VP, _VP, _U32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "aim_map_records_contigs_device": (C.c_int, [_U32, _U32, _VP, _VP, _VP, _VP, _U32, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "aim_contig_kernel_names": (C.c_char_p, []),
    "aim_mapper_device_bytes_contigs": (C.c_int, [C.POINTER(MapperParams), _U32, _VP, C.POINTER(C.c_uint64)]),
    "aim_mapper_create_contigs": (C.c_int, [C.POINTER(MapperParams), C.c_int, _U32, _VP, _VP, C.POINTER(_VP)]),
    "aim_mapper_contigs": (C.c_int, [_VP, C.POINTER(_U32), C.POINTER(_VP), C.POINTER(_VP)]),
    "aim_pair_rescue_rows_device": (C.c_int, [C.POINTER(MapPairParams), _U32, _U32, C.c_uint64, _U32, _VP, _VP, _U32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "aim_pair_select_device": (C.c_int, [C.POINTER(MapPairParams), _U32, _U32, _U32, _VP, _VP, _VP, _VP, _VP, _VP, _U32, _U32, _VP, _VP]),
    "aim_map_mates_device": (C.c_int, [_U32, _U32, _VP, _VP, _VP, _VP, _U32, _VP, _VP, _VP, _VP, _VP]),
    "aim_pair_kernel_names": (C.c_char_p, []),
    "aim_mapper_pairing_device_bytes": (C.c_int, [C.POINTER(MapperParams), C.POINTER(MapPairParams), C.POINTER(C.c_uint64)]),
    "aim_mapper_set_pairing": (C.c_int, [_VP, C.POINTER(MapPairParams)]),
    "aim_mapper_pairs": (C.c_int, [_VP, _U32, C.POINTER(MapperPairsOut)]),
    "aim_pair_estimate_scratch": (C.c_size_t, [_U32]),
    "aim_pair_estimate_device": (C.c_int, [C.POINTER(MapPairParams), C.POINTER(PairEstParams), _U32, _U32, _U32, _VP, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "aim_pair_rescue_rows_device_est": (C.c_int, [C.POINTER(MapPairParams), _U32, _U32, C.c_uint64, _U32, _VP, _VP, _U32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP]),
    "aim_pair_select_device_est": (C.c_int, [C.POINTER(MapPairParams), _U32, _U32, _U32, _VP, _VP, _VP, _VP, _VP, _VP, _U32, _U32, _VP, _VP, _VP]),
    "aim_pair_estimate_kernel_names": (C.c_char_p, []),
    "aim_mapper_set_pairing_estimated": (C.c_int, [_VP, C.POINTER(MapPairParams), C.POINTER(PairEstParams)]),
    "aim_mapper_pair_estimate": (C.c_int, [_VP, _U32, C.POINTER(PairEstimate)]),
    "aim_secondary_rows_device": (C.c_int, [_U32, _U32, _I32, C.c_uint64, _U32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _U32, _VP]),
    "aim_secondary_select_device": (C.c_int, [_U32, _U32, _VP, _VP, _VP, _VP, _I32, _I32, _VP, _VP]),
    "aim_map_records_secondary_device": (C.c_int, [_U32, _U32, _U32, _VP, _VP, _VP, _VP, _VP, _U32, _VP, _VP, _VP, _VP, _VP, C.c_size_t, _VP]),
    "aim_secondary_kernel_names": (C.c_char_p, []),
    "aim_mapper_secondary_device_bytes": (C.c_int, [C.POINTER(MapperParams), C.POINTER(MapSecParams), C.POINTER(C.c_uint64)]),
    "aim_mapper_set_secondary": (C.c_int, [_VP, C.POINTER(MapSecParams)]),
    "aim_mapper_secondary": (C.c_int, [_VP, _U32, C.POINTER(MapperSecondaryOut)]),
    "aim_pair_rescue_rows_secondary_device": (C.c_int, [C.POINTER(MapPairParams), _U32, _U32, C.c_uint64, _U32, _VP, _VP, _U32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _VP,
                                                        _VP]),
    "aim_pair_select_secondary_device": (C.c_int, [C.POINTER(MapPairParams), _U32, _U32, _U32, _VP, _VP, _VP, _VP, _VP, _VP, _VP, _I32, _VP, _U32, _U32, _VP, _VP, _VP, _VP]),
    "aim_map_mates_secondary_device": (C.c_int, [_U32, _U32, _VP, _VP, _VP, _VP, _VP, _U32, _VP, _VP, _VP, _VP, _VP]),
    "aim_pair_secondary_kernel_names": (C.c_char_p, []),
    "aim_mapper_pairing_secondary_device_bytes": (C.c_int, [C.POINTER(MapperParams), C.POINTER(MapPairParams), C.POINTER(MapSecParams), C.POINTER(C.c_uint64)]),
    "aim_mapper_set_pairing_secondary": (C.c_int, [_VP, C.POINTER(MapPairParams), C.POINTER(PairEstParams), C.POINTER(MapSecParams)]),
    "aim_mapper_pair_mapq": (C.c_int, [_VP, _U32, C.POINTER(_VP)]),
}

_lib = None


class AimError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("aim_hip error %d: %s" % (code, message))
        self.code = code


def load(strict=True):
    """Load libaim_hip.so (built by aim_amd.build).  Fails loudly when it is missing. strict=False accepts a library built before
    a declared symbol existed (AIM_LIB=<an older build of this ABI>, for A/B measurements): that symbol is simply absent from it."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError("%s is missing: run `python -m aim_amd.build` (hipcc, gfx950). "
                           "There is no CPU fallback for the alignment path." % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        if not strict and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)   # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc):
    if rc < 0:
        raise AimError(rc, load().aim_last_error().decode(errors="replace"))
    return rc


def ptr(arr):
    """void* of a C-contiguous numpy array (or None)."""
    if arr is None:
        return None
    assert arr.flags["C_CONTIGUOUS"]
    return arr.ctypes.data_as(C.c_void_p)
