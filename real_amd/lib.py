"""ctypes binding of the C ABI in include/real_hip.h (libreal_hip.so).

There is no CPU fallback: if the HIP library is missing or no MI355X is visible,
the calls raise.  PyTorch is only used by callers for device buffers, streams and
torch.distributed -- nothing here depends on it.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("REAL_HIP_LIB") or os.path.join(_HERE, "libreal_hip.so")     # (REAL_HIP_LIB: an experimental build, bench_support/ab_match.py)

REAL_HIP_OK = 0
REAL_HIP_E_INVALID = -1
REAL_HIP_E_NOMEM = -2
REAL_HIP_E_DEVICE = -3
REAL_HIP_E_OVERFLOW = -4
REAL_HIP_E_STATE = -5
REAL_HIP_E_UNSUPPORTED = -6
REAL_HIP_MAX_PATL = 320
REAL_HIP_MAX_PATL_LONG = 16384
REAL_HIP_MATE_SEARCH_MAX_INSERT = 4096   # the widest insert bound the mate search takes
REAL_HIP_INSERT_HIST_MAX_BINS = 16384    # the most bins of an insert-size histogram
REAL_HIP_INSERT_MIN_COUNT = 32           # the fewest valid Unique records `real` takes insert bounds from

K_MATCH_UNIQUE, K_MATCH_ALL, K_ALL_SORT, K_INDEX, K_MATCH_REPEAT, K_PARSE = range(6)
K_PAIR, K_PAIR_WAVE = 6, 7          # the paired-end join: lane per fragment, wave per handed-over fragment
PAIR_NOMATCH, PAIR_UNIQUE, PAIR_NONUNIQUE = range(3)
# resident index layouts, as real_hip_index_table_kind reports them (HipMatcher.table_kind)
LAYOUT_STARTS, LAYOUT_DIGEST, LAYOUT_FINGERPRINT, LAYOUT_ROWS = range(4)

# every symbol include/real_hip.h declares (tests check the library exports all of them)
ABI_SYMBOLS = [
    "real_hip_scoring_table", "real_hip_create", "real_hip_destroy", "real_hip_strerror",
    "real_hip_last_error", "real_hip_abi_version", "real_hip_set_match_params", "real_hip_wait_event", "real_hip_device_memory", "real_hip_set_text", "real_hip_set_text_symbols",
    "real_hip_set_index_block", "real_hip_build_index_block", "real_hip_index_info", "real_hip_index_build_stats",
    "real_hip_index_table_kind", "real_hip_index_download", "real_hip_index_export", "real_hip_match_unique", "real_hip_match_all", "real_hip_match_unique_submit", "real_hip_wait",
    "real_hip_host_alloc", "real_hip_host_free",
    "real_hip_comm_id", "real_hip_comm_init", "real_hip_comm_destroy", "real_hip_gather_records", "real_hip_gather_hits",
    "real_hip_pair_hits", "real_hip_match_pairs", "real_hip_pair_stats_get",
    "real_hip_pair_search", "real_hip_match_pairs_search", "real_hip_mate_search_stats_get",
    "real_hip_pair_all_hits", "real_hip_match_pairs_all", "real_hip_pair_all_stats_get",
    "real_hip_single_hits", "real_hip_match_pairs_singles", "real_hip_single_stats_get",
    "real_hip_pair_insert_hist", "real_hip_insert_bounds", "real_hip_insert_stats_get",
    "real_hip_pileup_begin", "real_hip_pileup_add", "real_hip_pileup_add_pairs", "real_hip_pileup_finish", "real_hip_pileup_depth",
    "real_hip_pileup_sites", "real_hip_pileup_end", "real_hip_pileup_stats_get",
    "real_hip_call_begin", "real_hip_call_add", "real_hip_call_add_pairs", "real_hip_call_finish", "real_hip_call_evidence",
    "real_hip_call_variants", "real_hip_call_end", "real_hip_call_stats_get",
    "real_hip_mismatches", "real_hip_mismatches_pairs", "real_hip_mismatch_stats_get",
    "real_hip_read_summary", "real_hip_mark_duplicates", "real_hip_mark_duplicates_pairs", "real_hip_dup_stats_get",
    "real_hip_mapq_acc_merge", "real_hip_mapq_of", "real_hip_mapq_hits", "real_hip_mapq_pair_hits", "real_hip_match_mapq",
    "real_hip_match_pairs_mapq", "real_hip_mapq", "real_hip_mapq_pairs", "real_hip_mapq_stats_get",
    "real_hip_gap_rescue", "real_hip_gap_cigar", "real_hip_gap_stats_get",
    "real_hip_gap_anchor_hits", "real_hip_match_gapped", "real_hip_gap_anchor_stats_get",
    "real_hip_mismatches_gapped", "real_hip_gapped_list_stats_get",
    "real_hip_indel_begin", "real_hip_indel_add", "real_hip_indel_finish", "real_hip_indel_events", "real_hip_indel_calls",
    "real_hip_indel_end", "real_hip_indel_stats_get",
    "real_hip_pileup_add_gapped", "real_hip_call_add_gapped", "real_hip_pileup_depth_gapped", "real_hip_pileup_gapped_stats_get",
    "real_hip_mark_duplicates_gapped",
    "real_hip_parse_reads", "real_hip_download", "real_hip_counters_get", "real_hip_kernel_time", "real_hip_timing_enable",
]


def sized(struct, **fields):
    """a struct of the ABI with struct_size set and the fields given"""
    return struct(struct_size=C.sizeof(struct), **fields)


def _stats_struct(name: str, fields):
    """a statistics struct of the ABI: struct_size, reserved, then the counts (uint64) and the times (*_ms, double)"""
    return type(name, (C.Structure,), {"_fields_": [("struct_size", C.c_uint32), ("reserved", C.c_uint32)] +
                                                   [(k, C.c_double if k.endswith("_ms") else C.c_uint64) for k in fields]})


def stats_fields(struct):
    """the names a statistics struct reports: everything behind struct_size, reserved"""
    return tuple(k for k, _ in struct._fields_[2:])


class RealHipParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("seedl", C.c_uint32), ("seedkmax", C.c_uint32),
                ("totalkmax", C.c_uint32), ("scores", C.c_uint32), ("prefix_bits", C.c_uint32),
                ("device", C.c_int32), ("table_kind", C.c_uint32), ("filter_mult", C.c_double),
                ("LL", C.c_double * 1024)]


class RealHipBatch(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("on_device", C.c_uint32), ("n_reads", C.c_uint64),
                ("bases", C.c_void_p), ("qual", C.c_void_p), ("offsets", C.c_void_p),
                ("patl", C.c_uint32), ("max_patl", C.c_uint32),
                ("packed", C.c_uint32), ("fresh", C.c_uint32), ("nflags", C.c_void_p)]


class RealHipParsed(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_patl", C.c_uint32), ("n_reads", C.c_uint64), ("n_symbols", C.c_uint64),
                ("bases", C.c_void_p), ("qual", C.c_void_p), ("offsets", C.c_void_p),
                ("id_start", C.c_void_p), ("id_len", C.c_void_p)]


RealHipBuildStats = _stats_struct("RealHipBuildStats", ("wall_ms", "kernel_ms", "alloc_ms", "free_ms", "alloc_bytes", "alloc_calls", "free_calls"))


class RealHipCounters(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("lookups", C.c_uint64), ("probes", C.c_uint64),
                ("candidates", C.c_uint64), ("seedpass", C.c_uint64), ("hits", C.c_uint64),
                ("verified", C.c_uint64), ("handed_over", C.c_uint64)]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class RealHipPairParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_insert", C.c_uint32), ("max_insert", C.c_uint32), ("orientation", C.c_uint32)]


class RealHipMateSearchParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_anchors", C.c_uint32), ("reserved", C.c_uint32 * 2)]


class RealHipInsertEstimate(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("n", C.c_uint64), ("q1", C.c_uint32), ("median", C.c_uint32),
                ("q3", C.c_uint32), ("low", C.c_uint32), ("high", C.c_uint32), ("pad", C.c_uint32)]


# the work of the paired-end stages (real_hip_*_stats)
RealHipPairStats = _stats_struct("RealHipPairStats", ("pairs", "products", "handed_over"))
RealHipMateSearchStats = _stats_struct("RealHipMateSearchStats", ("fragments", "anchors", "anchors_skipped", "positions", "placements",
                                                                  "launches", "kernel_ms"))
RealHipPairAllStats = _stats_struct("RealHipPairAllStats", ("fragments", "products", "pairs_out", "handed_over", "launches", "kernel_ms"))
RealHipSingleStats = _stats_struct("RealHipSingleStats", ("reads", "hits", "handed_over", "launches", "kernel_ms"))
RealHipInsertStats = _stats_struct("RealHipInsertStats", ("records", "counted", "overflow", "invalid", "launches", "kernel_ms"))


class RealHipPileupParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_qual", C.c_uint32)]


class RealHipPileupSite(C.Structure):
    """real_hip_pileup_site: one position where a placed read shows another base than the text (PILEUP_SITE_DTYPE is the same
    record as a numpy dtype)"""
    _fields_ = [("pos", C.c_uint32), ("depth", C.c_uint32), ("alt", C.c_uint32 * 4), ("ref", C.c_uint32), ("reserved", C.c_uint32)]


PILEUP_SITE_DTYPE = np.dtype(RealHipPileupSite)
assert PILEUP_SITE_DTYPE.itemsize == 32

PILEUP_STATS_FIELDS = ("reads", "placed", "other_file", "invalid", "bases", "mismatches", "low_qual", "n_dropped", "covered", "sites",
                       "max_depth", "launches", "kernel_ms")
RealHipPileupStats = _stats_struct("RealHipPileupStats", PILEUP_STATS_FIELDS)


class RealHipCallParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_call_qual", C.c_uint32), ("min_depth", C.c_uint32)]


# the constants of the genotype model (include/real_hip.h, "variant calls")
CALL_HET, CALL_ERR, CALL_PRIOR_HET, CALL_PRIOR_HOM, CALL_PRIOR_HET2 = 3, 5, 30, 33, 60
# real_hip_call_evidence_rec (record s belongs to site s of the pileup) and real_hip_call as numpy dtypes
CALL_EVIDENCE_DTYPE = np.dtype([("cnt", "<u4", (4,)), ("qsum", "<u4", (4,))])
CALL_DTYPE = np.dtype([("pos", "<u4"), ("depth", "<u4"), ("cnt", "<u4", (4,)), ("qual", "<u4"), ("ref", "u1"), ("a1", "u1"), ("a2", "u1"), ("gq", "u1")])
assert CALL_EVIDENCE_DTYPE.itemsize == 32 and CALL_DTYPE.itemsize == 32

CALL_STATS_FIELDS = ("reads", "placed", "other_file", "invalid", "site_bases", "low_qual", "calls", "het", "hom", "launches", "kernel_ms")
RealHipCallStats = _stats_struct("RealHipCallStats", CALL_STATS_FIELDS)


class RealHipMismatch(C.Structure):
    """real_hip_mismatch: one base of a placed read that differs from the text (MISMATCH_DTYPE is the same record as a numpy dtype)"""
    _fields_ = [("off", C.c_uint16), ("ref", C.c_uint8), ("base", C.c_uint8)]


MISMATCH_DTYPE = np.dtype(RealHipMismatch)
assert MISMATCH_DTYPE.itemsize == 4

MISMATCH_STATS_FIELDS = ("reads", "placed", "other_file", "invalid", "bases", "mismatches", "on_n", "disagree", "launches", "kernel_ms")
RealHipMismatchStats = _stats_struct("RealHipMismatchStats", MISMATCH_STATS_FIELDS)


class RealHipReadSum(C.Structure):
    """real_hip_read_sum: a read's length and the sum of its qualities >= min_qual (READ_SUM_DTYPE is the same record as a numpy dtype)"""
    _fields_ = [("len", C.c_uint32), ("qsum", C.c_uint32)]


READ_SUM_DTYPE = np.dtype(RealHipReadSum)
assert READ_SUM_DTYPE.itemsize == 8

DUP_STATS_FIELDS = ("reads", "placed", "groups", "duplicates", "launches", "kernel_ms")
RealHipDupStats = _stats_struct("RealHipDupStats", DUP_STATS_FIELDS)


# mapping quality (include/real_hip.h, "mapping quality"): real_hip_mapq_acc, the in/out accumulator of one read or fragment
MAPQ_LEVELS, MAPQ_MISMATCH_LEVELS, MAPQ_MAX, MAPQ_NONE = 32, 12, 60, 255
MAPQ_EMPTY_LEVEL = -(1 << 31)


class RealHipMapqAcc(C.Structure):
    """real_hip_mapq_acc: the candidates of one read or fragment by level (MAPQ_ACC_DTYPE is the same record as a numpy dtype)"""
    _fields_ = [("level", C.c_int32), ("n", C.c_uint32), ("cnt", C.c_uint8 * MAPQ_LEVELS)]


MAPQ_ACC_DTYPE = np.dtype(RealHipMapqAcc)
assert MAPQ_ACC_DTYPE.itemsize == 40
MAPQ_STATS_FIELDS = ("folded", "candidates", "handed_over", "placements", "unlisted", "launches", "kernel_ms")
RealHipMapqStats = _stats_struct("RealHipMapqStats", MAPQ_STATS_FIELDS)


# gap rescue (include/real_hip.h, "gap rescue"): a mate placed with one insertion or deletion beside its uniquely placed mate
GAP_MAX, GAP_NONE = 16, 0xFFFF


class RealHipGapParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("max_gap", C.c_uint32), ("min_flank", C.c_uint32), ("cost_mismatch", C.c_uint32),
                ("cost_open", C.c_uint32), ("cost_extend", C.c_uint32), ("max_cost", C.c_uint32), ("margin", C.c_uint32),
                ("reserved", C.c_uint32 * 2)]


class RealHipGapPlace(C.Structure):
    """real_hip_gap_place: the record of one fragment (GAP_PLACE_DTYPE is the same record as a numpy dtype); tag = the target
    mate (bit 0) | inverted << 4 | state << 5"""
    _fields_ = [("pos", C.c_uint32), ("frag", C.c_uint16), ("fileid", C.c_uint8), ("tag", C.c_uint8), ("split", C.c_uint16),
                ("gap", C.c_int8), ("k", C.c_uint8), ("cost", C.c_uint16), ("second", C.c_uint16)]


GAP_PLACE_DTYPE = np.dtype(RealHipGapPlace)
assert GAP_PLACE_DTYPE.itemsize == 16
GAP_STATS_FIELDS = ("fragments", "eligible", "other_file", "skipped", "positions", "placed", "unique", "gapped", "launches", "kernel_ms")
RealHipGapStats = _stats_struct("RealHipGapStats", GAP_STATS_FIELDS)
# anchored gap placement (include/real_hip.h, "anchored gap placement"): a single read placed around the hits of its two ends
GAP_ANCHORS_MAX = 64


class RealHipGapAnchorParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("anchor_len", C.c_uint32), ("max_anchors", C.c_uint32), ("reserved", C.c_uint32 * 2)]


GAP_ANCHOR_STATS_FIELDS = ("reads", "eligible", "skipped", "crowded", "unanchored", "anchors", "invalid_anchors", "positions", "placed", "unique",
                           "gapped", "launches", "kernel_ms")
RealHipGapAnchorStats = _stats_struct("RealHipGapAnchorStats", GAP_ANCHOR_STATS_FIELDS)
# gapped mismatch lists (include/real_hip.h, "gapped mismatch lists"): MISMATCH_DTYPE records in the text coordinates of a gap record
MISMATCH_DELETED = 4   # `base` of a text position the read's deletion skips
GAPPED_LIST_STATS_FIELDS = ("fragments", "placed", "other_file", "invalid", "aligned_bases", "mismatches", "deleted", "inserted", "on_n",
                            "disagree", "launches", "kernel_ms")
RealHipGappedListStats = _stats_struct("RealHipGappedListStats", GAPPED_LIST_STATS_FIELDS)

# indel calls (include/real_hip.h, "indel calls"): the rescued mates' insertions and deletions, grouped and genotyped
INDEL_SHIFT_MAX, INDEL_REF_Q, INDEL_PRIOR_HET, INDEL_PRIOR_HOM = 256, 30, 40, 43


class RealHipIndelParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_call_qual", C.c_uint32), ("min_alt", C.c_uint32), ("min_depth", C.c_uint32)]


class RealHipIndel(C.Structure):
    """real_hip_indel: one distinct event of the event list or the call list (INDEL_DTYPE is the same record as a numpy dtype);
    pos = the anchor, seq = the inserted bases 2 bits each, the first lowest"""
    _fields_ = [("pos", C.c_uint32), ("ref_n", C.c_uint32), ("alt_n", C.c_uint32), ("alt_fwd", C.c_uint32), ("qsum", C.c_uint32),
                ("qual", C.c_uint32), ("seq", C.c_uint32), ("gap", C.c_int8), ("gt", C.c_uint8), ("gq", C.c_uint8), ("ref", C.c_uint8)]


INDEL_DTYPE = np.dtype(RealHipIndel)
assert INDEL_DTYPE.itemsize == 32
INDEL_STATS_FIELDS = ("fragments", "placed", "other_file", "invalid", "ungapped", "events", "on_n", "low_qual", "shifted", "shift_capped",
                      "distinct", "calls", "het", "hom", "deletions", "insertions", "launches", "kernel_ms")
RealHipIndelStats = _stats_struct("RealHipIndelStats", INDEL_STATS_FIELDS)
# gapped placements in the pileup and the calls (include/real_hip.h, the block of that name)
PILEUP_GAPPED_STATS_FIELDS = ("records", "placed", "other_file", "invalid", "ungapped", "aligned_bases", "deleted", "inserted", "mismatches",
                              "low_qual", "n_dropped", "site_bases", "site_low_qual", "launches", "kernel_ms")
RealHipPileupGappedStats = _stats_struct("RealHipPileupGappedStats", PILEUP_GAPPED_STATS_FIELDS)


class RealHipPairHit(C.Structure):
    """real_hip_pair_hit: one concordant pair (PAIR_HIT_DTYPE is the same record as a numpy dtype)"""
    _fields_ = [("pair", C.c_uint32), ("pos1", C.c_uint32), ("pos2", C.c_uint32), ("outer", C.c_uint32),
                ("score1", C.c_float), ("score2", C.c_float), ("frag", C.c_uint16), ("fileid", C.c_uint8),
                ("inverted1", C.c_uint8), ("k1", C.c_uint8), ("k2", C.c_uint8), ("reserved", C.c_uint16)]


PAIR_HIT_DTYPE = np.dtype(RealHipPairHit)
assert PAIR_HIT_DTYPE.itemsize == 32

# real_hip_pair: the in/out record of one fragment
PAIR_DTYPE = np.dtype([("best", "<f8"), ("second", "<f8"), ("pos1", "<u4"), ("pos2", "<u4"), ("score1", "<f4"), ("score2", "<f4"),
                       ("frag", "<u2"), ("fileid", "u1"), ("k1", "u1"), ("k2", "u1"), ("inverted1", "u1"), ("state", "u1"),
                       ("reserved", "u1")])
assert PAIR_DTYPE.itemsize == 40

# real_hip_single: the in/out record of one mate on its own; tag = k (bits 0-3) | inverted << 4 | state << 5
SINGLE_DTYPE = np.dtype([("score", "<f4"), ("second", "<f4"), ("pos", "<u4"), ("frag", "<u2"), ("fileid", "u1"), ("tag", "u1")])
assert SINGLE_DTYPE.itemsize == 16


def single_k(tag):
    return np.asarray(tag) & 15


def single_inverted(tag):
    return (np.asarray(tag) >> 4) & 1


def single_state(tag):
    return (np.asarray(tag) >> 5) & 3


HIT_DTYPE = np.dtype([("read", "<u4"), ("pos", "<u4"), ("score", "<f4"), ("frag", "<u2"),
                      ("k", "u1"), ("inverted", "u1")])
assert HIT_DTYPE.itemsize == 16


class RealHipError(RuntimeError):
    def __init__(self, status: int, msg: str):
        super().__init__("real_hip status %d: %s" % (status, msg))
        self.status = status


_lib = None


def load():
    """Load libreal_hip.so; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RealHipError(REAL_HIP_E_DEVICE, "libreal_hip.so is not built: run __graft_entry__.build() "
                                              "(make -C real_amd/csrc); there is no CPU fallback")
    L = C.CDLL(LIB_PATH)
    vp, u64, u32, ci = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    pu64, batch, pairp, searchp = C.POINTER(u64), C.POINTER(RealHipBatch), C.POINTER(RealHipPairParams), C.POINTER(RealHipMateSearchParams)
    L.real_hip_scoring_table.argtypes = [C.c_double] * 5 + [vp]
    L.real_hip_scoring_table.restype = None
    L.real_hip_create.argtypes = [C.POINTER(vp), C.POINTER(RealHipParams)]
    L.real_hip_destroy.argtypes = [vp]
    L.real_hip_destroy.restype = None
    L.real_hip_strerror.argtypes = [ci]
    L.real_hip_strerror.restype = C.c_char_p
    L.real_hip_last_error.argtypes = [vp]
    L.real_hip_last_error.restype = C.c_char_p
    L.real_hip_set_match_params.argtypes = [vp, u32, u32, u32, C.c_double]
    L.real_hip_wait_event.argtypes = [vp, vp]
    L.real_hip_device_memory.argtypes = [vp, pu64, pu64]
    L.real_hip_set_text.argtypes = [vp, u32, vp, vp, u64, vp, u32]
    L.real_hip_set_text_symbols.argtypes = [vp, u32, vp, u64, ci, vp, u32]
    L.real_hip_set_index_block.argtypes = [vp, u64, C.POINTER(vp), C.POINTER(vp)]
    L.real_hip_build_index_block.argtypes = [vp, u64, u64, pu64, C.POINTER(C.c_int)]
    L.real_hip_index_build_stats.argtypes = [vp, C.POINTER(RealHipBuildStats), ci]
    L.real_hip_index_info.argtypes = [vp, pu64, C.POINTER(u32)]
    L.real_hip_index_table_kind.argtypes = [vp, C.POINTER(u32)]
    L.real_hip_parse_reads.argtypes = [vp, vp, u64, ci, ci, ci, C.POINTER(RealHipParsed)]
    L.real_hip_download.argtypes = [vp, vp, vp, C.c_size_t]
    L.real_hip_index_download.argtypes = [vp, ci, vp, vp]
    L.real_hip_index_export.argtypes = [vp, ci, vp, vp]
    L.real_hip_match_unique.argtypes = [vp, batch, vp, vp]
    L.real_hip_match_unique_submit.argtypes = [vp, batch, vp, vp, u32, ci]
    L.real_hip_wait.argtypes = [vp, u32]
    L.real_hip_host_alloc.argtypes = [C.c_size_t]
    L.real_hip_host_alloc.restype = vp
    L.real_hip_host_free.argtypes = [vp]
    L.real_hip_host_free.restype = None
    L.real_hip_comm_id.argtypes = [vp]
    L.real_hip_comm_init.argtypes = [vp, vp, ci, ci]
    L.real_hip_comm_destroy.argtypes = [vp]
    L.real_hip_gather_records.argtypes = [vp, ci, vp, vp, u64, vp, vp, u64, pu64]
    L.real_hip_gather_hits.argtypes = [vp, ci, vp, vp, u64, u64, vp, u64, vp, u64, pu64, pu64]
    L.real_hip_match_all.argtypes = [vp, batch, vp, u64, pu64, vp]
    L.real_hip_pair_hits.argtypes = [vp, pairp, vp, vp, vp, vp, vp, vp, u64, u32, ci, ci, vp]
    L.real_hip_match_pairs.argtypes = [vp, batch, batch, pairp, vp]
    L.real_hip_pair_stats_get.argtypes = [vp, C.POINTER(RealHipPairStats), ci]
    L.real_hip_pair_search.argtypes = [vp, pairp, searchp, batch, batch, vp, vp, vp, vp, u32, ci, vp]
    L.real_hip_match_pairs_search.argtypes = [vp, batch, batch, pairp, searchp, vp]
    L.real_hip_mate_search_stats_get.argtypes = [vp, C.POINTER(RealHipMateSearchStats), ci]
    L.real_hip_pair_all_hits.argtypes = [vp, pairp, vp, vp, vp, vp, vp, vp, u64, u32, ci, vp, u64, pu64, vp]
    L.real_hip_match_pairs_all.argtypes = [vp, batch, batch, pairp, vp, u64, pu64, vp]
    L.real_hip_pair_all_stats_get.argtypes = [vp, C.POINTER(RealHipPairAllStats), ci]
    L.real_hip_single_hits.argtypes = [vp, vp, vp, vp, u64, u32, ci, ci, vp]
    L.real_hip_match_pairs_singles.argtypes = [vp, batch, batch, pairp, searchp, vp, vp, vp]
    L.real_hip_single_stats_get.argtypes = [vp, C.POINTER(RealHipSingleStats), ci]
    L.real_hip_pair_insert_hist.argtypes = [vp, vp, vp, vp, u64, ci, ci, u32, vp]
    L.real_hip_insert_bounds.argtypes = [vp, u32, u64, u32, C.POINTER(RealHipInsertEstimate)]
    L.real_hip_insert_stats_get.argtypes = [vp, C.POINTER(RealHipInsertStats), ci]
    L.real_hip_pileup_begin.argtypes = [vp, C.POINTER(RealHipPileupParams)]
    L.real_hip_pileup_add.argtypes = [vp, batch, vp]
    L.real_hip_pileup_add_pairs.argtypes = [vp, batch, batch, vp]
    L.real_hip_pileup_finish.argtypes = [vp, pu64]
    L.real_hip_pileup_depth.argtypes = [vp, u64, u64, vp, ci]
    L.real_hip_pileup_sites.argtypes = [vp, vp, u64, pu64, ci]
    L.real_hip_pileup_end.argtypes = [vp]
    L.real_hip_pileup_stats_get.argtypes = [vp, C.POINTER(RealHipPileupStats), ci]
    L.real_hip_call_begin.argtypes = [vp]
    L.real_hip_call_add.argtypes = [vp, batch, vp]
    L.real_hip_call_add_pairs.argtypes = [vp, batch, batch, vp]
    L.real_hip_call_finish.argtypes = [vp, C.POINTER(RealHipCallParams), pu64]
    L.real_hip_call_evidence.argtypes = [vp, vp, u64, pu64, ci]
    L.real_hip_call_variants.argtypes = [vp, vp, u64, pu64, ci]
    L.real_hip_call_end.argtypes = [vp]
    L.real_hip_call_stats_get.argtypes = [vp, C.POINTER(RealHipCallStats), ci]
    L.real_hip_mismatches.argtypes = [vp, batch, vp, vp, u64, pu64, vp]
    L.real_hip_mismatches_pairs.argtypes = [vp, batch, batch, vp, vp, vp, vp, u64, pu64, vp]
    L.real_hip_mismatch_stats_get.argtypes = [vp, C.POINTER(RealHipMismatchStats), ci]
    L.real_hip_read_summary.argtypes = [vp, batch, u32, vp]
    L.real_hip_mark_duplicates.argtypes = [vp, vp, vp, u64, ci, vp]
    L.real_hip_mark_duplicates_pairs.argtypes = [vp, vp, vp, vp, u64, ci, vp]
    L.real_hip_mark_duplicates_gapped.argtypes = [vp, vp, vp, vp, u64, ci, vp]
    L.real_hip_dup_stats_get.argtypes = [vp, C.POINTER(RealHipDupStats), ci]
    L.real_hip_mapq_acc_merge.argtypes = [vp, vp]
    L.real_hip_mapq_of.argtypes = [vp, C.c_int32, C.POINTER(ci)]
    L.real_hip_mapq_hits.argtypes = [vp, vp, vp, u64, ci, ci, vp]
    L.real_hip_mapq_pair_hits.argtypes = [vp, pairp, vp, vp, vp, vp, vp, vp, u64, ci, ci, vp]
    L.real_hip_match_mapq.argtypes = [vp, batch, vp]
    L.real_hip_match_pairs_mapq.argtypes = [vp, batch, batch, pairp, searchp, vp, vp, vp, vp, vp, vp]
    L.real_hip_mapq.argtypes = [vp, vp, vp, vp, u64, ci, vp]
    L.real_hip_mapq_pairs.argtypes = [vp, vp, vp, vp, vp, vp, vp, u64, ci, vp]
    L.real_hip_mapq_stats_get.argtypes = [vp, C.POINTER(RealHipMapqStats), ci]
    L.real_hip_gap_rescue.argtypes = [vp, pairp, C.POINTER(RealHipGapParams), batch, batch, vp, vp, vp, ci, vp]
    L.real_hip_gap_cigar.argtypes = [vp, u32, C.c_char_p, C.c_size_t]
    L.real_hip_gap_stats_get.argtypes = [vp, C.POINTER(RealHipGapStats), ci]
    L.real_hip_gap_anchor_hits.argtypes = [vp, C.POINTER(RealHipGapParams), C.POINTER(RealHipGapAnchorParams), batch, vp, vp, vp, ci, vp]
    L.real_hip_match_gapped.argtypes = [vp, C.POINTER(RealHipGapParams), C.POINTER(RealHipGapAnchorParams), batch, vp, ci, vp]
    L.real_hip_gap_anchor_stats_get.argtypes = [vp, C.POINTER(RealHipGapAnchorStats), ci]
    L.real_hip_mismatches_gapped.argtypes = [vp, batch, batch, vp, vp, u64, pu64, vp]
    L.real_hip_gapped_list_stats_get.argtypes = [vp, C.POINTER(RealHipGappedListStats), ci]
    L.real_hip_indel_begin.argtypes = [vp]
    L.real_hip_indel_add.argtypes = [vp, batch, batch, vp]
    L.real_hip_indel_finish.argtypes = [vp, C.POINTER(RealHipIndelParams), pu64, pu64]
    L.real_hip_indel_events.argtypes = [vp, vp, u64, pu64, ci]
    L.real_hip_indel_calls.argtypes = [vp, vp, u64, pu64, ci]
    L.real_hip_indel_end.argtypes = [vp]
    L.real_hip_indel_stats_get.argtypes = [vp, C.POINTER(RealHipIndelStats), ci]
    L.real_hip_pileup_add_gapped.argtypes = [vp, batch, batch, vp]
    L.real_hip_call_add_gapped.argtypes = [vp, batch, batch, vp]
    L.real_hip_pileup_depth_gapped.argtypes = [vp, u64, u64, vp, ci]
    L.real_hip_pileup_gapped_stats_get.argtypes = [vp, C.POINTER(RealHipPileupGappedStats), ci]
    L.real_hip_counters_get.argtypes = [vp, C.POINTER(RealHipCounters), ci]
    L.real_hip_kernel_time.argtypes = [vp, ci, C.POINTER(C.c_double), pu64, ci]
    L.real_hip_timing_enable.argtypes = [vp, ci]
    _lib = L
    return L


def scoring_table(similarity=0.995, gc=0.41, trans=0.71, err=0.0, gcmut_bias=2.0) -> np.ndarray:
    """Scoring::init defaults: Scoring.cpp:204-208."""
    LL = np.zeros(1024, dtype=np.float64)
    load().real_hip_scoring_table(similarity, gc, trans, err, gcmut_bias, LL.ctypes.data)
    return LL


def gap_cigar(rec, length: int) -> str:
    """real_hip_gap_cigar (host only): the CIGAR of one GAP_PLACE_DTYPE record of a read of `length` bases"""
    r = np.ascontiguousarray(np.array(rec, dtype=GAP_PLACE_DTYPE).reshape(1))
    buf = C.create_string_buffer(48)
    rc = load().real_hip_gap_cigar(r.ctypes.data, int(length), buf, len(buf))
    if rc < 0:
        raise RealHipError(rc, "real_hip_gap_cigar")
    return buf.value.decode()


def mapq_acc_merge(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """real_hip_mapq_acc_merge (host only): the merge of two accumulators (MAPQ_ACC_DTYPE records of one element) as a new one"""
    out = np.array(a, dtype=MAPQ_ACC_DTYPE).reshape(1).copy()
    other = np.ascontiguousarray(np.array(b, dtype=MAPQ_ACC_DTYPE).reshape(1))
    rc = load().real_hip_mapq_acc_merge(out.ctypes.data, other.ctypes.data)
    if rc != REAL_HIP_OK:
        raise RealHipError(rc, "invalid argument")
    return out[0]


def mapq_of(acc: np.ndarray, level: int):
    """real_hip_mapq_of (host only): (quality, unlisted) of a placement of `level` against one accumulator"""
    rec = np.ascontiguousarray(np.array(acc, dtype=MAPQ_ACC_DTYPE).reshape(1))
    unlisted = C.c_int(0)
    q = load().real_hip_mapq_of(rec.ctypes.data, int(level), C.byref(unlisted))
    if q < 0:
        raise RealHipError(q, "invalid argument")
    return int(q), bool(unlisted.value)


def _ptr(a) -> Optional[int]:
    """host numpy array, torch tensor (host or device) or raw int address -> address."""
    if a is None:
        return None
    if isinstance(a, int):
        return a
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    raise TypeError(type(a))
