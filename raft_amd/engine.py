"""ctypes binding of the C ABI in ``include/raft_hip.h`` (libraft_hip.so).

This is the host-side mirror of the seam the engine replaces in the reference --
``create_pileup`` / ``repeat_annotate`` / ``break_reads`` (chop.hpp:366-372) -- for Python
callers (tests, bench.py, the multi-GPU driver).  There is no CPU fallback: if the HIP
library is missing or no gfx950 device is present, construction fails.
"""
from __future__ import annotations

import ctypes as C
import operator
import os
from dataclasses import dataclass

import numpy as np

from . import _marshal as M
from .params import RaftParams

_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libraft_hip.so")

OK, ERR_PARAM, ERR_READ_ID, ERR_COORD, ERR_FRAGMENT, ERR_NOMEM, ERR_DEVICE, ERR_STATE, ERR_TOO_LARGE = range(9)
# Summary.flags (RAFT_HIP_SUM_*)
SUM_BUCKET_WINDOWS, SUM_SPECULATED, SUM_DEEP_TILES, SUM_RERUN, SUM_KEPT_GEOMETRY, SUM_GRADED_RANGES = 1, 2, 4, 8, 16, 32

COV_HIST_BINS = 4096              # RAFT_HIP_COV_HIST_BINS
LOW_INTERIOR, LOW_HEAD, LOW_TAIL, LOW_UNCOVERED = 1, 2, 4, 8    # RAFT_HIP_LOW_*: bits of low_flags (Engine.low_coverage)
# RAFT_HIP_OVL_*: bits of a record's class byte and of read_flags (Engine.repeat_overlaps)
OVL_Q_REPEAT, OVL_T_REPEAT, OVL_Q_TOUCH, OVL_T_TOUCH, OVL_Q_CONTAINED, OVL_T_CONTAINED = 1, 2, 4, 8, 16, 32
OVL_READ_CONTAINED, OVL_READ_ANCHORED = 1, 2


class _Params(C.Structure):
    _fields_ = [("reso", C.c_int32), ("est_cov", C.c_int32), ("cov_mul", C.c_double),
                ("repeat_length", C.c_int32), ("interval_length", C.c_int32), ("read_length", C.c_int32),
                ("overlap_length", C.c_int32), ("flanking_length", C.c_int32), ("symmetric_mode", C.c_int32)]


class _Summary(C.Structure):
    _fields_ = [("n_reads", C.c_int32), ("symmetric", C.c_int32), ("high_cov", C.c_int32),
                ("interval_path", C.c_int32), ("n_segments", C.c_int32),
                ("n_records", C.c_int64), ("n_intervals", C.c_int64), ("n_bins", C.c_int64),
                ("n_repeats", C.c_int64), ("n_cuts", C.c_int64), ("n_fragments", C.c_int64),
                ("total_coverage", C.c_int64), ("total_windows", C.c_int64),
                ("total_repeat_length", C.c_int64), ("total_read_length", C.c_int64),
                ("error_index", C.c_int64), ("n_devices_used", C.c_int32), ("flags", C.c_int32)]


class _HostOutputs(C.Structure):
    _fields_ = [("cov_offset", C.c_void_p), ("cov8", C.c_void_p), ("cov8_cap", C.c_int64),
                ("exc_index", C.c_void_p), ("exc_value", C.c_void_p), ("exc_cap", C.c_int64), ("n_exc", C.c_int64),
                ("rep_offset", C.c_void_p), ("rep_s", C.c_void_p), ("rep_e", C.c_void_p), ("rep_cap", C.c_int64),
                ("frag_offset", C.c_void_p), ("frag_begin", C.c_void_p), ("frag_end", C.c_void_p), ("frag_cap", C.c_int64),
                ("cov_width", C.c_int32), ("reserved", C.c_int32), ("cov_anchor", C.c_void_p), ("anchor_cap", C.c_int64)]


class _Slice(C.Structure):
    _fields_ = [("n_rec", C.c_int64), ("n_runs", C.c_int32), ("rec_offset", C.c_void_p), ("d_qs", C.c_void_p), ("d_qe", C.c_void_p),
                ("d_rec_offset", C.c_void_p)]


class _Records(C.Structure):
    _fields_ = [("n_rec", C.c_int64)] + [(n, C.c_void_p) for n in ("d_qid", "d_qs", "d_qe", "d_tid", "d_ts", "d_te")]


class _Received(C.Structure):
    _fields_ = [("n_reads", C.c_int32), ("n_runs", C.c_int32), ("n_rec", C.c_int64), ("d_rec_offset", C.c_void_p), ("d_qs", C.c_void_p),
                ("d_qe", C.c_void_p)]


class _CovEstimate(C.Structure):
    _fields_ = [("est_cov", C.c_int32), ("median", C.c_int32), ("windows", C.c_int64), ("windows_covered", C.c_int64),
                ("windows_clamped", C.c_int64), ("mean", C.c_double)]


def _counts_struct(name: str, *fields):
    """A summary structure of a query: 64-bit counts, in the order of its header."""
    return type(name, (C.Structure,), {"_fields_": [(f, C.c_int64) for f in fields]})


_LowSummary = _counts_struct("_LowSummary", "n_runs", "low_windows", "low_bases", "reads_with_runs", "reads_interior", "reads_uncovered")
_OvlSummary = _counts_struct("_OvlSummary", "n_records", "q_touch", "t_touch", "q_repeat", "t_repeat", "both_repeat", "q_contained", "t_contained",
                             "reads_contained", "reads_repeat_contained")
_FragSummary = _counts_struct("_FragSummary", "n_records", "n_fragments", "frags_untouched", "frags_spanned", "frags_contained",
                              "frags_contained_repeat", "reads_whole_spanned", "reads_any_contained", "reads_all_contained")
_RstSummary = _counts_struct("_RstSummary", "n_runs", "runs_empty", "runs_interior", "runs_touched", "runs_spanned", "interior_spanned",
                             "sides_touch", "sides_span", "sides_inside", "windows", "cov_sum")
_FltSummary = _counts_struct("_FltSummary", "n_records", "n_kept", "below_identity", "below_span", "first_kept", "symmetric")
_EndSummary = _counts_struct("_EndSummary", "n_records", "kind_invalid", "kind_internal", "kind_query_contained", "kind_target_contained", "kind_end3",
                             "kind_end5", "kind_self", "reads_linked", "reads_contained", "reads_isolated", "reads_dead5", "reads_dead3")
_BestSummary = _counts_struct("_BestSummary", "n_records", "candidates", "left_out", "ends_best", "ends_mutual", "reads_both_best",
                              "reads_both_mutual", "reads_no_best", "reads_skipped")
_UtgSummary = _counts_struct("_UtgSummary", "reads_in", "reads_skipped", "unitigs", "singletons", "circular", "longest_reads", "longest_length",
                             "total_length")
_LiftSummary = _counts_struct("_LiftSummary", "n_records", "n_out", "records_none", "records_cut", "pairs_dropped", "most_per_record")
_CcSummary = _counts_struct("_CcSummary", "n_reads", "n_records", "edge_records", "components", "singletons", "largest_reads", "largest_bases",
                            "total_bases", "reads_in_largest_permille")
_SgSummary = _counts_struct("_SgSummary", "records", "dovetail_views", "views_left_out", "arcs", "duplicate_arcs", "unpaired_arcs", "reducible_arcs",
                            "edges", "removed_edges", "kept_edges", "ends_with_arc", "ends_kept_one", "ends_kept_more", "ends_mutual", "ends_dead",
                            "reads_flagged", "longest_row")
_CtnSummary = _counts_struct("_CtnSummary", "records", "containment_views", "views_not_longer", "reads_with_parent", "orphans", "roots",
                             "roots_with_tree", "greatest_depth", "largest_tree_reads", "largest_tree_bases", "launches")
_PlaceSummary = _counts_struct("_PlaceSummary", "n_reads", "n_unitigs", "placed", "unplaced", "unitigs_gained", "greatest_depth_permille")
_ClnSummary = _counts_struct("_ClnSummary", "reads", "reads_flagged", "edges", "weak_arcs", "weak_edges", "rounds_run", "converged", "tips", "tip_reads",
                             "tip_bases", "tip_edges", "candidates_kept", "isolated_short", "kept_edges", "ends_kept_one", "ends_kept_more",
                             "ends_mutual", "ends_dead", "longest_row")


class _FragTable(C.Structure):      # raft_hip_frag_table and raft_hip_frag_repeats: a count and the three arrays of a CSR table
    _fields_ = [("n", C.c_int64), ("offset", C.c_void_p), ("first", C.c_void_p), ("second", C.c_void_p)]


class _Outputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("cov_offset", "cov", "rep_offset", "rep_s", "rep_e", "cut_offset", "cuts",
                                          "frag_offset", "frag_read", "frag_begin", "frag_end")]


_vp, _i32, _i64, _f64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
_P = C.POINTER
_COLUMNS = [_i32, _vp, _i64] + [_vp] * 6                    # n_reads, read_len, n_rec, qid, qs, qe, tid, ts, te
_GROUPED = [_i32, _vp, _i64, _i32, _vp]                     # n_reads, read_len, n_rec, n_runs, rec_offset
_JOB = [_P(_HostOutputs), _P(_Summary)]
_CENSUS = [_vp] + _COLUMNS + [_i32, _vp, _vp, _P(_i64), _P(_i64), _P(_f64)]

# The C ABI: every entry point of include/raft_hip.h, in the header's order, as (restype, argtypes).  load_library declares
# exactly this; tests/test_binding_tables.py compares it with the header, class by class.
ABI = {
    "raft_hip_abi_version": (C.c_int, []),
    "raft_hip_strerror": (C.c_char_p, [C.c_int]),
    "raft_hip_last_error": (C.c_char_p, [_vp]),
    "raft_hip_create": (C.c_int, [C.c_int, _P(_Params), _P(_vp)]),
    "raft_hip_destroy": (None, [_vp]),
    "raft_hip_set_params": (C.c_int, [_vp, _P(_Params)]),
    "raft_hip_set_stream": (C.c_int, [_vp, _vp]),
    "raft_hip_use_own_stream": (C.c_int, [_vp]),
    "raft_hip_get_stream": (_vp, [_vp]),
    "raft_hip_run_device": (C.c_int, [_vp] + _COLUMNS),
    "raft_hip_run_host": (C.c_int, [_vp] + _COLUMNS),
    "raft_hip_run_device_grouped": (C.c_int, [_vp] + _GROUPED + [_vp, _vp, _vp, _i64]),
    "raft_hip_run_host_grouped": (C.c_int, [_vp] + _GROUPED + [_vp, _vp, _i64]),
    "raft_hip_run_device_windows": (C.c_int, [_vp] + _GROUPED + [_vp, _i64]),
    "raft_hip_run_host_windows": (C.c_int, [_vp] + _GROUPED + [_vp, _i64]),
    "raft_hip_finish": (C.c_int, [_vp, _P(_Summary)]),
    "raft_hip_outputs_device": (C.c_int, [_vp, _P(_Outputs)]),
    "raft_hip_fetch": (C.c_int, [_vp] + [_vp] * 11),
    "raft_hip_fetch_packed": (C.c_int, [_vp, _vp, _vp, _i64, _vp, _vp, _P(_i64)] + [_vp] * 7),
    "raft_hip_fetch_packed_w": (C.c_int, [_vp, _i32, _vp, _vp, _i64, _vp, _vp, _P(_i64)] + [_vp] * 7),
    "raft_hip_fetch_delta4": (C.c_int, [_vp, _vp, _vp, _vp, _i64, _vp, _vp, _P(_i64)] + [_vp] * 7),
    "raft_hip_set_output_width": (C.c_int, [_vp, _i32]),
    "raft_hip_set_emit_cuts": (C.c_int, [_vp, _i32]),
    "raft_hip_device_alloc": (C.c_int, [_vp, _i64, _P(_vp)]),
    "raft_hip_device_free": (C.c_int, [_vp, _vp]),
    "raft_hip_trim": (_i64, [C.c_int, _i64]),
    "raft_hip_pool_bytes": (_i64, [C.c_int]),
    "raft_hip_set_placement": (_i32, [_i32]),
    "raft_hip_set_placement_trial": (C.c_int, [_vp, _i32]),
    "raft_hip_placement_trial": (C.c_int, [_vp, _P(_f64), _P(_f64), _P(_i32)]),
    "raft_hip_packed_device": (C.c_int, [_vp, _P(_i32), _P(_vp), _P(_vp), _P(_vp), _P(_i64)]),
    "raft_hip_packed_anchor_device": (C.c_int, [_vp, _P(_vp), _P(_i64)]),
    "raft_hip_run_pipelined": (C.c_int, [_vp] + _COLUMNS + [_i32] + _JOB),
    "raft_hip_run_multi": (C.c_int, [_P(_vp), _i32] + _COLUMNS + [_i32] + _JOB),
    "raft_hip_run_multi_grouped": (C.c_int, [_P(_vp), _i32] + _GROUPED + [_vp, _vp, _i32] + _JOB),
    "raft_hip_run_multi_windows": (C.c_int, [_P(_vp), _i32] + _GROUPED + [_vp, _i32] + _JOB),
    "raft_hip_comm_unique_id": (C.c_int, [_vp]),
    "raft_hip_comm_create": (C.c_int, [C.c_int, _vp, _i32, _i32, _P(_vp)]),
    "raft_hip_comm_destroy": (None, [_vp]),
    "raft_hip_exchange": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _vp, _P(_Slice), _P(_Received)]),
    "raft_hip_exchange_local": (C.c_int, [_P(_vp), _i32, _i32, _vp, _P(_Slice), _P(_Received)]),
    "raft_hip_group_sides": (C.c_int, [_vp, _i32, _i64] + [_vp] * 6 + [_i32, _P(_Slice)]),
    "raft_hip_presplit_symmetric": (C.c_int, [_vp, _vp, _i32, _i32, _P(_Records), _P(_i32)]),
    "raft_hip_presplit_symmetric_local": (C.c_int, [_P(_vp), _i32, _P(_Records), _P(_i32)]),
    "raft_hip_run_presplit_local": (C.c_int, [_P(_vp), _i32] + _COLUMNS + _JOB),
    "raft_hip_host_register": (C.c_int, [_vp, C.c_uint64]),
    "raft_hip_host_unregister": (C.c_int, [_vp]),
    "raft_hip_warm_up": (C.c_int, [_vp]),
    "raft_hip_reserve": (C.c_int, [_vp, _i32, _vp, _i64, _i32, _i32]),
    "raft_hip_cov_histogram": (C.c_int, [_vp, _vp, _P(_f64)]),
    "raft_hip_estimate_coverage": (C.c_int, [_vp, _i32, _P(_CovEstimate)]),
    "raft_hip_read_stats": (C.c_int, [_vp, _i32, _vp, _vp, _vp, _P(_f64)]),
    "raft_hip_census_device": (C.c_int, _CENSUS),
    "raft_hip_census_host": (C.c_int, _CENSUS),
    "raft_hip_last_timing": (C.c_int, [_vp, _P(_f64), _P(_f64)]),
    "raft_hip_set_tuning": (C.c_int, [_vp, _i32, _i32, _i32]),
    "raft_hip_selftest": (C.c_int, [C.c_int]),
}
EXPORTS = tuple(ABI)

# ... and the entry points of include/raft_hip_low.h (libraft_hip_low.so, beside libraft_hip.so): load_side_library("low") declares these
LOW_ABI = {
    "raft_hip_low_abi": (C.c_int, []),
    "raft_hip_low_coverage": (C.c_int, [_vp, _i32, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _P(_LowSummary), _P(_f64)]),
}

# ... and those of include/raft_hip_ovl.h (libraft_hip_ovl.so): load_side_library("ovl") declares these
_OVL_CALL = [_vp, _i32, _vp, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _P(_OvlSummary), _P(_i64), _P(_f64)]
OVL_ABI = {
    "raft_hip_ovl_abi": (C.c_int, []),
    "raft_hip_repeat_overlaps_device": (C.c_int, _OVL_CALL),
    "raft_hip_repeat_overlaps_host": (C.c_int, _OVL_CALL),
}

# ... and those of include/raft_hip_frag.h (libraft_hip_frag.so): load_side_library("frag") declares these
_FRAG_CALL = [_vp, _i32, _vp, _P(_Records), _i32, _P(_FragTable), _P(_FragTable), _vp, _vp, _vp, _vp, _vp, _P(_FragSummary), _P(_i64), _P(_f64)]
FRAG_ABI = {
    "raft_hip_frag_abi": (C.c_int, []),
    "raft_hip_frag_overlaps_device": (C.c_int, _FRAG_CALL),
    "raft_hip_frag_overlaps_host": (C.c_int, _FRAG_CALL),
}

# ... and those of include/raft_hip_rst.h (libraft_hip_rst.so): load_side_library("rst") declares these
_RST_CALL = [_vp, _i32, _vp, _P(_Records), _i32, _i64, _vp, _vp, _vp, _i32] + [_vp] * 9 + [_P(_RstSummary), _P(_i64), _P(_f64)]
RST_ABI = {
    "raft_hip_rst_abi": (C.c_int, []),
    "raft_hip_repeat_stats_device": (C.c_int, _RST_CALL),
    "raft_hip_repeat_stats_host": (C.c_int, _RST_CALL),
}
RST_EMPTY, RST_AT_START, RST_AT_END = 1, 2, 4

# ... and those of include/raft_hip_flt.h (libraft_hip_flt.so): load_side_library("flt") declares these
_FLT_CALL = [_vp, _i64] + [_vp] * 8 + [_i32, _i32] + [_vp] * 6 + [_P(_FltSummary), _P(_f64)]
FLT_ABI = {
    "raft_hip_flt_abi": (C.c_int, []),
    "raft_hip_filter_overlaps_device": (C.c_int, _FLT_CALL),
    "raft_hip_filter_overlaps_host": (C.c_int, _FLT_CALL),
}

# ... and those of include/raft_hip_end.h (libraft_hip_end.so): load_side_library("end") declares these
_END_CALL = [_vp] + _COLUMNS + [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _P(_EndSummary), _P(_i64), _P(_f64)]
END_ABI = {
    "raft_hip_end_abi": (C.c_int, []),
    "raft_hip_overlap_ends_device": (C.c_int, _END_CALL),
    "raft_hip_overlap_ends_host": (C.c_int, _END_CALL),
}
# the kinds of a record and the statuses of a read (RAFT_HIP_END_*, RAFT_HIP_END_READ_*), and the rows of the counts table
END_INVALID, END_INTERNAL, END_QUERY_CONTAINED, END_TARGET_CONTAINED, END_QUERY_3, END_QUERY_5, END_SELF = range(7)
END_READ_LINKED, END_READ_CONTAINED, END_READ_ISOLATED, END_READ_DEAD5, END_READ_DEAD3 = range(5)
END_COUNTS = ("internal", "contained_in", "contains", "end5", "end3")

# ... and those of include/raft_hip_best.h (libraft_hip_best.so): load_side_library("best") declares these
_BEST_CALL = [_vp] + _COLUMNS + [_vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _P(_BestSummary), _P(_i64), _P(_f64)]
BEST_ABI = {
    "raft_hip_best_abi": (C.c_int, []),
    "raft_hip_best_overlaps_device": (C.c_int, _BEST_CALL),
    "raft_hip_best_overlaps_host": (C.c_int, _BEST_CALL),
}
# the bits of a read's flag byte (RAFT_HIP_BEST_*)
BEST_REV5, BEST_MUTUAL5, BEST_REV3, BEST_MUTUAL3, BEST_SKIPPED = 1, 2, 4, 8, 16

# ... and those of include/raft_hip_utg.h (libraft_hip_utg.so): load_side_library("utg") declares these
_UTG_CALL = [_vp, _i32] + [_vp] * 4 + [_vp] * 9 + [_P(_UtgSummary), _P(_i64), _P(_f64), _P(_i64)]
UTG_ABI = {
    "raft_hip_utg_abi": (C.c_int, []),
    "raft_hip_unitigs_device": (C.c_int, _UTG_CALL),
    "raft_hip_unitigs_host": (C.c_int, _UTG_CALL),
}
UTG_MAX_READS = (1 << 30) - 1     # half-edge ids are int32

# ... and those of include/raft_hip_lift.h (libraft_hip_lift.so): load_side_library("lift") declares these
_LIFT_CALL = [_vp, _i32, _P(_Records), _vp, _P(_FragTable), _i32, _i64] + [_vp] * 8 + [_P(_LiftSummary), _P(_i64), _P(_f64)]
LIFT_ABI = {
    "raft_hip_lift_abi": (C.c_int, []),
    "raft_hip_lift_overlaps_device": (C.c_int, _LIFT_CALL),
    "raft_hip_lift_overlaps_host": (C.c_int, _LIFT_CALL),
}
LIFT_COLUMNS = ("qfrag", "qs", "qe", "tfrag", "ts", "te", "rev", "src")      # int32, but for rev: uint8

# ... and those of include/raft_hip_cc.h (libraft_hip_cc.so): load_side_library("cc") declares these
_CC_CALL = [_vp] + _COLUMNS + [_vp, _i32, _i32, _i32, _i32] + [_vp] * 6 + [_P(_CcSummary), _P(_i64), _P(_f64), _P(_i64)]
CC_ABI = {
    "raft_hip_cc_abi": (C.c_int, []),
    "raft_hip_components_device": (C.c_int, _CC_CALL),
    "raft_hip_components_host": (C.c_int, _CC_CALL),
}
# the masks of kinds that count as edges (RAFT_HIP_CC_KINDS_*): containments and dovetails; those and the internal matches
CC_KINDS_PROPER, CC_KINDS_ALL = 60, 62

# ... and those of include/raft_hip_sg.h (libraft_hip_sg.so): load_side_library("sg") declares these
_SG_CALL = [_vp] + _COLUMNS + [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i64] + [_vp] * 11 + [_P(_i64), _P(_SgSummary), _P(_i64), _P(_f64), _P(_i64)]
SG_ABI = {
    "raft_hip_sg_abi": (C.c_int, []),
    "raft_hip_string_graph_device": (C.c_int, _SG_CALL),
    "raft_hip_string_graph_host": (C.c_int, _SG_CALL),
}
SG_EDGE_RED_U, SG_EDGE_RED_W, SG_EDGE_UNPAIRED = 1, 2, 4      # RAFT_HIP_SG_EDGE_*: the bits of ``edge_flags``
SG_EDGE_COLUMNS = ("edge_u", "edge_w", "edge_span", "edge_ext", "edge_back", "edge_flags")      # int32, but for edge_flags: uint8

# ... and those of include/raft_hip_ctn.h (libraft_hip_ctn.so): load_side_library("ctn") declares these
_CTN_CALL = [_vp] + _COLUMNS + [_vp, _i32, _i32, _i32] + [_vp] * 11 + [_P(_CtnSummary), _P(_i64), _P(_f64)]
_PLACE_CALL = [_vp, _i32] + [_vp] * 7 + [_i32, _vp] + [_vp] * 6 + [_P(_PlaceSummary), _P(_i64), _P(_f64)]
CTN_ABI = {
    "raft_hip_ctn_abi": (C.c_int, []),
    "raft_hip_containment_device": (C.c_int, _CTN_CALL),
    "raft_hip_containment_host": (C.c_int, _CTN_CALL),
    "raft_hip_place_contained_device": (C.c_int, _PLACE_CALL),
    "raft_hip_place_contained_host": (C.c_int, _PLACE_CALL),
}
# the bits of a read's flag byte (RAFT_HIP_CTN_*)
CTN_HAS_PARENT, CTN_PARENT_REV, CTN_ROOT_REV, CTN_UNPLACED_VIEW, CTN_ORPHAN = 1, 2, 4, 8, 16
CTN_MAX_READS = (1 << 30) - 1
# what ``Engine.containment`` returns per read (numpy dtypes), in the order of the entry point's outputs
CTN_PER_READ = (("parent", np.int32), ("pos", np.int32), ("span", np.int32), ("root", np.int32), ("root_pos", np.int32), ("depth", np.int32),
                ("children", np.int32), ("flags", np.uint8), ("tree_reads", np.int32), ("tree_bases", np.int64), ("tree_depth", np.int32))
# ... and ``Engine.place_contained``: per read, per unitig
PLACE_PER_READ = (("placed_unitig", np.int32), ("start", np.int64), ("placed_orient", np.uint8))
PLACE_PER_UNITIG = (("placed_reads", np.int32), ("placed_bases", np.int64), ("depth_permille", np.int64))

# ... and those of include/raft_hip_cln.h (libraft_hip_cln.so): load_side_library("cln") declares these
# ctx, n_reads, read_len, skip, n_edges, the three edge columns, W, T, R, the fourteen outputs
_CLN_CALL = [_vp, _i32, _vp, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32] + [_vp] * 10 + [_P(_ClnSummary), _P(_i64), _P(_f64), _P(_i64)]
CLN_ABI = {
    "raft_hip_cln_abi": (C.c_int, []),
    "raft_hip_graph_clean_device": (C.c_int, _CLN_CALL),
    "raft_hip_graph_clean_host": (C.c_int, _CLN_CALL),
}
CLN_WEAK_U, CLN_WEAK_W, CLN_TIP = 1, 2, 4                      # RAFT_HIP_CLN_*: the bits of ``edge_state``
CLN_READ_STAYS, CLN_READ_TIP, CLN_READ_FLAGGED = 0, 1, 2      # RAFT_HIP_CLN_READ_*: ``read_state``
CLN_MAX_ROUNDS = 64


@dataclass
class Summary:
    n_reads: int
    symmetric: int
    high_cov: int
    interval_path: int
    n_segments: int
    n_records: int
    n_intervals: int
    n_bins: int
    n_repeats: int
    n_cuts: int
    n_fragments: int
    total_coverage: int
    total_windows: int
    total_repeat_length: int
    total_read_length: int
    error_index: int
    n_devices_used: int = 0
    flags: int = 0                # RAFT_HIP_SUM_* (SUM_* above): bit 0 = the general bucketing handed the pileup kernel window records


@dataclass
class CoverageEstimate:
    """raft_hip_cov_estimate: what ``estimate_coverage`` reads from a coverage histogram."""
    est_cov: int                  # the smoothed mode of the covered, unclamped bins; 0 = none
    median: int                   # lower weighted median over the windows with coverage >= 1 (0 = none)
    windows: int
    windows_covered: int
    windows_clamped: int
    mean: float


class RaftError(RuntimeError):
    def __init__(self, code: int, message: str, index: int = -1):
        super().__init__(f"raft_hip error {code}: {message}" + (f" (index {index})" if index >= 0 else ""))
        self.code = code
        self.index = index


_lib = None


def load_library(path: str | None = None) -> C.CDLL:
    """Loads libraft_hip.so and declares every entry point of include/raft_hip.h."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or os.environ.get("RAFT_HIP_LIB") or _LIB_PATH   # RAFT_HIP_LIB: A/B runs of two builds in one session
    if not os.path.exists(p):
        raise RuntimeError(f"{p} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                           "(there is no CPU fallback for the RAFT hot path)")
    try:
        # PyTorch-ROCm bundles its own libamdhip64.so.7.  It must be the first HIP runtime in the process:
        # loading the system one (our DT_NEEDED) first leaves torch with a second, device-less runtime.
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(p)
    for name, (restype, argtypes) in ABI.items():
        fn = getattr(lib, name)
        fn.restype, fn.argtypes = restype, argtypes
    if path is None:
        _lib = lib
    return lib


# The libraries beside libraft_hip.so, in the order they came: tag -> (file, its ABI table, the function that says which engine ABI
# it was built beside).  The next library is one more entry here.
_SIDE = {
    "low": ("libraft_hip_low.so", LOW_ABI, "raft_hip_low_abi"), "ovl": ("libraft_hip_ovl.so", OVL_ABI, "raft_hip_ovl_abi"),
    "frag": ("libraft_hip_frag.so", FRAG_ABI, "raft_hip_frag_abi"), "rst": ("libraft_hip_rst.so", RST_ABI, "raft_hip_rst_abi"),
    "flt": ("libraft_hip_flt.so", FLT_ABI, "raft_hip_flt_abi"), "end": ("libraft_hip_end.so", END_ABI, "raft_hip_end_abi"),
    "best": ("libraft_hip_best.so", BEST_ABI, "raft_hip_best_abi"), "utg": ("libraft_hip_utg.so", UTG_ABI, "raft_hip_utg_abi"),
    "lift": ("libraft_hip_lift.so", LIFT_ABI, "raft_hip_lift_abi"),
}
# That table is closed at the nine; the libraries that came later stand here, rows of the same type under tags of their own, and the
# next one is a row here.
_SIDE_LATER = {
    "cc": ("libraft_hip_cc.so", CC_ABI, "raft_hip_cc_abi"),
    "sg": ("libraft_hip_sg.so", SG_ABI, "raft_hip_sg_abi"),
}
# ... and that one is closed at the two; a third holds what came behind them, and load_side_library looks through every table of
# _SIDE_TABLES: the next library is a row of the last one.
_SIDE_THIRD = {
    "ctn": ("libraft_hip_ctn.so", CTN_ABI, "raft_hip_ctn_abi"),
}
_SIDE_TABLES = (_SIDE, _SIDE_LATER, _SIDE_THIRD)
# Those three are closed.  _SIDE_OPEN is the open one: the next library is a row here, and nothing counts its rows.
_SIDE_OPEN = {
    "cln": ("libraft_hip_cln.so", CLN_ABI, "raft_hip_cln_abi"),
}
_side_libs: dict = {}


def load_side_library(tag: str) -> C.CDLL:
    """libraft_hip_<tag>.so of a table of ``_SIDE_TABLES`` or of ``_SIDE_OPEN`` (behind libraft_hip.so, whose contexts it takes) with
    every entry point of include/raft_hip_<tag>.h declared; the two must have been built beside each other."""
    if tag not in _side_libs:
        file, abi, abi_fn = next((t[tag] for t in _SIDE_TABLES if tag in t), None) or _SIDE_OPEN[tag]
        main = load_library()
        p = os.path.join(os.path.dirname(_LIB_PATH), file)
        if not os.path.exists(p):
            raise RuntimeError(f"{p} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'`")
        lib = C.CDLL(p)
        for name, (restype, argtypes) in abi.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
        built_beside = getattr(lib, abi_fn)()
        if built_beside != main.raft_hip_abi_version():
            raise RuntimeError(f"{p} was built beside ABI {built_beside}, libraft_hip.so is ABI {main.raft_hip_abi_version()}")
        _side_libs[tag] = lib
    return _side_libs[tag]


def _cparams(p: RaftParams) -> _Params:
    return _Params(p.reso, p.est_cov, p.cov_mul, p.repeat_length, p.interval_length, p.read_length,
                   p.overlap_length, p.flanking_length, p.symmetric_mode)


class _DevArray:
    """Zero-copy view of a device buffer for ``torch.as_tensor`` (CUDA array interface v2)."""

    def __init__(self, ptr: int, n: int, typestr: str, owner):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr or 0, False), "version": 2}
        self._owner = owner


def _view(eng, ptr, n, typestr, dtype):
    """Zero-copy torch view of n elements of the engine's device memory (an empty tensor for n = 0)."""
    import torch
    dev = f"cuda:{eng.device}"
    if n == 0:
        return torch.empty(0, dtype=dtype, device=dev)
    return torch.as_tensor(_DevArray(ptr, n, typestr, eng), device=dev)


# ---- the output layout ------------------------------------------------------------------------------------------------------
# Every array a finished pass hands back, in the order the ABI lists them: key, dtype, the count that sizes it ("n1" = n_reads + 1,
# "n_exc" = what the library reports, the others are Summary fields) and the forms that hold it -- F: raft_hip_fetch /
# raft_hip_outputs_device, P: the packed fetches, H: the host-to-host entry points' raft_hip_host_outputs.  The coverage arrays
# of the form's encoding come after cov_offset.
_OUTPUTS = (
    ("cov_offset", np.int64, "n1", "FPH"),
    ("exc_index", np.int64, "n_exc", "PH"), ("exc_value", np.int32, "n_exc", "PH"),
    ("rep_offset", np.int64, "n1", "FPH"), ("rep_s", np.int32, "n_repeats", "FPH"), ("rep_e", np.int32, "n_repeats", "FPH"),
    ("cut_offset", np.int64, "n1", "F"), ("cuts", np.int32, "n_cuts", "F"),
    ("frag_offset", np.int64, "n1", "FPH"), ("frag_read", np.int32, "n_fragments", "FP"),
    ("frag_begin", np.int32, "n_fragments", "FPH"), ("frag_end", np.int32, "n_fragments", "FPH"),
)
# The coverage encodings by width (bytes per window; 8 = RAFT_HIP_COV_DELTA4): key, dtype, elements for n windows.
_COVERAGE = {
    4: (("cov", np.int32, lambda n: n),),
    1: (("cov8", np.uint8, lambda n: n),),
    2: (("cov8", np.uint16, lambda n: n),),
    8: (("cov_nib", np.uint8, lambda n: (n + 1) // 2),              # two windows per byte
        ("cov_anchor", np.int32, lambda n: (n + 1023) // 1024)),    # an anchor per 1024 windows
}


def _layout(form: str, width: int, n_windows: int, counts: dict) -> list:
    """(key, dtype, elements) of every array of one form in one coverage width."""
    rows = [(k, dt, counts[c]) for k, dt, c, forms in _OUTPUTS if form in forms]
    rows[1:1] = [(k, dt, size(n_windows)) for k, dt, size in _COVERAGE[width]]
    return rows


def _counts(s, n_exc: int = 0) -> dict:
    return {"n1": s.n_reads + 1, "n_exc": n_exc, "n_repeats": s.n_repeats, "n_cuts": s.n_cuts, "n_fragments": s.n_fragments}


# outputs_device runs once per pass of a stream of batches: its rows (key, typestr, Summary field or "n1") are laid out here, once
_DEVICE_VIEWS = tuple((k, np.dtype(dt).str, c) for k, dt, c in _layout("F", 4, "n_bins", {c: c for _, _, c, _ in _OUTPUTS}))
_summary_values = operator.attrgetter(*(f for f, _ in _Summary._fields_))     # Summary(*_summary_values(s)): a _Summary as a Summary


# ---- the input forms ----------------------------------------------------------------------------------------------------------
def _need_int32_cuda(who: str, cols):
    import torch
    for t in cols:
        if t is not None and (t.dtype != torch.int32 or not t.is_cuda or not t.is_contiguous()):
            raise TypeError(f"{who} contiguous int32 CUDA tensors")


def _host_columns(cols) -> list:
    return [None if a is None else M.carray(a, np.int32) for a in cols]


def _plain(cols) -> tuple:
    """Plain columns -- read_len, qid, qs, qe and what there is of tid, ts, te (numpy arrays or tensors; None = absent) -- as
    every entry point takes them: n_reads, read_len, n_rec, the record columns."""
    return (M.count(cols[0]), M.ptr(cols[0]), M.count(cols[1]), *[M.ptr(c) for c in cols[1:]])


def _need_equal_lengths(cols, n_rec: int):
    for c in cols:
        if c is not None and (c.size if isinstance(c, np.ndarray) else c.numel()) != n_rec:
            raise ValueError("PAF columns differ in length")


def _offsets_misfit(rec_offset, n_reads: int, int64=None) -> bool:
    """Are these not the offsets [n_runs, n_reads + 1] of grouped input?  ``int64``: torch.int64 for a tensor, which must then be a
    contiguous CUDA tensor of that dtype as well (a numpy array has been made contiguous int64 by then)."""
    if int64 is not None and (rec_offset.dtype != int64 or not rec_offset.is_cuda or not rec_offset.is_contiguous()):
        return True
    shape = rec_offset.shape
    return len(shape) != 2 or shape[1] != n_reads + 1


_DEVICE_OFFSETS = "%s needs rec_offset as a contiguous int64 CUDA tensor [n_runs, n_reads + 1]"


def _grouped_host(method: str, read_len, rec_offset, records, dtype) -> tuple:
    """Grouped host input -- ``records``: the int32 columns (qs, qe), or (win,) as uint32 window records -- as the arrays to keep
    alive (read_len, the records, rec_offset) and the arguments: n_reads, read_len, n_rec, n_runs, rec_offset, the records."""
    rl = M.carray(read_len, np.int32)
    rec = [M.carray(x, dtype) for x in records]
    off = M.carray(rec_offset, np.int64)
    if _offsets_misfit(off, rl.size) or any(x.size != rec[0].size for x in rec):
        raise ValueError(f"{method}: rec_offset must be [n_runs, n_reads + 1]" + (", qs/qe of equal length" if len(rec) == 2 else ""))
    return (rl, *rec, off), (rl.size, M.ptr(rl), rec[0].size, off.shape[0], M.ptr(off), *[M.ptr(x) for x in rec])


_CSR_DTYPES = (np.int64, np.int32, np.int32)      # a CSR table by read: offsets [n_reads + 1], two row arrays


def _csr_count(given: bool, table) -> int:
    """The count a library takes with the three arrays of a table: -1 = the context's own pass, else its rows (0 without row arrays)."""
    return -1 if not given else (M.count(table[1]) if table[1] is not None else 0)


def _twin(n: int, dtype, like=None, zeroed: bool = True):
    """``n`` elements of a numpy dtype where a query's inputs are: a tensor on the device of the input ``like``, or (None) a numpy array."""
    if like is None:
        return (np.zeros if zeroed else np.empty)(n, dtype)
    import torch
    return (torch.zeros if zeroed else torch.empty)(n, dtype=getattr(torch, np.dtype(dtype).name), device=like.device)


def _summary_dict(sm) -> dict:
    """A summary structure of 64-bit counts as the dict entries a query's result ends with."""
    return {name: int(getattr(sm, name)) for name, _ in sm._fields_}


def _contexts(engines) -> tuple:
    """The contexts of a job that several engines share, as the ABI takes them: the array and its length."""
    return (C.c_void_p * len(engines))(*[e._ctx for e in engines]), len(engines)


class Engine:
    """One context on one MI355X: ``run*`` -> ``finish`` -> ``fetch`` / ``outputs_device``."""

    def __init__(self, params: RaftParams, device: int = 0):
        self._lib = load_library()
        self._ctx = C.c_void_p()
        self.params = params
        cp = _cparams(params)
        rc = self._lib.raft_hip_create(device, C.byref(cp), C.byref(self._ctx))
        if rc != OK:
            self._ctx = C.c_void_p()
            raise RaftError(rc, self._lib.raft_hip_strerror(rc).decode())
        self.device = device
        self._keep = None

    def close(self):
        if getattr(self, "_ctx", None) and self._ctx.value:
            self._lib.raft_hip_destroy(self._ctx)
            self._ctx = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, index: int = -1):
        if rc != OK:
            msg = self._lib.raft_hip_strerror(rc).decode()
            detail = self._lib.raft_hip_last_error(self._ctx).decode()
            raise RaftError(rc, msg + (f" [{detail}]" if detail else ""), index)

    def set_params(self, params: RaftParams):
        cp = _cparams(params)
        self._check(self._lib.raft_hip_set_params(self._ctx, C.byref(cp)))
        self.params = params

    def set_tuning(self, tile_bins: int = 0, force_bucket_path: bool = False, variant: int = -1):
        self._check(self._lib.raft_hip_set_tuning(self._ctx, tile_bins, int(force_bucket_path), variant))

    def set_placement_trial(self, candidates: int):
        """Opt in to the coverage array's placement trial at the context's first large pass: 2..8 candidate arrays, 0 = off (the default)."""
        self._check(self._lib.raft_hip_set_placement_trial(self._ctx, candidates))

    def warm_up(self):
        """raft_hip_warm_up: the engine's code on the device, the pipeline's lanes -- what a context's first host-to-host job would
        otherwise pay inside its own clock."""
        self._check(self._lib.raft_hip_warm_up(self._ctx))

    def reserve(self, read_len, n_rec_estimate: int, n_ctx: int = 1, cov_width: int = 1):
        """raft_hip_reserve: device buffers and page-locked staging of a coming host-to-host job, from the reads' lengths and an
        estimate of the record count (cov_width: 1, 2 or 8 = four-bit steps)."""
        rl = M.carray(read_len, np.int32)
        self._check(self._lib.raft_hip_reserve(self._ctx, rl.size, M.ptr(rl), int(n_rec_estimate), int(n_ctx), int(cov_width)))

    def placement_trial(self):
        """(first_ms, best_other_ms, kept) of the coverage array's placement trial -- kept: 0 the first placement, 1 a plain block, 2 another
        chunk mapping -- or None when none has run (raft_hip_placement_trial)."""
        a, b, k = C.c_double(), C.c_double(), C.c_int32()
        if self._lib.raft_hip_placement_trial(self._ctx, C.byref(a), C.byref(b), C.byref(k)) != OK:
            return None
        return a.value, b.value, int(k.value)

    def set_output_width(self, width: int):
        """4: cov[] as int32 (default); 1 / 2: later passes write the transfer encoding directly (raft_hip_set_output_width)."""
        self._check(self._lib.raft_hip_set_output_width(self._ctx, width))

    def set_emit_cuts(self, on: bool):
        """True (default): every pass writes the cut points itself; False: the first fetch that asks for them does."""
        self._check(self._lib.raft_hip_set_emit_cuts(self._ctx, 1 if on else 0))

    def device_tensor(self, shape, dtype):
        """A torch tensor over device memory from raft_hip_device_alloc (the engine's placement: shuffled 32 MiB chunks); it
        lives until the context is closed or device_free(tensor) is called."""
        import torch
        shape = tuple(int(x) for x in (shape if isinstance(shape, (tuple, list)) else (shape,)))
        n = 1
        for x in shape:
            n *= x
        item = torch.empty(0, dtype=dtype).element_size()
        ptr = C.c_void_p()
        self._check(self._lib.raft_hip_device_alloc(self._ctx, n * item, C.byref(ptr)))
        typestr = {torch.int32: "<i4", torch.int64: "<i8", torch.uint8: "|u1", torch.int16: "<i2"}[dtype]

        class _Mem:
            pass
        m = _Mem()
        m.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (int(ptr.value or 0), False), "version": 2}
        t = torch.as_tensor(m, device=f"cuda:{self.device}")
        t._raft_ptr = int(ptr.value or 0)
        return t

    def device_copy(self, t):
        """`t` copied into memory from device_tensor."""
        out = self.device_tensor(tuple(t.shape), t.dtype)
        out.copy_(t)
        return out

    def device_free(self, t):
        self._check(self._lib.raft_hip_device_free(self._ctx, C.c_void_p(getattr(t, "_raft_ptr", None) or t.data_ptr())))

    def group_sides(self, n_reads_total: int, qid, qs, qe, tid=None, ts=None, te=None, symmetric: bool = False) -> "Slice":
        """raft_hip_group_sides: the (read, start, end) intervals of a slice's records -- query sides, and target sides of records
        whose two reads differ unless ``symmetric`` -- sorted by read id on the device, as a Slice in grouped form with one run
        (ready for exchange_local / Comm.exchange).  The arrays are the context's (valid until its next group_sides)."""
        import torch
        self.use_torch_stream()
        cols = [qid, qs, qe] + ([] if symmetric else [tid, ts, te])
        _need_int32_cuda("group_sides needs", cols)
        ptr = [M.ptr(t) for t in cols] + ([C.c_void_p(0)] * 3 if symmetric else [])
        out = _Slice()
        self._check(self._lib.raft_hip_group_sides(self._ctx, n_reads_total, int(qid.numel()), *ptr, 1 if symmetric else 0, C.byref(out)))
        n = int(out.n_rec)
        off = np.ctypeslib.as_array(C.cast(out.rec_offset, C.POINTER(C.c_int64)), shape=(1, n_reads_total + 1)).copy()
        sl = Slice(off, *[_view(self, p, n, "<i4", torch.int32) for p in (out.d_qs, out.d_qe)])
        sl.ptrs = (int(out.d_qs or 0), int(out.d_qe or 0))   # (the context's columns as they are: not NULL, not even without intervals)
        return sl

    def use_torch_stream(self):
        import torch
        self._check(self._lib.raft_hip_set_stream(self._ctx, C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)))

    # -- passes -----------------------------------------------------------------
    def run_device(self, read_len, qid, qs, qe, tid=None, ts=None, te=None):
        """Inputs: int32 torch tensors on this engine's device (kept alive until the next pass); tid / ts / te may be None when
        the params assert symmetric_mode = 1."""
        cols = (read_len, qid, qs, qe, tid, ts, te)
        # (a caller that hands over the same tensors again -- a stream of batches through fixed buffers -- is checked once; a tensor
        # resized in place keeps its address, so the lengths are part of what must match)
        last = getattr(self, "_last_device_call", None)
        if last is not None and all(a is b for a, b in zip(last[0], cols)) and \
                all(t is None or (t.data_ptr(), t.numel()) == q for t, q in zip(cols, last[2])):
            args = last[1]
        else:
            _need_int32_cuda("run_device needs", cols)
            args = _plain(cols)
            _need_equal_lengths(cols[2:], args[2])
            self._last_device_call = (cols, args, [None if t is None else (t.data_ptr(), t.numel()) for t in cols])
        self._keep = cols
        self.use_torch_stream()     # the tensors were produced on torch's current stream: order after it
        self._check(self._lib.raft_hip_run_device(self._ctx, *args))

    def run_device_grouped(self, read_len, rec_offset, qid, qs, qe, n_bins: int = -1):
        """raft_hip_run_device_grouped: ``rec_offset`` int64 CUDA tensor [n_runs, n_reads + 1] (first record of every read in
        every sorted run), ``qid`` may be None (the ids are then rebuilt from the offsets on the device), ``n_bins`` the
        caller's sum of ceil(len / reso) (-1: unknown; >= 0: the pass runs without a host wait).  symmetric_mode must be 1."""
        import torch
        n_reads = int(read_len.numel())
        if _offsets_misfit(rec_offset, n_reads, torch.int64):
            raise TypeError(_DEVICE_OFFSETS % "run_device_grouped")
        cols = (read_len, qs, qe) + (() if qid is None else (qid,))
        _need_int32_cuda("run_device_grouped needs", cols)
        n_rec = int(qs.numel())
        _need_equal_lengths(cols[2:], n_rec)
        self._keep = cols + (rec_offset,)
        self.use_torch_stream()
        P = M.ptr
        self._check(self._lib.raft_hip_run_device_grouped(self._ctx, n_reads, P(read_len), n_rec, int(rec_offset.shape[0]), P(rec_offset),
                                                          P(qid), P(qs), P(qe), int(n_bins)))

    def run_device_windows(self, read_len, rec_offset, win, n_bins: int = -1):
        """raft_hip_run_device_windows: grouped input whose records are ONE word each -- first window | one past the last << 16
        (``hostio.pack_windows``); ``win`` an int32 or uint32-viewed CUDA tensor of 32-bit words.  symmetric_mode must be 1."""
        import torch
        n_reads = int(read_len.numel())
        if _offsets_misfit(rec_offset, n_reads, torch.int64):
            raise TypeError(_DEVICE_OFFSETS % "run_device_windows")
        for t in (read_len, win):
            if t.element_size() != 4 or t.is_floating_point() or not t.is_cuda or not t.is_contiguous():
                raise TypeError("run_device_windows needs contiguous 32-bit integer CUDA tensors")
        self._keep = (read_len, win, rec_offset)
        self.use_torch_stream()
        P = M.ptr
        self._check(self._lib.raft_hip_run_device_windows(self._ctx, n_reads, P(read_len), int(win.numel()), int(rec_offset.shape[0]), P(rec_offset),
                                                          P(win), int(n_bins)))

    def run_host_windows(self, read_len, rec_offset, win, n_bins: int = -1):
        """raft_hip_run_host_windows: numpy arrays; ``win`` uint32 window records."""
        self._keep, args = _grouped_host("run_host_windows", read_len, rec_offset, (win,), np.uint32)
        self._check(self._lib.raft_hip_run_host_windows(self._ctx, *args, int(n_bins)))

    def run_host_grouped(self, read_len, rec_offset, qs, qe, n_bins: int = -1):
        """raft_hip_run_host_grouped: numpy arrays; ``rec_offset`` int64 [n_runs, n_reads + 1]."""
        self._keep, args = _grouped_host("run_host_grouped", read_len, rec_offset, (qs, qe), np.int32)
        self._check(self._lib.raft_hip_run_host_grouped(self._ctx, *args, int(n_bins)))

    def run_host(self, read_len, qid, qs, qe, tid=None, ts=None, te=None):
        """tid/ts/te may be None when the params assert symmetric_mode = 1 (they are then neither read nor uploaded)."""
        cols = _host_columns((read_len, qid, qs, qe, tid, ts, te))
        args = _plain(cols)
        _need_equal_lengths(cols[2:], args[2])
        self._keep = cols
        self._check(self._lib.raft_hip_run_host(self._ctx, *args))

    def finish(self) -> Summary:
        s = _Summary()
        rc = self._lib.raft_hip_finish(self._ctx, C.byref(s))
        summ = Summary(*_summary_values(s))
        self.summary = summ
        self._check(rc, summ.error_index)
        return summ

    def timing(self) -> tuple[float, float]:
        a, b = C.c_double(), C.c_double()
        self._check(self._lib.raft_hip_last_timing(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def fetch(self, coverage: bool = True, pinned: bool = False, out: dict | None = None) -> dict:
        """Host copies (numpy) of the finished pass, CSR per read.

        pinned: allocate the arrays in page-locked memory (the copies then run at the link's rate instead of the
        pageable path's).  out: arrays of an earlier fetch to reuse when their sizes still fit (a caller that keeps
        one pinned set of buffers pays neither allocation nor page faults per pass)."""
        s = self.summary
        have = out or {}
        out = {k: M.fit(have.get(k), n, dt, pinned) for k, dt, n in _layout("F", 4, s.n_bins if coverage else 0, _counts(s))}
        self._check(self._lib.raft_hip_fetch(self._ctx, *[M.ptr(a) for a in out.values()]))
        return out

    def host_output_buffers(self, read_len, pinned: bool = True, exc_cap: int = 1 << 20, width: int = 1) -> dict:
        """Caller-owned arrays for ``run_pipelined`` sized by the upper bounds of include/raft_hip.h (page-locked when
        ``pinned``): allocate once, reuse for every pass over inputs of this shape."""
        p = self.params
        rl = np.asarray(read_len, np.int64)
        nb = (rl + p.reso - 1) // p.reso
        minw = max((p.repeat_length + p.reso - 1) // p.reso, 1)
        caps = {"cov8": int(nb.sum()), "rep": (int(nb.sum()) + rl.size) // (minw + 1), "frag": int(rl.sum()) // p.interval_length + 2 * rl.size,
                "exc": int(exc_cap)}
        if width == 8:       # delta4: two windows per byte + an anchor per 1024 windows ("cov_nib" / "cov_anchor" name the encoding)
            caps["exc"] = max(caps["exc"], caps["cov8"] // 128)      # (every tile's first window and the large steps: 0.2-0.3 % of a 32x set)
        counts = {"n1": rl.size + 1, "n_exc": caps["exc"], "n_repeats": caps["rep"], "n_fragments": caps["frag"]}
        rows = _layout("H", width if width in (2, 8) else 1, caps["cov8"], counts)
        return {k: M.empty(max(int(n), 1), dt, pinned) for k, dt, n in rows}     # (at least one element: every pointer is a real one)

    def run_pipelined_grouped(self, read_len, rec_offset, qs, qe, n_chunks: int = 0, out: dict | None = None,
                              others: list | None = None):
        """raft_hip_run_multi_grouped: as ``run_pipelined`` with the caller's per-read record offsets (int64
        [n_runs, n_reads + 1]) in place of the query column."""
        keep, args = _grouped_host("run_pipelined_grouped", read_len, rec_offset, (qs, qe), np.int32)
        return self._host_job(self._lib.raft_hip_run_multi_grouped, _contexts([self, *(others or [])]), keep[0], (*args, int(n_chunks)), out)

    def run_pipelined_windows(self, read_len, rec_offset, win, n_chunks: int = 0, out: dict | None = None, others: list | None = None):
        """raft_hip_run_multi_windows: as ``run_pipelined_grouped`` with window records (uint32, ``hostio.pack_windows``) in place
        of the two coordinate columns."""
        keep, args = _grouped_host("run_pipelined_windows", read_len, rec_offset, (win,), np.uint32)
        return self._host_job(self._lib.raft_hip_run_multi_windows, _contexts([self, *(others or [])]), keep[0], (*args, int(n_chunks)), out)

    def _host_job(self, entry, head, read_len, args, out):
        """What the host-to-host methods share once their input is packed: buffers by default, the job, its trimmed results."""
        if out is None:
            out = self.host_output_buffers(read_len, pinned=False)
        ho, s = self._host_outputs(out), _Summary()
        rc = entry(*head, *args, C.byref(ho), C.byref(s))
        return self._pipelined_result(rc, s, ho, out)

    def _host_outputs(self, out: dict) -> "_HostOutputs":
        ho = _HostOutputs()
        for k, _, _, forms in _OUTPUTS:
            if "H" in forms:
                setattr(ho, k, out[k].ctypes.data)
        ho.exc_cap, ho.rep_cap, ho.frag_cap = out["exc_index"].size, out["rep_s"].size, out["frag_begin"].size
        if "cov_nib" in out:                                               # delta4 (host_output_buffers(width=8))
            ho.cov8, ho.cov8_cap = out["cov_nib"].ctypes.data, 2 * out["cov_nib"].size
            ho.cov_anchor, ho.anchor_cap = out["cov_anchor"].ctypes.data, out["cov_anchor"].size
            ho.cov_width = 8
        else:
            ho.cov8, ho.cov8_cap = out["cov8"].ctypes.data, out["cov8"].size
            ho.cov_width = 2 if out["cov8"].dtype == np.uint16 else 1      # the buffer's dtype chooses the encoding's width
        return ho

    def _pipelined_result(self, rc, s, ho, out):
        summ = Summary(*_summary_values(s))
        self.summary = summ
        self.last_n_exc = int(ho.n_exc)
        self._check(rc, summ.error_index)
        rows = _layout("H", 8 if "cov_nib" in out else 1, summ.n_bins, _counts(summ, ho.n_exc))
        return {k: out[k][:n] for k, _, n in rows}, summ

    def run_pipelined(self, read_len, qid, qs, qe, tid=None, ts=None, te=None, n_chunks: int = 0, out: dict | None = None,
                      others: list | None = None):
        """raft_hip_run_pipelined: host columns in, host outputs out, with upload / pass / download of consecutive read
        ranges overlapped.  ``others``: more Engines (other GPUs of the node, or the same one) to share the job with
        (raft_hip_run_multi).  Returns (dict of arrays trimmed to their sizes -- views of ``out`` --, Summary)."""
        cols = _host_columns((read_len, qid, qs, qe, tid, ts, te))
        if others:
            entry, head = self._lib.raft_hip_run_multi, _contexts([self, *others])
        else:
            entry, head = self._lib.raft_hip_run_pipelined, (self._ctx,)
        return self._host_job(entry, head, cols[0], (*_plain(cols), int(n_chunks)), out)

    def run_presplit(self, read_len, qid, qs, qe, tid, ts, te, others: list, out: dict | None = None):
        """raft_hip_run_presplit_local: this Engine is rank 0, ``others`` ranks 1 .. -- the record stream is cut into as many
        contiguous slices, every slice's sides are grouped on its rank's device, ONE exchange routes them to the owners of their
        reads, every rank runs its grouped pass.  Same return as ``run_pipelined``."""
        cols = _host_columns((read_len, qid, qs, qe, tid, ts, te))
        return self._host_job(self._lib.raft_hip_run_presplit_local, _contexts([self, *others]), cols[0], _plain(cols), out)

    def fetch_packed(self, pinned: bool = False, out: dict | None = None, width: int = 1) -> dict:
        """Host copies with the coverage array in its transfer encoding (raft_hip_fetch_packed_w): ``cov8`` (uint8 per
        window, 255 = see exceptions; with ``width=2`` uint16, 65535), ``exc_index`` / ``exc_value`` (ascending), and the
        repeat / fragment tables.  ``out``: arrays of an earlier call to reuse (pinned buffers kept by the caller; the
        dtype of its ``cov8`` decides the width)."""
        if out is not None and out.get("cov8") is not None:
            width = 2 if out["cov8"].dtype == np.uint16 else 1
        return self._fetch_encoded(self._lib.raft_hip_fetch_packed_w, (self._ctx, width), 2 if width == 2 else 1, pinned, out)

    def fetch_delta4(self, pinned: bool = False, out: dict | None = None) -> dict:
        """Host copies with the coverage array in the four-bit step encoding (raft_hip_fetch_delta4): ``cov_nib`` (uint8,
        two windows per byte), ``cov_anchor`` (int32 per 1024 windows), ``exc_index`` / ``exc_value`` (ascending; ABSOLUTE values
        of the escaped windows), and the repeat / fragment tables.  ``hostio.unpack_coverage_d4`` restores the int32 array."""
        return self._fetch_encoded(self._lib.raft_hip_fetch_delta4, (self._ctx,), 8, pinned, out)

    def _fetch_encoded(self, entry, head, width, pinned, out):
        """The packed fetches: the size query (every pointer NULL, no room for exceptions), then the arrays."""
        n_cov = len(_COVERAGE[width])
        n_exc = C.c_int64(0)
        self._check(entry(*head, *[None] * (1 + n_cov), 0, None, None, C.byref(n_exc), *[None] * 7))
        have = out or {}
        res = {k: M.fit(have.get(k), n, dt, pinned) for k, dt, n in _layout("P", width, self.summary.n_bins, _counts(self.summary, n_exc.value))}
        ptr = [M.ptr(a) for a in res.values()]
        self._check(entry(*head, *ptr[:1 + n_cov], n_exc.value, *ptr[1 + n_cov:3 + n_cov], C.byref(n_exc), *ptr[3 + n_cov:]))
        return res

    def outputs_device(self) -> dict:
        """Zero-copy torch views of the device-resident outputs (valid until the next pass).  Treat them as read-only: torch takes no
        read-only CUDA array interface, so nothing stops a write, and the library scans the per-read geometry again in the next pass
        rather than trust ``cov_offset`` after this call."""
        import torch
        o = _Outputs()
        self._check(self._lib.raft_hip_outputs_device(self._ctx, C.byref(o)))
        s = self.summary
        n1 = s.n_reads + 1
        res = {}
        for k, ts, c in _DEVICE_VIEWS:
            n = n1 if c == "n1" else getattr(s, c)
            if n == 0:
                res[k] = torch.empty(0, dtype=torch.int64 if ts == "<i8" else torch.int32, device=f"cuda:{self.device}")
            else:
                res[k] = torch.as_tensor(_DevArray(getattr(o, k), n, ts, self), device=f"cuda:{self.device}")
        return res

    # -- the estimated coverage from the data -------------------------------------------
    last_histogram_seconds = 0.0      # device time of the last coverage_histogram() call's launches

    def coverage_histogram(self) -> np.ndarray:
        """raft_hip_cov_histogram: int64 [4096], ``hist[v]`` = windows of the finished pass with coverage v (the last bin: >= 4095).
        Computed on the device from the form the pass wrote; cov[] is not downloaded."""
        hist = np.zeros(COV_HIST_BINS, np.int64)
        secs = C.c_double(0.0)
        self._check(self._lib.raft_hip_cov_histogram(self._ctx, C.c_void_p(hist.ctypes.data), C.byref(secs)))
        self.last_histogram_seconds = secs.value
        return hist

    def estimate_from(self, read_len, qid, qs, qe, tid=None, ts=None, te=None) -> "CoverageEstimate":
        """One pass over the device tensors (``run_device`` + ``finish``), its coverage histogram and the estimate read from it; when
        there is one (``est_cov > 0``) it becomes the context's est_cov for the passes that follow."""
        import dataclasses
        self.run_device(read_len, qid, qs, qe, tid, ts, te)
        self.finish()
        est = estimate_coverage(self.coverage_histogram())
        if est.est_cov > 0:
            self.set_params(dataclasses.replace(self.params, est_cov=est.est_cov))
        return est

    # -- the per-read table ------------------------------------------------------------
    last_read_stats_seconds = 0.0     # device time of the last read_stats() call's launches
    last_census_seconds = 0.0         # ... and of the last census()

    def read_stats(self, threshold: int | None = None) -> dict:
        """raft_hip_read_stats: per read of the finished pass ``cov_sum`` (int64), ``cov_max`` and ``high_windows`` (int32; windows
        with coverage >= ``threshold``, by default the context's high_cov = int(est_cov * cov_mul) under the parameters in force at
        this call -- after a ``set_params`` those, not the finished pass's).  Reduced on the device from the form the pass wrote;
        cov[] is not downloaded."""
        if threshold is None:
            threshold = int(self.params.est_cov * self.params.cov_mul)
        n = max(self._own_rows("n_reads"), 0)
        out = {"cov_sum": np.zeros(n, np.int64), "cov_max": np.zeros(n, np.int32), "high_windows": np.zeros(n, np.int32)}
        secs = C.c_double(0.0)
        self._check(self._lib.raft_hip_read_stats(self._ctx, int(threshold), *[M.ptr(a) for a in out.values()],
                                                  C.byref(secs)))
        self.last_read_stats_seconds = secs.value
        return out

    # -- where a read is not covered ---------------------------------------------------
    last_low_coverage_seconds = 0.0   # device time of the launches of one raft_hip_low_coverage call: the last low_coverage()'s fetch

    def low_coverage(self, low_cov: int = 0, uncovered_permille: int = 800) -> dict:
        """raft_hip_low_coverage (libraft_hip_low.so): the runs of consecutive windows with coverage <= ``low_cov`` of every read of the finished pass, as
        CSR in read order -- ``low_offset`` (int64 [n_reads + 1]), ``low_s`` / ``low_e`` (int32, bases) --, per read ``low_windows``
        (int32) and ``low_flags`` (uint8: LOW_INTERIOR | LOW_HEAD | LOW_TAIL | LOW_UNCOVERED), and the totals ``n_runs``,
        ``total_low_windows``, ``low_bases``, ``reads_with_runs``, ``reads_interior``, ``reads_uncovered``.  Computed on the device
        from the form the pass wrote; cov[] is not downloaded.  Two calls of the library: the size query, then the fetch into arrays
        of that size."""
        n = max(self._own_rows("n_reads"), 0)
        sm, secs = _LowSummary(), C.c_double(0.0)
        null = C.c_void_p(0)
        args = (int(low_cov), int(uncovered_permille))
        low = load_side_library("low")
        self._check(low.raft_hip_low_coverage(self._ctx, *args, 0, null, null, null, null, null, C.byref(sm), C.byref(secs)))
        out = {"low_offset": M.empty(n + 1, np.int64), "low_s": M.empty(int(sm.n_runs), np.int32), "low_e": M.empty(int(sm.n_runs), np.int32),
               "low_windows": M.empty(n, np.int32), "low_flags": M.empty(n, np.uint8)}
        self._check(low.raft_hip_low_coverage(self._ctx, *args, int(sm.n_runs), *[M.ptr(a) for a in out.values()], C.byref(sm),
                                                    C.byref(secs)))
        self.last_low_coverage_seconds = secs.value
        out.update(n_runs=int(sm.n_runs), total_low_windows=int(sm.low_windows), low_bases=int(sm.low_bases),
                   reads_with_runs=int(sm.reads_with_runs), reads_interior=int(sm.reads_interior), reads_uncovered=int(sm.reads_uncovered))
        return out

    # -- the queries about a record stream ------------------------------------------------
    def _own_rows(self, field: str) -> int:
        """Rows of the context's own pass -- ``n_fragments``, ``n_repeats`` or ``n_reads`` of the last summary --, 0 with no pass: what
        the outputs need; the library checks the state."""
        last = getattr(self, "summary", None)
        return int(getattr(last, field)) if last is not None else 0

    def _record_query(self, who: str, cols, *, lead: int = 1, rec_u8=None, read_u8=None, tables=None, tables_vote: bool = False,
                      offsets_error: str = "", device_out=()) -> tuple:
        """The input of a query, ready for its library.  ``cols``: the int32 arrays (None = absent) -- ``lead`` arrays the method
        measures itself (read_len; none; read_len and the two per-end arrays of unitigs), then the record columns that there are.
        ``lead == 0`` also says that there is no read_len: ``n_reads`` is then None and no table is measured here -- the method does it.
        ``rec_u8`` / ``read_u8``: by name the uint8 arrays with a byte per record (as long as the columns) / per read (the method checks
        their length: the words differ).  ``tables``: by name the three arrays of a CSR table the caller gave, or three None.
        ``device_out``: int32 outputs of the caller's, which in the device form must be tensors like the columns (refused with them,
        before the stream is touched); they have no say in the form and the host form leaves them to the method.
        The form: all int32 and uint8 arrays on the device -- and, under ``tables_vote``, the tables' -- is the device form, every array
        then a contiguous CUDA tensor of its dtype, on the engine's torch stream; else the host form, every array a contiguous numpy
        array.  Record columns are of one length; with a read_len a table is (offsets [n_reads + 1], two arrays of one length) -- the
        library is told no lengths: what it will read must be there.
        -> on_device, cols, the uint8 arrays (per record, then per read), the tables' arrays, n_reads (None without read_len), n_rec"""
        rec_u8, read_u8, tables = rec_u8 or {}, read_u8 or {}, tables or {}
        u8 = {**rec_u8, **read_u8}
        tabs = [list(t) for t in tables.values()]
        voters = [x for x in [*cols, *u8.values()] + ([a for t in tabs for a in t] if tables_vote else []) if x is not None]
        on_device = bool(voters) and all(hasattr(x, "is_cuda") and x.is_cuda for x in voters)
        if on_device:
            import torch
            _need_int32_cuda(f"{who} needs", list(cols) + [a for t in tabs for a in t[1:]] + list(device_out))
            for name, x in u8.items():          # (it voted: it is on the device)
                if x is not None and (x.dtype != torch.uint8 or not x.is_contiguous()):
                    raise TypeError(f"{who} needs {name} as a contiguous uint8 CUDA tensor")
            for t in tabs:
                if t[0] is not None and (t[0].dtype != torch.int64 or not t[0].is_cuda or not t[0].is_contiguous()):
                    raise TypeError(offsets_error)
            self.use_torch_stream()
            u8 = list(u8.values())
        else:
            host = lambda a, dt: None if a is None else M.carray(a.cpu() if hasattr(a, "is_cuda") else a, dt)
            cols = [host(x, np.int32) for x in cols]
            u8 = [host(x, np.uint8) for x in u8.values()]
            tabs = [[host(a, dt) for a, dt in zip(t, _CSR_DTYPES)] for t in tabs]
        has_read_len = lead > 0
        records = [c for c in cols[lead:] if c is not None]
        n_reads = M.count(cols[0]) if has_read_len else None
        n_rec = M.count(records[0]) if records else 0
        _need_equal_lengths(records[1:] + u8[:len(rec_u8)], n_rec)
        for what, t in zip(tables, tabs) if has_read_len else ():
            if any(a is not None for a in t) and (t[0] is None or (t[1] is None) != (t[2] is None) or M.count(t[0]) != n_reads + 1
                                                  or (t[1] is not None and M.count(t[1]) != M.count(t[2]))):
                raise ValueError(f"{what} is (offsets [n_reads + 1], two arrays of one length)")
        return on_device, cols, u8, tabs, n_reads, n_rec

    # -- which overlaps lie inside repeats ----------------------------------------------
    last_repeat_overlaps_seconds = 0.0   # device time of the launches of the last repeat_overlaps()

    def repeat_overlaps(self, read_len, qid, qs, qe, tid, ts=None, te=None, *, min_anchor: int = 1000, symmetric: bool = False, repeats=None) -> dict:
        """raft_hip_repeat_overlaps_device / _host (libraft_hip_ovl.so): every record classified against the repeat annotation --
        ``cls`` (one byte per record: OVL_Q_REPEAT | OVL_T_REPEAT | OVL_Q_TOUCH | OVL_T_TOUCH | OVL_Q_CONTAINED | OVL_T_CONTAINED; a
        side is REPEAT when it touches the union of its read's runs and fewer than ``min_anchor`` of its bases lie outside) --, per
        read ``read_touch`` / ``read_repeat`` (int32: its sides with TOUCH / REPEAT, sides counted as the census counts them under
        ``symmetric``) and ``read_flags`` (uint8: OVL_READ_CONTAINED | OVL_READ_ANCHORED; a read whose flags are OVL_READ_CONTAINED
        alone is contained only inside repeats of its containers), and the summary's counts.  The columns are int32 torch tensors on
        this engine's device (``cls`` is then a torch.uint8 tensor there; ``repeats`` must be tensors too) or numpy arrays (staged by
        the library); ts / te may be None when ``symmetric``.  ``repeats``: None = the annotation of this context's finished pass,
        else (rep_offset int64 [n_reads + 1], rep_s, rep_e int32)."""
        if any(x is None for x in (read_len, qid, qs, qe, tid)) or (ts is None) != (te is None) or (not symmetric and ts is None):
            raise ValueError("repeat_overlaps needs read_len, qid, qs, qe, tid (and ts, te unless symmetric)")
        cols = [read_len, qid, qs, qe, tid] + ([] if ts is None else [ts, te])
        rep = [None, None, None] if repeats is None else list(repeats)
        if len(rep) != 3:
            raise ValueError("repeats is (rep_offset, rep_s, rep_e)")
        ovl = load_side_library("ovl")
        on_device, cols, _, (rep,), n_reads, n_rec = self._record_query(
            "repeat_overlaps", cols, tables={"repeats": rep}, offsets_error="repeat_overlaps needs rep_offset as a contiguous int64 CUDA tensor")
        fn = ovl.raft_hip_repeat_overlaps_device if on_device else ovl.raft_hip_repeat_overlaps_host
        args = _plain(cols) + ((C.c_void_p(0),) * 2 if ts is None else ())
        out = {"cls": _twin(n_rec, np.uint8, qid if on_device else None), "read_touch": np.zeros(n_reads, np.int32),
               "read_repeat": np.zeros(n_reads, np.int32), "read_flags": np.zeros(n_reads, np.uint8)}
        sm, err, secs = _OvlSummary(), C.c_int64(-1), C.c_double(0.0)
        rc = fn(self._ctx, *args, 1 if symmetric else 0, int(min_anchor), _csr_count(repeats is not None, rep), *[M.ptr(a) for a in rep],
                *[M.ptr(a) for a in out.values()], C.byref(sm), C.byref(err), C.byref(secs))
        self._check(rc, err.value)
        self.last_repeat_overlaps_seconds = secs.value
        out.update(_summary_dict(sm))
        return out

    # -- which fragments stay contained ------------------------------------------------------
    last_fragment_overlaps_seconds = 0.0   # device time of the launches of the last fragment_overlaps()

    def fragment_overlaps(self, read_len, qid, qs, qe, tid, ts, te, symmetric: bool = False, fragments=None, repeats=None) -> dict:
        """raft_hip_frag_overlaps_device / _host (libraft_hip_frag.so): the record stream joined with a fragment table -- per fragment
        ``frag_touch``, ``frag_span``, ``frag_contained`` (int32: the overlap sides that touch the row, span it end to end, and span it
        with the partner's side inside one fragment of the partner) and ``frag_repeat`` (its bases inside the read's repeats), per read
        ``read_contained`` (int32 numpy: its rows with frag_contained > 0), and the summary's counts.  Sides are counted as the census
        counts them under ``symmetric``; all six columns are needed either way.  The columns are int32 torch tensors on this engine's
        device (the per-fragment arrays are then tensors there; ``fragments`` and ``repeats`` must be tensors too) or numpy arrays
        (staged by the library).  ``fragments``: None = the rows of this context's finished pass, else (frag_offset int64
        [n_reads + 1], frag_begin, frag_end int32).  ``repeats``: None = the annotation of this context's finished pass, () = none
        (frag_repeat is 0), else (rep_offset int64 [n_reads + 1], rep_s, rep_e int32)."""
        cols = [read_len, qid, qs, qe, tid, ts, te]
        if any(x is None for x in cols):
            raise ValueError("fragment_overlaps needs read_len, qid, qs, qe, tid, ts, te")
        tab = [None, None, None] if fragments is None else list(fragments)
        rep = [None, None, None] if repeats is None or len(repeats) == 0 else list(repeats)
        if len(tab) != 3 or len(rep) != 3:
            raise ValueError("fragments is (frag_offset, frag_begin, frag_end), repeats is (rep_offset, rep_s, rep_e)")
        frag = load_side_library("frag")
        on_device, cols, _, (tab, rep), n_reads, n_rec = self._record_query(
            "fragment_overlaps", cols, tables={"fragments": tab, "repeats": rep},
            offsets_error="fragment_overlaps needs frag_offset and rep_offset as contiguous int64 CUDA tensors")
        fn = frag.raft_hip_frag_overlaps_device if on_device else frag.raft_hip_frag_overlaps_host
        n_frag = _csr_count(fragments is not None, tab)
        rows = self._own_rows("n_fragments") if fragments is None else n_frag
        n_rep = _csr_count(repeats is not None, rep)
        out = {k: _twin(rows, np.int32, qid if on_device else None) for k in ("frag_touch", "frag_span", "frag_contained", "frag_repeat")}
        out["read_contained"] = np.zeros(n_reads, np.int32)
        records = _Records(n_rec, *[M.address(c) for c in cols[1:]])
        table, annotation = _FragTable(n_frag, *[M.address(a) for a in tab]), _FragTable(n_rep, *[M.address(a) for a in rep])
        sm, err, secs = _FragSummary(), C.c_int64(-1), C.c_double(0.0)
        rc = fn(self._ctx, n_reads, M.ptr(cols[0]), C.byref(records), 1 if symmetric else 0, C.byref(table), C.byref(annotation),
                *[M.ptr(a) for a in out.values()], C.byref(sm), C.byref(err), C.byref(secs))
        self._check(rc, err.value)
        self.last_fragment_overlaps_seconds = secs.value
        out.update(_summary_dict(sm))
        return out

    # -- one row per repeat run ----------------------------------------------------------------
    last_repeat_stats_seconds = 0.0   # device time of the launches of the last repeat_stats()
    RUN_COUNTS = ("run_touch", "run_span", "run_inside")
    RUN_COVERAGE = ("run_windows", "run_cov_min", "run_cov_max", "run_high", "run_cov_sum")

    def repeat_stats(self, read_len, qid=None, qs=None, qe=None, tid=None, ts=None, te=None, *, symmetric: bool = False, repeats=None,
                     threshold=None) -> dict:
        """raft_hip_repeat_stats_device / _host (libraft_hip_rst.so): one row per repeat run -- ``run_touch``, ``run_span``,
        ``run_inside`` (int32: the overlap sides that reach into the run, cover it end to end, lie wholly inside it; sides counted as
        the census counts them under ``symmetric``), ``run_windows``, ``run_cov_min``, ``run_cov_max``, ``run_high`` (int32) and
        ``run_cov_sum`` (int64) over the run's windows of the finished pass's coverage (``run_high``: windows with coverage >=
        ``threshold``), ``run_flags`` (uint8: RST_EMPTY | RST_AT_START | RST_AT_END; 0 = interior), and the summary's counts.  All
        arrays are numpy.  ``threshold``: None = the context's high_cov = int(est_cov * cov_mul) under the parameters in force at
        this call (after a ``set_params`` those, not the finished pass's), 0 = no coverage part (the five coverage arrays are then
        None).  The columns are int32 torch tensors on this engine's device (``repeats`` must be tensors too) or numpy arrays (staged
        by the library); qid .. te all None = no records; ts / te may be None when ``symmetric``.
        ``repeats``: None = the annotation of this context's finished pass, else (rep_offset int64 [n_reads + 1], rep_s, rep_e int32)."""
        if read_len is None:
            raise ValueError("repeat_stats needs read_len")
        rec = [qid, qs, qe, tid, ts, te]
        have = qid is not None
        if have and (any(x is None for x in rec[:4]) or (ts is None) != (te is None) or (not symmetric and ts is None)):
            raise ValueError("repeat_stats needs qid, qs, qe, tid (and ts, te unless symmetric), or no record column at all")
        if not have and any(x is not None for x in rec):
            raise ValueError("repeat_stats needs qid, qs, qe, tid (and ts, te unless symmetric), or no record column at all")
        if threshold is None:
            threshold = int(self.params.est_cov * self.params.cov_mul)
        rep = [None, None, None] if repeats is None else list(repeats)
        if len(rep) != 3:
            raise ValueError("repeats is (rep_offset, rep_s, rep_e)")
        rst = load_side_library("rst")
        on_device, cols, _, (rep,), n_reads, n_rec = self._record_query(
            "repeat_stats", [read_len] + [x for x in rec if x is not None], tables={"repeats": rep},
            offsets_error="repeat_stats needs rep_offset as a contiguous int64 CUDA tensor")
        fn = rst.raft_hip_repeat_stats_device if on_device else rst.raft_hip_repeat_stats_host
        n_rep = _csr_count(repeats is not None, rep)
        rows = self._own_rows("n_repeats") if repeats is None else n_rep
        out = {k: np.zeros(rows, np.int32) for k in self.RUN_COUNTS}
        out.update({k: (np.zeros(rows, np.int64 if k == "run_cov_sum" else np.int32) if threshold != 0 else None) for k in self.RUN_COVERAGE})
        out["run_flags"] = np.zeros(rows, np.uint8)
        fields = cols[1:] + [None] * (7 - len(cols))
        records = _Records(n_rec, *[M.address(c) for c in fields])
        sm, err, secs = _RstSummary(), C.c_int64(-1), C.c_double(0.0)
        rc = fn(self._ctx, n_reads, M.ptr(cols[0]), C.byref(records) if have else None, 1 if symmetric else 0, n_rep, *[M.ptr(a) for a in rep],
                int(threshold), *[M.ptr(a) for a in out.values()], C.byref(sm), C.byref(err), C.byref(secs))
        self._check(rc, err.value)
        self.last_repeat_stats_seconds = secs.value
        out.update(_summary_dict(sm))
        return out

    # -- which records go into a job at all -------------------------------------------------------
    last_filter_overlaps_seconds = 0.0   # device time of the launches of the last filter_overlaps()

    def filter_overlaps(self, qid, qs, qe, tid, ts, te, matches=None, block=None, *, min_identity_permille: int = 0, min_span: int = 0,
                        out=None) -> dict:
        """raft_hip_filter_overlaps_device / _host (libraft_hip_flt.so): the records with ``matches * 1000 >= min_identity_permille *
        block`` (``block`` > 0, ``matches`` >= 0; PAF columns 10 and 11) and ``qe - qs >= min_span and te - ts >= min_span``, in
        their order; 0 switches a rule off, and ``matches`` / ``block`` may be None without the identity rule.  -> ``columns`` (the
        six kept columns, views of length ``n_kept``: what ``run_device`` / ``run_host`` / ``census`` take), ``n_kept``,
        ``below_identity``, ``below_span`` (a record may count in both), ``first_kept`` (index in the input, -1 = none),
        ``symmetric`` (the symmetric flag of the kept stream) and ``kernel_seconds``.  The columns are int32 torch tensors on this
        engine's device -- the kept columns then go into ``out`` (six such tensors of the input's length that overlap no input) or
        into tensors from ``device_tensor``, which live until ``device_free`` or the context's end -- or numpy arrays (staged by the library), where ``out`` may be the input arrays
        themselves: the stream is then compacted in place."""
        cols = [qid, qs, qe, tid, ts, te, matches, block]
        if out is not None and len(out) != 6:
            raise ValueError("filter_overlaps: out is six columns")
        flt = load_side_library("flt")
        on_device, cols, _, _, _, n_rec = self._record_query("filter_overlaps", cols, lead=0, device_out=out or ())
        fn = flt.raft_hip_filter_overlaps_device if on_device else flt.raft_hip_filter_overlaps_host
        # (``out`` is no input: it comes from the engine's allocator, or is the caller's and a numpy array in the host form)
        if on_device:
            if out is None:
                import torch
                out = [self.device_tensor(n_rec, torch.int32) for _ in range(6)]
        elif out is None:
            out = [np.empty(n_rec, np.int32) for _ in range(6)]
        elif any(not isinstance(o, np.ndarray) or o.dtype != np.int32 or not o.flags["C_CONTIGUOUS"] for o in out):
            raise TypeError("filter_overlaps needs out as contiguous int32 numpy arrays")
        if any(M.count(o) < n_rec for o in out):
            raise ValueError("filter_overlaps: every out column needs room for all records")
        sm, secs = _FltSummary(), C.c_double(0.0)
        rc = fn(self._ctx, n_rec, *[M.ptr(x) for x in cols], int(min_identity_permille), int(min_span), *[M.ptr(o) for o in out],
                C.byref(sm), C.byref(secs))
        self._check(rc)
        self.last_filter_overlaps_seconds = secs.value
        res = _summary_dict(sm)
        del res["n_records"]
        res["kernel_seconds"] = secs.value
        res["columns"] = tuple(o[: res["n_kept"]] for o in out)
        return res

    # -- what kind of overlap each record is, which end of each read it supports ---------------------
    last_overlap_ends_seconds = 0.0      # device time of the launches of the last overlap_ends()

    def overlap_ends(self, read_len, qid, qs, qe, tid, ts, te, strand, *, max_overhang: int = 1000, min_ratio_permille: int = 800,
                     symmetric: bool = False, kinds: bool = False) -> dict:
        """raft_hip_overlap_ends_device / _host (libraft_hip_end.so): every record under the rule of include/raft_hip_end.h -- an
        internal match, a containment, a dovetail at the query's 5' or 3' end -- with ``strand`` one uint8 per record (1: PAF field 5
        begins with '-'; ``hostio.load_paf(strand=True)`` gives it).  -> ``counts`` (int32 [5, n_reads]: the rows ``END_COUNTS``),
        ``status`` (uint8 [n_reads]: ``END_READ_*``), the summary's counts (``kind_*``, ``reads_*``, ``n_records``),
        ``kernel_seconds`` and, with ``kinds=True``, ``kinds`` (uint8 per record, ``END_*``: a torch tensor on the input's
        device, else a numpy array).  The columns are torch tensors on this engine's device (int32; strand uint8) or numpy
        arrays (staged by the library).  Unless ``symmetric`` a record counts on its target's row as well.  Independent of any pass."""
        cols = [read_len, qid, qs, qe, tid, ts, te]
        if any(x is None for x in cols) or strand is None:
            raise ValueError("overlap_ends needs read_len, the six columns and strand")
        end = load_side_library("end")
        on_device, cols, (strand,), _, n_reads, n_rec = self._record_query("overlap_ends", cols, rec_u8={"strand": strand})
        fn = end.raft_hip_overlap_ends_device if on_device else end.raft_hip_overlap_ends_host
        kind_out = _twin(n_rec, np.uint8, strand if on_device else None, zeroed=not on_device) if kinds else None   # (the kernel writes every byte)
        counts, status = np.zeros((5, n_reads), np.int32), np.zeros(n_reads, np.uint8)
        sm, err, secs = _EndSummary(), C.c_int64(-1), C.c_double(0.0)
        rc = fn(self._ctx, *_plain(cols), M.ptr(strand), int(max_overhang), int(min_ratio_permille), 1 if symmetric else 0, M.ptr(counts),
                M.ptr(status), M.ptr(kind_out), C.byref(sm), C.byref(err), C.byref(secs))
        self._check(rc, err.value)
        self.last_overlap_ends_seconds = secs.value
        res = {"counts": counts, "status": status, "kernel_seconds": secs.value}
        if kinds:
            res["kinds"] = kind_out
        res.update(_summary_dict(sm))
        return res

    # -- the best overlap of every read end, and whether it is mutual ----------------------------------
    last_best_overlaps_seconds = 0.0     # device time of the launches of the last best_overlaps()

    def best_overlaps(self, read_len, qid, qs, qe, tid, ts, te, strand, *, max_overhang: int = 1000, min_ratio_permille: int = 800,
                      symmetric: bool = False, skip=None) -> dict:
        """raft_hip_best_overlaps_device / _host (libraft_hip_best.so): per read and end (0 = 5', 1 = 3') the longest dovetail, under
        the rule of include/raft_hip_best.h, to a read that ``skip`` (uint8 per read, non-zero: left out; ``None``: nobody) does not
        flag -- ``overlap_ends``' ``status == END_READ_CONTAINED`` is the usual mask.  -> ``partner`` (int32 [n_reads, 2], -1: none),
        ``span`` (int32 [n_reads, 2], 0: none), ``flags`` (uint8 [n_reads]: ``BEST_*``), the summary's counts (``candidates``,
        ``left_out``, ``ends_best``, ``ends_mutual``, ``reads_*``, ``n_records``) and ``kernel_seconds``.  The columns are torch tensors
        on this engine's device (int32; strand and skip uint8) or numpy arrays (staged by the library).  Unless ``symmetric`` a record
        is a candidate at its target's end as well.  Independent of any pass."""
        cols = [read_len, qid, qs, qe, tid, ts, te]
        if any(x is None for x in cols) or strand is None:
            raise ValueError("best_overlaps needs read_len, the six columns and strand")
        best = load_side_library("best")
        on_device, cols, (strand, skip), _, n_reads, _ = self._record_query("best_overlaps", cols, rec_u8={"strand": strand}, read_u8={"skip": skip})
        fn = best.raft_hip_best_overlaps_device if on_device else best.raft_hip_best_overlaps_host
        if skip is not None and M.count(skip) != n_reads:
            raise ValueError("best_overlaps: skip is one byte per read")
        partner, span, flags = np.zeros((n_reads, 2), np.int32), np.zeros((n_reads, 2), np.int32), np.zeros(n_reads, np.uint8)
        sm, err, secs = _BestSummary(), C.c_int64(-1), C.c_double(0.0)
        rc = fn(self._ctx, *_plain(cols), M.ptr(strand), M.ptr(skip), int(max_overhang), int(min_ratio_permille), 1 if symmetric else 0,
                M.ptr(partner), M.ptr(span), M.ptr(flags), C.byref(sm), C.byref(err), C.byref(secs))
        self._check(rc, err.value)
        self.last_best_overlaps_seconds = secs.value
        res = {"partner": partner, "span": span, "flags": flags, "kernel_seconds": secs.value}
        res.update(_summary_dict(sm))
        return res

    # -- the unitigs of the best overlap graph -----------------------------------------------------------
    last_unitigs_seconds = 0.0           # device time of the launches of the last unitigs()
    last_unitigs_launches = 0            # ... and how many there were (the second ranking runs only if the table holds a cycle)

    def unitigs(self, read_len, partner, span, flags) -> dict:
        """raft_hip_unitigs_device / _host (libraft_hip_utg.so): the chains and cycles that the mutual best overlaps form, under the
        rule of include/raft_hip_utg.h.  ``partner``, ``span`` ([n_reads, 2] or [2 * n_reads]) and ``flags`` are what
        ``best_overlaps`` returned, as torch tensors on this engine's device (int32; flags uint8) or numpy arrays (staged by the
        library).  -> per read ``unitig``, ``index`` (int32; -1 for a read left out), ``offset`` (int64), ``orient`` (uint8, 1: '-');
        ``order`` (int32, the reads in layout order) with ``utg_off`` (int64 [U + 1]); per unitig ``utg_reads``, ``utg_length``,
        ``utg_circular``; ``summary`` (the counts of raft_hip_utg_summary), ``kernel_seconds`` and ``launches``.  A table that is not
        consistent raises RaftError(ERR_READ_ID) with the smallest such read as its index.  Independent of any pass."""
        arrs = [read_len, partner, span]
        if any(x is None for x in arrs) or flags is None:
            raise ValueError("unitigs needs read_len, partner, span and flags")
        utg = load_side_library("utg")
        # (no record columns: partner and span are per read end, and one sentence refuses all three lengths, so they are checked here)
        on_device, arrs, (flags,), _, n, _ = self._record_query("unitigs", arrs, lead=3, read_u8={"flags": flags})
        fn = utg.raft_hip_unitigs_device if on_device else utg.raft_hip_unitigs_host
        if M.count(arrs[1]) != 2 * n or M.count(arrs[2]) != 2 * n or M.count(flags) != n:
            raise ValueError("unitigs: partner and span are two values per read, flags one byte")
        unitig, index, order, utg_reads = (np.zeros(n, np.int32) for _ in range(4))
        offset, utg_off, utg_length = np.zeros(n, np.int64), np.zeros(n + 1, np.int64), np.zeros(n, np.int64)
        orient, utg_circular = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        sm, err, secs, launches = _UtgSummary(), C.c_int64(-1), C.c_double(0.0), C.c_int64(0)
        rc = fn(self._ctx, n, M.ptr(arrs[0]), M.ptr(arrs[1]), M.ptr(arrs[2]), M.ptr(flags), M.ptr(unitig), M.ptr(index), M.ptr(offset),
                M.ptr(orient), M.ptr(order), M.ptr(utg_off), M.ptr(utg_reads), M.ptr(utg_length), M.ptr(utg_circular), C.byref(sm),
                C.byref(err), C.byref(secs), C.byref(launches))
        self.last_unitigs_seconds, self.last_unitigs_launches = secs.value, launches.value
        self._check(rc, err.value)
        n_utg, placed = int(sm.unitigs), n - int(sm.reads_skipped)
        return {"unitig": unitig, "index": index, "offset": offset, "orient": orient, "order": order[:placed], "utg_off": utg_off[:n_utg + 1],
                "utg_reads": utg_reads[:n_utg], "utg_length": utg_length[:n_utg], "utg_circular": utg_circular[:n_utg],
                "summary": _summary_dict(sm), "kernel_seconds": secs.value, "launches": launches.value}

    # -- the connected components of the overlap graph ----------------------------------------------------
    last_components_seconds = 0.0        # device time of the launches of the last components()
    last_components_launches = 0         # ... and how many there were

    def components(self, read_len, qid, qs, qe, tid, ts, te, strand, max_overhang: int = 1000, min_ratio_permille: int = 800,
                   kind_mask: int = CC_KINDS_PROPER, symmetric: bool = False) -> dict:
        """raft_hip_components_device / _host (libraft_hip_cc.so): the connected components of the graph over all reads whose edges
        are the records with a kind of ``kind_mask`` (bit k: kind ``END_*`` k; ``CC_KINDS_PROPER``, ``CC_KINDS_ALL``) under the rule of
        include/raft_hip_end.h, as include/raft_hip_cc.h says.  -> per read ``component`` and ``degree`` (int32); per component, in
        the order of the smallest read ids, ``comp_first``, ``comp_reads`` (int32), ``comp_bases``, ``comp_sides`` (int64);
        ``summary`` (the counts of raft_hip_cc_summary), ``kernel_seconds`` and ``launches``.  The columns are torch tensors on this
        engine's device (int32; strand uint8) or numpy arrays (staged by the library).  Unless ``symmetric`` an edge counts in its
        target's degree as well.  Independent of any pass."""
        cols = [read_len, qid, qs, qe, tid, ts, te]
        if any(x is None for x in cols) or strand is None:
            raise ValueError("components needs read_len, the six columns and strand")
        cc = load_side_library("cc")
        on_device, cols, (strand,), _, n, _ = self._record_query("components", cols, rec_u8={"strand": strand})
        fn = cc.raft_hip_components_device if on_device else cc.raft_hip_components_host
        component, degree, comp_first, comp_reads = (np.zeros(n, np.int32) for _ in range(4))
        comp_bases, comp_sides = np.zeros(n, np.int64), np.zeros(n, np.int64)
        sm, err, secs, launches = _CcSummary(), C.c_int64(-1), C.c_double(0.0), C.c_int64(0)
        rc = fn(self._ctx, *_plain(cols), M.ptr(strand), int(max_overhang), int(min_ratio_permille), int(kind_mask), 1 if symmetric else 0,
                M.ptr(component), M.ptr(degree), M.ptr(comp_first), M.ptr(comp_reads), M.ptr(comp_bases), M.ptr(comp_sides), C.byref(sm),
                C.byref(err), C.byref(secs), C.byref(launches))
        self.last_components_seconds, self.last_components_launches = secs.value, launches.value
        self._check(rc, err.value)
        n_comp = int(sm.components)
        return {"component": component, "degree": degree, "comp_first": comp_first[:n_comp], "comp_reads": comp_reads[:n_comp],
                "comp_bases": comp_bases[:n_comp], "comp_sides": comp_sides[:n_comp], "summary": _summary_dict(sm),
                "kernel_seconds": secs.value, "launches": launches.value}

    # -- the string graph: the dovetails between the reads that stay, transitively reduced ---------------------
    last_string_graph_seconds = 0.0      # device time of the launches of the last string_graph()
    last_string_graph_launches = 0       # ... and how many there were

    def string_graph(self, read_len, qid, qs, qe, tid, ts, te, strand, *, max_overhang: int = 1000, min_ratio_permille: int = 800,
                     fuzz: int = 1000, symmetric: bool = False, skip=None, emit_removed: bool = False) -> dict:
        """raft_hip_string_graph_device / _host (libraft_hip_sg.so): one arc per pair of read ends among the dovetails between the reads
        that ``skip`` (uint8 per read, non-zero: left out; ``None``: nobody) does not flag, and which of them two nearer arcs imply
        within ``fuzz``, under the rule of include/raft_hip_sg.h.  -> per read end ``arcs`` and ``kept`` (int32 [n_reads, 2]); the
        table ``unitigs`` takes: ``partner``, ``span`` (int32 [n_reads, 2]) and ``flags`` (uint8 [n_reads], ``BEST_*``); the edge list
        ``SG_EDGE_COLUMNS`` of length ``n_out`` in ascending (u, w), node u = 2 * read + end -- the surviving edges, or with
        ``emit_removed`` every edge, ``edge_flags`` (``SG_EDGE_*``) saying what fell; ``summary`` (the counts of raft_hip_sg_summary),
        ``kernel_seconds`` and ``launches``.  The columns are torch tensors on this engine's device (int32; strand and skip uint8) or
        numpy arrays (staged by the library).  Two calls: the size query, then the one that fills.  Independent of any pass."""
        cols = [read_len, qid, qs, qe, tid, ts, te]
        if any(x is None for x in cols) or strand is None:
            raise ValueError("string_graph needs read_len, the six columns and strand")
        sg = load_side_library("sg")
        on_device, cols, (strand, skip), _, n, _ = self._record_query("string_graph", cols, rec_u8={"strand": strand}, read_u8={"skip": skip})
        fn = sg.raft_hip_string_graph_device if on_device else sg.raft_hip_string_graph_host
        if skip is not None and M.count(skip) != n:
            raise ValueError("string_graph: skip is one byte per read")
        arcs, kept, partner, span = (np.zeros((n, 2), np.int32) for _ in range(4))
        flags = np.zeros(n, np.uint8)
        per_read = [M.ptr(a) for a in (arcs, kept, partner, span, flags)]
        sm, err, secs, launches, n_out = _SgSummary(), C.c_int64(-1), C.c_double(0.0), C.c_int64(0), C.c_int64(0)
        head = [self._ctx, *_plain(cols), M.ptr(strand), M.ptr(skip), int(max_overhang), int(min_ratio_permille), 1 if symmetric else 0, int(fuzz),
                1 if emit_removed else 0]
        tail = [C.byref(n_out), C.byref(sm), C.byref(err), C.byref(secs), C.byref(launches)]
        rc = fn(*head, 0, *per_read, *([C.c_void_p(0)] * 6), *tail)
        self.last_string_graph_seconds, self.last_string_graph_launches = secs.value, launches.value
        self._check(rc, err.value)
        m = int(n_out.value)
        edges = {k: np.zeros(m, np.uint8 if k == "edge_flags" else np.int32) for k in SG_EDGE_COLUMNS}
        if m > 0:
            rc = fn(*head, m, *per_read, *[M.ptr(a) for a in edges.values()], *tail)
            self.last_string_graph_seconds, self.last_string_graph_launches = secs.value, launches.value
            self._check(rc, err.value)
        return {"arcs": arcs, "kept": kept, "partner": partner, "span": span, "flags": flags, **edges, "n_out": m, "summary": _summary_dict(sm),
                "kernel_seconds": secs.value, "launches": launches.value}

    # -- the containment forest, and the forest on a unitig layout -------------------------------------------
    last_containment_seconds = 0.0       # device time of the launches of the last containment()
    last_place_contained_seconds = 0.0   # ... of the last place_contained()

    def containment(self, read_len, qid, qs, qe, tid, ts, te, strand, *, max_overhang: int = 1000, min_ratio_permille: int = 800,
                    symmetric: bool = False) -> dict:
        """raft_hip_containment_device / _host (libraft_hip_ctn.so): in which read every contained read sits, where and on which
        strand, and its place in the read its chain of containers ends in, under the rule of include/raft_hip_ctn.h.  -> per read
        ``parent`` (int32, -1: none), ``pos``, ``span``, ``root``, ``root_pos``, ``depth``, ``children`` (int32), ``flags`` (uint8,
        ``CTN_*``), and in the rows of the roots ``tree_reads`` (int32), ``tree_bases`` (int64), ``tree_depth`` (int32); ``summary``
        (the counts of raft_hip_ctn_summary, ``launches`` among them) and ``kernel_seconds``.  The columns are torch tensors on this
        engine's device (int32; strand uint8) or numpy arrays (staged by the library).  Unless ``symmetric`` a record of kind
        ``END_TARGET_CONTAINED`` places its target as well.  Independent of any pass."""
        cols = [read_len, qid, qs, qe, tid, ts, te]
        if any(x is None for x in cols) or strand is None:
            raise ValueError("containment needs read_len, the six columns and strand")
        ctn = load_side_library("ctn")
        on_device, cols, (strand,), _, n, _ = self._record_query("containment", cols, rec_u8={"strand": strand})
        fn = ctn.raft_hip_containment_device if on_device else ctn.raft_hip_containment_host
        out = {k: np.zeros(n, dt) for k, dt in CTN_PER_READ}
        sm, err, secs = _CtnSummary(), C.c_int64(-1), C.c_double(0.0)
        rc = fn(self._ctx, *_plain(cols), M.ptr(strand), int(max_overhang), int(min_ratio_permille), 1 if symmetric else 0,
                *[M.ptr(a) for a in out.values()], C.byref(sm), C.byref(err), C.byref(secs))
        self.last_containment_seconds = secs.value
        self._check(rc, err.value)
        return {**out, "summary": _summary_dict(sm), "kernel_seconds": secs.value}

    def place_contained(self, read_len, forest, unitig, offset, orient, utg_length) -> dict:
        """raft_hip_place_contained_device / _host (libraft_hip_ctn.so): the forest ``containment`` returned (``forest``: its dict, of
        which ``root``, ``root_pos`` and ``flags`` are read) laid onto the layout ``unitigs`` returned (``unitig``, ``offset``,
        ``orient`` per read; ``utg_length`` per unitig), under the rule of include/raft_hip_ctn.h.  -> per read ``placed_unitig``
        (int32, -1: unplaced), ``start`` (int64), ``placed_orient`` (uint8, 1: '-'); per unitig ``placed_reads`` (int32, the backbone
        included), ``placed_bases`` and ``depth_permille`` (int64); ``summary`` (the counts of raft_hip_place_summary) and
        ``kernel_seconds``.  All arrays are torch tensors on this engine's device (int32; offset and utg_length int64; flags and
        orient uint8) or all numpy arrays (staged by the library).  A table that names a unitig or a root outside its range raises
        RaftError(ERR_READ_ID) with the smallest such read as its index.  No wrap on circular unitigs."""
        given = [read_len, forest["root"], forest["root_pos"], forest["flags"], unitig, offset, orient, utg_length]
        if any(x is None for x in given):
            raise ValueError("place_contained needs read_len, the forest, unitig, offset, orient and utg_length")
        ctn = load_side_library("ctn")
        on_device = all(hasattr(x, "is_cuda") and x.is_cuda for x in given)
        dtypes = (np.int32, np.int32, np.int32, np.uint8, np.int32, np.int64, np.uint8, np.int64)
        if on_device:
            import torch
            for x, dt in zip(given, dtypes):
                if x.dtype != getattr(torch, np.dtype(dt).name) or not x.is_contiguous():
                    raise TypeError("place_contained needs contiguous CUDA tensors: int32, but offset and utg_length int64, flags and orient uint8")
            self.use_torch_stream()
        else:
            given = [M.carray(x.cpu() if hasattr(x, "is_cuda") else x, dt) for x, dt in zip(given, dtypes)]
        n, n_utg = M.count(given[0]), M.count(given[7])
        if any(M.count(x) != n for x in given[1:7]):
            raise ValueError("place_contained: root, root_pos, flags, unitig, offset and orient are one value per read")
        fn = ctn.raft_hip_place_contained_device if on_device else ctn.raft_hip_place_contained_host
        out = {**{k: np.zeros(n, dt) for k, dt in PLACE_PER_READ}, **{k: np.zeros(n_utg, dt) for k, dt in PLACE_PER_UNITIG}}
        sm, err, secs = _PlaceSummary(), C.c_int64(-1), C.c_double(0.0)
        rc = fn(self._ctx, n, *[M.ptr(x) for x in given[:7]], n_utg, M.ptr(given[7]), *[M.ptr(a) for a in out.values()], C.byref(sm),
                C.byref(err), C.byref(secs))
        self.last_place_contained_seconds = secs.value
        self._check(rc, err.value)
        return {**out, "summary": _summary_dict(sm), "kernel_seconds": secs.value}

    # -- a string graph cleaned: the weak edges cut, the tips removed ----------------------------------------
    last_graph_clean_seconds = 0.0       # device time of the launches of the last graph_clean()
    last_graph_clean_launches = 0        # ... and how many there were

    def graph_clean(self, read_len, edge_u, edge_w, edge_span, *, skip=None, min_ratio_permille: int = 500, max_tip_reads: int = 4,
                    rounds: int = 3) -> dict:
        """raft_hip_graph_clean_device / _host (libraft_hip_cln.so): the edge list of a string graph (node u = 2 * read + end; what
        ``string_graph`` returned as ``edge_u``, ``edge_w``, ``edge_span`` is one) without the edges that are weak beside the best one
        at the same end (span * 1000 < ``min_ratio_permille`` * the end's greatest span) and without the dead-end chains of at most
        ``max_tip_reads`` reads that hang beside something greater, removed over at most ``rounds`` rounds, under the rule of
        include/raft_hip_cln.h.  -> per edge, in the caller's order, ``edge_state`` (uint8, ``CLN_WEAK_U | CLN_WEAK_W | CLN_TIP``; 0:
        stays) and ``edge_round`` (uint8); per read ``read_state`` (uint8, ``CLN_READ_*``) and ``read_round``; per read end ``arcs``,
        ``weak``, ``kept`` (int32 [n_reads, 2]); the table ``unitigs`` takes: ``partner``, ``span`` (int32 [n_reads, 2]) and ``flags``
        (uint8 [n_reads], ``BEST_*``); ``summary`` (the counts of raft_hip_cln_summary), ``kernel_seconds`` and ``launches``.  The
        arrays are torch tensors on this engine's device (int32; skip uint8) or numpy arrays (staged by the library).  A bad edge
        raises RaftError(ERR_READ_ID) with the smallest such edge as its index.  Independent of any pass."""
        cols = [read_len, edge_u, edge_w, edge_span]
        if any(x is None for x in cols):
            raise ValueError("graph_clean needs read_len, edge_u, edge_w and edge_span")
        cln = load_side_library("cln")
        on_device, cols, (skip,), _, n, n_edges = self._record_query("graph_clean", cols, read_u8={"skip": skip})
        fn = cln.raft_hip_graph_clean_device if on_device else cln.raft_hip_graph_clean_host
        if skip is not None and M.count(skip) != n:
            raise ValueError("graph_clean: skip is one byte per read")
        per_edge = {k: np.zeros(n_edges, np.uint8) for k in ("edge_state", "edge_round")}
        per_read = {k: np.zeros(n, np.uint8) for k in ("read_state", "read_round")}
        per_end = {k: np.zeros((n, 2), np.int32) for k in ("arcs", "weak", "kept", "partner", "span")}
        flags = np.zeros(n, np.uint8)
        sm, err, secs, launches = _ClnSummary(), C.c_int64(-1), C.c_double(0.0), C.c_int64(0)
        rc = fn(self._ctx, n, M.ptr(cols[0]), M.ptr(skip), n_edges, M.ptr(cols[1]), M.ptr(cols[2]), M.ptr(cols[3]), int(min_ratio_permille),
                int(max_tip_reads), int(rounds), *[M.ptr(a) for a in (*per_edge.values(), *per_read.values(), *per_end.values(), flags)],
                C.byref(sm), C.byref(err), C.byref(secs), C.byref(launches))
        self.last_graph_clean_seconds, self.last_graph_clean_launches = secs.value, launches.value
        self._check(rc, err.value)
        return {**per_edge, **per_read, **per_end, "flags": flags, "summary": _summary_dict(sm), "kernel_seconds": secs.value,
                "launches": launches.value}

    # -- the overlaps between the fragments ------------------------------------------------------------------
    last_lift_overlaps_seconds = 0.0     # device time of the launches of the last lift_overlaps()

    def lift_overlaps(self, qid, qs, qe, tid, ts, te, strand, fragments=None, min_len: int = 1) -> dict:
        """raft_hip_lift_overlaps_device / _host (libraft_hip_lift.so): every record cut at the fragment bounds of both of its reads
        and shifted into fragment coordinates, under the rule of include/raft_hip_lift.h; pairs shorter than ``min_len`` on either
        side are dropped.  ``strand`` is one uint8 per record (1: PAF field 5 begins with '-').  -> the eight columns ``LIFT_COLUMNS``
        of length ``n_out`` (``qfrag`` / ``tfrag``: global row indices of the table; ``src``: the record an output came from), the
        summary's counts (``n_records``, ``n_out``, ``records_none``, ``records_cut``, ``pairs_dropped``, ``most_per_record``) and
        ``kernel_seconds``.  The columns are torch tensors on this engine's device (int32; strand uint8; the outputs are then tensors
        there and ``fragments`` must be tensors too) or numpy arrays (staged by the library).  ``fragments``: None = the rows of this
        context's finished pass, else (frag_offset int64 [n_reads + 1], frag_begin, frag_end int32).  Two calls: the size query, then
        the one that fills."""
        cols = [qid, qs, qe, tid, ts, te]
        if any(x is None for x in cols) or strand is None:
            raise ValueError("lift_overlaps needs the six columns and strand")
        tab = [None, None, None] if fragments is None else list(fragments)
        if len(tab) != 3:
            raise ValueError("fragments is (frag_offset, frag_begin, frag_end)")
        lift = load_side_library("lift")
        on_device, cols, (strand,), (tab,), _, n_rec = self._record_query(
            "lift_overlaps", cols, lead=0, rec_u8={"strand": strand}, tables={"fragments": tab}, tables_vote=True,
            offsets_error="lift_overlaps needs frag_offset as a contiguous int64 CUDA tensor")
        fn = lift.raft_hip_lift_overlaps_device if on_device else lift.raft_hip_lift_overlaps_host
        # (no read_len to measure the table against: the offsets say how many reads there are, and the table is checked here)
        if fragments is None:
            n_reads = self._own_rows("n_reads")
        else:
            if tab[0] is None or (tab[1] is None) != (tab[2] is None) or M.count(tab[0]) < 1 or (tab[1] is not None and M.count(tab[1]) != M.count(tab[2])):
                raise ValueError("fragments is (offsets [n_reads + 1], two arrays of one length)")
            n_reads = M.count(tab[0]) - 1
        records = _Records(n_rec, *[M.address(c) for c in cols])
        table = _FragTable(_csr_count(fragments is not None, tab), *[M.address(a) for a in tab])
        sm, err, secs = _LiftSummary(), C.c_int64(-1), C.c_double(0.0)
        null = [C.c_void_p(0)] * 8
        rc = fn(self._ctx, n_reads, C.byref(records), M.ptr(strand), C.byref(table), int(min_len), 0, *null, C.byref(sm), C.byref(err), C.byref(secs))
        self._check(rc, err.value)
        n_out, seconds = int(sm.n_out), secs.value
        out = {k: _twin(n_out, np.uint8 if k == "rev" else np.int32, qid if on_device else None, zeroed=False) for k in LIFT_COLUMNS}
        if n_out > 0:
            rc = fn(self._ctx, n_reads, C.byref(records), M.ptr(strand), C.byref(table), int(min_len), n_out, *[M.ptr(a) for a in out.values()],
                    C.byref(sm), C.byref(err), C.byref(secs))
            self._check(rc, err.value)
            seconds = secs.value
        self.last_lift_overlaps_seconds = seconds
        out.update(_summary_dict(sm))
        out["kernel_seconds"] = seconds
        return out

    def census(self, read_len, qid, qs, qe, tid, ts=None, te=None, symmetric: bool = False) -> dict:
        """raft_hip_census_device / _host: ``intervals`` (int32 [n_reads]: what a pass piles up on each read under ``symmetric``),
        ``contained`` (uint8 flags: bit 0 through a query side, bit 1 through a target side) and ``n_contained``.  The columns are
        int32 torch tensors on this engine's device, or numpy arrays (staged by the library); ts / te may be None when
        ``symmetric``.  Independent of any pass."""
        cols = [read_len, qid, qs, qe, tid] + ([] if symmetric else [ts, te])
        if any(x is None for x in cols[:4]) or (not symmetric and (ts is None or te is None)):
            raise ValueError("census needs read_len, qid, qs, qe (and ts, te unless symmetric)")
        on_device, cols, _, _, n_reads, _ = self._record_query("census", cols)
        fn = self._lib.raft_hip_census_device if on_device else self._lib.raft_hip_census_host
        args = _plain(cols) + ((C.c_void_p(0),) * 2 if symmetric else ())
        intervals, contained = np.zeros(n_reads, np.int32), np.zeros(n_reads, np.uint8)
        n_cont, err, secs = C.c_int64(0), C.c_int64(-1), C.c_double(0.0)
        rc = fn(self._ctx, *args, 1 if symmetric else 0, M.ptr(intervals), M.ptr(contained), C.byref(n_cont), C.byref(err), C.byref(secs))
        self._check(rc, err.value)
        self.last_census_seconds = secs.value
        return {"intervals": intervals, "contained": contained, "n_contained": int(n_cont.value)}

    def packed_device(self) -> dict | None:
        """Zero-copy torch views of the encoding the finished pass holds (raft_hip_packed_device), or None when the pass
        wrote int32: ``cov8`` (uint8; for width 2 the uint16 codes as an int16 tensor -- same bits, ``.view(torch.uint16)`` or
        ``& 0xFFFF`` after widening), ``exc_index`` / ``exc_value`` in no particular order."""
        import torch
        w, n = C.c_int32(0), C.c_int64(0)
        codes, ei, ev = C.c_void_p(), C.c_void_p(), C.c_void_p()
        self._check(self._lib.raft_hip_packed_device(self._ctx, C.byref(w), C.byref(codes), C.byref(ei), C.byref(ev), C.byref(n)))
        if w.value == 0:
            return None
        (key, _, size), *anchor = _COVERAGE[w.value]
        wide = w.value == 2
        res = {"width": w.value, key: _view(self, codes.value, size(self.summary.n_bins), "<i2" if wide else "|u1", torch.int16 if wide else torch.uint8)}
        if anchor:                            # delta4: two windows per byte + block anchors
            an, na = C.c_void_p(), C.c_int64(0)
            self._check(self._lib.raft_hip_packed_anchor_device(self._ctx, C.byref(an), C.byref(na)))
            res[anchor[0][0]] = _view(self, an.value, na.value, "<i4", torch.int32)
        res["exc_index"], res["exc_value"] = _view(self, ei.value, n.value, "<i8", torch.int64), _view(self, ev.value, n.value, "<i4", torch.int32)
        return res


class Slice:
    """One rank's part of a pre-split PAF (raft_hip_slice): the slice's query coordinates on the device and, on the host, its
    grouped form -- int64 [n_runs, n_reads_total + 1], where every read of the whole set begins in every sorted run of the slice
    (raft_amd.hostio.group_offsets on the slice's query column)."""

    def __init__(self, rec_offset, qs, qe=None, device_offsets=False):
        """``qe=None``: ``qs`` holds window records (one int32-viewed word per record, hostio.pack_windows) -- one column travels.
        ``device_offsets``: keep a copy of the offsets on the slice's device (raft_hip_slice::d_rec_offset), so that exchanging the
        same slice again uploads nothing."""
        self.off = M.carray(rec_offset, np.int64)
        if self.off.ndim != 2 or not (1 <= self.off.shape[0] <= 4):
            raise ValueError("Slice: rec_offset must be [n_runs (1..4), n_reads_total + 1]")
        _need_int32_cuda("Slice needs", (qs, qe))
        self.qs, self.qe = qs, qe
        self.ptrs = None                                      # group_sides: where the context's columns lie (an empty tensor has no address)
        self.d_off = None
        if device_offsets:
            import torch
            self.d_off = torch.as_tensor(self.off).to(qs.device)

    def c(self) -> "_Slice":
        d_qs, d_qe = self.ptrs or (M.address(self.qs), M.address(self.qe))
        return _Slice(int(self.qs.numel()), int(self.off.shape[0]), self.off.ctypes.data, d_qs, d_qe, M.address(self.d_off))


def _received_views(eng, r: "_Received") -> dict:
    """Zero-copy torch views of what a context received (valid until its next exchange)."""
    import torch
    off = _view(eng, r.d_rec_offset, r.n_runs * (r.n_reads + 1), "<i8", torch.int64).reshape(r.n_runs, r.n_reads + 1)
    return {"n_reads": int(r.n_reads), "n_rec": int(r.n_rec), "n_runs": int(r.n_runs), "rec_offset": off,
            "qs": _view(eng, r.d_qs, r.n_rec, "<i4", torch.int32),      # (window records when the slices carried them: then "qe" is None)
            "qe": _view(eng, r.d_qe, r.n_rec, "<i4", torch.int32) if (r.d_qe or r.n_rec == 0) else None}


def exchange_local(engines, bounds, slices) -> list:
    """raft_hip_exchange_local: one process, one Engine per rank; ``bounds`` = int64 [world + 1] read ranges, ``slices`` one
    Slice per rank (on that rank's device).  Returns, per rank, the grouped input it received (torch views)."""
    import torch
    lib = load_library()
    b = M.carray(bounds, np.int64)
    torch.cuda.synchronize()
    ctxs, w = _contexts(engines)
    sl = (_Slice * w)(*[s.c() for s in slices])
    out = (_Received * w)()
    rc = lib.raft_hip_exchange_local(ctxs, w, int(slices[0].off.shape[1] - 1), C.c_void_p(b.ctypes.data), sl, out)
    engines[0]._check(rc)
    return [_received_views(e, out[i]) for i, e in enumerate(engines)]


def _records(cols) -> "_Records":
    _need_int32_cuda("record columns must be", cols)
    return _Records(int(cols[0].numel()), *[M.address(t) for t in cols])


def presplit_symmetric_local(engines, slices_cols) -> bool:
    """raft_hip_presplit_symmetric_local: is the pre-split PAF symmetric?  ``slices_cols``: per rank its six device columns."""
    import torch
    lib = load_library()
    torch.cuda.synchronize()
    ctxs, w = _contexts(engines)
    recs = (_Records * w)(*[_records(c) for c in slices_cols])
    flag = C.c_int32(-1)
    engines[0]._check(lib.raft_hip_presplit_symmetric_local(ctxs, w, recs, C.byref(flag)))
    return bool(flag.value)


class Comm:
    """An RCCL communicator for raft_hip_exchange (one process per GPU).  ``unique_id()`` on rank 0, handed to the other ranks
    by the caller (e.g. a torch.distributed broadcast of its 128 bytes), then ``Comm(device, id, rank, world)`` everywhere."""

    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(128)
        rc = load_library().raft_hip_comm_unique_id(buf)
        if rc != OK:
            raise RaftError(rc, "ncclGetUniqueId (is librccl.so.1 loadable?)")
        return buf.raw

    def __init__(self, device: int, uid: bytes, rank: int, world: int):
        self._lib = load_library()
        self._comm = C.c_void_p()
        self.rank, self.world = rank, world
        rc = self._lib.raft_hip_comm_create(device, C.c_char_p(uid), rank, world, C.byref(self._comm))
        if rc != OK:
            raise RaftError(rc, "ncclCommInitRank")

    def exchange(self, eng, bounds, sl: Slice) -> dict:
        """raft_hip_exchange on the engine's stream; returns the grouped input this rank received (torch views)."""
        b = M.carray(bounds, np.int64)
        eng.use_torch_stream()
        cs, out = sl.c(), _Received()
        rc = self._lib.raft_hip_exchange(eng._ctx, self._comm, self.rank, self.world, int(sl.off.shape[1] - 1), C.c_void_p(b.ctypes.data),
                                         C.byref(cs), C.byref(out))
        eng._check(rc)
        return _received_views(eng, out)

    def symmetric(self, eng, cols) -> bool:
        """raft_hip_presplit_symmetric: the OR over the ranks of "my slice holds the mirror of record 0"."""
        eng.use_torch_stream()
        import torch
        torch.cuda.current_stream(eng.device).synchronize()
        rec, flag = _records(cols), C.c_int32(-1)
        eng._check(self._lib.raft_hip_presplit_symmetric(eng._ctx, self._comm, self.rank, self.world, C.byref(rec), C.byref(flag)))
        return bool(flag.value)

    def close(self):
        if self._comm.value:
            self._lib.raft_hip_comm_destroy(self._comm)
            self._comm = C.c_void_p()


def estimate_coverage(hist) -> CoverageEstimate:
    """raft_hip_estimate_coverage on a histogram whose last bin is the clamp bin (host arithmetic: needs no device)."""
    h = M.carray(hist, np.int64)
    if h.ndim != 1:
        raise ValueError("estimate_coverage needs a one-dimensional histogram")
    lib = load_library()
    e = _CovEstimate()
    rc = lib.raft_hip_estimate_coverage(M.ptr(h), int(h.size), C.byref(e))
    if rc != OK:
        raise RaftError(rc, lib.raft_hip_strerror(rc).decode())
    return CoverageEstimate(int(e.est_cov), int(e.median), int(e.windows), int(e.windows_covered), int(e.windows_clamped), float(e.mean))


def selftest(device: int = 0) -> int:
    return int(load_library().raft_hip_selftest(device))


def trim(device: int = 0, keep_bytes: int = 0) -> int:
    """Hands the device's pooled placement chunks beyond keep_bytes back to the driver; returns the bytes released."""
    return int(load_library().raft_hip_trim(device, keep_bytes))


def set_placement(spread: int) -> int:
    """Placement of buffers made from now on: 0 hipMalloc, k >= 1 shuffled chunks with k-fold spread (default 8); returns the old setting."""
    return int(load_library().raft_hip_set_placement(spread))


def pool_bytes(device: int = 0) -> int:
    """Bytes of physical chunks the placement pool of the device holds at the moment (mapped by no buffer)."""
    return int(load_library().raft_hip_pool_bytes(device))
