"""ctypes binding of libmpfitch.so (include/mpfitch.h) -- the product's Python face.

There is no fallback: if the HIP library is missing or no GPU is present the
calls raise.  Nothing here imports the oracle.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# (MPF_LIB_PATH: a differently built library, e.g. the experiments build of tools/scan_bounds.sh -- never the default)
LIB_PATH = os.environ.get("MPF_LIB_PATH") or os.path.join(HERE, "libmpfitch.so")
# Engines on several host threads launch side by side only as far as their streams get hardware queues of their own, and a
# persistent climb kernel holds its queue for a whole sweep.  The number of queues (GPU_MAX_HW_QUEUES) belongs to whoever starts
# the process: neither the library nor this module changes it.

DNA, AA, BIN, GENERIC = 0, 1, 2, 3      # PLL_DNA_DATA, PLL_AA_DATA, PLL_BINARY_DATA (2 states), PLL_GENERIC_32 (multistate)
TIE_FIRST, TIE_RANDOM = 0, 1

EXPORTS = [
    "mpf_last_error", "mpf_abi_version", "mpf_engine_create", "mpf_engine_create_sankoff", "mpf_engine_destroy",
    "mpf_set_weights",
    "mpf_get_geometry", "mpf_get_informative", "mpf_get_tip_vector", "mpf_set_tree", "mpf_get_tree",
    "mpf_reset_node_order", "mpf_score_tree", "mpf_score_trees", "mpf_pattern_scores", "mpf_site_scores", "mpf_compute_parsimony", "mpf_compute_parsimony_at",
    "mpf_encode_iqtree_states", "mpf_seed_ties", "mpf_set_tie_state", "mpf_get_tie_state", "mpf_tie_state_after",
    "mpf_set_rand_callback", "mpf_spr_scan", "mpf_spr_sweep_scan", "mpf_spr_sweep_costs", "mpf_get_node_order", "mpf_optimize_spr",
    "mpf_make_parsimony_tree", "mpf_stepwise_addition", "mpf_get_moves", "mpf_get_stats", "mpf_reset_stats",
    "mpf_set_option", "mpf_get_option", "mpf_get_scan_trace", "mpf_reps_create", "mpf_reps_scores", "mpf_reps_destroy",
    "mpf_ufboot_attach", "mpf_ufboot_refine_sweep", "mpf_ufboot_attach_sharded", "mpf_ufboot_detach", "mpf_ufboot_set_cutoff", "mpf_ufboot_set_ratchet_booking", "mpf_ufboot_set_mulhits", "mpf_ufboot_set_store_trees", "mpf_ufboot_get_duplicates", "mpf_ufboot_get_sample_trees", "mpf_ufboot_set_topboot", "mpf_ufboot_get_sample_top", "mpf_ufboot_set_distinct_iter", "mpf_ufboot_set_iteration", "mpf_ufboot_get_sample_iters", "mpf_ufboot_next_cutoff", "mpf_ufboot_set_cutoff_from_btrees", "mpf_ufboot_get_orig_logl", "mpf_rccl_available", "mpf_rccl_unique_id", "mpf_rccl_create", "mpf_rccl_destroy", "mpf_rccl_exchange", "mpf_rccl_allreduce_min", "mpf_rccl_counters", "mpf_ufboot_num_trees",
    "mpf_ufboot_tree_logl", "mpf_ufboot_get_state", "mpf_ufboot_get_tree", "mpf_ufboot_get_counters",
    "mpf_min_pars_score_patterns", "mpf_mst_scores", "mpf_segment_patterns", "mpf_remain_bounds",
    "mpf_cost_matrix_load", "mpf_cost_matrix_triangle_fix",
    "mpf_iq_random_nnis", "mpf_iq_perturb_weights", "mpf_iq_topology_key", "mpf_ufboot_adopt", "mpf_optimize_spr_many", "mpf_optimize_spr_many_round",
    "mpf_optimize_nni", "mpf_nni_scores", "mpf_get_nni_moves", "mpf_ufboot_optimize_nni", "mpf_nni_pattern_terms", "mpf_nni_pattern_lengths",
    "mpf_branch_substitutions", "mpf_branch_lengths",
    "mpf_polytomy_parsimony", "mpf_polytomy_branch_substitutions", "mpf_polytomy_branch_lengths",
    "mpf_insertion_costs", "mpf_place_taxa", "mpf_iq_parsimony_tree",
    "mpf_tbr_scan", "mpf_tbr_sweep_best", "mpf_apply_tbr", "mpf_optimize_tbr", "mpf_get_tbr_moves",
    "mpf_ufboot_tbr_sweep", "mpf_ufboot_optimize_tbr", "mpf_tbr_pattern_terms", "mpf_tbr_pattern_lengths",
    "mpf_split_counts", "mpf_split_support", "mpf_consensus_tree", "mpf_ufboot_summarize", "mpf_ufboot_summary_trees",
    "mpf_rf_distances",
    "mpf_split_counts_set", "mpf_split_support_set", "mpf_consensus_tree_set", "mpf_rf_distances_set",
]


class MpfError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libmpfitch error {code}: {msg}")
        self.code = code


def load_cost_matrix(file_or_keyword: str, n_states_alignment: int):
    """ParsTree::loadCostMatrixFile: ("fitch" | "e" | path) -> (cost[S, S] uint32 after the triangle repair, repaired?)"""
    cap = 64
    cost = np.zeros(cap * cap, dtype=np.uint32)
    S, ch = C.c_int32(), C.c_int32()
    _chk(load_library().mpf_cost_matrix_load(str(file_or_keyword).encode(), n_states_alignment, cap, _p(cost), C.byref(S), C.byref(ch)))
    return cost[:S.value * S.value].reshape(S.value, S.value).copy(), bool(ch.value)


class Config(C.Structure):
    _fields_ = [("device", C.c_int32), ("n_taxa", C.c_int32), ("n_patterns", C.c_int32), ("datatype", C.c_int32),
                ("keep_all_sites", C.c_int32), ("reserved", C.c_int32 * 3)]


class Stats(C.Structure):
    _fields_ = [("insertion_tests", C.c_uint64), ("newview_ops", C.c_uint64), ("scan_launches", C.c_uint64),
                ("view_launches", C.c_uint64), ("moves_applied", C.c_uint64), ("algorithmic_bytes", C.c_uint64),
                ("last_scan_kernel_ms", C.c_double), ("scan_kernel_ms_total", C.c_double),
                ("view_kernel_ms_total", C.c_double), ("host_plan_ms_total", C.c_double),
                ("host_views_ms_total", C.c_double), ("host_scan_ms_total", C.c_double),
                ("host_sweep_ms_total", C.c_double), ("plan_kernel_ms_total", C.c_double), ("plan_launches", C.c_uint64),
                ("climb_launches", C.c_uint64), ("climb_steps", C.c_uint64), ("climb_nodes", C.c_uint64),
                ("climb_moves", C.c_uint64), ("climb_ms_total", C.c_double)]

    def as_dict(self):
        return {f: getattr(self, f) for f, _ in self._fields_}


_lib = None


class BbSummary(C.Structure):
    """mpf_bb_summary (include/mpfitch.h)"""
    _fields_ = [("split_cap", C.c_int32), ("bits", C.c_void_p), ("count", C.c_void_p),
                ("target_back", C.c_void_p), ("branch_cap", C.c_int32), ("node1", C.c_void_p), ("node2", C.c_void_p), ("support", C.c_void_p),
                ("threshold", C.c_double), ("first", C.c_void_p), ("nbr", C.c_void_p), ("support_of_inner", C.c_void_p),
                ("n_trees", C.c_int32), ("n_distinct", C.c_int32), ("n_branches", C.c_int32), ("n_inner", C.c_int32),
                ("total_weight", C.c_int64)]


class TreeSet(C.Structure):
    """mpf_tree_set (include/mpfitch.h): record-format trees, then trees given as neighbour lists"""
    _fields_ = [("n_records", C.c_int32), ("backs", C.c_void_p), ("n_lists", C.c_int32), ("n_inner", C.c_void_p),
                ("first", C.c_void_p), ("nbr", C.c_void_p)]


SUMMARY_AUTO, SUMMARY_DEFAULT, SUMMARY_MULHITS, SUMMARY_TOPBOOT = -1, 0, 1, 2
RF_ALL_PAIRS, RF_ADJACENT, RF_TWO_SETS = 0, 1, 2       # MPF_RF_* (include/mpfitch.h)


def load_library():
    """Load libmpfitch.so; raises if it has not been built (no silent fallback)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise FileNotFoundError(f"{LIB_PATH} not built: run `python -c 'import __graft_entry__ as g; g.build()'`")
        L = C.CDLL(LIB_PATH)
        L.mpf_last_error.restype = C.c_char_p
        vp = C.c_void_p
        L.mpf_engine_create.argtypes = [C.POINTER(vp), C.POINTER(Config), vp, vp]
        L.mpf_engine_create_sankoff.argtypes = [C.POINTER(vp), C.POINTER(Config), vp, vp, vp]
        L.mpf_engine_destroy.argtypes = [vp]
        L.mpf_engine_destroy.restype = None
        L.mpf_set_weights.argtypes = [vp, vp]
        L.mpf_get_geometry.argtypes = [vp, vp, vp, vp, vp]
        L.mpf_get_informative.argtypes = [vp, vp]
        L.mpf_get_tip_vector.argtypes = [vp, C.c_int32, vp]
        L.mpf_set_tree.argtypes = [vp, vp]
        L.mpf_get_tree.argtypes = [vp, vp]
        L.mpf_reset_node_order.argtypes = [vp]
        L.mpf_score_tree.argtypes = [vp, vp]
        L.mpf_score_trees.argtypes = [vp, C.c_int32, vp, vp]
        L.mpf_pattern_scores.argtypes = [vp, vp, vp]
        L.mpf_site_scores.argtypes = [vp, vp, C.c_int32, vp]
        L.mpf_compute_parsimony.argtypes = [vp, vp, vp, vp]
        L.mpf_compute_parsimony_at.argtypes = [vp, vp, C.c_int32, vp, vp]
        L.mpf_encode_iqtree_states.argtypes = [C.c_int32, vp, C.c_int64, vp]
        L.mpf_seed_ties.argtypes = [vp, C.c_int32, C.c_int32]
        L.mpf_set_tie_state.argtypes = [vp, C.c_uint64]
        L.mpf_get_tie_state.argtypes = [vp, vp]
        L.mpf_tie_state_after.argtypes = [C.c_uint64, C.c_uint64]
        L.mpf_tie_state_after.restype = C.c_uint64
        L.mpf_spr_scan.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp]
        L.mpf_spr_sweep_scan.argtypes = [vp, C.c_int32, C.c_int32, vp, vp]
        L.mpf_spr_sweep_costs.argtypes = [vp, C.c_int32, C.c_int32, C.c_uint64, vp, vp, vp]
        L.mpf_get_node_order.argtypes = [vp, vp]
        L.mpf_optimize_spr.argtypes = [vp, C.c_int32, C.c_int32, vp]
        L.mpf_make_parsimony_tree.argtypes = [vp, C.c_int64, C.c_int32, vp]
        L.mpf_stepwise_addition.argtypes = [vp, C.c_int64, vp, vp, vp]
        L.mpf_get_moves.argtypes = [vp, C.c_int32, vp, vp, vp, vp]
        L.mpf_get_stats.argtypes = [vp, C.POINTER(Stats)]
        L.mpf_reset_stats.argtypes = [vp]
        L.mpf_set_option.argtypes = [vp, C.c_char_p, C.c_int64]
        L.mpf_get_option.argtypes = [vp, C.c_char_p, C.POINTER(C.c_int64)]
        L.mpf_get_scan_trace.argtypes = [vp, vp, C.c_uint64, vp]
        L.mpf_reps_create.argtypes = [C.POINTER(vp), C.c_int32, C.c_int32, C.c_int32, vp]
        L.mpf_reps_scores.argtypes = [vp, C.c_int32, vp, vp]
        L.mpf_reps_destroy.argtypes = [vp]
        L.mpf_reps_destroy.restype = None
        L.mpf_ufboot_attach.argtypes = [vp, C.c_int32, vp, C.c_double]
        L.mpf_ufboot_refine_sweep.argtypes = [vp, C.c_int32, vp, vp, vp, vp]
        L.mpf_ufboot_attach_sharded.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, C.c_double, vp, vp]
        L.mpf_ufboot_detach.argtypes = [vp]
        L.mpf_ufboot_set_cutoff.argtypes = [vp, C.c_double]
        L.mpf_ufboot_set_ratchet_booking.argtypes = [vp, C.c_int32]
        L.mpf_ufboot_set_mulhits.argtypes = [vp, C.c_int32]
        L.mpf_ufboot_set_store_trees.argtypes = [vp, C.c_int32]
        L.mpf_ufboot_get_duplicates.argtypes = [vp, C.POINTER(C.c_uint64)]
        L.mpf_ufboot_get_sample_trees.argtypes = [vp, C.c_int32, vp, C.c_int32, vp]
        L.mpf_ufboot_set_distinct_iter.argtypes = [vp, C.c_int32]
        L.mpf_ufboot_set_iteration.argtypes = [vp, C.c_int32]
        L.mpf_ufboot_get_sample_iters.argtypes = [vp, C.c_int32, vp, C.c_int32, vp]
        L.mpf_ufboot_set_topboot.argtypes = [vp, C.c_int32]
        L.mpf_ufboot_get_sample_top.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, vp]
        L.mpf_ufboot_next_cutoff.argtypes = [vp, C.c_int32, vp]
        L.mpf_ufboot_set_cutoff_from_btrees.argtypes = [vp, C.c_int32]
        L.mpf_rccl_unique_id.argtypes = [vp]
        L.mpf_rccl_create.argtypes = [vp, vp, C.c_int32, C.c_int32, C.c_int32]
        L.mpf_rccl_destroy.argtypes = [vp]
        L.mpf_rccl_destroy.restype = None
        L.mpf_rccl_allreduce_min.argtypes = [vp, vp, C.c_int32]
        L.mpf_rccl_counters.argtypes = [vp, vp, vp]
        L.mpf_ufboot_get_orig_logl.argtypes = [vp, vp]
        L.mpf_ufboot_num_trees.argtypes = [vp, vp]
        L.mpf_ufboot_tree_logl.argtypes = [vp, vp]
        L.mpf_ufboot_get_state.argtypes = [vp, vp, vp, vp]
        L.mpf_ufboot_get_tree.argtypes = [vp, C.c_int64, vp]
        L.mpf_ufboot_get_counters.argtypes = [vp, vp, vp, vp, vp]
        L.mpf_min_pars_score_patterns.argtypes = [C.c_int32, C.c_int32, C.c_int32, vp, vp]
        L.mpf_mst_scores.argtypes = [C.c_int32, vp, C.c_int32, C.c_int32, vp, vp]
        L.mpf_segment_patterns.argtypes = [C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp]
        L.mpf_remain_bounds.argtypes = [C.c_int32, C.c_int32, vp, vp, vp, vp]
        L.mpf_cost_matrix_load.argtypes = [C.c_char_p, C.c_int32, C.c_int32, vp, vp, vp]
        L.mpf_cost_matrix_triangle_fix.argtypes = [C.c_int32, vp, vp]
        L.mpf_optimize_spr_many.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp]
        L.mpf_optimize_spr_many_round.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp, vp]
        L.mpf_ufboot_adopt.argtypes = [vp, C.c_int32, vp, vp, vp, C.c_int32, vp, vp, vp]
        L.mpf_iq_random_nnis.argtypes = [C.c_int32, vp, C.c_int32, vp, vp]
        L.mpf_iq_perturb_weights.argtypes = [C.c_int32, vp, vp, C.c_int32, C.c_int32, vp, vp]
        L.mpf_iq_topology_key.argtypes = [C.c_int32, vp, vp]
        L.mpf_optimize_nni.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp]
        L.mpf_nni_scores.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, vp]
        L.mpf_get_nni_moves.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp]
        L.mpf_ufboot_optimize_nni.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp]
        L.mpf_nni_pattern_terms.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp]
        L.mpf_nni_pattern_lengths.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp]
        L.mpf_branch_substitutions.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, vp]
        L.mpf_branch_lengths.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp]
        L.mpf_polytomy_parsimony.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, vp]
        L.mpf_polytomy_branch_substitutions.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, C.c_int32, vp, vp, vp, vp]
        L.mpf_polytomy_branch_lengths.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp]
        L.mpf_insertion_costs.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, C.c_int32, vp, C.c_int32, vp, vp, vp, vp, vp]
        L.mpf_place_taxa.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, C.c_int32, vp, vp, vp, vp, vp, vp]
        L.mpf_iq_parsimony_tree.argtypes = [vp, vp, vp, vp, vp, vp, vp]
        L.mpf_tbr_scan.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, vp, vp, vp, vp, vp]
        L.mpf_tbr_sweep_best.argtypes = [vp, C.c_int32, vp, vp, vp, vp]
        L.mpf_apply_tbr.argtypes = [vp, C.c_int32, C.c_int32, C.c_int32, vp]
        L.mpf_optimize_tbr.argtypes = [vp, C.c_int32, C.c_int32, vp, vp]
        L.mpf_get_tbr_moves.argtypes = [vp, C.c_int32, vp, vp, vp, vp, vp]
        L.mpf_ufboot_tbr_sweep.argtypes = [vp, C.c_int32, vp, vp, vp, vp]
        L.mpf_ufboot_optimize_tbr.argtypes = [vp, C.c_int32, C.c_int32, vp, vp]
        L.mpf_tbr_pattern_terms.argtypes = [vp, C.c_int32, C.c_int32, C.c_int64, vp, vp, vp]
        L.mpf_tbr_pattern_lengths.argtypes = [vp, C.c_int32, C.c_int32, C.c_int64, vp, vp, vp]
        L.mpf_split_counts.argtypes = [vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, vp]
        L.mpf_split_support.argtypes = [vp, C.c_int32, vp, vp, vp, C.c_int32, vp, vp, vp, vp, vp]
        L.mpf_consensus_tree.argtypes = [vp, C.c_int32, vp, vp, C.c_double, vp, vp, vp, vp, vp]
        L.mpf_ufboot_summarize.argtypes = [vp, C.c_int32, C.POINTER(BbSummary)]
        L.mpf_ufboot_summary_trees.argtypes = [vp, C.c_int32, C.c_int32, vp, vp, vp, vp]
        L.mpf_rf_distances.argtypes = [vp, C.c_int32, C.c_int32, vp, C.c_int32, vp, C.c_int64, vp]
        ts = C.POINTER(TreeSet)
        L.mpf_split_counts_set.argtypes = [vp, ts, vp, C.c_int32, vp, vp, vp, vp]
        L.mpf_split_support_set.argtypes = [vp, ts, vp, C.c_int32, vp, vp, C.c_int32, vp, vp, vp, vp, vp]
        L.mpf_consensus_tree_set.argtypes = [vp, ts, vp, C.c_double, vp, vp, vp, vp, vp]
        L.mpf_rf_distances_set.argtypes = [vp, C.c_int32, ts, ts, C.c_int64, vp]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _chk(rc):
    if rc != 0:
        raise MpfError(rc, load_library().mpf_last_error().decode())


def min_pars_score_patterns(codes: np.ndarray, datatype: int = DNA) -> np.ndarray:
    """pllCalcMinParsScorePattern for every pattern (host only)."""
    codes = np.ascontiguousarray(codes, dtype=np.uint8)
    out = np.zeros(codes.shape[1], dtype=np.int32)
    _chk(load_library().mpf_min_pars_score_patterns(datatype, codes.shape[0], codes.shape[1], _p(codes), _p(out)))
    return out


def mst_scores(states: np.ndarray, cost: np.ndarray) -> np.ndarray:
    """ParsTree::findMstScore for every pattern (host only); states = IQ-TREE codes [n][P]."""
    states = np.ascontiguousarray(states, dtype=np.int8)
    cost = np.ascontiguousarray(cost, dtype=np.uint32)
    out = np.zeros(states.shape[1], dtype=np.uint32)
    _chk(load_library().mpf_mst_scores(cost.shape[0], _p(cost), states.shape[0], states.shape[1], _p(states), _p(out)))
    return out


def segment_patterns(ras_pars_score, frequency, n_informative: int, vcsize: int = 16) -> np.ndarray:
    """IQTree::doSegmenting: returns segment_upper[0 .. n_segments)."""
    r = np.ascontiguousarray(ras_pars_score, dtype=np.int32)
    f = np.ascontiguousarray(frequency, dtype=np.int32)
    up = np.zeros(len(r), dtype=np.int32)
    k = C.c_int32()
    _chk(load_library().mpf_segment_patterns(len(r), n_informative, vcsize, _p(r), _p(f), _p(up), C.byref(k)))
    return up[:k.value].copy()


def remain_bounds(segment_upper, min_unit_pars, weight) -> np.ndarray:
    """remain[s] = sum over positions >= segment_upper[s] of min_unit_pars * weight (all but the last segment)."""
    up = np.ascontiguousarray(segment_upper, dtype=np.int32)
    m = np.ascontiguousarray(min_unit_pars, dtype=np.int32)
    w = np.ascontiguousarray(weight, dtype=np.uint16)
    out = np.zeros(max(len(up) - 1, 1), dtype=np.int32)
    _chk(load_library().mpf_remain_bounds(len(m), len(up), _p(up), _p(m), _p(w), _p(out)))
    return out[:len(up) - 1]


def optimize_spr_many(engines, mintrav: int = 1, maxtrav: int = 6):
    """mpf_optimize_spr_many: one SPR hill climb per engine (tree, weights, tie stream set on each as for optimize_spr), all of them
    side by side -- a resident workgroup per climb, all of its sweeps inside ONE launch.  -> final lengths, one per engine."""
    n = len(engines)
    hs = (C.c_void_p * n)(*[e.h for e in engines])
    out = np.zeros(n, dtype=np.uint32)
    _chk(load_library().mpf_optimize_spr_many(hs, n, int(mintrav), int(maxtrav), _p(out)))
    return out


class ClimbBatch:
    """mpf_optimize_spr_many_round for callers with more climbs than engines: start(k) after setting engine k up (tree, weights, tie
    stream), round() runs one launch for every active climb and returns the engines whose climb has just finished."""

    def __init__(self, engines, mintrav: int = 1, maxtrav: int = 6):
        self.engines = list(engines)
        self.n = len(self.engines)
        self.hs = (C.c_void_p * self.n)(*[e.h for e in self.engines])
        self.state = np.zeros(self.n, dtype=np.uint8)
        self.scores = np.zeros(self.n, dtype=np.uint32)
        self.mintrav, self.maxtrav = int(mintrav), int(maxtrav)

    def start(self, k: int):
        self.state[k] = 1

    def active(self) -> int:
        return int((self.state != 0).sum())

    def round(self):
        before = self.state != 0
        _chk(load_library().mpf_optimize_spr_many_round(self.hs, self.n, self.mintrav, self.maxtrav, _p(self.state), _p(self.scores)))
        return [int(k) for k in np.nonzero(before & (self.state == 0))[0]]


def iq_random_nnis(back: np.ndarray, num_nni: int, tie_state: int):
    """IQTree::doRandomNNIs (iqtree.cpp:1083-1106) on a copy of `back` -> (perturbed back, stream state behind the draws, re-listings)."""
    b = np.ascontiguousarray(back, dtype=np.int32).copy()
    n = (len(b) // 3 + 1) // 2
    st = C.c_uint64(tie_state & ((1 << 64) - 1))
    rl = C.c_int32()
    _chk(load_library().mpf_iq_random_nnis(n, _p(b), int(num_nni), C.byref(st), C.byref(rl)))
    return b, int(st.value), int(rl.value)


def iq_perturb_weights(weights, informative, percent: int, add: int, tie_state: int):
    """Alignment::createPerturbAlignment (alignment.cpp:1915-1969) as pattern weights -> (weights, stream state behind the draws)."""
    w = np.ascontiguousarray(weights, dtype=np.int32)
    inf = np.ascontiguousarray(informative, dtype=np.uint8)
    out = np.zeros_like(w)
    st = C.c_uint64(tie_state & ((1 << 64) - 1))
    _chk(load_library().mpf_iq_perturb_weights(len(w), _p(w), _p(inf), int(percent), int(add), C.byref(st), _p(out)))
    return out, int(st.value)


def iq_topology_key(back: np.ndarray) -> bytes:
    """16-byte digest of the canonical unrooted topology (the key CandidateSet::topologies looks trees up by)."""
    b = np.ascontiguousarray(back, dtype=np.int32)
    n = (len(b) // 3 + 1) // 2
    key = np.zeros(2, dtype=np.uint64)
    _chk(load_library().mpf_iq_topology_key(n, _p(b), _p(key)))
    return key.tobytes()


def encode_iqtree_states(states: np.ndarray, datatype: int = DNA) -> np.ndarray:
    """Alignment::convertState codes -> PLL tip codes (host only, no GPU needed)."""
    states = np.ascontiguousarray(states, dtype=np.int8)
    out = np.zeros(states.shape, dtype=np.uint8)
    _chk(load_library().mpf_encode_iqtree_states(datatype, _p(states), states.size, _p(out)))
    return out


class Reps:
    """REPS contraction (IQTree::saveCurrentTree, iqtree.cpp:3411-3449): boot weights resident on the GPU."""

    def __init__(self, boot: np.ndarray, device: int = 0):
        boot = np.ascontiguousarray(boot, dtype=np.uint16)
        self.B, self.P = boot.shape
        h = C.c_void_p()
        _chk(load_library().mpf_reps_create(C.byref(h), device, self.B, self.P, _p(boot)))
        self.h = h

    def scores(self, pattern_pars: np.ndarray) -> np.ndarray:
        pp = np.ascontiguousarray(np.atleast_2d(pattern_pars), dtype=np.uint16)
        assert pp.shape[1] == self.P
        out = np.zeros((pp.shape[0], self.B), dtype=np.int32)
        _chk(load_library().mpf_reps_scores(self.h, pp.shape[0], _p(pp), _p(out)))
        return out

    def close(self):
        if getattr(self, "h", None):
            load_library().mpf_reps_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RcclComm:
    """The library's own RCCL communicator (include/mpfitch.h: mpf_rccl_*): event exchange of a sample-sharded online phase and the
    all-reduce of best scores, native -- no torch in the data path.  `uid`: 128 bytes from RcclComm.unique_id() on rank 0, carried
    to the other ranks by the caller (mpboot_amd.shard.native_comm does it over torch.distributed's store)."""

    def __init__(self, uid: bytes, rank: int, world: int, device: int = 0):
        L = load_library()
        self.h = C.c_void_p()
        buf = (C.c_uint8 * 128).from_buffer_copy(uid)
        _chk(L.mpf_rccl_create(C.byref(self.h), buf, rank, world, device))
        self.rank, self.world = rank, world
        self._users = 0                          # engines whose tracker holds self.h as its exchange argument

    @staticmethod
    def available() -> bool:
        return bool(load_library().mpf_rccl_available())

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        _chk(load_library().mpf_rccl_unique_id(buf))
        return bytes(buf)

    def allreduce_min(self, vals):
        v = np.ascontiguousarray(vals, dtype=np.uint32).copy()
        _chk(load_library().mpf_rccl_allreduce_min(self.h, _p(v), len(v)))
        return v

    def counters(self):
        a, b = C.c_uint64(), C.c_uint64()
        _chk(load_library().mpf_rccl_counters(self.h, C.byref(a), C.byref(b)))
        return {"exchanges": a.value, "overflows": b.value}

    def close(self):
        """Frees the native communicator.  Refused while an engine's tracker still has it registered as its exchange
        (mpf_ufboot_attach_sharded stored the raw handle: a later climb or the closing handshake would call into freed memory);
        detach or close those engines first."""
        if getattr(self, "h", None):
            if getattr(self, "_users", 0) > 0:
                raise MpfError(-1, "RcclComm.close(): %d engine(s) still attached through this communicator -- ufboot_detach() them first" % self._users)
            load_library().mpf_rccl_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FitchEngine:
    """One alignment resident on one MI355X; mirrors the reference's PLL-instance-level calls."""

    def __init__(self, codes: np.ndarray, weights=None, datatype: int = DNA, keep_all: bool = False, device: int = 0,
                 cost=None):
        """cost: optional [S, S] matrix -> weighted (Sankoff) parsimony, the reference's `-cost` mode"""
        L = load_library()
        codes = np.ascontiguousarray(codes, dtype=np.uint8)
        self.n, self.P = codes.shape
        if weights is None:
            weights = np.ones(self.P, dtype=np.int32)
        weights = np.ascontiguousarray(weights, dtype=np.int32)
        self._weights = weights.copy()           # the pattern weights in force (mpf_set_weights keeps it in step)
        self.weighted = cost is not None         # the Sankoff (-cost) engine
        cfg = Config(device, self.n, self.P, datatype, int(keep_all))
        h = C.c_void_p()
        if cost is None:
            _chk(L.mpf_engine_create(C.byref(h), C.byref(cfg), _p(codes), _p(weights)))
        else:
            cost = np.ascontiguousarray(cost, dtype=np.uint32)
            _chk(L.mpf_engine_create_sankoff(C.byref(h), C.byref(cfg), _p(codes), _p(weights), _p(cost)))
        self.h = h
        self.nrec = 3 * (2 * self.n - 1)
        s, w, ni, wp = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _chk(L.mpf_get_geometry(self.h, C.byref(s), C.byref(w), C.byref(ni), C.byref(wp)))
        self.S, self.W, self.num_informative, self.Wp = s.value, w.value, ni.value, wp.value

    def _drop_exchange(self):
        ex = getattr(self, "_ufb_exchange", None)
        if isinstance(ex, RcclComm):
            ex._users -= 1
        self._ufb_exchange = None

    def close(self):
        if getattr(self, "h", None):
            load_library().mpf_engine_destroy(self.h)
            self.h = None
            self._drop_exchange()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _refresh_geometry(self):
        s, w, ni, wp = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
        _chk(load_library().mpf_get_geometry(self.h, C.byref(s), C.byref(w), C.byref(ni), C.byref(wp)))
        self.S, self.W, self.num_informative, self.Wp = s.value, w.value, ni.value, wp.value

    def set_weights(self, w):
        w = np.ascontiguousarray(w, dtype=np.int32)
        _chk(load_library().mpf_set_weights(self.h, _p(w)))
        self._weights = w.copy()
        self._refresh_geometry()

    def weights(self):
        """The pattern weights in force (a copy)."""
        return self._weights.copy()

    def informative(self):
        f = np.zeros(self.P, dtype=np.int32)
        _chk(load_library().mpf_get_informative(self.h, _p(f)))
        return f

    def tip_vector(self, tip: int):
        out = np.zeros((self.S, self.W), dtype=np.uint32)
        _chk(load_library().mpf_get_tip_vector(self.h, tip, _p(out)))
        return out

    def set_tree(self, back):
        back = np.ascontiguousarray(back, dtype=np.int32)
        assert len(back) == self.nrec
        _chk(load_library().mpf_set_tree(self.h, _p(back)))

    def get_tree(self):
        back = np.empty(self.nrec, dtype=np.int32)
        _chk(load_library().mpf_get_tree(self.h, _p(back)))
        return back

    def reset_node_order(self):
        _chk(load_library().mpf_reset_node_order(self.h))

    def score_tree(self, back=None) -> int:
        if back is not None:
            self.set_tree(back)
        s = C.c_uint32()
        _chk(load_library().mpf_score_tree(self.h, C.byref(s)))
        return s.value

    def score_trees(self, backs):
        backs = np.ascontiguousarray(backs, dtype=np.int32)
        out = np.zeros(len(backs), dtype=np.uint32)
        _chk(load_library().mpf_score_trees(self.h, len(backs), _p(backs), _p(out)))
        return out

    def pattern_scores(self):
        out = np.zeros(self.P, dtype=np.uint16)
        tot = C.c_int32()
        _chk(load_library().mpf_pattern_scores(self.h, _p(out), C.byref(tot)))
        return out, tot.value

    def compute_parsimony(self, back=None, want_patterns: bool = True):
        """PhyloTree::computeParsimony(): (score, _pattern_pars)"""
        s = C.c_uint32()
        ptn = np.zeros(self.P, dtype=np.uint16) if want_patterns else None
        bp = None
        if back is not None:
            back = np.ascontiguousarray(back, dtype=np.int32)
            bp = _p(back)
        _chk(load_library().mpf_compute_parsimony(self.h, bp, C.byref(s), _p(ptn) if want_patterns else None))
        return s.value, ptn

    def seed_ties(self, mode: int, seed: int = 1):
        _chk(load_library().mpf_seed_ties(self.h, mode, seed))

    def set_tie_state(self, state: int):
        """Hand the 64-bit state of the host's SPRNG lcg64 stream over (mpf_set_tie_state)."""
        _chk(load_library().mpf_set_tie_state(self.h, state & ((1 << 64) - 1)))

    def tie_state(self) -> int:
        s = C.c_uint64()
        _chk(load_library().mpf_get_tie_state(self.h, C.byref(s)))
        return int(s.value)

    def site_scores(self, n_sites: int):
        """pllComputeSiteParsimony: lengths per expanded (weight-replicated) site of the kept patterns."""
        out = np.zeros(n_sites, dtype=np.int32)
        tot = C.c_int32()
        _chk(load_library().mpf_site_scores(self.h, _p(out), n_sites, C.byref(tot)))
        return out, tot.value

    def spr_scan(self, rec: int, mintrav: int = 1, maxtrav: int = 6, cap: int = 1 << 16):
        q = np.zeros(cap, dtype=np.int32)
        mp = np.zeros(cap, dtype=np.uint32)
        n_p, n_t = C.c_int32(), C.c_int32()
        _chk(load_library().mpf_spr_scan(self.h, rec, mintrav, maxtrav, cap, _p(q), _p(mp), C.byref(n_p), C.byref(n_t)))
        return q[:n_t.value].copy(), mp[:n_t.value].copy(), n_p.value

    def sweep_scan(self, mintrav: int = 1, maxtrav: int = 6):
        n = C.c_uint64()
        m = C.c_uint32()
        _chk(load_library().mpf_spr_sweep_scan(self.h, mintrav, maxtrav, C.byref(n), C.byref(m)))
        return n.value, m.value

    def sweep_costs(self, mintrav: int = 1, maxtrav: int = 6):
        """(n_tests, mp[n_tests], offsets[2n-1]): every insertion test of a whole sweep, prune nodes in sweep order"""
        L = load_library()
        n = C.c_uint64()
        _chk(L.mpf_spr_sweep_costs(self.h, mintrav, maxtrav, 0, None, None, C.byref(n)))
        mp = np.zeros(max(1, n.value), dtype=np.uint32)
        off = np.zeros(2 * self.n - 1, dtype=np.uint64)
        _chk(L.mpf_spr_sweep_costs(self.h, mintrav, maxtrav, n.value, _p(mp), _p(off), C.byref(n)))
        return n.value, mp[:n.value], off

    def node_order(self):
        recs = np.zeros(2 * self.n - 2, dtype=np.int32)
        _chk(load_library().mpf_get_node_order(self.h, _p(recs)))
        return recs

    def optimize_spr(self, mintrav: int = 1, maxtrav: int = 6) -> int:
        s = C.c_uint32()
        _chk(load_library().mpf_optimize_spr(self.h, mintrav, maxtrav, C.byref(s)))
        return s.value

    def make_parsimony_tree(self, seed: int, spr_dist: int) -> int:
        s = C.c_uint32()
        _chk(load_library().mpf_make_parsimony_tree(self.h, seed, spr_dist, C.byref(s)))
        return s.value

    def stepwise_addition(self, seed: int):
        best = np.zeros(self.n + 1, dtype=np.uint32)
        ins = np.zeros(self.n + 1, dtype=np.int32)
        s = C.c_uint32()
        _chk(load_library().mpf_stepwise_addition(self.h, seed, _p(best), _p(ins), C.byref(s)))
        return s.value, best, ins

    def moves(self):
        k = C.c_int32()
        L = load_library()
        _chk(L.mpf_get_moves(self.h, 0, None, None, None, C.byref(k)))
        a = np.zeros(k.value, dtype=np.int32)
        b = np.zeros(k.value, dtype=np.int32)
        s = np.zeros(k.value, dtype=np.uint32)
        if k.value:
            _chk(L.mpf_get_moves(self.h, k.value, _p(a), _p(b), _p(s), C.byref(k)))
        return a, b, s

    # ---- NNI hill climb (IQTree::optimizeNNI in MP mode: -nni_pars, -hclimb1_nni)
    def optimize_nni(self, root_taxon: int = 1, speednni: bool = True, max_steps: int = 50):
        """-> (length, nni_count, nni_steps); the tree is modified in place.

        A weighted engine (cost=...) serves this after set_option("nni_weighted", 1) only (default 0: MpfError -6, as before):
        the reference's -cost m -nni_pars, where the tree is a ParsTree -- every NNI scored by Sankoff rooted at its branch
        (node2's side the parent, ParsTree::computeParsimonyBranch), the tree's own length taken at the leaf root_taxon
        (ParsTree::computeParsimony), and NO rollback (iqtree.cpp:2258): a step that left the tree longer than its best NNI
        promised keeps its moves and is not counted; get_option("nni_kept_worse") counts such steps.  Not served there: a
        tracker attached, nni_pattern_terms, and -- unless set_option("nni_weighted_tracked", 1) as well -- ufboot_optimize_nni."""
        s, cnt, steps = C.c_uint32(), C.c_int32(), C.c_int32()
        _chk(load_library().mpf_optimize_nni(self.h, root_taxon, int(bool(speednni)), max_steps, C.byref(s), C.byref(cnt),
                                             C.byref(steps)))
        return s.value, cnt.value, steps.value

    def nni_scores(self, root_taxon: int = 1):
        """one full evaluation: (node1[m], node2[m], len[m][2]) for the m inner branches in evalNNIs() order; on a weighted engine
        under set_option("nni_weighted", 1) the two full weighted lengths, each rooted at its branch with node2's side the parent"""
        L = load_library()
        n = C.c_int32()
        _chk(L.mpf_nni_scores(self.h, root_taxon, 0, None, None, None, C.byref(n)))
        m = n.value
        a = np.zeros(max(m, 1), dtype=np.int32)
        b = np.zeros(max(m, 1), dtype=np.int32)
        ln = np.zeros(2 * max(m, 1), dtype=np.uint32)
        _chk(L.mpf_nni_scores(self.h, root_taxon, m, _p(a), _p(b), _p(ln), C.byref(n)))
        return a[:m].copy(), b[:m].copy(), ln[:2 * m].reshape(m, 2).copy()

    # ---- parsimony branch lengths (PhyloTree::fixNegativeBranch)
    def branch_substitutions(self, root_taxon: int = 1):
        """(node1[m], node2[m], subst[m]) for the m = 2 n - 3 branches of the current tree in fixNegativeBranch's order (pre-order
        from the leaf root_taxon, neighbours in slot order, node1 the end nearer that leaf): what computeParsimonyBranch hands back
        as branch_subst -- on a Fitch engine the weighted count of kept patterns whose two sides share no state, on a weighted
        engine (cost=...) the full length of the tree rooted at the branch (ParsTree's rule).  One kernel launch for all branches."""
        m = 2 * self.n - 3
        n = C.c_int32()
        a = np.zeros(m, dtype=np.int32)
        b = np.zeros(m, dtype=np.int32)
        s = np.zeros(m, dtype=np.uint32)
        _chk(load_library().mpf_branch_substitutions(self.h, root_taxon, m, _p(a), _p(b), _p(s), C.byref(n)))
        assert n.value == m
        return a, b, s

    def branch_lengths(self, n_sites: int, root_taxon: int = 1, unit_cost_parstree: bool = False):
        """(node1[m], node2[m], length[m] float64): the lengths fixNegativeBranch(force=True) gives the branches, from
        branch_substitutions, n_sites (the alignment's site count) and the number of states; unit_cost_parstree: a ParsTree under
        -cost fitch | e -- every branch takes the tree's Fitch length as its count (no effect on a weighted engine)"""
        m = 2 * self.n - 3
        n = C.c_int32()
        a = np.zeros(m, dtype=np.int32)
        b = np.zeros(m, dtype=np.int32)
        ln = np.zeros(m, dtype=np.float64)
        _chk(load_library().mpf_branch_lengths(self.h, root_taxon, int(n_sites), int(bool(unit_cost_parstree)), m, _p(a), _p(b), _p(ln),
                                               C.byref(n)))
        assert n.value == m
        return a, b, ln

    # ---- multifurcating trees (neighbour lists: trees.collapse_branches)
    @staticmethod
    def _lists(first, nbr):
        f = np.ascontiguousarray(first, dtype=np.int32)
        return f, np.ascontiguousarray(nbr, dtype=np.int32), len(f) - 1

    def polytomy_parsimony(self, first, nbr, root_taxon: int = 1, with_patterns: bool = False):
        """length of the tree given as CSR neighbour lists (tips 1 .. n, inner node i = node n + 1 + i with the neighbours
        nbr[first[i]:first[i + 1]]) by the reference's rules for nodes of any degree, evaluated at the leaf root_taxon's edge
        (computeParsimony()); with_patterns: (length, _pattern_pars[P]).  The engine's own tree is not touched."""
        f, nb, k = self._lists(first, nbr)
        s = C.c_uint32()
        pp = np.zeros(self.P, dtype=np.uint16) if with_patterns else None
        _chk(load_library().mpf_polytomy_parsimony(self.h, k, _p(f), _p(nb), root_taxon, C.byref(s), _p(pp) if with_patterns else None))
        return (int(s.value), pp) if with_patterns else int(s.value)

    def polytomy_branch_substitutions(self, first, nbr, root_taxon: int = 1):
        """branch_substitutions for such a tree: (node1[m], node2[m], subst[m]), m = n + n_inner - 1, the walk from root_taxon with
        the neighbours in list order; all directed views of the tree in one launch, all branches in another"""
        f, nb, k = self._lists(first, nbr)
        m = self.n + k - 1
        n = C.c_int32()
        a = np.zeros(max(m, 1), dtype=np.int32)
        b = np.zeros(max(m, 1), dtype=np.int32)
        s = np.zeros(max(m, 1), dtype=np.uint32)
        _chk(load_library().mpf_polytomy_branch_substitutions(self.h, k, _p(f), _p(nb), root_taxon, m, _p(a), _p(b), _p(s), C.byref(n)))
        assert n.value == m
        return a[:m], b[:m], s[:m]

    def polytomy_branch_lengths(self, first, nbr, n_sites: int, root_taxon: int = 1, unit_cost_parstree: bool = False):
        """branch_lengths for such a tree: (node1[m], node2[m], length[m] float64)"""
        f, nb, k = self._lists(first, nbr)
        m = self.n + k - 1
        n = C.c_int32()
        a = np.zeros(max(m, 1), dtype=np.int32)
        b = np.zeros(max(m, 1), dtype=np.int32)
        ln = np.zeros(max(m, 1), dtype=np.float64)
        _chk(load_library().mpf_polytomy_branch_lengths(self.h, k, _p(f), _p(nb), root_taxon, int(n_sites), int(bool(unit_cost_parstree)), m,
                                                        _p(a), _p(b), _p(ln), C.byref(n)))
        assert n.value == m
        return a[:m], b[:m], ln[:m]

    # ---- taxon insertion (host/place.cpp, place.hip): a binary backbone over a subset of the tips, as neighbour lists
    def insertion_costs(self, first, nbr, queries, root_taxon: int = 1, cap=None):
        """every insertion test of addTaxonMPFast: (node1[m], node2[m], cost[Q][m], tree_length) -- cost[q][i] = the length of the
        backbone (first, nbr: the lists of polytomy_branch_substitutions with tips allowed to be absent, every inner degree 3) with
        taxon queries[q] attached to branch i = (node1[i], node2[i]), branches in the walk order from root_taxon, m = 2 tips - 3.
        cap (tests): the room handed to the C call; below m nothing is filled and only (m, tree_length) comes back.

        A weighted engine (cost=...) serves this, place_taxa and iq_parsimony_tree after set_option("place_weighted", 1) only
        (default 0: MpfError -6, as before): cost[q][i] is then the FULL weighted length of the completed tree evaluated at the new
        taxon's edge (what mpf_compute_parsimony_at gives for that tree at root_taxon = queries[q]); tree_length is the backbone's
        own length at root_taxon, and iq_parsimony_tree's lengths[j] for j >= 1 are the scores at the edge of the taxon just added."""
        f, nb, k = self._lists(first, nbr)
        q = np.ascontiguousarray(queries, dtype=np.int32).reshape(-1)
        m = 2 * k + 1 if cap is None else int(cap)
        n = C.c_int32()
        ln = C.c_uint32()
        a = np.zeros(max(m, 1), dtype=np.int32)
        b = np.zeros(max(m, 1), dtype=np.int32)
        c = np.zeros((max(len(q), 1), max(m, 1)), dtype=np.uint32)
        _chk(load_library().mpf_insertion_costs(self.h, k, _p(f), _p(nb), root_taxon, len(q), _p(q) if len(q) else None, m, _p(a), _p(b),
                                                _p(c), C.byref(n), C.byref(ln)))
        if n.value > m:
            return int(n.value), int(ln.value)
        return a[:n.value], b[:n.value], c[:len(q), :n.value], int(ln.value)

    def place_taxa(self, first, nbr, queries, root_taxon: int = 1):
        """addTaxonMPFast's answer for every query taxon: (branch[Q], node1[Q], node2[Q], length[Q], tree_length) -- the first branch
        of the walk from root_taxon with the smallest length (found on the device: the Q x m matrix is not copied back).

        IQTree::reinsertLeavesByParsimony, leaves deleted from the record tree `back` put back one by one at their best branch:

            first, nbr = trees.drop_tips(back, n, leaves)
            for t in leaves:
                _, a, b, _, _ = eng.place_taxa(first, nbr, [t])
                first, nbr = trees.insert_tip(first, nbr, n, t, int(a[0]), int(b[0]))
            back = trees.lists_to_back(first, nbr, n)
        """
        f, nb, k = self._lists(first, nbr)
        q = np.ascontiguousarray(queries, dtype=np.int32).reshape(-1)
        Q = len(q)
        br = np.zeros(max(Q, 1), dtype=np.int32)
        a = np.zeros(max(Q, 1), dtype=np.int32)
        b = np.zeros(max(Q, 1), dtype=np.int32)
        ln = np.zeros(max(Q, 1), dtype=np.uint32)
        tl = C.c_uint32()
        _chk(load_library().mpf_place_taxa(self.h, k, _p(f), _p(nb), root_taxon, Q, _p(q) if Q else None, _p(br), _p(a), _p(b), _p(ln),
                                           C.byref(tl)))
        return br[:Q], a[:Q], b[:Q], ln[:Q], int(tl.value)

    # ---- TBR (host/tbr.cpp, tbr.hip): no reference function, MPBoot has SPR and NNI only.  An engine without a tracker; a weighted
    # engine (cost=...) after set_option("tbr_weighted", 1) only, and only with a symmetric cost matrix
    def tbr_scan(self, rec: int, maxtrav: int = 6, cap=None):
        """one visit: (f_recs, g_recs, cost[1 + len(f), 1 + len(g)]) -- cut the edge (rec, back[rec]); g_recs lists the branches of
        rec's part, f_recs those of back[rec]'s part (the SPR scan's one side with mintrav = 1); cost[i][j] = the length of the tree
        that joins the middle of f_recs[i - 1] to the middle of g_recs[j - 1], index 0 = the part's own root: row 0 and column 0
        are SPR tests, cost[0][0] is the current length.  The tree of an entry is trees.apply_tbr(back, rec, f, g).
        A weighted engine (cost=...) serves this, tbr_sweep_best, apply_tbr and optimize_tbr after set_option("tbr_weighted", 1) only
        (default 0: MpfError -6 as before): an entry is then the FULL weighted length of the joined tree, in either store
        ("sankoff_short"); a cost matrix that is not symmetric is refused (-6, "not symmetric": the length would depend on the edge it
        is evaluated at).
        cap (tests): (cap_f, cap_g) handed to the C call; where one is too small only (n_f, n_g) comes back."""
        L = load_library()
        nf, ng = C.c_int32(), C.c_int32()
        if cap is None:
            _chk(L.mpf_tbr_scan(self.h, rec, maxtrav, -1, -1, None, None, None, C.byref(nf), C.byref(ng)))
            cap = (nf.value, ng.value)
        f = np.zeros(max(cap[0], 1), dtype=np.int32)
        g = np.zeros(max(cap[1], 1), dtype=np.int32)
        c = np.zeros((1 + max(cap[0], 0)) * (1 + max(cap[1], 0)), dtype=np.uint32)
        _chk(L.mpf_tbr_scan(self.h, rec, maxtrav, cap[0], cap[1], _p(f), _p(g), _p(c), C.byref(nf), C.byref(ng)))
        if nf.value > cap[0] or ng.value > cap[1]:
            return nf.value, ng.value
        return f[:nf.value].copy(), g[:ng.value].copy(), c[:(1 + nf.value) * (1 + ng.value)].reshape(1 + nf.value, 1 + ng.value).copy()

    def tbr_sweep_best(self, maxtrav: int = 6):
        """the best of every visit of a sweep over node_order(): (cost[2n - 2], f[2n - 2], g[2n - 2], n_pairs) -- the first minimum
        of each visit's matrix in row-major order, [0][0] left out; records -1 for "none"; cost 0xFFFFFFFF where a visit has no
        entry; n_pairs = matrix entries scored.  Found on the device: three words per visit come back."""
        m = 2 * self.n - 2
        c = np.zeros(m, dtype=np.uint32)
        f = np.zeros(m, dtype=np.int32)
        g = np.zeros(m, dtype=np.int32)
        k = C.c_uint64()
        _chk(load_library().mpf_tbr_sweep_best(self.h, maxtrav, _p(c), _p(f), _p(g), C.byref(k)))
        return c, f, g, int(k.value)

    def apply_tbr(self, rec: int, f_rec: int, g_rec: int) -> int:
        """edit the engine's tree to trees.apply_tbr(back, rec, f_rec, g_rec) -> its length (as set_tree + score_tree)"""
        s = C.c_uint32()
        _chk(load_library().mpf_apply_tbr(self.h, rec, f_rec, g_rec, C.byref(s)))
        return s.value

    def optimize_tbr(self, maxtrav: int = 6, max_moves: int = 0):
        """steepest descent over the TBR neighbourhood: the sweep's best is applied while it is strictly below the current length.
        -> (length, n_moves); the moves are in tbr_moves().  Deterministic, the tie stream is not touched."""
        s, k = C.c_uint32(), C.c_int32()
        _chk(load_library().mpf_optimize_tbr(self.h, maxtrav, max_moves, C.byref(s), C.byref(k)))
        return s.value, k.value

    def tbr_moves(self):
        """moves of the last optimize_tbr: (rec[k], f_rec[k], g_rec[k], length[k])"""
        L = load_library()
        k = C.c_int32()
        _chk(L.mpf_get_tbr_moves(self.h, 0, None, None, None, None, C.byref(k)))
        r, f, g = (np.zeros(k.value, dtype=np.int32) for _ in range(3))
        s = np.zeros(k.value, dtype=np.uint32)
        if k.value:
            _chk(L.mpf_get_tbr_moves(self.h, k.value, _p(r), _p(f), _p(g), _p(s), C.byref(k)))
        return r, f, g, s

    # ---- ... under -bb (a tracker attached): every entry of every visit's matrix goes to saveCurrentTree's rule -- the visits in
    # node_order(), a visit's entries in row-major order from [0][0] (the current tree under its own length), every other entry the
    # joined tree under cost[i][j].  Default rule, -mulhits, a cut-off, -cutoff_from_btrees; the rest is refused (-6)
    # A weighted engine (cost=...) serves both after set_option("tbr_weighted", 1) and set_option("tbr_weighted_tracked", 1) only
    def ufboot_tbr_sweep(self, maxtrav: int = 6):
        """tbr_sweep_best with every entry booked through the tracker -> (cost, f, g, n_pairs); the tree does not change.
        get_option("tbr_booked") counts the trees handed over since the attach; set_option("tbr_book_rows", k) caps the entries of
        a booking batch (books and draws do not depend on it)."""
        m = 2 * self.n - 2
        c = np.zeros(m, dtype=np.uint32)
        f = np.zeros(m, dtype=np.int32)
        g = np.zeros(m, dtype=np.int32)
        k = C.c_uint64()
        _chk(load_library().mpf_ufboot_tbr_sweep(self.h, maxtrav, _p(c), _p(f), _p(g), C.byref(k)))
        return c, f, g, int(k.value)

    def ufboot_optimize_tbr(self, maxtrav: int = 6, max_moves: int = 0):
        """optimize_tbr with every sweep booked through the tracker, the last one, which finds nothing, included
        -> (length, n_moves); the moves are in tbr_moves().  The climb itself draws nothing."""
        s, k = C.c_uint32(), C.c_int32()
        _chk(load_library().mpf_ufboot_optimize_tbr(self.h, maxtrav, max_moves, C.byref(s), C.byref(k)))
        return s.value, k.value

    def tbr_pattern_terms(self, rec: int, maxtrav: int = 6, cap=None):
        """DIAGNOSTIC: the mask rows of one visit as the tracked sweep's kernel writes them -> (n_f, n_g,
        terms[1 + n_f][1 + n_g][n_patterns] uint8); per pattern, length of the tree of entry [i][j] = length of the current tree -
        terms[0][0] + terms[i][j].  cap (tests): cap_entries handed to the C call; too small, only (n_f, n_g) comes back."""
        L = load_library()
        nf, ng = C.c_int32(), C.c_int32()
        if cap is None:
            _chk(L.mpf_tbr_pattern_terms(self.h, rec, maxtrav, 0, None, C.byref(nf), C.byref(ng)))
            cap = (1 + nf.value) * (1 + ng.value)
        t = np.zeros(max(cap, 1) * self.P, dtype=np.uint8)
        _chk(L.mpf_tbr_pattern_terms(self.h, rec, maxtrav, cap, _p(t), C.byref(nf), C.byref(ng)))
        k = (1 + nf.value) * (1 + ng.value)
        if k > cap:
            return nf.value, ng.value
        return nf.value, ng.value, t[:k * self.P].reshape(1 + nf.value, 1 + ng.value, self.P).copy()

    def tbr_pattern_lengths(self, rec: int, maxtrav: int = 6, cap=None):
        """DIAGNOSTIC, weighted engines after set_option("tbr_weighted", 1) and set_option("tbr_weighted_tracked", 1) (refused on a
        Fitch engine): the rows of one visit as the weighted tracked sweep's kernel writes them -> (n_f, n_g,
        rows[1 + n_f][1 + n_g][n_patterns] uint16): per pattern the length of the tree of entry [i][j], 0 for a pattern the engine
        drops; a row's weighted sum is the entry's cost.  cap (tests): cap_entries handed to the C call; too small, only (n_f, n_g)
        comes back."""
        L = load_library()
        nf, ng = C.c_int32(), C.c_int32()
        if cap is None:
            _chk(L.mpf_tbr_pattern_lengths(self.h, rec, maxtrav, 0, None, C.byref(nf), C.byref(ng)))
            cap = (1 + nf.value) * (1 + ng.value)
        t = np.zeros(max(cap, 1) * self.P, dtype=np.uint16)
        _chk(L.mpf_tbr_pattern_lengths(self.h, rec, maxtrav, cap, _p(t), C.byref(nf), C.byref(ng)))
        k = (1 + nf.value) * (1 + ng.value)
        if k > cap:
            return nf.value, ng.value
        return nf.value, ng.value, t[:k * self.P].reshape(1 + nf.value, 1 + ng.value, self.P).copy()

    def iq_parsimony_tree(self, order=None, tie_state=None):
        """PhyloTree::computeParsimonyTree (-starttree PARS): stepwise addition with every branch tried at every step and the first
        minimum taken -> (first, nbr, lengths[n - 2], order[n], tie_state).  order (1-based permutation) is taken as given; with
        tie_state instead it is drawn by my_random_shuffle from that state of the host's random_double() stream (n - 1 draws), and the
        state behind them comes back.  lengths[j] = the length of the tree of the first j + 3 taxa.  The engine's own tree stays:
        set_tree(trees.lists_to_back(first, nbr, n)) to climb from the result."""
        n = self.n
        if (order is None) == (tie_state is None):
            raise ValueError("iq_parsimony_tree: give either order or tie_state")
        o = np.zeros(n, dtype=np.int32) if order is None else np.ascontiguousarray(order, dtype=np.int32).copy()
        if len(o) != n:
            raise ValueError("iq_parsimony_tree: order must list all taxa")
        st = None if tie_state is None else C.c_uint64(int(tie_state) & ((1 << 64) - 1))
        f = np.zeros(n - 1, dtype=np.int32)
        nb = np.zeros(3 * (n - 2), dtype=np.int32)
        ln = np.zeros(max(n - 2, 1), dtype=np.uint32)
        sc = C.c_uint32()
        _chk(load_library().mpf_iq_parsimony_tree(self.h, None if st is None else C.byref(st), _p(o), _p(f), _p(nb), _p(ln), C.byref(sc)))
        assert int(sc.value) == int(ln[-1])
        return f, nb, ln, o, (None if st is None else int(st.value))

    # ---- the summary of a -bb run: split counts, supports on a tree, consensus tree (host/splits.cpp, splits.hip)
    def _tree_set(self, backs, weights):
        b = np.ascontiguousarray(backs, dtype=np.int32).reshape(-1, 3 * (2 * self.n - 1))
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.int32)
        assert w is None or len(w) == len(b)
        return b, w

    def _mixed_set(self, backs, lists, weights=None):
        """(TreeSet, its number of trees, weights or None, the arrays it points into) of record-format trees `backs` (may be None or
        empty) followed by the list-form trees lists = [(first, nbr), ...]"""
        keep = []
        s = TreeSet()
        T = 0
        if backs is not None and len(backs):
            b = np.ascontiguousarray(backs, dtype=np.int32).reshape(-1, 3 * (2 * self.n - 1))
            keep.append(b)
            s.n_records, s.backs, T = len(b), b.ctypes.data, len(b)
        if lists is not None and len(lists):
            fs = [np.ascontiguousarray(f, dtype=np.int32).reshape(-1) for f, _ in lists]
            ns = [np.ascontiguousarray(x, dtype=np.int32).reshape(-1) for _, x in lists]
            ni = np.array([len(f) - 1 for f in fs], dtype=np.int32)
            first = np.ascontiguousarray(np.concatenate(fs), dtype=np.int32)
            nbr = np.ascontiguousarray(np.concatenate(ns + [np.zeros(1, dtype=np.int32)]), dtype=np.int32)
            keep += [ni, first, nbr]
            s.n_lists, s.n_inner, s.first, s.nbr = len(lists), ni.ctypes.data, first.ctypes.data, nbr.ctypes.data
            T += len(lists)
        w = None if weights is None else np.ascontiguousarray(weights, dtype=np.int32)
        assert w is None or len(w) == T
        return s, T, w, keep

    def split_counts(self, backs, weights=None, counts_only: bool = False, *, lists=None):
        """The distinct non-trivial splits of the trees backs[T][3 (2n - 1)] with the summed weights of the trees that hold them
        (weights int32 >= 0, None = all 1): (bits[D][ceil(n / 32)] uint32, count[D] int64, total_weight), ordered by count
        descending, then by the words ascending.  Bit (t - 1) % 32 of word (t - 1) / 32 = tip t is on the side without tip 1.
        counts_only: (D, total_weight).  Exact: counted on the device, sets compared as whole sets.
        lists=[(first, nbr), ...]: trees given as neighbour lists (any inner degree >= 3; trees.collapse_branches, consensus_tree)
        behind the record-format ones, which may then be None; weights run over the records, then the lists."""
        nd, tot = C.c_int32(), C.c_int64()
        L = load_library()
        if lists is not None:
            ts, _, w, _keep = self._mixed_set(backs, lists, weights)
            wp = None if w is None else _p(w)
            _chk(L.mpf_split_counts_set(self.h, C.byref(ts), wp, 0, None, None, C.byref(nd), C.byref(tot)))
            if counts_only:
                return int(nd.value), int(tot.value)
            D, words = int(nd.value), (self.n + 31) // 32
            bits = np.zeros((max(D, 1), words), dtype=np.uint32)
            cnt = np.zeros(max(D, 1), dtype=np.int64)
            _chk(L.mpf_split_counts_set(self.h, C.byref(ts), wp, D, _p(bits), _p(cnt), C.byref(nd), C.byref(tot)))
            assert nd.value == D
            return bits[:D], cnt[:D], int(tot.value)
        b, w = self._tree_set(backs, weights)
        _chk(L.mpf_split_counts(self.h, len(b), _p(b), None if w is None else _p(w), 0, None, None, C.byref(nd), C.byref(tot)))
        if counts_only:
            return int(nd.value), int(tot.value)
        D, words = int(nd.value), (self.n + 31) // 32
        bits = np.zeros((max(D, 1), words), dtype=np.uint32)
        cnt = np.zeros(max(D, 1), dtype=np.int64)
        _chk(L.mpf_split_counts(self.h, len(b), _p(b), None if w is None else _p(w), D, _p(bits), _p(cnt), C.byref(nd), C.byref(tot)))
        assert nd.value == D
        return bits[:D], cnt[:D], int(tot.value)

    def split_support(self, backs, target=None, weights=None, *, lists=None, target_lists=None):
        """(node1[m], node2[m], support[m] int64, total_weight) for the m = 2 n - 3 branches of `target` in the order of
        branch_substitutions(root_taxon=1): the summed weight of the trees that hold the branch's split, -1 on a leaf branch.
        target_lists=(first, nbr) instead of target: the target is given as neighbour lists, m = n + n_inner - 1 branches in the
        order of polytomy_branch_substitutions(root_taxon=1), -1 also on the branch at tip 1; lists= as in split_counts."""
        if target is None and target_lists is None:
            raise ValueError("target or target_lists is needed")
        if target_lists is not None or lists is not None:
            if target_lists is None:
                from . import trees
                target_lists = trees.back_to_lists(target, self.n)
            elif target is not None:
                raise ValueError("target or target_lists, not both")
            ts, _, w, _keep = self._mixed_set(backs, lists, weights)
            f, nb, k = self._lists(*target_lists)
            m = self.n + k - 1
            n, tot = C.c_int32(), C.c_int64()
            a, c, s = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int64)
            _chk(load_library().mpf_split_support_set(self.h, C.byref(ts), None if w is None else _p(w), k, _p(f), _p(nb), m, _p(a), _p(c), _p(s),
                                                      C.byref(n), C.byref(tot)))
            assert n.value == m
            return a, c, s, int(tot.value)
        b, w = self._tree_set(backs, weights)
        t = np.ascontiguousarray(target, dtype=np.int32)
        m = 2 * self.n - 3
        n, tot = C.c_int32(), C.c_int64()
        a, c, s = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int64)
        _chk(load_library().mpf_split_support(self.h, len(b), _p(b), None if w is None else _p(w), _p(t), m, _p(a), _p(c), _p(s), C.byref(n),
                                              C.byref(tot)))
        assert n.value == m
        return a, c, s, int(tot.value)

    def consensus_tree(self, backs, weights=None, threshold: float = 0.0, *, lists=None):
        """The reference's consensus of the weighted trees: splits with count <= threshold * total dropped, then the greedy maximal
        compatible set (threshold 0: the greedy consensus of .contree; >= 0.5: majority rule).  -> (first, nbr, support_of_inner,
        total_weight): the neighbour lists polytomy_parsimony / polytomy_branch_lengths take, inner nodes in pre-order from tip 1,
        support_of_inner[i] = the count of the split above inner node n + 1 + i (-1 for the first).  lists= as in split_counts."""
        n = self.n
        ni, tot = C.c_int32(), C.c_int64()
        first, nbr, sup = np.zeros(n - 1, dtype=np.int32), np.zeros(3 * n - 6, dtype=np.int32), np.zeros(n - 2, dtype=np.int64)
        if lists is not None:
            ts, _, w, _keep = self._mixed_set(backs, lists, weights)
            _chk(load_library().mpf_consensus_tree_set(self.h, C.byref(ts), None if w is None else _p(w), float(threshold), C.byref(ni),
                                                       _p(first), _p(nbr), _p(sup), C.byref(tot)))
            k = int(ni.value)
            return first[:k + 1].copy(), nbr[:int(first[k])].copy(), sup[:k].copy(), int(tot.value)
        b, w = self._tree_set(backs, weights)
        _chk(load_library().mpf_consensus_tree(self.h, len(b), _p(b), None if w is None else _p(w), float(threshold), C.byref(ni), _p(first),
                                               _p(nbr), _p(sup), C.byref(tot)))
        k = int(ni.value)
        return first[:k + 1].copy(), nbr[:int(first[k])].copy(), sup[:k].copy(), int(tot.value)

    def ufboot_summary_trees(self, rule: int = SUMMARY_AUTO):
        """(tree_index[T] int64, weights[T] int32, backs[T][3 (2n - 1)]): the weighted tree set IQTree::summarizeBootstrap makes of the
        attached tracker under `rule` (SUMMARY_*)"""
        L = load_library()
        n = C.c_int32()
        _chk(L.mpf_ufboot_summary_trees(self.h, rule, 0, None, None, None, C.byref(n)))
        T = int(n.value)
        idx, w = np.zeros(T, dtype=np.int64), np.zeros(T, dtype=np.int32)
        b = np.zeros((T, 3 * (2 * self.n - 1)), dtype=np.int32)
        _chk(L.mpf_ufboot_summary_trees(self.h, rule, T, _p(idx), _p(w), _p(b), C.byref(n)))
        return idx, w, b

    def ufboot_summarize(self, target=None, threshold: float = 0.0, rule: int = SUMMARY_AUTO):
        """split_counts, split_support (if a target tree is given) and consensus_tree of the attached tracker's trees, weighted as
        the reference weights them (rule: SUMMARY_AUTO = by the tracker's own options, SUMMARY_DEFAULT, SUMMARY_MULHITS,
        SUMMARY_TOPBOOT) -> dict"""
        L = load_library()
        n, words = self.n, (self.n + 31) // 32
        s = BbSummary()
        s.threshold = float(threshold)
        _chk(L.mpf_ufboot_summarize(self.h, rule, C.byref(s)))          # sizes first
        D = int(s.n_distinct)
        bits, cnt = np.zeros((max(D, 1), words), dtype=np.uint32), np.zeros(max(D, 1), dtype=np.int64)
        m = 2 * n - 3
        a, c, sup = np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int32), np.zeros(m, dtype=np.int64)
        first, nbr, isup = np.zeros(n - 1, dtype=np.int32), np.zeros(3 * n - 6, dtype=np.int32), np.zeros(n - 2, dtype=np.int64)
        t = None if target is None else np.ascontiguousarray(target, dtype=np.int32)
        s.split_cap, s.bits, s.count = D, bits.ctypes.data, cnt.ctypes.data
        if t is not None:
            s.target_back, s.branch_cap, s.node1, s.node2, s.support = t.ctypes.data, m, a.ctypes.data, c.ctypes.data, sup.ctypes.data
        s.first, s.nbr, s.support_of_inner = first.ctypes.data, nbr.ctypes.data, isup.ctypes.data
        _chk(L.mpf_ufboot_summarize(self.h, rule, C.byref(s)))
        assert s.n_distinct == D
        k = int(s.n_inner)
        out = {"bits": bits[:D], "count": cnt[:D], "total_weight": int(s.total_weight), "n_trees": int(s.n_trees),
               "first": first[:k + 1].copy(), "nbr": nbr[:int(first[k])].copy(), "support_of_inner": isup[:k].copy()}
        if t is not None:
            out.update(node1=a, node2=c, support=sup)
        return out

    def rf_distances(self, backs, backs2=None, mode: str = "all", *, lists=None, lists2=None):
        """Robinson-Foulds distances between trees (MTreeSet::computeRFDist; -rf_all, -rf_adj, -rf of the reference): the number of
        non-trivial splits in one tree and not in the other, int32.  backs[T][3 (2n - 1)] alone: mode "all" -> [T][T] (symmetric,
        diagonal 0), mode "adjacent" -> [T - 1], d(tree i, tree i + 1).  With backs2[T2][...]: [T][T2], tree i of backs against
        tree j of backs2.  Exact: one split pass over all the trees on the device, then a binary matrix product.
        lists=[(first, nbr), ...] / lists2=: trees given as neighbour lists behind the record-format trees of the first / second set
        (either part of a set may be None); the distance is then c_i + c_j - 2 shared for trees with c_i and c_j splits."""
        if mode not in ("all", "adjacent"):
            raise ValueError("mode: 'all' or 'adjacent'")
        if lists is not None or lists2 is not None:
            s1, T, _, _k1 = self._mixed_set(backs, lists)
            if backs2 is not None or lists2 is not None:
                if mode != "all":
                    raise ValueError("two sets: every tree of the first against every tree of the second (mode 'all')")
                s2, T2, _, _k2 = self._mixed_set(backs2, lists2)
                out = np.zeros((T, T2), dtype=np.int32)
                _chk(load_library().mpf_rf_distances_set(self.h, RF_TWO_SETS, C.byref(s1), C.byref(s2), out.size, _p(out)))
                return out
            out = np.zeros((T, T) if mode == "all" else (max(T - 1, 0),), dtype=np.int32)
            _chk(load_library().mpf_rf_distances_set(self.h, RF_ALL_PAIRS if mode == "all" else RF_ADJACENT, C.byref(s1), None, out.size,
                                                     _p(out) if out.size else None))
            return out
        b, _ = self._tree_set(backs, None)
        T = len(b)
        if backs2 is not None:
            if mode != "all":
                raise ValueError("two sets: every tree of the first against every tree of the second (mode 'all')")
            b2, _ = self._tree_set(backs2, None)
            out = np.zeros((T, len(b2)), dtype=np.int32)
            _chk(load_library().mpf_rf_distances(self.h, RF_TWO_SETS, T, _p(b), len(b2), _p(b2), out.size, _p(out)))
            return out
        out = np.zeros((T, T) if mode == "all" else (max(T - 1, 0),), dtype=np.int32)
        _chk(load_library().mpf_rf_distances(self.h, RF_ALL_PAIRS if mode == "all" else RF_ADJACENT, T, _p(b), 0, None, out.size,
                                             _p(out) if out.size else None))
        return out

    def nni_pattern_terms(self, root_taxon: int = 1):
        """nni_scores by the mask-writing kernel of the tracked climb: (node1[m], node2[m], len[m][2], terms[m][3][n_patterns]);
        per pattern, length after move k of branch i = length of the current tree - terms[i][0] + terms[i][1 + k]"""
        L = load_library()
        n = C.c_int32()
        _chk(L.mpf_nni_pattern_terms(self.h, root_taxon, 0, None, None, None, None, C.byref(n)))
        m = n.value
        a = np.zeros(max(m, 1), dtype=np.int32)
        b = np.zeros(max(m, 1), dtype=np.int32)
        ln = np.zeros(2 * max(m, 1), dtype=np.uint32)
        t = np.zeros(3 * max(m, 1) * self.P, dtype=np.uint8)
        _chk(L.mpf_nni_pattern_terms(self.h, root_taxon, m, _p(a), _p(b), _p(ln), _p(t), C.byref(n)))
        return a[:m].copy(), b[:m].copy(), ln[:2 * m].reshape(m, 2).copy(), t[:3 * m * self.P].reshape(m, 3, self.P).copy()

    def nni_pattern_lengths(self, root_taxon: int = 1):
        """nni_scores by the row-writing kernel of the tracked weighted climb (set_option("nni_weighted", 1) and
        set_option("nni_weighted_tracked", 1); refused on a Fitch engine): (node1[m], node2[m], len[m][2],
        rows[1 + 2 m][n_patterns] uint16) -- row 0 the current tree's per-pattern lengths at root_taxon's edge, row 1 + 2 i + k those
        of the tree after move k of branch i, rooted at that branch with node2's side the parent"""
        L = load_library()
        n = C.c_int32()
        _chk(L.mpf_nni_pattern_lengths(self.h, root_taxon, -1, None, None, None, None, C.byref(n)))
        m = n.value
        a = np.zeros(max(m, 1), dtype=np.int32)
        b = np.zeros(max(m, 1), dtype=np.int32)
        ln = np.zeros(2 * max(m, 1), dtype=np.uint32)
        r = np.zeros((1 + 2 * m) * self.P, dtype=np.uint16)
        _chk(L.mpf_nni_pattern_lengths(self.h, root_taxon, m, _p(a), _p(b), _p(ln), _p(r), C.byref(n)))
        return a[:m].copy(), b[:m].copy(), ln[:2 * m].reshape(m, 2).copy(), r.reshape(1 + 2 * m, self.P)

    def nni_moves(self):
        """the swaps of the last optimize_nni, reverts included: int32[k][4] rows (node1, slot1, node2, slot2)"""
        L = load_library()
        k = C.c_int32()
        _chk(L.mpf_get_nni_moves(self.h, 0, None, None, None, None, C.byref(k)))
        cols = [np.zeros(max(k.value, 1), dtype=np.int32) for _ in range(4)]
        if k.value:
            _chk(L.mpf_get_nni_moves(self.h, k.value, *[_p(c) for c in cols], C.byref(k)))
        return np.stack([c[:k.value] for c in cols], axis=1) if k.value else np.zeros((0, 4), dtype=np.int32)

    # ---- online UFBoot-MP bookkeeping (IQTree::saveCurrentTree during optimize_spr)
    def ufboot_attach(self, samples, epsilon: float = 0.5, shard=None, exchange=None, sample_ids=None):
        """samples: [n_samples][n_patterns] bootstrap weights (all of them, on every rank).
        shard = (rank, world): multi-GPU online phase -- this engine keeps samples rank, rank + world, ... (or `sample_ids`, any
        other split the ranks agree on) and `exchange` (default: mpboot_amd.shard.event_exchange(), an all-gather over
        torch.distributed) merges the per-batch events of all ranks; every rank must then make the same optimize_spr /
        ufboot_optimize_nni calls (the latter on a sharded tracker: set_option("nni_tracked_rules", 1))."""
        samples = np.ascontiguousarray(samples, dtype=np.uint16)
        if samples.ndim != 2 or samples.shape[1] != self.P:
            raise ValueError("samples must be [n_samples][n_patterns]")
        self.ufb_B = samples.shape[0]
        if shard is None or shard[1] == 1:
            _chk(load_library().mpf_ufboot_attach(self.h, self.ufb_B, _p(samples), float(epsilon)))
            self._drop_exchange()
            return
        rank, world = shard
        ids = np.arange(rank, self.ufb_B, world, dtype=np.int32) if sample_ids is None else np.ascontiguousarray(sample_ids, dtype=np.int32)
        local = np.ascontiguousarray(samples[ids])
        if exchange is None:
            from . import shard as _shard
            exchange = _shard.event_exchange()
        self._drop_exchange()
        if isinstance(exchange, RcclComm):       # the library's own exchange: mpf_rccl_exchange with the communicator as its argument
            fn = C.cast(load_library().mpf_rccl_exchange, C.c_void_p)
            _chk(load_library().mpf_ufboot_attach_sharded(self.h, self.ufb_B, len(ids), _p(ids), _p(local), float(epsilon), fn, exchange.h))
            self._ufb_exchange = exchange
            exchange._users += 1                 # (RcclComm.close() refuses while a tracker holds the raw handle)
            return
        self._ufb_exchange = exchange            # keep the ctypes callback alive as long as the tracker
        _chk(load_library().mpf_ufboot_attach_sharded(self.h, self.ufb_B, len(ids), _p(ids), _p(local), float(epsilon),
                                                      C.cast(exchange, C.c_void_p), None))

    def ufboot_optimize_nni(self, root_taxon: int = 1, speednni: bool = True, max_steps: int = 50):
        """optimize_nni under -bb: the attached tracker books the current tree of every scoring step and both NNIs of every
        evaluated branch (mpf_ufboot_optimize_nni) -> (length, nni_count, nni_steps).  A weighted engine serves it after
        set_option("nni_weighted", 1) and set_option("nni_weighted_tracked", 1) (defaults 0: MpfError -6): every booked tree with
        its own row of per-pattern lengths -- a candidate's at its branch, the current tree's at the leaf root_taxon.
        With -storetrees, -mulhits -topboot or -distinct_iter_top_boot in force, or on a sample-sharded tracker, it is served after
        set_option("nni_tracked_rules", 1) (default 0: MpfError -6); ufboot_set_iteration keeps the iteration number in step"""
        s, cnt, steps = C.c_uint32(), C.c_int32(), C.c_int32()
        _chk(load_library().mpf_ufboot_optimize_nni(self.h, root_taxon, int(bool(speednni)), max_steps, C.byref(s), C.byref(cnt),
                                                    C.byref(steps)))
        return s.value, cnt.value, steps.value

    def ufboot_refine_sweep(self, maxtrav: int, tie_seeds=None):
        """Batched bootstrap refinement (mpf_ufboot_refine_sweep): the first sweep of the SPR climb from the CURRENT tree under
        every attached sample's weights at once -> (scores[B], stable[B] bool, first_move_visit[B])."""
        B = self.ufb_B
        seeds = None if tie_seeds is None else np.ascontiguousarray(tie_seeds, dtype=np.int32)
        if seeds is not None and len(seeds) != B:
            raise ValueError("one tie seed per attached sample")
        scores = np.zeros(B, dtype=np.uint32)
        stable = np.zeros(B, dtype=np.uint8)
        first = np.zeros(B, dtype=np.int32)
        _chk(load_library().mpf_ufboot_refine_sweep(self.h, maxtrav, None if seeds is None else _p(seeds), _p(scores), _p(stable), _p(first)))
        return scores, stable.astype(bool), first

    def ufboot_detach(self):
        _chk(load_library().mpf_ufboot_detach(self.h))
        self._drop_exchange()

    def ufboot_set_cutoff(self, logl_cutoff: float):
        _chk(load_library().mpf_ufboot_set_cutoff(self.h, float(logl_cutoff)))

    def ufboot_set_ratchet_booking(self, on: bool):
        """False = mpboot's -no_hclimb1_bb: climbs under other weights than the attach-time ones are not booked"""
        _chk(load_library().mpf_ufboot_set_ratchet_booking(self.h, 1 if on else 0))

    def ufboot_set_store_trees(self, on: bool):
        """params->store_candidate_trees (-storetrees, iqtree.cpp:3302-3346); right after the attach"""
        _chk(load_library().mpf_ufboot_set_store_trees(self.h, 1 if on else 0))

    def ufboot_duplicates(self) -> int:
        """duplication_counter: trees that reached saveCurrentTree with a topology booked before (-storetrees)"""
        n = C.c_uint64()
        _chk(load_library().mpf_ufboot_get_duplicates(self.h, C.byref(n)))
        return int(n.value)

    def ufboot_set_mulhits(self, on: bool):
        """params->multiple_hits: the -mulhits update rule (iqtree.cpp:3498-3540); right after the attach"""
        _chk(load_library().mpf_ufboot_set_mulhits(self.h, 1 if on else 0))

    def ufboot_set_topboot(self, n_top: int):
        """params->store_top_boot_trees (-topboot N, with -mulhits; iqtree.cpp:3542-3585)"""
        self.ufb_topboot = int(n_top)
        _chk(load_library().mpf_ufboot_set_topboot(self.h, int(n_top)))

    def ufboot_set_distinct_iter(self, k: int):
        """params->distinct_iter_top_boot (iqtree.cpp:3587-3680); without -mulhits"""
        self.ufb_topboot = int(k)
        _chk(load_library().mpf_ufboot_set_distinct_iter(self.h, int(k)))

    def ufboot_set_iteration(self, cur_it: int):
        _chk(load_library().mpf_ufboot_set_iteration(self.h, int(cur_it)))

    def ufboot_sample_iters(self, sample: int):
        cap = max(int(getattr(self, "ufb_topboot", 0)), 1)
        it = np.zeros(cap, dtype=np.int32)
        n = C.c_int32(0)
        _chk(load_library().mpf_ufboot_get_sample_iters(self.h, int(sample), _p(it), cap, C.byref(n)))
        return [int(x) for x in it[:n.value]]

    def ufboot_sample_top(self, sample: int):
        """([(tree index, rell)...] best first, boot_threshold) of one sample under -mulhits -topboot"""
        cap = max(int(getattr(self, "ufb_topboot", 0)), 1)
        trees = np.zeros(cap, dtype=np.int64)
        rell = np.zeros(cap, dtype=np.int32)
        n, thr = C.c_int32(0), C.c_int32(0)
        _chk(load_library().mpf_ufboot_get_sample_top(self.h, int(sample), _p(trees), _p(rell), cap, C.byref(n), C.byref(thr)))
        return [(int(trees[i]), int(rell[i])) for i in range(n.value)], int(thr.value)

    def ufboot_sample_trees(self, sample: int):
        """boot_trees_parsimony[sample] under -mulhits, sorted"""
        L = load_library()
        n = C.c_int32(0)
        _chk(L.mpf_ufboot_get_sample_trees(self.h, int(sample), None, 0, C.byref(n)))
        out = np.zeros(max(n.value, 1), dtype=np.int64)
        _chk(L.mpf_ufboot_get_sample_trees(self.h, int(sample), _p(out), n.value, C.byref(n)))
        return [int(x) for x in out[:n.value]]

    def ufboot_set_cutoff_from_btrees(self, on: bool):
        """-cutoff_from_btrees: ufboot_next_cutoff = min over the samples of the logl their tree was booked under"""
        _chk(load_library().mpf_ufboot_set_cutoff_from_btrees(self.h, 1 if on else 0))

    def ufboot_orig_logl(self):
        """boot_tree_orig_logl [n_samples]"""
        out = np.zeros(self.ufb_B, dtype=np.int32)
        _chk(load_library().mpf_ufboot_get_orig_logl(self.h, _p(out)))
        return out

    def ufboot_next_cutoff(self, percent: int = 10) -> float:
        c = C.c_double()
        _chk(load_library().mpf_ufboot_next_cutoff(self.h, percent, C.byref(c)))
        return c.value

    def ufboot_tree_logl(self):
        k = C.c_int64()
        L = load_library()
        _chk(L.mpf_ufboot_num_trees(self.h, C.byref(k)))
        out = np.zeros(k.value, dtype=np.float64)
        if k.value:
            _chk(L.mpf_ufboot_tree_logl(self.h, _p(out)))
        return out

    def ufboot_state(self):
        logl = np.zeros(self.ufb_B, dtype=np.float64)
        counts = np.zeros(self.ufb_B, dtype=np.int32)
        trees = np.zeros(self.ufb_B, dtype=np.int32)
        _chk(load_library().mpf_ufboot_get_state(self.h, _p(logl), _p(counts), _p(trees)))
        return logl, counts, trees

    def ufboot_tree(self, tree_index: int):
        back = np.empty(self.nrec, dtype=np.int32)
        _chk(load_library().mpf_ufboot_get_tree(self.h, int(tree_index), _p(back)))
        return back

    def ufboot_adopt(self, samples, scores, tree_of, trees, lengths) -> int:
        """mpf_ufboot_adopt: books of another search chain of the same run -- sample samples[k] is offered trees[tree_of[k]] at REPS
        length scores[k] and takes it when that is strictly shorter than what it holds.  -> number of samples that took one."""
        sm = np.ascontiguousarray(samples, dtype=np.int32)
        sc = np.ascontiguousarray(scores, dtype=np.uint32)
        to = np.ascontiguousarray(tree_of, dtype=np.int32)
        tr = np.ascontiguousarray(trees, dtype=np.int32).reshape(-1, 3 * (2 * self.n - 1)) if len(trees) else np.zeros((0, 3 * (2 * self.n - 1)), dtype=np.int32)
        ln = np.ascontiguousarray(lengths, dtype=np.uint32)
        assert len(sm) == len(sc) == len(to) and len(tr) == len(ln)
        k = C.c_int32()
        _chk(load_library().mpf_ufboot_adopt(self.h, len(sm), _p(sm), _p(sc), _p(to), len(tr), _p(tr), _p(ln), C.byref(k)))
        return int(k.value)

    def ufboot_counters(self) -> dict:
        d, e, r, ms = C.c_uint64(), C.c_uint64(), C.c_uint64(), C.c_double()
        _chk(load_library().mpf_ufboot_get_counters(self.h, C.byref(d), C.byref(e), C.byref(r), C.byref(ms)))
        return {"tie_draws": d.value, "events": e.value, "reps_rows": r.value, "reps_kernel_ms": ms.value}

    def stats(self) -> dict:
        st = Stats()
        _chk(load_library().mpf_get_stats(self.h, C.byref(st)))
        d = st.as_dict()
        # the host's time at the two ends of a device-planned sweep step (booked with option timing >= 1): read-only options in
        # nanoseconds -- mpf_stats keeps its size, callers hold one on their stack
        for key in ("host_front", "host_behind"):
            v = C.c_int64(0)
            if load_library().mpf_get_option(self.h, (key + "_ns_total").encode(), C.byref(v)) == 0:
                d[key + "_ms_total"] = v.value * 1e-6
        return d

    def reset_stats(self):
        _chk(load_library().mpf_reset_stats(self.h))

    def set_option(self, key: str, value: int):
        _chk(load_library().mpf_set_option(self.h, key.encode(), int(value)))

    def scan_trace(self):
        """[workgroups, 4] uint64 timeline of the last planned-program scan (option scan_trace = 1)"""
        L = load_library()
        n = C.c_uint64()
        _chk(L.mpf_get_scan_trace(self.h, None, 0, C.byref(n)))
        out = np.zeros(max(4, n.value), dtype=np.uint64)
        _chk(L.mpf_get_scan_trace(self.h, _p(out), n.value, C.byref(n)))
        return out[:n.value].reshape(-1, 4)

    def get_option(self, key: str) -> int:
        v = C.c_int64(0)
        _chk(load_library().mpf_get_option(self.h, key.encode(), C.byref(v)))
        return int(v.value)
