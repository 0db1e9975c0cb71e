"""ctypes binding of libimpop_hip.so — the stub a reference maintainer would add
(see INTEGRATION.md).  Declares every entry point of include/impop_hip.h.

There is no CPU fallback: if the library cannot be loaded, or no gfx950 device
is usable, the product path raises.
"""
from __future__ import annotations

import ctypes as C
import importlib.util
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
SO_PATH = os.environ.get("IMPOP_HIP_LIBRARY") or os.path.join(_HERE, "libimpop_hip.so")  # env override: tuning builds


class ImpopError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"[impop {code}] {message}")
        self.code = code
        self.message = message


ABI_VERSION = 4  # IMPOP_ABI_VERSION of include/impop_hip.h
E_INVALID, E_NODEVICE, E_HIP, E_NOMEM, E_UNSUPPORTED, E_INTERNAL = -1, -2, -3, -4, -5, -6
KEEP_SITE_BLOCKED, KEEP_HAP_MAJOR, KEEP_DENSE_SCAN, KEEP_NO_RARE_SPLIT = 1, 2, 4, 8
KEEP_NO_SINGLE_STREAM = 16
KEEP_NO_UNIQUE_ROWS = 32
IDENTITY_MATCH, IDENTITY_DICE = 0, 1
EHH_FLANKS_REFERENCE, EHH_FLANKS_TWO_SIDED = 0, 1
EHH_SCAN_MAX_N = 4096  # IMPOP_EHH_SCAN_MAX_N
HAPLOTYPE_MAX_N = 4096  # IMPOP_HAPLOTYPE_MAX_N


class Window(C.Structure):
    _fields_ = [("site_begin", C.c_uint64), ("site_end", C.c_uint64), ("seq_len", C.c_uint64)]


class WindowStats(C.Structure):
    _fields_ = [("n_sites", C.c_uint32), ("s_all", C.c_uint32), ("s_p", C.c_uint32), ("s_a", C.c_uint32),
                ("s_b", C.c_uint32), ("flags", C.c_uint32),
                ("sum_p", C.c_uint64), ("sum_a", C.c_uint64), ("sum_b", C.c_uint64), ("sum_ab", C.c_uint64),
                ("pi", C.c_double), ("pi_site", C.c_double), ("pi_a", C.c_double), ("pi_b", C.c_double),
                ("pi_xy", C.c_double), ("dxy", C.c_double), ("da", C.c_double), ("fst", C.c_double),
                ("tajima_d", C.c_double)]


class ScanParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("d_pi_mode", C.c_int32), ("s_scope", C.c_int32),
                ("tile_blocks", C.c_uint32)]


class SynthParams(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("n_founder", C.c_uint32), ("p_founder", C.c_double),
                ("p_private_word", C.c_double)]


class PairStats(C.Structure):
    _fields_ = [("fst", C.c_double), ("pi_a", C.c_double), ("pi_b", C.c_double), ("pi_xy", C.c_double),
                ("dxy", C.c_double), ("da", C.c_double)]


class PairwiseParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("identity_kind", C.c_int32), ("threshold", C.c_double),
                ("round_digits", C.c_int32), ("d_pi_mode", C.c_int32), ("s_scope", C.c_int32),
                ("fst_method", C.c_uint32)]


class PairwiseStats(C.Structure):
    _fields_ = [("pi", C.c_double), ("pi_site", C.c_double), ("fst", C.c_double), ("pi_a", C.c_double),
                ("pi_b", C.c_double), ("pi_xy", C.c_double), ("dxy", C.c_double), ("da", C.c_double),
                ("tajima_d", C.c_double), ("n_groups", C.c_uint32), ("s_all", C.c_uint32), ("s_p", C.c_uint32),
                ("n_sites", C.c_uint32), ("reserved", C.c_uint64)]


class PanelStats(C.Structure):
    _fields_ = [("pi", C.c_double), ("pi_site", C.c_double), ("tajima_d", C.c_double), ("n_members", C.c_uint32),
                ("n_groups", C.c_uint32), ("s_p", C.c_uint32), ("reserved", C.c_uint32), ("reserved2", C.c_uint64)]


class PanelWindow(C.Structure):
    _fields_ = [("n_sites", C.c_uint32), ("s_all", C.c_uint32)]


class ClusterParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("identity_kind", C.c_int32), ("threshold", C.c_double),
                ("round_digits", C.c_int32), ("reserved", C.c_uint32)]


class ClusterStats(C.Structure):
    _fields_ = [("n_members", C.c_uint32), ("n_clusters", C.c_uint32), ("largest", C.c_uint32), ("n_singletons", C.c_uint32),
                ("sum_sq", C.c_uint64), ("n_sites", C.c_uint32), ("reserved", C.c_uint32)]


class PairdistParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("hist_bins", C.c_uint32), ("hist_width", C.c_uint32), ("reserved", C.c_uint32)]


class PcaParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("k", C.c_uint32), ("tol", C.c_double), ("max_iter", C.c_uint32), ("reserved", C.c_uint32)]


class TreeParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("linkage", C.c_uint32)]


class TreeWindow(C.Structure):
    _fields_ = [("n_members", C.c_uint32), ("n_sites", C.c_uint32), ("n_zero_merges", C.c_uint32), ("n_tied_merges", C.c_uint32),
                ("sum_h", C.c_uint64), ("root_num", C.c_uint64), ("root_size_a", C.c_uint32), ("root_size_b", C.c_uint32),
                ("reserved", C.c_uint64)]


class TreeMerge(C.Structure):
    _fields_ = [("a", C.c_uint32), ("b", C.c_uint32), ("size_a", C.c_uint32), ("size_b", C.c_uint32), ("num", C.c_uint64)]


class TreePanel(C.Structure):
    _fields_ = [("n_members", C.c_uint32), ("largest_clade", C.c_uint32), ("mrca_size", C.c_uint32), ("mrca_merge", C.c_uint32)]


class PermtestParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("n_perm", C.c_uint32), ("seed", C.c_uint64)]


class PermPair(C.Structure):
    _fields_ = [("n_a", C.c_uint32), ("n_b", C.c_uint32), ("n_sites", C.c_uint32), ("n_perm", C.c_uint32), ("wa", C.c_uint64),
                ("wb", C.c_uint64), ("ab", C.c_uint64), ("nn", C.c_uint64), ("ge_fst", C.c_uint32), ("ge_phi", C.c_uint32),
                ("ge_dxy", C.c_uint32), ("ge_snn", C.c_uint32), ("fst", C.c_double), ("phi_st", C.c_double), ("dxy", C.c_double),
                ("snn", C.c_double), ("p_fst", C.c_double), ("p_phi", C.c_double), ("p_dxy", C.c_double), ("p_snn", C.c_double)]


class PermNull(C.Structure):
    _fields_ = [("wa", C.c_uint64), ("wb", C.c_uint64), ("nn", C.c_uint64)]


class PcaWindow(C.Structure):
    _fields_ = [("n_members", C.c_uint32), ("n_sites", C.c_uint32), ("rank", C.c_uint32), ("iterations", C.c_uint32), ("flags", C.c_uint32),
                ("reserved", C.c_uint32), ("sum_h", C.c_uint64), ("lambda", C.c_double * 8), ("resid", C.c_double * 8)]


class DistPanel(C.Structure):
    _fields_ = [("n_members", C.c_uint32), ("n_sites", C.c_uint32), ("n_pairs", C.c_uint64), ("sum_h", C.c_uint64), ("sum_h2", C.c_uint64),
                ("n_zero", C.c_uint64), ("min_h", C.c_uint32), ("max_h", C.c_uint32), ("min_i", C.c_uint32), ("min_j", C.c_uint32),
                ("max_i", C.c_uint32), ("max_j", C.c_uint32)]


class DistPair(C.Structure):
    _fields_ = [("n_pairs", C.c_uint64), ("sum_h", C.c_uint64), ("sum_h2", C.c_uint64), ("n_zero", C.c_uint64), ("min_h", C.c_uint32),
                ("max_h", C.c_uint32), ("min_i", C.c_uint32), ("min_j", C.c_uint32), ("max_i", C.c_uint32), ("max_j", C.c_uint32),
                ("nn_same_a", C.c_uint32), ("nn_same_b", C.c_uint32), ("nn_other_a", C.c_uint32), ("nn_other_b", C.c_uint32),
                ("snn", C.c_double), ("gmin", C.c_double), ("reserved", C.c_uint64)]


class KinshipParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("kin_num", C.c_uint32), ("kin_den", C.c_uint32), ("reserved", C.c_uint32)]


class KinWindow(C.Structure):
    _fields_ = [("n_ind", C.c_uint32), ("n_sites", C.c_uint32), ("n_pairs", C.c_uint64), ("het_het", C.c_uint64), ("ibs0", C.c_uint64),
                ("ibs2", C.c_uint64), ("n_related", C.c_uint32), ("n_undefined", C.c_uint32)]


class KinPair(C.Structure):
    _fields_ = [("t", C.c_uint64 * 9)]


class KinWatch(C.Structure):
    _fields_ = [("het_het", C.c_uint32), ("ibs0", C.c_uint32), ("het_i", C.c_uint32), ("het_j", C.c_uint32)]


class EhhWindow(C.Structure):
    _fields_ = [("site_begin", C.c_uint64), ("site_end", C.c_uint64), ("core_site", C.c_uint64)]


class EhhParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("flanks", C.c_int32), ("ref_hap", C.c_uint32), ("reserved", C.c_uint32),
                ("max_chunk_bytes", C.c_uint64)]


class EhhStats(C.Structure):
    _fields_ = [("n_members", C.c_uint32 * 2), ("ref_allele", C.c_uint32), ("reserved", C.c_uint32),
                ("area_milli", (C.c_int64 * 2) * 2), ("area", C.c_double * 2)]


class HaplotypeParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("reserved", C.c_uint32), ("max_chunk_bytes", C.c_uint64)]


class HaplotypeStats(C.Structure):
    _fields_ = [("n_members", C.c_uint32), ("n_distinct", C.c_uint32), ("largest", C.c_uint32), ("second", C.c_uint32),
                ("n_singletons", C.c_uint32), ("n_sites", C.c_uint32), ("sum_sq", C.c_uint64),
                ("h1", C.c_double), ("h12", C.c_double), ("h2_h1", C.c_double), ("hap_diversity", C.c_double)]


class LdParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_mac", C.c_uint32), ("max_sites", C.c_uint32), ("reserved", C.c_uint32),
                ("max_chunk_bytes", C.c_uint64)]


class LdStats(C.Structure):
    _fields_ = [("n_members", C.c_uint32), ("n_sites", C.c_uint32), ("n_qualifying", C.c_uint32), ("n_used", C.c_uint32),
                ("n_perfect", C.c_uint32), ("n_complete", C.c_uint32), ("omega_split", C.c_uint32), ("reserved", C.c_uint32),
                ("sum_r2", C.c_double), ("sum_dprime", C.c_double), ("zns", C.c_double), ("mean_dprime", C.c_double),
                ("omega_max", C.c_double)]


class RecombParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_mac", C.c_uint32), ("max_sites", C.c_uint32), ("reserved", C.c_uint32),
                ("max_chunk_bytes", C.c_uint64)]


class RecombStats(C.Structure):
    _fields_ = [("n_members", C.c_uint32), ("n_sites", C.c_uint32), ("n_qualifying", C.c_uint32), ("n_used", C.c_uint32),
                ("rmin", C.c_uint32), ("n_incompatible_adjacent", C.c_uint32), ("n_blocks", C.c_uint32),
                ("longest_block_sites", C.c_uint32), ("n_congruent_adjacent", C.c_uint32), ("n_congruent_partitions", C.c_uint32),
                ("n_partitions", C.c_uint32), ("reserved", C.c_uint32), ("n_incompatible", C.c_uint64),
                ("longest_block_begin", C.c_uint64), ("longest_block_end", C.c_uint64), ("four_gamete_fraction", C.c_double),
                ("wall_b", C.c_double), ("wall_q", C.c_double)]


class RecombSite(C.Structure):
    _fields_ = [("left1", C.c_uint32), ("n_left", C.c_uint32), ("rep", C.c_uint32), ("carriers", C.c_uint32)]


class LdbandParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_mac", C.c_uint32), ("band_sites", C.c_uint32), ("n_bins", C.c_uint32),
                ("thr_num", C.c_uint32), ("thr_den", C.c_uint32), ("bin_width", C.c_uint64), ("max_dist", C.c_uint64),
                ("max_chunk_bytes", C.c_uint64)]


class LdbandStats(C.Structure):
    _fields_ = [("n_members", C.c_uint32), ("n_sites", C.c_uint32), ("n_qualifying", C.c_uint32), ("n_kept", C.c_uint32),
                ("n_pairs", C.c_uint64), ("sum_r2_fx", C.c_uint64), ("n_strong", C.c_uint64), ("n_perfect", C.c_uint64),
                ("site_off", C.c_uint64), ("mean_r2", C.c_double)]


class LdbandBin(C.Structure):
    _fields_ = [("pairs", C.c_uint64), ("sum_r2_fx", C.c_uint64), ("n_strong", C.c_uint64)]


class LdbandSite(C.Structure):
    _fields_ = [("coord", C.c_uint64), ("ld_score_fx", C.c_uint64), ("carriers", C.c_uint32), ("n_partners", C.c_uint32),
                ("n_strong", C.c_uint32), ("kept", C.c_uint32)]


class DiploidParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_run", C.c_uint32), ("max_chunk_bytes", C.c_uint64)]


class DiploidStats(C.Structure):
    _fields_ = [("n_ind", C.c_uint32), ("n_sites", C.c_uint32), ("s_p", C.c_uint32), ("het_sites", C.c_uint32),
                ("het_total", C.c_uint64), ("sum_p", C.c_uint64), ("roh_sites_total", C.c_uint64), ("roh_runs_total", C.c_uint32),
                ("longest_run", C.c_uint32), ("ho", C.c_double), ("he", C.c_double), ("f_is", C.c_double), ("f_roh", C.c_double)]


class DiploidInd(C.Structure):
    _fields_ = [("het", C.c_uint32), ("hom_alt", C.c_uint32), ("longest_run", C.c_uint32), ("roh_runs", C.c_uint32),
                ("roh_sites", C.c_uint32), ("reserved", C.c_uint32)]


class IbsParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_sites", C.c_uint32), ("site_begin", C.c_uint64), ("site_end", C.c_uint64),
                ("max_chunk_bytes", C.c_uint64)]


class IbsPair(C.Structure):
    _fields_ = [("h1", C.c_uint32), ("h2", C.c_uint32), ("n_diff", C.c_uint32), ("longest", C.c_uint32), ("n_tracts", C.c_uint32),
                ("reserved", C.c_uint32), ("tract_sites", C.c_uint64)]


class IbsSegment(C.Structure):
    _fields_ = [("h1", C.c_uint32), ("h2", C.c_uint32), ("begin", C.c_uint64), ("end", C.c_uint64), ("pair", C.c_uint32),
                ("flags", C.c_uint32)]


class IbsWindow(C.Structure):
    _fields_ = [("pair_sites", C.c_uint64), ("tracts", C.c_uint32), ("pairs_spanning", C.c_uint32), ("n_sites", C.c_uint32),
                ("reserved", C.c_uint32), ("share", C.c_double)]


class PaintParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("mismatch_cost", C.c_uint32), ("switch_cost", C.c_uint32), ("n_panels", C.c_uint32),
                ("site_begin", C.c_uint64), ("site_end", C.c_uint64), ("site_switch_cost", C.POINTER(C.c_uint32)),
                ("n_site_switch_cost", C.c_uint64), ("group", C.POINTER(C.c_uint32)), ("panel", C.POINTER(C.c_uint8)),
                ("max_chunk_bytes", C.c_uint64)]


class PaintRecipient(C.Structure):
    _fields_ = [("h", C.c_uint32), ("n_donors", C.c_uint32), ("n_segments", C.c_uint32), ("n_mismatch", C.c_uint32),
                ("distinct_donors", C.c_uint32), ("longest_sites", C.c_uint32), ("longest_donor", C.c_uint32), ("reserved", C.c_uint32),
                ("cost", C.c_uint64)]


class PaintSegment(C.Structure):
    _fields_ = [("h", C.c_uint32), ("donor", C.c_uint32), ("begin", C.c_uint64), ("end", C.c_uint64), ("n_sites", C.c_uint32),
                ("n_mismatch", C.c_uint32), ("recipient", C.c_uint32), ("reserved", C.c_uint32)]


class PaintWindow(C.Structure):
    _fields_ = [("n_switches", C.c_uint64), ("n_mismatch", C.c_uint64), ("cells", C.c_uint64), ("copied", C.c_uint64 * 9)]


class IbdParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_sites", C.c_uint32), ("site_begin", C.c_uint64), ("site_end", C.c_uint64),
                ("min_seed", C.c_uint64), ("min_extend", C.c_uint64), ("min_output", C.c_uint64), ("max_gap", C.c_uint64),
                ("map_pos", C.POINTER(C.c_uint64)), ("map_g", C.POINTER(C.c_uint64)), ("n_map", C.c_uint32), ("reserved", C.c_uint32),
                ("max_chunk_bytes", C.c_uint64)]


class IbdPair(C.Structure):
    _fields_ = [("h1", C.c_uint32), ("h2", C.c_uint32), ("n_segments", C.c_uint32), ("n_candidates", C.c_uint32),
                ("total_len", C.c_uint64), ("total_extent", C.c_uint64), ("longest_len", C.c_uint64), ("ibs_sites", C.c_uint64)]


class IbdSegment(C.Structure):
    _fields_ = [("h1", C.c_uint32), ("h2", C.c_uint32), ("begin", C.c_uint64), ("end", C.c_uint64), ("len", C.c_uint64),
                ("ibs_sites", C.c_uint32), ("n_tracts", C.c_uint32), ("pair", C.c_uint32), ("flags", C.c_uint32)]


class IhsParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("min_mac", C.c_uint32), ("cutoff_milli", C.c_uint32), ("reserved", C.c_uint32),
                ("max_extend_bp", C.c_uint64), ("max_extend_sites", C.c_uint64)]


class IhsCore(C.Structure):
    _fields_ = [("site", C.c_uint64), ("n", C.c_uint32 * 2), ("c1", C.c_uint32 * 2), ("flags", C.c_uint32), ("reserved", C.c_uint32),
                ("ihh2", (C.c_uint64 * 2) * 2), ("sl2", (C.c_uint64 * 2) * 2)]


class DstatParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("polarize", C.c_int32), ("tile_blocks", C.c_uint32), ("reserved", C.c_uint32)]


class DstatStats(C.Structure):
    _fields_ = [("n_sites", C.c_uint32), ("n_informative", C.c_uint32), ("n_skipped", C.c_uint32), ("flags", C.c_uint32),
                ("abba", C.c_int64), ("baba", C.c_int64), ("f4_num", C.c_int64), ("fd_den_p2", C.c_int64), ("fd_den_p3", C.c_int64),
                ("d", C.c_double), ("f4", C.c_double), ("fd", C.c_double)]


class SfsParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("outgroup", C.c_int32), ("tile_blocks", C.c_uint32), ("tables", C.c_uint32),
                ("max_chunk_bytes", C.c_uint64)]


class SfsStats(C.Structure):
    _fields_ = [("n_sites", C.c_uint32), ("seg", C.c_uint32), ("eta1", C.c_uint32), ("eta_n1", C.c_uint32), ("n_skipped", C.c_uint32),
                ("flags", C.c_uint32), ("sum_het", C.c_uint64), ("sum_c", C.c_uint64), ("sum_c2", C.c_uint64),
                ("theta_w", C.c_double), ("theta_pi", C.c_double), ("theta_h", C.c_double), ("theta_l", C.c_double),
                ("tajima_d", C.c_double), ("faywu_h", C.c_double), ("faywu_h_norm", C.c_double), ("zeng_e", C.c_double)]


class SfsPair(C.Structure):
    _fields_ = [("private_a", C.c_uint32), ("private_b", C.c_uint32), ("shared", C.c_uint32), ("fixed_a", C.c_uint32),
                ("fixed_b", C.c_uint32), ("n_union", C.c_uint32), ("n_skipped", C.c_uint32), ("flags", C.c_uint32)]


class Pica2Detail(C.Structure):
    _fields_ = [("sum_2pairs", C.c_double), ("n_pairs_with_data", C.c_uint64)]


class IdentityProblem(C.Structure):
    _fields_ = [("ident", C.POINTER(C.c_double)), ("n", C.c_uint32), ("reserved", C.c_uint32), ("seq_len", C.c_uint64),
                ("seed_rank", C.POINTER(C.c_uint32)), ("in_a", C.POINTER(C.c_uint8)), ("in_b", C.POINTER(C.c_uint8)),
                ("tajima_n", C.c_int64), ("tajima_S", C.c_double)]


class IdentityStats(C.Structure):
    _fields_ = [("status", C.c_int32), ("n_groups", C.c_uint32), ("pi", C.c_double), ("pi_site", C.c_double),
                ("sum_2pairs", C.c_double), ("n_pairs_with_data", C.c_uint64), ("fst", C.c_double * 6),
                ("fst_counts", C.c_uint64 * 6), ("tajima_d", C.c_double)]


class IdentityBatchParams(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("round_digits", C.c_int32), ("threshold", C.c_double),
                ("fst_round_digits", C.c_int32), ("reserved", C.c_uint32), ("max_chunk_bytes", C.c_uint64)]


assert C.sizeof(IdentityStats) == 144 and C.sizeof(IdentityProblem) == 64 and C.sizeof(IdentityBatchParams) == 32
assert C.sizeof(WindowStats) == 128 and C.sizeof(Window) == 24 and C.sizeof(PairwiseStats) == 96
assert C.sizeof(ClusterStats) == 32 and C.sizeof(ClusterParams) == 24
assert C.sizeof(PanelStats) == 48 and C.sizeof(PanelWindow) == 8
assert C.sizeof(DistPanel) == 64 and C.sizeof(DistPair) == 96 and C.sizeof(PairdistParams) == 16
PAIRDIST_MAX_N, PAIRDIST_MAX_BINS = 4096, 1024  # IMPOP_PAIRDIST_MAX_N, IMPOP_PAIRDIST_MAX_BINS
assert C.sizeof(PcaParams) == 24 and C.sizeof(PcaWindow) == 160
PCA_MAX_N, PCA_MAX_K, PCA_MAX_DIST_WINDOWS = 1024, 8, 16384  # IMPOP_PCA_MAX_N, IMPOP_PCA_MAX_K, the most windows out_dist2 takes
assert C.sizeof(TreeParams) == 8 and C.sizeof(TreeWindow) == 48 and C.sizeof(TreeMerge) == 24 and C.sizeof(TreePanel) == 16
TREE_MAX_N, TREE_LINKAGES = 1024, {"single": 0, "complete": 1, "average": 2}  # IMPOP_TREE_MAX_N, IMPOP_LINKAGE_*
assert C.sizeof(PermtestParams) == 16 and C.sizeof(PermPair) == 128 and C.sizeof(PermNull) == 24
# IMPOP_PERMTEST_MAX_N, IMPOP_PERMTEST_MAX_PERM, the most entries out_null takes, SCALE of the nn sums
PERMTEST_MAX_N, PERMTEST_MAX_PERM, PERMTEST_MAX_NULL, PERMTEST_SCALE = 1024, 16384, 1 << 22, 2952069120
assert C.sizeof(KinWindow) == 48 and C.sizeof(KinPair) == 72 and C.sizeof(KinWatch) == 16 and C.sizeof(KinshipParams) == 16
KINSHIP_MAX_N, KINSHIP_MAX_WATCH = 2048, 1024  # IMPOP_KINSHIP_MAX_N, IMPOP_KINSHIP_MAX_WATCH
assert C.sizeof(EhhStats) == 64 and C.sizeof(EhhParams) == 24 and C.sizeof(EhhWindow) == 24
assert C.sizeof(HaplotypeStats) == 64 and C.sizeof(HaplotypeParams) == 16
assert C.sizeof(LdStats) == 72 and C.sizeof(LdParams) == 24
LD_MAX_N, LD_MAX_SITES = 4096, 1024
assert C.sizeof(RecombStats) == 96 and C.sizeof(RecombParams) == 24 and C.sizeof(RecombSite) == 16
RECOMB_MAX_N, RECOMB_MAX_SITES = 4096, 16384  # IMPOP_RECOMB_MAX_N, IMPOP_RECOMB_MAX_SITES
assert C.sizeof(LdbandStats) == 64 and C.sizeof(LdbandParams) == 48 and C.sizeof(LdbandBin) == 24 and C.sizeof(LdbandSite) == 32
# IMPOP_LDBAND_MAX_N, IMPOP_LDBAND_MAX_BAND, IMPOP_LDBAND_MAX_BINS, IMPOP_LDBAND_FX_ONE
LDBAND_MAX_N, LDBAND_MAX_BAND, LDBAND_MAX_BINS, LDBAND_FX_ONE = 4096, 1024, 4096, 1 << 30
assert C.sizeof(DiploidStats) == 80 and C.sizeof(DiploidInd) == 24 and C.sizeof(DiploidParams) == 16
DIPLOID_MAX_N = 2048
assert C.sizeof(IbsParams) == 32 and C.sizeof(IbsPair) == 32 and C.sizeof(IbsSegment) == 32 and C.sizeof(IbsWindow) == 32
IBS_MAX_N, IBS_MAX_PAIRS, IBS_OPEN_LEFT, IBS_OPEN_RIGHT = 4096, 8388608, 1, 2
assert C.sizeof(IbdParams) == 88 and C.sizeof(IbdPair) == 48 and C.sizeof(IbdSegment) == 48
IBD_MAX_MAP = 1 << 22  # IMPOP_IBD_MAX_MAP
assert C.sizeof(PaintParams) == 72 and C.sizeof(PaintRecipient) == 40 and C.sizeof(PaintSegment) == 40 and C.sizeof(PaintWindow) == 96
# IMPOP_PAINT_MAX_DONORS, IMPOP_PAINT_MAX_RECIPIENTS, IMPOP_PAINT_MAX_PANELS, IMPOP_PAINT_MAX_COST, IMPOP_PAINT_NO_PANEL
PAINT_MAX_DONORS, PAINT_MAX_RECIPIENTS, PAINT_MAX_PANELS, PAINT_MAX_COST, PAINT_NO_PANEL = 1024, 4096, 8, 1 << 20, 255
assert C.sizeof(IhsParams) == 32 and C.sizeof(IhsCore) == 96
IHS_SCAN_MAX_N = 4096
assert C.sizeof(DstatStats) == 80 and C.sizeof(DstatParams) == 16
DSTAT_GROUP, DSTAT_MAX_QUARTETS = 3, 64
assert C.sizeof(SfsStats) == 112 and C.sizeof(SfsPair) == 32 and C.sizeof(SfsParams) == 24
SFS_PAIR_GROUP, SFS_MAX_PAIRS, SFS_TABLE_1D, SFS_TABLE_JOINT = 4, 28, 1, 2

_vp = C.c_void_p
_u64p = C.POINTER(C.c_uint64)
_u32p = C.POINTER(C.c_uint32)
_u8p = C.POINTER(C.c_uint8)
_i32p = C.POINTER(C.c_int32)
_i64p = C.POINTER(C.c_int64)
_f64p = C.POINTER(C.c_double)

# name -> (restype, argtypes): one line per declaration in include/impop_hip.h
SIGNATURES = {
    "impop_version": (C.c_int, []),
    "impop_last_error": (C.c_char_p, []),
    "impop_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "impop_ctx_create": (C.c_int, [C.c_int, _vp, C.POINTER(_vp)]),
    "impop_ctx_destroy": (C.c_int, [_vp]),
    "impop_ctx_synchronize": (C.c_int, [_vp]),
    "impop_ctx_device_name": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    "impop_matrix_upload": (C.c_int, [_vp, _u64p, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint32, C.POINTER(_vp)]),
    "impop_matrix_synthetic": (C.c_int, [_vp, C.c_uint32, C.c_uint64, C.POINTER(SynthParams), C.c_uint32, C.POINTER(_vp)]),
    "impop_debug_raise_device_error": (C.c_int, [_vp, C.c_uint32]),
    "impop_ctx_gram_timing": (C.c_int, [_vp, C.c_int]),
    "impop_ctx_gram_elapsed": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "impop_ctx_cluster_elapsed": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "impop_ctx_pairdist_elapsed": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "impop_ctx_ehh_elapsed": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "impop_ctx_pca_elapsed": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "impop_debug_timer_pool_sizes": (C.c_int, [_vp, _vp, _u64p]),
    "impop_matrix_synthetic_slab": (C.c_int, [_vp, C.c_uint32, C.c_uint64, C.c_uint64, C.POINTER(SynthParams), C.c_uint32, C.POINTER(_vp)]),
    "impop_matrix_download": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, _u64p, C.c_uint64]),
    "impop_matrix_info": (C.c_int, [_vp, _u32p, _u64p, _u64p, _u32p]),
    "impop_matrix_scan_index_info": (C.c_int, [_vp, _u64p, _u64p, C.c_char_p, C.c_size_t]),
    "impop_matrix_scan_split_info": (C.c_int, [_vp, _u64p, _u64p, _u64p, C.c_char_p, C.c_size_t]),
    "impop_matrix_scan_single_info": (C.c_int, [_vp, _u64p, _u64p, _u64p, C.c_char_p, C.c_size_t]),
    "impop_matrix_scan_unique_info": (C.c_int, [_vp, _u64p, _u64p, _u64p, C.c_char_p, C.c_size_t]),
    "impop_matrix_free": (C.c_int, [_vp, _vp]),
    "impop_scan_plan_create": (C.c_int, [_vp, _vp, C.POINTER(Window), C.c_uint64, _u64p, _u64p, _u64p,
                                         C.POINTER(ScanParams), C.POINTER(_vp)]),
    "impop_scan_plan_set_masks": (C.c_int, [_vp, _u64p, _u64p, _u64p]),
    "impop_scan_plan_launch": (C.c_int, [_vp, _vp]),
    "impop_scan_plan_fetch": (C.c_int, [_vp, C.POINTER(WindowStats)]),
    "impop_scan_plan_info": (C.c_int, [_vp, _u64p, _u64p]),
    "impop_scan_plan_digest_info": (C.c_int, [_vp, C.POINTER(C.c_int), _u64p, _u64p, _u64p, C.c_char_p, C.c_size_t]),
    "impop_scan_plan_device_records": (C.c_int, [_vp, C.POINTER(_vp)]),
    "impop_shard_range": (C.c_int, [C.c_uint64, C.c_int, C.c_int, _u64p, _u64p]),
    "impop_shard_windows": (C.c_int, [C.POINTER(Window), C.c_uint64, C.c_int, C.c_int, _u64p, _u64p, _u64p, _u64p]),
    "impop_scan_sharded": (C.c_int, [C.POINTER(_vp), C.POINTER(_vp), _u64p, C.c_int, C.POINTER(Window), C.c_uint64, _u64p, _u64p,
                                     _u64p, C.POINTER(ScanParams), C.POINTER(WindowStats)]),
    "impop_pairwise_scan_sharded": (C.c_int, [C.POINTER(_vp), C.POINTER(_vp), _u64p, C.c_int, C.POINTER(Window), C.c_uint64, _u64p,
                                              _u64p, _u64p, C.POINTER(PairwiseParams), C.POINTER(PairwiseStats)]),
    "impop_comm_unique_id": (C.c_int, [C.c_char_p]),
    "impop_comm_create": (C.c_int, [_vp, C.c_char_p, C.c_int, C.c_int, C.POINTER(_vp)]),
    "impop_comm_destroy": (C.c_int, [_vp]),
    "impop_gather": (C.c_int, [_vp, _vp, C.c_size_t, _vp]),
    "impop_gather_records": (C.c_int, [_vp, _vp, C.c_uint64, C.POINTER(WindowStats)]),
    "impop_allreduce_i64": (C.c_int, [_vp, _vp, C.c_size_t]),
    "impop_scan_plan_timing": (C.c_int, [_vp, C.c_int]),
    "impop_scan_plan_elapsed": (C.c_int, [_vp, _f64p, _u64p]),
    "impop_scan_plan_destroy": (C.c_int, [_vp]),
    "impop_scan": (C.c_int, [_vp, _vp, C.POINTER(Window), C.c_uint64, _u64p, _u64p, _u64p, C.POINTER(ScanParams),
                             C.POINTER(WindowStats)]),
    "impop_scan_multi": (C.c_int, [_vp, _vp, C.POINTER(Window), C.c_uint64, _u64p, C.c_uint32, C.POINTER(PairStats)]),
    "impop_afs": (C.c_int, [_vp, _vp, C.POINTER(Window), C.c_uint64, _u64p, _u32p]),
    "impop_site_counts": (C.c_int, [_vp, _vp, _u64p, C.c_uint64, C.c_uint64, _u32p]),
    "impop_pairwise_counts": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, _i32p]),
    "impop_pairwise_identity": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, C.c_int, _f64p]),
    "impop_pairwise_scan": (C.c_int, [_vp, _vp, C.POINTER(Window), C.c_uint64, _u64p, _u64p, _u64p,
                                      C.POINTER(PairwiseParams), C.POINTER(PairwiseStats)]),
    "impop_pairwise_scan_panel": (C.c_int, [_vp, _vp, C.POINTER(Window), C.c_uint64, _u64p, C.c_uint32, C.POINTER(PairwiseParams),
                                            C.POINTER(PanelStats), C.POINTER(PairStats), C.POINTER(PanelWindow)]),
    "impop_pairdist_scan": (C.c_int, [_vp, _vp, C.POINTER(Window), C.c_uint64, _u64p, C.c_uint32, C.POINTER(PairdistParams),
                                      C.POINTER(DistPanel), C.POINTER(DistPair), _u32p, _u32p]),
    "impop_pca_scan": (C.c_int, [_vp, _vp, C.POINTER(Window), C.c_uint64, _u64p, C.POINTER(PcaParams), C.POINTER(PcaWindow), _f64p, _f64p]),
    "impop_tree_scan": (C.c_int, [_vp, _vp, C.POINTER(Window), C.c_uint64, _u64p, _u64p, C.c_uint32, C.POINTER(TreeParams),
                                  C.POINTER(TreeWindow), C.POINTER(TreeMerge), C.POINTER(TreePanel)]),
    "impop_ctx_tree_elapsed": (C.c_int, [_vp, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]),
    "impop_permtest_scan": (C.c_int, [_vp, _vp, C.POINTER(Window), C.c_uint64, _u64p, C.c_uint32, C.POINTER(PermtestParams),
                                      C.POINTER(PermPair), C.POINTER(PermNull)]),
    "impop_permtest_labels": (C.c_int, [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, _u64p]),
    "impop_ctx_permtest_elapsed": (C.c_int, [_vp, _f64p, _u64p]),
    "impop_genotypes_create": (C.c_int, [_vp, _vp, _u32p, C.c_uint32, C.POINTER(_vp)]),
    "impop_genotypes_info": (C.c_int, [_vp, _u32p, _u64p, _u64p]),
    "impop_genotypes_download": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, _u64p, C.c_uint64]),
    "impop_genotypes_free": (C.c_int, [_vp, _vp]),
    "impop_kinship_scan": (C.c_int, [_vp, _vp, C.POINTER(Window), C.c_uint64, C.POINTER(KinshipParams), _u32p, C.c_uint32,
                                     C.POINTER(KinWindow), C.POINTER(KinPair), C.POINTER(KinWatch)]),
    "impop_ctx_kinship_elapsed": (C.c_int, [_vp, _f64p, _u64p]),
    "impop_cluster_scan": (C.c_int, [_vp, _vp, C.POINTER(Window), C.c_uint64, _u64p, C.POINTER(ClusterParams),
                                     C.POINTER(ClusterStats), _u32p, _u32p]),
    "impop_pi_from_identity": (C.c_int, [_vp, _f64p, C.c_uint32, C.c_double, C.c_int, C.c_uint64, _u32p, _f64p, _f64p, _u32p, _u32p,
                                         C.POINTER(Pica2Detail)]),
    "impop_pica2_pair_terms": (C.c_int, [_vp, _f64p, C.c_uint32, C.c_int, _u32p, _u32p, C.c_uint32, _f64p, _f64p]),
    "impop_fst_from_identity": (C.c_int, [_vp, _f64p, C.c_uint32, _u8p, _u8p, C.c_uint64, C.c_int, _f64p, _u64p]),
    "impop_matrix_set_site_weights": (C.c_int, [_vp, _vp, _u32p]),
    "impop_matrix_compact": (C.c_int, [_vp, _vp, C.POINTER(_vp)]),
    "impop_matrix_positions": (C.c_int, [_vp, C.c_uint64, C.c_uint64, _u64p, _u64p]),
    "impop_ehh": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, _u64p, C.c_int, _f64p, _u32p]),
    "impop_ehh_scan": (C.c_int, [_vp, _vp, C.POINTER(EhhWindow), C.c_uint64, _u64p, C.POINTER(EhhParams), C.POINTER(EhhStats)]),
    "impop_haplotype_scan": (C.c_int, [_vp, _vp, C.POINTER(Window), C.c_uint64, _u64p, C.POINTER(HaplotypeParams),
                                       C.POINTER(HaplotypeStats), _u32p, _u32p]),
    "impop_ctx_haplotype_elapsed": (C.c_int, [_vp, _f64p, _u64p]),
    "impop_ld_scan": (C.c_int, [_vp, _vp, C.POINTER(Window), C.c_uint64, _u64p, C.POINTER(LdParams), C.POINTER(LdStats), _u64p]),
    "impop_ctx_ld_elapsed": (C.c_int, [_vp, _f64p, _u64p]),
    "impop_recomb_scan": (C.c_int, [_vp, _vp, C.POINTER(Window), C.c_uint64, _u64p, C.POINTER(RecombParams), C.POINTER(RecombStats), _u64p,
                                    C.POINTER(RecombSite)]),
    "impop_ctx_recomb_elapsed": (C.c_int, [_vp, _f64p, _u64p]),
    "impop_ldband_scan": (C.c_int, [_vp, _vp, C.POINTER(Window), C.c_uint64, _u64p, C.POINTER(LdbandParams), C.POINTER(LdbandStats),
                                    C.POINTER(LdbandBin), C.POINTER(LdbandSite), C.c_uint64, _u64p]),
    "impop_ctx_ldband_elapsed": (C.c_int, [_vp, _f64p, _u64p]),
    "impop_diploid_scan": (C.c_int, [_vp, _vp, C.POINTER(Window), C.c_uint64, _u32p, C.c_uint32, C.POINTER(DiploidParams),
                                     C.POINTER(DiploidStats), C.POINTER(DiploidInd)]),
    "impop_ctx_diploid_elapsed": (C.c_int, [_vp, _f64p, _u64p]),
    "impop_ibs_scan": (C.c_int, [_vp, _vp, _u64p, _u32p, C.c_uint64, C.POINTER(Window), C.c_uint64, C.POINTER(IbsParams),
                                 C.POINTER(IbsPair), C.POINTER(IbsSegment), C.c_uint64, _u64p, C.POINTER(IbsWindow)]),
    "impop_ctx_ibs_elapsed": (C.c_int, [_vp, _f64p, _u64p]),
    "impop_ibd_scan": (C.c_int, [_vp, _vp, _u64p, _u32p, C.c_uint64, C.POINTER(Window), C.c_uint64, C.POINTER(IbdParams),
                                 C.POINTER(IbdPair), C.POINTER(IbdSegment), C.c_uint64, _u64p, C.POINTER(IbsWindow)]),
    "impop_ctx_ibd_elapsed": (C.c_int, [_vp, _f64p, _u64p]),
    "impop_paint_scan": (C.c_int, [_vp, _vp, _u64p, _u32p, C.c_uint32, C.POINTER(Window), C.c_uint64, C.POINTER(PaintParams),
                                   C.POINTER(PaintRecipient), C.POINTER(PaintSegment), C.c_uint64, _u64p, _u32p, _u64p,
                                   C.POINTER(PaintWindow), _u32p]),
    "impop_ctx_paint_elapsed": (C.c_int, [_vp, _f64p, _u64p]),
    "impop_ihs_scan": (C.c_int, [_vp, _vp, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, _u64p, _u64p, C.POINTER(IhsParams),
                                 C.POINTER(IhsCore), C.c_uint64, _u64p]),
    "impop_ctx_ihs_elapsed": (C.c_int, [_vp, _f64p, _u64p]),
    "impop_dstat_scan": (C.c_int, [_vp, _vp, C.POINTER(Window), C.c_uint64, _u64p, C.c_uint32, _u32p, C.c_uint32, C.POINTER(DstatParams),
                                   C.POINTER(DstatStats)]),
    "impop_ctx_dstat_elapsed": (C.c_int, [_vp, _f64p, _u64p]),
    "impop_sfs_scan": (C.c_int, [_vp, _vp, C.POINTER(Window), C.c_uint64, _u64p, C.c_uint32, _u32p, C.c_uint32, C.POINTER(SfsParams),
                                 C.POINTER(SfsStats), C.POINTER(SfsPair), _u32p, _u32p]),
    "impop_sfs_neutrality": (C.c_int, [C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, _f64p]),
    "impop_ctx_sfs_elapsed": (C.c_int, [_vp, _f64p, _u64p]),
    "impop_fst_grouped_from_identity": (C.c_int, [_vp, _f64p, C.c_uint32, _u8p, _u8p, C.c_double, C.c_uint64, C.c_int, _u32p, _f64p,
                                                  _u64p]),
    "impop_tajimas_d": (C.c_int, [_vp, _i64p, _f64p, _f64p, C.c_uint64, _f64p, _f64p]),
    "impop_cluster_from_identity": (C.c_int, [_vp, _f64p, C.c_uint32, C.c_double, _u32p, _u32p, _u32p]),
    "impop_py_round": (C.c_int, [_vp, _f64p, C.c_uint64, C.c_int, _f64p]),
    "impop_sim_parse": (C.c_int, [C.c_char_p, C.c_int, C.POINTER(_vp)]),
    "impop_sim_info": (C.c_int, [_vp, _u32p, _u64p, _u64p, _i64p, _u64p]),
    "impop_sim_names": (C.c_int, [_vp, C.c_char_p]),
    "impop_sim_first_seen": (C.c_int, [_vp, _u32p]),
    "impop_sim_bad_text": (C.c_int, [_vp, C.c_char_p, C.c_size_t]),
    "impop_sim_dense": (C.c_int, [_vp, _f64p]),
    "impop_sim_free": (C.c_int, [_vp]),
    "impop_sim_parse_many": (C.c_int, [C.POINTER(C.c_char_p), C.c_uint64, C.c_int, C.c_int, C.POINTER(_vp), _i32p]),
    "impop_tajimas_d_from_pi_site": (C.c_int, [C.c_int64, C.c_double, C.c_double, _f64p]),
    "impop_stats_from_identity_batch": (C.c_int, [_vp, C.POINTER(IdentityProblem), C.c_uint64, C.POINTER(IdentityBatchParams),
                                                  C.POINTER(IdentityStats), _u32p]),
    "impop_gfa_parse": (C.c_int, [C.c_char_p, C.c_char_p, C.POINTER(_vp)]),
    "impop_paths_table_parse": (C.c_int, [C.c_char_p, C.POINTER(_vp)]),
    "impop_gfa_info": (C.c_int, [_vp, _u32p, _u64p, _u64p, _i64p]),
    "impop_gfa_names": (C.c_int, [_vp, C.c_char_p]),
    "impop_gfa_bits": (C.c_int, [_vp, _u64p, C.c_uint64]),
    "impop_gfa_lengths": (C.c_int, [_vp, _u32p]),
    "impop_gfa_positions": (C.c_int, [_vp, _i64p]),
    "impop_gfa_free": (C.c_int, [_vp]),
}

_lib = None


def _preload_hip_runtime() -> None:
    """Make sure exactly one HIP runtime lives in the process.

    PyTorch-ROCm wheels bundle their own libamdhip64.so (soname libamdhip64.so.7,
    same as /opt/rocm's).  If torch is installed we load ITS copy first, by path,
    so that libimpop_hip.so (NEEDED libamdhip64.so.7) and a later `import torch`
    both bind to the same runtime; otherwise the RUNPATH (/opt/rocm/lib) copy is
    used.  torch itself is not imported here.
    """
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec and spec.submodule_search_locations:
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)


def load() -> C.CDLL:
    """Load libimpop_hip.so; raise (never fall back) if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(SO_PATH):
        raise ImpopError(E_UNSUPPORTED, f"{SO_PATH} not found: build it with `python -m impop_amd.build` "
                                         "(hipcc, gfx950). impop_amd has no CPU fallback.")
    _preload_hip_runtime()
    lib = C.CDLL(SO_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if an export is missing
        fn.restype = res
        fn.argtypes = args
    if lib.impop_version() != ABI_VERSION:
        raise ImpopError(E_UNSUPPORTED, f"ABI version {lib.impop_version()} != {ABI_VERSION}")
    _lib = lib
    return lib


def check(rc: int) -> None:
    if rc != 0:
        msg = load().impop_last_error().decode("utf-8", "replace")
        raise ImpopError(rc, msg)
