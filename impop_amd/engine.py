"""Host-side objects over the C ABI: Context, BitMatrix, ScanPlan.

Everything here is marshalling — numpy arrays in, numpy structured records out;
all arithmetic runs in libimpop_hip.so on the GPU.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from ._lib import (IDENTITY_DICE, IDENTITY_MATCH, KEEP_DENSE_SCAN, KEEP_HAP_MAJOR, KEEP_NO_RARE_SPLIT, KEEP_NO_SINGLE_STREAM, KEEP_NO_UNIQUE_ROWS, KEEP_SITE_BLOCKED, ImpopError, PairwiseParams,
                   ClusterParams, ClusterStats, HaplotypeParams, HaplotypeStats, LdParams, LdStats, RecombParams, RecombStats, RecombSite, LdbandParams, LdbandStats, LdbandBin, LdbandSite, DiploidParams, DiploidStats, DiploidInd, IbsParams, IbsPair, IbsSegment, IbsWindow, IbdParams, IbdPair, IbdSegment, PaintParams, PaintRecipient, PaintSegment, PaintWindow, IhsParams, IhsCore, DstatParams, DstatStats, SfsParams, SfsStats, SfsPair, EhhParams, EhhStats, EhhWindow, PairwiseStats, ScanParams, SynthParams, Window, WindowStats, check)

from .ihs import IHS_DTYPE  # noqa: E402

STATS_DTYPE = np.dtype([
    ("n_sites", "<u4"), ("s_all", "<u4"), ("s_p", "<u4"), ("s_a", "<u4"), ("s_b", "<u4"), ("flags", "<u4"),
    ("sum_p", "<u8"), ("sum_a", "<u8"), ("sum_b", "<u8"), ("sum_ab", "<u8"),
    ("pi", "<f8"), ("pi_site", "<f8"), ("pi_a", "<f8"), ("pi_b", "<f8"), ("pi_xy", "<f8"), ("dxy", "<f8"),
    ("da", "<f8"), ("fst", "<f8"), ("tajima_d", "<f8")])
assert STATS_DTYPE.itemsize == 128

PAIRWISE_DTYPE = np.dtype([
    ("pi", "<f8"), ("pi_site", "<f8"), ("fst", "<f8"), ("pi_a", "<f8"), ("pi_b", "<f8"), ("pi_xy", "<f8"),
    ("dxy", "<f8"), ("da", "<f8"), ("tajima_d", "<f8"), ("n_groups", "<u4"), ("s_all", "<u4"), ("s_p", "<u4"),
    ("n_sites", "<u4"), ("reserved", "<u8")])
assert PAIRWISE_DTYPE.itemsize == 96

CLUSTER_DTYPE = np.dtype([("n_members", "<u4"), ("n_clusters", "<u4"), ("largest", "<u4"), ("n_singletons", "<u4"), ("sum_sq", "<u8"),
                          ("n_sites", "<u4"), ("reserved", "<u4")])
assert CLUSTER_DTYPE.itemsize == 32

EHH_DTYPE = np.dtype([("n_members", "<u4", (2,)), ("ref_allele", "<u4"), ("reserved", "<u4"), ("area_milli", "<i8", (2, 2)),
                      ("area", "<f8", (2,))])
assert EHH_DTYPE.itemsize == 64
EHH_WINDOW_DTYPE = np.dtype([("site_begin", "<u8"), ("site_end", "<u8"), ("core_site", "<u8")])
EHH_FLANKS = {"reference": _lib.EHH_FLANKS_REFERENCE, "two-sided": _lib.EHH_FLANKS_TWO_SIDED}

HAPLOTYPE_DTYPE = np.dtype([("n_members", "<u4"), ("n_distinct", "<u4"), ("largest", "<u4"), ("second", "<u4"), ("n_singletons", "<u4"),
                            ("n_sites", "<u4"), ("sum_sq", "<u8"), ("h1", "<f8"), ("h12", "<f8"), ("h2_h1", "<f8"), ("hap_diversity", "<f8")])
assert HAPLOTYPE_DTYPE.itemsize == 64
LD_DTYPE = np.dtype([("n_members", "<u4"), ("n_sites", "<u4"), ("n_qualifying", "<u4"), ("n_used", "<u4"), ("n_perfect", "<u4"),
                     ("n_complete", "<u4"), ("omega_split", "<u4"), ("reserved", "<u4"), ("sum_r2", "<f8"), ("sum_dprime", "<f8"),
                     ("zns", "<f8"), ("mean_dprime", "<f8"), ("omega_max", "<f8")])
assert LD_DTYPE.itemsize == 72
RECOMB_DTYPE = np.dtype([("n_members", "<u4"), ("n_sites", "<u4"), ("n_qualifying", "<u4"), ("n_used", "<u4"), ("rmin", "<u4"),
                         ("n_incompatible_adjacent", "<u4"), ("n_blocks", "<u4"), ("longest_block_sites", "<u4"),
                         ("n_congruent_adjacent", "<u4"), ("n_congruent_partitions", "<u4"), ("n_partitions", "<u4"), ("reserved", "<u4"),
                         ("n_incompatible", "<u8"), ("longest_block_begin", "<u8"), ("longest_block_end", "<u8"),
                         ("four_gamete_fraction", "<f8"), ("wall_b", "<f8"), ("wall_q", "<f8")])
RECOMB_SITE_DTYPE = np.dtype([("left1", "<u4"), ("n_left", "<u4"), ("rep", "<u4"), ("carriers", "<u4")])
assert RECOMB_DTYPE.itemsize == 96 and RECOMB_SITE_DTYPE.itemsize == 16
LDBAND_DTYPE = np.dtype([("n_members", "<u4"), ("n_sites", "<u4"), ("n_qualifying", "<u4"), ("n_kept", "<u4"), ("n_pairs", "<u8"),
                         ("sum_r2_fx", "<u8"), ("n_strong", "<u8"), ("n_perfect", "<u8"), ("site_off", "<u8"), ("mean_r2", "<f8")])
LDBAND_BIN_DTYPE = np.dtype([("pairs", "<u8"), ("sum_r2_fx", "<u8"), ("n_strong", "<u8")])
LDBAND_SITE_DTYPE = np.dtype([("coord", "<u8"), ("ld_score_fx", "<u8"), ("carriers", "<u4"), ("n_partners", "<u4"), ("n_strong", "<u4"),
                              ("kept", "<u4")])
assert LDBAND_DTYPE.itemsize == 64 and LDBAND_BIN_DTYPE.itemsize == 24 and LDBAND_SITE_DTYPE.itemsize == 32
DIPLOID_DTYPE = np.dtype([("n_ind", "<u4"), ("n_sites", "<u4"), ("s_p", "<u4"), ("het_sites", "<u4"), ("het_total", "<u8"), ("sum_p", "<u8"),
                          ("roh_sites_total", "<u8"), ("roh_runs_total", "<u4"), ("longest_run", "<u4"), ("ho", "<f8"), ("he", "<f8"),
                          ("f_is", "<f8"), ("f_roh", "<f8")])
DIPLOID_IND_DTYPE = np.dtype([("het", "<u4"), ("hom_alt", "<u4"), ("longest_run", "<u4"), ("roh_runs", "<u4"), ("roh_sites", "<u4"),
                              ("reserved", "<u4")])
assert DIPLOID_DTYPE.itemsize == 80 and DIPLOID_IND_DTYPE.itemsize == 24
IBS_PAIR_DTYPE = np.dtype([("h1", "<u4"), ("h2", "<u4"), ("n_diff", "<u4"), ("longest", "<u4"), ("n_tracts", "<u4"), ("reserved", "<u4"),
                           ("tract_sites", "<u8")])
IBS_SEGMENT_DTYPE = np.dtype([("h1", "<u4"), ("h2", "<u4"), ("begin", "<u8"), ("end", "<u8"), ("pair", "<u4"), ("flags", "<u4")])
IBS_WINDOW_DTYPE = np.dtype([("pair_sites", "<u8"), ("tracts", "<u4"), ("pairs_spanning", "<u4"), ("n_sites", "<u4"), ("reserved", "<u4"),
                             ("share", "<f8")])
assert IBS_PAIR_DTYPE.itemsize == 32 and IBS_SEGMENT_DTYPE.itemsize == 32 and IBS_WINDOW_DTYPE.itemsize == 32
IBD_PAIR_DTYPE = np.dtype([("h1", "<u4"), ("h2", "<u4"), ("n_segments", "<u4"), ("n_candidates", "<u4"), ("total_len", "<u8"),
                           ("total_extent", "<u8"), ("longest_len", "<u8"), ("ibs_sites", "<u8")])
IBD_SEGMENT_DTYPE = np.dtype([("h1", "<u4"), ("h2", "<u4"), ("begin", "<u8"), ("end", "<u8"), ("len", "<u8"), ("ibs_sites", "<u4"),
                              ("n_tracts", "<u4"), ("pair", "<u4"), ("flags", "<u4")])
assert IBD_PAIR_DTYPE.itemsize == 48 and IBD_SEGMENT_DTYPE.itemsize == 48
PAINT_RECIPIENT_DTYPE = np.dtype([("h", "<u4"), ("n_donors", "<u4"), ("n_segments", "<u4"), ("n_mismatch", "<u4"), ("distinct_donors", "<u4"),
                                  ("longest_sites", "<u4"), ("longest_donor", "<u4"), ("reserved", "<u4"), ("cost", "<u8")])
PAINT_SEGMENT_DTYPE = np.dtype([("h", "<u4"), ("donor", "<u4"), ("begin", "<u8"), ("end", "<u8"), ("n_sites", "<u4"), ("n_mismatch", "<u4"),
                                ("recipient", "<u4"), ("reserved", "<u4")])
PAINT_WINDOW_DTYPE = np.dtype([("n_switches", "<u8"), ("n_mismatch", "<u8"), ("cells", "<u8"), ("copied", "<u8", (9,))])
assert PAINT_RECIPIENT_DTYPE.itemsize == 40 and PAINT_SEGMENT_DTYPE.itemsize == 40 and PAINT_WINDOW_DTYPE.itemsize == 96
DSTAT_DTYPE = np.dtype([("n_sites", "<u4"), ("n_informative", "<u4"), ("n_skipped", "<u4"), ("flags", "<u4"), ("abba", "<i8"), ("baba", "<i8"),
                        ("f4_num", "<i8"), ("fd_den_p2", "<i8"), ("fd_den_p3", "<i8"), ("d", "<f8"), ("f4", "<f8"), ("fd", "<f8")])
assert DSTAT_DTYPE.itemsize == 80
SFS_DTYPE = np.dtype([("n_sites", "<u4"), ("seg", "<u4"), ("eta1", "<u4"), ("eta_n1", "<u4"), ("n_skipped", "<u4"), ("flags", "<u4"),
                      ("sum_het", "<u8"), ("sum_c", "<u8"), ("sum_c2", "<u8"), ("theta_w", "<f8"), ("theta_pi", "<f8"), ("theta_h", "<f8"),
                      ("theta_l", "<f8"), ("tajima_d", "<f8"), ("faywu_h", "<f8"), ("faywu_h_norm", "<f8"), ("zeng_e", "<f8")])
SFS_PAIR_DTYPE = np.dtype([("private_a", "<u4"), ("private_b", "<u4"), ("shared", "<u4"), ("fixed_a", "<u4"), ("fixed_b", "<u4"),
                           ("n_union", "<u4"), ("n_skipped", "<u4"), ("flags", "<u4")])
assert SFS_DTYPE.itemsize == 112 and SFS_PAIR_DTYPE.itemsize == 32

PAIR_DTYPE = np.dtype([("fst", "<f8"), ("pi_a", "<f8"), ("pi_b", "<f8"), ("pi_xy", "<f8"), ("dxy", "<f8"), ("da", "<f8")])
PANEL_DTYPE = np.dtype([("pi", "<f8"), ("pi_site", "<f8"), ("tajima_d", "<f8"), ("n_members", "<u4"), ("n_groups", "<u4"), ("s_p", "<u4"),
                        ("reserved", "<u4"), ("reserved2", "<u8")])
PANEL_WINDOW_DTYPE = np.dtype([("n_sites", "<u4"), ("s_all", "<u4")])
assert PANEL_DTYPE.itemsize == 48 and PANEL_WINDOW_DTYPE.itemsize == 8

DIST_PANEL_DTYPE = np.dtype([("n_members", "<u4"), ("n_sites", "<u4"), ("n_pairs", "<u8"), ("sum_h", "<u8"), ("sum_h2", "<u8"), ("n_zero", "<u8"),
                             ("min_h", "<u4"), ("max_h", "<u4"), ("min_i", "<u4"), ("min_j", "<u4"), ("max_i", "<u4"), ("max_j", "<u4")])
DIST_PAIR_DTYPE = np.dtype([("n_pairs", "<u8"), ("sum_h", "<u8"), ("sum_h2", "<u8"), ("n_zero", "<u8"), ("min_h", "<u4"), ("max_h", "<u4"),
                            ("min_i", "<u4"), ("min_j", "<u4"), ("max_i", "<u4"), ("max_j", "<u4"), ("nn_same_a", "<u4"), ("nn_same_b", "<u4"),
                            ("nn_other_a", "<u4"), ("nn_other_b", "<u4"), ("snn", "<f8"), ("gmin", "<f8"), ("reserved", "<u8")])
assert DIST_PANEL_DTYPE.itemsize == 64 and DIST_PAIR_DTYPE.itemsize == 96
PCA_WINDOW_DTYPE = np.dtype([("n_members", "<u4"), ("n_sites", "<u4"), ("rank", "<u4"), ("iterations", "<u4"), ("flags", "<u4"),
                             ("reserved", "<u4"), ("sum_h", "<u8"), ("lambda", "<f8", (8,)), ("resid", "<f8", (8,))])
assert PCA_WINDOW_DTYPE.itemsize == 160
TREE_WINDOW_DTYPE = np.dtype([("n_members", "<u4"), ("n_sites", "<u4"), ("n_zero_merges", "<u4"), ("n_tied_merges", "<u4"), ("sum_h", "<u8"),
                              ("root_num", "<u8"), ("root_size_a", "<u4"), ("root_size_b", "<u4"), ("reserved", "<u8")])
TREE_MERGE_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("size_a", "<u4"), ("size_b", "<u4"), ("num", "<u8")])
TREE_PANEL_DTYPE = np.dtype([("n_members", "<u4"), ("largest_clade", "<u4"), ("mrca_size", "<u4"), ("mrca_merge", "<u4")])
assert TREE_WINDOW_DTYPE.itemsize == 48 and TREE_MERGE_DTYPE.itemsize == 24 and TREE_PANEL_DTYPE.itemsize == 16
PERM_PAIR_DTYPE = np.dtype([("n_a", "<u4"), ("n_b", "<u4"), ("n_sites", "<u4"), ("n_perm", "<u4"), ("wa", "<u8"), ("wb", "<u8"), ("ab", "<u8"),
                            ("nn", "<u8"), ("ge_fst", "<u4"), ("ge_phi", "<u4"), ("ge_dxy", "<u4"), ("ge_snn", "<u4"), ("fst", "<f8"),
                            ("phi_st", "<f8"), ("dxy", "<f8"), ("snn", "<f8"), ("p_fst", "<f8"), ("p_phi", "<f8"), ("p_dxy", "<f8"),
                            ("p_snn", "<f8")])
PERM_NULL_DTYPE = np.dtype([("wa", "<u8"), ("wb", "<u8"), ("nn", "<u8")])
assert PERM_PAIR_DTYPE.itemsize == 128 and PERM_NULL_DTYPE.itemsize == 24

KIN_WINDOW_DTYPE = np.dtype([("n_ind", "<u4"), ("n_sites", "<u4"), ("n_pairs", "<u8"), ("het_het", "<u8"), ("ibs0", "<u8"), ("ibs2", "<u8"),
                             ("n_related", "<u4"), ("n_undefined", "<u4")])
KIN_PAIR_DTYPE = np.dtype([("t", "<u8", (9,))])
KIN_WATCH_DTYPE = np.dtype([("het_het", "<u4"), ("ibs0", "<u4"), ("het_i", "<u4"), ("het_j", "<u4")])
assert KIN_WINDOW_DTYPE.itemsize == 48 and KIN_PAIR_DTYPE.itemsize == 72 and KIN_WATCH_DTYPE.itemsize == 16

IDENTITY_STATS_DTYPE = np.dtype([
    ("status", "<i4"), ("n_groups", "<u4"), ("pi", "<f8"), ("pi_site", "<f8"), ("sum_2pairs", "<f8"), ("n_pairs_with_data", "<u8"),
    ("fst", "<f8", (6,)), ("fst_counts", "<u8", (6,)), ("tajima_d", "<f8")])
assert IDENTITY_STATS_DTYPE.itemsize == 144

WINDOW_DTYPE = np.dtype([("site_begin", "<u8"), ("site_end", "<u8"), ("seq_len", "<u8")])

IDENTITY_KINDS = {"match": IDENTITY_MATCH, "dice": IDENTITY_DICE}


def pack_hap_major(mat01) -> np.ndarray:
    """0/1 array [n_hap, n_site] -> uint64 [n_hap, ceil(n_site/64)] (bit s&63 of word s>>6)."""
    m = np.ascontiguousarray(mat01, dtype=np.uint8)
    if m.ndim != 2:
        raise ValueError("presence matrix must be 2-D [haplotype, site]")
    n, W = m.shape
    words = max((W + 63) // 64, 1)
    pad = np.zeros((n, words * 64), dtype=np.uint8)
    pad[:, :W] = m
    return np.ascontiguousarray(np.packbits(pad, axis=1, bitorder="little")).view(np.uint64).reshape(n, words)


def unpack_hap_major(bits: np.ndarray, n_site: int) -> np.ndarray:
    b = np.ascontiguousarray(bits, dtype=np.uint64)
    return np.unpackbits(b.view(np.uint8), axis=1, bitorder="little")[:, :n_site]


def pack_mask(flags, n: int) -> np.ndarray:
    """Length-n membership flags (bool / 0-1) -> n-bit uint64 bitset."""
    f = np.ascontiguousarray(flags).astype(np.uint8).ravel()
    if f.size != n:
        raise ValueError(f"mask has {f.size} flags, expected {n}")
    words = max((n + 63) // 64, 1)
    pad = np.zeros(words * 64, dtype=np.uint8)
    pad[:n] = f != 0
    return np.packbits(pad, bitorder="little").view(np.uint64).copy()


def mask_from_indices(indices, n: int) -> np.ndarray:
    f = np.zeros(n, dtype=np.uint8)
    f[np.asarray(list(indices), dtype=np.int64)] = 1
    return pack_mask(f, n)


def _mask_ptr(mask, n):
    if mask is None:
        return None, None
    a = np.asarray(mask)
    if a.dtype != np.uint64:  # flags; uint64 arrays are taken as ready-made bitsets
        a = pack_mask(a, n)
    elif a.size != max((n + 63) // 64, 1):
        raise ValueError("bitset mask has the wrong number of words")
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data_as(C.POINTER(C.c_uint64))


def permtest_labels(seed: int, pair_index: int, m: int, m_a: int, n_perm: int) -> np.ndarray:
    """The labellings impop_permtest_scan uses (impop_permtest_labels; host only): [n_perm, ceil(m / 64)] uint64 masks over the
    m positions of a pair's members in ascending haplotype index, each with exactly m_a ones."""
    out = np.zeros((int(n_perm), (int(m) + 63) // 64), dtype=np.uint64)
    check(_lib.load().impop_permtest_labels(int(seed) & 0xFFFFFFFFFFFFFFFF, int(pair_index), int(m), int(m_a), int(n_perm),
                                            out.ctypes.data_as(C.POINTER(C.c_uint64))))
    return out


def make_windows(windows) -> np.ndarray:
    """[(begin, end[, seq_len])] or structured array -> WINDOW_DTYPE array.
    seq_len defaults to end-begin (LENGTH=end-start, run_pica2_impg.sh:133)."""
    if isinstance(windows, np.ndarray) and windows.dtype == WINDOW_DTYPE:
        return np.ascontiguousarray(windows)
    rows = list(windows)
    out = np.zeros(len(rows), dtype=WINDOW_DTYPE)
    if not rows:
        return out
    # column-wise (a BED file's worth of tuples costs a Python loop over fields otherwise: 1.5 us per field)
    begin = np.fromiter((int(r[0]) for r in rows), dtype=np.uint64, count=len(rows))
    end = np.fromiter((int(r[1]) for r in rows), dtype=np.uint64, count=len(rows))
    out["site_begin"], out["site_end"] = begin, end
    out["seq_len"] = np.fromiter((int(r[2]) if len(r) > 2 and r[2] is not None else max(int(r[1]) - int(r[0]), 0) for r in rows),
                                 dtype=np.uint64, count=len(rows))
    return out


def fixed_windows(n_site: int, size: int, step: Optional[int] = None, seq_len: Optional[int] = None) -> np.ndarray:
    """bedtools-makewindows-style tiling (doc/how_pi.md:42); the last window is clipped."""
    step = step or size
    starts = np.arange(0, max(n_site, 1), step, dtype=np.uint64)
    if step < size:
        starts = starts[starts + np.uint64(1) <= np.uint64(n_site)]
    out = np.zeros(len(starts), dtype=WINDOW_DTYPE)
    out["site_begin"] = starts
    out["site_end"] = np.minimum(starts + np.uint64(size), np.uint64(n_site))
    out["seq_len"] = (out["site_end"] - out["site_begin"]) if seq_len is None else seq_len
    return out[out["site_end"] > out["site_begin"]]


class Context:
    """One GPU + one HIP stream (impop_ctx)."""

    def __init__(self, device: int = 0, stream: Optional[int] = None):
        """stream: None = the context creates its own non-blocking HIP stream; otherwise the integer handle
        of an existing hipStream_t whose ordering the caller relies on (e.g. torch.cuda.Stream(dev).cuda_stream).
        Handle 0 — HIP's legacy null stream, which is what torch's DEFAULT stream reports — is refused: the C
        ABI reads NULL as "create a private stream", and silently doing that would leave the caller's
        collectives / copies unordered with the scans."""
        self._lib = _lib.load()
        self._h = C.c_void_p()
        if stream is not None and int(stream) == 0:
            raise ValueError("Context(stream=0): the null stream cannot be adopted; pass stream=None for a private stream "
                             "or the handle of an explicit stream (torch.cuda.Stream(dev).cuda_stream)")
        check(self._lib.impop_ctx_create(int(device), C.c_void_p(int(stream)) if stream is not None else None, C.byref(self._h)))
        self.device = int(device)

    @property
    def handle(self):
        if not self._h:
            raise ImpopError(_lib.E_INVALID, "context is closed")
        return self._h

    def device_name(self) -> str:
        buf = C.create_string_buffer(128)
        check(self._lib.impop_ctx_device_name(self.handle, buf, 128))
        return buf.value.decode()

    def synchronize(self) -> None:
        check(self._lib.impop_ctx_synchronize(self.handle))

    def gram_timing(self, enable: bool = True) -> None:
        """HIP events around every Gram launch of pairwise_scan on this context (impop_ctx_gram_timing)."""
        check(self._lib.impop_ctx_gram_timing(self.handle, 1 if enable else 0))

    def gram_elapsed(self):
        """-> (summed Gram-kernel ms, launches) since gram_timing(True)"""
        t, k = C.c_double(), C.c_uint64()
        check(self._lib.impop_ctx_gram_elapsed(self.handle, C.byref(t), C.byref(k)))
        return t.value, k.value

    def cluster_elapsed(self):
        """-> (summed clustering-kernel ms of cluster_scan — and Fst-kernel ms of pairwise_scan_panel —, chunks) since gram_timing(True)"""
        t, k = C.c_double(), C.c_uint64()
        check(self._lib.impop_ctx_cluster_elapsed(self.handle, C.byref(t), C.byref(k)))
        return t.value, k.value

    def pairdist_elapsed(self):
        """-> (summed ms of pairdist_scan's distribution kernel, chunks) since gram_timing(True)"""
        t, k = C.c_double(), C.c_uint64()
        check(self._lib.impop_ctx_pairdist_elapsed(self.handle, C.byref(t), C.byref(k)))
        return t.value, k.value

    def pca_elapsed(self):
        """-> ([eigen kernel, distance kernel] ms of pca_scan, chunks) since gram_timing(True)"""
        t, k = (C.c_double * 2)(), C.c_uint64()
        check(self._lib.impop_ctx_pca_elapsed(self.handle, t, C.byref(k)))
        return list(t), k.value

    def tree_elapsed(self):
        """-> (tree kernel ms of tree_scan, chunks) since gram_timing(True)"""
        t, k = C.c_double(), C.c_uint64()
        check(self._lib.impop_ctx_tree_elapsed(self.handle, C.byref(t), C.byref(k)))
        return t.value, k.value

    def permtest_elapsed(self):
        """-> ([preparation kernel, labelling kernel] ms of permtest_scan, chunks) since gram_timing(True)"""
        t, k = (C.c_double * 2)(), C.c_uint64()
        check(self._lib.impop_ctx_permtest_elapsed(self.handle, t, C.byref(k)))
        return list(t), k.value

    def kinship_elapsed(self):
        """-> ([plane build, epilogue] kernel ms of genotypes() / kinship_scan, chunks) since gram_timing(True)"""
        t, k = (C.c_double * 2)(), C.c_uint64()
        check(self._lib.impop_ctx_kinship_elapsed(self.handle, t, C.byref(k)))
        return list(t), k.value

    def ehh_elapsed(self):
        """-> (summed kernel ms of ehh_scan, chunks) since gram_timing(True)"""
        t, k = C.c_double(), C.c_uint64()
        check(self._lib.impop_ctx_ehh_elapsed(self.handle, C.byref(t), C.byref(k)))
        return t.value, k.value

    def haplotype_elapsed(self):
        """-> ([fingerprint, grouping, verification] kernel ms of haplotype_scan, chunks) since gram_timing(True)"""
        t, k = (C.c_double * 3)(), C.c_uint64()
        check(self._lib.impop_ctx_haplotype_elapsed(self.handle, t, C.byref(k)))
        return list(t), k.value

    def ld_elapsed(self):
        """-> ([select, gather, pairs] kernel ms of ld_scan, chunks) since gram_timing(True)"""
        t, k = (C.c_double * 3)(), C.c_uint64()
        check(self._lib.impop_ctx_ld_elapsed(self.handle, t, C.byref(k)))
        return list(t), k.value

    def ldband_elapsed(self):
        """-> ([select, rank + gather, pairs, prune, reduce] kernel ms of ldband_scan, chunks) since gram_timing(True)"""
        t, k = (C.c_double * 5)(), C.c_uint64()
        check(self._lib.impop_ctx_ldband_elapsed(self.handle, t, C.byref(k)))
        return list(t), k.value

    def recomb_elapsed(self):
        """-> ([select, gather, pairs, finish] kernel ms of recomb_scan, chunks) since gram_timing(True)"""
        t, k = (C.c_double * 4)(), C.c_uint64()
        check(self._lib.impop_ctx_recomb_elapsed(self.handle, t, C.byref(k)))
        return list(t), k.value

    def diploid_elapsed(self):
        """-> ([tile, window] kernel ms of diploid_scan, chunks) since gram_timing(True)"""
        t, k = (C.c_double * 2)(), C.c_uint64()
        check(self._lib.impop_ctx_diploid_elapsed(self.handle, t, C.byref(k)))
        return list(t), k.value

    def ibd_elapsed(self):
        """-> ([transpose, walk, combine + close, chain] kernel ms of ibd_scan, site chunks transposed) since gram_timing(True)"""
        t, k = (C.c_double * 4)(), C.c_uint64(0)
        check(self._lib.impop_ctx_ibd_elapsed(self.handle, t, C.byref(k)))
        return [t[0], t[1], t[2], t[3]], int(k.value)

    def paint_elapsed(self):
        """-> ([transpose, forward, backtrack + emit, windows] kernel ms of paint_scan, site chunks the forward kernel ran) since
        gram_timing(True)"""
        t, k = (C.c_double * 4)(), C.c_uint64()
        check(self._lib.impop_ctx_paint_elapsed(self.handle, t, C.byref(k)))
        return list(t), k.value

    def ibs_elapsed(self):
        """-> ([transpose, walk, combine + close] kernel ms of ibs_scan, site chunks transposed) since gram_timing(True)"""
        t, k = (C.c_double * 3)(), C.c_uint64()
        check(self._lib.impop_ctx_ibs_elapsed(self.handle, t, C.byref(k)))
        return list(t), k.value

    def ihs_elapsed(self):
        """-> ([classify + tables, walk] kernel ms of ihs_scan, walks timed) since gram_timing(True)"""
        t, k = (C.c_double * 2)(), C.c_uint64()
        check(self._lib.impop_ctx_ihs_elapsed(self.handle, t, C.byref(k)))
        return list(t), k.value

    def dstat_elapsed(self):
        """-> (summed ms of dstat_scan's streaming launches, launches) since gram_timing(True)"""
        t, k = C.c_double(), C.c_uint64()
        check(self._lib.impop_ctx_dstat_elapsed(self.handle, C.byref(t), C.byref(k)))
        return t.value, k.value

    def sfs_elapsed(self):
        """-> ([summary, table] kernel ms of sfs_scan, summary launches) since gram_timing(True)"""
        t, k = (C.c_double * 2)(), C.c_uint64()
        check(self._lib.impop_ctx_sfs_elapsed(self.handle, t, C.byref(k)))
        return list(t), k.value

    def close(self) -> None:
        if self._h:
            self._lib.impop_ctx_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- matrices -----------------------------------------------------------------
    def upload(self, bits_hap_major: np.ndarray, n_site: int, keep_hap_major: bool = True, dense_scan: bool = False,
               rare_split: bool = True, single_stream: bool = True, unique_rows: bool = True) -> "BitMatrix":
        """dense_scan=True: no variable-site scan index (IMPOP_KEEP_DENSE_SCAN); scans then stream every site.
        rare_split=False: the index keeps every variable site as a row (IMPOP_KEEP_NO_RARE_SPLIT).
        single_stream=False: the split keeps no 2-byte singleton stream (IMPOP_KEEP_NO_SINGLE_STREAM).
        unique_rows=False: the split keeps no distinct-row stream (IMPOP_KEEP_NO_UNIQUE_ROWS)."""
        b = np.ascontiguousarray(bits_hap_major, dtype=np.uint64)
        if b.ndim != 2:
            raise ValueError("bits must be [n_hap, words]")
        h = C.c_void_p()
        keep = KEEP_SITE_BLOCKED | (KEEP_HAP_MAJOR if keep_hap_major else 0) | (KEEP_DENSE_SCAN if dense_scan else 0) \
            | (0 if rare_split else KEEP_NO_RARE_SPLIT) | (0 if single_stream else KEEP_NO_SINGLE_STREAM) \
            | (0 if unique_rows else KEEP_NO_UNIQUE_ROWS)
        check(self._lib.impop_matrix_upload(self.handle, b.ctypes.data_as(C.POINTER(C.c_uint64)), b.shape[0], int(n_site),
                                            b.shape[1], keep, C.byref(h)))
        return BitMatrix(self, h)

    def upload_dense(self, mat01, keep_hap_major: bool = True, dense_scan: bool = False, rare_split: bool = True,
                     single_stream: bool = True, unique_rows: bool = True) -> "BitMatrix":
        m = np.asarray(mat01)
        return self.upload(pack_hap_major(m), m.shape[1], keep_hap_major, dense_scan, rare_split, single_stream, unique_rows)

    def synthetic(self, n_hap: int, n_site: int, seed: int = 20251031, n_founder: int = 8, p_founder: float = 1e-3,
                  p_private_word: float = 3.2e-3, keep_hap_major: bool = False, site_begin: int = 0,
                  dense_scan: bool = False, rare_split: bool = True, single_stream: bool = True,
                  unique_rows: bool = True) -> "BitMatrix":
        """Sites [site_begin, site_begin + n_site) of the synthetic chromosome of `seed` (counter-based generator: a slab is
        a cut of the whole, impop_matrix_synthetic_slab); site 0 of the result is global site `site_begin`.
        dense_scan=True: no variable-site scan index (IMPOP_KEEP_DENSE_SCAN); rare_split=False: an index without the rare/common
        split (IMPOP_KEEP_NO_RARE_SPLIT); single_stream=False: a split without the singleton stream (IMPOP_KEEP_NO_SINGLE_STREAM);
        unique_rows=False: a split without the distinct-row stream (IMPOP_KEEP_NO_UNIQUE_ROWS)."""
        p = SynthParams(int(seed), int(n_founder), float(p_founder), float(p_private_word))
        h = C.c_void_p()
        keep = KEEP_SITE_BLOCKED | (KEEP_HAP_MAJOR if keep_hap_major else 0) | (KEEP_DENSE_SCAN if dense_scan else 0) \
            | (0 if rare_split else KEEP_NO_RARE_SPLIT) | (0 if single_stream else KEEP_NO_SINGLE_STREAM) \
            | (0 if unique_rows else KEEP_NO_UNIQUE_ROWS)
        check(self._lib.impop_matrix_synthetic_slab(self.handle, int(n_hap), int(site_begin), int(n_site), C.byref(p), keep, C.byref(h)))
        return BitMatrix(self, h)

    # ---- statistics on a given identity matrix (the .sim drop-in path) -----------------
    def pi_from_identity(self, ident: np.ndarray, threshold: float, round_digits: Optional[int], seq_len: Optional[int],
                         seed_rank=None, detail: bool = False):
        """-> (pi, pi_site, group_of, n_groups[, (sum_2pairs, n_pairs_with_data)]).  seed_rank: see
        impop_pi_from_identity (position of every element in the reference's set iteration order)."""
        a = np.ascontiguousarray(ident, dtype=np.float64)
        n = a.shape[0] if a.ndim == 2 else 0
        pi, ps, G = C.c_double(), C.c_double(), C.c_uint32()
        grp = np.zeros(max(n, 1), dtype=np.uint32)
        sr = None if seed_rank is None else np.ascontiguousarray(seed_rank, dtype=np.uint32)
        if sr is not None and sr.shape != (n,):
            raise ValueError("seed_rank must have one entry per element")
        det = _lib.Pica2Detail()
        check(self._lib.impop_pi_from_identity(self.handle, a.ctypes.data_as(C.POINTER(C.c_double)), n, float(threshold),
                                               -1 if round_digits is None else int(round_digits), int(seq_len or 0),
                                               sr.ctypes.data_as(C.POINTER(C.c_uint32)) if sr is not None and n else None,
                                               C.byref(pi), C.byref(ps), grp.ctypes.data_as(C.POINTER(C.c_uint32)),
                                               C.byref(G), C.byref(det)))
        out = (pi.value, ps.value, grp[:n].copy(), G.value)
        return out + ((det.sum_2pairs, int(det.n_pairs_with_data)),) if detail else out

    def stats_from_identity_batch(self, problems, threshold: float = 1.0, round_digits: Optional[int] = None,
                                  fst_round_digits: Optional[int] = None, max_chunk_bytes: int = 0, with_groups: bool = True):
        """pica2 / h-fst / Tajima's D for many identity tables of different size in one call (impop_stats_from_identity_batch).
        `problems`: dicts with `ident` ([n, n] doubles, NaN = absent) and optionally `seq_len`, `seed_rank`, `in_a` + `in_b`,
        `tajima_n` + `tajima_S`.  -> (records [k] of IDENTITY_STATS_DTYPE, list of per-problem group_of arrays or None).
        A problem of 1024 or more elements comes back with status E_UNSUPPORTED in its own record."""
        k = len(problems)
        arr = (_lib.IdentityProblem * max(k, 1))()
        keep = []  # the arrays the pointers refer to
        total = 0
        f64p, u32p, u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.POINTER(C.c_uint8)
        for q, pr in zip(arr, problems):
            a = np.ascontiguousarray(pr["ident"], dtype=np.float64)
            n = a.shape[0] if a.ndim == 2 else 0
            if n and a.shape != (n, n):
                raise ValueError("ident must be a square matrix")
            keep.append(a)
            q.ident = a.ctypes.data_as(f64p) if n else None
            q.n = n
            q.seq_len = int(pr.get("seq_len") or 0) if (pr.get("seq_len") or 0) > 0 else 0
            sr = pr.get("seed_rank")
            if sr is not None:
                sr = np.ascontiguousarray(sr, dtype=np.uint32)
                if sr.shape != (n,):
                    raise ValueError("seed_rank must have one entry per element")
                keep.append(sr)
                q.seed_rank = sr.ctypes.data_as(u32p) if n else None
            fa, fb = pr.get("in_a"), pr.get("in_b")
            if (fa is None) != (fb is None):
                raise ValueError("in_a and in_b go together")
            if fa is not None:
                fa = np.ascontiguousarray(fa, dtype=np.uint8)
                fb = np.ascontiguousarray(fb, dtype=np.uint8)
                if fa.shape != (n,) or fb.shape != (n,):
                    raise ValueError("in_a / in_b must have one flag per element")
                if n == 0:  # the flags' presence is carried by the pointers
                    fa, fb = np.zeros(1, np.uint8), np.zeros(1, np.uint8)
                keep += [fa, fb]
                q.in_a, q.in_b = fa.ctypes.data_as(u8p), fb.ctypes.data_as(u8p)
            tn = pr.get("tajima_n")
            q.tajima_n = int(tn) if tn is not None else 0
            q.tajima_S = float(pr.get("tajima_S") or 0.0)
            total += n
        par = _lib.IdentityBatchParams(C.sizeof(_lib.IdentityBatchParams), -1 if round_digits is None else int(round_digits),
                                       float(threshold), -1 if fst_round_digits is None else int(fst_round_digits), 0,
                                       int(max_chunk_bytes))
        out = np.zeros(k, dtype=IDENTITY_STATS_DTYPE)
        grp = np.zeros(max(total, 1), dtype=np.uint32) if with_groups else None
        check(self._lib.impop_stats_from_identity_batch(self.handle, arr, k, C.byref(par),
                                                        out.ctypes.data_as(C.POINTER(_lib.IdentityStats)),
                                                        grp.ctypes.data_as(u32p) if with_groups else None))
        if not with_groups:
            return out, None
        groups, o = [], 0
        for q in arr[:k]:
            groups.append(grp[o:o + q.n].copy())
            o += q.n
        return out, groups

    def pica2_pair_terms(self, ident: np.ndarray, round_digits: Optional[int], rep, group_size):
        """Identity of the representatives and (1 - sim) f_g f_h for every group pair g < h, row-major
        (the Step 2 table of pica2's log, pica2.py:125-145)."""
        a = np.ascontiguousarray(ident, dtype=np.float64)
        n = a.shape[0] if a.ndim == 2 else 0
        r = np.ascontiguousarray(rep, dtype=np.uint32)
        z = np.ascontiguousarray(group_size, dtype=np.uint32)
        G = len(r)
        npair = G * (G - 1) // 2
        sims, vals = np.zeros(max(npair, 1)), np.zeros(max(npair, 1))
        check(self._lib.impop_pica2_pair_terms(self.handle, a.ctypes.data_as(C.POINTER(C.c_double)), n,
                                               -1 if round_digits is None else int(round_digits),
                                               r.ctypes.data_as(C.POINTER(C.c_uint32)), z.ctypes.data_as(C.POINTER(C.c_uint32)), G,
                                               sims.ctypes.data_as(C.POINTER(C.c_double)), vals.ctypes.data_as(C.POINTER(C.c_double))))
        return sims[:npair], vals[:npair]

    def fst_from_identity(self, ident: np.ndarray, in_a, in_b, seq_len: Optional[int], round_digits: Optional[int]):
        a = np.ascontiguousarray(ident, dtype=np.float64)
        n = a.shape[0] if a.ndim == 2 else 0
        fa = np.ascontiguousarray(in_a, dtype=np.uint8)
        fb = np.ascontiguousarray(in_b, dtype=np.uint8)
        out = np.zeros(6)
        cnt = np.zeros(6, dtype=np.uint64)
        check(self._lib.impop_fst_from_identity(self.handle, a.ctypes.data_as(C.POINTER(C.c_double)), n,
                                                fa.ctypes.data_as(C.POINTER(C.c_uint8)), fb.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                int(seq_len) if seq_len and seq_len > 0 else 0,
                                                -1 if round_digits is None else int(round_digits),
                                                out.ctypes.data_as(C.POINTER(C.c_double)), cnt.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out, cnt

    def fst_grouped_from_identity(self, ident: np.ndarray, in_a, in_b, threshold: float, seq_len: Optional[int],
                                  round_digits: Optional[int], seed_rank=None):
        a = np.ascontiguousarray(ident, dtype=np.float64)
        n = a.shape[0] if a.ndim == 2 else 0
        fa = np.ascontiguousarray(in_a, dtype=np.uint8)
        fb = np.ascontiguousarray(in_b, dtype=np.uint8)
        out = np.zeros(6)
        cnt = np.zeros(6, dtype=np.uint64)
        sr = None if seed_rank is None else np.ascontiguousarray(seed_rank, dtype=np.uint32)
        if sr is not None and sr.shape != (n,):
            raise ValueError("seed_rank must have one entry per element")
        check(self._lib.impop_fst_grouped_from_identity(self.handle, a.ctypes.data_as(C.POINTER(C.c_double)), n,
                                                        fa.ctypes.data_as(C.POINTER(C.c_uint8)), fb.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                        float(threshold), int(seq_len) if seq_len and seq_len > 0 else 0,
                                                        -1 if round_digits is None else int(round_digits),
                                                        sr.ctypes.data_as(C.POINTER(C.c_uint32)) if sr is not None and n else None,
                                                        out.ctypes.data_as(C.POINTER(C.c_double)), cnt.ctypes.data_as(C.POINTER(C.c_uint64))))
        return out, cnt

    def tajimas_d(self, n, S, pi, components: bool = False):
        n_a = np.ascontiguousarray(np.atleast_1d(n), dtype=np.int64)
        S_a = np.ascontiguousarray(np.atleast_1d(S), dtype=np.float64)
        pi_a = np.ascontiguousarray(np.atleast_1d(pi), dtype=np.float64)
        cnt = n_a.size
        D = np.zeros(cnt)
        comps = np.zeros((cnt, 10)) if components else None
        check(self._lib.impop_tajimas_d(self.handle, n_a.ctypes.data_as(C.POINTER(C.c_int64)),
                                        S_a.ctypes.data_as(C.POINTER(C.c_double)), pi_a.ctypes.data_as(C.POINTER(C.c_double)),
                                        cnt, D.ctypes.data_as(C.POINTER(C.c_double)),
                                        comps.ctypes.data_as(C.POINTER(C.c_double)) if components else None))
        return (D, comps) if components else D

    def cluster_from_identity(self, ident: np.ndarray, threshold: float):
        a = np.ascontiguousarray(ident, dtype=np.float64)
        n = a.shape[0] if a.ndim == 2 else 0
        cl = np.zeros(max(n, 1), dtype=np.uint32)
        sz = np.zeros(max(n, 1), dtype=np.uint32)
        K = C.c_uint32()
        check(self._lib.impop_cluster_from_identity(self.handle, a.ctypes.data_as(C.POINTER(C.c_double)), n, float(threshold),
                                                    cl.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(K),
                                                    sz.ctypes.data_as(C.POINTER(C.c_uint32))))
        return cl[:n].copy(), K.value, sz[: K.value].copy()

    def py_round(self, x, ndigits: int) -> np.ndarray:
        a = np.ascontiguousarray(np.atleast_1d(x), dtype=np.float64)
        out = np.zeros_like(a)
        check(self._lib.impop_py_round(self.handle, a.ctypes.data_as(C.POINTER(C.c_double)), a.size, int(ndigits),
                                       out.ctypes.data_as(C.POINTER(C.c_double))))
        return out


class BitMatrix:
    """A haplotype x site presence matrix resident in HBM (impop_matrix)."""

    def __init__(self, ctx: Context, handle):
        self.ctx = ctx
        self._h = handle
        n, s, b, bps = C.c_uint32(), C.c_uint64(), C.c_uint64(), C.c_uint32()
        check(ctx._lib.impop_matrix_info(handle, C.byref(n), C.byref(s), C.byref(b), C.byref(bps)))
        self.n_hap, self.n_site, self.device_bytes, self.bytes_per_site = n.value, s.value, b.value, bps.value

    @property
    def handle(self):
        if not self._h:
            raise ImpopError(_lib.E_INVALID, "matrix is freed")
        return self._h

    def free(self) -> None:
        """Release the device memory.  Raises if scan plans created from this matrix are still alive."""
        if self._h:
            check(self.ctx._lib.impop_matrix_free(self.ctx.handle if self.ctx._h else None, self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def set_site_weights(self, weights) -> None:
        """Per-site weights (bp per column; None removes them): scans return the records of the bp-expanded
        matrix while the segregating-site counts keep counting columns (impop_matrix_set_site_weights)."""
        if weights is None:
            check(self.ctx._lib.impop_matrix_set_site_weights(self.ctx.handle, self.handle, None))
            return
        w = np.ascontiguousarray(weights, dtype=np.uint32)
        if w.shape != (self.n_site,):
            raise ValueError("weights must have one entry per site")
        check(self.ctx._lib.impop_matrix_set_site_weights(self.ctx.handle, self.handle, w.ctypes.data_as(C.POINTER(C.c_uint32))))

    def compact(self) -> "BitMatrix":
        """A new matrix holding only the sites that are variable among all haplotypes.  Scans of it take
        windows in THIS matrix's site coordinates and return the same records (impop_matrix_compact)."""
        out = C.c_void_p()
        check(self.ctx._lib.impop_matrix_compact(self.ctx.handle, self.handle, C.byref(out)))
        bm = BitMatrix(self.ctx, out)
        bm.compacted_from_sites = self.n_site
        return bm

    def scan_index_info(self) -> dict:
        """The variable-site scan index: {"n_kept", "index_bytes" (0 = none), "why" (reason there is none, else "")}."""
        k, b = C.c_uint64(), C.c_uint64()
        why = C.create_string_buffer(256)
        check(self.ctx._lib.impop_matrix_scan_index_info(self.handle, C.byref(k), C.byref(b), why, len(why)))
        return {"n_kept": k.value, "index_bytes": b.value, "why": why.value.decode()}

    def scan_split_info(self) -> dict:
        """The rare/common split of the scan index: {"n_rare", "n_common", "rare_bytes"} (all 0 = no split) and "why" (the reason
        there is none, else "")."""
        r, c, b = C.c_uint64(), C.c_uint64(), C.c_uint64()
        why = C.create_string_buffer(256)
        check(self.ctx._lib.impop_matrix_scan_split_info(self.handle, C.byref(r), C.byref(c), C.byref(b), why, len(why)))
        return {"n_rare": r.value, "n_common": c.value, "rare_bytes": b.value, "why": why.value.decode()}

    def scan_single_info(self) -> dict:
        """The singleton stream of the split index: {"n_single", "n_multi", "stream_bytes"} (all 0 = none) and "why" (the reason
        there is none, else "")."""
        s_, m_, b = C.c_uint64(), C.c_uint64(), C.c_uint64()
        why = C.create_string_buffer(256)
        check(self.ctx._lib.impop_matrix_scan_single_info(self.handle, C.byref(s_), C.byref(m_), C.byref(b), why, len(why)))
        return {"n_single": s_.value, "n_multi": m_.value, "stream_bytes": b.value, "why": why.value.decode()}

    def scan_unique_info(self) -> dict:
        """The distinct-row stream of the split index: {"n_unique", "n_common", "stream_bytes"} (all 0 = none) and "why" (the
        reason there is none, else "")."""
        u, c, b = C.c_uint64(), C.c_uint64(), C.c_uint64()
        why = C.create_string_buffer(256)
        check(self.ctx._lib.impop_matrix_scan_unique_info(self.handle, C.byref(u), C.byref(c), C.byref(b), why, len(why)))
        return {"n_unique": u.value, "n_common": c.value, "stream_bytes": b.value, "why": why.value.decode()}

    def positions(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """Original site index of the kept sites of a compacted matrix."""
        count = self.n_site - first if count is None else count
        out = np.zeros(max(count, 0), dtype=np.uint64)
        check(self.ctx._lib.impop_matrix_positions(self.handle, int(first), int(count), out.ctypes.data_as(C.POINTER(C.c_uint64)), None))
        return out

    def download(self, site_begin: int = 0, site_end: Optional[int] = None) -> np.ndarray:
        site_end = self.n_site if site_end is None else site_end
        words = max((site_end - site_begin + 63) // 64, 1)
        out = np.zeros((self.n_hap, words), dtype=np.uint64)
        check(self.ctx._lib.impop_matrix_download(self.ctx.handle, self.handle, int(site_begin), int(site_end),
                                                  out.ctypes.data_as(C.POINTER(C.c_uint64)), words))
        return out

    def plan(self, windows, mask_p=None, mask_a=None, mask_b=None, d_pi_mode: int = 0, s_scope: int = 0,
             tile_blocks: int = 0) -> "ScanPlan":
        return ScanPlan(self, make_windows(windows), mask_p, mask_a, mask_b, d_pi_mode, s_scope, tile_blocks)

    def scan(self, windows, mask_p=None, mask_a=None, mask_b=None, d_pi_mode: int = 0, s_scope: int = 0,
             tile_blocks: int = 0) -> np.ndarray:
        """pi + Hudson Fst + Tajima's D + S for every window in one streaming pass (impop_scan: a plan made, launched once and
        destroyed, which therefore builds no tile digest; plan() is for launching again)."""
        w = make_windows(windows)
        prm = ScanParams(C.sizeof(ScanParams), int(d_pi_mode), int(s_scope), int(tile_blocks))
        kp, pp = _mask_ptr(mask_p, self.n_hap)
        ka, pa = _mask_ptr(mask_a, self.n_hap)
        kb, pb = _mask_ptr(mask_b, self.n_hap)
        out = np.zeros(len(w), dtype=STATS_DTYPE)
        check(self.ctx._lib.impop_scan(self.ctx.handle, self.handle, w.ctypes.data_as(C.POINTER(Window)), len(w), pp, pa, pb,
                                       C.byref(prm), out.ctypes.data_as(C.POINTER(WindowStats))))
        return out

    def scan_multi(self, windows, pops) -> np.ndarray:
        """All-pairs Hudson Fst of K disjoint populations in one pass -> array [n_windows, K(K-1)/2] of
        (fst, pi_a, pi_b, pi_xy, dxy, da); pair order (0,1),(0,2),...,(1,2),..."""
        w = make_windows(windows)
        K = len(pops)
        packed = np.concatenate([_mask_ptr(p, self.n_hap)[0] for p in pops]).astype(np.uint64)
        out = np.zeros((len(w), K * (K - 1) // 2), dtype=PAIR_DTYPE)
        check(self.ctx._lib.impop_scan_multi(self.ctx.handle, self.handle, w.ctypes.data_as(C.POINTER(Window)), len(w),
                                             packed.ctypes.data_as(C.POINTER(C.c_uint64)), K,
                                             out.ctypes.data_as(C.POINTER(_lib.PairStats))))
        return out

    def afs(self, windows, mask=None) -> np.ndarray:
        """Allele-frequency spectrum per window: out[w, c] = #sites with c carriers among `mask`."""
        w = make_windows(windows)
        keep, ptr = _mask_ptr(mask, self.n_hap)
        nP = self.n_hap if mask is None else int(np.unpackbits(keep.view(np.uint8), bitorder="little")[: self.n_hap].sum())
        out = np.zeros((len(w), nP + 1), dtype=np.uint32)
        check(self.ctx._lib.impop_afs(self.ctx.handle, self.handle, w.ctypes.data_as(C.POINTER(Window)), len(w), ptr,
                                      out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def site_counts(self, site_begin: int, site_end: int, mask=None) -> np.ndarray:
        out = np.zeros(max(site_end - site_begin, 0), dtype=np.uint32)
        keep, ptr = _mask_ptr(mask, self.n_hap)
        check(self.ctx._lib.impop_site_counts(self.ctx.handle, self.handle, ptr, int(site_begin), int(site_end),
                                              out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def ehh(self, site_begin: int, site_end: int, mask=None, reverse: bool = False) -> np.ndarray:
        """calc_EHH (scripts/wip/ehhgfa.py:6-21) of the members of `mask` over [site_begin, site_end)."""
        out = np.zeros(max(site_end - site_begin, 0))
        keep, ptr = _mask_ptr(mask, self.n_hap)
        check(self.ctx._lib.impop_ehh(self.ctx.handle, self.handle, int(site_begin), int(site_end), ptr, 1 if reverse else 0,
                                      out.ctypes.data_as(C.POINTER(C.c_double)), None))
        return out

    def pairwise_counts(self, site_begin: int, site_end: int) -> np.ndarray:
        out = np.zeros((self.n_hap, self.n_hap), dtype=np.int32)
        check(self.ctx._lib.impop_pairwise_counts(self.ctx.handle, self.handle, int(site_begin), int(site_end),
                                                  out.ctypes.data_as(C.POINTER(C.c_int32))))
        return out

    def pairwise_identity(self, site_begin: int, site_end: int, kind: str = "match") -> np.ndarray:
        out = np.zeros((self.n_hap, self.n_hap))
        check(self.ctx._lib.impop_pairwise_identity(self.ctx.handle, self.handle, int(site_begin), int(site_end),
                                                    IDENTITY_KINDS[kind], out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def pairwise_scan(self, windows, mask_p=None, mask_a=None, mask_b=None, kind: str = "match", threshold: float = 0.99,
                      round_digits: Optional[int] = None, d_pi_mode: int = 0, s_scope: int = 0,
                      fst_method: str = "direct") -> np.ndarray:
        """Full pica2 / h-fst semantics (threshold grouping, rounding) per window from the bit matrix;
        fst_method='grouped' switches the Fst fields to hud.py's grouped method at the same threshold."""
        w = make_windows(windows)
        out = np.zeros(len(w), dtype=PAIRWISE_DTYPE)
        prm = PairwiseParams(C.sizeof(PairwiseParams), IDENTITY_KINDS[kind], float(threshold),
                             -1 if round_digits is None else int(round_digits), int(d_pi_mode), int(s_scope),
                             {"direct": 0, "grouped": 1}[fst_method])
        kp, pp = _mask_ptr(mask_p, self.n_hap)
        ka, pa = _mask_ptr(mask_a, self.n_hap)
        kb, pb = _mask_ptr(mask_b, self.n_hap)
        check(self.ctx._lib.impop_pairwise_scan(self.ctx.handle, self.handle, w.ctypes.data_as(C.POINTER(Window)), len(w),
                                                pp, pa, pb, C.byref(prm), out.ctypes.data_as(C.POINTER(PairwiseStats))))
        return out

    def pairwise_scan_panel(self, windows, pops, kind: str = "match", threshold: float = 0.99, round_digits: Optional[int] = None,
                            d_pi_mode: int = 0, s_scope: int = 0, want_pairs: bool = True):
        """K disjoint panels and all their pairs from ONE Gram pass per window (impop_pairwise_scan_panel): per panel what
        pairwise_scan(mask_p=panel) returns of pica2 / Tajima's D, per pair what pairwise_scan(mask_a, mask_b) returns of h-fst,
        at any threshold, rounding and identity.
        -> (panels [n_windows, K] PANEL_DTYPE, pairs [n_windows, K(K-1)/2] PAIR_DTYPE in the pair order of scan_multi,
            windows [n_windows] PANEL_WINDOW_DTYPE); want_pairs False skips the Fst work (pairs has no column then)."""
        w = make_windows(windows)
        K = len(pops)
        packed = np.concatenate([_mask_ptr(p, self.n_hap)[0] for p in pops]).astype(np.uint64) if K else np.zeros(1, np.uint64)
        panels = np.zeros((len(w), K), dtype=PANEL_DTYPE)
        pairs = np.zeros((len(w), K * (K - 1) // 2 if want_pairs else 0), dtype=PAIR_DTYPE)
        wins = np.zeros(len(w), dtype=PANEL_WINDOW_DTYPE)
        prm = PairwiseParams(C.sizeof(PairwiseParams), IDENTITY_KINDS[kind], float(threshold),
                             -1 if round_digits is None else int(round_digits), int(d_pi_mode), int(s_scope), 0)
        check(self.ctx._lib.impop_pairwise_scan_panel(self.ctx.handle, self.handle, w.ctypes.data_as(C.POINTER(Window)), len(w),
                                                      packed.ctypes.data_as(C.POINTER(C.c_uint64)), K, C.byref(prm),
                                                      panels.ctypes.data_as(C.POINTER(_lib.PanelStats)),
                                                      pairs.ctypes.data_as(C.POINTER(_lib.PairStats)) if want_pairs else None,
                                                      wins.ctypes.data_as(C.POINTER(_lib.PanelWindow))))
        return panels, pairs, wins

    def pairdist_scan(self, windows, pops, hist_bins: int = 0, hist_width: int = 1):
        """Pairwise-distance distributions of K (1..8) disjoint panels and all their pairs from ONE Gram pass per window
        (impop_pairdist_scan): sums, extremes with the pairs that attain them, nearest-neighbour counts and S_nn, G_min.
        -> (panels [n_windows, K] DIST_PANEL_DTYPE, pairs [n_windows, K(K-1)/2] DIST_PAIR_DTYPE in the pair order of scan_multi,
            hist_within [n_windows, K, hist_bins] uint32, hist_between [n_windows, K(K-1)/2, hist_bins] uint32; both None when
            hist_bins is 0).  A pair counts in bin min(H // hist_width, hist_bins - 1)."""
        w = make_windows(windows)
        K = len(pops)
        NP = K * (K - 1) // 2
        packed = np.concatenate([_mask_ptr(p, self.n_hap)[0] for p in pops]).astype(np.uint64) if K else np.zeros(1, np.uint64)
        panels = np.zeros((len(w), K), dtype=DIST_PANEL_DTYPE)
        pairs = np.zeros((len(w), NP), dtype=DIST_PAIR_DTYPE)
        B = int(hist_bins)
        hw = np.zeros((len(w), K, B), dtype=np.uint32) if B else None
        hb = np.zeros((len(w), NP, B), dtype=np.uint32) if B else None
        prm = _lib.PairdistParams(C.sizeof(_lib.PairdistParams), B, int(hist_width), 0)
        u32p = C.POINTER(C.c_uint32)
        check(self.ctx._lib.impop_pairdist_scan(self.ctx.handle, self.handle, w.ctypes.data_as(C.POINTER(Window)), len(w),
                                                packed.ctypes.data_as(C.POINTER(C.c_uint64)), K, C.byref(prm),
                                                panels.ctypes.data_as(C.POINTER(_lib.DistPanel)),
                                                pairs.ctypes.data_as(C.POINTER(_lib.DistPair)) if NP else None,
                                                hw.ctypes.data_as(u32p) if B else None, hb.ctypes.data_as(u32p) if B and NP else None))
        return panels, pairs, hw, hb

    def pca_scan(self, windows, mask_p=None, k: int = 2, tol: float = 1e-10, max_iter: int = 500, want_vectors: bool = True,
                 want_dist: bool = False):
        """Principal components per window (impop_pca_scan): the k (1..8) largest eigenpairs of the double-centred Hamming
        distance matrix of the members of mask_p, from ONE Gram pass per window.
        -> (records [n_windows] PCA_WINDOW_DTYPE, vectors [n_windows, k, |P|] float64 or None, dist2 [n_windows, n_windows]
            float64 or None).  Vector j of a window is unit length, orthogonal to the ones vector, its largest component positive;
        all zeros for j >= rank.  dist2 is lostruct's distance between windows (NaN rows for windows of rank 0 or unconverged);
        it needs the vectors."""
        w = make_windows(windows)
        if want_dist and not want_vectors:
            raise ValueError("want_dist needs want_vectors")
        kp, pp = _mask_ptr(mask_p, self.n_hap)
        n_p = self.n_hap if mask_p is None else int(np.unpackbits(kp.view(np.uint8), bitorder="little")[: self.n_hap].sum())
        out = np.zeros(len(w), dtype=PCA_WINDOW_DTYPE)
        k = int(k)
        vec = np.zeros((len(w), max(k, 0), n_p), dtype=np.float64) if want_vectors else None
        d2 = np.zeros((len(w), len(w)), dtype=np.float64) if want_dist else None
        prm = _lib.PcaParams(C.sizeof(_lib.PcaParams), k, float(tol), int(max_iter), 0)
        f64p = C.POINTER(C.c_double)
        check(self.ctx._lib.impop_pca_scan(self.ctx.handle, self.handle, w.ctypes.data_as(C.POINTER(Window)), len(w), pp, C.byref(prm),
                                           out.ctypes.data_as(C.POINTER(_lib.PcaWindow)),
                                           vec.ctypes.data_as(f64p) if want_vectors else None,
                                           d2.ctypes.data_as(f64p) if want_dist else None))
        return out, vec, d2

    def tree_scan(self, windows, mask_p=None, pops=None, linkage: str = "average", want_merges: bool = True):
        """Exact linkage trees per window (impop_tree_scan): the single / complete / average (UPGMA) tree of the members of mask_p
        over their Hamming distances, in integers with a fixed tie rule, from ONE Gram pass per window.  pops: up to 8 disjoint
        0/1 flag arrays inside mask_p.
        -> (windows [n_windows] TREE_WINDOW_DTYPE, merges [n_windows, |P| - 1] TREE_MERGE_DTYPE or None, panels [n_windows, K]
            TREE_PANEL_DTYPE or None when there are no pops).  A merge names its two clusters by their lowest member POSITION in
        mask_p; num is the numerator of its value (impop_amd.tree.heights)."""
        w = make_windows(windows)
        kp, pp = _mask_ptr(mask_p, self.n_hap)
        n_p = self.n_hap if mask_p is None else int(np.unpackbits(kp.view(np.uint8), bitorder="little")[: self.n_hap].sum())
        K = len(pops) if pops else 0
        packed = np.concatenate([_mask_ptr(p, self.n_hap)[0] for p in pops]).astype(np.uint64) if K else None
        out = np.zeros(len(w), dtype=TREE_WINDOW_DTYPE)
        merges = np.zeros((len(w), max(n_p - 1, 0)), dtype=TREE_MERGE_DTYPE) if want_merges else None
        panels = np.zeros((len(w), K), dtype=TREE_PANEL_DTYPE) if K else None
        if linkage not in _lib.TREE_LINKAGES:
            raise ValueError("linkage must be one of %s" % ", ".join(_lib.TREE_LINKAGES))
        prm = _lib.TreeParams(C.sizeof(_lib.TreeParams), _lib.TREE_LINKAGES[linkage])
        check(self.ctx._lib.impop_tree_scan(self.ctx.handle, self.handle, w.ctypes.data_as(C.POINTER(Window)), len(w), pp,
                                            packed.ctypes.data_as(C.POINTER(C.c_uint64)) if K else None, K, C.byref(prm),
                                            out.ctypes.data_as(C.POINTER(_lib.TreeWindow)),
                                            merges.ctypes.data_as(C.POINTER(_lib.TreeMerge)) if want_merges else None,
                                            panels.ctypes.data_as(C.POINTER(_lib.TreePanel)) if K else None))
        return out, merges, panels

    def permtest_scan(self, windows, pops, n_perm: int = 1000, seed: int = 1, null: bool = False):
        """Permutation p-values for Hudson's Fst, AMOVA Phi_ST, Dxy and S_nn of every pair of K (2..8) disjoint panels, from ONE Gram
        pass per window (impop_permtest_scan).  The same n_perm labellings (permtest_labels) serve every window of the call.
        -> (pairs [n_windows, K(K-1)/2] PERM_PAIR_DTYPE in the pair order of scan_multi,
            null [n_windows, K(K-1)/2, n_perm] PERM_NULL_DTYPE or None): the observed integers and doubles, how many labellings were
        at least as extreme per test, p = (1 + ge) / (n_perm + 1); null holds every labelling's (wa, wb, nn)."""
        w = make_windows(windows)
        K = len(pops)
        NP = K * (K - 1) // 2
        packed = np.concatenate([_mask_ptr(p, self.n_hap)[0] for p in pops]).astype(np.uint64) if K else np.zeros(1, np.uint64)
        n_perm = int(n_perm)
        pairs = np.zeros((len(w), NP), dtype=PERM_PAIR_DTYPE)
        nul = None
        if null:  # a shape the call refuses (n_perm, the 2^22 entries of a null table) gets no table allocated for it first
            ok = 0 < n_perm <= _lib.PERMTEST_MAX_PERM and len(w) * NP * n_perm <= _lib.PERMTEST_MAX_NULL
            nul = np.zeros((len(w), NP, n_perm) if ok else (1, 1, 1), dtype=PERM_NULL_DTYPE)
        prm = _lib.PermtestParams(C.sizeof(_lib.PermtestParams), max(n_perm, 0), int(seed) & 0xFFFFFFFFFFFFFFFF)
        check(self.ctx._lib.impop_permtest_scan(self.ctx.handle, self.handle, w.ctypes.data_as(C.POINTER(Window)), len(w),
                                                packed.ctypes.data_as(C.POINTER(C.c_uint64)), K, C.byref(prm),
                                                pairs.ctypes.data_as(C.POINTER(_lib.PermPair)),
                                                nul.ctypes.data_as(C.POINTER(_lib.PermNull)) if null else None))
        return pairs, nul

    def genotypes(self, pairs) -> "Genotypes":
        """The genotype planes of N >= 2 diploid individuals (impop_genotypes_create): pairs = [N, 2] haplotype indices as
        diploid_scan takes them.  The handle owns its memory; this matrix may be freed afterwards."""
        pr = np.asarray(pairs)
        if pr.size and (pr.ndim != 2 or pr.shape[1] != 2):
            raise ValueError("pairs must be [N, 2] haplotype indices")
        if pr.size and (pr.min() < 0 or pr.max() > 0xFFFFFFFF):
            raise ValueError("haplotype index outside 0 .. 2^32 - 1")
        pr = np.ascontiguousarray(pr.reshape(-1, 2), dtype=np.uint32)
        out = C.c_void_p()
        check(self.ctx._lib.impop_genotypes_create(self.ctx.handle, self.handle, pr.ctypes.data_as(C.POINTER(C.c_uint32)), len(pr),
                                                   C.byref(out)))
        return Genotypes(self.ctx, out)

    def cluster_scan(self, windows, mask_p=None, kind: str = "match", threshold: float = 1.0, round_digits: Optional[int] = None,
                     want_members: bool = True):
        """af.cluster (af.py:35-54) per window from the bit matrix (impop_cluster_scan): components of
        {identity >= threshold} over the members of mask_p, ordered by (-size, smallest member index).
        -> records (CLUSTER_DTYPE), and with want_members also cluster_of and sizes, both [n_windows, |P|]
        (members in ascending haplotype index; sizes: first n_clusters valid, the rest 0)."""
        w = make_windows(windows)
        out = np.zeros(len(w), dtype=CLUSTER_DTYPE)
        prm = ClusterParams(C.sizeof(ClusterParams), IDENTITY_KINDS[kind], float(threshold),
                            -1 if round_digits is None else int(round_digits), 0)
        kp, pp = _mask_ptr(mask_p, self.n_hap)
        n_p = self.n_hap if mask_p is None else int(np.unpackbits(kp.view(np.uint8), bitorder="little")[: self.n_hap].sum())
        cl = np.zeros((len(w), n_p), dtype=np.uint32) if want_members else None
        sz = np.zeros((len(w), n_p), dtype=np.uint32) if want_members else None
        u32p = C.POINTER(C.c_uint32)
        check(self.ctx._lib.impop_cluster_scan(self.ctx.handle, self.handle, w.ctypes.data_as(C.POINTER(Window)), len(w), pp, C.byref(prm),
                                               out.ctypes.data_as(C.POINTER(ClusterStats)),
                                               cl.ctypes.data_as(u32p) if want_members else None,
                                               sz.ctypes.data_as(u32p) if want_members else None))
        return (out, cl, sz) if want_members else out

    def haplotype_scan(self, windows, mask_p=None, want_members: bool = False, max_chunk_bytes: int = 0):
        """Haplotype-frequency statistics per window (impop_haplotype_scan): the classes of members of mask_p whose bits agree at
        every column of the window, from the scan's own stream (no hap-major operand).  -> records (HAPLOTYPE_DTYPE: K = n_distinct,
        H1, H12, H2/H1, haplotype diversity), and with want_members also class_of and sizes, both [n_windows, |P|], laid out and
        ordered like cluster_scan's tables."""
        w = make_windows(windows)
        out = np.zeros(len(w), dtype=HAPLOTYPE_DTYPE)
        prm = HaplotypeParams(C.sizeof(HaplotypeParams), 0, int(max_chunk_bytes))
        kp, pp = _mask_ptr(mask_p, self.n_hap)
        n_p = self.n_hap if mask_p is None else int(np.unpackbits(kp.view(np.uint8), bitorder="little")[: self.n_hap].sum())
        cl = np.zeros((len(w), n_p), dtype=np.uint32) if want_members else None
        sz = np.zeros((len(w), n_p), dtype=np.uint32) if want_members else None
        u32p = C.POINTER(C.c_uint32)
        check(self.ctx._lib.impop_haplotype_scan(self.ctx.handle, self.handle, w.ctypes.data_as(C.POINTER(Window)), len(w), pp, C.byref(prm),
                                                 out.ctypes.data_as(C.POINTER(HaplotypeStats)),
                                                 cl.ctypes.data_as(u32p) if want_members else None,
                                                 sz.ctypes.data_as(u32p) if want_members else None))
        return (out, cl, sz) if want_members else out

    def ld_scan(self, windows, mask_p=None, min_mac: int = 1, max_sites: int = 512, want_sites: bool = False, max_chunk_bytes: int = 0):
        """Linkage disequilibrium per window (impop_ld_scan): among the members of mask_p, the sites with minor-allele count >=
        min_mac, thinned evenly to at most max_sites, all their pairs.  -> records (LD_DTYPE: ZnS, mean |D'|, the perfect and
        complete pairs, Kim-Nielsen omega_max and its split), and with want_sites also used_sites [n_windows, max_sites] uint64:
        the original coordinates of a window's used sites, first n_used valid, the rest 0."""
        w = make_windows(windows)
        out = np.zeros(len(w), dtype=LD_DTYPE)
        prm = LdParams(C.sizeof(LdParams), int(min_mac), int(max_sites), 0, int(max_chunk_bytes))
        kp, pp = _mask_ptr(mask_p, self.n_hap)
        sites = np.zeros((len(w), int(max_sites) if max_sites else 512), dtype=np.uint64) if want_sites else None
        check(self.ctx._lib.impop_ld_scan(self.ctx.handle, self.handle, w.ctypes.data_as(C.POINTER(Window)), len(w), pp, C.byref(prm),
                                          out.ctypes.data_as(C.POINTER(LdStats)),
                                          sites.ctypes.data_as(C.POINTER(C.c_uint64)) if want_sites else None))
        return (out, sites) if want_sites else out

    def recomb_scan(self, windows, mask_p=None, min_mac: int = 2, max_sites: int = 4096, want_sites: bool = False,
                    want_site_table: bool = False, max_chunk_bytes: int = 0):
        """Recombination per window (impop_recomb_scan): among the members of mask_p, the sites with minor-allele count >= min_mac,
        thinned evenly to at most max_sites, the four-gamete test over all their pairs.  -> records (RECOMB_DTYPE: Hudson-Kaplan
        R_min, incompatible pairs, four-gamete blocks, Wall's B and Q), then with want_sites used_sites [n_windows, max_sites]
        uint64 (original coordinates), then with want_site_table the per-site rows [n_windows, max_sites] (RECOMB_SITE_DTYPE:
        left1, n_left, rep, carriers); the first n_used entries of a row are valid, the rest 0."""
        w = make_windows(windows)
        out = np.zeros(len(w), dtype=RECOMB_DTYPE)
        prm = RecombParams(C.sizeof(RecombParams), int(min_mac), int(max_sites), 0, int(max_chunk_bytes))
        kp, pp = _mask_ptr(mask_p, self.n_hap)
        cols = int(max_sites) if max_sites else 4096
        sites = np.zeros((len(w), cols), dtype=np.uint64) if want_sites else None
        table = np.zeros((len(w), cols), dtype=RECOMB_SITE_DTYPE) if want_site_table else None
        check(self.ctx._lib.impop_recomb_scan(self.ctx.handle, self.handle, w.ctypes.data_as(C.POINTER(Window)), len(w), pp, C.byref(prm),
                                              out.ctypes.data_as(C.POINTER(RecombStats)),
                                              sites.ctypes.data_as(C.POINTER(C.c_uint64)) if want_sites else None,
                                              table.ctypes.data_as(C.POINTER(RecombSite)) if want_site_table else None))
        res = (out,) + ((sites,) if want_sites else ()) + ((table,) if want_site_table else ())
        return res if len(res) > 1 else out

    def ldband_scan(self, windows, mask_p=None, min_mac: int = 2, band_sites: int = 256, max_dist: int = 0, bin_width: int = 1000,
                    n_bins: int = 100, threshold=(1, 5), want_bins: bool = False, want_sites: bool = False, max_chunk_bytes: int = 0):
        """Banded LD per window (impop_ldband_scan): among the members of mask_p, every site with minor-allele count >= min_mac (no
        thinning) against its next band_sites such sites, no further than max_dist apart (0: no limit).  -> records (LDBAND_DTYPE:
        pairs, the fixed-point sum of r2, strong and perfect pairs, sites a greedy pruning at r2 > threshold[0] / threshold[1]
        keeps, site_off, mean_r2), then with want_bins the decay counters [n_windows, n_bins] (LDBAND_BIN_DTYPE), then with
        want_sites the site table as ONE flat array (LDBAND_SITE_DTYPE: coord, ld_score_fx, carriers, n_partners, n_strong, kept):
        window w's rows are [site_off[w], site_off[w] + n_qualifying[w]).  The table is sized by a first call without one."""
        w = make_windows(windows)
        out = np.zeros(len(w), dtype=LDBAND_DTYPE)
        prm = LdbandParams(C.sizeof(LdbandParams), int(min_mac), int(band_sites), int(n_bins), int(threshold[0]), int(threshold[1]),
                           int(bin_width), int(max_dist), int(max_chunk_bytes))
        kp, pp = _mask_ptr(mask_p, self.n_hap)
        bins = np.zeros((len(w), max(int(n_bins), 0)), dtype=LDBAND_BIN_DTYPE) if want_bins else None

        def call(table, capacity):
            rows = C.c_uint64(0)
            check(self.ctx._lib.impop_ldband_scan(self.ctx.handle, self.handle, w.ctypes.data_as(C.POINTER(Window)), len(w), pp, C.byref(prm),
                                                  out.ctypes.data_as(C.POINTER(LdbandStats)),
                                                  bins.ctypes.data_as(C.POINTER(LdbandBin)) if want_bins else None,
                                                  table.ctypes.data_as(C.POINTER(LdbandSite)) if table is not None else None, capacity,
                                                  C.byref(rows)))
            return rows.value

        table = None
        if want_sites:
            total = call(None, 0)
            table = np.zeros(total, dtype=LDBAND_SITE_DTYPE)
            if total and call(table, total) != total:
                raise ImpopError("impop_ldband_scan: the site table's size changed between two calls")
        else:
            call(None, 0)
        res = (out,) + ((bins,) if want_bins else ()) + ((table,) if want_sites else ())
        return res if len(res) > 1 else out

    def diploid_scan(self, windows, pairs, min_run: int, want_individuals: bool = False, max_chunk_bytes: int = 0):
        """The individual level of a windowed scan (impop_diploid_scan): pairs = [N, 2] haplotype indices, the two copies of each
        diploid individual.  -> records (DIPLOID_DTYPE: heterozygous sites, observed / expected heterozygosity, F_IS, runs of
        homozygosity of at least min_run sites, F_ROH), and with want_individuals also the rows [n_windows, N]
        (DIPLOID_IND_DTYPE: het, hom_alt, longest_run, roh_runs, roh_sites per individual)."""
        w = make_windows(windows)
        pr = np.asarray(pairs)
        if pr.size and (pr.ndim != 2 or pr.shape[1] != 2):
            raise ValueError("pairs must be [N, 2] haplotype indices")
        if pr.size and (pr.min() < 0 or pr.max() > 0xFFFFFFFF):
            raise ValueError("haplotype index outside 0 .. 2^32 - 1")
        pr = np.ascontiguousarray(pr.reshape(-1, 2), dtype=np.uint32)
        n_ind = len(pr)
        out = np.zeros(len(w), dtype=DIPLOID_DTYPE)
        prm = DiploidParams(C.sizeof(DiploidParams), int(min_run), int(max_chunk_bytes))
        ind = np.zeros((len(w), n_ind), dtype=DIPLOID_IND_DTYPE) if want_individuals else None
        check(self.ctx._lib.impop_diploid_scan(self.ctx.handle, self.handle, w.ctypes.data_as(C.POINTER(Window)), len(w),
                                               pr.ctypes.data_as(C.POINTER(C.c_uint32)), n_ind, C.byref(prm),
                                               out.ctypes.data_as(C.POINTER(DiploidStats)),
                                               ind.ctypes.data_as(C.POINTER(DiploidInd)) if want_individuals else None))
        return (out, ind) if want_individuals else out

    def _pair_list_args(self, pairs, mask_p):
        """the pair arguments of ibs_scan / ibd_scan -> (pointer or None, n_pairs, the array it points into, records to expect)"""
        pp, n_pairs, pr = None, 0, None
        if pairs is not None:
            pr = np.asarray(pairs)
            if pr.size and (pr.ndim != 2 or pr.shape[1] != 2):
                raise ValueError("pairs must be [n, 2] haplotype indices")
            if pr.size and (pr.min() < 0 or pr.max() > 0xFFFFFFFF):
                raise ValueError("haplotype index outside 0 .. 2^32 - 1")
            pr = np.ascontiguousarray(pr.reshape(-1, 2), dtype=np.uint32)
            n_pairs = len(pr)
            pp = pr.ctypes.data_as(C.POINTER(C.c_uint32))
            n_rec = n_pairs
        else:
            flags = None if mask_p is None else np.asarray(mask_p)
            if flags is None:
                k = self.n_hap
            elif flags.dtype == np.uint64:
                k = int(sum(bin(int(x)).count("1") for x in flags))
            else:
                k = int(np.count_nonzero(flags))
            n_rec = k * (k - 1) // 2
        return pp, n_pairs, pr, n_rec

    def ibs_scan(self, pairs=None, mask_p=None, min_sites: int = 1, site_begin: int = 0, site_end: Optional[int] = None, windows=None,
                 want_segments: bool = True, max_chunk_bytes: int = 0, seg_capacity: Optional[int] = None):
        """Pairwise identity-by-state tracts over [site_begin, site_end) (impop_ibs_scan; site_end None = the matrix's end): every
        pair of the members of mask_p (None = all haplotypes), or pairs = [n, 2] haplotype indices.  -> (pair records
        (IBS_PAIR_DTYPE), segments (IBS_SEGMENT_DTYPE: the tracts of at least min_sites sites, pair-major) or None, window records
        (IBS_WINDOW_DTYPE) or None, the total number of segments).  Segments: one counting call, then one filling call; or, with
        seg_capacity given, one call with room for that many (None when the list is longer)."""
        pp, n_pairs, pr, n_rec = self._pair_list_args(pairs, mask_p)
        mk, mp = _mask_ptr(mask_p, self.n_hap)
        w = None if windows is None else make_windows(windows)
        prm = IbsParams(C.sizeof(IbsParams), int(min_sites), int(site_begin), 0 if site_end is None else int(site_end), int(max_chunk_bytes))
        rec = np.zeros(max(n_rec, 0), dtype=IBS_PAIR_DTYPE)
        win = None if w is None else np.zeros(len(w), dtype=IBS_WINDOW_DTYPE)
        total = C.c_uint64(0)

        def call(seg, cap):
            check(self.ctx._lib.impop_ibs_scan(self.ctx.handle, self.handle, mp, pp, n_pairs,
                                               None if w is None else w.ctypes.data_as(C.POINTER(Window)), 0 if w is None else len(w),
                                               C.byref(prm), rec.ctypes.data_as(C.POINTER(IbsPair)),
                                               None if seg is None else seg.ctypes.data_as(C.POINTER(IbsSegment)), cap, C.byref(total),
                                               None if win is None else win.ctypes.data_as(C.POINTER(IbsWindow))))

        seg = None
        if not want_segments:
            call(None, 0)
        elif seg_capacity is not None:
            seg = np.zeros(int(seg_capacity), dtype=IBS_SEGMENT_DTYPE)
            call(seg, len(seg))
            seg = seg[:total.value] if total.value <= len(seg) else None
        else:
            call(None, 0)
            seg = np.zeros(total.value, dtype=IBS_SEGMENT_DTYPE)
            if total.value:
                call(seg, len(seg))
        return rec, seg, win, int(total.value)

    def ibd_scan(self, min_seed: int, min_extend: int, min_output: int, max_gap: int = 0, min_sites: int = 1, map_pos=None, map_g=None,
                 pairs=None, mask_p=None, site_begin: int = 0, site_end: Optional[int] = None, windows=None, want_segments: bool = True,
                 max_chunk_bytes: int = 0, seg_capacity: Optional[int] = None):
        """IBD segments over [site_begin, site_end) (impop_ibd_scan): a pair's exact IBS tracts of at least min_sites sites and
        min_extend length, joined across gaps of at most max_gap coordinates; a chain is reported when it holds a tract of at least
        min_seed and is min_output long.  Lengths are in the units of the map (map_pos, map_g: breakpoints in original site
        coordinates and their uint64 map values), or sites without one.  Pairs as ibs_scan.  -> (pair records (IBD_PAIR_DTYPE),
        segments (IBD_SEGMENT_DTYPE, pair-major) or None, window records (IBS_WINDOW_DTYPE, over the segments) or None, the total
        number of segments).  Segments: one counting call, then one filling call; or, with seg_capacity given, one call with room
        for that many (None when the list is longer)."""
        pp, n_pairs, pr, n_rec = self._pair_list_args(pairs, mask_p)
        mk, mp = _mask_ptr(mask_p, self.n_hap)
        w = None if windows is None else make_windows(windows)
        if (map_pos is None) != (map_g is None):
            raise ValueError("map_pos and map_g go together")
        mpos = mg = None
        if map_pos is not None:
            mpos, mg = np.ascontiguousarray(map_pos, dtype=np.uint64).reshape(-1), np.ascontiguousarray(map_g, dtype=np.uint64).reshape(-1)
            if len(mpos) != len(mg):
                raise ValueError("map_pos and map_g differ in length")
        n_map = 0 if mpos is None else len(mpos)
        prm = IbdParams(C.sizeof(IbdParams), int(min_sites), int(site_begin), 0 if site_end is None else int(site_end), int(min_seed),
                        int(min_extend), int(min_output), int(max_gap), mpos.ctypes.data_as(C.POINTER(C.c_uint64)) if n_map else None,
                        mg.ctypes.data_as(C.POINTER(C.c_uint64)) if n_map else None, n_map, 0, int(max_chunk_bytes))
        rec = np.zeros(max(n_rec, 0), dtype=IBD_PAIR_DTYPE)
        win = None if w is None else np.zeros(len(w), dtype=IBS_WINDOW_DTYPE)
        total = C.c_uint64(0)

        def call(seg, cap):
            check(self.ctx._lib.impop_ibd_scan(self.ctx.handle, self.handle, mp, pp, n_pairs,
                                               None if w is None else w.ctypes.data_as(C.POINTER(Window)), 0 if w is None else len(w),
                                               C.byref(prm), rec.ctypes.data_as(C.POINTER(IbdPair)),
                                               None if seg is None else seg.ctypes.data_as(C.POINTER(IbdSegment)), cap, C.byref(total),
                                               None if win is None else win.ctypes.data_as(C.POINTER(IbsWindow))))

        seg = None
        if not want_segments:
            call(None, 0)
        elif seg_capacity is not None:
            seg = np.zeros(int(seg_capacity), dtype=IBD_SEGMENT_DTYPE)
            call(seg, len(seg))
            seg = seg[:total.value] if total.value <= len(seg) else None
        else:
            call(None, 0)
            seg = np.zeros(total.value, dtype=IBD_SEGMENT_DTYPE)
            if total.value:
                call(seg, len(seg))
        return rec, seg, win, int(total.value)

    def paint_scan(self, recipients, donors=None, mismatch_cost: int = 1, switch_cost: int = 1, site_switch_cost=None, group=None,
                   panel=None, n_panels: int = 0, site_begin: int = 0, site_end: Optional[int] = None, windows=None,
                   want_segments: bool = True, want_chunks: bool = True, want_ancestry: bool = True, max_chunk_bytes: int = 0,
                   seg_capacity: Optional[int] = None):
        """Li-Stephens Viterbi mosaics (impop_paint_scan): every haplotype of `recipients` painted from the donors (a 0/1 or packed
        mask over the haplotypes, None = all) other than those of its own group (group: uint32 per haplotype, None = every
        haplotype its own group), with integer costs: mismatch_cost per differing site, switch_cost (or site_switch_cost[s], one
        per stored site of the range) per change of donor.  panel: uint8 per haplotype (0 .. n_panels - 1, 255 = none).
        -> dict(recipients=PAINT_RECIPIENT_DTYPE, segments=PAINT_SEGMENT_DTYPE or None, n_segments, chunk_counts / chunk_sites =
        [n_rec, n_hap] or None, windows=PAINT_WINDOW_DTYPE or None, anc=[n_windows, n_rec, n_panels + 1] or None).  Segments: one
        call without the list, then one with room; or, with seg_capacity given, one call (None when the list is longer)."""
        rcp = np.ascontiguousarray(recipients, dtype=np.uint32).reshape(-1)
        mk, mp = _mask_ptr(donors, self.n_hap)
        w = None if windows is None else make_windows(windows)
        csw = None if site_switch_cost is None else np.ascontiguousarray(site_switch_cost, dtype=np.uint32).reshape(-1)
        grp = None if group is None else np.ascontiguousarray(group, dtype=np.uint32).reshape(-1)
        pan = None if panel is None else np.ascontiguousarray(panel, dtype=np.uint8).reshape(-1)
        for name, a in (("group", grp), ("panel", pan)):
            if a is not None and len(a) != self.n_hap:
                raise ValueError(f"{name} needs one entry per haplotype ({self.n_hap}), got {len(a)}")
        prm = PaintParams(C.sizeof(PaintParams), int(mismatch_cost), int(switch_cost), int(n_panels), int(site_begin),
                          0 if site_end is None else int(site_end), None if csw is None else csw.ctypes.data_as(C.POINTER(C.c_uint32)),
                          0 if csw is None else len(csw), None if grp is None else grp.ctypes.data_as(C.POINTER(C.c_uint32)),
                          None if pan is None else pan.ctypes.data_as(C.POINTER(C.c_uint8)), int(max_chunk_bytes))
        n_rec = len(rcp)
        rec = np.zeros(n_rec, dtype=PAINT_RECIPIENT_DTYPE)
        cc = np.zeros((n_rec, self.n_hap), dtype=np.uint32) if want_chunks else None
        cs = np.zeros((n_rec, self.n_hap), dtype=np.uint64) if want_chunks else None
        win = None if w is None else np.zeros(len(w), dtype=PAINT_WINDOW_DTYPE)
        anc = np.zeros((len(w), n_rec, int(n_panels) + 1), dtype=np.uint32) if w is not None and want_ancestry else None
        total = C.c_uint64(0)

        def call(seg, cap):
            check(self.ctx._lib.impop_paint_scan(self.ctx.handle, self.handle, mp, rcp.ctypes.data_as(C.POINTER(C.c_uint32)), n_rec,
                                                 None if w is None else w.ctypes.data_as(C.POINTER(Window)), 0 if w is None else len(w),
                                                 C.byref(prm), rec.ctypes.data_as(C.POINTER(PaintRecipient)),
                                                 None if seg is None else seg.ctypes.data_as(C.POINTER(PaintSegment)), cap, C.byref(total),
                                                 None if cc is None else cc.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                 None if cs is None else cs.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                 None if win is None else win.ctypes.data_as(C.POINTER(PaintWindow)),
                                                 None if anc is None else anc.ctypes.data_as(C.POINTER(C.c_uint32))))

        seg = None
        if not want_segments:
            call(None, 0)
        elif seg_capacity is not None:
            seg = np.zeros(int(seg_capacity), dtype=PAINT_SEGMENT_DTYPE)
            call(seg, len(seg))
            seg = seg[:total.value] if total.value <= len(seg) else None
        else:
            # every path has at most one segment per stored site; a first guess of 64 per recipient usually holds
            seg = np.zeros(max(64 * n_rec, 1), dtype=PAINT_SEGMENT_DTYPE)
            call(seg, len(seg))
            if total.value > len(seg):
                seg = np.zeros(total.value, dtype=PAINT_SEGMENT_DTYPE)
                call(seg, len(seg))
            seg = seg[:total.value]
        return dict(recipients=rec, segments=seg, n_segments=int(total.value), chunk_counts=cc, chunk_sites=cs, windows=win, anc=anc)

    def ihs_scan(self, mask_a=None, mask_b=None, site_begin: int = 0, site_end: Optional[int] = None, core_begin: Optional[int] = None,
                 core_end: Optional[int] = None, min_mac: int = 1, cutoff_milli: int = 50, max_extend_bp: int = 0, max_extend_sites: int = 0,
                 capacity: Optional[int] = None):
        """Integrated haplotype homozygosity per core site (impop_ihs_scan): one population (mask_a, None = all haplotypes; classes
        by allele: iHS, nSL) or two (mask_a, mask_b; classes by population: XP-EHH, XP-nSL).  Stepped sites are those of
        [site_begin, site_end) that vary in the population(s); cores those inside [core_begin, core_end) (None = the site range)
        with a minor-allele count of at least min_mac.  -> records (IHS_DTYPE, exact integers; impop_amd.ihs.ihs_values and
        standardize make the scores).  One counting call, then one filling call; with capacity given, one call with room for that
        many (-> None, and the count, when there are more cores: see n_cores of the returned tuple).
        -> (records or None, number of cores)."""
        ma, pa = _mask_ptr(mask_a, self.n_hap)
        mb, pb = _mask_ptr(mask_b, self.n_hap)
        se = 0 if site_end is None else int(site_end)
        kb = int(site_begin) if core_begin is None else int(core_begin)
        ke = 0 if core_end is None else int(core_end)  # 0: the site range's end, as in the ABI
        prm = IhsParams(C.sizeof(IhsParams), int(min_mac), int(cutoff_milli), 0, int(max_extend_bp), int(max_extend_sites))
        total = C.c_uint64(0)

        def call(rec):
            check(self.ctx._lib.impop_ihs_scan(self.ctx.handle, self.handle, int(site_begin), se, kb, ke, pa, pb, C.byref(prm),
                                               None if rec is None else rec.ctypes.data_as(C.POINTER(IhsCore)),
                                               0 if rec is None else len(rec), C.byref(total)))

        if capacity is not None:
            rec = np.zeros(int(capacity), dtype=IHS_DTYPE)
            call(rec if len(rec) else None)
            return (rec[:total.value] if total.value <= len(rec) else None), int(total.value)
        call(None)
        rec = np.zeros(total.value, dtype=IHS_DTYPE)
        if total.value:
            call(rec)
        return rec, int(total.value)

    def dstat_scan(self, windows, pops, quartets, polarize: bool = False, tile_blocks: int = 0) -> np.ndarray:
        """Patterson's D (ABBA-BABA), f4 and Martin's f_d per window and quartet (impop_dstat_scan): pops = 4..8 masks, quartets =
        rows (P1, P2, P3, O) of indices into pops, the four populations of a row pairwise disjoint.  polarize: the outgroup's major
        allele is ancestral, per site and quartet.  -> records [n_windows, n_quartets] (DSTAT_DTYPE: the exact integers abba, baba,
        f4_num, fd_den_p2, fd_den_p3 and the doubles d, f4, fd formed from them)."""
        w = make_windows(windows)
        K = len(pops)
        packed = np.concatenate([_mask_ptr(p, self.n_hap)[0] for p in pops]).astype(np.uint64) if K else np.zeros(1, np.uint64)
        qa = np.asarray(quartets, dtype=np.int64)
        if qa.size and (qa.ndim != 2 or qa.shape[1] != 4):
            raise ValueError("quartets must be rows (P1, P2, P3, O) of population indices")
        if qa.size and (qa.min() < 0 or qa.max() > 0xFFFFFFFF):
            raise ValueError("population index outside 0 .. 2^32 - 1")
        qa = np.ascontiguousarray(qa.reshape(-1, 4), dtype=np.uint32)
        out = np.zeros((len(w), len(qa)), dtype=DSTAT_DTYPE)
        prm = DstatParams(C.sizeof(DstatParams), 1 if polarize else 0, int(tile_blocks), 0)
        check(self.ctx._lib.impop_dstat_scan(self.ctx.handle, self.handle, w.ctypes.data_as(C.POINTER(Window)), len(w),
                                             packed.ctypes.data_as(C.POINTER(C.c_uint64)), K, qa.ctypes.data_as(C.POINTER(C.c_uint32)),
                                             len(qa), C.byref(prm), out.ctypes.data_as(C.POINTER(DstatStats))))
        return out

    def sfs_scan(self, windows, pops, pairs=(), outgroup=None, tables=(), tile_blocks: int = 0, max_chunk_bytes: int = 0):
        """What is read from the site-frequency spectrum, per window (impop_sfs_scan): pops = 1..8 masks, pairs = rows (a, b) of
        indices into pops (the two populations of a row disjoint), outgroup = the index of the population whose major allele is
        ancestral, or None (counts as stored), tables = any of "sfs" (the 1-D spectra) and "jsfs" (the pairs' joint spectra).
        -> (stats [n_windows, K] (SFS_DTYPE), pair records [n_windows, P] (SFS_PAIR_DTYPE), sfs, jsfs): sfs = None or a list of K
        uint32 arrays [n_windows, n_k + 1], jsfs = None or a list of P arrays [n_windows, n_a + 1, n_b + 1]."""
        w = make_windows(windows)
        K = len(pops)
        cols = [_mask_ptr(p, self.n_hap)[0] for p in pops]
        packed = np.concatenate(cols).astype(np.uint64) if K else np.zeros(1, np.uint64)
        pa = np.asarray(pairs, dtype=np.int64)
        if pa.size and (pa.ndim != 2 or pa.shape[1] != 2):
            raise ValueError("pairs must be rows (a, b) of population indices")
        if pa.size and (pa.min() < 0 or pa.max() > 0xFFFFFFFF):
            raise ValueError("population index outside 0 .. 2^32 - 1")
        pa = np.ascontiguousarray(pa.reshape(-1, 2), dtype=np.uint32)
        tables = (tables,) if isinstance(tables, str) else tuple(tables)
        for t in tables:
            if t not in ("sfs", "jsfs"):
                raise ValueError(f"unknown table {t!r}: 'sfs' or 'jsfs'")
        bits = (_lib.SFS_TABLE_1D if "sfs" in tables else 0) | (_lib.SFS_TABLE_JOINT if "jsfs" in tables else 0)
        og = -1 if outgroup is None else int(outgroup)
        if og < -1 or og > 0x7FFFFFFF:
            raise ValueError("outgroup must be a population index or None")
        nk = [int(sum(bin(int(x)).count("1") for x in c)) for c in cols]
        stats = np.zeros((len(w), K), dtype=SFS_DTYPE)
        prec = np.zeros((len(w), len(pa)), dtype=SFS_PAIR_DTYPE)
        ok = all(int(x) < K for x in pa.ravel())  # the library refuses the call otherwise: no table is sized from a bad index
        sfs_len = sum(n + 1 for n in nk)
        jsfs_len = sum((nk[a] + 1) * (nk[b] + 1) for a, b in pa.tolist()) if ok else 0
        sfs = np.zeros((len(w), sfs_len), dtype=np.uint32) if bits & 1 else None
        jsfs = np.zeros((len(w), jsfs_len), dtype=np.uint32) if bits & 2 else None
        prm = SfsParams(C.sizeof(SfsParams), og, int(tile_blocks), bits, int(max_chunk_bytes))
        u32 = C.POINTER(C.c_uint32)
        check(self.ctx._lib.impop_sfs_scan(self.ctx.handle, self.handle, w.ctypes.data_as(C.POINTER(Window)), len(w),
                                           packed.ctypes.data_as(C.POINTER(C.c_uint64)), K, pa.ctypes.data_as(u32) if len(pa) else None,
                                           len(pa), C.byref(prm), stats.ctypes.data_as(C.POINTER(SfsStats)),
                                           prec.ctypes.data_as(C.POINTER(SfsPair)) if len(pa) else None,
                                           sfs.ctypes.data_as(u32) if sfs is not None else None,
                                           jsfs.ctypes.data_as(u32) if jsfs is not None else None))
        sfs_list = jsfs_list = None
        if sfs is not None:
            off = np.concatenate([[0], np.cumsum([n + 1 for n in nk])])
            sfs_list = [sfs[:, off[k]:off[k + 1]] for k in range(K)]
        if jsfs is not None:
            jsfs_list, o = [], 0
            for a, b in pa.tolist():
                cells = (nk[a] + 1) * (nk[b] + 1)
                jsfs_list.append(jsfs[:, o:o + cells].reshape(len(w), nk[a] + 1, nk[b] + 1))
                o += cells
        return stats, prec, sfs_list, jsfs_list

    def ehh_scan(self, windows, cores, mask=None, ref_hap: int = 0, flanks: str = "reference", max_chunk_bytes: int = 0) -> np.ndarray:
        """Integrated EHH per core site (impop_ehh_scan; the area of scripts/wip/ehhgfa.py:63) for a batch of windows:
        windows = (site_begin, site_end) rows, cores = one site per window inside it.  For the members of `mask` carrying
        allele a at the core, area_milli[a][h] = sum over the half's sites of 1000 * EHH, exact; flanks 'reference' takes both
        halves from (core, end) like ehhgfa.py:56-61, 'two-sided' half 0 from [begin, core) walking away from the core.
        -> records (EHH_DTYPE)."""
        wv = np.asarray(windows)
        cv = np.asarray(cores, dtype=np.int64).ravel()
        if wv.dtype.names:
            be = np.stack([wv["site_begin"], wv["site_end"]], axis=1)
        else:
            be = wv.reshape(-1, wv.shape[-1] if wv.ndim > 1 else 2)[:, :2] if wv.size else np.zeros((0, 2), np.int64)
        if len(be) != len(cv):
            raise ValueError(f"{len(be)} windows but {len(cv)} cores")
        if len(be) and (np.asarray(be).astype(np.int64).min() < 0 or cv.min() < 0):
            raise ValueError("negative site index")
        w = np.zeros(len(be), dtype=EHH_WINDOW_DTYPE)
        w["site_begin"], w["site_end"], w["core_site"] = be[:, 0], be[:, 1], cv
        out = np.zeros(len(w), dtype=EHH_DTYPE)
        prm = EhhParams(C.sizeof(EhhParams), EHH_FLANKS[flanks], int(ref_hap), 0, int(max_chunk_bytes))
        keep, ptr = _mask_ptr(mask, self.n_hap)
        check(self.ctx._lib.impop_ehh_scan(self.ctx.handle, self.handle, w.ctypes.data_as(C.POINTER(EhhWindow)), len(w), ptr,
                                           C.byref(prm), out.ctypes.data_as(C.POINTER(EhhStats))))
        return out


class Genotypes:
    """Per-individual genotype planes H = h1 ^ h2 and A = h1 & h2 resident in HBM (impop_genotypes)."""

    def __init__(self, ctx: Context, handle):
        self.ctx = ctx
        self._h = handle
        n, s, b = C.c_uint32(), C.c_uint64(), C.c_uint64()
        check(ctx._lib.impop_genotypes_info(handle, C.byref(n), C.byref(s), C.byref(b)))
        self.n_ind, self.n_site, self.device_bytes = n.value, s.value, b.value

    @property
    def handle(self):
        if not self._h:
            raise ImpopError(_lib.E_INVALID, "genotypes are freed")
        return self._h

    def free(self) -> None:
        if self._h:
            check(self.ctx._lib.impop_genotypes_free(self.ctx.handle if self.ctx._h else None, self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def download(self, site_begin: int = 0, site_end: Optional[int] = None) -> np.ndarray:
        """-> [2N, words] uint64: rows H_0 .. H_{N-1}, A_0 .. A_{N-1} of the plane sites [site_begin, site_end), bit k of a row =
        site site_begin + k."""
        site_end = self.n_site if site_end is None else site_end
        words = max((site_end - site_begin + 63) // 64, 1)
        out = np.zeros((2 * self.n_ind, words), dtype=np.uint64)
        check(self.ctx._lib.impop_genotypes_download(self.ctx.handle, self.handle, int(site_begin), int(site_end),
                                                     out.ctypes.data_as(C.POINTER(C.c_uint64)), words))
        return out

    def kinship_scan(self, windows, kin=(884, 10000), watch=None, want_pairs: bool = True):
        """Joint genotype tables and KING kinship of every pair of individuals per window (impop_kinship_scan).  kin = (num, den):
        a pair is related in a window when its KING-robust kinship is at least num / den.  watch: [n_watch, 2] individual indices.
        -> (windows KIN_WINDOW_DTYPE [n_windows], pairs KIN_PAIR_DTYPE [N(N-1)/2] summed over the windows, in the pair order of
        scan_multi, or None, watch rows KIN_WATCH_DTYPE [n_windows, n_watch] or None)."""
        w = make_windows(windows)
        N = self.n_ind
        wa = np.zeros((0, 2), np.uint32) if watch is None else np.asarray(watch)
        if wa.size and (wa.ndim != 2 or wa.shape[1] != 2):
            raise ValueError("watch must be [n_watch, 2] individual indices")
        if wa.size and (wa.min() < 0 or wa.max() > 0xFFFFFFFF):
            raise ValueError("individual index outside 0 .. 2^32 - 1")
        wa = np.ascontiguousarray(wa.reshape(-1, 2), dtype=np.uint32)
        nw = len(wa)
        out = np.zeros(len(w), dtype=KIN_WINDOW_DTYPE)
        pairs = np.zeros(N * (N - 1) // 2, dtype=KIN_PAIR_DTYPE) if want_pairs else None
        rows = np.zeros((len(w), nw), dtype=KIN_WATCH_DTYPE) if nw else None
        prm = _lib.KinshipParams(C.sizeof(_lib.KinshipParams), int(kin[0]), int(kin[1]), 0)
        check(self.ctx._lib.impop_kinship_scan(self.ctx.handle, self.handle, w.ctypes.data_as(C.POINTER(Window)), len(w), C.byref(prm),
                                               wa.ctypes.data_as(C.POINTER(C.c_uint32)) if nw else None, nw,
                                               out.ctypes.data_as(C.POINTER(_lib.KinWindow)),
                                               pairs.ctypes.data_as(C.POINTER(_lib.KinPair)) if want_pairs else None,
                                               rows.ctypes.data_as(C.POINTER(_lib.KinWatch)) if nw else None))
        return out, pairs, rows


class ScanPlan:
    """Pre-planned windowed scan (impop_scan_plan): tile tables live on the device, so
    launch() is two kernel launches with no host synchronisation."""

    def __init__(self, matrix: BitMatrix, windows: np.ndarray, mask_p, mask_a, mask_b, d_pi_mode, s_scope, tile_blocks):
        self.matrix = matrix
        self.windows = windows
        lib = matrix.ctx._lib
        prm = ScanParams(C.sizeof(ScanParams), int(d_pi_mode), int(s_scope), int(tile_blocks))
        kp, pp = _mask_ptr(mask_p, matrix.n_hap)
        ka, pa = _mask_ptr(mask_a, matrix.n_hap)
        kb, pb = _mask_ptr(mask_b, matrix.n_hap)
        self._h = C.c_void_p()
        check(lib.impop_scan_plan_create(matrix.ctx.handle, matrix.handle, windows.ctypes.data_as(C.POINTER(Window)),
                                         len(windows), pp, pa, pb, C.byref(prm), C.byref(self._h)))
        t, b = C.c_uint64(), C.c_uint64()
        check(lib.impop_scan_plan_info(self._h, C.byref(t), C.byref(b)))
        self.n_tiles, self.bytes_streamed = t.value, b.value
        self.n_windows = len(windows)

    def digest_info(self) -> dict:
        """The plan's tile digest: {"on", "n_rows" (representatives over all tiles), "n_hist_tiles", "digest_bytes"} and "why"
        (the reason there is none, else "")."""
        on, r, h, b = C.c_int(), C.c_uint64(), C.c_uint64(), C.c_uint64()
        why = C.create_string_buffer(256)
        check(self.matrix.ctx._lib.impop_scan_plan_digest_info(self._h, C.byref(on), C.byref(r), C.byref(h), C.byref(b), why, len(why)))
        return {"on": bool(on.value), "n_rows": r.value, "n_hist_tiles": h.value, "digest_bytes": b.value, "why": why.value.decode()}

    def set_masks(self, mask_p=None, mask_a=None, mask_b=None) -> None:
        """Swap the subset / population masks; the tile tables (windows) are kept."""
        n = self.matrix.n_hap
        kp, pp = _mask_ptr(mask_p, n)
        ka, pa = _mask_ptr(mask_a, n)
        kb, pb = _mask_ptr(mask_b, n)
        check(self.matrix.ctx._lib.impop_scan_plan_set_masks(self._h, pp, pa, pb))

    def launch(self, d_out: Optional[int] = None) -> None:
        check(self.matrix.ctx._lib.impop_scan_plan_launch(self._h, C.c_void_p(d_out) if d_out else None))

    def fetch(self) -> np.ndarray:
        out = np.zeros(self.n_windows, dtype=STATS_DTYPE)
        check(self.matrix.ctx._lib.impop_scan_plan_fetch(self._h, out.ctypes.data_as(C.POINTER(WindowStats))))
        return out

    def timing(self, enable: bool = True) -> None:
        check(self.matrix.ctx._lib.impop_scan_plan_timing(self._h, 1 if enable else 0))

    def elapsed(self):
        """-> (summed streaming-kernel ms, launches) since timing(True)"""
        t, k = C.c_double(), C.c_uint64()
        check(self.matrix.ctx._lib.impop_scan_plan_elapsed(self._h, C.byref(t), C.byref(k)))
        return t.value, k.value

    def destroy(self) -> None:
        if self._h:
            self.matrix.ctx._lib.impop_scan_plan_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass


# ---- multi-GPU entries of the C ABI ------------------------------------------------------------------

def shard_windows_c(windows, n_shards: int, shard: int):
    """impop_shard_windows -> (first_window, n_windows, slab_begin, slab_end)"""
    w = make_windows(windows)
    out = [C.c_uint64() for _ in range(4)]
    check(_lib.load().impop_shard_windows(w.ctypes.data_as(C.POINTER(Window)), len(w), int(n_shards), int(shard),
                                          *[C.byref(x) for x in out]))
    return tuple(int(x.value) for x in out)


def scan_sharded(slabs, slab_site_begin, windows, mask_p=None, mask_a=None, mask_b=None, d_pi_mode: int = 0, s_scope: int = 0,
                 tile_blocks: int = 0) -> np.ndarray:
    """One process, several contexts (impop_scan_sharded): slabs[k] is a BitMatrix resident on its own context and
    holds the sites [slab_site_begin[k], ...) of the chromosome; `windows` in chromosome coordinates.  Returns the
    records in the order of `windows`."""
    lib = _lib.load()
    w = make_windows(windows)
    n = len(slabs)
    n_hap = slabs[0].n_hap
    ctxs = (C.c_void_p * n)(*[s.ctx.handle for s in slabs])
    mats = (C.c_void_p * n)(*[s.handle for s in slabs])
    begins = np.ascontiguousarray(slab_site_begin, dtype=np.uint64)
    prm = ScanParams(C.sizeof(ScanParams), int(d_pi_mode), int(s_scope), int(tile_blocks))
    kp, pp = _mask_ptr(mask_p, n_hap)
    ka, pa = _mask_ptr(mask_a, n_hap)
    kb, pb = _mask_ptr(mask_b, n_hap)
    out = np.zeros(len(w), dtype=STATS_DTYPE)
    check(lib.impop_scan_sharded(ctxs, mats, begins.ctypes.data_as(C.POINTER(C.c_uint64)), n,
                                 w.ctypes.data_as(C.POINTER(Window)), len(w), pp, pa, pb, C.byref(prm),
                                 out.ctypes.data_as(C.POINTER(WindowStats))))
    return out


def pairwise_scan_sharded(slabs, slab_site_begin, windows, mask_p=None, mask_a=None, mask_b=None, kind: str = "match",
                          threshold: float = 0.99, round_digits: Optional[int] = None, d_pi_mode: int = 0, s_scope: int = 0,
                          fst_method: str = "direct") -> np.ndarray:
    """The all-pairs mode over several contexts (impop_pairwise_scan_sharded): like scan_sharded, with
    BitMatrix.pairwise_scan's parameters; every slab needs its hap-major operand (keep_hap_major=True)."""
    lib = _lib.load()
    w = make_windows(windows)
    n = len(slabs)
    n_hap = slabs[0].n_hap
    ctxs = (C.c_void_p * n)(*[s.ctx.handle for s in slabs])
    mats = (C.c_void_p * n)(*[s.handle for s in slabs])
    begins = np.ascontiguousarray(slab_site_begin, dtype=np.uint64)
    prm = PairwiseParams(C.sizeof(PairwiseParams), IDENTITY_KINDS[kind], float(threshold),
                         -1 if round_digits is None else int(round_digits), int(d_pi_mode), int(s_scope),
                         {"direct": 0, "grouped": 1}[fst_method])
    kp, pp = _mask_ptr(mask_p, n_hap)
    ka, pa = _mask_ptr(mask_a, n_hap)
    kb, pb = _mask_ptr(mask_b, n_hap)
    out = np.zeros(len(w), dtype=PAIRWISE_DTYPE)
    check(lib.impop_pairwise_scan_sharded(ctxs, mats, begins.ctypes.data_as(C.POINTER(C.c_uint64)), n,
                                          w.ctypes.data_as(C.POINTER(Window)), len(w), pp, pa, pb, C.byref(prm),
                                          out.ctypes.data_as(C.POINTER(PairwiseStats))))
    return out


def _preload_torch_rccl() -> None:
    """One RCCL per process: if PyTorch-ROCm is installed, load ITS librccl (soname librccl.so.1) first, by path,
    so that the library's dlopen("librccl.so.1") and a later `import torch` bind to the same copy."""
    import importlib.util
    import os
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec and spec.submodule_search_locations:
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "librccl.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)


class Comm:
    """One process per GPU: an RCCL communicator bound to a Context (impop_comm).  Rank 0 makes the id with
    Comm.unique_id() and ships the 128 bytes to the other ranks out of band."""

    ID_BYTES = 128

    @staticmethod
    def unique_id() -> bytes:
        _preload_torch_rccl()
        buf = C.create_string_buffer(Comm.ID_BYTES)
        check(_lib.load().impop_comm_unique_id(buf))
        return buf.raw

    def __init__(self, ctx: Context, unique_id: bytes, world: int, rank: int):
        if len(unique_id) != Comm.ID_BYTES:
            raise ValueError("unique_id must be 128 bytes")
        _preload_torch_rccl()
        self.ctx, self.world, self.rank = ctx, int(world), int(rank)
        self._h = C.c_void_p()
        check(ctx._lib.impop_comm_create(ctx.handle, unique_id, int(world), int(rank), C.byref(self._h)))

    def gather(self, d_local: int, bytes_per_rank: int, d_all: int) -> None:
        """ncclAllGather on the context's stream (device pointers, no host sync)."""
        check(self.ctx._lib.impop_gather(self._h, C.c_void_p(d_local), int(bytes_per_rank), C.c_void_p(d_all)))

    def gather_records(self, plan: "ScanPlan", n_total_windows: int) -> np.ndarray:
        """All-gather the records of `plan` (this rank's shard of n_total_windows) -> every window, global order."""
        d = C.c_void_p()
        check(self.ctx._lib.impop_scan_plan_device_records(plan._h, C.byref(d)))
        out = np.zeros(int(n_total_windows), dtype=STATS_DTYPE)
        check(self.ctx._lib.impop_gather_records(self._h, d, int(n_total_windows), out.ctypes.data_as(C.POINTER(WindowStats))))
        return out

    def allreduce_i64(self, d_values: int, count: int) -> None:
        check(self.ctx._lib.impop_allreduce_i64(self._h, C.c_void_p(d_values), int(count)))

    def close(self) -> None:
        if self._h:
            self.ctx._lib.impop_comm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
