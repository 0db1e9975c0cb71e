"""impop_amd — MI355X-native windowed population statistics (pi, Hudson Fst, Tajima's D,
haplotype-cluster frequencies) for the pairwise-diversity hot path of pangenome/impop.

Hand-written HIP for gfx950 behind a C ABI (include/impop_hip.h, libimpop_hip.so); this
package is the thin ctypes host layer that mirrors the reference's Python interfaces.
There is no CPU fallback: without the built library and a gfx950 GPU every compute
entry point raises ImpopError.
"""
from ._lib import ImpopError, SO_PATH  # noqa: F401
from . import distributed  # noqa: F401
from . import ldband  # noqa: F401
from . import paint  # noqa: F401
from . import recomb  # noqa: F401
from . import tree  # noqa: F401
from .tree import cut, heights, rf_distance, to_newick  # noqa: F401
from .engine import (Comm, pairwise_scan_sharded, scan_sharded, shard_windows_c,  # noqa: F401
                     BitMatrix, Context, Genotypes, ScanPlan, KIN_WINDOW_DTYPE, KIN_PAIR_DTYPE, KIN_WATCH_DTYPE, STATS_DTYPE, PAIRWISE_DTYPE, CLUSTER_DTYPE, HAPLOTYPE_DTYPE, LD_DTYPE, RECOMB_DTYPE, RECOMB_SITE_DTYPE, LDBAND_DTYPE, LDBAND_BIN_DTYPE, LDBAND_SITE_DTYPE, DIPLOID_DTYPE, DIPLOID_IND_DTYPE, IBS_PAIR_DTYPE, IBS_SEGMENT_DTYPE, IBS_WINDOW_DTYPE, IBD_PAIR_DTYPE, IBD_SEGMENT_DTYPE, PAINT_RECIPIENT_DTYPE, PAINT_SEGMENT_DTYPE, PAINT_WINDOW_DTYPE, IHS_DTYPE, DSTAT_DTYPE, SFS_DTYPE, SFS_PAIR_DTYPE, EHH_DTYPE, PANEL_DTYPE, PANEL_WINDOW_DTYPE, PAIR_DTYPE, DIST_PANEL_DTYPE, DIST_PAIR_DTYPE, PCA_WINDOW_DTYPE, TREE_WINDOW_DTYPE, TREE_MERGE_DTYPE, TREE_PANEL_DTYPE, PERM_PAIR_DTYPE, PERM_NULL_DTYPE, WINDOW_DTYPE, permtest_labels, fixed_windows,  # noqa: F401
                     make_windows, mask_from_indices, pack_hap_major, pack_mask, unpack_hap_major)

__version__ = "0.1.0"
