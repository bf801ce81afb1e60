"""ctypes binding of the C ABI declared in include/v2m_hip.h.

The HIP library is the only implementation: if libv2m_hip.so is missing this module raises,
it never substitutes a CPU path.
"""

import ctypes as C
import os

from . import build as _build

_u64p = C.POINTER(C.c_uint64)

V2M_OK = 0
ERROR_NAMES = {
	1: "V2M_ERR_INVALID_ARGUMENT", 2: "V2M_ERR_PRECONDITION", 3: "V2M_ERR_UNSUPPORTED", 4: "V2M_ERR_NO_DEVICE",
	5: "V2M_ERR_HIP", 6: "V2M_ERR_OUT_OF_MEMORY", 7: "V2M_ERR_SINK", 8: "V2M_ERR_STATE",
}
V2M_ERR_INVALID_ARGUMENT, V2M_ERR_PRECONDITION, V2M_ERR_UNSUPPORTED, V2M_ERR_NO_DEVICE = 1, 2, 3, 4
V2M_ERR_HIP, V2M_ERR_OUT_OF_MEMORY, V2M_ERR_SINK, V2M_ERR_STATE = 5, 6, 7, 8
V2M_PLOIDY_MAX = 0xFFFFFFFF
V2M_SPLICE_UNALIGNED = 0x1
V2M_SPLICE_BGZF = 0x2

KERNEL_TRANSPOSE, KERNEL_RESOLVE, KERNEL_SPLICE_ALIGNED, KERNEL_SPLICE_UNALIGNED, KERNEL_TEMPLATE, KERNEL_UNALIGNED_COUNT = range(6)
KERNEL_BGZF = 6
KERNEL_INFLATE = 7
KERNEL_VCF = 8
KERNEL_ROW_OPS_COUNT, KERNEL_ROW_OPS_SCAN, KERNEL_ROW_OPS_EMIT = 9, 10, 11   # the passes of v2m_row_ops
KERNEL_DISTINCT_HASH, KERNEL_DISTINCT_GATHER, KERNEL_DISTINCT_VERIFY = 12, 13, 14   # the kernels of v2m_splice_window_set_distinct
KERNEL_NAMES = ["transpose_bits_kernel", "resolve_effective_edges_kernel", "splice_aligned_kernel", "splice_unaligned_kernel", "expand_reference_row_kernel", "count_unaligned_kernel",
	"bgzf_deflate_kernel", "bgzf_inflate_kernel", "vcf_scan_kernels", "count_row_ops_kernel", "scan_row_ops_kernel", "emit_row_ops_kernel",
	"hash_pieces_kernel", "gather_pieces_kernel", "verify_pieces_kernel"]
# the passes of v2m_column_counts[_device], behind V2M_KERNEL_END (KERNEL_NAMES keeps the ids below it; KERNEL_LIMIT bounds profile_get)
KERNEL_COLUMN_COUNTS, KERNEL_COLUMN_SELECT, KERNEL_LIMIT = 15, 16, 17
COLUMN_KERNEL_NAMES = {KERNEL_COLUMN_COUNTS: "column_counts_kernel", KERNEL_COLUMN_SELECT: "emit_column_counts_kernel"}
COUNT_CLASSES = 6                # v2m_column_count.count: A, C, G, T, N, gap ("other" is n_rows minus their sum)
COUNTS_VARIABLE_ONLY = 0x8       # v2m_column_counts flag: only the columns no class holds all rows of
COUNTS_ACCUMULATE = 0x10         # v2m_column_counts_device flag: add to the table instead of overwriting it
# csrc/kernels.hpp: kCountColumns (columns per workgroup of column_counts_kernel), kCountRun (rows between two flushes of its byte
# lanes), kSelectColumns (columns per workgroup of the selection); csrc/v2m_hip.hip: kColumnCountsMinRows (the least rows of a row group)
COUNT_COLUMNS = 4096
COUNT_RUN = 255
SELECT_COLUMNS = 256
COLUMN_COUNTS_MIN_ROWS = 32
# v2m_pair_distances[_device]: the one flag, the row limit, and csrc/distance_kernels.hpp's kPairTile (rows per side of a workgroup's
# tile) and kPairChunkWords (64-bit site words per LDS chunk); tests/test_pair_distances_host.py holds them to the sources
DIST_ACGT_ONLY = 0x20
PAIR_DISTANCES_MAX_ROWS = 32768
PAIR_TILE = 64
PAIR_CHUNK_WORDS = 8
# v2m_variable_sites[_device]: the one flag, and csrc/site_kernels.hpp's kGatherSites (sites a lane owns), kGatherThreads (lanes of a
# workgroup) and kGatherMinGroupRows (the fewest rows of a row group); tests/test_variable_sites_host.py holds them to the sources
SITES_SNP = 0x40
GATHER_SITES = 4
GATHER_THREADS = 256
GATHER_MIN_GROUP_ROWS = 16
# v2m_site_ld[_device]: the limits, and csrc/ld_kernels.hpp's kLdTile (sites per side of a workgroup's tile) and kLdChunkWords (64-row
# words per LDS chunk); tests/test_site_ld_host.py holds them to the sources
SITE_LD_MAX_WINDOW = 4096
SITE_LD_MAX_ROWS = 32768
LD_TILE = 64
LD_CHUNK_WORDS = 8
# v2m_nj_tree[_of_distances]: the id that is none, the limit, and csrc/nj_kernels.hpp's kNjRowsPerGroup (rows per workgroup of
# nj_rowmin_kernel), kNjJoinThreads (nj_join_kernel's one workgroup) and kNjJoinBatch (the live slots a lane of it has in flight);
# tests/test_nj_tree_host.py holds them to the sources
NJ_NONE = 0xFFFFFFFF
NJ_MAX_ROWS = 32768
NJ_ROWS_PER_GROUP = 8
NJ_JOIN_THREADS = 256
NJ_JOIN_BATCH = 4
# v2m_pair_distances_weighted, v2m_bootstrap_distances, v2m_nj_bootstrap: the limit, and csrc/bootstrap_kernels.hpp's kBootDrawThreads
# (draws per workgroup of bootstrap_weights_kernel) and kBootSlices (bit slices of a weight); tests/test_nj_bootstrap_host.py holds them
# to the sources
NJ_BOOTSTRAP_MAX_REPLICATES = 100000
BOOT_DRAW_THREADS = 256
BOOT_SLICES = 32
# v2m_parsimony_of_sites, v2m_tree_parsimony: csrc/parsimony_kernels.hpp's kFitchSites (sites a lane owns), kFitchThreads (lanes of a
# workgroup) and kFitchBatch (records whose leaf rows a lane reads ahead); tests/test_tree_parsimony_host.py holds them to the sources
FITCH_SITES = 4
FITCH_THREADS = 256
FITCH_BATCH = 4
# v2m_diversity_of_counts, v2m_window_diversity: the limit, and csrc/diversity_kernels.hpp's kDiversityColumns (columns of a workgroup's
# tile) and kDiversitySfsLdsBins (entries of the spectrum's on-chip histogram); tests/test_window_diversity_host.py holds them to the sources
DIVERSITY_MAX_ROWS = 32768
DIVERSITY_COLUMNS = 1024
DIVERSITY_SFS_LDS_BINS = 4096
# csrc/kernels.hpp: kDistinctChunkBytes (a long piece is hashed, gathered and verified in chunks of this many bytes) and
# kDistinctLongBytes (windows longer than this are hashed in chunks); tests/test_distinct_model_host.py holds them to the source
DISTINCT_CHUNK_BYTES = 8192
DISTINCT_LONG_BYTES = 16384
OP_M, OP_I, OP_D = 0, 1, 2   # v2m_aln_op.op (BAM's codes)
OP_EQ, OP_X = 7, 8           # with OPS_SPLIT_MATCH, in place of OP_M
OPS_SPLIT_MATCH = 0x4        # v2m_row_ops flag: M split into = and X (letters compare without case)
ABI_VERSION = 5


class GraphView(C.Structure):
	_fields_ = [
		("node_count", C.c_uint64), ("edge_count", C.c_uint64),
		("reference_positions", C.c_void_p), ("aligned_positions", C.c_void_p),
		("alt_edge_targets", C.c_void_p), ("alt_edge_count_csum", C.c_void_p),
		("alt_edge_label_offsets", C.c_void_p), ("alt_edge_label_bytes", C.c_void_p),
		("paths_by_chrom_copy_and_edge", C.c_void_p), ("path_rows", C.c_uint64), ("path_cols", C.c_uint64),
	]


class RowBatchStruct(C.Structure):
	_fields_ = [
		("n_rows", C.c_uint64), ("copy_index", C.c_void_p), ("cut_offsets", C.c_void_p),
		("cut_nodes", C.c_void_p), ("cut_copies", C.c_void_p),
	]


class VcfLine(C.Structure):
	"""v2m_vcf_line"""
	_fields_ = [("kind", C.c_uint32), ("n_alts", C.c_uint32), ("head_offset", C.c_uint32), ("head_length", C.c_uint32), ("column_begin", C.c_uint64)]


class VcfLayout(C.Structure):
	"""v2m_vcf_layout"""
	_fields_ = [("n_samples", C.c_uint32), ("n_rows", C.c_uint32), ("words_per_column", C.c_uint64), ("copy_begin", C.c_void_p), ("row_lookup", C.c_void_p)]


class VcfChunk(C.Structure):
	"""v2m_vcf_chunk"""
	_fields_ = [("first_line", C.c_uint64), ("n_lines", C.c_uint64), ("lines", C.c_void_p), ("heads", C.c_void_p), ("head_bytes", C.c_uint64),
		("columns", C.c_void_p), ("n_columns", C.c_uint64), ("words_per_column", C.c_uint64)]


VCF_LAYOUT_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(VcfLayout))   # v2m_vcf_layout_fn
VCF_CHUNK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.POINTER(VcfChunk))   # v2m_vcf_chunk_fn
VCF_LINE_DTYPE = [("kind", "<u4"), ("n_alts", "<u4"), ("head_offset", "<u4"), ("head_length", "<u4"), ("column_begin", "<u8")]

SINK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64)
HOLD_SINK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p)   # v2m_hold_sink_fn
WINDOW_SINK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.POINTER(C.c_uint32))   # v2m_window_sink_fn
DISTINCT_SINK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64)   # v2m_distinct_sink_fn
OPS_SINK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64)   # v2m_ops_sink_fn
COLUMN_COUNT_DTYPE = [("column", "<u8"), ("count", "<u4", (6,))]   # v2m_column_count
COLUMN_COUNTS_SINK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64)   # v2m_column_counts_sink_fn


class PairDistancesInfo(C.Structure):   # v2m_pair_distances_info
	_fields_ = [("n_sites", C.c_uint64), ("n_columns", C.c_uint64), ("n_passes", C.c_uint64), ("counts_ms", C.c_double), ("pack_ms", C.c_double), ("pairs_ms", C.c_double)]

class VariableSitesInfo(C.Structure):   # v2m_variable_sites_info
	_fields_ = [("n_sites", C.c_uint64), ("n_columns", C.c_uint64), ("counts_ms", C.c_double), ("gather_ms", C.c_double)]


class SiteLdParams(C.Structure):   # v2m_site_ld_params
	_fields_ = [("window_sites", C.c_uint32), ("min_allele_count", C.c_uint32), ("min_r2_num", C.c_uint32), ("min_r2_den", C.c_uint32), ("window_columns", C.c_uint64)]

class SiteLdInfo(C.Structure):   # v2m_site_ld_info
	_fields_ = [("n_sites", C.c_uint64), ("n_columns", C.c_uint64), ("n_pairs", C.c_uint64), ("n_candidates", C.c_uint64),
		("counts_ms", C.c_double), ("pack_ms", C.c_double), ("pairs_ms", C.c_double)]


LD_SITE_DTYPE = [("column", "<u8"), ("class_lo", "<u4"), ("class_hi", "<u4"), ("count_lo", "<u4"), ("count_hi", "<u4")]   # v2m_ld_site
LD_PAIR_DTYPE = [("site_a", "<u4"), ("site_b", "<u4"), ("n", "<u4"), ("n_a", "<u4"), ("n_b", "<u4"), ("n_ab", "<u4")]   # v2m_ld_pair
LD_SINK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64)   # v2m_ld_sites_sink_fn, v2m_ld_pairs_sink_fn


class NjTreeInfo(C.Structure):   # v2m_nj_tree_info
	_fields_ = [("n_nodes", C.c_uint64), ("n_sites", C.c_uint64), ("n_columns", C.c_uint64), ("n_passes", C.c_uint64), ("distances_ms", C.c_double), ("tree_ms", C.c_double)]


class NjBootstrapInfo(C.Structure):   # v2m_nj_bootstrap_info
	_fields_ = [("n_rows", C.c_uint64), ("n_sites", C.c_uint64), ("n_columns", C.c_uint64), ("n_passes", C.c_uint64), ("n_pack_passes", C.c_uint64),
		("n_replicates", C.c_uint64), ("max_slices", C.c_uint64), ("distances_ms", C.c_double), ("weights_ms", C.c_double), ("pairs_ms", C.c_double),
		("trees_ms", C.c_double)]


class TreeParsimonyInfo(C.Structure):   # v2m_tree_parsimony_info
	_fields_ = [("n_sites", C.c_uint64), ("n_columns", C.c_uint64), ("n_mutations", C.c_uint64), ("n_ranges", C.c_uint64),
		("counts_ms", C.c_double), ("gather_ms", C.c_double), ("parsimony_ms", C.c_double)]


class WindowDiversityInfo(C.Structure):   # v2m_window_diversity_info
	_fields_ = [("n_columns", C.c_uint64), ("n_bins", C.c_uint64), ("multiallelic", C.c_uint64), ("counts_ms", C.c_double), ("bins_ms", C.c_double)]


DIVERSITY_BIN_DTYPE = [("columns", "<u8"), ("called", "<u8"), ("diffs", "<u8"), ("pairs", "<u8"), ("segregating", "<u8"), ("complete", "<u8"),
	("complete_segregating", "<u8"), ("complete_diffs", "<u8")]   # v2m_diversity_bin
DIVERSITY_BETWEEN_BIN_DTYPE = [("columns", "<u8"), ("called", "<u8"), ("diffs", "<u8"), ("pairs", "<u8")]   # v2m_diversity_between_bin
PARSIMONY_SITE_DTYPE = [("steps", "<u4"), ("present", "<u4")]   # v2m_parsimony_site
TREE_SITE_DTYPE = [("column", "<u8"), ("steps", "<u4"), ("present", "<u4")]   # v2m_tree_site
TREE_MUTATION_DTYPE = [("site", "<u4"), ("node", "<u4"), ("from", "<u4"), ("to", "<u4")]   # v2m_tree_mutation
TREE_SINK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64)   # v2m_tree_sites_sink_fn, v2m_tree_mutations_sink_fn
NJ_NODE_DTYPE = [("a", "<u4"), ("b", "<u4"), ("c", "<u4"), ("reserved", "<u4"), ("len_a", "<f8"), ("len_b", "<f8"), ("len_c", "<f8")]   # v2m_nj_node
SITE_COLUMNS_SINK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_uint64)   # v2m_site_columns_sink_fn
SITE_ROWS_SINK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64)   # v2m_site_rows_sink_fn
TRIALS_SINK_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64)   # v2m_trials_sink

# every symbol include/v2m_hip.h declares: (restype, argtypes)
SIGNATURES = {
	"v2m_abi_version": (C.c_uint32, []),
	"v2m_ctx_create": (C.c_int, [C.c_int, C.POINTER(C.c_void_p)]),
	"v2m_ctx_destroy": (None, [C.c_void_p]),
	"v2m_last_error": (C.c_char_p, [C.c_void_p]),
	"v2m_ctx_synchronize": (C.c_int, [C.c_void_p]),
	"v2m_ctx_stream": (C.c_void_p, [C.c_void_p]),
	"v2m_ctx_info": (C.c_char_p, [C.c_void_p]),
	"v2m_transpose_bits": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
	"v2m_transpose_bits_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]),
	"v2m_upload_graph": (C.c_int, [C.c_void_p, C.POINTER(GraphView), C.c_void_p, C.c_uint64]),
	"v2m_set_paths_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
	"v2m_upload_path_slice": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]),
	"v2m_upload_path_blocks": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64]),
	"v2m_bind_path_matrix_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]),
	"v2m_aligned_length": (C.c_uint64, [C.c_void_p]),
	"v2m_min_row_pitch": (C.c_uint64, [C.c_void_p]),
	"v2m_max_unaligned_length": (C.c_uint64, [C.c_void_p]),
	"v2m_set_column_window": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64]),
	"v2m_window_length": (C.c_uint64, [C.c_void_p]),
	"v2m_window_set_layout": (C.c_int, [C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, _u64p]),
	"v2m_set_window_set": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
	"v2m_window_set_size": (C.c_uint64, [C.c_void_p]),
	"v2m_window_set_pitch": (C.c_uint64, [C.c_void_p]),
	"v2m_splice_window_set": (C.c_int, [C.c_void_p, C.POINTER(RowBatchStruct), C.c_uint32, WINDOW_SINK_FN, C.c_void_p]),
	"v2m_splice_window_set_device": (C.c_int, [C.c_void_p, C.POINTER(RowBatchStruct), C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]),
	"v2m_splice_window_set_distinct": (C.c_int, [C.c_void_p, C.POINTER(RowBatchStruct), C.c_uint32, DISTINCT_SINK_FN, C.c_void_p, C.c_void_p, C.c_void_p]),
	"v2m_splice_rows": (C.c_int, [C.c_void_p, C.POINTER(RowBatchStruct), C.c_uint32, SINK_FN, C.c_void_p]),
	"v2m_splice_rows_held": (C.c_int, [C.c_void_p, C.POINTER(RowBatchStruct), C.c_uint32, C.c_uint32, HOLD_SINK_FN, C.c_void_p]),
	"v2m_row_release": (None, [C.c_void_p]),
	"v2m_splice_rows_device": (C.c_int, [C.c_void_p, C.POINTER(RowBatchStruct), C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p]),
	"v2m_row_ops": (C.c_int, [C.c_void_p, C.POINTER(RowBatchStruct), C.c_uint32, OPS_SINK_FN, C.c_void_p]),
	"v2m_column_counts": (C.c_int, [C.c_void_p, C.POINTER(RowBatchStruct), C.c_uint32, COLUMN_COUNTS_SINK_FN, C.c_void_p]),
	"v2m_column_counts_device": (C.c_int, [C.c_void_p, C.POINTER(RowBatchStruct), C.c_uint32, C.c_void_p, C.c_uint64]),
	"v2m_pair_distances": (C.c_int, [C.c_void_p, C.POINTER(RowBatchStruct), C.c_uint32, C.c_void_p, C.POINTER(PairDistancesInfo)]),
	"v2m_pair_distances_device": (C.c_int, [C.c_void_p, C.POINTER(RowBatchStruct), C.c_uint32, C.c_void_p, C.c_uint64]),
	"v2m_variable_sites": (C.c_int, [C.c_void_p, C.POINTER(RowBatchStruct), C.c_uint32, SITE_COLUMNS_SINK_FN, SITE_ROWS_SINK_FN, C.c_void_p, C.POINTER(VariableSitesInfo)]),
	"v2m_variable_sites_device": (C.c_int, [C.c_void_p, C.POINTER(RowBatchStruct), C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]),
	"v2m_site_ld": (C.c_int, [C.c_void_p, C.POINTER(RowBatchStruct), C.POINTER(SiteLdParams), LD_SINK_FN, LD_SINK_FN, C.c_void_p, C.POINTER(SiteLdInfo)]),
	"v2m_site_ld_device": (C.c_int, [C.c_void_p, C.POINTER(RowBatchStruct), C.POINTER(SiteLdParams), C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, _u64p, _u64p]),
	"v2m_nj_tree_of_distances": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.POINTER(NjTreeInfo)]),
	"v2m_nj_tree": (C.c_int, [C.c_void_p, C.POINTER(RowBatchStruct), C.c_uint32, C.c_void_p, C.POINTER(NjTreeInfo)]),
	"v2m_pair_distances_weighted": (C.c_int, [C.c_void_p, C.POINTER(RowBatchStruct), C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(PairDistancesInfo)]),
	"v2m_bootstrap_distances": (C.c_int, [C.c_void_p, C.POINTER(RowBatchStruct), C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p, C.POINTER(PairDistancesInfo)]),
	"v2m_nj_bootstrap": (C.c_int, [C.c_void_p, C.POINTER(RowBatchStruct), C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NjBootstrapInfo)]),
	"v2m_parsimony_of_sites": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, _u64p]),
	"v2m_tree_parsimony": (C.c_int, [C.c_void_p, C.POINTER(RowBatchStruct), C.c_void_p, C.c_uint32, C.c_void_p, TREE_SINK_FN, TREE_SINK_FN, C.c_void_p, C.POINTER(TreeParsimonyInfo)]),
	"v2m_diversity_of_counts": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
		C.POINTER(WindowDiversityInfo)]),
	"v2m_window_diversity": (C.c_int, [C.c_void_p, C.POINTER(RowBatchStruct), C.POINTER(RowBatchStruct), C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
		C.POINTER(WindowDiversityInfo)]),
	"v2m_pbwt_cut_trials": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
		C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
	"v2m_pbwt_cut_trials_streamed": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
		C.c_uint64, C.c_void_p, C.c_void_p, TRIALS_SINK_FN, C.c_void_p]),
	"v2m_pbwt_cut_records": (C.c_int, [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
		C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
	"v2m_alloc_output": (C.c_int, [C.c_void_p, C.c_uint64, C.c_int, C.POINTER(C.c_void_p)]),
	"v2m_free_output": (C.c_int, [C.c_void_p, C.c_void_p]),
	"v2m_read_output": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
	"v2m_bgzf_bound": (C.c_uint64, [C.c_uint64]),
	"v2m_bgzf_frame_stored": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, _u64p]),
	"v2m_bgzf_compress": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, _u64p]),
	"v2m_bgzf_scan": (C.c_int, [C.c_void_p, C.c_uint64, _u64p, _u64p, C.POINTER(C.c_int)]),
	"v2m_bgzf_decompress": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, _u64p]),
	"v2m_vcf_scan": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, VCF_LAYOUT_FN, VCF_CHUNK_FN, C.c_void_p]),
	"v2m_checksum_rows_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]),
	"v2m_profile_enable": (C.c_int, [C.c_void_p, C.c_int]),
	"v2m_profile_reset": (C.c_int, [C.c_void_p]),
	"v2m_profile_get": (C.c_int, [C.c_void_p, C.c_int, _u64p, C.POINTER(C.c_double)]),
	"v2m_profile_get_launches": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_uint64, _u64p]),
}

_lib = None


def library_path():
	"""The product library; V2M_HIP_LIBRARY names another build of the same sources (the tuning build, tools and tests only)."""
	return os.environ.get("V2M_HIP_LIBRARY") or _build.LIB_PATH


def load():
	"""Loads libv2m_hip.so.  Raises ImportError if it has not been built -- there is no fallback."""
	global _lib
	if _lib is not None:
		return _lib
	path = library_path()
	if not os.path.exists(path):
		raise ImportError(
			"%s is missing: build the HIP extension first (python -c 'import __graft_entry__ as g; g.build()'). "
			"vcf2multialign_amd has no CPU fallback." % path)
	# One HIP runtime per process: torch ships its own libamdhip64 (SONAME libamdhip64.so.7, the same as
	# /opt/rocm's).  Importing torch first makes our NEEDED entry resolve to the copy torch already
	# loaded; the other order would load two runtimes and the second one finds no GPU.
	try:
		import torch  # noqa: F401
	except ImportError:
		pass
	lib = C.CDLL(path)
	for name, (restype, argtypes) in SIGNATURES.items():
		fn = getattr(lib, name)   # AttributeError if the library does not export a declared symbol
		fn.restype = restype
		fn.argtypes = argtypes
	_lib = lib
	return lib


def hip_runtime():
	"""The HIP runtime this process already has loaded (torch's copy, or /opt/rocm's through libv2m_hip.so), as a ctypes handle --
	found by its mapping, not by a versioned soname.  For device <-> host copies in tools, tests and bench.py."""
	load()
	with open("/proc/self/maps") as f:
		for line in f:
			path = line.split()[-1]
			if "libamdhip64.so" in os.path.basename(path):
				return C.CDLL(path)
	raise ImportError("no libamdhip64 is loaded in this process")
