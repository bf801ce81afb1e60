"""Binding of the C++ host library's graph builder (libv2m_host.so: csrc/host/readers.cc + graph_builder.cc),
used by the tests to compare it with the oracle's builder.  The transpose is not part of it (GPU)."""

import ctypes as C
import os
import stat

import numpy as np

from . import _native
from . import build as _build

_u64p = C.POINTER(C.c_uint64)
_lib = None


def library_path():
	"""The host library; V2M_HOST_LIBRARY names another build (libv2m_host_checked.so, linked against the checked HIP library: tests only)."""
	return os.environ.get("V2M_HOST_LIBRARY") or _build.HOST_LIB_PATH


def _load():
	global _lib
	if _lib is None:
		path = library_path()
		if not os.path.exists(path):
			raise ImportError(path + " is missing: run __graft_entry__.build()")
		try:
			import torch  # noqa: F401  (one HIP runtime per process, see _native.load)
		except ImportError:
			pass
		L = C.CDLL(path)
		L.v2mh_build_variant_graph.restype = C.c_void_p
		L.v2mh_build_variant_graph.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_int, C.c_uint, C.c_char_p, C.c_size_t]
		L.v2mh_build_variant_graph_gpu.restype = C.c_void_p
		L.v2mh_build_variant_graph_gpu.argtypes = [C.c_void_p] + L.v2mh_build_variant_graph.argtypes
		L.v2mh_build_variant_graph_scanned.restype = C.c_void_p
		L.v2mh_build_variant_graph_scanned.argtypes = L.v2mh_build_variant_graph_gpu.argtypes + [C.c_int]
		L.v2mh_scan_statistics.argtypes = [C.c_void_p, _u64p, _u64p]
		L.v2mh_scan_lines_host.restype = C.c_int
		L.v2mh_scan_lines_host.argtypes = [C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
		L.v2mh_free.argtypes = [C.c_void_p]
		L.v2mh_graph_from_arrays.restype = C.c_void_p
		L.v2mh_graph_from_arrays.argtypes = [C.c_uint64, C.c_uint64] + [C.c_void_p] * 5 + [C.c_char_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_uint32]
		L.v2mh_write_graph.restype = C.c_int
		L.v2mh_write_graph.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_size_t]
		L.v2mh_read_graph.restype = C.c_void_p
		L.v2mh_read_graph.argtypes = [C.c_char_p, C.c_char_p, C.c_size_t]
		for n in ("node_count", "edge_count", "sample_count", "ref_length", "sample_blob_size", "ploidy_csum_size", "handled_variants", "chr_id_mismatches", "overlap_count"):
			f = getattr(L, "v2mh_" + n)
			f.restype = C.c_uint64
			f.argtypes = [C.c_void_p]
		for n in ("reference_positions", "aligned_positions", "alt_edge_targets", "alt_edge_count_csum", "label_offsets"):
			f = getattr(L, "v2mh_" + n)
			f.restype = _u64p
			f.argtypes = [C.c_void_p]
		for n in ("reference", "label_bytes", "sample_blob", "ploidy_csum"):
			f = getattr(L, "v2mh_" + n)
			f.restype = C.c_void_p
			f.argtypes = [C.c_void_p]
		L.v2mh_paths_by_edge_and_chrom_copy.restype = _u64p
		L.v2mh_paths_by_edge_and_chrom_copy.argtypes = [C.c_void_p, _u64p, _u64p]
		L.v2mh_find_founders.restype = C.c_uint64
		L.v2mh_find_founders.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32)]
		L.v2mh_find_founders_mt.restype = C.c_uint64
		L.v2mh_find_founders_mt.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.c_uint]
		L.v2mh_set_paths_by_chrom_copy_and_edge.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]
		L.v2mh_overlap_get.argtypes = [C.c_void_p, C.c_uint64, _u64p, _u64p, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
		L.v2mh_columns_of_reference_range.restype = C.c_int
		L.v2mh_columns_of_reference_range.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, _u64p, _u64p]
		L.v2mh_chain_text.restype = C.c_int64
		L.v2mh_chain_text.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
		L.v2mh_paf_text.restype = C.c_int64
		L.v2mh_paf_text.argtypes = [C.c_void_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
		L.v2mh_column_counts_text.restype = C.c_int64
		L.v2mh_column_counts_text.argtypes = [C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
		L.v2mh_distances_text.restype = C.c_int64
		L.v2mh_distances_text.argtypes = [C.POINTER(C.c_char_p), C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
		L.v2mh_site_positions_text.restype = C.c_int64
		L.v2mh_site_positions_text.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
		L.v2mh_site_ld_text.restype = C.c_int64
		L.v2mh_site_ld_text.argtypes = [C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
			C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
		L.v2mh_parse_decimal_fraction.restype = C.c_int
		L.v2mh_parse_decimal_fraction.argtypes = [C.c_char_p, C.POINTER(C.c_uint32), C.POINTER(C.c_uint32)]
		L.v2mh_nj_tree_cpu.restype = C.c_int
		L.v2mh_nj_tree_cpu.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
		L.v2mh_nj_newick_text.restype = C.c_int64
		L.v2mh_nj_newick_text.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_char_p), C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
		L.v2mh_nj_newick_support_text.restype = C.c_int64
		L.v2mh_nj_newick_support_text.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
		L.v2mh_nj_split_support.restype = C.c_int
		L.v2mh_nj_split_support.argtypes = [C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
		L.v2mh_tree_parsimony_cpu.restype = C.c_int64
		L.v2mh_tree_parsimony_cpu.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
		L.v2mh_nj_newick_parsimony_text.restype = C.c_int64
		L.v2mh_nj_newick_parsimony_text.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_char_p), C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
		L.v2mh_tree_mutations_text.restype = C.c_int64
		L.v2mh_tree_mutations_text.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.POINTER(C.c_char_p), C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
			C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
		L.v2mh_tree_sites_text.restype = C.c_int64
		L.v2mh_tree_sites_text.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
		L.v2mh_window_diversity_cpu.restype = C.c_int
		L.v2mh_window_diversity_cpu.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, _u64p,
			C.c_char_p, C.c_size_t]
		L.v2mh_window_diversity_values.restype = C.c_int
		L.v2mh_window_diversity_values.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p]
		L.v2mh_window_divergence_values.restype = C.c_int
		L.v2mh_window_divergence_values.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
		L.v2mh_window_diversity_text.restype = C.c_int64
		L.v2mh_window_diversity_text.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
		L.v2mh_window_divergence_text.restype = C.c_int64
		L.v2mh_window_divergence_text.argtypes = [C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64,
			C.c_char_p, C.c_size_t]
		L.v2mh_diversity_sfs_text.restype = C.c_int64
		L.v2mh_diversity_sfs_text.argtypes = [C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
		L.v2mh_shard_copies.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, _u64p, _u64p]
		L.v2mh_write_cut_positions.restype = C.c_int
		L.v2mh_write_cut_positions.argtypes = [C.c_char_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_uint32, C.c_char_p, C.c_size_t]
		L.v2mh_read_cut_positions.restype = C.c_int
		L.v2mh_read_cut_positions.argtypes = [C.c_char_p, C.c_void_p, _u64p, _u64p, C.POINTER(C.c_uint32), C.c_char_p, C.c_size_t]
		_lib = L
	return _lib


def shard_copies(n_copies, world, rank):
	"""The C++ driver's copy range of GPU `rank` of `world` (csrc/host/gpu_path.cc: shard_copies)."""
	a, b = C.c_uint64(), C.c_uint64()
	_load().v2mh_shard_copies(n_copies, world, rank, C.byref(a), C.byref(b))
	return a.value, b.value


def chain_text(ops, t_name, t_size, q_name, q_size, chain_id):
	"""The host library's chain formatter (csrc/host/output.cc: chain_text; no GPU): the UCSC chain, as bytes, of the alignment ops
	`ops` ((n, 2) of (op, length), 0 = M, 1 = I, 2 = D) with the reference as target and the row as query; b"" for ops without any M."""
	a = np.ascontiguousarray(ops, dtype=np.uint32).reshape(-1, 2)
	L = _load()
	err = C.create_string_buffer(512)
	args = (a.ctypes.data if a.size else None, a.shape[0], str(t_name).encode(), int(t_size), str(q_name).encode(), int(q_size), int(chain_id))
	n = L.v2mh_chain_text(*args, None, 0, err, len(err))
	if n < 0:
		raise ValueError(err.value.decode())
	dst = C.create_string_buffer(max(1, n))
	if n != L.v2mh_chain_text(*args, dst, n, err, len(err)):
		raise ValueError(err.value.decode())
	return dst.raw[:n]


def paf_text(ops, t_name, t_size, q_name, q_size):
	"""The host library's PAF formatter (csrc/host/output.cc: paf_text; no GPU): the PAF line, as bytes, of the SPLIT alignment ops `ops`
	((n, 2) of (op, length), 7 = '=', 8 = X, 1 = I, 2 = D) with the reference as target and the row as query; b"" for ops without any
	= / X.  ValueError for any other op code (0 = M: ops made without split_match)."""
	a = np.ascontiguousarray(ops, dtype=np.uint32).reshape(-1, 2)
	L = _load()
	err = C.create_string_buffer(512)
	args = (a.ctypes.data if a.size else None, a.shape[0], str(t_name).encode(), int(t_size), str(q_name).encode(), int(q_size))
	n = L.v2mh_paf_text(*args, None, 0, err, len(err))
	if n < 0:
		raise ValueError(err.value.decode())
	dst = C.create_string_buffer(max(1, n))
	if n != L.v2mh_paf_text(*args, dst, n, err, len(err)):
		raise ValueError(err.value.decode())
	return dst.raw[:n]


def column_counts_text(n_rows, columns, counts, reference_positions, aligned_positions):
	"""The host library's column-count formatter (csrc/host/output.cc: column_counts_text; no GPU): the TSV, as bytes, of the records
	(columns[i], counts[i, 0..6)) of a batch of n_rows rows over the graph whose node arrays are given."""
	columns = np.ascontiguousarray(columns, dtype=np.uint64).reshape(-1)
	counts = np.ascontiguousarray(counts, dtype=np.uint32).reshape(-1, 6)
	if columns.shape[0] != counts.shape[0]:
		raise ValueError("columns and counts differ in length")
	records = np.zeros(columns.shape[0], dtype=np.dtype(_native.COLUMN_COUNT_DTYPE))
	records["column"] = columns
	records["count"] = counts
	ref = np.ascontiguousarray(reference_positions, dtype=np.uint64)
	aln = np.ascontiguousarray(aligned_positions, dtype=np.uint64)
	if ref.shape != aln.shape:
		raise ValueError("reference_positions and aligned_positions differ in length")
	L = _load()
	err = C.create_string_buffer(512)
	args = (int(n_rows), records.ctypes.data if records.size else None, records.shape[0], ref.ctypes.data if ref.size else None, aln.ctypes.data if aln.size else None, ref.shape[0])
	n = L.v2mh_column_counts_text(*args, None, 0, err, len(err))
	if n < 0:
		raise ValueError(err.value.decode())
	dst = C.create_string_buffer(max(1, n))
	if n != L.v2mh_column_counts_text(*args, dst, n, err, len(err)):
		raise ValueError(err.value.decode())
	return dst.raw[:n]


def distances_text(ids, dist, n_columns, n_sites, acgt_only=False):
	"""The host library's distance formatter (csrc/host/output.cc: distances_text; no GPU): the TSV, as bytes, of the matrix dist[n, n]
	of the sequences named `ids` over n_columns columns of which n_sites are variable."""
	names = [i if isinstance(i, bytes) else str(i).encode() for i in ids]
	n = len(names)
	dist = np.ascontiguousarray(dist, dtype=np.uint32).reshape(n, n)
	if any(b"\0" in i for i in names):
		raise ValueError("a sequence name holds a NUL byte")
	array = (C.c_char_p * max(1, n))(*names)
	L = _load()
	err = C.create_string_buffer(512)
	args = (array, n, dist.ctypes.data if dist.size else None, int(n_columns), int(n_sites), 1 if acgt_only else 0)
	size = L.v2mh_distances_text(*args, None, 0, err, len(err))
	if size < 0:
		raise ValueError(err.value.decode())
	dst = C.create_string_buffer(max(1, size))
	if size != L.v2mh_distances_text(*args, dst, size, err, len(err)):
		raise ValueError(err.value.decode())
	return dst.raw[:size]


def site_positions_text(columns, reference_positions, aligned_positions):
	"""The host library's formatter of --output-site-positions (csrc/host/output.cc: site_positions_text; no GPU): one line per absolute
	aligned column, `column<TAB>reference position`, as bytes -- the first two fields of column_counts_text's line for that column."""
	columns = np.ascontiguousarray(columns, dtype=np.uint64)
	ref = np.ascontiguousarray(reference_positions, dtype=np.uint64)
	aln = np.ascontiguousarray(aligned_positions, dtype=np.uint64)
	L = _load()
	err = C.create_string_buffer(512)
	args = (columns.ctypes.data if len(columns) else None, len(columns), ref.ctypes.data, aln.ctypes.data, len(aln))
	size = L.v2mh_site_positions_text(*args, None, 0, err, len(err))
	if size < 0:
		raise ValueError(err.value.decode())
	dst = C.create_string_buffer(max(1, size))
	if size != L.v2mh_site_positions_text(*args, dst, size, err, len(err)):
		raise ValueError(err.value.decode())
	return dst.raw[:size]


def site_ld_text(n_rows, n_columns, sites, pairs, reference_positions, aligned_positions, window_sites=1000, window_columns=0, min_r2=(1, 5), min_allele_count=1):
	"""The host library's formatter of --output-ld (csrc/host/output.cc: site_ld_text; no GPU): the TSV, as bytes, of the site and pair
	records of Context.site_ld for n_rows rows over n_columns columns, under the parameters of the call."""
	from . import _native as N
	sites = np.ascontiguousarray(sites, dtype=np.dtype(N.LD_SITE_DTYPE))
	pairs = np.ascontiguousarray(pairs, dtype=np.dtype(N.LD_PAIR_DTYPE))
	ref = np.ascontiguousarray(reference_positions, dtype=np.uint64)
	aln = np.ascontiguousarray(aligned_positions, dtype=np.uint64)
	params = N.SiteLdParams(int(window_sites), int(min_allele_count), int(min_r2[0]), int(min_r2[1]), int(window_columns))
	L = _load()
	err = C.create_string_buffer(512)
	args = (int(n_rows), int(n_columns), sites.ctypes.data if len(sites) else None, len(sites), pairs.ctypes.data if len(pairs) else None, len(pairs),
		C.addressof(params), ref.ctypes.data, aln.ctypes.data, len(aln))
	size = L.v2mh_site_ld_text(*args, None, 0, err, len(err))
	if size < 0:
		raise ValueError(err.value.decode())
	dst = C.create_string_buffer(max(1, size))
	if size != L.v2mh_site_ld_text(*args, dst, size, err, len(err)):
		raise ValueError(err.value.decode())
	return dst.raw[:size]


def parse_decimal_fraction(text):
	"""--ld-min-r2's value as (numerator, denominator) in lowest terms, from its digits (csrc/host/output.cc: parse_decimal_fraction);
	ValueError unless it is DIGITS[.DIGITS] with at most 6 decimals inside [0, 1]."""
	num, den = C.c_uint32(), C.c_uint32()
	if not _load().v2mh_parse_decimal_fraction(str(text).encode(), C.byref(num), C.byref(den)):
		raise ValueError("%r is no decimal number from 0 to 1 with at most 6 decimals" % (text,))
	return int(num.value), int(den.value)


def nj_tree_cpu(dist):
	"""The host library's plain-loop neighbour joining (csrc/host/output.cc: nj_tree_cpu; no GPU): the n - 2 v2m_nj_node records, as a
	structured array, of the tree of dist[n, n] (u32; only the upper triangle is read), n >= 3."""
	from . import _native as N
	dist = np.ascontiguousarray(dist, dtype=np.uint32)
	if dist.ndim != 2 or dist.shape[0] != dist.shape[1]:
		raise ValueError("dist is no square matrix")
	n = dist.shape[0]
	if n < 3:
		raise ValueError("a neighbour-joining tree needs at least 3 taxa (got %d)" % n)
	nodes = np.zeros(n - 2, dtype=np.dtype(N.NJ_NODE_DTYPE))
	if 0 != _load().v2mh_nj_tree_cpu(dist.ctypes.data, n, n, nodes.ctypes.data):
		raise ValueError("v2mh_nj_tree_cpu failed")
	return nodes


def nj_newick_text(nodes, labels):
	"""The host library's Newick writer (csrc/host/output.cc: nj_newick_text; no GPU): the text, as bytes, of the tree of the
	v2m_nj_node records `nodes` (len(labels) - 2 of them) over the leaves named `labels`."""
	from . import _native as N
	names = [i if isinstance(i, bytes) else str(i).encode() for i in labels]
	n = len(names)
	nodes = np.ascontiguousarray(nodes, dtype=np.dtype(N.NJ_NODE_DTYPE))
	if n < 3 or len(nodes) != n - 2:
		raise ValueError("%d records and %d labels are no tree" % (len(nodes), n))
	if any(b"\0" in i for i in names):
		raise ValueError("a label holds a NUL byte")
	array = (C.c_char_p * n)(*names)
	L = _load()
	err = C.create_string_buffer(512)
	args = (nodes.ctypes.data, n, array)
	size = L.v2mh_nj_newick_text(*args, None, 0, err, len(err))
	if size < 0:
		raise ValueError(err.value.decode())
	dst = C.create_string_buffer(max(1, size))
	if size != L.v2mh_nj_newick_text(*args, dst, size, err, len(err)):
		raise ValueError(err.value.decode())
	return dst.raw[:size]


def nj_newick_support_text(nodes, labels, support):
	"""The host library's Newick writer with bootstrap support (csrc/host/output.cc: nj_newick_support_text; no GPU): nj_newick_text
	with support[t] written as the label of join node len(labels) + t."""
	from . import _native as N
	names = [i if isinstance(i, bytes) else str(i).encode() for i in labels]
	n = len(names)
	nodes = np.ascontiguousarray(nodes, dtype=np.dtype(N.NJ_NODE_DTYPE))
	support = np.ascontiguousarray(support, dtype=np.uint32)
	if n < 3 or len(nodes) != n - 2 or support.shape != (n - 3,):
		raise ValueError("%d records, %d labels and %d counts are no tree with support" % (len(nodes), n, support.size))
	if any(b"\0" in i for i in names):
		raise ValueError("a label holds a NUL byte")
	array = (C.c_char_p * n)(*names)
	L = _load()
	err = C.create_string_buffer(512)
	args = (nodes.ctypes.data, n, array, support.ctypes.data if n > 3 else None)
	size = L.v2mh_nj_newick_support_text(*args, None, 0, err, len(err))
	if size < 0:
		raise ValueError(err.value.decode())
	dst = C.create_string_buffer(max(1, size))
	if size != L.v2mh_nj_newick_support_text(*args, dst, size, err, len(err)):
		raise ValueError(err.value.decode())
	return dst.raw[:size]


def nj_split_support(main_nodes, replicate_nodes):
	"""The host library's split counting (csrc/nj_support.hpp; no GPU): np.uint32[n - 3], per join record of the tree `main_nodes`
	(n - 2 v2m_nj_node records) the number of the trees `replicate_nodes` ([B, n - 2]) that hold the record's split.  ValueError for
	records that are no tree."""
	from . import _native as N
	main_nodes = np.ascontiguousarray(main_nodes, dtype=np.dtype(N.NJ_NODE_DTYPE))
	n = len(main_nodes) + 2
	replicate_nodes = np.ascontiguousarray(replicate_nodes, dtype=np.dtype(N.NJ_NODE_DTYPE)).reshape(-1, n - 2)
	if main_nodes.ndim != 1 or n < 3:
		raise ValueError("a tree has at least one record")
	support = np.zeros(max(1, n - 3), dtype=np.uint32)
	B = replicate_nodes.shape[0]
	if 0 != _load().v2mh_nj_split_support(n, main_nodes.ctypes.data, replicate_nodes.ctypes.data if B else None, B, support.ctypes.data):
		raise ValueError("v2mh_nj_split_support: the records are no trees over %d leaves" % n)
	return support[:n - 3]


def tree_parsimony_cpu(rows, nodes, n_sites=None, want_mutations=True):
	"""The host library's plain-loop parsimony (csrc/host/output.cc: tree_parsimony_cpu; no GPU) of the sites of rows[n, pitch] (u8; the
	first n_sites bytes of a row count, all of them by default) on the tree of the n - 2 v2m_nj_node records `nodes`: (sites,
	branch_changes, mutations) -- v2m_parsimony_site[n_sites], np.uint32[2 n - 3] and the v2m_tree_mutation records (none with
	want_mutations=False).  ValueError for records that are no tree."""
	from . import _native as N
	rows = np.ascontiguousarray(rows, dtype=np.uint8)
	if rows.ndim != 2:
		raise ValueError("rows is no matrix of bytes")
	n, pitch = rows.shape
	V = pitch if n_sites is None else int(n_sites)
	nodes = np.ascontiguousarray(nodes, dtype=np.dtype(N.NJ_NODE_DTYPE))
	if n < 3 or len(nodes) != n - 2 or not 0 <= V <= pitch:
		raise ValueError("%d records, %d rows and %d sites of %d bytes are no tree with sites" % (len(nodes), n, V, pitch))
	sites = np.zeros(V, dtype=np.dtype(N.PARSIMONY_SITE_DTYPE))
	branch_changes = np.zeros(2 * n - 3, dtype=np.uint32)
	L = _load()
	err = C.create_string_buffer(512)
	args = (rows.ctypes.data if rows.size else None, n, V, pitch, nodes.ctypes.data, sites.ctypes.data if V else None, branch_changes.ctypes.data)
	total = L.v2mh_tree_parsimony_cpu(*args, None, 0, err, len(err))
	if total < 0:
		raise ValueError(err.value.decode())
	mutations = np.zeros(total if want_mutations else 0, dtype=np.dtype(N.TREE_MUTATION_DTYPE))
	if want_mutations and total and total != L.v2mh_tree_parsimony_cpu(*args, mutations.ctypes.data, total, err, len(err)):
		raise ValueError(err.value.decode())
	return sites, branch_changes, mutations


def nj_newick_parsimony_text(nodes, labels, branch_changes):
	"""The host library's Newick writer of --output-tree-parsimony (csrc/host/output.cc: nj_newick_parsimony_text; no GPU):
	nj_newick_text's topology with branch_changes[x] as the length of node x's branch and node<t> as the label of internal node
	len(labels) + t."""
	from . import _native as N
	names = [i if isinstance(i, bytes) else str(i).encode() for i in labels]
	n = len(names)
	nodes = np.ascontiguousarray(nodes, dtype=np.dtype(N.NJ_NODE_DTYPE))
	branch_changes = np.ascontiguousarray(branch_changes, dtype=np.uint32)
	if n < 3 or len(nodes) != n - 2 or branch_changes.shape != (2 * n - 3,):
		raise ValueError("%d records, %d labels and %d counts are no tree with branch changes" % (len(nodes), n, branch_changes.size))
	if any(b"\0" in i for i in names):
		raise ValueError("a label holds a NUL byte")
	array = (C.c_char_p * n)(*names)
	L = _load()
	err = C.create_string_buffer(512)
	args = (nodes.ctypes.data, n, array, branch_changes.ctypes.data)
	size = L.v2mh_nj_newick_parsimony_text(*args, None, 0, err, len(err))
	if size < 0:
		raise ValueError(err.value.decode())
	dst = C.create_string_buffer(max(1, size))
	if size != L.v2mh_nj_newick_parsimony_text(*args, dst, size, err, len(err)):
		raise ValueError(err.value.decode())
	return dst.raw[:size]


def tree_mutations_text(mutations, sites, labels, reference_positions, aligned_positions):
	"""The host library's formatter of --output-tree-mutations (csrc/host/output.cc: tree_mutations_text; no GPU): one line per
	v2m_tree_mutation record, `node<TAB>column<TAB>reference position<TAB>from<TAB>to`, as bytes; sites are the v2m_tree_site records the
	mutations index, labels the leaves' names."""
	from . import _native as N
	mutations = np.ascontiguousarray(mutations, dtype=np.dtype(N.TREE_MUTATION_DTYPE))
	sites = np.ascontiguousarray(sites, dtype=np.dtype(N.TREE_SITE_DTYPE))
	names = [i if isinstance(i, bytes) else str(i).encode() for i in labels]
	if any(b"\0" in i for i in names):
		raise ValueError("a label holds a NUL byte")
	array = (C.c_char_p * max(1, len(names)))(*names)
	ref = np.ascontiguousarray(reference_positions, dtype=np.uint64)
	aln = np.ascontiguousarray(aligned_positions, dtype=np.uint64)
	L = _load()
	err = C.create_string_buffer(512)
	args = (mutations.ctypes.data if len(mutations) else None, len(mutations), sites.ctypes.data if len(sites) else None, len(sites), array, len(names),
		ref.ctypes.data, aln.ctypes.data, len(aln))
	size = L.v2mh_tree_mutations_text(*args, None, 0, err, len(err))
	if size < 0:
		raise ValueError(err.value.decode())
	dst = C.create_string_buffer(max(1, size))
	if size != L.v2mh_tree_mutations_text(*args, dst, size, err, len(err)):
		raise ValueError(err.value.decode())
	return dst.raw[:size]


def tree_sites_text(sites, reference_positions, aligned_positions):
	"""The host library's formatter of --output-tree-sites (csrc/host/output.cc: tree_sites_text; no GPU): one line per v2m_tree_site
	record, `column<TAB>reference position<TAB>states<TAB>steps<TAB>homoplasy`, as bytes."""
	from . import _native as N
	sites = np.ascontiguousarray(sites, dtype=np.dtype(N.TREE_SITE_DTYPE))
	ref = np.ascontiguousarray(reference_positions, dtype=np.uint64)
	aln = np.ascontiguousarray(aligned_positions, dtype=np.uint64)
	L = _load()
	err = C.create_string_buffer(512)
	args = (sites.ctypes.data if len(sites) else None, len(sites), ref.ctypes.data, aln.ctypes.data, len(aln))
	size = L.v2mh_tree_sites_text(*args, None, 0, err, len(err))
	if size < 0:
		raise ValueError(err.value.decode())
	dst = C.create_string_buffer(max(1, size))
	if size != L.v2mh_tree_sites_text(*args, dst, size, err, len(err)):
		raise ValueError(err.value.decode())
	return dst.raw[:size]


def window_diversity_cpu(rows, bounds, rows_b=None, length=None, want_sfs=True):
	"""The host library's plain-loop window diversity (csrc/host/output.cc: window_diversity_cpu; no GPU) from spliced rows: rows[n, pitch]
	(u8; the first `length` bytes of a row count, all of them by default) and, for the between form, rows_b[n_b, pitch], over the bins of
	`bounds` (relative to the rows).  Within: (bins, sfs, multiallelic) -- v2m_diversity_bin records, np.uint64[n / 2 + 1] (None and 0 with
	want_sfs=False).  Between: (bins, None, 0), bins of v2m_diversity_between_bin.  ValueError for bad bounds."""
	from . import _native as N
	rows = np.ascontiguousarray(rows, dtype=np.uint8)
	if rows.ndim != 2:
		raise ValueError("rows is no matrix of bytes")
	n, pitch = rows.shape
	between = rows_b is not None
	if between:
		rows_b = np.ascontiguousarray(rows_b, dtype=np.uint8)
		if rows_b.ndim != 2 or rows_b.shape[1] != pitch:
			raise ValueError("rows_b is no matrix of bytes of the same pitch")
	n_b = rows_b.shape[0] if between else 0
	L_cols = pitch if length is None else int(length)
	bounds = np.ascontiguousarray(bounds, dtype=np.uint64)
	n_bins = max(0, len(bounds) - 1)
	bins = np.zeros(max(1, n_bins), dtype=np.dtype(N.DIVERSITY_BETWEEN_BIN_DTYPE if between else N.DIVERSITY_BIN_DTYPE))
	sfs = np.zeros(n // 2 + 1, dtype=np.uint64) if (want_sfs and not between) else None
	multiallelic = C.c_uint64(0)
	err = C.create_string_buffer(512)
	if 0 == n_bins:   # (no bin: nothing to walk, as the library's calls return before any work)
		return bins[:0], sfs, 0
	if 0 != _load().v2mh_window_diversity_cpu(rows.ctypes.data if rows.size else None, n, rows_b.ctypes.data if between and rows_b.size else None, n_b, L_cols, pitch,
			bounds.ctypes.data if len(bounds) else None, n_bins, bins.ctypes.data, sfs.ctypes.data if sfs is not None else None, C.byref(multiallelic), err, len(err)):
		raise ValueError(err.value.decode())
	return bins[:n_bins], sfs, int(multiallelic.value)


def window_diversity_values(windows, n):
	"""The host library's doubles of include/v2m_hip.h's "window diversity" (csrc/host/output.cc: diversity_values_of): np.float64[len, 3]
	-- pi, theta_w, tajima_d -- of v2m_diversity_bin records over n sequences; NaN where a value does not exist."""
	from . import _native as N
	windows = np.ascontiguousarray(windows, dtype=np.dtype(N.DIVERSITY_BIN_DTYPE))
	out = np.zeros((len(windows), 3), dtype=np.float64)
	if len(windows) and 0 != _load().v2mh_window_diversity_values(windows.ctypes.data, len(windows), int(n), out.ctypes.data):
		raise ValueError("v2mh_window_diversity_values failed")
	return out


def window_divergence_values(between, windows_a, windows_b):
	"""Likewise np.float64[len, 2] -- dxy, fst -- of v2m_diversity_between_bin records and the two groups' v2m_diversity_bin records."""
	from . import _native as N
	between = np.ascontiguousarray(between, dtype=np.dtype(N.DIVERSITY_BETWEEN_BIN_DTYPE))
	windows_a = np.ascontiguousarray(windows_a, dtype=np.dtype(N.DIVERSITY_BIN_DTYPE))
	windows_b = np.ascontiguousarray(windows_b, dtype=np.dtype(N.DIVERSITY_BIN_DTYPE))
	if not len(between) == len(windows_a) == len(windows_b):
		raise ValueError("the three record lists differ in length")
	out = np.zeros((len(between), 2), dtype=np.float64)
	if len(between) and 0 != _load().v2mh_window_divergence_values(between.ctypes.data, windows_a.ctypes.data, windows_b.ctypes.data, len(between), out.ctypes.data):
		raise ValueError("v2mh_window_divergence_values failed")
	return out


def _handed_over_text(fn, args):
	err = C.create_string_buffer(512)
	size = fn(*args, None, 0, err, len(err))
	if size < 0:
		raise ValueError(err.value.decode())
	dst = C.create_string_buffer(max(1, size))
	if size != fn(*args, dst, size, err, len(err)):
		raise ValueError(err.value.decode())
	return dst.raw[:size]


def _group_name(group):
	name = group if isinstance(group, bytes) else str(group).encode()
	if b"\0" in name:
		raise ValueError("a group name holds a NUL byte")
	return name


def window_diversity_text(group, n, windows, starts, ends, header=False):
	"""The host library's formatter of --output-diversity (csrc/host/output.cc: window_diversity_text; no GPU): one line per window of
	group, start, end, columns, called, diffs, pairs, pi, segregating, complete, theta_w, tajima_d, as bytes."""
	from . import _native as N
	windows = np.ascontiguousarray(windows, dtype=np.dtype(N.DIVERSITY_BIN_DTYPE))
	starts = np.ascontiguousarray(starts, dtype=np.uint64)
	ends = np.ascontiguousarray(ends, dtype=np.uint64)
	if not len(windows) == len(starts) == len(ends):
		raise ValueError("windows, starts and ends differ in length")
	k = len(windows)
	return _handed_over_text(_load().v2mh_window_diversity_text, (_group_name(group), int(n), windows.ctypes.data if k else None, starts.ctypes.data if k else None,
		ends.ctypes.data if k else None, k, 1 if header else 0))


def window_divergence_text(group_a, group_b, between, windows_a, windows_b, starts, ends, header=False):
	"""The host library's formatter of --output-divergence (csrc/host/output.cc: window_divergence_text; no GPU): one line per window of
	group_a, group_b, start, end, columns, called, diffs, pairs, dxy, fst, as bytes."""
	from . import _native as N
	between = np.ascontiguousarray(between, dtype=np.dtype(N.DIVERSITY_BETWEEN_BIN_DTYPE))
	windows_a = np.ascontiguousarray(windows_a, dtype=np.dtype(N.DIVERSITY_BIN_DTYPE))
	windows_b = np.ascontiguousarray(windows_b, dtype=np.dtype(N.DIVERSITY_BIN_DTYPE))
	starts = np.ascontiguousarray(starts, dtype=np.uint64)
	ends = np.ascontiguousarray(ends, dtype=np.uint64)
	if not len(between) == len(windows_a) == len(windows_b) == len(starts) == len(ends):
		raise ValueError("the record lists, starts and ends differ in length")
	k = len(between)
	return _handed_over_text(_load().v2mh_window_divergence_text, (_group_name(group_a), _group_name(group_b), between.ctypes.data if k else None,
		windows_a.ctypes.data if k else None, windows_b.ctypes.data if k else None, starts.ctypes.data if k else None, ends.ctypes.data if k else None, k, 1 if header else 0))


def diversity_sfs_text(group, n, sfs, multiallelic, header=False):
	"""The host library's formatter of --diversity-sfs (csrc/host/output.cc: diversity_sfs_text; no GPU): one line per entry of the folded
	spectrum of n sequences, `group<TAB>n<TAB>minor count<TAB>columns`, then the multiallelic count, as bytes."""
	sfs = np.ascontiguousarray(sfs, dtype=np.uint64)
	if len(sfs) != int(n) // 2 + 1:
		raise ValueError("a spectrum of %d sequences has %d entries, not %d" % (n, int(n) // 2 + 1, len(sfs)))
	return _handed_over_text(_load().v2mh_diversity_sfs_text, (_group_name(group), int(n), sfs.ctypes.data, int(multiallelic), 1 if header else 0))


def write_cut_positions(path, cut_positions, min_distance, score):
	"""--output-cut-positions file (layout: vcf2multialign_amd/csrc/host/founder.hh)."""
	cuts = np.ascontiguousarray(cut_positions, dtype=np.uint64)
	err = C.create_string_buffer(512)
	if 0 != _load().v2mh_write_cut_positions(str(path).encode(), cuts.ctypes.data, len(cuts), min_distance, score, err, len(err)):
		raise OSError(err.value.decode())


def read_cut_positions(path):
	"""Returns (cut_positions, min_distance, score)."""
	L = _load()
	err = C.create_string_buffer(512)
	n, md, sc = C.c_uint64(0), C.c_uint64(), C.c_uint32()
	if 0 != L.v2mh_read_cut_positions(str(path).encode(), None, C.byref(n), C.byref(md), C.byref(sc), err, len(err)):
		raise ValueError(err.value.decode())
	cuts = np.zeros(max(1, n.value), dtype=np.uint64)
	if 0 != L.v2mh_read_cut_positions(str(path).encode(), cuts.ctypes.data, C.byref(n), C.byref(md), C.byref(sc), err, len(err)):
		raise ValueError(err.value.decode())
	return cuts[:n.value].tolist(), md.value, sc.value


def _has_gzip_magic(path):
	"""A regular file that starts with 1f 8b (a pipe is never read here: its first bytes belong to the reader)."""
	try:
		if not stat.S_ISREG(os.stat(path).st_mode):
			return False
		with open(path, "rb") as f:
			return f.read(2) == b"\x1f\x8b"
	except OSError:
		return False


def scan_lines_host(text, wanted_chr, layout=None, slice_bytes=0):
	"""The host's implementation of the VCF scan rule (csrc/host/readers.cc: scan_lines_host) over plain VCF text: the chunks v2m_vcf_scan
	gives for the same text and slice size, as Context.vcf_scan returns them.  Returns (code, chunks)."""
	from . import context as _context
	from . import _native as N
	L = _load()
	text = bytes(text)
	fn = layout or (lambda _i, line: _context.first_record_layout(line))
	rc, chunks, _ = _context.collect_vcf_scan(
		lambda lf, cf: L.v2mh_scan_lines_host(text, len(text), wanted_chr.encode(), slice_bytes, C.cast(lf, C.c_void_p), C.cast(cf, C.c_void_p), None), fn)
	return rc, chunks


def _arr(ptr, n, dtype):
	if n == 0 or not ptr:
		return np.zeros(0, dtype=dtype)
	return np.ctypeslib.as_array(ptr, shape=(n,)).astype(dtype, copy=True)


class HostGraph:
	"""Result of the host's build_variant_graph (without the final transpose)."""

	def __init__(self, fasta_path, vcf_path, chr_id, seq_id=None, exclude_sample=None, exclude_copy=-1, threads=0, _graph_file=None, _handle=None, ctx=None,
			gpu_parse=False, host_scan=False):
		"""ctx: a Context whose GPU inflates BGZF input (either file, recognised by its first bytes); without one, BGZF input is an error.
		gpu_parse (with ctx): the VCF's genotype columns become path bits on the GPU (v2m_vcf_scan), the text never reaches the host.
		host_scan: the same build through the host's implementation of the scan rule (plain files, no GPU).  Both leave
		scanned_lines / declined_lines."""
		L = _load()
		err = C.create_string_buffer(512)
		if _handle is not None:
			h = _handle
		elif _graph_file is not None:
			h = L.v2mh_read_graph(str(_graph_file).encode(), err, len(err))
		elif gpu_parse or host_scan:
			if gpu_parse and ctx is None:
				raise ValueError("HostGraph(..., gpu_parse=True) needs ctx=Context(...)")
			for path in (fasta_path, vcf_path) if ctx is None else ():
				if _has_gzip_magic(path):
					raise ValueError("%s is BGZF-compressed: HostGraph(..., ctx=Context(...)) needs a GPU context to inflate it" % path)
			h = L.v2mh_build_variant_graph_scanned(ctx._h if ctx is not None else None, str(fasta_path).encode(), seq_id.encode() if seq_id else None, str(vcf_path).encode(),
				chr_id.encode(), exclude_sample.encode() if exclude_sample else None, exclude_copy, threads, err, len(err), 1 if gpu_parse else 2)
		elif ctx is not None:
			h = L.v2mh_build_variant_graph_gpu(ctx._h, str(fasta_path).encode(), seq_id.encode() if seq_id else None, str(vcf_path).encode(), chr_id.encode(),
				exclude_sample.encode() if exclude_sample else None, exclude_copy, threads, err, len(err))
		else:
			for path in (fasta_path, vcf_path):
				if _has_gzip_magic(path):
					raise ValueError("%s is BGZF-compressed: HostGraph(..., ctx=Context(...)) needs a GPU context to inflate it" % path)
			h = L.v2mh_build_variant_graph(str(fasta_path).encode(), seq_id.encode() if seq_id else None, str(vcf_path).encode(), chr_id.encode(),
				exclude_sample.encode() if exclude_sample else None, exclude_copy, threads, err, len(err))
		if not h:
			raise ValueError(err.value.decode())
		self._h = h
		a, b = C.c_uint64(), C.c_uint64()
		L.v2mh_scan_statistics(h, C.byref(a), C.byref(b))
		self.scanned_lines, self.declined_lines = a.value, b.value
		if True:
			N, E, S = L.v2mh_node_count(h), L.v2mh_edge_count(h), L.v2mh_sample_count(h)
			self.ref = C.string_at(L.v2mh_reference(h), L.v2mh_ref_length(h))
			self.reference_positions = _arr(L.v2mh_reference_positions(h), N, np.uint64)
			self.aligned_positions = _arr(L.v2mh_aligned_positions(h), N, np.uint64)
			self.alt_edge_targets = _arr(L.v2mh_alt_edge_targets(h), E, np.uint64)
			self.alt_edge_count_csum = _arr(L.v2mh_alt_edge_count_csum(h), N + 1, np.uint64)
			self.label_offsets = _arr(L.v2mh_label_offsets(h), E + 1, np.uint64)
			self.label_bytes = C.string_at(L.v2mh_label_bytes(h), int(self.label_offsets[-1])) if E else b""
			blob = C.string_at(L.v2mh_sample_blob(h), L.v2mh_sample_blob_size(h))
			self.sample_names = [s.decode() for s in blob.split(b"\0")[:-1]] if S else []
			n_pc = L.v2mh_ploidy_csum_size(h)
			self.ploidy_csum = np.ctypeslib.as_array(C.cast(L.v2mh_ploidy_csum(h), C.POINTER(C.c_uint32)), shape=(n_pc,)).copy() if n_pc else np.zeros(1, np.uint32)
			r, c = C.c_uint64(), C.c_uint64()
			p = L.v2mh_paths_by_edge_and_chrom_copy(h, C.byref(r), C.byref(c))
			self.paths_by_edge_and_chrom_copy_dims = (r.value, c.value)
			self.paths_by_edge_and_chrom_copy = _arr(p, r.value * c.value // 64, np.uint64)
			self.handled_variants = L.v2mh_handled_variants(h)
			self.chr_id_mismatches = L.v2mh_chr_id_mismatches(h)
			self.overlaps = []
			for i in range(L.v2mh_overlap_count(h)):
				ln, rp, vid, smp, ci, gt = C.c_uint64(), C.c_uint64(), C.c_char_p(), C.c_char_p(), C.c_uint32(), C.c_uint32()
				L.v2mh_overlap_get(h, i, C.byref(ln), C.byref(rp), C.byref(vid), C.byref(smp), C.byref(ci), C.byref(gt))
				self.overlaps.append({"lineno": ln.value, "ref_pos": rp.value, "var_id": vid.value.decode(), "sample": smp.value.decode(), "chrom_copy_idx": ci.value, "gt": gt.value})

	def columns_of_reference_range(self, s, e):
		"""The column window of the 0-based half-open reference range [s, e), computed by the C++ host
		(v2mh_columns_of_reference_range; VariantGraph.columns_of_reference_range is the same rule in Python)."""
		b, en = C.c_uint64(), C.c_uint64()
		if _load().v2mh_columns_of_reference_range(self._h, int(s), int(e), C.byref(b), C.byref(en)):
			raise ValueError("reference range [%d, %d) is empty or not within the reference (%d)" % (int(s), int(e), len(self.ref)))
		return b.value, en.value

	def __del__(self):
		try:
			if getattr(self, "_h", None):
				_load().v2mh_free(self._h)
				self._h = None
		except Exception:
			pass

	@classmethod
	def from_arrays(cls, graph, paths_by_edge_and_chrom_copy, path_rows, path_cols, n_samples, ploidy):
		"""A host graph from a VariantGraph-like object plus the (copies x edges) path matrix words."""
		u64 = lambda x: np.ascontiguousarray(x, dtype=np.uint64)
		a = [u64(graph.reference_positions), u64(graph.aligned_positions), u64(graph.alt_edge_targets), u64(graph.alt_edge_count_csum), u64(graph.label_offsets)]
		pw = u64(paths_by_edge_and_chrom_copy)
		h = _load().v2mh_graph_from_arrays(len(a[0]), len(a[2]), a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, a[3].ctypes.data, a[4].ctypes.data,
			bytes(graph.label_bytes) + b"\0", pw.ctypes.data if pw.size else None, path_rows, path_cols, n_samples, ploidy)
		return cls(None, None, None, _handle=h)

	@classmethod
	def read(cls, path):
		"""read_graph(): a graph from this build's flat V2MGRAF1 file (no reference sequence)."""
		return cls(None, None, None, _graph_file=path)

	def write(self, path):
		err = C.create_string_buffer(512)
		if 0 != _load().v2mh_write_graph(self._h, str(path).encode(), err, len(err)):
			raise OSError(err.value.decode())

	def set_transposed_paths(self, words, rows, cols):
		"""paths_by_chrom_copy_and_edge (rows = edges, cols = copies) as produced by the transpose: needed by the
		multi-threaded founder search when the graph was built without a GPU context."""
		w = np.ascontiguousarray(words, dtype=np.uint64)
		assert w.size == rows // 64 * cols
		_load().v2mh_set_paths_by_chrom_copy_and_edge(self._h, w.ctypes.data, rows, cols)

	def find_cut_positions_gpu(self, ctx, min_distance=0, threads=0):
		"""find_cut_positions with the chunk walks on the GPU (v2m_pbwt_cut_trials): `ctx` is a vcf2multialign_amd.Context that holds
		this graph WITH its transposed path matrix.  Returns (cut_positions, score) or None."""
		L = _load()
		L.v2mh_find_cut_positions_gpu.restype = C.c_uint64
		L.v2mh_find_cut_positions_gpu.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint, C.c_void_p, C.POINTER(C.c_uint32), C.c_void_p, C.c_char_p, C.c_size_t]
		n = len(self.reference_positions)
		cuts = np.zeros(n, dtype=np.uint64)
		score = C.c_uint32()
		err = C.create_string_buffer(512)
		chunks = (C.c_uint64 * 2)()
		k = L.v2mh_find_cut_positions_gpu(self._h, ctx._h, min_distance, threads, cuts.ctypes.data, C.byref(score), chunks, err, len(err))
		if err.value:
			raise RuntimeError(err.value.decode())
		self.gpu_chunks_walked, self.gpu_chunks_left = int(chunks[0]), int(chunks[1])   # by the GPU / by the host after all
		if k == 0:
			return None
		return cuts[:k].tolist(), score.value

	def find_founders_gpu(self, ctx, founder_count, min_distance=0, keep_ref_edges=False, threads=0, cut_positions=None):
		"""find_cut_positions + find_matchings with the chunk walks of both on the GPU (v2m_pbwt_cut_trials, v2m_pbwt_cut_records);
		cut_positions: skip the search and match over these.  Returns (cut_positions, assigned_samples column-major, score) or None;
		self.gpu_chunks = (search: on the GPU, on the host; matching: on the GPU, on the host)."""
		L = _load()
		L.v2mh_find_founders_gpu.restype = C.c_uint64
		L.v2mh_find_founders_gpu.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_uint, C.c_int, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64,
			C.POINTER(C.c_uint32), C.c_void_p, C.c_char_p, C.c_size_t]
		n = len(self.reference_positions)
		cuts = np.zeros(n, dtype=np.uint64)
		n_in = 0
		if cut_positions is not None:
			n_in = len(cut_positions)
			cuts[:n_in] = cut_positions
		assigned = np.zeros(max(1, n * founder_count), dtype=np.uint32)
		score = C.c_uint32()
		chunks = (C.c_uint64 * 4)()
		err = C.create_string_buffer(512)
		k = L.v2mh_find_founders_gpu(self._h, ctx._h, min_distance, founder_count, int(keep_ref_edges), threads, int(cut_positions is None), n_in,
			cuts.ctypes.data, assigned.ctypes.data, assigned.size, C.byref(score), chunks, err, len(err))
		if err.value:
			raise RuntimeError(err.value.decode())
		self.gpu_chunks = tuple(int(x) for x in chunks)
		if k == 0:
			return None
		return cuts[:k].tolist(), assigned[:(k - 1) * founder_count].tolist(), score.value

	def find_founders_walked_on_host(self, founder_count, min_distance=0, keep_ref_edges=False, threads=2, max_copies=2 ** 63):
		"""The walked searches (chunks handed to a founder_walker) with the host's own edge-by-edge walker: what the GPU path runs around
		its kernels, testable without a GPU.  self.gpu_chunks = chunks (search: walked, handed back; matching: walked, handed back)."""
		L = _load()
		L.v2mh_find_founders_walked_on_host.restype = C.c_uint64
		L.v2mh_find_founders_walked_on_host.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_uint, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint32), C.c_void_p, C.c_char_p, C.c_size_t]
		n = len(self.reference_positions)
		cuts = np.zeros(n, dtype=np.uint64)
		assigned = np.zeros(max(1, n * founder_count), dtype=np.uint32)
		score = C.c_uint32()
		chunks = (C.c_uint64 * 4)()
		err = C.create_string_buffer(512)
		k = L.v2mh_find_founders_walked_on_host(self._h, min_distance, founder_count, int(keep_ref_edges), threads, max_copies, cuts.ctypes.data, assigned.ctypes.data, assigned.size, C.byref(score), chunks, err, len(err))
		self.gpu_chunks = tuple(int(x) for x in chunks)
		if k == 0:
			if err.value:
				raise RuntimeError(err.value.decode())
			return None
		return cuts[:k].tolist(), assigned[:(k - 1) * founder_count].tolist(), score.value

	def find_matchings_walked_on_host(self, cut_positions, founder_count, keep_ref_edges=False, threads=2):
		"""find_matchings over the given cut positions with the host's own walker: find_founders_gpu(..., cut_positions=...) without a GPU.
		Returns assigned_samples column-major, None when there is nothing to match; RuntimeError for a cut list find_matchings refuses."""
		L = _load()
		L.v2mh_find_matchings_walked_on_host.restype = C.c_int
		L.v2mh_find_matchings_walked_on_host.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_uint, C.c_void_p, C.c_uint64, C.c_char_p, C.c_size_t]
		cuts = np.ascontiguousarray(cut_positions, dtype=np.uint64)
		assigned = np.zeros(max(1, len(cuts) * founder_count), dtype=np.uint32)
		err = C.create_string_buffer(512)
		if not L.v2mh_find_matchings_walked_on_host(self._h, cuts.ctypes.data, len(cuts), founder_count, int(keep_ref_edges), threads, assigned.ctypes.data, assigned.size, err, len(err)):
			if err.value:
				raise RuntimeError(err.value.decode())
			return None
		return assigned[:(len(cuts) - 1) * founder_count].tolist()

	def find_founders(self, founder_count, min_distance=0, keep_ref_edges=False, threads=1):
		"""find_cut_positions + find_matchings (host algorithms).  Returns (cut_positions, assigned_samples column-major, score)
		or None when there is no solution.  threads > 1 (0 = automatic) spreads the matching's pBWT over threads."""
		n = len(self.reference_positions)
		cuts = np.zeros(n, dtype=np.uint64)
		assigned = np.zeros(max(1, n * founder_count), dtype=np.uint32)
		score = C.c_uint32()
		k = _load().v2mh_find_founders_mt(self._h, min_distance, founder_count, int(keep_ref_edges), cuts.ctypes.data, assigned.ctypes.data, assigned.size, C.byref(score), threads)
		if k == 0:
			return None
		return cuts[:k].tolist(), assigned[:(k - 1) * founder_count].tolist(), score.value
