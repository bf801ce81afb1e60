"""The model of the variable sites (include/v2m_hip.h, "variable sites"): numpy over the aligned rows of the column counts' model
(tests/column_counts_model.py: matrix(g, rows, window), the CPU oracle's bodies).

selection() is the mask of the selected columns: the pair distances' sites (the VARIABLE columns of the column counts) for flags 0, and
for V2M_SITES_SNP the columns where at least two of the classes A, C, G, T are present.  expected() returns the selected absolute columns
and the rows' bytes there, unchanged.  One fact ties the two selections to what the pair distances compute and is held by
tests/test_variable_sites_host.py: the distances over the selected columns alone equal the distances over all columns -- for flags 0
under the all-classes definition, for the SNP selection under acgt_only.

corpus() is what tests/test_gpu_variable_sites.py runs: the pair distances' corpus as it is, and items at the seams of
gather_sites_kernel (csrc/site_kernels.hpp), whose constants are read from the source."""

import functools
import os
import re

import numpy as np

import column_counts_model as CM
import pair_distances_model as PM

PLOIDY_MAX = PM.PLOIDY_MAX
Item = PM.Item
SITE_KERNELS_HPP = os.path.join(PM.ROOT, "vcf2multialign_amd", "csrc", "site_kernels.hpp")


@functools.lru_cache(maxsize=None)
def kernel_constants():
	"""(S, T, G): kGatherSites, the sites a lane owns, kGatherThreads, the lanes of a workgroup, and kGatherMinGroupRows, the fewest rows
	of a row group, read from csrc/site_kernels.hpp."""
	with open(SITE_KERNELS_HPP) as f:
		text = f.read()
	out = []
	for name in ("kGatherSites", "kGatherThreads", "kGatherMinGroupRows"):
		found = re.findall(r"^constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text, re.M)
		assert len(found) == 1, "%s: %d definitions of the form `constexpr int %s = value;`" % (name, len(found), name)
		out.append(int(found[0]))
	return tuple(out)


# ---- the rule ------------------------------------------------------------------------------------------------------------------------------

def snp(m):
	"""bool[L]: at least two of the classes 0-3 (A, C, G, T, either case) are present in the column."""
	cls = PM.classes(m)
	return sum((cls == k).any(axis=0).astype(np.int64) for k in range(4)) >= 2 if m.shape[0] else np.zeros(m.shape[1], dtype=bool)


def selection(m, snp_only=False):
	"""bool[L]: the selected columns of the alignment m[n, L]."""
	return snp(m) if snp_only else PM.sites(m)


def expected(g, rows, window=None, snp_only=False):
	"""(columns u64[V], bytes u8[n, V], L) as Context.variable_sites reports them: the columns absolute."""
	m = CM.matrix(g, rows, window)
	mask = selection(m, snp_only)
	columns = np.flatnonzero(mask).astype(np.uint64) + np.uint64(window[0] if window else 0)
	return columns, np.ascontiguousarray(m[:, mask]), m.shape[1]


def fasta(ids, data):
	"""What --output-variable-sites writes: the -s file with every sequence line cut down to the selected columns."""
	return b"".join(b">" + i.encode() + b"\n" + bytes(row.tobytes()) + b"\n" for i, row in zip(ids, data))


def positions_text(g, columns):
	"""What --output-site-positions writes: the first two fields of the column counts' line of every selected column."""
	lines = []
	for col in (int(c) for c in columns):
		p = CM.reference_position(g, col)
		lines.append("%d\t%s\n" % (col, "." if p is None else str(p)))
	return "".join(lines).encode()


def a2m_ids(g, omit_reference=False):
	"""(ids, rows) of --haplotypes: the rows of the A2M output under the names the -s file gives them."""
	ids, rows = ([], []) if omit_reference else (["REF"], [PLOIDY_MAX])
	for s, sample in enumerate(g.sample_names):
		for c in range(int(g.ploidy_csum[s + 1]) - int(g.ploidy_csum[s])):
			ids.append("%s-%d" % (sample, 1 + c))
			rows.append(int(g.ploidy_csum[s]) + c)
	return ids, rows


# ---- the corpus of the GPU tests -----------------------------------------------------------------------------------------------------------

def seam_site_counts():
	"""With S sites a lane, W = 64 S a wave and B a workgroup: 1 ... S + 1, W - 1, W, W + 1, B - 1, B, B + 1, 2 B + 1."""
	S, T, _ = kernel_constants()
	W, B = 64 * S, T * S
	return tuple(sorted(set(list(range(1, S + 2)) + [W - 1, W, W + 1, B - 1, B, B + 1, 2 * B + 1])))


def seam_row_counts():
	"""1 ... 9 (every remainder of the loop's unrolling by four, twice), and around the row-group size G: a group short of one row, a full
	one, a group and a row, two groups and a row."""
	_, _, G = kernel_constants()
	return tuple(sorted(set(list(range(1, 10)) + [G - 1, G, G + 1, 2 * G + 1])))


@functools.lru_cache(maxsize=None)
def corpus():
	"""The items every GPU test of the forms runs: (name, graph, rows, window)."""
	S, T, G = kernel_constants()
	B = T * S
	items = list(PM.corpus())
	taken = {i.name for i in items}
	for V in seam_site_counts():
		if "sites_%d" % V not in taken:
			items.append(Item("sites_%d" % V, PM.sites_graph_of(V), PM.SITE_ROWS))
	for n in seam_row_counts():
		if "rows_%d" % n not in taken:
			items.append(Item("rows_%d" % n, PM.row_count_graph(), PM.row_count_rows(n)))
	# rows with cuts and a repeated row over more than a wave of sites; two row groups and a row over two workgroups of sites
	g = PM.sites_graph_of(64 * S + 1)
	items.append(Item("cuts", g, PM.SITE_ROWS + PM.cut_rows(g)))
	g = PM.sites_graph_of(B + 1, n_copies=9, seed=4)
	items.append(Item("two_blocks_three_groups", g, CM.repeated([0, 1, 2, PLOIDY_MAX, 3, 4, 5, 6, 7, 8, 3] + PM.cut_rows(g), 2 * G + 1)))
	names = [i.name for i in items]
	assert len(set(names)) == len(names)
	return items
