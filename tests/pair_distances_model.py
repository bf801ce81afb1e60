"""The model of the pair distances (include/v2m_hip.h, "pair distances"): numpy over the aligned rows of the column counts' model
(tests/column_counts_model.py: matrix(g, rows, window), the CPU oracle's bodies).

classes() applies the header's rule to the bytes; distances() compares every two rows over ALL columns of the view, by brute force;
sites() are the variable columns as the column counts define them.  One fact carries the library's design and is stated here so that
tests/test_pair_distances_host.py can hold the model to it: a column where one class holds every row adds 0 to every pair under both
definitions, so distances(cls[:, sites]) == distances(cls).

sites_graph() makes graphs in which all seven classes meet in pairs, from flat arrays (oracle.graph_from_arrays) as
column_counts_model.hostile_graph is made; corpus() is what tests/test_gpu_pair_distances.py runs, kept here so that the host tests can
assert what it holds."""

import functools
import itertools
import os
import re

import numpy as np

import column_counts_model as CM
import oracle

PLOIDY_MAX = oracle.PLOIDY_MAX
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DISTANCE_KERNELS_HPP = os.path.join(ROOT, "vcf2multialign_amd", "csrc", "distance_kernels.hpp")


@functools.lru_cache(maxsize=None)
def kernel_constants():
	"""(T, C): kPairTile, the rows per side of a workgroup's tile, and kPairChunkWords, the 64-bit site words per LDS chunk, read from
	csrc/distance_kernels.hpp."""
	with open(DISTANCE_KERNELS_HPP) as f:
		text = f.read()
	out = []
	for name in ("kPairTile", "kPairChunkWords"):
		found = re.findall(r"^constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text, re.M)
		assert len(found) == 1, "%s: %d definitions of the form `constexpr int %s = value;`" % (name, len(found), name)
		out.append(int(found[0]))
	return tuple(out)


# ---- the rule ------------------------------------------------------------------------------------------------------------------------------

def classes(m):
	"""u8, the shape of m: 0-3 A, C, G, T and 4 N (either case: exactly the two ASCII letters), 5 gap ('-' exactly), 6 other."""
	m = np.asarray(m, dtype=np.uint8)
	low = m | 0x20
	cls = np.full(m.shape, 6, dtype=np.uint8)
	for k, c in enumerate("acgtn"):
		cls[low == ord(c)] = k
	cls[m == 0x2D] = 5
	return cls


def distances(cls, acgt_only=False):
	"""u32[n, n] over every column of cls[n, L]: the columns where two rows' classes differ; acgt_only: where both are in 0-3 and differ."""
	n = cls.shape[0]
	d = np.zeros((n, n), dtype=np.uint32)
	base = cls < 4
	for i in range(n):
		diff = cls != cls[i]
		if acgt_only:
			diff &= base & base[i]
		d[i] = diff.sum(axis=1)
	return d


def sites(m):
	"""bool[L]: the variable columns, as the column counts define them (none of the seven classes holds every row)."""
	return CM.variable(CM.counts(m), m.shape[0])


def expected(g, rows, window=None, acgt_only=False):
	"""(dist, n_sites, n_columns) as Context.pair_distances reports them."""
	m = CM.matrix(g, rows, window)
	return distances(classes(m), acgt_only), int(sites(m).sum()) if len(rows) else 0, m.shape[1]


def text(ids, dist, n_columns, n_sites, acgt_only=False):
	n = len(ids)
	lines = ["#rows\t%d\tcolumns\t%d\tsites\t%d\tmodel\t%s" % (n, n_columns, n_sites, "acgt" if acgt_only else "all"), "\t".join(["id"] + list(ids))]
	for i in range(n):
		lines.append("\t".join([ids[i]] + [str(int(x)) for x in np.asarray(dist).reshape(n, n)[i]]))
	return ("\n".join(lines) + "\n").encode()


def haplotype_ids(g, omit_reference=False):
	"""(ids, rows) of --haplotypes: the rows of the A2M output under the names --output-paf writes."""
	ids, rows = ([], []) if omit_reference else (["REF"], [PLOIDY_MAX])
	for s, sample in enumerate(g.sample_names):
		for c in range(int(g.ploidy_csum[s + 1]) - int(g.ploidy_csum[s])):
			ids.append("%s.%d" % (sample, 1 + c))
			rows.append(int(g.ploidy_csum[s]) + c)
	return ids, rows


def file_text(g, ids, rows, window=None, acgt_only=False):
	"""What --output-distances writes for `rows` named `ids`."""
	d, v, L = expected(g, rows, window, acgt_only)
	return text(ids, d, L, v, acgt_only)


# ---- graphs of sites -----------------------------------------------------------------------------------------------------------------------

# one byte per class but A, in two spellings; a site's two edges carry a pair of them, and the reference holds 'A'
SPELLINGS = ((b"C", b"G", b"T", b"N", b"-", b"R"), (b"c", b"g", b"t", b"n", b"-", bytes([0xC1])))
CLASS_PAIRS = list(itertools.combinations(range(6), 2))      # the 15 pairs of the six
TWO_BYTE_EVERY = 11                                           # sites 3, 14, 25, ... may carry a two-byte label
SECOND_BYTES = b"aCgTnR"


def sites_graph(n_sites, n_copies, seed, spacing=1, n_two_byte=None):
	"""A reference of 'A's with a site every `spacing` bases.  Site k has two one-base edges to the next node whose labels are a pair of the
	six classes but A (pair k % 15, in upper case for even k // 15 and in lower case / as another "other" byte for odd), so its column
	holds three classes; the first n_two_byte sites with k % 11 == 3 (default: all of them) have ONE edge with a two-byte label instead,
	whose second byte makes a padding column that holds a class or '-'.  Copy 0 takes every site's first edge, copy 1 none, copy 2
	every site's last edge; the others choose at random among none, first and last.  So a batch that holds copies 0 and 1 has exactly
	n_sites + n_two_byte variable columns (variable_columns())."""
	rng = np.random.default_rng(seed)
	k = np.arange(n_sites, dtype=np.int64)
	slots = np.flatnonzero(k % TWO_BYTE_EVERY == 3)
	two = np.zeros(n_sites, dtype=bool)
	two[slots if n_two_byte is None else slots[:n_two_byte]] = True
	assert n_two_byte is None or int(two.sum()) == n_two_byte
	# nodes: a site's node, the node its edges end at (the next site's when spacing is 1), and the sink
	pos = np.unique(np.r_[k * spacing, k * spacing + 1, n_sites * spacing]).astype(np.int64)
	site_node = np.searchsorted(pos, k * spacing)
	width = np.diff(pos)                                       # the reference bases of every node but the sink
	aligned_width = width.copy()
	aligned_width[site_node[two]] = 2                          # (a site's node holds one base: spacing >= 1 and its edges end one base on)
	aligned = np.r_[0, np.cumsum(aligned_width)]
	n_edges_of = np.zeros(len(pos), dtype=np.int64)
	n_edges_of[site_node] = np.where(two, 1, 2)
	csum = np.r_[0, np.cumsum(n_edges_of)]                     # [nodes + 1]
	first_edge = csum[site_node]
	E = int(csum[-1])
	targets = np.zeros(E, dtype=np.int64)
	targets[first_edge] = site_node + 1
	targets[(first_edge + 1)[~two]] = site_node[~two] + 1
	labels, lengths = [], np.zeros(E, dtype=np.int64)
	for s in range(n_sites):
		if two[s]:
			labels.append(SPELLINGS[(s // 15) & 1][s % 6] + SECOND_BYTES[s % 6:s % 6 + 1])
		else:
			a, b = CLASS_PAIRS[s % 15]
			spell = SPELLINGS[(s // 15) & 1]
			labels += [spell[a], spell[b]]
	lengths[:] = [len(x) for x in labels]
	label_offsets = np.r_[0, np.cumsum(lengths)]
	ep, hp = max(64, (E + 63) // 64 * 64), max(64, (n_copies + 63) // 64 * 64)
	bits = np.zeros((hp, ep), dtype=bool)
	last_edge = first_edge + np.where(two, 0, 1)
	for c in range(n_copies):
		choice = np.full(n_sites, (1, 0, 2)[c], dtype=np.int64) if c < 3 else rng.integers(0, 3, size=n_sites)
		bits[c, first_edge[choice == 1]] = True
		bits[c, last_edge[choice == 2]] = True
	words = np.packbits(bits, axis=1, bitorder="little").view("<u8").reshape(-1).copy()
	g = oracle.graph_from_arrays(pos, aligned, targets, csum, label_offsets, b"".join(labels), words, ep, hp, ["S"], [0, n_copies])
	g.ref = b"A" * int(pos[-1])
	g.name = "sites_%d_%d_%d_%d" % (n_sites, n_copies, seed, spacing)
	g.site_columns = aligned[site_node]                        # the column of every site's first byte
	g.two_byte = two
	g.site_nodes = site_node
	return g


def variable_columns(g):
	"""The variable columns of a batch that holds copies 0 and 1 of a sites_graph."""
	return len(g.site_columns) + int(g.two_byte.sum())


def sites_graph_of(V, n_copies=7, seed=1):
	"""A sites_graph with exactly V variable columns (V // 12 of them a two-byte label's padding column)."""
	t = V // 12
	g = sites_graph(V - t, n_copies, seed, n_two_byte=t)
	assert variable_columns(g) == V
	return g


def cut_rows(g, seed=3):
	"""Rows with cuts over a sites_graph: every edge ends at the node behind its own, so a row may switch copies at any node."""
	n_nodes, H = len(g.aligned_positions), g.total_chromosome_copies
	rng = np.random.default_rng(seed)
	rows = []
	for k in (1, 2, 5):
		cuts = [0] + sorted(int(x) for x in rng.choice(np.arange(1, n_nodes - 1), size=min(k, n_nodes - 2), replace=False))
		rows.append(list(zip(cuts, [int(x) for x in rng.integers(0, H, size=len(cuts))])))
	return rows


# ---- the corpus of the GPU tests -----------------------------------------------------------------------------------------------------------

class Item:
	def __init__(self, name, g, rows, window=None):
		self.name, self.g, self.rows, self.window = name, g, rows, window

	def __repr__(self):
		return self.name


@functools.lru_cache(maxsize=None)
def row_count_graph():
	return sites_graph(40, 12, 11)


def row_count_rows(n):
	g = row_count_graph()
	return CM.repeated([0, 1, PLOIDY_MAX] + list(range(2, 12)) + cut_rows(g), n)


def row_counts():
	T, _ = kernel_constants()
	return (1, 2, T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 3 * T + 1)


def site_counts():
	_, C = kernel_constants()
	return (1, 63, 64, 65, 64 * C - 1, 64 * C, 64 * C + 1)


SITE_ROWS = [0, 1, 2, PLOIDY_MAX, 3, 4, 5, 6, 3]             # a repeated row among them


@functools.lru_cache(maxsize=None)
def window_graph():
	return sites_graph(30, 7, 5, spacing=5)


def windows():
	"""Over window_graph(): begin and end at every residue mod 4, a site on the first and on the last column of the window, and a
	window without a site."""
	g = window_graph()
	col = [int(c) for c in g.site_columns]
	out = [(col[2] + i, col[20] + j) for i, j in ((0, 1), (1, 2), (2, 3), (3, 4))]       # col[2] + 0: a site on the first column; col[20] + 1 - 1: on the last
	out += [(col[5], col[9] + 1), (col[7] + 1, col[8]), (0, 1), (g.aligned_length - 3, g.aligned_length)]
	return out


@functools.lru_cache(maxsize=None)
def corpus():
	"""The items every GPU test of the forms runs: (name, graph, rows, window)."""
	items = [Item(CM.hostile_graph(s).name, CM.hostile_graph(s), CM.HOSTILE_ROWS) for s in CM.HOSTILE_SHIFTS]
	items.append(Item("all_other", CM.other_graph(), [PLOIDY_MAX, 0, 1]))
	items += [Item("rows_%d" % n, row_count_graph(), row_count_rows(n)) for n in row_counts()]
	items.append(Item("sites_0", sites_graph_of(20), [PLOIDY_MAX] * 3))
	items += [Item("sites_%d" % V, sites_graph_of(V), SITE_ROWS) for V in site_counts()]
	items += [Item("window_%d_%d" % w, window_graph(), SITE_ROWS, w) for w in windows()]
	return items


# ---- rows that all differ --------------------------------------------------------------------------------------------------------------------
#
# row_count_rows(n) repeats with period 16, which divides the 16 rows of pack_sites_kernel's smallest row group, the 32 of pair_row()'s
# second half and the 64 of a tile: a row group written one group off, two halves of a tile exchanged or a tile taken for its neighbour
# give the same matrix (tests/test_pair_distances_host.py asserts that, and that the items below tell every one of them).

def distinct_rows(g, n):
	"""n rows over a sites_graph of n copies: the REF row, copy 0, copies 2 ... n - 4 (copy 1 takes no edge and equals REF) and the three
	cut_rows(g), one near the front, one in the middle, one last."""
	rows = [PLOIDY_MAX, 0] + list(range(2, n - 3))
	for at, cut in zip((7, n // 2, n - 1), cut_rows(g)):
		rows.insert(at, cut)
	assert len(rows) == n
	return rows


def distinct_counts():
	"""(rows, variable columns, seed): 3 T + 1 rows are four tiles, the last of one row, with a full tile pair (1, 2) off the diagonal that
	does not touch tile 0, over two chunks of sites and five more; 8 T + 1 rows are 45 tile pairs over a chunk and 70 sites; J B + 64 rows
	(J B: the slots nj_join_kernel takes in one trip) are 17 tiles, 153 tile pairs, over about 60 sites."""
	import nj_tree_model
	T, C = kernel_constants()
	_, B, J = nj_tree_model.kernel_constants()
	return ((3 * T + 1, 2 * 64 * C + 5, 11), (8 * T + 1, 64 * C + 70, 12), (J * B + 64, 60, 13))


@functools.lru_cache(maxsize=None)
def distinct_items():
	"""Items whose rows all differ, in the class matrix and in the expected matrix under both definitions."""
	items = []
	for n, V, seed in distinct_counts():
		g = sites_graph_of(V, n_copies=n, seed=seed)
		items.append(Item("distinct_%d" % n, g, distinct_rows(g, n)))
	return items


def distinct_item(n):
	return next(i for i in distinct_items() if len(i.rows) == n)
