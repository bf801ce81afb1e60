"""The model of the site LD (include/v2m_hip.h, "site LD"): numpy over the aligned rows of the column counts' model
(tests/column_counts_model.py: matrix(g, rows, window), the CPU oracle's bodies) and the classes of the pair distances' model.

sites() applies the header's site rule to the class counts; pair_counts() makes the four integer matrices by brute force over every
row; reported() compares D^2 min_r2_den against min_r2_num den with Python's integers, which never round.  expected() returns the site
records, the reported pairs in the order (s, t) and the number of candidates, as Context.site_ld reports them.

graph_from_choice() makes graphs of biallelic sites from a matrix of what every copy holds at every site (the reference base, the
other base, or a byte that is missing data), ld_graph() a small one with the pairs a random graph rarely holds, random_graph() graphs of
a chosen number of sites with founders behind them, so that r^2 takes many values.  corpus() is what tests/test_gpu_site_ld.py runs,
kept here so that tests/test_site_ld_host.py can assert what it holds; wide_items() are batches of 4 160 and 32 768 rows, where the two
sides of the threshold pass 2^64, and band_items() 581 sites under windows of 4 to 10 tiles a strip."""

import functools
import math
import os
import re

import numpy as np

import column_counts_model as CM
import oracle
import pair_distances_model as PM

PLOIDY_MAX = PM.PLOIDY_MAX
LD_KERNELS_HPP = os.path.join(PM.ROOT, "vcf2multialign_amd", "csrc", "ld_kernels.hpp")
MAX_WINDOW = 4096
SITE_DTYPE = np.dtype([("column", "<u8"), ("class_lo", "<u4"), ("class_hi", "<u4"), ("count_lo", "<u4"), ("count_hi", "<u4")])
PAIR_DTYPE = np.dtype([("site_a", "<u4"), ("site_b", "<u4"), ("n", "<u4"), ("n_a", "<u4"), ("n_b", "<u4"), ("n_ab", "<u4")])


@functools.lru_cache(maxsize=None)
def kernel_constants():
	"""(T, C): kLdTile, the sites per side of a workgroup's tile, and kLdChunkWords, the 64-row words per LDS chunk, read from
	csrc/ld_kernels.hpp."""
	with open(LD_KERNELS_HPP) as f:
		text = f.read()
	out = []
	for name in ("kLdTile", "kLdChunkWords"):
		found = re.findall(r"^constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text, re.M)
		assert len(found) == 1, "%s: %d definitions of the form `constexpr int %s = value;`" % (name, len(found), name)
		out.append(int(found[0]))
	return tuple(out)


class Params:
	"""v2m_site_ld_params, with min_r2 as (numerator, denominator)."""
	def __init__(self, window_sites=MAX_WINDOW, window_columns=0, min_r2=(1, 5), min_allele_count=1):
		self.window_sites, self.window_columns, self.min_r2, self.min_allele_count = window_sites, window_columns, min_r2, min_allele_count

	def kwargs(self):
		return dict(window_sites=self.window_sites, window_columns=self.window_columns, min_r2=self.min_r2, min_allele_count=self.min_allele_count)

	def __repr__(self):
		return "w%d_c%d_r%d_%d_m%d" % (self.window_sites, self.window_columns, self.min_r2[0], self.min_r2[1], self.min_allele_count)


# ---- the rule ------------------------------------------------------------------------------------------------------------------------------

def sites(cls, min_allele_count=1, first_column=0):
	"""The site records of the classes cls[n, L]: the columns where exactly two of the classes 0-3 have a non-zero count and both counts
	reach min_allele_count."""
	n, L = cls.shape
	counts = np.stack([(cls == k).sum(axis=0) for k in range(4)], axis=1).astype(np.int64) if n else np.zeros((L, 4), dtype=np.int64)
	out = []
	for col in range(L):
		present = [k for k in range(4) if counts[col, k]]
		if len(present) == 2 and all(counts[col, k] >= min_allele_count for k in present):
			lo, hi = present
			out.append((first_column + col, lo, hi, counts[col, lo], counts[col, hi]))
	return np.array(out, dtype=SITE_DTYPE)


def planes(cls, records, first_column=0):
	"""(called, carries), bool[n, V]: the row's class at the site is lo or hi; it is hi."""
	cols = records["column"].astype(np.int64) - first_column
	at = cls[:, cols]
	carries = at == records["class_hi"].astype(np.uint8)[None, :]
	return carries | (at == records["class_lo"].astype(np.uint8)[None, :]), carries


def pair_counts(called, carries):
	"""(n, n_a, n_b, n_ab), int64[V, V] each, entry [s, t]: by brute force over every row."""
	ca, ka = called.astype(np.int64), carries.astype(np.int64)
	return ca.T @ ca, ka.T @ ca, ca.T @ ka, ka.T @ ka


def d_and_den(n, n_a, n_b, n_ab):
	n, n_a, n_b, n_ab = int(n), int(n_a), int(n_b), int(n_ab)
	return n * n_ab - n_a * n_b, n_a * (n - n_a) * n_b * (n - n_b)


def is_reported(n, n_a, n_b, n_ab, min_r2):
	d, den = d_and_den(n, n_a, n_b, n_ab)
	return den != 0 and d * d * int(min_r2[1]) >= int(min_r2[0]) * den


def candidates(records, params):
	"""[(s, t)] ascending: s < t, t - s <= window_sites and, unless window_columns is 0, column[t] - column[s] <= window_columns."""
	cols = [int(c) for c in records["column"]]
	out = []
	for s in range(len(cols)):
		for t in range(s + 1, min(len(cols), s + params.window_sites + 1)):
			if params.window_columns == 0 or cols[t] - cols[s] <= params.window_columns:
				out.append((s, t))
	return out


def evaluate(cls, params, first_column=0):
	"""(site records, pair records of EVERY candidate, bool[candidates] reported) of the classes cls[n, L]."""
	records = sites(cls, params.min_allele_count, first_column)
	called, carries = planes(cls, records, first_column)
	n, n_a, n_b, n_ab = pair_counts(called, carries)
	cand = candidates(records, params)
	pairs = np.array([(s, t, n[s, t], n_a[s, t], n_b[s, t], n_ab[s, t]) for s, t in cand], dtype=PAIR_DTYPE)
	keep = np.array([is_reported(n[s, t], n_a[s, t], n_b[s, t], n_ab[s, t], params.min_r2) for s, t in cand], dtype=bool)
	return records, pairs, keep


def evaluate_arrays(cls, params, first_column=0):
	"""evaluate() without its loops over the pairs, for the bands of many tiles (band_items(): 170 000 candidates): the candidates from
	the index pairs above the diagonal, which numpy lists in the order (s, t), and the rule on arrays of Python's integers (dtype
	object), which round no more than is_reported() does.  tests/test_site_ld_host.py holds it equal to evaluate() on every item of
	corpus() and wide_items()."""
	records = sites(cls, params.min_allele_count, first_column)
	called, carries = planes(cls, records, first_column)
	counts = pair_counts(called, carries)
	cols = records["column"].astype(np.int64)
	s, t = np.triu_indices(len(records), k=1)
	ok = t - s <= params.window_sites
	if params.window_columns:
		ok &= cols[t] - cols[s] <= params.window_columns
	s, t = s[ok], t[ok]
	pairs = np.zeros(len(s), dtype=PAIR_DTYPE)
	pairs["site_a"], pairs["site_b"] = s, t
	for name, c in zip(("n", "n_a", "n_b", "n_ab"), counts):
		pairs[name] = c[s, t]
	n, n_a, n_b, n_ab = (c[s, t].astype(object) for c in counts)
	d, den = n * n_ab - n_a * n_b, n_a * (n - n_a) * n_b * (n - n_b)
	keep = (den != 0).astype(bool) & (d * d * int(params.min_r2[1]) >= int(params.min_r2[0]) * den).astype(bool)
	return records, pairs, keep


@functools.lru_cache(maxsize=None)
def _expected(item):
	m = CM.matrix(item.g, item.rows, item.window)
	records, pairs, keep = (evaluate_arrays if item.arrays else evaluate)(PM.classes(m), item.params, item.window[0] if item.window else 0)
	return records, pairs[keep], len(pairs), m.shape[1]


def expected(item):
	"""(sites, pairs, n_candidates, n_columns) as Context.site_ld reports them for an item of the corpus.  Computed once per item."""
	return _expected(item)


def r2_text(pair):
	d, den = d_and_den(pair["n"], pair["n_a"], pair["n_b"], pair["n_ab"])
	return "%.6f" % (float(d * d) / float(den))


def text(g, n_rows, n_columns, records, pairs, params):
	"""What --output-ld writes."""
	num, den = params.min_r2
	lines = ["#rows\t%d\tcolumns\t%d\tsites\t%d\tpairs\t%d\twindow\t%d\twindow_columns\t%d\tmin_r2\t%d/%d\tmin_count\t%d"
		% (n_rows, n_columns, len(records), len(pairs), params.window_sites, params.window_columns, num, den, params.min_allele_count),
		"#column_a\tpos_a\tcolumn_b\tpos_b\tn\tn_a\tn_b\tn_ab\tr2"]
	def where(site):
		col = int(records["column"][site])
		p = CM.reference_position(g, col)
		return [str(col), "." if p is None else str(p)]
	for p in pairs:
		lines.append("\t".join(where(int(p["site_a"])) + where(int(p["site_b"])) + [str(int(p[k])) for k in ("n", "n_a", "n_b", "n_ab")] + [r2_text(p)]))
	return ("\n".join(lines) + "\n").encode()


def file_text(g, rows, window, params):
	"""What --output-ld writes for `rows`."""
	m = CM.matrix(g, rows, window)
	records, pairs, keep = evaluate(PM.classes(m), params, window[0] if window else 0)
	return text(g, len(rows), m.shape[1], records, pairs[keep], params)


# ---- graphs of biallelic sites -------------------------------------------------------------------------------------------------------------

REF_BASES = b"ACGTacgt"          # the reference's byte at site k is REF_BASES[k % 8] ...
ALT_BASES = b"CGTAgtac"          # ... and its first edge's label ALT_BASES[k % 8], of another class: at sites 3, 6, 7 mod 8 the REFERENCE carries
MISSING = [b"N", b"-", b"R", b"n", bytes([0xC1]), b"@"]   # the second edge's label: a byte of the classes N, gap and other


def graph_from_choice(choice, spacing=1, name="choice"):
	"""A reference with a site every `spacing` bases ('A' between them).  Site k has two one-base edges to the next node: the first
	labelled with its other base, the second with a byte that is missing data.  choice[c, k] says what copy c holds there: 0 the
	reference's base, 1 the other base, 2 the missing byte."""
	choice = np.asarray(choice, dtype=np.int64)
	n_copies, n_sites = choice.shape
	assert n_sites >= 1
	k = np.arange(n_sites, dtype=np.int64)
	pos = np.unique(np.r_[k * spacing, k * spacing + 1, n_sites * spacing]).astype(np.int64)
	site_node = np.searchsorted(pos, k * spacing)
	n_edges_of = np.zeros(len(pos), dtype=np.int64)
	n_edges_of[site_node] = 2
	csum = np.r_[0, np.cumsum(n_edges_of)]
	first_edge = csum[site_node]
	E = int(csum[-1])
	targets = np.zeros(E, dtype=np.int64)
	targets[first_edge] = site_node + 1
	targets[first_edge + 1] = site_node + 1
	labels = []
	for s in range(n_sites):
		labels += [ALT_BASES[s % 8:s % 8 + 1], MISSING[s % len(MISSING)]]
	label_offsets = np.arange(E + 1, dtype=np.int64)
	ep, hp = max(64, (E + 63) // 64 * 64), max(64, (n_copies + 63) // 64 * 64)
	bits = np.zeros((hp, ep), dtype=bool)
	for c in range(n_copies):
		bits[c, first_edge[choice[c] == 1]] = True
		bits[c, first_edge[choice[c] == 2] + 1] = True
	words = np.packbits(bits, axis=1, bitorder="little").view("<u8").reshape(-1).copy()
	g = oracle.graph_from_arrays(pos, pos.copy(), targets, csum, label_offsets, b"".join(labels), words, ep, hp, ["S"], [0, n_copies])
	ref = bytearray(b"A" * int(pos[-1]))
	for s in range(n_sites):
		ref[s * spacing] = REF_BASES[s % 8]
	g.ref = bytes(ref)
	g.name = name
	g.site_columns = pos[site_node]
	g.choice = choice
	return g


LD_CHOICE = np.array([
	# copy: 0  1  2  3  4  5  6  7
	[1, 1, 1, 1, 0, 0, 0, 0],      # site 0
	[1, 1, 1, 1, 0, 0, 0, 0],      # site 1: in perfect LD with site 0 (D > 0)
	[0, 0, 0, 0, 1, 1, 1, 1],      # site 2: in perfect LD with both (D < 0)
	[1, 1, 1, 0, 0, 0, 0, 0],      # site 3: differs from site 0 in one row only
	[2, 2, 2, 2, 1, 1, 0, 0],      # site 4: missing wherever site 0 has its other base: the rows called at both are monomorphic at sites 0-2 (den = 0)
	[1, 0, 1, 0, 1, 0, 1, 0],      # site 5: D = 0 against sites 0-2
	[1, 2, 0, 1, 2, 0, 0, 1],      # site 6: missing rows among the called ones
]).T


@functools.lru_cache(maxsize=None)
def ld_graph():
	return graph_from_choice(LD_CHOICE, name="ld_graph")


LD_ROWS = list(range(8))
N_COPIES = 12


@functools.lru_cache(maxsize=None)
def random_graph(n_sites, seed=1, spacing=1):
	"""N_COPIES copies made of three founders in blocks of sites, with a base flipped here and there and one byte in ten missing: r^2 takes
	many values.  Copies k, k + 1 (mod N_COPIES) hold the other base at site k and copies k + 2, k + 3 the reference's, so that a batch of
	all copies has exactly n_sites sites under min_allele_count 1 and 2."""
	rng = np.random.default_rng(seed)
	founders = rng.integers(0, 2, size=(3, n_sites))
	choice = np.zeros((N_COPIES, n_sites), dtype=np.int64)
	for c in range(N_COPIES):
		owner = np.repeat(rng.integers(0, 3, size=n_sites // 8 + 1), 8)[:n_sites]
		choice[c] = founders[owner, np.arange(n_sites)]
		flip = rng.random(n_sites) < 0.08
		choice[c][flip] ^= 1
		choice[c][rng.random(n_sites) < 0.1] = 2
	for k in range(n_sites):
		choice[k % N_COPIES, k] = choice[(k + 1) % N_COPIES, k] = 1
		choice[(k + 2) % N_COPIES, k] = choice[(k + 3) % N_COPIES, k] = 0
	return graph_from_choice(choice, spacing, "random_%d_%d_%d" % (n_sites, seed, spacing))


def cut_rows(g, seed=3):
	"""Rows with cuts: every edge ends at the node behind its own, so a row may switch copies at any node."""
	n_nodes, H = len(g.aligned_positions), g.total_chromosome_copies
	if n_nodes < 4:
		return []
	rng = np.random.default_rng(seed)
	rows = []
	for k in (1, 2, 5):
		cuts = [0] + sorted(int(x) for x in rng.choice(np.arange(1, n_nodes - 1), size=min(k, n_nodes - 2), replace=False))
		rows.append(list(zip(cuts, [int(x) for x in rng.integers(0, H, size=len(cuts))])))
	return rows


def all_rows(g):
	"""Every copy, the reference, a repeated row and rows with cuts."""
	return list(range(N_COPIES)) + [PLOIDY_MAX, 3] + cut_rows(g)


# ---- the corpus of the GPU tests -----------------------------------------------------------------------------------------------------------

class Item:
	def __init__(self, name, g, rows, params=None, window=None, arrays=False):
		self.name, self.g, self.rows, self.params, self.window, self.arrays = name, g, rows, params or Params(), window, arrays   # arrays: expected() goes through evaluate_arrays()

	def __repr__(self):
		return self.name


def site_counts():
	T, _ = kernel_constants()
	return (1, 2, T - 1, T, T + 1, 2 * T + 1)


def window_sizes():
	T, _ = kernel_constants()
	return (1, T - 1, T, T + 1, 2 * T + 1, MAX_WINDOW)      # 2 T + 1 >= V of the graph they run over


def row_counts():
	_, C = kernel_constants()
	return (1, 2, 63, 64, 65, 64 * C - 1, 64 * C, 64 * C + 1, 128 * C + 1)


@functools.lru_cache(maxsize=None)
def window_graph():
	return random_graph(30, seed=5, spacing=5)


def windows():
	"""Over window_graph(): begin and end at every residue mod 4, a site on the first and on the last column of the window, and windows
	without a site."""
	g = window_graph()
	col = [int(c) for c in g.site_columns]
	out = [(col[2] + i, col[20] + j) for i, j in ((0, 1), (1, 2), (2, 3), (3, 4))]       # col[2] + 0: a site on the first column; col[20] + 1 - 1: on the last
	out += [(col[5], col[9] + 1), (col[7] + 1, col[8]), (g.aligned_length - 3, g.aligned_length)]
	return out


def lowest_terms(pair):
	d, den = d_and_den(pair["n"], pair["n_a"], pair["n_b"], pair["n_ab"])
	f = math.gcd(d * d, den)
	return d * d // f, den // f


def tie_threshold(g, rows):
	"""(numerator, denominator) of a realised pair's D^2 / den in lowest terms, strictly inside (0, 1) with a denominator the
	parameters take: the one nearest to 1/2 in the graph."""
	_, pairs, _ = evaluate(PM.classes(CM.matrix(g, rows)), Params(min_r2=(0, 1)))
	found = []
	for p in pairs:
		if d_and_den(p["n"], p["n_a"], p["n_b"], p["n_ab"])[1]:
			num, den = lowest_terms(p)
			if 0 < num < den <= 1000000:
				found.append((abs(2 * num - den) / den, num, den))
	assert found
	return min(found)[1:]


@functools.lru_cache(maxsize=None)
def corpus():
	"""The items every GPU test of the forms runs."""
	T, C = kernel_constants()
	items = [Item(CM.hostile_graph(s).name, CM.hostile_graph(s), CM.HOSTILE_ROWS, Params(min_r2=(0, 1))) for s in CM.HOSTILE_SHIFTS]
	items.append(Item("all_other", CM.other_graph(), [PLOIDY_MAX, 0, 1]))
	items.append(Item("pm_sites", PM.row_count_graph(), list(range(12))))
	# thresholds over the graph of special pairs and a random one, a tie of each among them
	for name, g, rows in (("ld_graph", ld_graph(), LD_ROWS), ("random_40", random_graph(40, seed=2), all_rows(random_graph(40, seed=2)))):
		for min_r2 in ((0, 1), (1, 1), (1, 5), tie_threshold(g, rows)):
			items.append(Item("%s_r2_%d_%d" % (name, min_r2[0], min_r2[1]), g, rows, Params(min_r2=min_r2)))
	# sites
	items.append(Item("sites_0", random_graph(20), [PLOIDY_MAX] * 3))
	for V in site_counts():
		g = random_graph(V)
		items.append(Item("sites_%d" % V, g, all_rows(g)))
	# the band
	g = random_graph(2 * T + 1)
	for w in window_sizes():
		items.append(Item("window_sites_%d" % w, g, all_rows(g), Params(window_sites=w)))
	# rows
	g = random_graph(T + 1, seed=3)
	for n in row_counts():
		items.append(Item("rows_%d" % n, g, CM.repeated(all_rows(g), n), Params(window_sites=T)))
	# the column distance: that of sites 3 and 9 of a graph with a site every three bases, and one less
	g = random_graph(T + 6, seed=4, spacing=3)
	reach = int(g.site_columns[9] - g.site_columns[3])
	for wc in (reach, reach - 1):
		items.append(Item("window_columns_%d" % wc, g, all_rows(g), Params(window_columns=wc)))
	items.append(Item("window_columns_and_sites", g, all_rows(g), Params(window_sites=4, window_columns=reach)))
	# the allele count: half of the copies, so that many sites hold an allele once
	g = random_graph(T + 1, seed=3)
	for mac in (1, 2):
		items.append(Item("min_count_%d" % mac, g, list(range(0, N_COPIES, 2)), Params(min_allele_count=mac)))
	# column windows
	g = window_graph()
	items += [Item("window_%d_%d" % w, g, all_rows(g), Params(min_r2=(1, 10)), w) for w in windows()]
	names = [i.name for i in items]
	assert len(set(names)) == len(names)
	return items


@functools.lru_cache(maxsize=None)
def row_words_item():
	"""64 * 5 + 7 rows over the graph of the row counts: six 64-row words, the last one ragged, for ld_pack_kernel's groups of several
	words (tests/test_gpu_site_ld.py: V2M_SITE_LD_WORDS_PER_GROUP).  The rows repeat with period 17, which no word is a multiple of."""
	T, _ = kernel_constants()
	g = random_graph(T + 1, seed=3)
	rows = CM.repeated(all_rows(g), 64 * 5 + 7)
	assert len(all_rows(g)) == 17 and (len(rows) + 63) // 64 == 6 and len(rows) % 64 == 7
	return Item("row_words_%d" % len(rows), g, rows, Params(window_sites=T))


# ---- batches of 4 160 to 32 768 rows: the threshold's two products beyond 64 bits -----------------------------------------------------------

WIDE_CHOICE = np.array([
	# copy: 0  1  2  3  4  5
	[0, 1, 0, 1, 2, 0],      # site 0
	[0, 0, 1, 1, 1, 2],      # site 1: copies 0-3 hold (0,0), (1,0), (0,1), (1,1) at sites (0, 1); copy 4 is missing at site 0, copy 5 at site 1
	[1, 0, 1, 0, 1, 1],      # site 2: site 0 with its two bases exchanged: against site 1 the same den and D of the other sign
	[0, 1, 1, 0, 0, 1],      # site 3: differs where exactly one of sites 0 and 1 holds its other base
	[0, 0, 1, 1, 0, 1],      # site 4: site 1 with every copy called
]).T


@functools.lru_cache(maxsize=None)
def wide_graph():
	return graph_from_choice(WIDE_CHOICE, name="wide_graph")


# (name, (c00, c10, c01, c11): how often copies 0-3 occur, (copies 4, 5), min_r2 as Context.site_ld gets it, NOT in lowest terms).
# At sites (0, 1): n = c00 + c10 + c01 + c11, n_a = c10 + c11, n_b = c01 + c11, n_ab = c11 and D = c00 c11 - c10 c01.
WIDE_TABLES = (
	("r1", (138, 22801, 7297, 2532), (0, 0), (333333, 1000000)),
	("r2", (16716, 1931, 8117, 6004), (0, 0), (999999, 1000000)),
	("r3a", (31921, 78, 413, 356), (0, 0), (333333, 1000000)),
	("r3b", (32326, 240, 39, 163), (0, 0), (333333, 1000000)),
	("tie_quarter", (12288, 4096, 4096, 12288), (0, 0), (250000, 1000000)),            # D = 2^27, den = 2^56: r^2 = 1/4
	("tie_quarter_above", (12289, 4095, 4096, 12288), (0, 0), (250000, 1000000)),      # one row from copy 1 to copy 0
	("tie_quarter_below", (12287, 4097, 4096, 12288), (0, 0), (250000, 1000000)),      # one row from copy 0 to copy 1
	("tie_one", (16384, 0, 0, 16384), (0, 0), (1000000, 1000000)),                     # r^2 = 1: nothing lies above it
	("tie_one_below", (16383, 1, 0, 16384), (0, 0), (1000000, 1000000)),
	("missing", (1900, 14727, 13182, 2448), (300, 211), (333333, 1000000)),            # 32 768 rows, n = 32 257 at sites (0, 1)
	("rows_4160_r1", (2080, 1, 0, 2079), (0, 0), (500000, 1000000)),                   # 65 row words: the ninth LDS chunk holds one word
	("rows_4160_r3b", (2070, 0, 1, 2089), (0, 0), (999999, 1000000)),
)
WIDE_MAX_ROWS = 32768


@functools.lru_cache(maxsize=None)
def wide_items():
	"""Batches over wide_graph() whose rows are its six copies, each as often as WIDE_TABLES says, in a fixed random order: D^2 min_r2_den
	and min_r2_num den pass 2^64 (from about 4 145 rows on with a denominator of 10^6), which no batch of corpus() reaches."""
	items = []
	for k, (name, table, missing, min_r2) in enumerate(WIDE_TABLES):
		rows = np.repeat(np.arange(6), list(table) + list(missing))
		rows = [int(r) for r in np.random.default_rng(100 + k).permutation(rows)]
		item = Item("wide_%s" % name, wide_graph(), rows, Params(min_r2=min_r2))
		item.table, item.missing = table, missing
		items.append(item)
	return items


# ---- bands of 4 to 10 tiles over 10 strips -------------------------------------------------------------------------------------------------

DEFAULT_WINDOW = 1000      # Context.site_ld's and --ld-window's


def band_sites():
	T, _ = kernel_constants()
	return 9 * T + 5


def band_windows():
	T, _ = kernel_constants()
	return (3 * T, 3 * T + 1, 4 * T + 1, 8 * T, 8 * T + 1, DEFAULT_WINDOW, MAX_WINDOW)


BAND_THRESHOLDS = ((0, 1), (1, 5))      # every candidate with den != 0; few enough that whole tiles of a band hold no pair


@functools.lru_cache(maxsize=None)
def band_items():
	"""band_sites() sites (10 strips) under windows that reach 4, 5, 6, 9 and all 10 tiles of a strip, and one graph with a site every
	three bases whose window_columns ends inside the farthest tile of window_sites."""
	T, _ = kernel_constants()
	g = random_graph(band_sites(), seed=6)
	items = [Item("band_w%d_r2_%d_%d" % (w, r2[0], r2[1]), g, all_rows(g), Params(window_sites=w, min_r2=r2), arrays=True) for w in band_windows() for r2 in BAND_THRESHOLDS]
	g = random_graph(band_sites(), seed=7, spacing=3)
	reach = int(g.site_columns[4 * T + 30] - g.site_columns[0])      # window_sites 5 T: the sixth tile holds the distances 4 T + 1 to 5 T
	items.append(Item("band_columns_%d" % reach, g, all_rows(g), Params(window_sites=5 * T, window_columns=reach, min_r2=(0, 1)), arrays=True))
	return items


def strips_and_blocks(n_sites, window_sites):
	"""(n_strips, n_blocks) as include/v2m_hip.h and csrc/ld_kernels.hpp say them: strips of T sites, and per strip the tiles its band
	reaches, the strip's own and ceil(window_sites / T) more, at most all strips."""
	T, _ = kernel_constants()
	n_strips = -(-n_sites // T)
	return n_strips, min(n_strips, -(-window_sites // T) + 1)
