"""The model of the bootstrap (include/v2m_hip.h, "bootstrap"): numpy and Python integers only.

draws() makes a replicate's L draws with the 128-bit product taken by 32-bit halves (draw_int() is the same in Python integers);
weights() counts them per column; weighted_distances() is the brute force over ALL columns of the rows the oracle makes
(tests/column_counts_model.py: matrix()); splits() are a tree's n - 3 splits as frozensets normalised to the side without leaf 0, and
support() counts them.  For trees the yardsticks are the parent's: tests/nj_tree_model.py's nj() and host.nj_tree_cpu."""

import functools
import os
import re

import numpy as np

import column_counts_model as CM
import nj_tree_model as M
import pair_distances_model as PM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOOTSTRAP_KERNELS_HPP = os.path.join(ROOT, "vcf2multialign_amd", "csrc", "bootstrap_kernels.hpp")
PLOIDY_MAX = PM.PLOIDY_MAX
MASK = (1 << 64) - 1
G = 0x9E3779B97F4A7C15
SEEDS = (0, 1, MASK)
REPLICATES = (0, 1, (1 << 32) - 1)


@functools.lru_cache(maxsize=None)
def kernel_constants():
	"""(D, S): kBootDrawThreads, the draws per workgroup of bootstrap_weights_kernel, and kBootSlices, the bit slices kept per site word,
	read from csrc/bootstrap_kernels.hpp."""
	with open(BOOTSTRAP_KERNELS_HPP) as f:
		text = f.read()
	out = []
	for name in ("kBootDrawThreads", "kBootSlices"):
		found = re.findall(r"^constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text, re.M)
		assert len(found) == 1, "%s: %d definitions of the form `constexpr int %s = value;`" % (name, len(found), name)
		out.append(int(found[0]))
	return tuple(out)


# ---- the draws -----------------------------------------------------------------------------------------------------------------------------

def mix(z):
	"""splitmix64's finaliser, on a Python integer."""
	z &= MASK
	z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
	z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
	return z ^ (z >> 31)


def key_of(seed):
	return mix(seed + G)


def draw_int(seed, r, k, L):
	"""The column draw k of replicate r selects, in Python integers."""
	x = mix(key_of(seed) + (((r << 32) | k) + 1) * G)
	return (x * L) >> 64


def _mix_np(z):
	z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
	z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
	return z ^ (z >> np.uint64(31))


def draws(seed, r, L):
	"""u64[L]: the columns of the L draws of replicate r.  floor(x * L / 2^64) by 32-bit halves, L < 2^32:
	x = xh * 2^32 + xl gives x * L = xh * L * 2^32 + xl * L, so the high 64 bits are (xh * L + ((xl * L) >> 32)) >> 32 -- neither
	product nor the sum passes 2^64."""
	assert 0 <= L < 1 << 32 and 0 <= r < 1 << 32
	with np.errstate(over="ignore"):
		k = np.arange(L, dtype=np.uint64)
		x = _mix_np(np.uint64(key_of(seed)) + ((np.uint64(r << 32) | k) + np.uint64(1)) * np.uint64(G))
		xh, xl = x >> np.uint64(32), x & np.uint64(0xFFFFFFFF)
		return (xh * np.uint64(L) + ((xl * np.uint64(L)) >> np.uint64(32))) >> np.uint64(32)


def weights(seed, r, L):
	"""u32[L]: replicate r's weight of every column of a view of L columns."""
	return np.bincount(draws(seed, r, L).astype(np.int64), minlength=L).astype(np.uint32)[:L] if L else np.zeros(0, dtype=np.uint32)


# ---- the weighted matrix ---------------------------------------------------------------------------------------------------------------------

def weighted_distances(cls, w, acgt_only=False):
	"""u32[n, n]: the sum over every column c of cls[n, L] of w[c] * differ(i, j, c), in Python-sized integers, checked to fit a u32."""
	n = cls.shape[0]
	w = np.asarray(w, dtype=np.uint64)
	assert w.shape == (cls.shape[1],) and int(w.sum()) < 1 << 32
	d = np.zeros((n, n), dtype=np.uint64)
	base = cls < 4
	for i in range(n):
		diff = cls != cls[i]
		if acgt_only:
			diff &= base & base[i]
		d[i] = (diff * w).sum(axis=1, dtype=np.uint64)
	assert int(d.max(initial=0)) < 1 << 32
	return d.astype(np.uint32)


@functools.lru_cache(maxsize=None)
def _classes(item):
	cls = PM.classes(CM.matrix(item.g, item.rows, item.window))
	cls.setflags(write=False)
	return cls


def expected_weighted(item, w, acgt_only=False):
	return weighted_distances(_classes(item), w, acgt_only)


@functools.lru_cache(maxsize=None)
def expected_replicate(item, seed, r, acgt_only=False):
	"""Replicate r's matrix of a corpus item: computed once, shared, read-only."""
	cls = _classes(item)
	d = weighted_distances(cls, weights(seed, r, cls.shape[1]), acgt_only)
	d.setflags(write=False)
	return d


def site_mask(item):
	return PM.sites(CM.matrix(item.g, item.rows, item.window)) if len(item.rows) else np.zeros(0, dtype=bool)


def slices_of(item, w):
	"""K: the bit length of the largest weight on a site."""
	on_sites = np.asarray(w, dtype=np.uint64)[site_mask(item)]
	return int(on_sites.max(initial=0)).bit_length()


# ---- splits and support ----------------------------------------------------------------------------------------------------------------------

def splits(nodes, n):
	"""The n - 3 splits of the join records, in order: frozensets of leaves, the side without leaf 0."""
	assert len(nodes) == n - 2
	below = {k: frozenset([k]) for k in range(n)}
	everything = frozenset(range(n))
	out = []
	for t in range(n - 3):
		s = below[int(nodes[t]["a"])] | below[int(nodes[t]["b"])]
		below[n + t] = s
		out.append(everything - s if 0 in s else s)
	return out


def support(main_nodes, replicate_trees, n):
	"""u32[n - 3]: per join record of the main tree the replicate trees that hold its split."""
	mine = splits(main_nodes, n)
	assert len(set(mine)) == len(mine) and all(1 < len(s) < n - 1 for s in mine)
	counts = np.zeros(n - 3, dtype=np.uint32)
	for tree in replicate_trees:
		theirs = set(splits(tree, n))
		for t, s in enumerate(mine):
			counts[t] += s in theirs
	return counts


def newick_support(nodes, labels, counts):
	"""What --output-tree writes with --tree-bootstrap, as bytes: M.newick with the count behind every join node's bracket."""
	n = len(labels)
	assert len(nodes) == n - 2 and len(counts) == n - 3
	text = {k: M.label_text(labels[k]) for k in range(n)}
	for t, nd in enumerate(nodes):
		kids = [("a", "len_a"), ("b", "len_b")] + ([("c", "len_c")] if t == n - 3 else [])
		body = ",".join(text.pop(int(nd[key])) + ":%.10g" % float(nd[length]) for key, length in kids)
		text[n + t] = "(" + body + ")" + (str(int(counts[t])) if t < n - 3 else "")
	return (text[2 * n - 3] + ";\n").encode()


# ---- the corpus of the GPU tests -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def bootstrap(item, B, seed, acgt_only=False):
	"""(main nodes, replicate trees [B], support) of an item by the yardstick M.nj over the model's matrices."""
	n = len(item.rows)
	main = M.nj(PM.expected(item.g, item.rows, item.window, acgt_only)[0])
	trees = [M.nj(expected_replicate(item, seed, r, acgt_only)) for r in range(B)]
	return main, trees, support(main, trees, n)


def tree_row_counts():
	T, _ = PM.kernel_constants()
	return (3, 4, 5, T - 1, T, T + 1, 2 * T + 1)


@functools.lru_cache(maxsize=None)
def tree_graph():
	"""Enough sites that the replicates' trees differ from each other and yet share splits."""
	return PM.sites_graph(90, 140, 23)


def tree_item(n):
	g = tree_graph()
	return PM.Item("tree_%d" % n, g, [PLOIDY_MAX] + list(range(n - 1)))


def replicates_of(n):
	"""B per row count: 1 and a few dozen at the small sizes, a handful at the large ones."""
	return (1, 36) if n <= 5 else (5,)


def draw_lengths():
	"""L at the draw kernel's block seams +- 1."""
	D, _ = kernel_constants()
	return (D - 1, D, D + 1, 2 * D - 1, 2 * D, 2 * D + 1)


def explicit_patterns(item):
	"""(name, weights u32[L], K): the explicit-weight patterns of an item, K the bit length of the largest weight on a site."""
	L = _classes(item).shape[1]
	is_site = site_mask(item)
	site_columns = np.flatnonzero(is_site)
	other_columns = np.flatnonzero(~is_site)
	V = len(site_columns)
	out = []
	def add(name, w):
		w = np.asarray(w, dtype=np.uint32)
		assert w.shape == (L,) and int(w.astype(np.uint64).sum()) < 1 << 32
		out.append((name, w, slices_of(item, w)))
	add("ones", np.ones(L, dtype=np.uint32))
	add("zeros", np.zeros(L, dtype=np.uint32))
	w = np.zeros(L, dtype=np.uint64)
	w[site_columns[:32]] = [1 << b for b in range(min(32, V))]                   # 2^b on site b: the sum is 2^32 - 1 with 32 sites
	add("powers", w)
	for b in (1, 2, 5, 31):
		w = np.zeros(L, dtype=np.uint64)
		if V:
			w[site_columns[b % V]] = (1 << b) - 1                                    # 2^b - 1 on one site, 1 more on its neighbour
			w[site_columns[(b + 1) % V]] += 1 if V > 1 else 0
		add("below_2_%d" % b, w)
	w = np.zeros(L, dtype=np.uint64)
	w[site_columns[V // 2:][:1]] = (1 << 32) - 1                                   # one site carries everything
	add("one_site", w)
	w = np.zeros(L, dtype=np.uint64)
	w[other_columns] = 1 + (np.arange(len(other_columns)) % 5) * 1000              # non-site columns weigh, sites weigh 3
	w[site_columns] = 3
	add("non_sites", w)
	return out
