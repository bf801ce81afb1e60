"""The models of the neighbour-joining tree (include/v2m_hip.h, "neighbour joining") and the corpus its tests run.

nj() is the definition in numpy: IEEE binary64, every operation of the header a ufunc call or a scalar operation of its own, so that
nothing is contracted; the pair of a step is the first minimum of Q in row-major order over the live taxa in ascending order of id,
which is the header's three-key order.  Its keyword arguments swap single operations for the near misses a port is likely to make
(tests/test_nj_tree_host.py holds the corpus to telling every one of them from the definition).  nj_exact() is the same algorithm
in fractions.Fraction.  leaf_distances() adds up the branch lengths of a result between every two leaves, exactly: on an additive
matrix neighbour joining gives the matrix back, which checks the records without any model.  newick() is the text of --output-tree.

corpus() holds matrices given directly (tests/test_gpu_nj_tree.py uploads them); graph_items() are the items of
tests/pair_distances_model.py for the calls that start from rows."""

import functools
import itertools
import os
import re
from fractions import Fraction

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NJ_KERNELS_HPP = os.path.join(ROOT, "vcf2multialign_amd", "csrc", "nj_kernels.hpp")
NONE = 0xFFFFFFFF
# v2m_nj_node, field by field as the header declares it
NODE_DTYPE = np.dtype([("a", "<u4"), ("b", "<u4"), ("c", "<u4"), ("reserved", "<u4"), ("len_a", "<f8"), ("len_b", "<f8"), ("len_c", "<f8")])


@functools.lru_cache(maxsize=None)
def kernel_constants():
	"""(W, B, J): kNjRowsPerGroup, the rows a workgroup of nj_rowmin_kernel takes, kNjJoinThreads, the size of nj_join_kernel's one
	workgroup, and kNjJoinBatch, the live slots a lane of it has in flight (a trip of its loop takes J B slots), read from
	csrc/nj_kernels.hpp."""
	with open(NJ_KERNELS_HPP) as f:
		text = f.read()
	out = []
	for name in ("kNjRowsPerGroup", "kNjJoinThreads", "kNjJoinBatch"):
		found = re.findall(r"^constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text, re.M)
		assert len(found) == 1, "%s: %d definitions of the form `constexpr int %s = value;`" % (name, len(found), name)
		out.append(int(found[0]))
	return tuple(out)


# ---- the definition, in binary64 ------------------------------------------------------------------------------------------------------------

def _start(d):
	d = np.asarray(d)
	n = d.shape[0]
	assert d.shape == (n, n) and n >= 3
	upper = np.triu(d.astype(np.uint32), 1).astype(np.float64)          # only d[i][j], i < j, is read
	return n, upper + upper.T


def nj(d, tie="id", ru="plain", rk="plain", qsum="plain", trace=None):
	"""The n - 2 records (NODE_DTYPE) of the tree of d[n, n].  The live taxa lie in slots as the library keeps them (the new node in the
	lower of the two joined slots, the last live slot moved into the other); with tie="id" that plays no part.
	  tie="slot"   ties broken by slot instead of id
	  ru="fma"     R(u) with r * D(a, b) and the difference rounded once, as a fused multiply-subtract does
	  rk="alt"     R(k) updated as R(k) - (s - D(u, k))
	  qsum="alt"   Q's sum taken as (X - R(a)) - R(b)
	  qsum="fma"   Q with the product and the difference rounded once
	trace, a list, receives per join (ids of the pairs that hold the minimum of Q)."""
	n, D = _start(d)
	R = D.sum(axis=1)                                                       # exact integers below 2^53: any order
	ids = np.arange(n, dtype=np.int64)
	nodes = np.zeros(n - 2, dtype=NODE_DTYPE)
	r = n
	for t in range(n - 3):
		order = np.argsort(ids[:r]) if tie == "id" else np.arange(r)
		Dp, Rp = D[np.ix_(order, order)], R[order]
		factor = np.float64(r - 2)
		product = factor * Dp
		if qsum == "plain":
			Q = product - (Rp[:, None] + Rp[None, :])
		elif qsum == "alt":
			Q = (product - Rp[:, None]) - Rp[None, :]
		else:
			Q = np.array([[float((r - 2) * Fraction(x) - Fraction(s)) for x, s in zip(row, srow)] for row, srow in zip(Dp, Rp[:, None] + Rp[None, :])])
		Q[np.tril_indices(r)] = np.inf
		x, y = divmod(int(np.argmin(Q)), r)                               # the first minimum, row-major: smallest lower key, then smallest higher key
		if trace is not None:
			trace.append([(int(ids[order[i]]), int(ids[order[j]])) for i, j in zip(*np.nonzero(Q == Q[x, y]))])
		si, sj = int(order[x]), int(order[y])
		sa, sb = (si, sj) if ids[si] < ids[sj] else (sj, si)
		d_ab, r_a, r_b = D[sa, sb], R[sa], R[sb]
		delta = (r_a - r_b) / factor
		len_a = np.float64(0.5) * (d_ab + delta)
		len_b = d_ab - len_a
		nodes[t] = (ids[sa], ids[sb], NONE, 0, len_a, len_b, 0.0)
		others = np.ones(r, dtype=bool)
		others[[sa, sb]] = False
		s = D[sa, :r] + D[sb, :r]
		d_u = np.float64(0.5) * (s - d_ab)
		if rk == "plain":
			r_new = (R[:r] - s) + d_u
		else:
			r_new = R[:r] - (s - d_u)
		if ru == "plain":
			r_u = np.float64(0.5) * ((r_a + r_b) - np.float64(r) * d_ab)
		else:
			r_u = np.float64(0.5) * np.float64(float(Fraction(float(r_a + r_b)) - r * Fraction(float(d_ab))))
		p, q, last = min(sa, sb), max(sa, sb), r - 1
		R[:r][others] = r_new[others]
		D[p, :r][others] = d_u[others]
		D[:r, p][others] = d_u[others]
		D[p, p] = 0.0
		R[p] = r_u
		ids[p] = n + t
		if q != last:
			D[q, :r] = D[last, :r]
			D[:r, q] = D[:r, last]
			D[q, q] = 0.0
			R[q] = R[last]
			ids[q] = ids[last]
		r -= 1
	a, b, c = (int(s) for s in np.argsort(ids[:3]))
	half = np.float64(0.5)
	nodes[n - 3] = (ids[a], ids[b], ids[c], 0, half * ((D[a, b] + D[a, c]) - D[b, c]), half * ((D[a, b] + D[b, c]) - D[a, c]), half * ((D[a, c] + D[b, c]) - D[a, b]))
	return nodes


def nj_exact(d):
	"""The records of nj() as tuples (a, b, c, len_a, len_b, len_c) with the lengths as Fractions: the same algorithm without rounding."""
	n, D0 = _start(d)
	live = list(range(n))                                                   # ascending by id: a new node has the largest
	D = {(i, j): Fraction(int(D0[i, j])) for i in range(n) for j in range(n)}
	R = {i: sum(D[i, j] for j in range(n)) for i in range(n)}
	out = []
	for t in range(n - 3):
		r = len(live)
		best = None
		for x, y in itertools.combinations(range(r), 2):
			i, j = live[x], live[y]
			q = (r - 2) * D[i, j] - (R[i] + R[j])
			if best is None or q < best[0]:
				best = (q, i, j)
		_, a, b = best
		d_ab = D[a, b]
		len_a = (d_ab + (R[a] - R[b]) / (r - 2)) / 2
		out.append((a, b, NONE, len_a, d_ab - len_a, Fraction(0)))
		u = n + t
		R[u] = ((R[a] + R[b]) - r * d_ab) / 2
		for k in live:
			if k in (a, b):
				continue
			s = D[a, k] + D[b, k]
			D[u, k] = D[k, u] = (s - d_ab) / 2
			R[k] = (R[k] - s) + D[u, k]
		D[u, u] = Fraction(0)
		live = [k for k in live if k not in (a, b)] + [u]
	a, b, c = live
	out.append((a, b, c, ((D[a, b] + D[a, c]) - D[b, c]) / 2, ((D[a, b] + D[b, c]) - D[a, c]) / 2, ((D[a, c] + D[b, c]) - D[a, b]) / 2))
	return out


def records_of_exact(exact):
	nodes = np.zeros(len(exact), dtype=NODE_DTYPE)
	for t, (a, b, c, la, lb, lc) in enumerate(exact):
		nodes[t] = (a, b, c, 0, float(la), float(lb), float(lc))
	return nodes


def leaf_distances(nodes, n):
	"""Fraction[n][n]: the summed branch lengths between every two leaves of the tree the records describe, exactly."""
	assert len(nodes) == n - 2
	adjacent = {k: [] for k in range(2 * n - 2)}
	for t, nd in enumerate(nodes):
		kids = [("a", "len_a"), ("b", "len_b")] + ([("c", "len_c")] if t == n - 3 else [])
		for key, length in kids:
			adjacent[n + t].append((int(nd[key]), Fraction(float(nd[length]))))
			adjacent[int(nd[key])].append((n + t, Fraction(float(nd[length]))))
	out = [[None] * n for _ in range(n)]
	for leaf in range(n):
		seen, todo = {leaf: Fraction(0)}, [leaf]
		while todo:
			k = todo.pop()
			for other, length in adjacent[k]:
				if other not in seen:
					seen[other] = seen[k] + length
					todo.append(other)
		assert len(seen) == 2 * n - 2, "the records are no connected tree"
		out[leaf] = [seen[j] for j in range(n)]
	return out


# ---- the text -------------------------------------------------------------------------------------------------------------------------------

def label_text(label):
	if label and re.fullmatch(r"[A-Za-z0-9.\-]+", label):
		return label
	return "'" + label.replace("'", "''") + "'"


def newick(nodes, labels):
	"""What --output-tree writes, as bytes: built from the leaves up, node by node, without recursion."""
	n = len(labels)
	assert len(nodes) == n - 2
	text = {k: [label_text(labels[k])] for k in range(n)}                  # lists of pieces: joined once at the end
	for t, nd in enumerate(nodes):
		kids = [("a", "len_a"), ("b", "len_b")] + ([("c", "len_c")] if t == n - 3 else [])
		pieces = ["("]
		for k, (key, length) in enumerate(kids):
			if k:
				pieces.append(",")
			pieces.append(text.pop(int(nd[key])))
			pieces.append(":%.10g" % float(nd[length]))
		pieces.append(")")
		text[n + t] = pieces
	assert list(text) == [2 * n - 3]
	flat, todo = [], [text[2 * n - 3]]
	while todo:
		piece = todo.pop()
		if isinstance(piece, str):
			flat.append(piece)
		else:
			todo.extend(reversed(piece))
	return ("".join(flat) + ";\n").encode()


# ---- matrices -------------------------------------------------------------------------------------------------------------------------------

def tree_matrix(n, edges):
	"""u32[n, n]: the path lengths between leaves 0 ... n - 1 of the tree with the edges (node, node, integer length)."""
	size = 1 + max(max(a, b) for a, b, _ in edges)
	adjacent = [[] for _ in range(size)]
	for a, b, w in edges:
		adjacent[a].append((b, w))
		adjacent[b].append((a, w))
	d = np.zeros((n, n), dtype=np.uint32)
	for leaf in range(n):
		dist = [-1] * size
		dist[leaf] = 0
		todo = [leaf]
		while todo:
			k = todo.pop()
			for other, w in adjacent[k]:
				if dist[other] < 0:
					dist[other] = dist[k] + w
					todo.append(other)
		d[leaf] = dist[:n]
	return d


def _length(rng, top):
	return int(rng.integers(1, top)) if rng.random() > 0.2 else 0          # a fifth of the branches have length 0


def caterpillar(n, seed, top=50):
	"""Leaves in a random order along a spine."""
	rng = np.random.default_rng(seed)
	leaves = [int(x) for x in rng.permutation(n)]
	edges = [(leaves[0], n, _length(rng, top)), (leaves[-1], 2 * n - 3, _length(rng, top))]
	for k, leaf in enumerate(leaves[1:-1]):
		edges.append((leaf, n + k, _length(rng, top)))
		if k:
			edges.append((n + k - 1, n + k, _length(rng, top)))
	return tree_matrix(n, edges)


def balanced(levels, seed, top=50):
	"""A complete binary tree over 2^levels leaves, labelled at random."""
	rng = np.random.default_rng(seed)
	n = 1 << levels
	layer = [int(x) for x in rng.permutation(n)]
	edges, following = [], n
	while len(layer) > 3:
		above = []
		for k in range(0, len(layer) - 1, 2):
			edges += [(layer[k], following, _length(rng, top)), (layer[k + 1], following, _length(rng, top))]
			above.append(following)
			following += 1
		layer = above + layer[len(layer) // 2 * 2:]
	edges.append((layer[0], layer[1], _length(rng, top)))
	if len(layer) == 3:
		edges.append((layer[1], layer[2], _length(rng, top)))
	return tree_matrix(n, edges)


def random_insertion(n, seed, top=1000):
	"""Leaf k + 1 splits a random edge of the tree of leaves 0 ... k."""
	rng = np.random.default_rng(seed)
	edges = [[0, n, _length(rng, top)], [1, n, _length(rng, top)], [2, n, _length(rng, top)]]
	for leaf in range(3, n):
		a, b, w = edges[int(rng.integers(len(edges)))]
		inner = n + leaf - 2
		cut = int(rng.integers(0, w + 1))
		edges.remove([a, b, w])
		edges += [[a, inner, cut], [inner, b, w - cut], [leaf, inner, _length(rng, top)]]
	return tree_matrix(n, [tuple(e) for e in edges])


# The six-leaf tree of the relabelings: ((0:3,1:5):2,(2:0,3:7):4,(4:1,5:6):0) -- a branch of length 0 at a leaf and one inside
SIX_LEAF_EDGES = ((0, 6, 3), (1, 6, 5), (2, 7, 0), (3, 7, 7), (4, 8, 1), (5, 8, 6), (6, 9, 2), (7, 9, 4), (8, 9, 0))


def relabelled(d, perm):
	d = np.asarray(d)
	return np.ascontiguousarray(d[np.ix_(perm, perm)])


def path_noise(n, seed):
	"""d = |p_i - p_j| + symmetric noise: p below 2^31, the noise below 2^12.  Far from additive: the halves of the updates pile up
	fraction bits until the sums round."""
	rng = np.random.default_rng(seed)
	p = rng.integers(0, 1 << 31, size=n, dtype=np.int64)
	noise = np.triu(rng.integers(0, 1 << 12, size=(n, n), dtype=np.int64), 1)
	d = np.abs(p[:, None] - p[None, :]) + noise + noise.T
	np.fill_diagonal(d, 0)
	return d.astype(np.uint32)


def groups_of_identical(sizes, seed):
	"""Groups of identical taxa: distance 0 inside a group, one distance for every two groups; the taxa shuffled."""
	rng = np.random.default_rng(seed)
	g = len(sizes)
	between = np.triu(rng.integers(1, 40, size=(g, g)), 1)
	between = between + between.T
	member = np.repeat(np.arange(g), sizes)
	rng.shuffle(member)
	return between[np.ix_(member, member)].astype(np.uint32)


# a leaf pair ties with a pair that holds an internal node: with r = 4 the two pairs of a split have the same Q, always; here join 0
# takes leaves 2 and 3 (node 5), and then (0, 1) ties with (4, 5): (0, 1) has the smaller lower id
TIE_LEAF_INTERNAL = np.array([[0, 4, 9, 11, 12], [4, 0, 9, 11, 12], [9, 9, 0, 6, 13], [11, 11, 6, 0, 15], [12, 12, 13, 15, 0]], dtype=np.uint32)

PATH_NOISE_SEEDS = ((101, 1), (127, 2), (150, 3), (163, 4), (180, 5))     # (n, seed)
# Small ones of the same family, for Q's sum.  With four taxa left the two pairs of a split have the same Q by value.  With about 30
# taxa the D and R have by then gathered some 20 fraction bits under 2^32 and have hardly been rounded, so the two Q still lie within a
# unit of each other, R(a) + R(b) no longer fits 53 bits, and which of the two pairs is joined hangs on how Q's sum is rounded.  (With
# 100 taxa and more the R have long been rounded by then, the two Q lie many units apart, and the order of Q's sum changed no record
# under any of 400 seeds; below 28 taxa it changed none of 150 either.)  These seeds are ones whose records (X - R(a)) - R(b) changes.
Q_SUM_SEEDS = ((28, 2), (30, 8), (32, 6))


class Item:
	def __init__(self, name, d, additive=False):
		self.name, self.d, self.additive = name, np.ascontiguousarray(d, dtype=np.uint32), additive
		self.n = self.d.shape[0]

	def __repr__(self):
		return self.name


def seam_counts():
	W, B, _ = kernel_constants()
	return sorted({3, 4, 5, W - 1, W, W + 1, B - 1, B, B + 1, 2 * B + 1})


@functools.lru_cache(maxsize=None)
def corpus():
	"""The matrices every test of the tree runs."""
	W, B, _ = kernel_constants()
	items = []
	for n in seam_counts():
		items.append(Item("noise_%d" % n, path_noise(n, 1000 + n)))
		if n <= B + 1:
			items.append(Item("inserted_%d" % n, random_insertion(n, 2000 + n), additive=True))
	for n in sorted({3, 4, 9, W + 1, 40}):
		items.append(Item("all_equal_%d" % n, 7 * (1 - np.eye(n, dtype=np.int64))))
	items.append(Item("all_equal_large_40", 0xFFFFFFFF * (1 - np.eye(40, dtype=np.int64))))
	items.append(Item("all_zero_10", np.zeros((10, 10))))
	items.append(Item("all_zero_3", np.zeros((3, 3))))
	items.append(Item("groups_4_4_4", groups_of_identical((4, 4, 4), 5)))
	items.append(Item("groups_1_2_3_5_8", groups_of_identical((1, 2, 3, 5, 8), 6)))
	items.append(Item("tie_leaf_internal", TIE_LEAF_INTERNAL))
	items.append(Item("caterpillar_12", caterpillar(12, 7), additive=True))
	items.append(Item("caterpillar_31", caterpillar(31, 8), additive=True))
	items.append(Item("balanced_16", balanced(4, 9), additive=True))
	items.append(Item("balanced_32", balanced(5, 10), additive=True))
	items.append(Item("inserted_20", random_insertion(20, 11), additive=True))
	items.append(Item("inserted_33", random_insertion(33, 12, top=1 << 24), additive=True))
	six = tree_matrix(6, SIX_LEAF_EDGES)
	for k, perm in enumerate(itertools.permutations(range(6))):
		items.append(Item("six_%03d" % k, relabelled(six, list(perm)), additive=True))
	for n, seed in PATH_NOISE_SEEDS + Q_SUM_SEEDS:
		items.append(Item("path_noise_%d_%d" % (n, seed), path_noise(n, seed)))
	return items


def join_batch_counts():
	"""Taxa around a full trip of nj_join_kernel's loop over the live slots, J B at a time, element e of a lane's batch the slot e B + lane:
	(J - 1) B + 1 -- element J - 1 runs, in lane 0 only; J B -- the batch exactly full, no second trip; J B + 64 -- 64 joins with
	r > J B, a wave of lanes in the second trip."""
	_, B, J = kernel_constants()
	return ((J - 1) * B + 1, J * B, J * B + 64)


@functools.lru_cache(maxsize=None)
def join_batch_items():
	"""A list of its own: corpus() ends at 2 B + 1 taxa, which its tests assert, and nj_exact() must not run at these sizes."""
	return [Item("path_noise_%d_1" % n, path_noise(n, 1)) for n in join_batch_counts()]


@functools.lru_cache(maxsize=None)
def expected(name):
	"""The model's records of an item of corpus() or join_batch_items(): computed once, shared, read-only."""
	item = next(i for i in corpus() + join_batch_items() if i.name == name)
	nodes = nj(item.d)
	nodes.setflags(write=False)
	return nodes


def graph_items():
	"""The items of tests/pair_distances_model.py (sites_graph() graphs: whole rows and windows, the REF row and repeated rows among
	the rows) that have at least three rows."""
	import pair_distances_model as PM
	return [item for item in PM.corpus() if len(item.rows) >= 3]
