"""The models of parsimony on a tree (include/v2m_hip.h, "parsimony") and the corpus its tests run.

fitch() is the definition in numpy, vectorised over the sites: the up pass in the order of the records, the down pass from the last
record to the first with the children in the order a, b, c, the mutations ascending by site and within a site in that order.  sankoff()
is an independent dynamic programme over the four states (a missing leaf costs nothing in any state) that gives the least number of
changes per site: what the steps of fitch() must equal, whatever the tree.  newick(), mutations_text() and sites_text() are the three
files of the driver.

Trees: the records tests/nj_tree_model.py's nj() builds from its caterpillar, balanced and random-insertion matrices; spine(), the
caterpillar written down directly, in which every record but the first reads the set the record before it stored; and random_joins(),
join orders that no neighbour joining gives.  corpus() holds (tree, bytes) items for the device form; graph_items() are the items of
tests/variable_sites_model.py with at least three rows, for the calls that start from rows."""

import functools
import os
import re

import numpy as np

import nj_tree_model as NJ

ROOT = NJ.ROOT
PARSIMONY_KERNELS_HPP = os.path.join(ROOT, "vcf2multialign_amd", "csrc", "parsimony_kernels.hpp")
NONE = NJ.NONE
NODE_DTYPE = NJ.NODE_DTYPE
# v2m_parsimony_site, v2m_tree_site and v2m_tree_mutation, field by field as the header declares them
SITE_DTYPE = np.dtype([("steps", "<u4"), ("present", "<u4")])
TREE_SITE_DTYPE = np.dtype([("column", "<u8"), ("steps", "<u4"), ("present", "<u4")])
MUTATION_DTYPE = np.dtype([("site", "<u4"), ("node", "<u4"), ("from", "<u4"), ("to", "<u4")])
LETTERS = "ACGT"


@functools.lru_cache(maxsize=None)
def kernel_constants():
	"""(S, T, J): kFitchSites, the sites a lane owns, kFitchThreads, the lanes of a workgroup, and kFitchBatch, the records whose leaf
	rows a lane of fitch_up_kernel reads ahead, read from csrc/parsimony_kernels.hpp."""
	with open(PARSIMONY_KERNELS_HPP) as f:
		text = f.read()
	out = []
	for name in ("kFitchSites", "kFitchThreads", "kFitchBatch"):
		found = re.findall(r"^constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text, re.M)
		assert len(found) == 1, "%s: %d definitions of the form `constexpr int %s = value;`" % (name, len(found), name)
		out.append(int(found[0]))
	return tuple(out)


# ---- the definition ---------------------------------------------------------------------------------------------------------------------

def leaf_sets(m):
	"""u8 masks of the bytes m: 1 << class for A, C, G, T (either case), 0xF for anything else."""
	m = np.asarray(m, dtype=np.uint8)
	out = np.full(m.shape, 0xF, dtype=np.uint8)
	for k, letter in enumerate(LETTERS):
		out[(m == ord(letter)) | (m == ord(letter.lower()))] = 1 << k
	return out


def children(nodes, t):
	nd = nodes[t]
	return [int(nd["a"]), int(nd["b"])] + ([int(nd["c"])] if t == len(nodes) - 1 else [])


def _lowest(s):
	return s & (~s + np.uint8(1))


def _class_of(one_hot):
	return np.log2(one_hot.astype(np.float64)).astype(np.uint32)


def fitch(m, nodes):
	"""(sites SITE_DTYPE[V], branch_changes u32[2 n - 3], mutations MUTATION_DTYPE[...]) of the bytes m[n, V] on the n - 2 records."""
	m = np.asarray(m, dtype=np.uint8)
	n, V = m.shape
	assert len(nodes) == n - 2 and n >= 3
	S = np.zeros((2 * n - 2, V), dtype=np.uint8)
	S[:n] = leaf_sets(m)
	steps = np.zeros(V, dtype=np.uint32)
	for t in range(n - 2):
		kids = children(nodes, t)
		a, b = S[kids[0]], S[kids[1]]
		x = a & b
		empty = x == 0
		x = np.where(empty, a | b, x)
		steps += empty
		if t == n - 3:
			y = x & S[kids[2]]
			empty = y == 0
			steps += empty
			x = np.where(empty, x, y)
		S[n + t] = x
	called = S[:n] != 0xF
	present = np.bitwise_or.reduce(np.where(called, S[:n], 0), axis=0).astype(np.uint32) if V else np.zeros(0, dtype=np.uint32)
	sites = np.zeros(V, dtype=SITE_DTYPE)
	sites["steps"], sites["present"] = steps, present
	state = np.zeros((2 * n - 2, V), dtype=np.uint8)
	state[2 * n - 3] = _lowest(S[2 * n - 3])
	branch_changes = np.zeros(2 * n - 3, dtype=np.uint32)
	found = []                                                              # per branch in the down pass's order: (sites, node, from, to)
	for t in range(n - 3, -1, -1):
		parent = state[n + t]
		for x in children(nodes, t):
			state[x] = np.where(S[x] & parent, parent, _lowest(S[x]))
			where = np.flatnonzero(state[x] != parent)
			branch_changes[x] = len(where)
			if len(where):
				found.append((where, x, _class_of(parent[where]), _class_of(state[x][where])))
	total = sum(len(f[0]) for f in found)
	mutations = np.zeros(total, dtype=MUTATION_DTYPE)
	at = 0
	for where, x, src, dst in found:
		block = mutations[at:at + len(where)]
		block["site"], block["node"], block["from"], block["to"] = where, x, src, dst
		at += len(where)
	mutations = mutations[np.argsort(mutations["site"], kind="stable")]         # by site; within a site the down pass's order stays
	return sites, branch_changes, mutations


def sankoff(m, nodes):
	"""u32[V]: the least number of changes of every site on the tree, by dynamic programming over the four states."""
	m = np.asarray(m, dtype=np.uint8)
	n, V = m.shape
	big = 1 << 20
	sets = leaf_sets(m)
	cost = [None] * (2 * n - 2)
	for leaf in range(n):
		cost[leaf] = np.stack([np.where(sets[leaf] >> k & 1, 0, big) for k in range(4)]).astype(np.int64)
	for t in range(n - 2):
		total = np.zeros((4, V), dtype=np.int64)
		for x in children(nodes, t):
			least = cost[x].min(axis=0)
			total += np.minimum(cost[x], least + 1)                          # stay in the state, or change from the child's cheapest
		cost[n + t] = total
	return cost[2 * n - 3].min(axis=0).astype(np.uint32)


def tree_sites(sites, columns):
	out = np.zeros(len(sites), dtype=TREE_SITE_DTYPE)
	out["column"], out["steps"], out["present"] = columns, sites["steps"], sites["present"]
	return out


def expected_of_rows(g, rows, nodes, window=None):
	"""(sites TREE_SITE_DTYPE[V], branch_changes, mutations, L) as Context.tree_parsimony reports them for the rows of a graph."""
	import variable_sites_model as VM
	columns, data, L = VM.expected(g, rows, window, snp_only=True)
	sites, branch_changes, mutations = fitch(data, nodes)
	return tree_sites(sites, columns), branch_changes, mutations, L


# ---- the texts --------------------------------------------------------------------------------------------------------------------------

def newick(nodes, labels, branch_changes):
	"""What --output-tree-parsimony writes, as bytes: built from the leaves up, node by node, without recursion."""
	n = len(labels)
	assert len(nodes) == n - 2 and len(branch_changes) == 2 * n - 3
	text = {k: [NJ.label_text(labels[k])] for k in range(n)}
	for t in range(n - 2):
		pieces = ["("]
		for k, x in enumerate(children(nodes, t)):
			if k:
				pieces.append(",")
			pieces.append(text.pop(x))
			pieces.append(":%d" % int(branch_changes[x]))
		pieces.append(")node%d" % t)
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


def _position(g, column):
	import column_counts_model as CM
	p = CM.reference_position(g, int(column))
	return "." if p is None else str(p)


def mutations_text(g, mutations, sites, labels):
	"""What --output-tree-mutations writes."""
	n = len(labels)
	lines = []
	for mu in mutations:
		x, column = int(mu["node"]), int(sites["column"][int(mu["site"])])
		lines.append("%s\t%d\t%s\t%s\t%s\n" % (labels[x] if x < n else "node%d" % (x - n), column, _position(g, column), LETTERS[int(mu["from"])], LETTERS[int(mu["to"])]))
	return "".join(lines).encode()


def sites_text(g, sites):
	"""What --output-tree-sites writes."""
	lines = []
	for s in sites:
		present = [LETTERS[k] for k in range(4) if int(s["present"]) >> k & 1]
		lines.append("%d\t%s\t%s\t%d\t%d\n" % (int(s["column"]), _position(g, s["column"]), "".join(present), int(s["steps"]), int(s["steps"]) - (len(present) - 1)))
	return "".join(lines).encode()


# ---- trees ------------------------------------------------------------------------------------------------------------------------------

def spine(n):
	"""The caterpillar joined from one end: record t > 0 joins leaf t + 1 and the node record t - 1 made."""
	nodes = np.zeros(n - 2, dtype=NODE_DTYPE)
	if n == 3:
		nodes[0] = (0, 1, 2, 0, 0.0, 0.0, 0.0)
		return nodes
	nodes[0] = (0, 1, NONE, 0, 0.0, 0.0, 0.0)
	for t in range(1, n - 3):
		nodes[t] = (t + 1, n + t - 1, NONE, 0, 0.0, 0.0, 0.0)
	nodes[n - 3] = (n - 2, n - 1, 2 * n - 4, 0, 0.0, 0.0, 0.0)
	return nodes


def random_joins(n, seed):
	"""Records of a random order of joins: any two live nodes, whatever their distance; the lengths are noise."""
	rng = np.random.default_rng(seed)
	live = list(range(n))
	nodes = np.zeros(n - 2, dtype=NODE_DTYPE)
	for t in range(n - 3):
		i, j = sorted(int(x) for x in rng.choice(len(live), size=2, replace=False))
		a, b = sorted((live[i], live[j]))
		nodes[t] = (a, b, NONE, 0, rng.normal(), rng.normal(), 0.0)
		live = [x for k, x in enumerate(live) if k not in (i, j)] + [n + t]
	a, b, c = sorted(live)
	nodes[n - 3] = (a, b, c, 0, rng.normal(), rng.normal(), rng.normal())
	return nodes


@functools.lru_cache(maxsize=None)
def _nj_of(kind, n, seed):
	if kind == "caterpillar":
		d = NJ.caterpillar(n, seed)
	elif kind == "balanced":
		d = NJ.balanced(n.bit_length() - 1, seed)
	else:
		d = NJ.random_insertion(n, seed)
	nodes = NJ.nj(d)
	nodes.setflags(write=False)
	return nodes


def tree(kind, n, seed=1):
	if kind == "spine":
		return spine(n)
	if kind == "joins":
		return random_joins(n, seed)
	return _nj_of(kind, n, seed)


def is_tree(nodes, n):
	"""The header's conditions."""
	if len(nodes) != n - 2 or n < 3:
		return False
	seen = []
	for t in range(n - 2):
		kids = children(nodes, t)
		if (int(nodes[t]["c"]) == NONE) != (t < n - 3) or kids != sorted(set(kids)) or kids[-1] >= n + t:
			return False
		seen += kids
	return sorted(seen) == list(range(2 * n - 3))


# ---- bytes ------------------------------------------------------------------------------------------------------------------------------

ALPHABET = np.frombuffer(b"ACGTacgtN-nR" + bytes([0, 0xC1]), dtype=np.uint8)


def evolved(nodes, n, V, seed, change=0.08, missing=0.1, noise=0.15):
	"""u8[n, V]: most sites evolved down the tree with a change on a branch now and then (few steps, some of them homoplasies), a share of
	sites drawn byte by byte from ALPHABET (many steps), a share of the bytes made missing in one spelling or another, case at random."""
	rng = np.random.default_rng(seed)
	state = np.zeros((2 * n - 2, V), dtype=np.int64)
	state[2 * n - 3] = rng.integers(0, 4, size=V)
	for t in range(n - 3, -1, -1):
		for x in children(nodes, t):
			flip = rng.random(V) < change
			state[x] = np.where(flip, rng.integers(0, 4, size=V), state[n + t])
	letters = np.frombuffer(b"ACGT", dtype=np.uint8)[state[:n]]
	letters = np.where(rng.random((n, V)) < 0.3, letters | 0x20, letters)       # lower case
	holes = np.frombuffer(b"N-nR" + bytes([0, 0xC1]), dtype=np.uint8)
	letters = np.where(rng.random((n, V)) < missing, holes[rng.integers(0, len(holes), size=(n, V))], letters)
	noisy = rng.random(V) < noise
	letters[:, noisy] = ALPHABET[rng.integers(0, len(ALPHABET), size=(n, int(noisy.sum())))]
	return np.ascontiguousarray(letters, dtype=np.uint8)


class Item:
	def __init__(self, name, nodes, m):
		self.name, self.nodes, self.m = name, nodes, m
		self.n, self.V = m.shape
		for a in (self.nodes, self.m):
			a.setflags(write=False)

	def __repr__(self):
		return self.name


def seam_site_counts():
	"""With S sites a lane, W = 64 S a wave and B a workgroup: 1 ... S + 1, W - 1, W, W + 1, B - 1, B, B + 1, 2 B + 1."""
	S, T, _ = kernel_constants()
	W, B = 64 * S, T * S
	return tuple(sorted(set(list(range(1, S + 2)) + [W - 1, W, W + 1, B - 1, B, B + 1, 2 * B + 1])))


def seam_taxa_counts():
	"""3 (the trifurcation alone), 4 ... 11 (every remainder of the join loop's batches, twice), 65 and 257."""
	_, _, J = kernel_constants()
	return tuple(sorted(set([3] + list(range(4, 4 + 2 * J)) + [65, 257])))


@functools.lru_cache(maxsize=None)
def corpus():
	"""The (tree, bytes) items every test of the device form and of the restatement runs."""
	S, T, _ = kernel_constants()
	W, B = 64 * S, T * S
	items = []
	for V in seam_site_counts():
		nodes = tree("inserted", 9, 3)
		items.append(Item("sites_%d" % V, nodes, evolved(nodes, 9, V, 100 + V)))
	for n in seam_taxa_counts():
		nodes = tree("inserted", n, 5) if n % 2 else tree("joins", n, 5)
		items.append(Item("taxa_%d" % n, nodes, evolved(nodes, n, W + 1, 200 + n)))
	for kind, n in (("spine", 34), ("caterpillar", 31), ("balanced", 32), ("inserted", 33), ("joins", 35)):
		nodes = tree(kind, n, 7)
		items.append(Item("%s_%d" % (kind, n), nodes, evolved(nodes, n, B + 1, 300 + n)))
	# a long spine over a few sites: every record reads what the record before it stored, 255 times over
	nodes = spine(257)
	items.append(Item("spine_257", nodes, evolved(nodes, 257, S + 1, 9, change=0.02)))
	# nothing but noise, and nothing but one letter
	nodes = tree("joins", 12, 2)
	rng = np.random.default_rng(5)
	items.append(Item("noise_12", nodes, np.ascontiguousarray(ALPHABET[rng.integers(0, len(ALPHABET), size=(12, W + 3))])))
	items.append(Item("constant_12", nodes, np.full((12, W + 3), ord("g"), dtype=np.uint8)))
	names = [i.name for i in items]
	assert len(set(names)) == len(names) and all(is_tree(i.nodes, i.n) for i in items)
	return items


@functools.lru_cache(maxsize=None)
def expected(name):
	"""The model's results of an item of corpus(): computed once, shared, read-only."""
	item = next(i for i in corpus() if i.name == name)
	out = fitch(item.m, item.nodes)
	for a in out:
		a.setflags(write=False)
	return out


def graph_items():
	"""The items of tests/variable_sites_model.py (whole rows and windows, rows with cuts and repeated rows among them) with at least
	three rows."""
	import variable_sites_model as VM
	return [item for item in VM.corpus() if len(item.rows) >= 3]
