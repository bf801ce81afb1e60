"""A plain positional BWT and the two walks the founder kernels do over it.  TEST INFRASTRUCTURE ONLY (numpy, no product code).

Written from the reference project's definitions -- pbwt_context::update_divergence (include/vcf2multialign/pbwt.hh:77-134), the
value walk of find_initial_cut_positions_lambda_min (libvcf2multialign/find_cut_positions.cc:134-165) and the class collection of
find_matchings (libvcf2multialign/founder_sequence_greedy_output.cc:215-251) -- and from nothing in csrc/.

Path bits are a bool array bits[copy, edge].  Divergence values are BIASED by one as in include/v2m_hip.h: 0 is the reference's
DIVERGENCE_MAX ("no match yet"), b = d + 1 otherwise, so that pbwt.hh's order (DIVERGENCE_MAX first, :36) is plain integer order.
Two copies that agree on every edge so far have biased 1; biased 0 exists only in the state before the first edge.
"""

import bisect

import numpy as np

PLOIDY_MAX = 0xFFFFFFFF


# ---- the state ----------------------------------------------------------------------------------------------------------------

def initial_state(n_copies):
	"""pbwt_context's constructor (pbwt.hh:62-75): the identity order, divergence 0 for the first copy and DIVERGENCE_MAX for the rest."""
	return list(range(n_copies)), [1] + [0] * (n_copies - 1) if n_copies else []


def step(order, div, column_bits, edge):
	"""update_divergence (pbwt.hh:77-134, Durbin's algorithm 2) for edge `edge` as a literal loop; column_bits[copy] is the edge's bit."""
	p = q = edge + 2                                                            # divergence_value pp{kk + 1}, biased
	zeros_o, zeros_d, ones_o, ones_d = [], [], [], []
	for c, d in zip(order, div):
		c, d = int(c), int(d)
		if p < d:
			p = d
		if q < d:
			q = d
		if not column_bits[c]:
			zeros_o.append(c)
			zeros_d.append(p)
			p = 1                                                               # pp = 0
		else:
			ones_o.append(c)
			ones_d.append(q)
			q = 1
	return zeros_o + ones_o, zeros_d + ones_d


def step_np(order, div, column_bits, edge):
	"""step() vectorised for thousands of copies (tests/test_pbwt_ref.py holds the two against each other): a copy of class 0 gets the
	largest value since the previous copy of class 0, itself included, and at least edge + 2 (the first one) or 1 (the others)."""
	order = np.asarray(order, dtype=np.int64)
	div = np.asarray(div, dtype=np.int64)
	ones = np.asarray(column_bits, dtype=bool)[order]
	out_o, out_d = [], []
	for mask in (~ones, ones):
		at = np.flatnonzero(mask)
		if at.size:
			starts = np.concatenate([[0], at[:-1] + 1])
			floor = np.ones(at.size, dtype=np.int64)
			floor[0] = edge + 2
			out_d.append(np.maximum(np.maximum.reduceat(div[:at[-1] + 1], starts), floor))
			out_o.append(order[at])
	return np.concatenate(out_o), np.concatenate(out_d)


def state_at_literal(bits, k):
	"""The state after k edges BY DEFINITION: the copies stably sorted by their reversed k-edge prefixes; div[0] = k + 1; for every other
	copy 2 + the highest edge (< k) where it differs from its predecessor in the order, 1 if there is none."""
	n = bits.shape[0]
	if 0 == k:
		return initial_state(n)
	order = sorted(range(n), key=lambda c: tuple(bool(b) for b in bits[c, :k][::-1]))   # (sorted() is stable)
	div = [k + 1]
	for a, b in zip(order, order[1:]):
		d = 1
		for e in range(k - 1, -1, -1):
			if bits[a, e] != bits[b, e]:
				d = e + 2
				break
		div.append(d)
	return order, div


def state_at(bits, k):
	"""state_at_literal() vectorised (np.lexsort, xor and highest set bit), for thousands of copies.  Returns u32 arrays."""
	n = bits.shape[0]
	if 0 == k or 0 == n:
		o, d = initial_state(n)
		return np.array(o, dtype=np.uint32), np.array(d, dtype=np.uint32)
	prefix = np.ascontiguousarray(bits[:, :k])
	order = np.lexsort(prefix.T)                                                # last key = edge k - 1 = the primary one; stable
	div = np.empty(n, dtype=np.uint32)
	div[0] = k + 1
	if n > 1:
		differ = prefix[order[1:]] != prefix[order[:-1]]
		highest = k - 1 - np.argmax(differ[:, ::-1], axis=1)
		div[1:] = np.where(differ.any(axis=1), highest + 2, 1)
	return order.astype(np.uint32), div


# ---- the cut search's walk at a candidate --------------------------------------------------------------------------------------

def trials_at(div, cand_edge, cand_aligned, next, min_distance, n_edges):
	"""find_cut_positions.cc:134-165 at candidate `next` (an index into cand_edge / cand_aligned; the list holds the sentinel and the
	current candidate, :112,131) with the divergence values `div` of the state after cand_edge[next] edges.
	Returns ([(pred, class_count), ...] in the order the loop calls update_if_needed -- the final "reaches further left" call
	(:162-165) included, calls with the candidate itself left out (they cannot lower its score: it starts at the copy count) --, the
	number of distinct bins).  A bin is what a value other than the largest and other than "no match yet" points to: the first
	candidate OF THE WHOLE LIST whose edge is not less than the value, or "none up to `next`" (one clipped bin)."""
	distinct, how_many = np.unique(np.asarray(div, dtype=np.int64), return_counts=True)
	counts = {int(d): int(n) for d, n in zip(distinct, how_many)}
	values = sorted(counts)                                                     # DIVERGENCE_MAX (biased 0) first, pbwt.hh:36
	edges = [int(e) for e in cand_edge]
	pairs = []
	rb = next + 1                                                               # cut_positions.end(): the current candidate is in the list
	eq_class_count = counts[values[-1]]
	bins = set()
	for b in reversed(values[:-1]):                                             # divergence_value_counts_reversed(): without the largest
		if 0 != b:
			it = bisect.bisect_left(edges, b - 1, 0, rb)                        # std::lower_bound(begin, cut_pos_rb, div_edge_idx)
			whole = bisect.bisect_left(edges, b - 1) if b - 1 <= n_edges else len(edges)
			bins.add(min(whole, next + 1))
		else:
			it = rb                                                             # DIVERGENCE_MAX: no candidate's edge reaches it
		if it != rb:
			rb = it
			if min_distance <= int(cand_aligned[next]) - int(cand_aligned[it]) and it != next:
				pairs.append((it, eq_class_count))
		eq_class_count += counts[b]
	if 0 != rb:
		rb -= 1
		if rb != next:
			pairs.append((rb, eq_class_count))
	return pairs, len(bins)


def bin_keys_at(div, cand_edge, next, n_edges):
	"""The distinct bins trials_at() counts, as keys: candidate indices, next + 1 for the clipped bin."""
	edges = [int(e) for e in cand_edge]
	largest = max(int(d) for d in div)
	return sorted({min(bisect.bisect_left(edges, int(d) - 1) if int(d) - 1 <= n_edges else len(edges), next + 1) for d in div if 0 != int(d) and largest != int(d)})


def walk_trials(bits, n_copies, cand_edge, cand_aligned, first, end, min_distance, n_edges, state=None, literal=False):
	"""The candidates [first, end) of one chunk from the state after cand_edge[first] edges (`state`, or built by definition), stepping
	edge by edge between them.  Returns ([pairs of candidate first, ...], [bins of candidate first, ...])."""
	if first >= end:
		return [], []
	b = bits[:n_copies]
	edge = int(cand_edge[first])
	order, div = state if state is not None else state_at(b, edge)
	one_step = step if literal else step_np
	all_pairs, all_bins = [], []
	for c in range(first, end):
		for edge in range(edge, int(cand_edge[c])):
			order, div = one_step(order, div, b[:, edge], edge)
		edge = int(cand_edge[c])
		pairs, n_bins = trials_at(div, cand_edge, cand_aligned, c, min_distance, n_edges)
		all_pairs.append(pairs)
		all_bins.append(n_bins)
	return all_pairs, all_bins


# ---- the score recurrence and the back-walk ------------------------------------------------------------------------------------

def cut_positions_from_trials(pairs_per_candidate, cand_edge, cand_node, n_copies, node_count):
	"""find_cut_positions.cc:55-63 over the pairs of candidates 1 .. (candidate 0 is the sentinel, :112) and the back-walk :182-209.
	Returns (cut positions, score) or None."""
	EDGE_MAX = None
	n = len(cand_edge)
	if n <= 1:
		return None
	score = [0] + [n_copies] * (n - 1)
	prev_edge = [EDGE_MAX] * n
	edges = [int(e) for e in cand_edge]
	for c in range(1, n):
		for pred, class_count in pairs_per_candidate[c - 1]:
			candidate_score = max(class_count, score[pred])
			if candidate_score < score[c]:
				score[c] = candidate_score
				prev_edge[c] = edges[pred]
	out = []
	it = n - 1
	while True:
		out.append(int(cand_node[it]))
		if prev_edge[it] is EDGE_MAX:
			break
		it = bisect.bisect_left(edges, prev_edge[it], 0, it)
	if 0 != out[-1]:
		out.append(0)
	out.reverse()
	if out[-1] != node_count - 1:
		out[-1] = node_count - 1
	return out, score[n - 1]


def candidates_of_graph(alt_edge_targets, alt_edge_count_csum, aligned_positions):
	"""The candidate list of find_cut_positions.cc:112,126-131: the sentinel, then every node no earlier ALT edge jumps over, one per
	distinct edge index.  Returns (cand_edge, cand_node, cand_aligned)."""
	cand_edge, cand_node = [0], [0]
	rightmost = 0
	prev_id = None
	csum = [int(x) for x in alt_edge_count_csum]
	for node in range(len(csum) - 1):
		edge_idx = csum[node]
		if rightmost <= node and prev_id != edge_idx:
			cand_edge.append(edge_idx)
			cand_node.append(node)
			prev_id = edge_idx
		for e in range(csum[node], csum[node + 1]):
			rightmost = max(rightmost, int(alt_edge_targets[e]))
	return cand_edge, cand_node, [int(aligned_positions[n]) for n in cand_node]


# ---- the matching's walk at a cut ------------------------------------------------------------------------------------------------

def records_at(order, div, prev_cut_edge, cut_pair_edge, lhs_classes, with_joined):
	"""founder_sequence_greedy_output.cc:215-251 at a cut: `prev_cut_edge` / `cut_pair_edge` are the edges before the previous cut and the
	one before that, lhs_classes[copy] the representatives the previous cut left (PLOIDY_MAX = none), with_joined = "0 < cut_pos_idx".
	Returns (distinct, first_class, [(lhs, rhs, size), ...] in pBWT order and UNSORTED, rhs_classes)."""
	rhs_classes = [PLOIDY_MAX] * len(lhs_classes)
	rep = PLOIDY_MAX
	distinct = 0
	joined = []
	for aa, b in zip(order, div):
		aa, b = int(aa), int(b)
		if 0 == b or prev_cut_edge < b - 1:                                     # prev_cut_edge_idx < dd, DIVERGENCE_MAX the largest edge_type
			rep = aa
			distinct += 1
		rhs_classes[aa] = rep
		if with_joined:
			if 0 == b or cut_pair_edge < b - 1:
				joined.append([lhs_classes[aa], rep, 0])
			if not joined:
				raise ValueError("no joined class to count the copy in (the reference's libbio_assert(!joined_path_eq_classes.empty()))")
			joined[-1][2] += 1
	return distinct, int(order[0]), [tuple(j) for j in joined], rhs_classes


def records_at_np(order, div, prev_cut_edge, cut_pair_edge, lhs_classes, with_joined):
	"""records_at() vectorised (held against it in tests/test_pbwt_ref.py): a copy's representative is the copy at the last class start at
	or before it, a joined class's size the distance to the next start."""
	order = np.asarray(order, dtype=np.int64)
	div = np.asarray(div, dtype=np.int64)
	lhs_classes = np.asarray(lhs_classes, dtype=np.int64)
	n = order.size
	starts = (0 == div) | (div - 1 > prev_cut_edge)
	last = np.maximum.accumulate(np.where(starts, np.arange(n), -1))
	rep = np.where(last >= 0, order[np.maximum(last, 0)], PLOIDY_MAX)
	rhs_classes = np.full(n, PLOIDY_MAX, dtype=np.int64)
	rhs_classes[order] = rep
	joined = []
	if with_joined:
		at = np.flatnonzero((0 == div) | (div - 1 > cut_pair_edge))
		if 0 == at.size or 0 != at[0]:
			raise ValueError("no joined class to count the copy in (the reference's libbio_assert(!joined_path_eq_classes.empty()))")
		sizes = np.diff(np.concatenate([at, [n]]))
		joined = [(int(l), int(r), int(z)) for l, r, z in zip(lhs_classes[order[at]], rep[at], sizes)]
	return int(starts.sum()), int(order[0]), joined, rhs_classes


def walk_records(bits, n_copies, cut_edge, first, end, start_edge=None, state=None, literal=False):
	"""The cuts [first, end) (first >= 1) of one chunk, from the state after `start_edge` (default cut_edge[first - 1]) edges.
	Returns a list of dicts per cut: distinct, first_class, first_is_ref, joined (None for cut 1)."""
	if first >= end:
		return []
	b = bits[:n_copies]
	cut_edge = [int(e) for e in cut_edge]
	edge = cut_edge[first - 1] if start_edge is None else int(start_edge)
	order, div = state if state is not None else state_at(b, edge)
	one_step, at_cut = (step, records_at) if literal else (step_np, records_at_np)
	for edge in range(edge, cut_edge[first - 1]):
		order, div = one_step(order, div, b[:, edge], edge)
	edge = cut_edge[first - 1]
	classes = [PLOIDY_MAX] * n_copies
	if first >= 2:                                                              # what the cut before the chunk's first one left behind
		_, _, _, classes = at_cut(order, div, cut_edge[first - 2], 0, classes, False)
	out = []
	for j in range(first, end):
		first_is_ref = True
		for edge in range(edge, cut_edge[j]):
			order, div = one_step(order, div, b[:, edge], edge)
			first_is_ref = first_is_ref and not b[order[0], edge]               # :454-462
		edge = cut_edge[j]
		distinct, first_class, joined, classes = at_cut(order, div, cut_edge[j - 1], cut_edge[j - 2] if j >= 2 else 0, classes, j >= 2)
		out.append(dict(distinct=distinct, first_class=first_class, first_is_ref=int(first_is_ref), joined=joined if j >= 2 else None))
	return out


# ---- the greedy assignment (founder_sequence_greedy_output.cc:254-457), literally ------------------------------------------------

class _Multimap:
	"""std::multimap <ploidy_type, ploidy_type>: ordered by key, equal keys in insertion order."""

	def __init__(self):
		self.items = []

	def emplace(self, key, value):
		self.items.insert(bisect.bisect_right([k for k, _ in self.items], key), (key, value))

	def pop_key(self, key):
		i = bisect.bisect_left([k for k, _ in self.items], key)
		if i < len(self.items) and self.items[i][0] == key:
			return self.items.pop(i)[1]
		return None

	def pop_first(self):
		return self.items.pop(0)[1]


def greedy_assignment(records, n_copies, founder_count, keep_ref_edges=False):
	"""`records` = walk_records(..., 1, n_cuts) of a whole cut list with at least three cuts.  Returns assigned_samples column-major
	(founders in columns: [founder][cut]), as the goldens hold it.  The joined classes are sorted by size with a STABLE sort; the
	reference's std::sort leaves the order of equal sizes open, so a caller compares only where no tie decides (see test_pbwt_ref.py)."""
	rows = len(records)
	assigned = [[PLOIDY_MAX] * founder_count for _ in range(rows)]
	by_class = _Multimap()
	lhs_distinct = rhs_distinct = 0
	lhs_first_is_ref = rhs_first_is_ref = True
	lhs_first_class = rhs_first_class = 0
	for idx, rec in enumerate(records):
		lhs_distinct, lhs_first_class = rhs_distinct, rhs_first_class
		rhs_distinct, rhs_first_class = rec["distinct"], rec["first_class"]
		lhs_first_is_ref, rhs_first_is_ref = rhs_first_is_ref if idx else True, bool(rec["first_is_ref"])
		if 0 == idx:
			continue
		joined = sorted(rec["joined"], key=lambda j: j[2])
		if not keep_ref_edges and lhs_first_is_ref and rhs_first_is_ref:
			joined = [j for j in joined if not (j[0] == lhs_first_class and j[1] == rhs_first_class)]
		reserved = [False] * n_copies
		if 1 == idx:
			remaining_founders = founder_count
			remaining_reserved = min(remaining_founders, lhs_distinct)
			remaining_founders -= remaining_reserved
			founder_idx = 0

			def do_assign(j):
				nonlocal founder_idx
				by_class.emplace(j[0], founder_idx)
				assigned[0][founder_idx] = j[0]
				founder_idx += 1

			for j in reversed(joined):
				if reserved[j[0]]:
					if remaining_founders:
						remaining_founders -= 1
						do_assign(j)
				elif remaining_reserved:
					remaining_reserved -= 1
					reserved[j[0]] = True
					do_assign(j)
			while remaining_founders:
				if not joined:
					raise ValueError("no joined class to fill the founders with (the reference loops for ever)")
				for j in reversed(joined):
					if not remaining_founders:
						break
					remaining_founders -= 1
					do_assign(j)
			reserved = [False] * n_copies
		arbitrarily = []
		remaining_founders = founder_count
		remaining_reserved = min(remaining_founders, rhs_distinct)
		remaining_founders -= remaining_reserved

		def try_assign(j):
			founder = by_class.pop_key(j[0])
			if founder is None:
				return False
			assigned[idx][founder] = j[1]
			return True

		is_first = True
		stop = False
		while not stop:
			did_assign = False
			for j in reversed(joined):
				if reserved[j[1]]:
					if remaining_founders:
						if try_assign(j):
							did_assign = True
							remaining_founders -= 1
					elif not is_first:
						stop = True
						break
				elif remaining_reserved:
					remaining_reserved -= 1
					if try_assign(j):
						reserved[j[1]] = True
					else:
						arbitrarily.append(j[1])
			if stop or not remaining_founders:
				break
			if is_first:
				is_first = False
				continue
			if not did_assign:
				break
		for rhs_rep in arbitrarily:
			if not reserved[rhs_rep]:
				assigned[idx][by_class.pop_first()] = rhs_rep
				reserved[rhs_rep] = True
		while by_class.items:
			if not joined:
				raise ValueError("no joined class to connect the remaining founders to")
			for j in reversed(joined):
				if not by_class.items:
					break
				assigned[idx][by_class.pop_first()] = j[1]
		by_class = _Multimap()
		for founder, cls in enumerate(assigned[idx]):
			by_class.emplace(cls, founder)
	return [assigned[r][f] for f in range(founder_count) for r in range(rows)]


def has_size_ties(records):
	"""True when some cut's joined classes hold two of the same size: the reference's std::sort may order them either way."""
	for rec in records:
		if rec["joined"]:
			sizes = [j[2] for j in rec["joined"]]
			if len(set(sizes)) != len(sizes):
				return True
	return False


# ---- inputs of the tests' own choosing -------------------------------------------------------------------------------------------

def chain_graph_arrays(n_edges, seed=0):
	"""A chain of n_edges + 1 nodes with one ALT edge from every node but the last to the next one: every node is a candidate, edge e
	leaves node e.  Aligned positions are irregular (2 .. 5 columns per node) so that distances differ.  Returns the arrays
	oracle.graph_from_arrays takes, without the path matrix, and the reference sequence."""
	rng = np.random.default_rng(9000 + seed)
	n = n_edges + 1
	reference_positions = np.arange(n, dtype=np.uint64) * 2
	aligned_positions = np.concatenate([[0], np.cumsum(rng.integers(2, 6, n - 1))]).astype(np.uint64)
	alt_edge_targets = np.arange(1, n, dtype=np.uint64)
	alt_edge_count_csum = np.minimum(np.arange(n + 1), n_edges).astype(np.uint64)
	label_offsets = np.arange(n_edges + 1, dtype=np.uint64)
	return dict(reference_positions=reference_positions, aligned_positions=aligned_positions, alt_edge_targets=alt_edge_targets,
		alt_edge_count_csum=alt_edge_count_csum, label_offsets=label_offsets, label_bytes=b"C" * n_edges), b"A" * int(reference_positions[-1])


def pack_paths(bits, path_rows, path_cols):
	"""bits[copy, edge] as paths_by_chrom_copy_and_edge: rows = edges, columns = copies, column-major u64 words (variant_graph.hh)."""
	n_copies, n_edges = bits.shape
	assert 0 == path_rows % 64 and 0 == path_cols % 64 and n_edges <= path_rows and n_copies <= path_cols
	full = np.zeros((path_cols, path_rows), dtype=bool)
	full[:n_copies, :n_edges] = bits
	return np.packbits(full, axis=1, bitorder="little").view("<u8").reshape(-1).copy()


def unpack_paths(words, path_rows, path_cols):
	"""The inverse: bits[copy, edge] of the whole padded matrix."""
	w = np.ascontiguousarray(words, dtype="<u8").reshape(path_cols, path_rows // 64)
	return np.unpackbits(w.view(np.uint8), axis=1, bitorder="little").astype(bool)


def round64(n):
	return (n + 63) // 64 * 64


FAMILIES = ("dense", "sparse", "clones", "constant_columns", "lane_blocks", "alternating", "identity", "genotypes")


def family(name, n_copies, n_edges, seed=0, per=1):
	"""bits[copy, edge] of the named family; `per` = the copies a thread of the kernels holds (block lengths follow it)."""
	rng = np.random.default_rng([seed, n_copies, n_edges, FAMILIES.index(name)])
	if "dense" == name:
		return rng.random((n_copies, n_edges)) < 0.5
	if "sparse" == name:
		return rng.random((n_copies, n_edges)) < 0.02
	if "clones" == name:                                                        # many identical copies: a handful of haplotypes dealt at random
		haplotypes = rng.random((7, n_edges)) < 0.3
		return haplotypes[rng.integers(0, 7, n_copies)]
	if "constant_columns" == name:                                              # all-zero and all-one columns, the first and the last among them
		bits = rng.random((n_copies, n_edges)) < 0.5
		for e in range(n_edges):
			if e in (0, n_edges - 1) or 0 == e % 5:
				bits[:, e] = bool((e // 5 + (e == n_edges - 1)) & 1)
		return bits
	if "lane_blocks" == name:                                                   # a column's ones = the copies of one wave or of one 16-lane row
		bits = np.zeros((n_copies, n_edges), dtype=bool)
		for e in range(n_edges):
			length = (64 if e & 1 else 16) * per
			start = int(rng.integers(0, max(1, (n_copies + length - 1) // length))) * length
			bits[start:start + length, e] = True
		return bits
	if "alternating" == name:                                                   # blocks of `per` copies, shifted from column to column
		c = np.arange(n_copies)[:, None]
		e = np.arange(n_edges)[None, :]
		return 1 == ((c + e * (per // 2 + 1)) // per) % 2
	if "identity" == name:                                                      # column e is set for copy e alone
		return np.arange(n_copies)[:, None] == np.arange(n_edges)[None, :]
	if "genotypes" == name:                                                     # what diploid samples with real-looking genotypes give
		import synth
		ref = synth.random_reference(rng, 40 * n_edges + 100)
		recs = synth.random_records(rng, ref, n_edges, (n_copies + 1) // 2, mix=(0.8, 0.1, 0.1), density=0.15)
		bits = np.zeros((n_copies, n_edges), dtype=bool)
		for k, rec in enumerate(recs[:n_edges]):
			gt = np.asarray(rec[3])
			bits[:, k] = (gt.reshape(-1) != 0)[:n_copies]
		return bits
	raise ValueError(name)


def every_node_candidates(n_edges, aligned_positions):
	"""The candidate list the search makes on a chain graph: the sentinel, then every node (the first shares edge 0 with the sentinel)."""
	cand_edge = [0] + list(range(n_edges + 1))
	cand_node = [0] + list(range(n_edges + 1))
	return cand_edge, cand_node, [int(aligned_positions[n]) for n in cand_node]


def collision_case():
	"""Five copies whose neighbours in the order differ last at edges 0, 1, 1292 and 2585, and a candidate list without the double edge 0
	(the sentinel, then node c at edge c): at the last candidates the bins are 1, 2, 1293 and 2586 -- 1 and 1293 share a slot of the
	2048-slot table, 2 and 2586 one of the 4096-slot table.  Returns (bits, n_edges, cand_edge)."""
	n_edges = 2600
	bits = np.zeros((5, n_edges), dtype=bool)
	for copy, e in ((1, 0), (2, 1), (3, 1292), (4, 2585)):
		bits[copy, e] = True
	return bits, n_edges, list(range(n_edges + 1))


def hash_slot(key, slots):
	"""The kernels' table slot of a bin (founder_kernels.hpp: pbwt_bin_add)."""
	return ((key * 2654435761) & 0xFFFFFFFF) >> 20 & (slots - 1)
