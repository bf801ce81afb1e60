"""A plain model of the row alignment ops (include/v2m_hip.h, "row alignment ops") and of the chain file made from them.  TEST INFRASTRUCTURE ONLY.

  ops_from_masks      the contract itself in numpy: per aligned column "the REF row holds a byte" and "the row holds a byte", classes M / I / D /
                      skipped, run-length encoded over the non-skipped columns;
  column_walk         output_sequence() (sequence_writer.cc:22-85) with the column of every byte, for any row, cuts included: the aligned row and
                      both masks.  Padding is what the walk pads with, never what a byte looks like: a '-' in the reference or in a label is a byte;
  seam_masks          the same masks for a seam_graphs.SeamGraph row from the builder's own column description (no walk: those graphs have up
                      to a million nodes; their bytes are ACGT / acgt, so padding is exactly the '-' columns of the model's rows);
  chain_text          the UCSC chain of a row, written from the format's description;
  the ops graphs      hand-made graphs (seam_graphs.Builder) that put runs, breakpoints and skipped stretches at the ops kernels' seams, and
                      reach(), which recomputes from the masks -- with the constants of csrc/kernels.hpp -- what each graph is meant to place."""

import functools

import numpy as np

import oracle
import seam_graphs as sgs

PLOIDY_MAX = oracle.PLOIDY_MAX
OP_M, OP_I, OP_D = 0, 1, 2
_OP_OF_CLASS = np.array([255, OP_D, OP_I, OP_M], dtype=np.uint32)    # class = ref + 2 * row


# ---- the contract ------------------------------------------------------------------------------------------------------------------------

def classes(ref_is_base, row_is_base):
	"""Per column: 0 skipped, 1 D (ref only), 2 I (row only), 3 M."""
	return np.asarray(ref_is_base, dtype=np.uint8) + 2 * np.asarray(row_is_base, dtype=np.uint8)


def ops_from_masks(ref_is_base, row_is_base):
	"""(n, 2) uint32 of (op, length): the run-length encoding of the classes of the non-skipped columns, in column order."""
	cls = classes(ref_is_base, row_is_base)
	seq = cls[cls != 0]
	if 0 == seq.size:
		return np.zeros((0, 2), dtype=np.uint32)
	starts = np.flatnonzero(np.r_[True, seq[1:] != seq[:-1]])
	lengths = np.diff(np.r_[starts, seq.size])
	return np.stack([_OP_OF_CLASS[seq[starts]], lengths.astype(np.uint32)], axis=1).astype(np.uint32)


def check_invariants(ops, ref_length, row_length, is_ref_row=False):
	ops = np.asarray(ops).reshape(-1, 2)
	assert np.all(ops[:, 1] > 0), "an op of length 0"
	assert np.all(ops[:, 0] <= OP_D)
	assert np.all(ops[1:, 0] != ops[:-1, 0]), "two neighbouring ops with the same code"
	lengths = ops[:, 1].astype(np.int64)
	assert int(lengths[ops[:, 0] != OP_I].sum()) == ref_length
	assert int(lengths[ops[:, 0] != OP_D].sum()) == row_length
	if is_ref_row:
		assert ops.tolist() == ([[OP_M, ref_length]] if ref_length else [])


# ---- the walk ----------------------------------------------------------------------------------------------------------------------------

def column_walk(g, copy_index=PLOIDY_MAX, cuts=None):
	"""The row output_sequence() writes, column by column: (aligned row bytes, ref_is_base, row_is_base).  At each node the walk visits it
	takes the first ALT edge of the node that is set in the current copy (label, then padding up to the target node), else the reference
	up to the next node (then padding); a row with cuts starts as REF and switches copy at each cut node.  Written over the set edges of the
	row instead of node by node: between two taken edges every node is left by its reference segment, which is the REF row's."""
	rp = np.asarray(g.reference_positions, dtype=np.int64)
	ap = np.asarray(g.aligned_positions, dtype=np.int64)
	csum = np.asarray(g.alt_edge_count_csum, dtype=np.int64)
	tgt = np.asarray(g.alt_edge_targets, dtype=np.int64)
	lo = np.asarray(g.label_offsets, dtype=np.int64)
	labels = np.frombuffer(g.label_bytes, dtype=np.uint8)
	ref = np.frombuffer(g.ref, dtype=np.uint8)
	N, E, L = rp.size, tgt.size, int(ap[-1])
	# the REF row: node n's segment ref[rp[n] : rp[n + 1]) from column ap[n] on
	seg = np.diff(rp)
	ref_is_base = np.zeros(L, dtype=bool)
	cols = np.repeat(ap[:-1] - rp[:-1], seg) + np.arange(int(rp[-1]), dtype=np.int64) if N > 1 else np.zeros(0, dtype=np.int64)
	ref_is_base[cols] = True
	row = np.full(L, ord("-"), dtype=np.uint8)
	row[cols] = ref[:cols.size]
	row_is_base = ref_is_base.copy()
	if E:
		# the copy in force at every node, hence for every edge (the edges of node n are [csum[n], csum[n + 1]))
		src = np.searchsorted(csum, np.arange(E), side="right") - 1
		node_copy = np.full(N, PLOIDY_MAX if cuts else copy_index, dtype=np.int64)
		for node, copy in (cuts or []):
			node_copy[int(node):] = copy
		words = np.asarray(g.paths_by_chrom_copy_and_edge, dtype=np.uint64)
		words_per_copy = g.path_rows // 64
		edge_copy = node_copy[src]
		has_copy = edge_copy != PLOIDY_MAX
		word = np.where(has_copy, edge_copy, 0) * words_per_copy + np.arange(E) // 64
		is_set = has_copy & (((words[word] >> (np.arange(E, dtype=np.uint64) & np.uint64(63))) & np.uint64(1)) == 1)
		at = 0
		for e in np.flatnonzero(is_set).tolist():
			n = int(src[e])
			if n < at:
				continue                  # the walk jumped over the edge's node, or has left it by an earlier edge
			b, en = int(ap[n]), int(ap[int(tgt[e])])
			k = int(lo[e + 1] - lo[e])
			row[b:en] = ord("-")
			row_is_base[b:en] = False
			row[b:b + k] = labels[int(lo[e]):int(lo[e + 1])]
			row_is_base[b:b + k] = True
			at = int(tgt[e])
	return row.tobytes(), ref_is_base, row_is_base


def walk_row(g, r):
	return column_walk(g, cuts=list(r)) if isinstance(r, (list, tuple)) else column_walk(g, copy_index=int(r))


def oracle_row(g, r, unaligned=False):
	if isinstance(r, (list, tuple)):
		return g.output_sequence(g.ref, cuts=list(r), unaligned=unaligned)
	return g.output_sequence(g.ref, copy_index=int(r), unaligned=unaligned)


def model_ops(g, r):
	"""(ops, row length) of row r of an oracle graph."""
	_, ref_is_base, row_is_base = walk_row(g, r)
	return ops_from_masks(ref_is_base, row_is_base), int(row_is_base.sum())


def seam_masks(sg, row):
	return sg.kept, sg.aligned(row) != sgs.GAP


def seam_ops(sg, row):
	ref_is_base, row_is_base = seam_masks(sg, row)
	return ops_from_masks(ref_is_base, row_is_base), int(row_is_base.sum())


def bridges(g):
	"""The nodes no ALT edge jumps over: where a founder row may cut."""
	reach, out = 0, []
	for n in range(g.node_count - 1):
		if n >= reach and n > 0:
			out.append(n)
		for e in range(int(g.alt_edge_count_csum[n]), int(g.alt_edge_count_csum[n + 1])):
			reach = max(reach, int(g.alt_edge_targets[e]))
	return out


def rows_with_cuts(g, seed=5):
	"""REF, every copy, and a few founder rows that cut at nodes no edge jumps over."""
	rows = [PLOIDY_MAX] + list(range(g.total_chromosome_copies))
	br, H = bridges(g), g.total_chromosome_copies
	if br and H:
		rng = np.random.default_rng(seed)
		for k in (1, min(3, len(br)), min(40, len(br))):
			cuts = [0] + sorted(int(x) for x in rng.choice(br, size=k, replace=False))
			copies = [int(x) for x in rng.integers(0, H, size=len(cuts))]
			copies[-1] = PLOIDY_MAX if k > 1 else copies[-1]
			rows.append(list(zip(cuts, copies)))
		rows.append([(br[len(br) // 2], H - 1)])          # REF up to the first cut, which is not node 0
	return rows


# ---- the chain format --------------------------------------------------------------------------------------------------------------------

def chain_text(ops, t_name, t_size, q_name, q_size, chain_id):
	"""UCSC chain, reference (target) -> row (query), both on the + strand:
	  chain score tName tSize + tStart tEnd qName qSize + qStart qEnd id
	  size dt dq        per aligned block but the last: the block's size, then the target / query bases before the next block
	  size              the last block
	  (blank line)
	Blocks are the M ops; dt / dq the D / I lengths between two of them; score the summed M lengths; leading and trailing D / I ops move
	the starts and ends inward.  b"" when there is no M op."""
	ops = [(int(o), int(n)) for o, n in np.asarray(ops, dtype=np.uint64).reshape(-1, 2).tolist()]
	m_at = [i for i, (o, _) in enumerate(ops) if o == OP_M]
	if not m_at:
		return b""
	first, last = m_at[0], m_at[-1]
	t_start = sum(n for o, n in ops[:first] if o == OP_D)
	q_start = sum(n for o, n in ops[:first] if o == OP_I)
	t_end = t_size - sum(n for o, n in ops[last + 1:] if o == OP_D)
	q_end = q_size - sum(n for o, n in ops[last + 1:] if o == OP_I)
	blocks = []          # [size, dt, dq]
	for o, n in ops[first:last + 1]:
		if o == OP_M:
			if blocks and blocks[-1][1] == 0 and blocks[-1][2] == 0:
				blocks[-1][0] += n
			else:
				blocks.append([n, 0, 0])
		elif o == OP_D:
			blocks[-1][1] += n
		else:
			blocks[-1][2] += n
	lines = ["chain %d %s %d + %d %d %s %d + %d %d %d" % (sum(n for o, n in ops if o == OP_M), t_name, t_size, t_start, t_end, q_name, q_size, q_start, q_end, chain_id)]
	lines += ["%d %d %d" % tuple(b) for b in blocks[:-1]] + ["%d" % blocks[-1][0], ""]
	return ("\n".join(lines) + "\n").encode()


def haplotype_chains(g, chromosome_id=None):
	"""The model's chain file for --haplotypes: one chain per chromosome copy, in the A2M output's order, named as one file per sequence is."""
	prefix = (chromosome_id + ".") if chromosome_id else ""
	out, k = [], 0
	for s, sample in enumerate(g.sample_names):
		for c in range(int(g.ploidy_csum[s + 1]) - int(g.ploidy_csum[s])):
			ops, length = model_ops(g, int(g.ploidy_csum[s]) + c)
			k += 1
			out.append(chain_text(ops, prefix + "REF", len(g.ref), "%s%s.%d" % (prefix, sample, 1 + c), length, k))
	return b"".join(out)


def founder_chains(g, cut_positions, assigned_column_major, chromosome_id=None):
	prefix = (chromosome_id + ".") if chromosome_id else ""
	n_rows = len(cut_positions) - 1
	out = []
	for col in range(len(assigned_column_major) // n_rows if n_rows else 0):
		cuts = list(zip(cut_positions[:-1], assigned_column_major[col * n_rows:(col + 1) * n_rows]))
		ops, length = model_ops(g, cuts)
		out.append(chain_text(ops, prefix + "REF", len(g.ref), "%s%d" % (prefix, 1 + col), length, 1 + col))
	return b"".join(out)


# ---- graphs for the ops kernels' seams ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def boundary_graph():
	"""Runs and breakpoints at the tile's, the slot's and the chunk's edges (situations 1, 5, 6, 7, 8 of tests/test_gpu_row_ops.py).
	Copy 0 takes every edge, copy 1 none, copy 2 every other one."""
	K = sgs.kernel_constants()
	T = K.kTileBytes
	b = sgs.Builder(9001)
	e = []
	e += b.add_site([0], 3, 3)                       # the row's first column in D: a deletion without a label at column 0
	b.add_ref(2)
	e += b.add_site([6], 6)                          # M I I I I I ...
	e += b.add_site([0], 4, 4)                       # ... D D D D: an I run directly followed by a D run, across two edges
	b.add_ref(3)
	begin = b.add_ref(1, 5)                          # the same inside one edge: an interval with padding, then one without, under one label of 6
	b.add_ref(4)
	e.append(b.edge(begin, begin + 10, 6))
	b.add_ref(5)
	b.ref_to(1024 - 1)
	e += b.add_site([1], 50, 50)                     # a D run that begins on a 1-KiB slot edge ...
	b.ref_to(2048 + 160 - 1)
	e += b.add_site([1], 16 * 3 + 1, 16 * 3 + 1)     # ... and one that begins and ends on 16-byte chunk edges
	b.ref_to(T - 40)
	e += b.add_site([1], 80, 80)                     # a D run across the boundary of tiles 0 and 1: one op (and so is the M run of the rows that do not take it)
	b.ref_to(2 * T - 30)
	e += b.add_site([1], 30, 30)                     # a D run up to a tile's last column: the M run after it begins at column 0 of tile 2
	b.ref_to(3 * T - 2)
	e += b.add_site([1], 22, 22)                     # a D run that begins on a tile's last column
	b.ref_to(3 * T + 500)
	e += b.add_site([1], 77, 77)                     # the row's last column in D; L is no multiple of the tile
	sg = b.finish([e, [], e[::2], e[1::2]], "ops_boundary")
	sg.notes["edges"] = e
	return sg


@functools.lru_cache(maxsize=None)
def skipped_graph(n_skipped):
	"""An insertion that covers n_skipped whole tiles (1 or 2) and more on either side: the rows that do not take it skip those tiles between
	an M run and an M run (one op), the row that takes it carries an I run through them."""
	K = sgs.kernel_constants()
	T = K.kTileBytes
	b = sgs.Builder(9100 + n_skipped)
	b.ref_to(T - 300)
	span = 300 + n_skipped * T + 200
	e, = b.add_site([span], span)                    # one reference byte, span - 1 padding columns
	b.add_ref(900)
	f, = b.add_site([1], 9, 9)
	b.add_ref(11)
	sg = b.finish([[e], [], [e, f], [f]], "ops_skipped_%d" % n_skipped)
	sg.notes["insertion"] = e
	return sg


@functools.lru_cache(maxsize=None)
def dense_graph():
	"""Tile 0: a 1-base insertion after every base (M I M I ...), all taken by copy 0: every column of the tile is a breakpoint."""
	K = sgs.kernel_constants()
	T = K.kTileBytes
	b = sgs.Builder(9200)
	first = b.add_sites(T // 2, 2, 1, 2)
	b.add_ref(37)
	sg = b.finish([list(range(first, first + T // 2)), [], list(range(first, first + T // 2, 3))], "ops_dense")
	return sg


@functools.lru_cache(maxsize=None)
def deletion_graph():
	"""A deletion over three tiles: the middle one is a single D run, entered through the crossing list and the long-patch queue."""
	K = sgs.kernel_constants()
	T = K.kTileBytes
	b = sgs.Builder(9300)
	b.ref_to(T - 100)
	d, = b.add_site([1], T + 200, T + 200)
	b.add_ref(40)
	f, = b.add_site([3], 3)
	b.add_ref(250)
	sg = b.finish([[d], [], [d, f], [f]], "ops_deletion")
	sg.notes["deletion"] = d
	return sg


@functools.lru_cache(maxsize=None)
def edgeless_graph():
	K = sgs.kernel_constants()
	b = sgs.Builder(9400)
	b.add_ref(K.kTileBytes + 19)
	return b.finish([[], []], "ops_edgeless")


@functools.lru_cache(maxsize=None)
def dash_graph():
	"""A reference and labels with literal '-' bytes (bytes, not padding): 5 nodes, 4 edges, built from flat arrays.
	    columns 0-3 "A-CG" | 4 "T" + 3 padding (edge 0: label "a-c", edge 1: label "-") | 8-10 "-GA" (edge 2: a deletion to the sink, label "-") | 11-12 "C-"."""
	ref = b"A-CGT-GAC-"
	reference_positions = [0, 4, 5, 8, 10]
	aligned_positions = [0, 4, 8, 11, 13]
	targets = [2, 2, 4]
	csum = [0, 0, 2, 3, 3, 3]
	labels = [b"a-c", b"-", b"-"]
	label_offsets = np.r_[0, np.cumsum([len(x) for x in labels])]
	copies = [[0], [1], [2], [0, 2], []]
	bits = np.zeros((64, 64), dtype=bool)
	for c, edges in enumerate(copies):
		bits[c, edges] = True
	words = np.packbits(bits, axis=1, bitorder="little").view("<u8").reshape(-1).copy()
	g = oracle.graph_from_arrays(reference_positions, aligned_positions, targets, csum, label_offsets, b"".join(labels), words, 64, 64, ["S"], [0, len(copies)])
	g.ref = ref
	return g


def ops_seam_graphs():
	return [boundary_graph(), skipped_graph(1), skipped_graph(2), dense_graph(), deletion_graph(), edgeless_graph()]


def many_rows(sg, n):
	"""n rows over REF and the graph's copies, REF rows among them (every fourth)."""
	copies = list(range(len(sg.copies)))
	return [PLOIDY_MAX if 0 == i % 4 else copies[(i - i // 4) % len(copies)] for i in range(n)]


def reach(sg, rows=None):
	"""What the rows of a seam graph place, recomputed from the masks with the kernels' constants: a set of names."""
	K = sgs.kernel_constants()
	T, S = K.kTileBytes, K.kTileBytes // K.kSlots
	tables = sgs.TileTables(sg)
	out = set()
	if sg.length % T:
		out.add("length_not_tile_multiple")
	if 0 == sg.n_edges:
		out.add("no_edges")
	for row in (sg.rows if rows is None else rows):
		ref_is_base, row_is_base = seam_masks(sg, row)
		cls = np.zeros(tables.n_tiles * T, dtype=np.uint8)
		cls[:sg.length] = classes(ref_is_base, row_is_base)
		live = np.flatnonzero(cls)
		seq = cls[live]
		breaks = live[np.r_[True, seq[1:] != seq[:-1]]]            # the columns that start an op
		if cls[0] == 1:
			out.add("first_column_D")
		if cls[1] == 2:
			out.add("I_from_column_1")
		if cls[sg.length - 1] == 1:
			out.add("last_column_D")
		out.update(name for name, hit in (("break_at_tile_column_0", np.any((breaks % T == 0) & (breaks > 0))), ("break_at_tile_last_column", np.any(breaks % T == T - 1)),
			("break_at_chunk_edge", np.any((breaks % 16 == 0) & (breaks % S != 0))), ("break_at_slot_edge", np.any((breaks % S == 0) & (breaks % T != 0)))) if hit)
		# an I op directly followed by a D op: inside one effective edge's span, or across two
		eff = sg.effective(row)
		for k in np.flatnonzero((seq[:-1] == 2) & (seq[1:] == 1)).tolist():
			owner = [next((e for e in eff if sg.begin[e] <= c < sg.end[e]), None) for c in (int(live[k]), int(live[k + 1]))]
			out.add("I_then_D_in_one_edge" if owner[0] == owner[1] else "I_then_D_across_two_edges")
		per_tile = cls.reshape(tables.n_tiles, T)
		empty = ~per_tile.any(axis=1)
		for t in range(1, tables.n_tiles):
			# what is carried over the boundary in front of tile t
			before, after = live[live < t * T], live[live >= t * T]
			if before.size and after.size and not empty[t] and not empty[t - 1] and after[0] == t * T and before[-1] == t * T - 1:
				same = cls[before[-1]] == cls[after[0]]
				out.add(("run_%s_merges_across_tiles" % "_DIM"[cls[after[0]]]) if same else "run_ends_at_tile_boundary")
		t = 0
		while t < tables.n_tiles:
			if not empty[t]:
				t += 1
				continue
			u = t
			while u < tables.n_tiles and empty[u]:
				u += 1
			before, after = live[live < t * T], live[live >= u * T]
			if before.size and after.size and cls[before[-1]] == cls[after[0]]:
				out.add("%d_skipped_tiles_between_equal_classes" % (u - t))
			t = u
		for t in range(tables.n_tiles):
			tile = per_tile[t]
			tile_live = tile[tile != 0]
			n_breaks = int(np.count_nonzero(np.r_[True, tile_live[1:] != tile_live[:-1]])) if tile_live.size else 0
			if n_breaks == T:
				out.add("every_column_a_breakpoint")
			if np.all(tile == 1) and tables.n_cross[t] >= 1 and any(tables.clipped(sg, e, t) > K.kLongPatch for e in tables.cross[t] if e in eff):
				out.add("tile_is_one_D_run_through_crossing_list_and_long_queue")
			if np.all(tile[tile != 0] == 2) and tile_live.size and t > 0 and not empty[t]:
				out.add("tile_is_one_I_run")
	return out


REACHED_BY = {
	"ops_boundary": {"length_not_tile_multiple", "first_column_D", "last_column_D", "break_at_tile_column_0", "break_at_tile_last_column", "break_at_chunk_edge",
		"break_at_slot_edge", "I_then_D_in_one_edge", "I_then_D_across_two_edges", "run_D_merges_across_tiles", "run_M_merges_across_tiles", "run_ends_at_tile_boundary"},
	"ops_skipped_1": {"1_skipped_tiles_between_equal_classes", "tile_is_one_I_run", "run_I_merges_across_tiles"},
	"ops_skipped_2": {"2_skipped_tiles_between_equal_classes", "tile_is_one_I_run"},
	"ops_dense": {"every_column_a_breakpoint", "I_from_column_1"},
	"ops_deletion": {"tile_is_one_D_run_through_crossing_list_and_long_queue", "run_D_merges_across_tiles"},
	"ops_edgeless": {"no_edges", "length_not_tile_multiple"},
}
