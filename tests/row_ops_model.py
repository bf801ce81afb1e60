"""A plain model of the row alignment ops (include/v2m_hip.h, "row alignment ops") and of the chain file made from them.  TEST INFRASTRUCTURE ONLY.

  ops_from_masks      the contract itself in numpy: per aligned column "the REF row holds a byte" and "the row holds a byte", classes M / I / D /
                      skipped, run-length encoded over the non-skipped columns;
  column_walk         output_sequence() (sequence_writer.cc:22-85) with the column of every byte, for any row, cuts included: the aligned row and
                      both masks.  Padding is what the walk pads with, never what a byte looks like: a '-' in the reference or in a label is a byte;
  seam_masks          the same masks for a seam_graphs.SeamGraph row from the builder's own column description (no walk: those graphs have up
                      to a million nodes; their bytes are ACGT / acgt, so padding is exactly the '-' columns of the model's rows);
  chain_text          the UCSC chain of a row, written from the format's description;
  the ops graphs      hand-made graphs (seam_graphs.Builder) that put runs, breakpoints and skipped stretches at the ops kernels' seams, and
                      reach(), which recomputes from the masks -- with the constants of csrc/kernels.hpp -- what each graph is meant to place;
  the scan graphs     graphs of 513 to 578 tiles that put runs, dense tiles and all-skipped stretches at the seams of the one-workgroup scan
                      kernels (a scan wave is 64 tiles, a scan block 256), and scan_reach(), reach()'s vectorised counterpart for them."""

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


# ---- graphs for the scan kernels' seams --------------------------------------------------------------------------------------------------
# scan_row_ops_kernel, scan_row_ops_eqx_kernel and scan_tile_counts_kernel walk a row's tiles in rounds of 256, one tile per thread: tile i is
# lane i % 64 of scan wave (i % 256) / 64 of scan block i / 256.  The graphs below put runs, dense tiles and all-skipped stretches at those
# seams.  Their substitution sites make no difference to the unsplit ops; row_ops_eqx_model.scan_graph() gives the same graphs with the
# bytes of those sites chosen (notes["eqx_plan"]), so that one Builder layout serves both class sets.

SCAN_WAVE, SCAN_BLOCK = 64, 256          # tiles per scan wave and per scan block (a round of the scan kernels)


def _seam_site(b, column, n=40):
	"""n reference bytes, half of them either side of `column`, under two edges: a label of one byte (the row is M, then a D run across
	the column) and one of n bytes (M all along; an X run once row_ops_eqx_model has chosen its bytes)."""
	b.ref_to(column - n // 2)
	return b.add_site([1, n], n, n)


def _stretch(b, first_tile, end_column, T, insertion=True, back=5, ahead=5):
	"""An all-padding stretch from column 0 of first_tile to end_column: the reference byte on the last column of the tile before it, padding
	up to end_column, a one-column substitution site there.  Edges, by name: DD a deletion from `back` columns before the stretch to `ahead`
	columns after it (D ... skipped ... D); DM one that ends on the first column after it (D ... skipped ... M); ins an insertion that fills
	the stretch (an I run through every tile of it); sub / after one-byte labels on the reference byte before and on the one after."""
	begin = first_tile * T - 1
	b.ref_to(begin - back)
	b.add_ref(back)
	e = {"DD": b.edge(begin - back, end_column + ahead, 0), "DM": b.edge(begin - back, end_column, 0)}
	span = end_column - begin
	got = b.add_site([span, 1] if insertion else [1], span)
	e["sub"] = got[-1]
	if insertion:
		e["ins"] = got[0]
	e["after"] = b.add_site([1], 1, 1)[0]
	b.add_ref(ahead + 3)
	return e


@functools.lru_cache(maxsize=None)
def scan_wave_graph():
	"""513 tiles and a few columns, every scan block live:
	  tiles 63, 64, 255, 256     every column a breakpoint (M I M I ...): the last and first tile of a scan wave and of a scan block;
	  127|128 and 511|512        a D run and a substituted run across a wave seam and across a block seam;
	  tiles 192 ... 196 (+ 100 columns)  all padding: a skipped stretch that begins at lane 0 of a wave and ends inside it;
	  tiles 320 ... 383          all padding: one whole scan wave, from its lane 0 to its lane 63, with live waves before and after it in the block.
	Copies: 0 every dense tile (65 536 ops from them), the insertion over the skipped wave, the substituted runs; 1 dense tiles 63 and 256, D
	either side of the skipped wave, the D runs across the seams; 2 dense tiles 64 and 255, D before the skipped wave and M after it; 3 - 5 the
	one-byte substitutions either side of the skipped wave: both, the later, the earlier; 6 those either side of the shorter stretch."""
	K = sgs.kernel_constants()
	T = K.kTileBytes
	b = sgs.Builder(9600)
	dense = {}
	b.ref_to(63 * T)
	dense[63] = b.add_sites(T // 2, 2, 1, 2)
	dense[64] = b.add_sites(T // 2, 2, 1, 2)
	b.add_ref(9)
	dw, xw = _seam_site(b, 128 * T)
	s2 = _stretch(b, 192, 197 * T + 100, T, insertion=False)
	b.ref_to(255 * T)
	dense[255] = b.add_sites(T // 2, 2, 1, 2)
	dense[256] = b.add_sites(T // 2, 2, 1, 2)
	b.add_ref(9)
	s1 = _stretch(b, 320, 384 * T, T)
	db, xb = _seam_site(b, 512 * T)
	b.add_ref(700)
	all_of = lambda t: list(range(dense[t], dense[t] + T // 2))
	copies = [
		all_of(63) + all_of(64) + [xw] + all_of(255) + all_of(256) + [s1["ins"], xb],
		all_of(63) + [dw] + all_of(256) + [s1["DD"], db],
		all_of(64) + all_of(255) + [s1["DM"]],
		[s1["sub"], s1["after"]],
		[s1["after"]],
		[s1["sub"], dw],
		[s2["sub"], s2["after"], xb],
	]
	sg = b.finish([sorted(c) for c in copies], "scan_waves")
	x_edges = [xw, xb, s1["sub"], s1["after"], s2["sub"], s2["after"]]
	plan = {e: "X" * int(sg.label_len[e]) for e in x_edges}
	for t in dense:                                       # the M columns of the dense tiles: = X = X ...
		plan.update({e: "=X"[(e - dense[t]) & 1] for e in all_of(t)})
	sg.notes.update(dense=dense, stretches={"wave": s1, "lane_0": s2}, seams={"wave": (dw, xw), "block": (db, xb)}, eqx_plan=plan, skipped=[(192, 197), (320, 384)])
	sg.notes["windows"] = [
		("begins_in_skipped_wave", 330 * T + 77, 420 * T + 5),                  # the window's first 53 tiles hold no byte
		("empty_then_full_at_its_tile_256", 128 * T, 400 * T),                   # its tiles 192 ... 255 are the skipped wave, its tile 256 is full
	]
	return sg


@functools.lru_cache(maxsize=None)
def scan_block_graph(extra_waves):
	"""Scan block 0 live, then all padding from tile 256 on: one whole scan block (extra_waves = 0: the first live tile is tile 512, lane 0 of
	wave 0 of the next block) or a scan block and the first wave of the next (extra_waves = 1: tile 576, in wave 1, which gets its carry past a
	zero entry of its own block).  Copies: 0 the insertion over the stretch (an I run across three wave seams and, with extra_waves, the block
	seam 511|512); 1 D either side; 2 D before and M after; 3 - 5 the one-byte substitutions either side: both, the later, the earlier."""
	K = sgs.kernel_constants()
	T = K.kTileBytes
	b = sgs.Builder(9610 + extra_waves)
	s = _stretch(b, SCAN_BLOCK, (2 * SCAN_BLOCK + extra_waves * SCAN_WAVE) * T, T)
	b.add_ref(T + 300)                                      # the first tile after the stretch is full
	sg = b.finish([[s["ins"]], [s["DD"]], [s["DM"]], [s["sub"], s["after"]], [s["after"]], [s["sub"]]], "scan_block_%d" % extra_waves)
	sg.notes.update(stretches={"block": s}, eqx_plan={s["sub"]: "X", s["after"]: "X"}, skipped=[(SCAN_BLOCK, 2 * SCAN_BLOCK + extra_waves * SCAN_WAVE)])
	sg.notes["windows"] = [
		("begins_in_skipped_block", 300 * T + 123, sg.length),
		("empty_then_full_at_its_tile_256", (SCAN_BLOCK + extra_waves * SCAN_WAVE) * T, sg.length),      # every tile of it up to 255 is empty
	]
	return sg


def scan_graphs():
	return [scan_wave_graph(), scan_block_graph(0), scan_block_graph(1)]


def tile_ends(cls, n_tiles, T):
	"""Per tile the first and the last non-zero class (0: the tile is all skipped), and the last non-zero class at or before each tile's
	end (0: none yet): the carry the scan hands to the next tile."""
	per_tile = cls.reshape(n_tiles, T)
	mask = per_tile != 0
	live = mask.any(axis=1)
	rows = np.arange(n_tiles)
	first = np.where(live, per_tile[rows, mask.argmax(axis=1)], 0)
	last = np.where(live, per_tile[rows, T - 1 - mask[:, ::-1].argmax(axis=1)], 0)
	at = np.maximum.accumulate(np.where(live, rows, -1))
	carried = np.where(at >= 0, last[np.maximum(at, 0)], 0)
	return first, last, carried, live, per_tile


def scan_reach_classes(cls, T, names, out):
	"""What one row's classes (0 = skipped; padded to whole tiles) place at the scan kernels' seams.  names: class code -> letter."""
	n_tiles = cls.size // T
	first, last, carried, live, per_tile = tile_ends(cls, n_tiles, T)
	bytes_in = (per_tile >= 2).sum(axis=1)                    # the row's bytes: classes with the row bit (2, 3, 7)
	for t in range(SCAN_WAVE, n_tiles, SCAN_WAVE):
		where = "block" if 0 == t % SCAN_BLOCK else "wave"
		if live[t - 1] and live[t]:
			out.add("%s_seam_merge_%s" % (where, names[int(first[t])]) if last[t - 1] == first[t] else "%s_seam_break" % where)
		if (0 == bytes_in[t - 1] and T == bytes_in[t]) or (T == bytes_in[t - 1] and 0 == bytes_in[t]):
			out.add("empty_tile_count_at_%s_seam" % where)
	# a dense tile: no column skipped, every column's class differs from the one before it
	for t in np.flatnonzero(per_tile.all(axis=1) & (per_tile[:, 1:] != per_tile[:, :-1]).all(axis=1)).tolist():
		for name, hit in (("dense_tile_last_of_wave", t % SCAN_WAVE == SCAN_WAVE - 1 and t % SCAN_BLOCK != SCAN_BLOCK - 1), ("dense_tile_first_of_wave", t % SCAN_WAVE == 0 and t % SCAN_BLOCK != 0),
				("dense_tile_last_of_block", t % SCAN_BLOCK == SCAN_BLOCK - 1), ("dense_tile_first_of_block", t % SCAN_BLOCK == 0 and t > 0)):
			if hit:
				out.add(name)
	# maximal runs of all-skipped tiles with live tiles either side
	edges = np.flatnonzero(np.diff(np.r_[True, live, True].astype(np.int8)))
	for a, z in zip(edges[0::2].tolist(), edges[1::2].tolist()):          # tiles [a, z) are skipped
		if 0 == a or z >= n_tiles:
			continue
		before, after = int(carried[a - 1]), int(first[z])
		same = "equal" if before == after else "different"
		w0, w1 = -(-a // SCAN_WAVE), z // SCAN_WAVE                          # whole scan waves [w0, w1) lie inside
		whole_blocks = [k for k in range(-(-a // SCAN_BLOCK), z // SCAN_BLOCK)]
		for w in range(w0, w1):
			blk = w // 4
			if live[blk * SCAN_BLOCK:w * SCAN_WAVE].any() and live[(w + 1) * SCAN_WAVE:(blk + 1) * SCAN_BLOCK].any():
				out.add("skipped_wave_" + same)
				if before == after and names[before] in "DX":
					out.add("carried_%s_through_skipped_wave" % names[before])
				if names[before] == "D" and names[after] in "M=":
					out.add("D_skipped_wave_M")
		if whole_blocks:
			out.add("skipped_block_" + same)
			if before == after and names[before] in "DX":
				out.add("carried_%s_through_skipped_block" % names[before])
			if names[before] == "D" and names[after] in "M=":
				out.add("D_skipped_block_M")
			if z // SCAN_BLOCK == whole_blocks[-1] + 1 and z % SCAN_BLOCK >= SCAN_WAVE:
				out.add("skipped_block_into_later_wave")
		if 0 == a % SCAN_WAVE and z % SCAN_WAVE and z // SCAN_WAVE == a // SCAN_WAVE:
			out.add("skipped_from_lane_0")                                   # the first live tile of the wave has no live lane before it
		if 0 == z % SCAN_WAVE and z % SCAN_BLOCK:
			out.add("skipped_up_to_lane_63")                                 # lane 0 of the next wave looks at the waves before it
	return out


def scan_reach(sg, rows=None):
	"""What the rows of a scan graph place, recomputed from the masks: a set of names.  Vectorised per row (reach() slices per tile and row,
	which takes minutes on graphs of 600 tiles)."""
	T = sgs.kernel_constants().kTileBytes
	n_tiles = -(-sg.length // T)
	out = set()
	for row in (sg.rows if rows is None else rows):
		ref_is_base, row_is_base = seam_masks(sg, row)
		cls = np.zeros(n_tiles * T, dtype=np.uint8)
		cls[:sg.length] = classes(ref_is_base, row_is_base)
		scan_reach_classes(cls, T, "_DIM", out)
		if len(seam_ops(sg, row)[0]) > 65535:
			out.add("row_with_more_than_65535_ops")
	return out


SCAN_REACHED_BY = {
	"scan_waves": {"wave_seam_merge_M", "wave_seam_merge_D", "wave_seam_break", "block_seam_merge_M", "block_seam_merge_D", "block_seam_break",
		"skipped_wave_equal", "skipped_wave_different", "carried_D_through_skipped_wave", "D_skipped_wave_M", "skipped_from_lane_0", "skipped_up_to_lane_63",
		"dense_tile_last_of_wave", "dense_tile_first_of_wave", "dense_tile_last_of_block", "dense_tile_first_of_block", "row_with_more_than_65535_ops",
		"empty_tile_count_at_wave_seam"},
	"scan_block_0": {"skipped_block_equal", "skipped_block_different", "carried_D_through_skipped_block", "D_skipped_block_M", "wave_seam_merge_I",
		"empty_tile_count_at_block_seam"},
	"scan_block_1": {"skipped_block_equal", "skipped_block_different", "skipped_block_into_later_wave", "carried_D_through_skipped_block", "D_skipped_block_M",
		"wave_seam_merge_I", "block_seam_merge_I", "empty_tile_count_at_block_seam", "empty_tile_count_at_wave_seam"},
}


REACHED_BY = {
	"ops_boundary": {"length_not_tile_multiple", "first_column_D", "last_column_D", "break_at_tile_column_0", "break_at_tile_last_column", "break_at_chunk_edge",
		"break_at_slot_edge", "I_then_D_in_one_edge", "I_then_D_across_two_edges", "run_D_merges_across_tiles", "run_M_merges_across_tiles", "run_ends_at_tile_boundary"},
	"ops_skipped_1": {"1_skipped_tiles_between_equal_classes", "tile_is_one_I_run", "run_I_merges_across_tiles"},
	"ops_skipped_2": {"2_skipped_tiles_between_equal_classes", "tile_is_one_I_run"},
	"ops_dense": {"every_column_a_breakpoint", "I_from_column_1"},
	"ops_deletion": {"tile_is_one_D_run_through_crossing_list_and_long_queue", "run_D_merges_across_tiles"},
	"ops_edgeless": {"no_edges", "length_not_tile_multiple"},
}
