"""A plain model of the SPLIT row alignment ops (include/v2m_hip.h, "row alignment ops", V2M_OPS_SPLIT_MATCH) and of the PAF line made from
them.  TEST INFRASTRUCTURE ONLY.

  ops_from_rows       the contract in numpy: the classes of row_ops_model.classes, a byte compare with the case rule on the M columns ('=' or
                      'X'), the same run-length code;
  fold                split ops back to those of flags = 0: 7 / 8 -> 0, equal neighbours merged;
  paf_text            the PAF line of a row, written from the PAF specification (the twelve mandatory columns, NM:i: and cg:Z: as minimap2
                      --eqx -c writes them);
  the eqx graphs      seam_graphs.Builder graphs whose bytes are then chosen (retouch(): '=' or 'X' per label byte, or literal bytes on both
                      sides), which put '=' / 'X' runs at the ops kernels' seams, and reach(), which recomputes from the model what each places;
  the scan graphs     row_ops_model's scan graphs retouched, and scan_reach() over the split classes."""

import functools

import numpy as np

import oracle
import row_ops_model as M
import seam_graphs as sgs

PLOIDY_MAX = M.PLOIDY_MAX
OP_I, OP_D, OP_EQ, OP_X = 1, 2, 7, 8
OPS_SPLIT_MATCH = 0x4
CLS_D, CLS_I, CLS_EQ, CLS_X = 1, 2, 3, 7                  # ref | row << 1 | mismatch << 2
_OP_OF_CLASS = np.array([255, OP_D, OP_I, OP_EQ, 255, 255, 255, OP_X], dtype=np.uint32)


# ---- the contract ------------------------------------------------------------------------------------------------------------------------

def bytes_equal(a, b):
	"""The case rule: a == b, or (a ^ b) == 0x20 and (a | 0x20) in 'a'..'z'."""
	a, b = np.asarray(a, dtype=np.uint8), np.asarray(b, dtype=np.uint8)
	low = a | np.uint8(0x20)
	return (a == b) | (((a ^ b) == 0x20) & (low >= ord("a")) & (low <= ord("z")))


def split_classes(ref_is_base, row_is_base, ref_bytes, row_bytes):
	"""Per column: 0 skipped, 1 D, 2 I, 3 '=', 7 'X'."""
	cls = M.classes(ref_is_base, row_is_base).astype(np.uint8)
	differs = (cls == 3) & ~bytes_equal(ref_bytes, row_bytes)
	cls[differs] = CLS_X
	return cls


def ops_from_classes(cls, op_of_class=_OP_OF_CLASS):
	seq = cls[cls != 0]
	if 0 == seq.size:
		return np.zeros((0, 2), dtype=np.uint32)
	starts = np.flatnonzero(np.r_[True, seq[1:] != seq[:-1]])
	lengths = np.diff(np.r_[starts, seq.size])
	return np.stack([op_of_class[seq[starts]], lengths.astype(np.uint32)], axis=1).astype(np.uint32)


def ops_from_rows(ref_is_base, row_is_base, ref_bytes, row_bytes):
	"""(n, 2) uint32 of (op, length): the run-length encoding of the split classes of the non-skipped columns, in column order."""
	return ops_from_classes(split_classes(ref_is_base, row_is_base, ref_bytes, row_bytes))


def fold(ops):
	"""7 / 8 -> 0, equal neighbours merged: what flags = 0 gives for the same row."""
	out = []
	for op, n in np.asarray(ops, dtype=np.uint64).reshape(-1, 2).tolist():
		op = M.OP_M if op in (OP_EQ, OP_X) else op
		if out and out[-1][0] == op:
			out[-1][1] += n
		else:
			out.append([op, n])
	return np.array(out, dtype=np.uint32).reshape(-1, 2)


def check_invariants(ops, ref_length, row_length, is_ref_row=False):
	ops = np.asarray(ops).reshape(-1, 2)
	assert np.all(ops[:, 1] > 0), "an op of length 0"
	assert np.all(np.isin(ops[:, 0], (OP_I, OP_D, OP_EQ, OP_X))), "an op code that is none of =, X, I, D"
	assert np.all(ops[1:, 0] != ops[:-1, 0]), "two neighbouring ops with the same code"
	lengths = ops[:, 1].astype(np.int64)
	assert int(lengths[ops[:, 0] != OP_I].sum()) == ref_length
	assert int(lengths[ops[:, 0] != OP_D].sum()) == row_length
	M.check_invariants(fold(ops), ref_length, row_length, is_ref_row=is_ref_row)
	if is_ref_row:
		assert ops.tolist() == ([[OP_EQ, ref_length]] if ref_length else [])


def model_ops(g, r):
	"""(split ops, row length) of row r of an oracle graph: the walk of row_ops_model.column_walk, the REF row's bytes under the row's."""
	ref_row, _, _ = M.column_walk(g)
	row, ref_is_base, row_is_base = M.walk_row(g, r)
	return ops_from_rows(ref_is_base, row_is_base, np.frombuffer(ref_row, np.uint8), np.frombuffer(row, np.uint8)), int(row_is_base.sum())


def seam_classes(sg, row):
	ref_is_base, row_is_base = M.seam_masks(sg, row)
	return split_classes(ref_is_base, row_is_base, sg.ref_row, sg.aligned(row))


def seam_ops(sg, row):
	return ops_from_classes(seam_classes(sg, row)), int(M.seam_masks(sg, row)[1].sum())


# ---- the PAF format ----------------------------------------------------------------------------------------------------------------------

def paf_text(ops, t_name, t_size, q_name, q_size):
	"""One PAF line, the row as query and the reference as target, both on the + strand (PAF: twelve tab-separated columns, then tags):
	  qName qSize qStart qEnd + tName tSize tStart tEnd nMatch blockLen mapq NM:i:<n> cg:Z:<cigar>
	Starts are 0-based and ends exclusive.  The alignment is the ops from the first to the last = / X op: I / D ops outside it move the
	starts and ends inward.  nMatch is the number of matching bytes (the = lengths), blockLen the number of alignment columns (all lengths
	inside the alignment, gaps included), mapq 255 (not available), NM the edit distance = blockLen - nMatch, cg the extended CIGAR.  b""
	when there is no = / X op."""
	ops = [(int(o), int(n)) for o, n in np.asarray(ops, dtype=np.uint64).reshape(-1, 2).tolist()]
	for o, _ in ops:
		if o not in (OP_I, OP_D, OP_EQ, OP_X):
			raise ValueError("op code %d" % o)
	at = [i for i, (o, _) in enumerate(ops) if o in (OP_EQ, OP_X)]
	if not at:
		return b""
	first, last = at[0], at[-1]
	q_start = sum(n for o, n in ops[:first] if o == OP_I)
	t_start = sum(n for o, n in ops[:first] if o == OP_D)
	q_end = q_size - sum(n for o, n in ops[last + 1:] if o == OP_I)
	t_end = t_size - sum(n for o, n in ops[last + 1:] if o == OP_D)
	inside = ops[first:last + 1]
	n_eq = sum(n for o, n in inside if o == OP_EQ)
	block_len = sum(n for _, n in inside)
	cigar = "".join("%d%s" % (n, {OP_EQ: "=", OP_X: "X", OP_I: "I", OP_D: "D"}[o]) for o, n in inside)
	assert q_end - q_start == sum(n for o, n in inside if o != OP_D) and t_end - t_start == sum(n for o, n in inside if o != OP_I)
	fields = [q_name, q_size, q_start, q_end, "+", t_name, t_size, t_start, t_end, n_eq, block_len, 255, "NM:i:%d" % (block_len - n_eq), "cg:Z:" + cigar]
	return ("\t".join(str(f) for f in fields) + "\n").encode()


def haplotype_paf(g, chromosome_id=None):
	"""The model's PAF file for --haplotypes: one line per chromosome copy, in the A2M output's order, named as one file per sequence is."""
	prefix = (chromosome_id + ".") if chromosome_id else ""
	out = []
	for s, sample in enumerate(g.sample_names):
		for c in range(int(g.ploidy_csum[s + 1]) - int(g.ploidy_csum[s])):
			ops, length = model_ops(g, int(g.ploidy_csum[s]) + c)
			out.append(paf_text(ops, prefix + "REF", len(g.ref), "%s%s.%d" % (prefix, sample, 1 + c), length))
	return b"".join(out)


def founder_paf(g, cut_positions, assigned_column_major, chromosome_id=None):
	prefix = (chromosome_id + ".") if chromosome_id else ""
	n_rows = len(cut_positions) - 1
	out = []
	for col in range(len(assigned_column_major) // n_rows if n_rows else 0):
		cuts = list(zip(cut_positions[:-1], assigned_column_major[col * n_rows:(col + 1) * n_rows]))
		ops, length = model_ops(g, cuts)
		out.append(paf_text(ops, prefix + "REF", len(g.ref), "%s%d" % (prefix, 1 + col), length))
	return b"".join(out)


# ---- graphs with chosen bytes ------------------------------------------------------------------------------------------------------------

_OTHER = {ord("A"): ord("c"), ord("C"): ord("g"), ord("G"): ord("t"), ord("T"): ord("a")}


def retouch(sg, name, plan=None, ref_at=None, label_at=None):
	"""The graph of a Builder with bytes of its labels (and of its reference) set, every array else the same.
	  plan       {edge: pattern}: label byte i of the edge, which must lie over a reference byte, becomes that byte in lower case ('=': equal
	             by case folding) or another letter ('X'); '.' leaves the byte as drawn;
	  ref_at     {column: byte}, label_at {(edge, i): byte}: literal bytes."""
	ref_row, labels = sg.ref_row.copy(), sg.label_bytes.copy()
	for col, byte in (ref_at or {}).items():
		assert sg.kept[col]
		ref_row[col] = byte
	for e, pattern in (plan or {}).items():
		assert len(pattern) <= sg.label_len[e]
		for i, what in enumerate(pattern):
			col = int(sg.begin[e]) + i
			if "." == what:
				continue
			assert sg.kept[col], "label byte %d of edge %d lies over padding" % (i, e)
			under = int(ref_row[col])
			labels[int(sg.label_offsets[e]) + i] = {"=": under | 0x20, "X": _OTHER[under]}[what]
	for (e, i), byte in (label_at or {}).items():
		assert i < sg.label_len[e]
		labels[int(sg.label_offsets[e]) + i] = byte
	ref = ref_row[sg.kept]
	g0 = sg.g
	g = oracle.graph_from_arrays(g0.reference_positions, g0.aligned_positions, g0.alt_edge_targets, g0.alt_edge_count_csum, g0.label_offsets, labels.tobytes(),
		g0.paths_by_chrom_copy_and_edge, g0.path_rows, g0.path_cols, ["S"], [0, len(sg.copies)])
	g.ref = ref.tobytes()
	out = sgs.SeamGraph(name, g, sg.kept, ref, sg.begin, sg.end, sg.label_offsets, sg.label_len, labels, sg.src, sg.tgt, sg.copies)
	out.notes = dict(sg.notes)
	return out


def _substitution(b, n=1):
	"""A site whose label replaces its n reference bytes one for one."""
	return b.add_site([n], n, n)[0]


@functools.lru_cache(maxsize=None)
def boundary_graph():
	"""One-byte X ops and X runs at the tile's, the slot's and the chunk's edges.  Every label differs from the reference bytes under it at
	every byte; copy 0 takes every edge, copy 1 none, copies 2 and 3 every other one."""
	K = sgs.kernel_constants()
	T, S = K.kTileBytes, K.kTileBytes // K.kSlots
	b = sgs.Builder(9501)
	e = []
	b.ref_to(S)
	e.append(_substitution(b))                       # a one-byte X on a 1-KiB slot edge
	b.ref_to(2 * S + 160)
	e.append(_substitution(b))                       # ... on a 16-byte chunk edge
	b.ref_to(3 * S - 2)
	e.append(_substitution(b, 5))                    # an X run across a slot edge
	b.ref_to(4 * S + 16 * 5 - 2)
	e.append(_substitution(b, 4))                    # ... across a chunk edge
	b.ref_to(T)
	e.append(_substitution(b))                       # a one-byte X at a tile's column 0: '=' on the last column of tile 0, X on the first of tile 1
	b.ref_to(2 * T - 1)
	e.append(_substitution(b))                       # a one-byte X on a tile's last column
	b.ref_to(3 * T - 3)
	e.append(_substitution(b, 6))                    # an X run across a tile boundary: X | X
	b.add_ref(211)
	sg = b.finish([e, [], e[::2], e[1::2]], "eqx_boundary_drawn")
	return retouch(sg, "eqx_boundary", {ed: "X" * int(sg.label_len[ed]) for ed in e})


@functools.lru_cache(maxsize=None)
def skipped_graph(n_skipped):
	"""An insertion taken by copy 0 alone covers n_skipped whole tiles and more on either side; its site's one reference byte has a second,
	one-byte label (X), and the first column after the stretch is a substitution site (X).  Copy 1 takes both: X ... skipped ... X, one op.
	Copy 2 takes the second only: = ... skipped ... X, two ops.  Copy 3 takes the first only: X ... skipped ... =."""
	K = sgs.kernel_constants()
	T = K.kTileBytes
	b = sgs.Builder(9510 + n_skipped)
	b.ref_to(T - 300)
	span = 300 + n_skipped * T + 200
	ins, sub = b.add_site([span, 1], span)
	after = _substitution(b)
	b.add_ref(700)
	sg = b.finish([[ins], [sub, after], [after], [sub]], "eqx_skipped_drawn")
	return retouch(sg, "eqx_skipped_%d" % n_skipped, {sub: "X", after: "X"})


@functools.lru_cache(maxsize=None)
def indel_graph():
	"""X beside I and D."""
	b = sgs.Builder(9520)
	b.add_ref(7)
	x_i, = b.add_site([5], 5, 2)                     # = X I I I: X directly followed by I inside one edge
	b.add_ref(9)
	x_d, = b.add_site([2], 4, 4)                     # = X D D: X followed by D inside one edge
	b.add_ref(5)
	d, = b.add_site([0], 3, 3)                       # D D D ...
	d_x = _substitution(b)                           # ... X: D followed by X across two edges
	b.add_ref(6)
	i, = b.add_site([4], 4, 1)                       # = I I I ...
	i_x = _substitution(b)                           # ... X: I followed by X
	b.add_ref(30)
	sg = b.finish([[x_i, x_d, d, d_x, i, i_x], [], [x_i, d_x, i_x], [x_d, d, i]], "eqx_indel_drawn")
	return retouch(sg, "eqx_indel", {x_i: "=X", x_d: "=X", d_x: "X", i: "=", i_x: "X"})


DASH_PAIR = (ord("-"), ord("-"), True)          # placed by row_ops_model.dash_graph (copy 2): a seam graph's model reads '-' as padding
CASE_PAIRS = [            # (the REF row's byte, the row's byte, equal?)
	(ord("a"), ord("A"), True), (ord("A"), ord("a"), True), (ord("a"), ord("C"), False), (ord("n"), ord("N"), True), (ord("N"), ord("A"), False),
	(ord("@"), ord("`"), False), (ord("["), ord("{"), False), (0xC4, 0xE4, False), (ord("*"), ord("*"), True),
	(ord("z"), ord("Z"), True), (ord("`"), ord("@"), False), (ord("{"), ord("["), False), (0xE4, 0xC4, False), (ord("1"), 0x11, False),
]


@functools.lru_cache(maxsize=None)
def case_graph():
	"""The case rule byte by byte: one substitution site per pair of CASE_PAIRS, two reference bytes between them; copy 0 takes all."""
	b = sgs.Builder(9530)
	b.add_ref(3)
	e = []
	for _ in CASE_PAIRS:
		e.append(_substitution(b))
		b.add_ref(2)
	sg = b.finish([e, [], e[::2]], "eqx_case_drawn")
	ref_at = {int(sg.begin[ed]): pair[0] for ed, pair in zip(e, CASE_PAIRS)}
	label_at = {(ed, 0): pair[1] for ed, pair in zip(e, CASE_PAIRS)}
	out = retouch(sg, "eqx_case", ref_at=ref_at, label_at=label_at)
	out.notes["edges"] = e
	return out


@functools.lru_cache(maxsize=None)
def dense_graph():
	"""Tile 0: a one-column substitution site on every column; copy 0 takes every other one, with a byte that differs: = X = X ..., every column
	of the tile a breakpoint under the split (16 384: the count field's maximum) and, but for the row's first column, none without it."""
	K = sgs.kernel_constants()
	T = K.kTileBytes
	b = sgs.Builder(9540)
	first = b.add_sites(T, 1, 1, 1)
	b.add_ref(37)
	taken = list(range(first + 1, first + T, 2))
	sg = b.finish([taken, [], list(range(first, first + T, 3))], "eqx_dense_drawn")
	return retouch(sg, "eqx_dense", {ed: "X" for ed in taken})


@functools.lru_cache(maxsize=None)
def long_graph():
	"""A label longer than kLongPatch (the long-patch queue) that replaces its reference bytes one for one, with mismatches at its first byte,
	its last byte and one in the middle; it begins in tile 0 and ends in tile 1, so its last mismatch lies in an edge that enters its tile
	through the crossing list."""
	K = sgs.kernel_constants()
	T = K.kTileBytes
	n = K.kLongPatch + 100
	b = sgs.Builder(9550)
	b.ref_to(T - 50)
	e = _substitution(b, n)
	b.add_ref(400)
	sg = b.finish([[e], []], "eqx_long_drawn")
	pattern = ["="] * n
	pattern[0] = pattern[n // 2] = pattern[-1] = "X"
	out = retouch(sg, "eqx_long", {e: "".join(pattern)})
	out.notes["edge"] = e
	return out


def eqx_graphs():
	return [boundary_graph(), skipped_graph(1), skipped_graph(2), indel_graph(), case_graph(), dense_graph(), long_graph()]


def pair_name(ref_byte, row_byte, equal):
	return "pair_%02x_over_%02x_is_%s" % (row_byte, ref_byte, "eq" if equal else "X")


def reach_pairs(g, rows):
	"""The listed byte pairs the rows of an oracle graph place on M columns, with the model's verdict (the walk: literal '-' bytes are bytes)."""
	listed = {(p[0], p[1]) for p in CASE_PAIRS + [DASH_PAIR]}
	ref_row = np.frombuffer(M.column_walk(g)[0], np.uint8)
	out = set()
	for r in rows:
		row, ref_is_base, row_is_base = M.walk_row(g, r)
		row = np.frombuffer(row, np.uint8)
		cls = split_classes(ref_is_base, row_is_base, ref_row, row)
		for c in np.flatnonzero((cls == CLS_EQ) | (cls == CLS_X)).tolist():
			if (int(ref_row[c]), int(row[c])) in listed:
				out.add(pair_name(int(ref_row[c]), int(row[c]), cls[c] == CLS_EQ))
	return out


def reach(sg, rows=None):
	"""What the rows of an eqx graph place, recomputed from the model's split classes with the kernels' constants: a set of names."""
	K = sgs.kernel_constants()
	T, S = K.kTileBytes, K.kTileBytes // K.kSlots
	tables = sgs.TileTables(sg)
	listed = {(p[0], p[1]) for p in CASE_PAIRS}
	out = set()
	for row in (sg.rows if rows is None else rows):
		cls = np.zeros(tables.n_tiles * T, dtype=np.uint8)
		cls[:sg.length] = seam_classes(sg, row)
		unsplit = np.where(cls == CLS_X, CLS_EQ, cls)
		live = np.flatnonzero(cls)
		seq = cls[live]
		first = np.flatnonzero(np.r_[True, seq[1:] != seq[:-1]])          # per op: index into live of its first column
		last = np.r_[first[1:] - 1, seq.size - 1]
		eff = sg.effective(row)
		owner = lambda c: next((e for e in eff if sg.begin[e] <= c < sg.end[e]), None)
		for f, l in zip(first.tolist(), last.tolist()):
			if seq[f] != CLS_X:
				continue
			a, z = int(live[f]), int(live[l])
			if a == z:
				for name, hit in (("X1_at_tile_column_0", a % T == 0 and a > 0), ("X1_at_tile_last_column", a % T == T - 1),
						("X1_at_slot_edge", a % S == 0 and a % T != 0), ("X1_at_chunk_edge", a % 16 == 0 and a % S != 0)):
					if hit:
						out.add(name)
			elif z - a == l - f:                                          # a run without skipped columns inside
				inside = np.arange(a + 1, z + 1)
				for name, hit in (("X_run_across_tile_boundary", np.any(inside % T == 0)), ("X_run_across_slot_edge", np.any((inside % S == 0) & (inside % T != 0))),
						("X_run_across_chunk_edge", np.any((inside % 16 == 0) & (inside % S != 0)))):
					if hit:
						out.add(name)
		for t in range(1, tables.n_tiles):
			pair = (int(cls[t * T - 1]), int(cls[t * T]))
			if pair == (CLS_EQ, CLS_X):
				out.add("eq_then_X_at_tile_boundary")                     # equal classes without the split: the scan must keep the breakpoint
			if pair == (CLS_X, CLS_X):
				out.add("X_then_X_at_tile_boundary")                      # the scan must drop it
		empty = ~cls.reshape(tables.n_tiles, T).any(axis=1)
		t = 0
		while t < tables.n_tiles:
			if not empty[t]:
				t += 1
				continue
			u = t
			while u < tables.n_tiles and empty[u]:
				u += 1
			before, after = live[live < t * T], live[live >= u * T]
			if before.size and after.size:
				pair = (int(cls[before[-1]]), int(cls[after[0]]))
				if pair == (CLS_X, CLS_X):
					out.add("X_%d_skipped_tiles_X" % (u - t))
				if pair == (CLS_EQ, CLS_X):
					out.add("eq_%d_skipped_tiles_X" % (u - t))
			t = u
		for k in range(seq.size - 1):
			pair = (int(seq[k]), int(seq[k + 1]))
			if pair[0] == pair[1] or CLS_X not in pair or CLS_EQ in pair:
				continue
			same = owner(int(live[k])) == owner(int(live[k + 1]))
			name = {(CLS_X, CLS_I): "X_then_I_in_one_edge" if same else None, (CLS_X, CLS_D): "X_then_D", (CLS_D, CLS_X): None if same else "D_then_X_across_two_edges",
				(CLS_I, CLS_X): "I_then_X"}[pair]
			if name:
				out.add(name)
		for t in range(tables.n_tiles):
			tile, plain = cls[t * T:(t + 1) * T], unsplit[t * T:(t + 1) * T]
			tile, plain = tile[tile != 0], plain[plain != 0]
			if tile.size and np.count_nonzero(np.r_[True, tile[1:] != tile[:-1]]) == T and np.count_nonzero(plain[1:] != plain[:-1]) == 0:
				out.add("every_column_a_breakpoint_with_the_split_only")
		m = np.flatnonzero((cls[:sg.length] == CLS_EQ) | (cls[:sg.length] == CLS_X))
		ref_b, row_b = sg.ref_row[m], sg.aligned(row)[m]
		for c, rb, qb in zip(m.tolist(), ref_b.tolist(), row_b.tolist()):
			if (rb, qb) in listed:
				out.add(pair_name(rb, qb, cls[c] == CLS_EQ))
		for e in eff:
			b, n = int(sg.begin[e]), int(sg.label_len[e])
			if n > K.kLongPatch and np.all(sg.kept[b:b + n]):
				x = np.flatnonzero(cls[b:b + n] == CLS_X)
				if x.size >= 3 and x[0] == 0 and x[-1] == n - 1 and np.any(cls[b:b + n] == CLS_EQ):
					out.add("long_label_X_first_middle_last")
			for t in (t for t in range(tables.n_tiles) if e in tables.cross[t]):
				lo, hi = int(tables.base[t]), int(min(sg.end[e], tables.tile_end[t]))
				if np.any(cls[lo:hi] == CLS_X):
					out.add("X_in_edge_from_the_crossing_list")
	return out


# ---- the scan graphs -------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def scan_graph(which):
	"""The scan graphs of row_ops_model.py (0: scan_waves, 1 and 2: scan_block_0 and _1) with the bytes of their substitution sites chosen:
	every byte of the runs across the seams and of the one-byte sites either side of the skipped stretches differs from the reference
	(X), and the M columns of the dense tiles alternate between '=' and X."""
	sg = M.scan_graphs()[which]
	return retouch(sg, sg.name + "_eqx", sg.notes["eqx_plan"])


def scan_graphs():
	return [scan_graph(i) for i in range(len(M.scan_graphs()))]


def scan_reach(sg, rows=None):
	"""row_ops_model.scan_reach over the split classes."""
	T = sgs.kernel_constants().kTileBytes
	n_tiles = -(-sg.length // T)
	out = set()
	for row in (sg.rows if rows is None else rows):
		cls = np.zeros(n_tiles * T, dtype=np.uint8)
		cls[:sg.length] = seam_classes(sg, row)
		M.scan_reach_classes(cls, T, "_DI=___X", out)
		if len(seam_ops(sg, row)[0]) > 65535:
			out.add("row_with_more_than_65535_ops")
	return out


SCAN_REACHED_BY = {
	"scan_waves_eqx": {"wave_seam_merge_=", "wave_seam_merge_X", "wave_seam_merge_D", "wave_seam_break", "block_seam_merge_=", "block_seam_merge_X", "block_seam_merge_D",
		"block_seam_break", "skipped_wave_equal", "skipped_wave_different", "carried_D_through_skipped_wave", "carried_X_through_skipped_wave", "D_skipped_wave_M",
		"skipped_from_lane_0", "skipped_up_to_lane_63", "dense_tile_last_of_wave", "dense_tile_first_of_wave", "dense_tile_last_of_block", "dense_tile_first_of_block",
		"row_with_more_than_65535_ops", "empty_tile_count_at_wave_seam"},
	"scan_block_0_eqx": {"skipped_block_equal", "skipped_block_different", "carried_D_through_skipped_block", "carried_X_through_skipped_block", "D_skipped_block_M",
		"wave_seam_merge_I", "empty_tile_count_at_block_seam"},
	"scan_block_1_eqx": {"skipped_block_equal", "skipped_block_different", "skipped_block_into_later_wave", "carried_D_through_skipped_block",
		"carried_X_through_skipped_block", "D_skipped_block_M", "wave_seam_merge_I", "block_seam_merge_I", "empty_tile_count_at_block_seam", "empty_tile_count_at_wave_seam"},
}


REACHED_BY = {
	"eqx_boundary": {"X1_at_tile_column_0", "X1_at_tile_last_column", "X1_at_slot_edge", "X1_at_chunk_edge", "X_run_across_tile_boundary", "X_run_across_slot_edge",
		"X_run_across_chunk_edge", "eq_then_X_at_tile_boundary", "X_then_X_at_tile_boundary"},
	"eqx_skipped_1": {"X_1_skipped_tiles_X", "eq_1_skipped_tiles_X"},
	"eqx_skipped_2": {"X_2_skipped_tiles_X", "eq_2_skipped_tiles_X"},
	"eqx_indel": {"X_then_I_in_one_edge", "X_then_D", "D_then_X_across_two_edges", "I_then_X"},
	"eqx_case": {pair_name(*p) for p in CASE_PAIRS},
	"eqx_dense": {"every_column_a_breakpoint_with_the_split_only"},
	"eqx_long": {"long_label_X_first_middle_last", "X_in_edge_from_the_crossing_list"},
	"dashes": {pair_name(*DASH_PAIR)},          # row_ops_model.dash_graph, through reach_pairs
}
