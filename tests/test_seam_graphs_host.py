"""The census of tests/seam_graphs.py: model == oracle for every graph and row, and every seam value the graphs are meant to put in front
of the row kernels is recomputed from the arrays, with the kernels' own definitions, and asserted to be there.  No GPU.

This is what keeps tests/test_gpu_splice_seams.py honest: a passing GPU test proves something only because the census proves that the
input is what its docstring says.  Move one edge of a graph by a column and a census test fails."""

import numpy as np
import pytest

import row_ops_model as M
import seam_graphs as S

K = S.kernel_constants()
T = K.kTileBytes


def _graphs():
	out = [S.mask_graph(0), S.mask_graph(0, K.kTileChunks // 4), S.mask_graph(7), S.short_count_graph(), S.cache_graph()]
	out += [S.geometry_graph(n) for n in S.geometry_lengths()]
	out += [S.resolve_graph(t) for t in (0, 1, 63)]
	return out


def test_constants_are_read_from_the_kernels():
	assert set(S.CONSTANT_NAMES) | {"kQueue", "kTileChunks", "kSlots"} == set(K)
	assert all(isinstance(v, int) and v > 0 for v in K.values())
	assert K.kCandLds % 64 == 0 and K.kCandDeltaLds > K.kCandLds and K.kCountRowsMax > 2 * K.kGroupRowsLds + 1 and K.kLabelLds < 0xFFFF


def test_model_equals_oracle_for_every_graph_and_row():
	for sg in _graphs():
		assert sg.length == sg.g.aligned_length
		for row in sg.rows:
			aligned = sg.body(row)
			assert len(aligned) == sg.length
			assert aligned == sg.oracle_body(row), (sg.name, row)
			assert sg.body(row, unaligned=True) == sg.oracle_body(row, unaligned=True), (sg.name, row)
		for name, b, e in sg.notes.get("windows", []):
			assert 0 <= b < e <= sg.length, (sg.name, name)


# ---- a. every chunk mask -------------------------------------------------------------------------------------------------------------------

def _mask_censuses(sg, window=None):
	tt = S.TileTables(sg, window)
	return [S.RowCensus(sg, row, tt) for row in [S.PLOIDY_MAX] + list(range(15))]


def test_every_mask_at_every_phase_on_both_routes():
	"""Each of the 65 534 keep-masks with 1 ... 15 bytes reaches the pack at all 16 destination phases: through the workgroup's queue in the
	graph with seven full chunks after every mask (alone), packed in place in the two orders of the graph without them (together).  The empty
	and the full mask, which the pack never sees, occur at all 16 phases too."""
	packable = S.packable_masks()
	s7 = _mask_censuses(S.mask_graph(7))
	queued, dense = S.mask_phase_coverage(s7)
	assert not dense.any() and max(int(c.tile_short.max()) for c in s7) <= K.kQueue          # everything queued
	assert queued[packable].all() and not queued[~packable].any()
	s0 = _mask_censuses(S.mask_graph(0)) + _mask_censuses(S.mask_graph(0, K.kTileChunks // 4))
	queued0, dense0 = S.mask_phase_coverage(s0)
	assert dense0[packable].all() and not dense0[~packable].any()
	assert queued0.any() and min(int(c.n_fit.min()) for c in s0) >= 1 and max(int(c.n_fit.max()) for c in s0) == K.kSlots   # the first slots of a tile are queued; the last tile fits whole
	one_order = S.mask_phase_coverage(s0[:16])[1]
	assert not one_order[packable].all()                       # what the second order is for
	for censuses in (s7, s0):
		phases = {m: set() for m in (0, 0xFFFF)}
		for c in censuses:
			for m in phases:
				phases[m] |= set(c.phase[c.mask == m].tolist())
		assert all(p == set(range(16)) for p in phases.values())
	assert {int(c.phase[1]) for c in s7} == set(range(16))      # the rows begin at 16 different phases


def test_mask_windows():
	sg = S.mask_graph(0)
	by_name = {n: (b, e) for n, b, e in sg.notes["windows"]}
	b, e = by_name["16_not_tile"]
	assert 0 == b % 16 and b % T and 0 == (e - b) % 16
	b, e = by_name["odd"]
	assert 1 == b % 2 and 0 == (e - b) % T
	b, e = by_name["ends_mid_chunk"]
	assert 0 == b % T and (e - b) % 16
	for name, (b, e) in by_name.items():
		for g in (sg, S.mask_graph(7)):
			cs = _mask_censuses(g, (b, e))
			queued, dense = S.mask_phase_coverage(cs)
			assert queued.any() and (g is not sg or dense.any()), name
			assert len({c.length for c in cs}) == 1 and len({c.phase.tobytes() for c in cs}) == 1    # the copies' labels lie before every window: its rows are equal
		tt = S.TileTables(sg, (b, e))
		assert tt.n_cross.sum() == 0 and tt.n_range.sum() == 0


# ---- b. short chunks per row tile -----------------------------------------------------------------------------------------------------------

def test_short_chunk_counts_per_tile():
	sg = S.short_count_graph()
	tiles, plan = sg.notes["tiles"], sg.notes["plan"]
	tt = S.TileTables(sg)
	ref, deleted, plain = (S.RowCensus(sg, row, tt) for row in (S.PLOIDY_MAX, 0, 1))
	Q, C = K.kQueue, K.kTileChunks
	for name, t in tiles.items():
		assert int(ref.tile_short[t]) == len(plan[name]), name
		assert np.array_equal(np.flatnonzero(ref.short[t * C:(t + 1) * C]), np.sort(plan[name])), name
	assert {0, 1, 63, 64, 65, Q - 1, Q, Q + 1} <= set(ref.tile_short.tolist())
	assert ref.short[tiles["one_first"] * C] and ref.short[tiles["one_last"] * C + C - 1]
	assert ref.slot_short[tiles["either_side"]].tolist()[:3] == [1, 2, 1]
	assert ref.slot_short[tiles["64_slot_end"]].tolist()[:2] == [64, 0]
	# which slots fit the queue
	assert ref.n_fit[tiles["q"]] == K.kSlots and ref.n_fit[tiles["q_minus_1"]] == K.kSlots and ref.n_fit[tiles["q_over_all_slots"]] == K.kSlots
	assert ref.slot_short[tiles["q_over_all_slots"]].min() > 0 and ref.tile_short[tiles["q_over_all_slots"]] == Q
	j = Q // 64
	assert ref.n_fit[tiles["q_plus_1"]] == j and ref.slot_short[tiles["q_plus_1"]][j] == 1 and ref.slot_short[tiles["q_plus_1"]][j + 1:].sum() == 0
	per = Q // 4 - 2
	assert ref.n_fit[tiles["later_slots_dense"]] == Q // per < K.kSlots - 1 and ref.slot_short[tiles["later_slots_dense"]].min() == per
	assert ref.n_fit[tiles["q_last_chunks"]] == K.kSlots and ref.slot_short[tiles["q_last_chunks"]][-1] == 64
	# copy 0: a tile that is all padding (its bytes go where the next tile's go), a short chunk made by the deletion's label in the tile before
	t = tiles["deleted"]
	assert deleted.tile_bytes[t] == 0 and deleted.tile_offset[t] == deleted.tile_offset[t + 1] and ref.tile_bytes[t] > 0
	assert deleted.short[t * C - 1] and deleted.count[t * C - 1] == 1 and not ref.short[t * C - 1]
	assert tt.cross[t] == [0] and tt.cross[t + 1] == [0] and deleted.n_long[t] == 1
	assert np.array_equal(plain.count, ref.count)
	assert {int(x) & 15 for x in ref.tile_offset} != {0} and sg.length % T == 16 * 3 + 5
	# windows
	by_name = {n: (b, e) for n, b, e in sg.notes["windows"]}
	w = S.TileTables(sg, by_name["empty_in_copy_0"])
	assert S.RowCensus(sg, 0, w).length == 0 and S.RowCensus(sg, S.PLOIDY_MAX, w).length > 0
	assert sg.body(0, unaligned=True, window=by_name["empty_in_copy_0"]) == b""
	w = S.TileTables(sg, by_name["from_deleted_tile"])
	assert w.cross[0] == [0] and S.RowCensus(sg, 0, w).tile_bytes[0] == 48 - 32       # the window's first tile ends 48 columns into the next tile, the deletion 32
	w = S.TileTables(sg, by_name["counts_shifted"])
	assert {Q, Q + 1} <= set(S.RowCensus(sg, S.PLOIDY_MAX, w).tile_short.tolist())   # three chunks in: those tiles lose three short chunks to the tile before and gain the next tile's first three


# ---- c. the patch cache ----------------------------------------------------------------------------------------------------------------------

def test_patch_cache_limits():
	sg = S.cache_graph()
	tiles, edges = sg.notes["tiles"], sg.notes["edges"]
	tt = S.TileTables(sg)
	eff = {row: set(sg.effective(row)) for row in sg.rows}

	def rows_with(*es):
		return [r for r in sg.rows if all(e in eff[r] for e in es)]

	def taken_and_not(e):
		assert rows_with(e) and len(rows_with(e)) < len(sg.rows), e    # effective in some row and not in another

	# n_range at the cache's size, range_begin & 63, the edges around the range in the same effective-edge word
	for which, (n, bit) in enumerate(((K.kCandLds - 1, 0), (K.kCandLds, 1), (K.kCandLds + 1, 63))):
		before, first, n_made, after = edges["range_%d" % which]
		t = tiles["range_%d" % which]
		assert tt.n_range[t] == n == n_made and tt.range_begin[t] == first and first & 63 == bit and tt.n_cross[t] == 0
		assert before == first - 1 and after == first + n
		cached_end = first + min(n, K.kCandLds)
		for e in (first, first + K.kCandLds - 2, first + n - 1, before, after):
			taken_and_not(e)
		if bit:
			assert before >> 6 == first >> 6 and rows_with(before, first)             # the count kernel's first mask has something to cut
		assert cached_end & 63 and (cached_end - 1) >> 6 == cached_end >> 6           # ... and its second
		assert rows_with(cached_end - 1, cached_end) or rows_with(cached_end) and rows_with(cached_end - 1)
		if n > K.kCandLds:
			assert rows_with(first + K.kCandLds) and rows_with(first + K.kCandLds - 1, first + K.kCandLds)
	assert {int(tt.n_range[tiles["range_%d" % i]]) for i in range(3)} == {K.kCandLds - 1, K.kCandLds, K.kCandLds + 1}

	# n_cross + n_range at the count kernel's table size
	for which, total in enumerate((K.kCandDeltaLds - 1, K.kCandDeltaLds, K.kCandDeltaLds + 1)):
		first_cross, n_cross, first, n_range = edges["delta_%d" % which]
		t = tiles["delta_%d" % which]
		assert tt.n_cross[t] == n_cross > 0 and tt.n_range[t] == n_range > K.kCandLds and n_cross + n_range == total
		assert tt.cross[t] == list(range(first_cross, first_cross + n_cross)) and tt.range_begin[t] == first
		assert all(sg.begin[e] < tt.base[t] < sg.end[e] < tt.base[t + 1] for e in tt.cross[t])
		assert np.all(np.diff(sg.end[first_cross:first_cross + n_cross]) < 0)         # nested
		for e in (first_cross, first_cross + n_cross - 1, first + n_range - 1, first + n_range - 2):
			taken_and_not(e)
		assert rows_with(first_cross + 1) and not rows_with(first_cross + 2)          # set with its blocker: never effective

	# the label slice
	for which, end_at in enumerate((K.kLabelLds - 1, K.kLabelLds, K.kLabelLds + 1)):
		e0, e1, e2, e3 = edges["label_%d" % which]
		t = tiles["label_%d" % which]
		assert tt.range_begin[t] == e0 and tt.n_range[t] == 4
		ends = tt.label_end_in_slice(sg, t).tolist()
		assert ends[1] == end_at and ends[2] == end_at and sg.label_len[e2] == 0 and ends[3] == end_at + 3 and ends[0] == end_at - 10
		for e in (e0, e1, e2, e3):
			taken_and_not(e)

	# spans at the cached form's limit
	for which, span in enumerate((0xFFFE, 0xFFFF, 0x10000)):
		e0, e1 = edges["span_%d" % which]
		t = tiles["span_%d" % which]
		assert sg.end[e0] - sg.begin[e0] == span and tt.tile_of(sg.begin[e0]) == t and tt.range_begin[t] == e0
		assert sum(e0 in c for c in tt.cross) >= 3                                     # it crosses into at least three more tiles
		taken_and_not(e0)
		taken_and_not(e1)

	# patch lengths around kLongPatch, whole and clipped
	p0, p1, p2, p3 = edges["long_patch"]
	t = tiles["long_patch"]
	assert [tt.clipped(sg, p0, t), tt.clipped(sg, p1, t), tt.clipped(sg, p2, t)] == [K.kLongPatch, K.kLongPatch + 1, K.kLongPatch]
	assert tt.clipped(sg, p2, t + 1) == K.kLongPatch and tt.cross[t + 1] == [p2] and sg.label_len[p2] > K.kLongPatch   # the label goes on in the next tile
	t = tiles["long_patch_clipped"]
	assert tt.clipped(sg, p3, t) == K.kLongPatch + 1 and tt.cross[t + 1] == [p3] and tt.clipped(sg, p3, t + 1) == K.kLongPatch
	for e in (p0, p1, p2, p3):
		taken_and_not(e)

	# the long-patch queue
	first, n = edges["long_queue"]
	t = tiles["long_queue"]
	per_row = {row: int(S.RowCensus(sg, row, tt).n_long[t]) for row in sg.rows}
	assert sorted(set(per_row.values())) == [0, K.kLongQueueLds - 1, K.kLongQueueLds, K.kLongQueueLds + 1]
	rows = S.cache_rows(2 * len(sg.rows))
	seq = [per_row[r] for r in rows]
	assert any(seq[i:i + 4] == [0, K.kLongQueueLds - 1, K.kLongQueueLds, K.kLongQueueLds + 1] for i in range(len(seq)))   # in consecutive rows

	# tile edges
	q0, q1, q2 = edges["tile_edges"]
	t = tiles["last_column"]
	assert sg.begin[q0] == tt.base[t + 1] - 1 and tt.cross[t + 1] == [q0] and sg.label_len[q0] > 1
	t = tiles["ends_on_boundary"]
	assert sg.end[q1] == tt.base[t + 1] == tiles["after_boundary"] * T and tt.cross[t + 1] == [] and tt.tile_of(sg.begin[q1]) == t
	for e in (q0, q1, q2):
		taken_and_not(e)

	# windows that begin inside, at and one column after each of these tiles
	names = {n for n, _, _ in sg.notes["windows"]}
	for name, t in tiles.items():
		if name.startswith(("range_", "delta_", "label_", "span_", "long_", "last_column", "ends_on_boundary")):
			assert {name + "_inside", name + "_at", name + "_after"} <= names
	for name, b, e in sg.notes["windows"]:
		w = S.TileTables(sg, (b, e))
		t = b // T
		if name.endswith("_at"):
			assert w.n_range[0] == tt.n_range[t] and w.cross[0] == tt.cross[t] and w.range_begin[0] == tt.range_begin[t]
		else:
			assert w.cross[0] == np.flatnonzero((sg.begin < b) & (sg.end > b)).tolist()


def test_cache_rows_per_group():
	assert S.cache_rows(5)[:4] == [S.PLOIDY_MAX, 9, 10, 11]
	assert set(S.cache_rows(13)) == set(S.cache_graph().rows)


# ---- d. tile geometry -----------------------------------------------------------------------------------------------------------------------

def test_geometry_lengths():
	lengths = S.geometry_lengths()
	assert {n - n // T * T for n in lengths if n < 6 * T} == {T - 1, 0, 1, 15, 16, 17}
	counts = sorted({(n + T - 1) // T for n in lengths if n > 6 * T})
	assert counts == [63, 64, 65, 71, 72]
	assert [c % 64 % 8 for c in counts] == [7, 0, 1, 7, 0]        # the last run of tiles: a multiple of 8 (remapped by the unaligned kernels) or not
	for n in lengths:
		sg = S.geometry_graph(n)
		assert sg.length == n and sg.n_edges >= 3
		tt = S.TileTables(sg)
		assert tt.n_tiles == (n + T - 1) // T
		if tt.n_tiles > 6:
			assert tt.n_cross.sum() >= 2               # deletions across tile boundaries
		assert sg.effective(0) and sg.effective(1)


# ---- e. resolve ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tail", [0, 1, 63])
def test_resolve_graph(tail):
	sg = S.resolve_graph(tail)
	assert sg.n_edges % 64 == tail
	reach = np.r_[0, np.maximum.accumulate(sg.tgt)][:-1]          # the furthest target of the edges before
	overlappable = sg.src < reach
	piece = 256 * K.kResolveWordsPerThread
	words = set()
	for p, q in sg.notes["pairs"]:
		assert overlappable[q] and not overlappable[p] and sg.tgt[p] > sg.src[q] and p < q
		assert q in sg.copies[0] and p in sg.copies[0] and q not in sg.effective(0) and q in sg.effective(1)
		words.add(((p & 63, p >> 6), (q & 63, q >> 6)))
	for k in (1, K.kResolveWordsPerThread, 256, piece):
		assert ((63, k - 1), (0, k)) in words
	assert sum(1 for (pb, pw), (qb, qw) in words if pw == qw and pb == 0 and qb == 63) == 2
	# the deletion's restart distance
	d, under, bw = sg.notes["deletion"], sg.notes["under"], sg.notes["back_words"]
	assert d & 63 == 0 and not overlappable[d] and bw == S.RESOLVE_BACK_WORDS < K.kMaxBackWords
	for i, u in enumerate(under):
		restart = int(np.flatnonzero(~overlappable[:u + 1])[-1])
		assert restart == d and (u >> 6) - (restart >> 6) == bw + i
		assert not (~overlappable[(u >> 6) * 64:u]).any()            # nothing in its own word ends the search
	assert under[0] not in sg.effective(0) and under[0] in sg.effective(1) and under[1] not in sg.effective(2) and under[1] in sg.effective(1)


# ---- f. founder rows: the segment table in front of assemble_row_bits_kernel -----------------------------------------------------------------

TAILS = (0, 1, 63)
R = S.PLOIDY_MAX


def _row_bits(sg, copy):
	return np.zeros(sg.n_edges, dtype=bool) if copy == R else sg.copy_bits(copy)


def _all_assemble_rows(tail):
	"""(name, row, word_base, n_words) of every row of the assemble graph: whole rows and rows under the windows."""
	sg = S.assemble_graph(tail)
	out = [(name, row, 0, None) for name, row in S.assemble_rows(tail).items()]
	for wname, b, e, rows in S.assemble_windows(tail):
		_, lo, hi = S.window_words(sg, b, e)
		out += [(wname + "/" + name, row, lo, hi) for name, row in rows.items() if hi]
	return out


@pytest.mark.parametrize("tail", TAILS)
def test_assemble_graph_shows_every_bit(tail):
	sg = S.assemble_graph(tail)
	n = sg.n_edges
	assert n == 64 * (256 + 64 + 3) + tail and n % 64 == tail
	assert np.all(sg.end - sg.begin == 1) and np.all(sg.label_len == 1) and np.all(sg.tgt - sg.src == 1)
	assert np.all(sg.end[:-1] <= sg.begin[1:])                                        # no edge overlaps another: effective == assembled
	assert np.all(sg.label_bytes != sg.ref_row[sg.begin])                             # a taken edge is seen in its column
	assert all(sg.is_bridge(v) for v in range(int(sg.tgt[-1]) + 1))
	for g in S.ASSEMBLE_GAPS:                                                         # two nodes, one first edge
		node = int(sg.src[g])
		assert sg.tgt[g - 1] == node - 1 and sg.first_edge_of_node(node - 1) == sg.first_edge_of_node(node) == g
	assert sg.first_edge_of_node(int(sg.tgt[-1])) == n and int(sg.tgt[-1]) < sg.g.node_count - 1   # a node past every edge that is not the last one
	for a, b in S.ASSEMBLE_PAIRS:
		assert np.all(sg.copy_bits(a) != sg.copy_bits(b))
	assert sg.copy_bits(0).all()                                                      # a REF segment read as copy 0 would set every bit of it
	row = S.assemble_rows(tail)["c_65_45"]
	assert sg.effective(row) == np.flatnonzero(sg.assembled(row)).tolist()
	assert np.array_equal(np.frombuffer(sg.body(row), np.uint8)[sg.begin] != sg.ref_row[sg.begin], sg.assembled(row))


@pytest.mark.parametrize("tail", TAILS)
def test_cut_rows_model_equals_oracle(tail):
	sg = S.assemble_graph(tail)
	windows = S.assemble_windows(tail)
	rows = list(S.assemble_rows(tail).items()) + [item for w in windows for item in w[3].items()]
	for name, row in rows:
		assert sg.body(row) == sg.oracle_body(row), name
		assert sg.body(row, unaligned=True) == sg.oracle_body(row, unaligned=True), name
	for wname, b, e, wrows in windows:
		assert 0 <= b < e <= sg.length
		for name, row in wrows.items():
			assert sg.body(row, True, (b, e)) == sg.oracle_body(row, True, (b, e)), (wname, name)
	rg = S.resolve_graph(tail)
	for name, row in S.resolve_cut_rows(tail).items():
		assert rg.body(row) == rg.oracle_body(row), name
		assert rg.body(row, unaligned=True) == rg.oracle_body(row, unaligned=True), name
	# the twin with empty labels, for the alignment ops: the same nodes, edges and copies, and a D of one byte per set bit
	dg = S.assemble_graph(tail, 0)
	assert np.array_equal(dg.src, sg.src) and np.array_equal(dg.tgt, sg.tgt) and not dg.label_len.any()
	assert all(np.array_equal(dg.copies[c], sg.copies[c]) for c in range(len(sg.copies)))
	for name, row in S.assemble_rows(tail).items():
		if name[0] in "acdf":
			assert dg.body(row) == dg.oracle_body(row) and dg.body(row, unaligned=True) == dg.oracle_body(row, unaligned=True), name
			ops, length = M.seam_ops(dg, row)
			deleted = np.zeros(dg.length, dtype=bool)
			deleted[dg.begin[dg.assembled(row)]] = True
			assert dg.kept.all() and np.array_equal(np.repeat(ops[:, 0], ops[:, 1]) == M.OP_D, deleted) and length == dg.length - deleted.sum(), name
			assert len(M.seam_ops(sg, row)[0]) == 1


@pytest.mark.parametrize("tail", TAILS)
def test_every_cut_is_visible(tail):
	"""At every change of copy the two copies differ at the last edge before the cut and at the first edge after it (REF counts as no bit
	set, so the copy beside it has both bits set): a mask one bit short or long changes a column.  An empty segment's copy differs at
	that edge from the copy that holds from there."""
	sg = S.assemble_graph(tail)
	for name, row, base, n_words in _all_assemble_rows(tail):
		c = S.SegmentCensus(sg, row, base, n_words)
		assert len(c.seg_copy) >= 2, name
		for edge, before, after in c.neighbours():
			assert edge >= 1 and before != after, (name, edge)
			for e in (edge - 1, edge):
				assert e >= sg.n_edges or _row_bits(sg, before)[e] != _row_bits(sg, after)[e], (name, edge, e)
		for s in c.empty:
			edge = int(c.seg_begin[s])
			holder = next(t for t in range(s + 1, len(c.seg_copy)) if t not in c.empty)
			assert c.seg_begin[holder] == edge and _row_bits(sg, c.seg_copy[s])[edge] != _row_bits(sg, c.seg_copy[holder])[edge], (name, s)
			assert sg.assembled(row)[edge] == _row_bits(sg, c.seg_copy[holder])[edge]


def _segments(c):
	"""(first edge, end edge or None, copy) of the census' segments."""
	ends = c.seg_begin[1:].tolist() + [None]
	return list(zip(c.seg_begin.tolist(), ends, c.seg_copy))


@pytest.mark.parametrize("tail", TAILS)
def test_segment_census_whole_rows(tail):
	sg = S.assemble_graph(tail)
	n = sg.n_edges
	rows = S.assemble_rows(tail)
	census = {name: S.SegmentCensus(sg, row) for name, row in rows.items()}
	assert {name[0] for name in rows} == set("abcdef")
	span_firsts = list(range(0, (n + 63) // 64, 64))
	for c in census.values():
		assert [s[0] for s in c.spans] == span_firsts and len(span_firsts) == 6 and c.n_words - span_firsts[-1] in (3, 4)

	# a. one-bit segments at bit 63 and at bit 0, from in {0, 1, 63} x to in {1, 63, 64}, at the words beside every span and workgroup edge
	for name in ("a_word_edges_01", "a_word_edges_23", "a_word_edges_45"):
		c = census[name]
		by_word = {}
		for (s, w), ft in c.mask_at.items():
			by_word.setdefault(w, set()).add(ft)
		for k in (1, 63, 64, 65, 255, 256, 257):
			assert by_word[k - 1] >= {(63, 64)} and by_word[k] >= {(0, 1), (1, 63), (63, 64)}, (name, k)
		assert c.masks >= {(0, 1), (1, 63), (63, 64), (0, 63), (0, 64)}
		assert {f for f, _ in c.masks} == {0, 1, 63} and {t for _, t in c.masks} == {1, 63, 64}
		assert c.writers.max() == 3 and not c.empty and not c.ref

	# b. a segment of one word, of one wave span, of 65 words across a span edge, across the workgroup edge; a segment longer than a workgroup
	segs = _segments(census["b_word_span_65"])
	assert (64 * 20, 64 * 21, 5) in segs
	assert any(b % (64 * 64) == 0 and e == b + 64 * 64 for b, e, _ in segs if e)
	assert any(e and e - b == 64 * 65 and b % 64 == 0 and b // (64 * 64) != (e - 1) // (64 * 64) for b, e, _ in segs)
	assert any(e and b % 64 and e % 64 and b < 64 * 256 < e for b, e, _ in _segments(census["b_across_workgroups"]))
	for name in ("b_two_long_01", "b_two_long_45"):
		(b0, e0, _), (b1, e1, _) = _segments(census[name])
		assert b0 == 0 and e0 == b1 > 64 * 256 and b1 % 64 and e1 is None            # every wave of the first workgroup sees one segment
		assert [s[2] for s in census[name].spans] == [1, 1, 1, 1, 2, 1]

	# c. 64, 65, 66, 129, 130 segments for one wave's lane loop; 64 writers into one word, the run going on in the next word
	for name, span, walked, rounds in (("c_63", 0, 64, 1), ("c_64", 0, 65, 2), ("c_65_01", 1, 66, 2), ("c_65_45", 1, 66, 2), ("c_128", 2, 129, 3), ("c_129", 3, 130, 3)):
		c = census[name]
		assert c.spans[span][2:] == (walked, rounds), (name, c.spans)
		assert all(s[3] == 1 for i, s in enumerate(c.spans) if i != span)
	assert census["c_64"].writers.max() == 64
	for name in ("c_65_01", "c_65_45"):
		c = census[name]
		w = int(np.argmax(c.writers))
		assert c.writers[w] == 64 and c.writers[w + 1] >= 1 and {64 * w + 63, 64 * w + 64} <= set(c.seg_begin.tolist())
	assert {64 * 201 - 1, 64 * 201, 64 * 202 - 1, 64 * 202} <= set(census["c_129"].seg_begin.tolist())

	# d. REF: before the first cut, one bit, one word, up to a wave span's first edge, the last segment
	c = census["d_ref"]
	segs = _segments(c)
	ref = [(b, e) for b, e, copy in segs if copy == R]
	assert ref[0][0] == 0 and ref[0][1] % 64 and c.ref[0] == 0 and rows["d_ref"][0][0] != 0
	assert any(e == b + 1 for b, e in ref[1:-1]) and any(b % 64 == 0 and e == b + 64 for b, e in ref[1:-1])
	assert any(b % 64 and e % (64 * 64) == 0 for b, e in ref[1:-1]) and ref[-1][1] is None and len(ref) == 5
	c = census["d_first_cut_late"]
	assert c.ref == [0] and len(c.seg_copy) == 2 and c.seg_begin[1] % 64

	# e. a last segment of the one last edge, and one that begins past every edge
	for name in ("e_last_edge_45", "e_last_edge_01", "e_last_edge_10"):
		assert census[name].seg_begin[-1] == n - 1
	for name in ("e_past_every_edge_45", "e_past_every_edge_10", "e_past_every_edge_01"):
		assert census[name].seg_begin[-1] == n and not census[name].empty
	assert ((n - 1) & 63, 64) in census["e_last_edge_45"].masks               # the last segment's end is the end of the words, not of the edges

	# f. empty segments at an ordinary edge, at a wave span's first edge, at a workgroup's
	for name in ("f_empty_45", "f_empty_10"):
		c = census[name]
		at = [int(c.seg_begin[s]) for s in c.empty]
		assert at == list(S.ASSEMBLE_GAPS) and at[0] % 64 and at[1] % (64 * 64) == 0 and at[1] % (64 * 256) and at[2] % (64 * 256) == 0
		assert c.spans[1][:2] == (64, 2) and c.spans[4][:2] == (256, 2) and c.spans[0][1] == 1


@pytest.mark.parametrize("tail", TAILS)
def test_segment_census_under_windows(tail):
	"""The windows' first edge words, and the cuts against the wave spans as the windows shift them."""
	sg = S.assemble_graph(tail)
	windows = S.assemble_windows(tail)
	assert [S.window_words(sg, b, e)[1] for _, b, e, _ in windows[:-1]] == list(S.ASSEMBLE_WINDOW_WORDS)
	for (wname, b, e, rows), k in zip(windows, S.ASSEMBLE_WINDOW_WORDS):
		restart, lo, hi = S.window_words(sg, b, e)
		assert restart == lo == k and hi == min(k + 131, (sg.n_edges + 63) // 64), wname
		for name, row in rows.items():
			c = S.SegmentCensus(sg, row, lo, hi)
			assert [s[0] for s in c.spans][:2] == [k, k + 64] and k % 64 or k == 64
			begins = set(c.seg_begin.tolist())
			for first in (64 * k, 64 * (k + 64)):
				assert {first - 1, first, first + 1} <= begins
			assert c.spans[0][1] == 1 and c.spans[1][1:] == (1, 67, 2), (wname, name, c.spans)
			assert any(0 < x < 64 * k for x in begins)                              # a cut before the window's words
	wname, b, e, rows = windows[-1]
	assert S.window_words(sg, b, e) == (0, 0, 0) and b >= sg.end[-1] and len(rows) == 2


@pytest.mark.parametrize("tail", TAILS)
def test_resolve_cut_rows(tail):
	"""Resolve on assembled rows: which copy's bits lie between the cuts and outside them, and what that makes effective."""
	sg = S.resolve_graph(tail)
	rows = S.resolve_cut_rows(tail)
	d, under = sg.notes["deletion"], sg.notes["under"]
	eff = {name: set(sg.effective(row)) for name, row in rows.items()}
	bits = {name: sg.assembled(row) for name, row in rows.items()}
	for p, q in sg.notes["pairs"]:
		for name, row in rows.items():
			cuts = [node for node, _ in row]
			assert int(sg.src[p]) in cuts and int(sg.tgt[q]) in cuts
		assert sg.copy_bits(0)[p] and sg.copy_bits(0)[q] and not sg.copy_bits(2)[p] and not sg.copy_bits(2)[q]
		for e in (p - 1, p, q, q + 1):                  # blocker and blocked edge from the one copy, the edges either side from the other
			assert bits["both_inside"][e] == sg.copy_bits(0 if e in (p, q) else 2)[e] and bits["both_outside"][e] == sg.copy_bits(2 if e in (p, q) else 0)[e]
		assert p in eff["both_inside"] and q not in eff["both_inside"] and not bits["both_outside"][p] and not bits["both_outside"][q]
		assert q in eff["blocked_alone_inside"] and not bits["blocked_alone_inside"][p] and sg.copy_bits(0)[p]     # the first segment's copy would block it
		assert p in eff["blocked_alone_outside"] and q not in eff["blocked_alone_outside"] and bits["blocked_alone_outside"][q]
		assert p in eff["blockers_inside"] and not bits["blockers_inside"][q]
	# under the deletion: the row's word and the first segment's copy disagree about the deletion, so a walk back that reads the copy decides wrongly
	assert not bits["blocked_alone_inside"][d] and sg.copy_bits(0)[d] and {under[0], under[1]} <= eff["blocked_alone_inside"]
	assert bits["blocked_alone_outside"][d] and not sg.copy_bits(1)[d] and bits["blocked_alone_outside"][under[0]] and under[0] not in eff["blocked_alone_outside"]
	assert bits["both_outside"][d] and bits["both_outside"][under[1]] and under[1] not in eff["both_outside"]       # bw + 1 words back: the serial kernel's
	inside = bits["sevenths_inside"][d:d + 64 * 4]                            # nine overlappable edges a word and no deletion: words decided by a walk back that blocks nothing
	assert not inside[0] and inside.reshape(4, 64)[:3].sum(axis=1).min() >= 9 and set(np.flatnonzero(inside) + d) <= eff["sevenths_inside"]
	for name, row in rows.items():
		c = S.SegmentCensus(sg, row)
		assert len(c.seg_copy) == 2 * (len(sg.notes["pairs"]) + 1) + 1 and not c.empty and not c.ref, name
	(_, b0, e0), (_, b1, e1) = S.resolve_cut_windows(tail)
	restart, lo, hi = S.window_words(sg, b0, e0)
	assert restart == lo == d >> 6 and hi > under[1] >> 6
	restart, lo, hi = S.window_words(sg, b1, e1)
	assert restart == lo - 1 == K.kResolveWordsPerThread - 1 and hi > under[1] >> 6      # a word is assembled that is not resolved
