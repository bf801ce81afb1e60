"""The model of the split row alignment ops (tests/row_ops_eqx_model.py): what its graphs place, its fold against the unsplit model, its X columns
against the recorded A2M rows, and the host library's PAF formatter against the model's.  No GPU."""

import glob
import os
import re

import numpy as np
import pytest

import oracle
import row_ops_eqx_model as E
import row_ops_model as M
import seam_graphs as sgs

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")
DERIVED = os.path.join(HERE, "golden", "derived")
PLOIDY_MAX = M.PLOIDY_MAX
DASH_ROWS = [PLOIDY_MAX, 0, 1, 2, 3, 4, [(0, 0), (2, 2)]]

# the situations of the issue's list, by the names reach() gives them
WANTED = {
	"X1_at_tile_column_0", "X1_at_tile_last_column", "X1_at_slot_edge", "X1_at_chunk_edge",
	"X_run_across_tile_boundary", "X_run_across_slot_edge", "X_run_across_chunk_edge",
	"eq_then_X_at_tile_boundary", "X_then_X_at_tile_boundary",
	"X_1_skipped_tiles_X", "eq_1_skipped_tiles_X", "X_2_skipped_tiles_X", "eq_2_skipped_tiles_X",
	"X_then_I_in_one_edge", "X_then_D", "D_then_X_across_two_edges", "I_then_X",
	"every_column_a_breakpoint_with_the_split_only",
	"long_label_X_first_middle_last", "X_in_edge_from_the_crossing_list",
} | {E.pair_name(*p) for p in E.CASE_PAIRS + [E.DASH_PAIR]}


def test_the_eqx_graphs_place_what_they_are_meant_to():
	K = sgs.kernel_constants()
	union = set()
	for sg in E.eqx_graphs():
		got = E.reach(sg)
		assert E.REACHED_BY[sg.name] <= got, (sg.name, sorted(E.REACHED_BY[sg.name] - got))
		union |= E.REACHED_BY[sg.name]
		assert 1 <= -(-sg.length // K.kTileBytes) <= 4
	got = E.reach_pairs(M.dash_graph(), DASH_ROWS)
	assert E.REACHED_BY["dashes"] <= got
	union |= E.REACHED_BY["dashes"]
	assert WANTED <= union, sorted(WANTED - union)
	# the verdicts the contract spells out, whatever the model says
	stated = {(ord("a"), ord("A")): True, (ord("a"), ord("C")): False, (ord("n"), ord("N")): True, (ord("@"), ord("`")): False, (ord("["), ord("{")): False,
		(0xC4, 0xE4): False, (ord("-"), ord("-")): True, (ord("*"), ord("*")): True, (ord("N"), ord("A")): False}
	table = {(p[0], p[1]): p[2] for p in E.CASE_PAIRS + [E.DASH_PAIR]}
	assert all(table[k] == v for k, v in stated.items())


def test_what_the_graphs_mean_in_ops():
	K = sgs.kernel_constants()
	T = K.kTileBytes
	dense = E.dense_graph()
	split, plain = E.seam_ops(dense, 0)[0], M.seam_ops(dense, 0)[0]
	assert len(split) == T + 1 and split[:T, 1].max() == 1 and plain.tolist() == [[M.OP_M, T + 37]]
	assert split[:4, 0].tolist() == [E.OP_EQ, E.OP_X, E.OP_EQ, E.OP_X]
	for n in (1, 2):
		sg = E.skipped_graph(n)
		assert [op for op, _ in E.seam_ops(sg, 1)[0].tolist()] == [E.OP_EQ, E.OP_X, E.OP_EQ] and E.seam_ops(sg, 1)[0][1, 1] == 2       # X ... skipped ... X: one op
		assert [op for op, _ in E.seam_ops(sg, 2)[0].tolist()] == [E.OP_EQ, E.OP_X, E.OP_EQ] and E.seam_ops(sg, 2)[0][1, 1] == 1       # = ... skipped ... X: two
		assert [op for op, _ in E.seam_ops(sg, 3)[0].tolist()] == [E.OP_EQ, E.OP_X, E.OP_EQ]
	boundary = E.boundary_graph()
	assert E.seam_ops(boundary, 0)[0][:, 0].tolist() == [E.OP_EQ, E.OP_X] * 7 + [E.OP_EQ]
	assert E.seam_ops(boundary, 0)[0][1::2, 1].tolist() == [1, 1, 5, 4, 1, 1, 6]
	long = E.long_graph()
	assert E.seam_ops(long, 0)[0][1::2].tolist() == [[E.OP_X, 1]] * 3


# what the scan graphs have to place between them under the split, by the names of scan_reach()
SCAN_WANTED = {
	"wave_seam_merge_=", "wave_seam_merge_X", "wave_seam_merge_I", "wave_seam_merge_D", "wave_seam_break",
	"block_seam_merge_=", "block_seam_merge_X", "block_seam_merge_I", "block_seam_merge_D", "block_seam_break",
	"skipped_wave_equal", "skipped_wave_different", "skipped_block_equal", "skipped_block_different", "skipped_block_into_later_wave",
	"skipped_from_lane_0", "skipped_up_to_lane_63",
	"carried_D_through_skipped_wave", "carried_D_through_skipped_block", "carried_X_through_skipped_wave", "carried_X_through_skipped_block",
	"D_skipped_wave_M", "D_skipped_block_M",
	"dense_tile_last_of_wave", "dense_tile_first_of_wave", "dense_tile_last_of_block", "dense_tile_first_of_block", "row_with_more_than_65535_ops",
	"empty_tile_count_at_wave_seam", "empty_tile_count_at_block_seam",
}


def test_the_scan_graphs_place_what_they_are_meant_to_under_the_split():
	K = sgs.kernel_constants()
	T = K.kTileBytes
	union = set()
	for sg, plain in zip(E.scan_graphs(), M.scan_graphs()):
		got = E.scan_reach(sg)
		assert E.SCAN_REACHED_BY[sg.name] <= got, (sg.name, sorted(E.SCAN_REACHED_BY[sg.name] - got))
		union |= E.SCAN_REACHED_BY[sg.name]
		assert 513 <= -(-sg.length // T) <= 640 and len(sg.rows) <= 8
		R = int(sg.kept.sum())
		for row in sg.rows:
			ops, length = E.seam_ops(sg, row)
			E.check_invariants(ops, R, length, is_ref_row=row == PLOIDY_MAX)
			assert np.array_equal(E.fold(ops), M.seam_ops(sg, row)[0]) and np.array_equal(E.fold(ops), M.seam_ops(plain, row)[0]), (sg.name, row)
	assert SCAN_WANTED <= union, sorted(SCAN_WANTED - union)
	# the unsplit model of the retouched graph's arrays is the walk's
	sg = E.scan_graph(2)
	for row in (0, 3):
		assert np.array_equal(E.model_ops(sg.g, row)[0], E.seam_ops(sg, row)[0])


def test_what_the_scan_graphs_mean_in_split_ops():
	"""Written down by hand: X ... a skipped block (and a wave) ... X is one X op of length 2."""
	T = sgs.kernel_constants().kTileBytes
	eq, x, d = E.OP_EQ, E.OP_X, E.OP_D
	for which, extra in ((1, 0), (2, 1)):
		sg = E.scan_graph(which)
		R = 256 * T + 1 + 8 + T + 300
		assert int(sg.kept.sum()) == R
		assert E.seam_ops(sg, PLOIDY_MAX)[0].tolist() == [[eq, R]]
		assert E.seam_ops(sg, 1)[0].tolist() == [[eq, 256 * T - 6], [d, 11], [eq, R - 256 * T - 5]]          # D ... skipped ... D
		assert E.seam_ops(sg, 2)[0].tolist() == [[eq, 256 * T - 6], [d, 6], [eq, R - 256 * T]]               # D ... skipped ... =
		assert E.seam_ops(sg, 3)[0].tolist() == [[eq, 256 * T - 1], [x, 2], [eq, T + 308]]                   # X ... skipped ... X
		assert E.seam_ops(sg, 4)[0].tolist() == [[eq, 256 * T], [x, 1], [eq, T + 308]]                       # = ... skipped ... X
		assert E.seam_ops(sg, 5)[0].tolist() == [[eq, 256 * T - 1], [x, 1], [eq, T + 309]]                   # X ... skipped ... =
	sg = E.scan_graph(0)
	ops = E.seam_ops(sg, 0)[0]
	assert len(ops) > 65535 and ops[:5, 0].tolist() == [eq, E.OP_I, x, E.OP_I, eq]                       # the dense tiles: = I X I = I ...
	ops = E.seam_ops(sg, 3)[0]                                                                        # X ... a skipped wave ... X
	assert ops[:, 0].tolist() == [eq, x, eq] and ops[1, 1] == 2
	ops = E.seam_ops(sg, 6)[0]                                                                        # X ... skipped from lane 0 ... X, then the X run across 511|512
	assert ops.tolist()[1:] == [[x, 2], [eq, ops[2, 1]], [x, 40], [eq, 700]]


def all_seam_graphs():
	return E.eqx_graphs() + M.ops_seam_graphs()


def test_fold_of_the_split_model_is_the_unsplit_model():
	for sg in all_seam_graphs():
		R = int(sg.kept.sum())
		for row in sg.rows:
			ops, length = E.seam_ops(sg, row)
			assert np.array_equal(E.fold(ops), M.seam_ops(sg, row)[0]), (sg.name, row)
			assert length == M.seam_ops(sg, row)[1]
			E.check_invariants(ops, R, length, is_ref_row=row == PLOIDY_MAX)
			# the builder's description and the walk over the graph's arrays agree on the split ops too
			assert np.array_equal(E.model_ops(sg.g, row)[0], ops), (sg.name, row)
	g = M.dash_graph()
	for r in DASH_ROWS:
		ops, length = E.model_ops(g, r)
		assert np.array_equal(E.fold(ops), M.model_ops(g, r)[0]) and length == M.model_ops(g, r)[1]
		E.check_invariants(ops, len(g.ref), length, is_ref_row=r == PLOIDY_MAX)
	assert E.model_ops(g, 0)[0].tolist() == [[E.OP_EQ, 4], [E.OP_X, 1], [E.OP_I, 2], [E.OP_EQ, 5]]        # "a-c" over "T": a/T is X
	assert E.model_ops(g, 2)[0].tolist() == [[E.OP_EQ, 6], [E.OP_D, 4]]                                 # "-" over "-": '='


@pytest.mark.parametrize("stem", ["test-1a", "test-1b", "test-2", "test-3", "test-4"])
def test_fixture_rows_with_cuts_fold_to_the_unsplit_model(stem):
	fasta = {"test-1a": "test-1.fa", "test-1b": "test-1.fa"}.get(stem, stem + ".fa")
	g = oracle.build_variant_graph(os.path.join(FIX, fasta), os.path.join(FIX, stem + ".vcf"), "1")
	for r in M.rows_with_cuts(g):
		ops, length = E.model_ops(g, r)
		assert np.array_equal(E.fold(ops), M.model_ops(g, r)[0])
		E.check_invariants(ops, len(g.ref), length, is_ref_row=r == PLOIDY_MAX)


def plain_bytes_equal(a, b):
	"""The case rule once more, byte by byte and without numpy."""
	return a == b or ((a ^ b) == 0x20 and ord("a") <= (a | 0x20) <= ord("z"))


def test_the_models_X_columns_are_where_the_recorded_rows_differ():
	"""Every tests/golden/derived/*.haplotypes.a2m: on the columns where both the recorded REF row and the recorded row hold a byte, the model's
	split ops of the row (rows from the oracle on the fixture's graph) say X exactly where the two recorded bytes differ under the case rule."""
	paths = sorted(glob.glob(os.path.join(DERIVED, "*.haplotypes.a2m")))
	assert len(paths) >= 5
	for path in paths:
		stem = os.path.basename(path).split(".")[0]
		fasta = {"test-1a": "test-1.fa", "test-1b": "test-1.fa"}.get(stem, stem + ".fa")
		g = oracle.build_variant_graph(os.path.join(FIX, fasta), os.path.join(FIX, stem + ".vcf"), "1")
		records = re.findall(rb">([^\n]*)\n([^\n>]*)\n", open(path, "rb").read())
		assert records[0][0] == b"REF" and len(records) == 1 + g.total_chromosome_copies
		ref_row = records[0][1]
		for copy, (_, row) in enumerate(records[1:]):
			assert len(row) == len(ref_row) == g.aligned_length
			_, ref_is_base, row_is_base = M.column_walk(g, copy_index=copy)
			both = [c for c in range(len(row)) if ref_is_base[c] and row_is_base[c]]
			want = {c for c in both if not plain_bytes_equal(ref_row[c], row[c])}
			# the model's ops, expanded back to columns
			ops, _ = E.model_ops(g, copy)
			live = np.flatnonzero(ref_is_base | row_is_base)
			per_column = np.repeat(ops[:, 0], ops[:, 1])
			assert per_column.size == live.size
			got = {int(c) for c in live[per_column == E.OP_X]}
			assert got == want, (stem, copy)
			assert {int(c) for c in live[per_column == E.OP_EQ]} == set(both) - want


# ---- the PAF formatter -------------------------------------------------------------------------------------------------------------------

q, x, i, d = E.OP_EQ, E.OP_X, E.OP_I, E.OP_D
BIG = 2 ** 32 - 1
HAND_MADE = [
	("single_eq", [(q, 10)]),
	("single_X", [(x, 4)]),
	("leading_I", [(i, 3), (q, 7)]),
	("leading_D", [(d, 4), (x, 6), (i, 2), (q, 1)]),
	("trailing_D", [(q, 6), (d, 4)]),
	("trailing_I", [(q, 6), (x, 1), (i, 9)]),
	("I_then_D", [(q, 5), (i, 2), (d, 3), (x, 4)]),
	("both_ends", [(d, 1), (i, 2), (q, 3), (d, 4), (x, 5), (q, 2), (i, 6), (d, 7)]),
	("no_eq_or_X", [(d, 4), (i, 2)]),
	("no_ops", []),
	("max_length", [(q, BIG), (d, BIG), (x, 1), (i, BIG), (q, BIG)]),
]


def sizes(ops):
	return sum(n for o, n in ops if o != i), sum(n for o, n in ops if o != d)


@pytest.mark.parametrize("name,ops", HAND_MADE, ids=[h[0] for h in HAND_MADE])
def test_host_paf_text_is_the_models(name, ops):
	from vcf2multialign_amd import host
	a = np.array(ops, dtype=np.uint32).reshape(-1, 2)
	t_size, q_size = sizes(ops)
	expected = E.paf_text(a, "chr1.REF", t_size, "chr1.S-1.2", q_size)
	assert host.paf_text(a, "chr1.REF", t_size, "chr1.S-1.2", q_size) == expected
	if name in ("no_eq_or_X", "no_ops"):
		assert expected == b""
	else:
		f = expected[:-1].split(b"\t")
		assert len(f) == 14 and expected.endswith(b"\n") and f[4] == b"+" and f[11] == b"255"
		assert int(f[9]) == sum(n for o, n in ops if o == q) and int(f[12][5:]) == int(f[10]) - int(f[9])


def test_paf_text_spelled_out():
	from vcf2multialign_amd import host
	ops = np.array([(d, 1), (i, 2), (q, 3), (d, 4), (x, 5), (q, 2), (i, 6), (d, 7)], dtype=np.uint32)
	text = b"S.1\t18\t2\t12\t+\tREF\t22\t1\t15\t5\t14\t255\tNM:i:9\tcg:Z:3=4D5X2=\n"
	assert E.paf_text(ops, "REF", 22, "S.1", 18) == text
	assert host.paf_text(ops, "REF", 22, "S.1", 18) == text
	for bad in (0, 3, 9):          # M: the caller has not asked for the split
		with pytest.raises(ValueError):
			host.paf_text(np.array([(q, 3), (bad, 3)], dtype=np.uint32), "REF", 6, "S.1", 6)


def test_host_paf_text_on_every_model_row():
	from vcf2multialign_amd import host
	n = 0
	for sg in all_seam_graphs():
		R = int(sg.kept.sum())
		for row in sg.rows:
			ops, length = E.seam_ops(sg, row)
			want = E.paf_text(ops, "REF", R, "S.%d" % n, length)
			assert host.paf_text(ops, "REF", R, "S.%d" % n, length) == want, (sg.name, row)
			if row == PLOIDY_MAX:
				assert want == ("S.%d\t%d\t0\t%d\t+\tREF\t%d\t0\t%d\t%d\t%d\t255\tNM:i:0\tcg:Z:%d=\n" % (n, R, R, R, R, R, R, R)).encode()
			n += 1
	g = M.dash_graph()
	for r in DASH_ROWS:
		ops, length = E.model_ops(g, r)
		assert host.paf_text(ops, "REF", len(g.ref), "d", length) == E.paf_text(ops, "REF", len(g.ref), "d", length)


def test_the_header_holds_the_split():
	with open(os.path.join(ROOT, "include", "v2m_hip.h")) as f:
		text = f.read()
	for line in ("#define V2M_OPS_SPLIT_MATCH 0x4u", "#define V2M_OP_EQ 7u", "#define V2M_OP_X 8u", "#define V2M_ABI_VERSION 5"):
		assert re.search(r"^" + re.escape(line) + r"\b", text, re.M), line
	from vcf2multialign_amd import _native as N
	assert (N.OP_EQ, N.OP_X, N.OPS_SPLIT_MATCH) == (E.OP_EQ, E.OP_X, E.OPS_SPLIT_MATCH) == (7, 8, 4)
