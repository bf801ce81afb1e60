"""The model of the row alignment ops (tests/row_ops_model.py) against the oracle, the host library's chain formatter against the model's, and
what the ops seam graphs and the scan graphs place.  No GPU."""

import json
import os

import numpy as np
import pytest

import oracle
import row_ops_model as M
import seam_graphs as sgs
import synth

HERE = os.path.dirname(os.path.abspath(__file__))
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")
FOUNDER_FIX = os.path.join(HERE, "golden", "reference-fixtures", "founder-sequences")
PLOIDY_MAX = M.PLOIDY_MAX
FIXTURES = [("test-1a", "test-1.fa"), ("test-1b", "test-1.fa"), ("test-2", "test-2.fa"), ("test-3", "test-3.fa"), ("test-4", "test-4.fa")]
FOUNDER_FIXTURES = [("test-1", "test-1.fa"), ("test-2", "test-2.fa"), ("test-3", "test-3.fa"), ("test-4", "test-4.fa")]


rows_with_cuts = M.rows_with_cuts


def check_graph(g, rows):
	R = len(g.ref)
	for r in rows:
		row, ref_is_base, row_is_base = M.walk_row(g, r)
		assert row == M.oracle_row(g, r), r
		unaligned = np.frombuffer(row, dtype=np.uint8)[row_is_base].tobytes()
		assert unaligned == M.oracle_row(g, r, unaligned=True), r
		assert int(ref_is_base.sum()) == R
		assert np.frombuffer(row, dtype=np.uint8)[ref_is_base & row_is_base].size <= R
		M.check_invariants(M.ops_from_masks(ref_is_base, row_is_base), R, len(unaligned), is_ref_row=(r == PLOIDY_MAX if not isinstance(r, list) else False))


@pytest.mark.parametrize("stem,fasta", FIXTURES)
def test_walk_and_invariants_on_the_variant_graph_fixtures(stem, fasta):
	g = oracle.build_variant_graph(os.path.join(FIX, fasta), os.path.join(FIX, stem + ".vcf"), "1")
	check_graph(g, rows_with_cuts(g))
	assert max(len(M.model_ops(g, r)[0]) for r in range(g.total_chromosome_copies)) <= 5


@pytest.mark.parametrize("stem,fasta", FOUNDER_FIXTURES)
def test_walk_and_invariants_on_the_founder_fixtures(stem, fasta):
	g = oracle.build_variant_graph(os.path.join(FOUNDER_FIX, fasta), os.path.join(FOUNDER_FIX, stem + ".vcf"), "1")
	check_graph(g, rows_with_cuts(g))


@pytest.mark.parametrize("seed", range(4))
def test_walk_and_invariants_on_synthetic_graphs(tmp_path, seed):
	g = synth.build_case(tmp_path, 8100 + seed, 30000 + 7000 * seed, 600, 3, multi_allelic=0.2, long_every=(0, 25)[seed & 1], max_indel=(8, 64)[seed >> 1])
	g = synth.with_random_paths(g, seed, (0.05, 0.3, 0.8, 0.3)[seed])
	check_graph(g, rows_with_cuts(g, seed))


def test_dash_graph_keeps_literal_dashes_as_bytes():
	g = M.dash_graph()
	assert b"-" in g.ref and b"-" in g.label_bytes
	check_graph(g, [PLOIDY_MAX] + list(range(5)))
	ops, length = M.model_ops(g, 0)          # copy 0: "A-CG" | label "a-c" over T + 3 padding | "-GA" | "C-"
	assert ops.tolist() == [[M.OP_M, 5], [M.OP_I, 2], [M.OP_M, 5]] and length == 12
	assert M.model_ops(g, 2)[0].tolist() == [[M.OP_M, 6], [M.OP_D, 4]]


def test_seam_graph_masks_are_the_walks():
	"""seam_masks (the builder's description) and column_walk (the graph's arrays) give the same masks and ops."""
	for sg in M.ops_seam_graphs() + [sgs.geometry_graph(sgs.kernel_constants().kTileBytes + 17)]:
		for row in sg.rows:
			_, ref_is_base, row_is_base = M.column_walk(sg.g, copy_index=row)
			a, b = M.seam_masks(sg, row)
			assert np.array_equal(a, ref_is_base) and np.array_equal(b, row_is_base), (sg.name, row)
			assert sg.body(row) == sg.oracle_body(row)
			M.check_invariants(M.seam_ops(sg, row)[0], int(sg.kept.sum()), int(b.sum()), is_ref_row=row == PLOIDY_MAX)


def test_the_ops_graphs_place_what_they_are_meant_to():
	K = sgs.kernel_constants()
	for sg in M.ops_seam_graphs():
		got = M.reach(sg)
		assert M.REACHED_BY[sg.name] <= got, (sg.name, sorted(M.REACHED_BY[sg.name] - got))
		assert 2 <= -(-sg.length // K.kTileBytes) <= 4
	dense = M.dense_graph()
	assert len(M.seam_ops(dense, 0)[0]) == K.kTileBytes + 1          # 16 384 ops from tile 0, and the M run of the tail
	for n in (K.kGroupRowsLds + 1, 2 * K.kGroupRowsLds + 1):
		rows = M.many_rows(M.boundary_graph(), n)
		assert len(rows) == n and rows.count(PLOIDY_MAX) >= 4 and len(set(rows)) == 5
	assert (K.kGroupRowsLds + 1, 2 * K.kGroupRowsLds + 1) == (17, 33)


# ---- the scan graphs -----------------------------------------------------------------------------------------------------------------

# what the graphs for the scan kernels' seams have to place between them, by the names of scan_reach()
SCAN_WANTED = {
	"wave_seam_merge_M", "wave_seam_merge_I", "wave_seam_merge_D", "wave_seam_break", "block_seam_merge_M", "block_seam_merge_I", "block_seam_merge_D", "block_seam_break",
	"skipped_wave_equal", "skipped_wave_different", "skipped_block_equal", "skipped_block_different", "skipped_block_into_later_wave",
	"skipped_from_lane_0", "skipped_up_to_lane_63",
	"carried_D_through_skipped_wave", "carried_D_through_skipped_block", "D_skipped_wave_M", "D_skipped_block_M",
	"dense_tile_last_of_wave", "dense_tile_first_of_wave", "dense_tile_last_of_block", "dense_tile_first_of_block", "row_with_more_than_65535_ops",
	"empty_tile_count_at_wave_seam", "empty_tile_count_at_block_seam",
}


def test_scan_reach_on_hand_made_classes():
	"""scan_reach_classes on class rows written out here: a tile is 4 columns, so tile i is columns [4 i, 4 i + 4)."""
	def row(*pieces):
		cls = np.zeros(4 * 600, dtype=np.uint8)
		for first_tile, codes in pieces:
			cls[4 * first_tile:4 * first_tile + len(codes)] = codes
		return cls
	live = [3] * (4 * 600)
	assert M.scan_reach_classes(row((0, live)), 4, "_DIM", set()) == {"wave_seam_merge_M", "block_seam_merge_M"}
	# tiles 64 ... 127 skipped, D before and D after: one whole wave of block 0, from lane 0 to lane 63
	got = M.scan_reach_classes(row((0, [3] * 255 + [1]), (128, [1, 3] + [3] * 400)), 4, "_DIM", set())
	assert {"skipped_wave_equal", "carried_D_through_skipped_wave", "skipped_up_to_lane_63"} <= got and "skipped_wave_different" not in got and "skipped_from_lane_0" not in got
	# tiles 63 ... 127 skipped, M before and I after: wave 1 is skipped whole, and no live tile stands at either side of the seam 63|64
	got = M.scan_reach_classes(row((0, [3] * 252), (128, [2] * 8)), 4, "_DIM", set())
	assert "skipped_wave_different" in got and "wave_seam_break" not in got
	# tiles 0 ... 63 live, 64 ... 255 skipped: no live tile after wave 1 in block 0
	got = M.scan_reach_classes(row((0, [3] * 256), (256, [3] * 8)), 4, "_DIM", set())
	assert not {"skipped_wave_equal", "skipped_block_equal"} & got
	# block 1 skipped, tile 512 live; then with wave 0 of block 2 as well
	got = M.scan_reach_classes(row((0, [3] * 1024), (512, [3] * 8)), 4, "_DIM", set())
	assert "skipped_block_equal" in got and "skipped_block_into_later_wave" not in got and "empty_tile_count_at_block_seam" in got
	got = M.scan_reach_classes(row((0, [3] * 1023 + [1]), (576, [3] * 8)), 4, "_DIM", set())
	assert {"skipped_block_different", "skipped_block_into_later_wave", "D_skipped_block_M", "empty_tile_count_at_wave_seam"} <= got and "skipped_block_equal" not in got
	# tiles 192 ... 196 skipped: from lane 0 of wave 3, which has live lanes after them
	got = M.scan_reach_classes(row((0, [3] * 768), (197, [3] * 40)), 4, "_DIM", set())
	assert "skipped_from_lane_0" in got and "skipped_wave_equal" not in got
	# dense tiles 63 and 256: M I D M | ... ; tile 64 with a skipped column is not dense
	got = M.scan_reach_classes(row((0, live), (63, [3, 2, 1, 3]), (64, [2, 0, 2, 3]), (256, [2, 3, 2, 3])), 4, "_DIM", set())
	assert {"dense_tile_last_of_wave", "dense_tile_first_of_block"} <= got and not {"dense_tile_first_of_wave", "dense_tile_last_of_block"} & got
	assert "wave_seam_break" in got and "block_seam_break" in got


def test_the_scan_graphs_place_what_they_are_meant_to():
	K = sgs.kernel_constants()
	T = K.kTileBytes
	union = set()
	for sg in M.scan_graphs():
		got = M.scan_reach(sg)
		assert M.SCAN_REACHED_BY[sg.name] <= got, (sg.name, sorted(M.SCAN_REACHED_BY[sg.name] - got))
		union |= M.SCAN_REACHED_BY[sg.name]
		assert 513 <= -(-sg.length // T) <= 640 and len(sg.rows) <= 8
		R = int(sg.kept.sum())
		for row in sg.rows:
			ops, length = M.seam_ops(sg, row)
			M.check_invariants(ops, R, length, is_ref_row=row == PLOIDY_MAX)
			# the builder's description and the walk over the graph's arrays agree
			_, ref_is_base, row_is_base = M.column_walk(sg.g, copy_index=row)
			assert np.array_equal(ref_is_base, sg.kept) and np.array_equal(row_is_base, M.seam_masks(sg, row)[1]), (sg.name, row)
		for start, end in sg.notes["skipped"]:
			assert not sg.kept[start * T:end * T].any() and sg.kept[start * T - 1]
	assert SCAN_WANTED <= union, sorted(SCAN_WANTED - union)


def test_what_the_scan_graphs_mean_in_ops():
	"""The op lists written down by hand, so that model and kernel cannot be wrong together."""
	T = sgs.kernel_constants().kTileBytes
	m, i, d = M.OP_M, M.OP_I, M.OP_D
	for extra in (0, 1):
		sg = M.scan_block_graph(extra)
		n_skipped = 256 + 64 * extra
		R = 256 * T + 1 + 8 + T + 300                    # block 0; after the stretch its substitution site and 8 columns; the tail
		assert int(sg.kept.sum()) == R and sg.length == (256 + n_skipped) * T + 1 + 8 + T + 300
		want = {
			PLOIDY_MAX: [[m, R]],
			0: [[m, 256 * T], [i, n_skipped * T], [m, 1 + 8 + T + 300]],              # the label's first byte lies over the reference byte
			1: [[m, 256 * T - 6], [d, 6 + 5], [m, R - 256 * T - 5]],                  # D ... skipped ... D: one op
			2: [[m, 256 * T - 6], [d, 6], [m, R - 256 * T]],
			3: [[m, R]], 4: [[m, R]], 5: [[m, R]],                                   # M ... a skipped block ... M: one op
		}
		for row in sg.rows:
			assert M.seam_ops(sg, row)[0].tolist() == want[row], (sg.name, row)
	sg = M.scan_wave_graph()
	ops = M.seam_ops(sg, 0)[0]
	assert len(ops) == 4 * T + 3 and ops[0].tolist() == [m, 63 * T + 1] and ops[1:2 * T, 1].max() == 1          # tiles 63 and 64: ops 1 ... 32 767 of one column each
	assert ops[2 * T - 1].tolist() == [i, 1] and ops[2 * T].tolist() == [m, 190 * T - 5 * T - 100 + 1]         # then the M run up to tile 255: 190 tiles less the stretch of 5 tiles and 100 columns
	for row in (3, 4, 6):
		assert M.seam_ops(sg, row)[0].tolist() == [[m, int(sg.kept.sum())]]
	# copy 5, the D run across 127|128: 63 full tiles, two dense ones with a reference byte on every other column, then up to 20 columns before tile 128
	before = 63 * T + T + (63 * T - 20)
	assert M.seam_ops(sg, 5)[0].tolist() == [[m, before + 1], [d, 39], [m, int(sg.kept.sum()) - before - 40]]


# ---- the chain formatter -------------------------------------------------------------------------------------------------------------

m, i, d = M.OP_M, M.OP_I, M.OP_D
BIG = 2 ** 32 - 1
HAND_MADE = [
	("single_M", [(m, 10)]),
	("leading_I", [(i, 3), (m, 7)]),
	("leading_D", [(d, 4), (m, 6), (i, 2), (m, 1)]),
	("trailing_D", [(m, 6), (d, 4)]),
	("trailing_I", [(m, 6), (i, 9)]),
	("I_then_D", [(m, 5), (i, 2), (d, 3), (m, 4)]),
	("D_then_I", [(m, 5), (d, 3), (i, 2), (m, 4)]),
	("both_ends", [(d, 1), (i, 2), (m, 3), (d, 4), (m, 5), (i, 6), (d, 7)]),
	("no_M", [(d, 4), (i, 2)]),
	("no_ops", []),
	("max_length", [(m, BIG), (d, BIG), (m, 1), (i, BIG), (m, BIG)]),
]


@pytest.mark.parametrize("name,ops", HAND_MADE, ids=[h[0] for h in HAND_MADE])
def test_host_chain_text_is_the_models(name, ops):
	from vcf2multialign_amd import host
	a = np.array(ops, dtype=np.uint32).reshape(-1, 2)
	t_size = sum(n for o, n in ops if o != i)
	q_size = sum(n for o, n in ops if o != d)
	expected = M.chain_text(a, "chr1.REF", t_size, "chr1.S-1.2", q_size, 7)
	assert host.chain_text(a, "chr1.REF", t_size, "chr1.S-1.2", q_size, 7) == expected
	if name in ("no_M", "no_ops"):
		assert expected == b""
	else:
		head = expected.split(b"\n")[0].split(b" ")
		assert head[0] == b"chain" and int(head[1]) == sum(n for o, n in ops if o == m) and head[-1] == b"7" and expected.endswith(b"\n\n")


def test_chain_text_spelled_out():
	from vcf2multialign_amd import host
	ops = np.array([(d, 1), (i, 2), (m, 3), (d, 4), (m, 5), (i, 6), (d, 7)], dtype=np.uint32)
	text = b"chain 8 REF 20 + 1 13 S.1 16 + 2 10 3\n3 4 0\n5\n\n"
	assert M.chain_text(ops, "REF", 20, "S.1", 16, 3) == text
	assert host.chain_text(ops, "REF", 20, "S.1", 16, 3) == text
	with pytest.raises(ValueError):
		host.chain_text(np.array([(7, 3)], dtype=np.uint32), "REF", 3, "S.1", 3, 1)


def test_fixture_chain_is_liftable():
	"""test-4's chains, from the model's ops through the host library's formatter (equal to the model's): the block lines of every chain add
	up to the ends in its header."""
	from vcf2multialign_amd import host
	g = oracle.build_variant_graph(os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf"), "1")
	text, k = b"", 0
	for s, sample in enumerate(g.sample_names):
		for c in range(int(g.ploidy_csum[s + 1]) - int(g.ploidy_csum[s])):
			ops, length = M.model_ops(g, int(g.ploidy_csum[s]) + c)
			k += 1
			text += host.chain_text(ops, "chr.REF", len(g.ref), "chr.%s.%d" % (sample, 1 + c), length, k)
	assert text == M.haplotype_chains(g, "chr")
	chains = [c for c in text.split(b"\n\n") if c]
	assert len(chains) == g.total_chromosome_copies
	for c in chains:
		lines = c.split(b"\n")
		head = lines[0].split()
		t, q = int(head[5]), int(head[10])
		for line in lines[1:]:
			f = [int(x) for x in line.split()]
			t += f[0] + (f[1] if len(f) == 3 else 0)
			q += f[0] + (f[2] if len(f) == 3 else 0)
		assert (t, q) == (int(head[6]), int(head[11])) and head[2] == b"chr.REF" and int(head[3]) == len(g.ref)
