"""The model of the row alignment ops (tests/row_ops_model.py) against the oracle, the host library's chain formatter against the model's, and
what the ops seam graphs place.  No GPU."""

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
