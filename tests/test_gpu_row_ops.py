"""Context.row_ops (v2m_row_ops: count_row_ops_kernel, scan_row_ops_kernel, emit_row_ops_kernel) against the model of tests/row_ops_model.py, op
for op and length for length, and --output-chain against the model's chain text.

Inputs: the reference's fixtures and two synthetic graphs, founder rows with cuts included; every seam graph of tests/seam_graphs.py with its
rows; the ops graphs of row_ops_model.py, which place (tests/test_row_ops_model_host.py asserts that they do, without a GPU):
  1  a run that crosses a tile boundary as one op (M, I and D) and one that ends there; a breakpoint at a tile's column 0, at its last column,
     at a 16-byte chunk edge and at a 1-KiB slot edge;
  2  one and two all-skipped tiles between an M run and an M run;
  3  a tile whose every column is a breakpoint (16 384 ops from one tile);
  4  a tile that is one D run, entered through the crossing list and the long-patch queue;
  5  the row's first column in D.  Its first column in I cannot be placed: column 0 of every graph v2m_upload_graph accepts holds the first
     reference byte (node 0 sits at reference position 0 and aligned position 0, and reference positions increase strictly), so a row's
     first column is M or D; the earliest I, from column 1, is placed instead;
  6  the row's last column in D;  7  an aligned length that is no multiple of the tile;
  8  an I run directly followed by a D run inside one edge, and across two edges;
  9  a reference and labels that hold a literal '-';  10  a graph without edges;
  11 17 and 33 rows in a launch, REF rows among them."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import row_ops_model as M
import seam_graphs as S
import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")
FOUNDER_FIX = os.path.join(HERE, "golden", "reference-fixtures", "founder-sequences")
K = S.kernel_constants()
T = K.kTileBytes
PLOIDY_MAX = M.PLOIDY_MAX
FIXTURES = [(FIX, "test-1a", "test-1.fa"), (FIX, "test-1b", "test-1.fa"), (FIX, "test-2", "test-2.fa"), (FIX, "test-3", "test-3.fa"), (FIX, "test-4", "test-4.fa"),
	(FOUNDER_FIX, "test-1", "test-1.fa"), (FOUNDER_FIX, "test-2", "test-2.fa"), (FOUNDER_FIX, "test-3", "test-3.fa"), (FOUNDER_FIX, "test-4", "test-4.fa")]


@pytest.fixture(scope="module")
def v2m():
	import vcf2multialign_amd as v
	return v


@pytest.fixture(scope="module")
def ctx(v2m):
	c = v2m.Context(0)
	yield c
	c.close()


def same_ops(got, want, what):
	assert len(got) == len(want), "%s: %d rows, %d expected" % (what, len(got), len(want))
	for i, ((ops, length), (w_ops, w_length)) in enumerate(zip(got, want)):
		assert ops.dtype == np.uint32 and ops.ndim == 2 and ops.shape[1] == 2
		if ops.shape != w_ops.shape or not np.array_equal(ops, w_ops):
			n = min(len(ops), len(w_ops))
			d = np.flatnonzero((ops[:n] != w_ops[:n]).any(axis=1))
			at = int(d[0]) if d.size else n
			raise AssertionError("%s row %d: %d ops, %d expected, the first difference at op %d: got %s, expected %s" % (
				what, i, len(ops), len(w_ops), at, ops[max(0, at - 2):at + 3].tolist(), w_ops[max(0, at - 2):at + 3].tolist()))
		assert length == w_length, "%s row %d: row length %d, expected %d" % (what, i, length, w_length)


def check_graph(v2m, ctx, g, rows, what):
	ctx.upload_graph(v2m.VariantGraph.from_object(g), g.ref)
	same_ops(ctx.row_ops(rows), [M.model_ops(g, r) for r in rows], what)


def seam_expected(sg, rows):
	by_row = {r: M.seam_ops(sg, r) for r in set(rows)}
	return [by_row[r] for r in rows]


def check_seam(v2m, ctx, sg, rows, upload=True):
	if upload:
		ctx.upload_graph(v2m.VariantGraph.from_object(sg.g), sg.g.ref)
	want = seam_expected(sg, rows)
	got = ctx.row_ops(rows)
	same_ops(got, want, sg.name)
	for r, (ops, length) in zip(rows, got):
		M.check_invariants(ops, int(sg.kept.sum()), length, is_ref_row=r == PLOIDY_MAX)
	return got


# ---- fixtures and synthetic graphs ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("where,stem,fasta", FIXTURES, ids=[os.path.basename(f[0])[:7] + "-" + f[1] for f in FIXTURES])
def test_reference_fixtures(v2m, ctx, where, stem, fasta):
	g = oracle.build_variant_graph(os.path.join(where, fasta), os.path.join(where, stem + ".vcf"), "1")
	rows = M.rows_with_cuts(g)
	check_graph(v2m, ctx, g, rows, stem)
	# the lengths are the unaligned splice's
	bodies = ctx.splice_rows(rows, unaligned=True)
	assert [len(b) for b in bodies] == [n for _, n in ctx.row_ops(rows)]


@pytest.mark.parametrize("seed", [0, 1])
def test_synthetic_graphs_with_founder_rows(v2m, ctx, tmp_path, seed):
	g = synth.build_case(tmp_path, 8200 + seed, 50000 + 30000 * seed, 1500, 3, multi_allelic=0.2, long_every=(0, 25)[seed], max_indel=(8, 64)[seed])
	g = synth.with_random_paths(g, seed, (0.3, 0.05)[seed])
	check_graph(v2m, ctx, g, M.rows_with_cuts(g, seed), "synth %d" % seed)


def test_literal_dashes_and_no_edges(v2m, ctx):
	g = M.dash_graph()
	check_graph(v2m, ctx, g, [PLOIDY_MAX, 0, 1, 2, 3, 4, [(0, 0), (2, 2)]], "dashes")
	check_seam(v2m, ctx, M.edgeless_graph(), [PLOIDY_MAX, 0, 1, PLOIDY_MAX])


# ---- the seam graphs of the row kernels --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["s0", "s0_rotated", "s7"])
def test_mask_graphs(v2m, ctx, which):
	sg = S.mask_graph(*{"s0": (0, 0), "s0_rotated": (0, K.kTileChunks // 4), "s7": (7, 0)}[which])
	check_seam(v2m, ctx, sg, S.mask_rows(8))


def test_short_count_graph(v2m, ctx):
	check_seam(v2m, ctx, S.short_count_graph(), [PLOIDY_MAX, 0, 1, 0, 0, PLOIDY_MAX, 1])


def test_cache_graph(v2m, ctx):
	sg = S.cache_graph()
	check_seam(v2m, ctx, sg, S.cache_rows(2 * K.kGroupRowsLds + 1 + K.kGroupRowsLds // 2))


@pytest.mark.parametrize("length", S.geometry_lengths())
def test_geometry_graphs(v2m, ctx, length):
	sg = S.geometry_graph(length)
	check_seam(v2m, ctx, sg, sg.rows)


@pytest.mark.parametrize("tail", [0, 1, 63])
def test_resolve_graphs(v2m, ctx, tail):
	sg = S.resolve_graph(tail)
	check_seam(v2m, ctx, sg, sg.rows)


# ---- the ops graphs ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("index", range(len(M.ops_seam_graphs())), ids=[sg.name for sg in M.ops_seam_graphs()])
def test_ops_graphs(v2m, ctx, index):
	sg = M.ops_seam_graphs()[index]
	got = check_seam(v2m, ctx, sg, sg.rows)
	if "ops_dense" == sg.name:
		assert len(got[1][0]) == T + 1 and got[1][0][:T, 1].max() == 1


@pytest.mark.parametrize("n_rows", [K.kGroupRowsLds + 1, 2 * K.kGroupRowsLds + 1])
def test_more_rows_than_the_cached_words_and_than_a_group(v2m, ctx, n_rows):
	for sg in (M.boundary_graph(), M.skipped_graph(2)):
		check_seam(v2m, ctx, sg, M.many_rows(sg, n_rows))


# ---- slices -----------------------------------------------------------------------------------------------------------------------------

SLICE_CHILD = r"""
import os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np
import row_ops_model as M
import vcf2multialign_amd as v2m
out = {}
with v2m.Context(0) as ctx:
	for sg, rows in ((M.boundary_graph(), M.many_rows(M.boundary_graph(), 33)), (M.dense_graph(), M.dense_graph().rows + [0, 0])):
		ctx.upload_graph(v2m.VariantGraph.from_object(sg.g), sg.g.ref)
		for i, (ops, length) in enumerate(ctx.row_ops(rows)):
			out["%%s_%%d_ops" %% (sg.name, i)] = ops
			out["%%s_%%d_length" %% (sg.name, i)] = np.array([length])
np.savez(%(path)r, **out)
"""


def test_several_slices_give_the_one_slice_result(v2m, ctx, tmp_path):
	"""V2M_OPS_SLICE_BYTES = 1024 (85 records): the 33 rows of the boundary graph, counted once, are emitted in more than two pieces from the
	slice's tables (a piece begins at a row that is not the slice's first), and a row of the dense graph alone (16 385 ops) exceeds the
	budget and goes through on its own."""
	path = str(tmp_path / "sliced.npz")
	env = dict(os.environ, V2M_OPS_SLICE_BYTES="1024")
	r = subprocess.run([sys.executable, "-c", SLICE_CHILD % {"root": ROOT, "path": path}], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=env)
	assert r.returncode == 0, r.stdout.decode(errors="replace")[-4000:]
	sliced = np.load(path)
	for sg, rows in ((M.boundary_graph(), M.many_rows(M.boundary_graph(), 33)), (M.dense_graph(), M.dense_graph().rows + [0, 0])):
		whole = check_seam(v2m, ctx, sg, rows)
		assert sum(len(ops) for ops, _ in whole) * 12 > 2 * 1024
		got = [(sliced["%s_%d_ops" % (sg.name, i)], int(sliced["%s_%d_length" % (sg.name, i)][0])) for i in range(len(rows))]
		same_ops(got, whole, sg.name + " in slices")


# ---- windows in force --------------------------------------------------------------------------------------------------------------------

def test_a_window_in_force_is_neither_used_nor_disturbed(v2m, ctx):
	sg = M.boundary_graph()
	rows = sg.rows
	ctx.upload_graph(v2m.VariantGraph.from_object(sg.g), sg.g.ref)
	want = seam_expected(sg, rows)
	b, e = T - 100, 2 * T + 333
	ctx.set_column_window(b, e)
	before = [ctx.splice_rows(rows, unaligned=u) for u in (False, True)]
	assert before[0] == [sg.body(r, False, (b, e)) for r in rows]
	same_ops(ctx.row_ops(rows), want, "under a column window")
	assert ctx.window_length == e - b
	assert [ctx.splice_rows(rows, unaligned=u) for u in (False, True)] == before
	windows = [(5, 900), (T - 7, T + 9), (3 * T, sg.length)]
	ctx.set_window_set(windows)
	pieces = [ctx.splice_window_set(rows, unaligned=u) for u in (False, True)]
	same_ops(ctx.row_ops(rows), want, "under a window set")
	assert [ctx.splice_window_set(rows, unaligned=u) for u in (False, True)] == pieces
	assert pieces[1] == [[sg.body(r, True, w) for w in windows] for r in rows]
	ctx.set_column_window(0, sg.length)
	same_ops(ctx.row_ops(rows), want, "whole rows again")


# ---- errors ------------------------------------------------------------------------------------------------------------------------------

def test_errors(v2m):
	from vcf2multialign_amd import _native as N
	with v2m.Context(0) as c:
		with pytest.raises(v2m.V2MError) as e:
			c.row_ops([PLOIDY_MAX])
		assert e.value.code == N.V2M_ERR_STATE
		sg = M.boundary_graph()
		c.upload_graph(v2m.VariantGraph.from_object(sg.g), sg.g.ref)
		d = next(e for e in range(sg.n_edges) if sg.tgt[e] - sg.src[e] >= 2)          # an edge that jumps over a node
		inside = int(sg.src[d]) + 1
		with pytest.raises(v2m.V2MError) as e:
			c.row_ops([[(0, 0), (inside, 1)]])
		assert e.value.code == N.V2M_ERR_PRECONDITION
		batch = v2m.RowBatch(sg.rows)
		seen = []
		sink = N.OPS_SINK_FN(lambda _u, row, _ops, _n, _len: seen.append(row) or (1 if row == 2 else 0))
		assert N.V2M_ERR_SINK == c._lib.v2m_row_ops(c._h, C.byref(batch.struct), 0, sink, None) and seen == [0, 1, 2]
		assert N.V2M_ERR_INVALID_ARGUMENT == c._lib.v2m_row_ops(c._h, C.byref(batch.struct), 1, sink, None)
		same_ops(c.row_ops(sg.rows), seam_expected(sg, sg.rows), "after the errors")


# ---- the driver ---------------------------------------------------------------------------------------------------------------------------

def _run(args, cwd=None):
	assert os.path.exists(CLI), "build the host driver first (__graft_entry__.build())"
	return subprocess.run([CLI] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def test_cli_output_chain_haplotypes(v2m, ctx, tmp_path):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	g = oracle.build_variant_graph(fa, vcf, "1")
	chain, out = tmp_path / "out.chain", tmp_path / "out.fa"
	r = _run(["-H", "-r", fa, "-a", vcf, "-c", "1", "--output-chain=" + str(chain)])
	assert r.returncode == 0, r.stderr.decode()
	assert chain.read_bytes() == M.haplotype_chains(g)
	# beside -s, with a chromosome prefix, with and without the REF row in the sequences: the same chains
	for extra in ([], ["--omit-reference"]):
		r = _run(["-H", "-r", fa, "-a", vcf, "-c", "1", "-s", str(out), "--unaligned", "-m", "chrT", "--output-chain=" + str(chain)] + extra)
		assert r.returncode == 0, r.stderr.decode()
		assert chain.read_bytes() == M.haplotype_chains(g, "chrT")
		assert out.read_bytes().count(b">") == g.total_chromosome_copies + (0 if extra else 1)
	# Output.output_chain writes the same bytes through the host library's formatter
	import io
	ctx.upload_graph(v2m.VariantGraph.from_object(g), g.ref)
	stream = io.BytesIO()
	assert v2m.HaplotypeOutput(ctx, chromosome_id="chrT").output_chain(v2m.VariantGraph.from_object(g), stream) == g.total_chromosome_copies
	assert stream.getvalue() == M.haplotype_chains(g, "chrT")


def test_cli_output_chain_founders(tmp_path):
	from vcf2multialign_amd import host
	g = synth.build_case(tmp_path, 44, 40000, 1200, 6)
	fa, vcf = str(tmp_path / "synth.fa"), str(tmp_path / "synth.vcf")
	chain, cuts_file = tmp_path / "f.chain", tmp_path / "cuts"
	r = _run(["-F", "3", "-d", "10", "-r", fa, "-a", vcf, "-c", "1", "--output-chain=" + str(chain), "-t", str(cuts_file), "--verbose"])
	assert r.returncode == 0, r.stderr.decode()
	cuts, _, _ = host.read_cut_positions(cuts_file)
	lines = r.stdout.decode().split("Matchings:\n")[1].splitlines()[:3]
	assigned = [int(x) for line in lines for x in line.split("\t")[1:]]
	assert len(assigned) == 3 * (len(cuts) - 1)
	assert chain.read_bytes() == M.founder_chains(g, cuts, assigned)
	assert chain.read_bytes().count(b"chain ") == 3


def test_cli_output_chain_refusals(tmp_path):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	bed = tmp_path / "r.bed"
	bed.write_text("1\t0\t4\n")
	common = ["-H", "-r", fa, "-a", vcf, "-c", "1", "--output-chain=" + str(tmp_path / "x.chain")]
	for extra, what in ((["--region=1-4", "-s", str(tmp_path / "x.a2m")], "--region"), (["--regions-file=" + str(bed)], "--regions-file"), (["--device=0,0"], "more than one --device entry")):
		r = _run(common + extra, cwd=str(tmp_path))
		assert r.returncode != 0
		assert ("ERROR: --output-chain cannot be combined with %s.\n" % what).encode() in r.stderr, r.stderr.decode()
	# a name with whitespace is refused before any GPU work
	r = _run(common + ["-m", "chr 1"])
	assert r.returncode != 0 and b"holds whitespace" in r.stderr and not (tmp_path / "x.chain").exists()


# ---- the checked build ----------------------------------------------------------------------------------------------------------------------

CHECKED_CORPUS = [
	"tests/test_gpu_row_ops.py::test_reference_fixtures",
	"tests/test_gpu_row_ops.py::test_synthetic_graphs_with_founder_rows",
	"tests/test_gpu_row_ops.py::test_literal_dashes_and_no_edges",
	"tests/test_gpu_row_ops.py::test_mask_graphs",
	"tests/test_gpu_row_ops.py::test_short_count_graph",
	"tests/test_gpu_row_ops.py::test_cache_graph",
	"tests/test_gpu_row_ops.py::test_geometry_graphs",
	"tests/test_gpu_row_ops.py::test_resolve_graphs",
	"tests/test_gpu_row_ops.py::test_ops_graphs",
	"tests/test_gpu_row_ops.py::test_more_rows_than_the_cached_words_and_than_a_group",
	"tests/test_gpu_row_ops.py::test_a_window_in_force_is_neither_used_nor_disturbed",
]


def test_corpus_on_the_checked_build():
	"""The list above with every LDS object, scratch buffer and staging area poisoned before use (tests/test_gpu_checked_build.py), one run per seed."""
	from test_gpu_checked_build import SEEDS, run_checked_corpus
	from vcf2multialign_amd import build
	assert os.path.exists(build.CHECKED_LIB_PATH) and os.path.exists(build.CHECKED_HOST_LIB_PATH), "build_native() builds them"
	for seed in SEEDS:   # the second seed only once the first has passed
		rc, out = run_checked_corpus(seed, build.CHECKED_LIB_PATH, build.CHECKED_HOST_LIB_PATH, corpus=CHECKED_CORPUS, timeout=600)
		assert rc == 0, "checked build, seed %s: exit %d\n%s" % (seed, rc, out[-6000:])
		assert " passed" in out and "libv2m_hip_checked.so" in out, out[-3000:]
		print(seed, out.strip().splitlines()[-2])
