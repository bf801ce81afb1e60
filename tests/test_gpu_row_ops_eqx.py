"""Context.row_ops(rows, split_match=True) (v2m_row_ops with V2M_OPS_SPLIT_MATCH: count_row_ops_eqx_kernel, scan_row_ops_eqx_kernel,
emit_row_ops_eqx_kernel) against the model of tests/row_ops_eqx_model.py, op for op and length for length; its fold against the unsplit call of
the same context; and --output-paf against the model's PAF text.

Inputs: the graphs of row_ops_eqx_model.py, which place '=' / 'X' runs at the kernels' seams (tests/test_row_ops_eqx_host.py asserts that they
do, without a GPU); the ops graphs and the dash graph of row_ops_model.py; the reference's fixtures and a synthetic graph, founder rows with
cuts among them."""

import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle
import row_ops_eqx_model as E
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
DASH_ROWS = [PLOIDY_MAX, 0, 1, 2, 3, 4, [(0, 0), (2, 2)]]


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


def check_both_forms(ctx, rows, want, ref_length, what, split_first):
	"""The split ops are the model's and hold the invariants; folded they are the unsplit call's, whichever is made first."""
	if split_first:
		got = ctx.row_ops(rows, split_match=True)
		plain = ctx.row_ops(rows)
	else:
		plain = ctx.row_ops(rows)
		got = ctx.row_ops(rows, split_match=True)
	same_ops(got, want, what)
	for r, (ops, length) in zip(rows, got):
		E.check_invariants(ops, ref_length, length, is_ref_row=not isinstance(r, list) and r == PLOIDY_MAX)
	same_ops([(E.fold(ops), length) for ops, length in got], plain, what + " folded")
	return got


def seam_expected(sg, rows):
	by_row = {r: E.seam_ops(sg, r) for r in set(rows)}
	return [by_row[r] for r in rows]


def check_seam(v2m, ctx, sg, rows, split_first=True):
	ctx.upload_graph(v2m.VariantGraph.from_object(sg.g), sg.g.ref)
	return check_both_forms(ctx, rows, seam_expected(sg, rows), int(sg.kept.sum()), sg.name, split_first)


def check_graph(v2m, ctx, g, rows, what, split_first=True):
	ctx.upload_graph(v2m.VariantGraph.from_object(g), g.ref)
	return check_both_forms(ctx, rows, [E.model_ops(g, r) for r in rows], len(g.ref), what, split_first)


# ---- the eqx graphs ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("index", range(len(E.eqx_graphs())), ids=[sg.name for sg in E.eqx_graphs()])
def test_eqx_graphs(v2m, ctx, index):
	sg = E.eqx_graphs()[index]
	got = check_seam(v2m, ctx, sg, sg.rows, split_first=bool(index & 1))
	if "eqx_dense" == sg.name:
		assert len(got[1][0]) == T + 1 and got[1][0][:T, 1].max() == 1          # = X = X ...: 16 384 ops from tile 0
		assert ctx.row_ops([0])[0][0].tolist() == [[M.OP_M, T + 37]]
	if "eqx_skipped_1" == sg.name:
		assert got[2][0][:, 0].tolist() == [E.OP_EQ, E.OP_X, E.OP_EQ] and got[2][0][1, 1] == 2      # X ... one skipped tile ... X: one op
		assert got[3][0][:, 0].tolist() == [E.OP_EQ, E.OP_X, E.OP_EQ] and got[3][0][1, 1] == 1      # = ... one skipped tile ... X: two


@pytest.mark.parametrize("index", range(len(M.ops_seam_graphs())), ids=[sg.name for sg in M.ops_seam_graphs()])
def test_ops_graphs(v2m, ctx, index):
	sg = M.ops_seam_graphs()[index]
	check_seam(v2m, ctx, sg, sg.rows, split_first=not (index & 1))


def test_literal_dashes(v2m, ctx):
	got = check_graph(v2m, ctx, M.dash_graph(), DASH_ROWS, "dashes")
	assert got[3][0].tolist() == [[E.OP_EQ, 6], [E.OP_D, 4]]          # copy 2: a literal '-' over a literal '-' is '='


# ---- fixtures and a synthetic graph, rows with cuts ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("where,stem,fasta", FIXTURES, ids=[os.path.basename(f[0])[:7] + "-" + f[1] for f in FIXTURES])
def test_reference_fixtures(v2m, ctx, where, stem, fasta):
	g = oracle.build_variant_graph(os.path.join(where, fasta), os.path.join(where, stem + ".vcf"), "1")
	check_graph(v2m, ctx, g, M.rows_with_cuts(g), stem)


def test_synthetic_graph_with_founder_rows(v2m, ctx, tmp_path):
	g = synth.build_case(tmp_path, 8201, 80000, 1500, 3, multi_allelic=0.2, long_every=25, max_indel=64)
	g = synth.with_random_paths(g, 1, 0.05)
	check_graph(v2m, ctx, g, M.rows_with_cuts(g, 1), "synth", split_first=False)


def test_seam_graph_rows_with_cuts(v2m, ctx):
	sg = E.boundary_graph()
	rows = M.rows_with_cuts(sg.g)
	assert any(isinstance(r, list) for r in rows)
	check_graph(v2m, ctx, sg.g, rows, sg.name + " with cuts")


# ---- many rows, slices ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_rows", [K.kGroupRowsLds + 1, 2 * K.kGroupRowsLds + 1])
def test_more_rows_than_the_cached_words_and_than_a_group(v2m, ctx, n_rows):
	for sg in (E.boundary_graph(), E.skipped_graph(2)):
		check_seam(v2m, ctx, sg, M.many_rows(sg, n_rows))


SLICE_CHILD = r"""
import os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np
import row_ops_model as M
import row_ops_eqx_model as E
import vcf2multialign_amd as v2m
out = {}
with v2m.Context(0) as ctx:
	for sg, rows in ((E.boundary_graph(), M.many_rows(E.boundary_graph(), 33)), (E.dense_graph(), E.dense_graph().rows + [0, 0])):
		ctx.upload_graph(v2m.VariantGraph.from_object(sg.g), sg.g.ref)
		for i, (ops, length) in enumerate(ctx.row_ops(rows, split_match=True)):
			out["%%s_%%d_ops" %% (sg.name, i)] = ops
			out["%%s_%%d_length" %% (sg.name, i)] = np.array([length])
np.savez(%(path)r, **out)
"""


def test_several_slices_give_the_one_slice_result(v2m, ctx, tmp_path):
	"""V2M_OPS_SLICE_BYTES = 1024 (85 records): the 33 rows of the boundary graph are emitted in more than two pieces from the slice's tables,
	and a row of the dense graph alone (16 385 split ops) exceeds the budget and goes through on its own."""
	path = str(tmp_path / "sliced.npz")
	env = dict(os.environ, V2M_OPS_SLICE_BYTES="1024")
	r = subprocess.run([sys.executable, "-c", SLICE_CHILD % {"root": ROOT, "path": path}], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=env)
	assert r.returncode == 0, r.stdout.decode(errors="replace")[-4000:]
	sliced = np.load(path)
	for sg, rows in ((E.boundary_graph(), M.many_rows(E.boundary_graph(), 33)), (E.dense_graph(), E.dense_graph().rows + [0, 0])):
		whole = check_seam(v2m, ctx, sg, rows)
		assert sum(len(ops) for ops, _ in whole) * 12 > 2 * 1024
		got = [(sliced["%s_%d_ops" % (sg.name, i)], int(sliced["%s_%d_length" % (sg.name, i)][0])) for i in range(len(rows))]
		same_ops(got, whole, sg.name + " in slices")


# ---- the raw ABI ---------------------------------------------------------------------------------------------------------------------------

def test_flags_and_sink(v2m):
	from vcf2multialign_amd import _native as N
	with v2m.Context(0) as c:
		sg = E.boundary_graph()
		c.upload_graph(v2m.VariantGraph.from_object(sg.g), sg.g.ref)
		batch = v2m.RowBatch(sg.rows)
		seen = []
		count = N.OPS_SINK_FN(lambda _u, row, _ops, _n, _len: seen.append(row) or 0)
		assert N.V2M_OK == c._lib.v2m_row_ops(c._h, C.byref(batch.struct), 0x4, count, None) and seen == list(range(len(sg.rows)))
		for flags in (1, 2, 5, 8):
			del seen[:]
			assert N.V2M_ERR_INVALID_ARGUMENT == c._lib.v2m_row_ops(c._h, C.byref(batch.struct), flags, count, None) and not seen
		del seen[:]
		abort = N.OPS_SINK_FN(lambda _u, row, _ops, _n, _len: seen.append(row) or (1 if row == 2 else 0))
		assert N.V2M_ERR_SINK == c._lib.v2m_row_ops(c._h, C.byref(batch.struct), N.OPS_SPLIT_MATCH, abort, None) and seen == [0, 1, 2]
		same_ops(c.row_ops(sg.rows, split_match=True), seam_expected(sg, sg.rows), "after the errors")


def test_a_window_in_force_is_neither_used_nor_disturbed(v2m, ctx):
	sg = E.boundary_graph()
	rows = sg.rows
	ctx.upload_graph(v2m.VariantGraph.from_object(sg.g), sg.g.ref)
	want = seam_expected(sg, rows)
	b, e = T - 100, 2 * T + 333
	ctx.set_column_window(b, e)
	before = [ctx.splice_rows(rows, unaligned=u) for u in (False, True)]
	assert before[0] == [sg.body(r, False, (b, e)) for r in rows]
	same_ops(ctx.row_ops(rows, split_match=True), want, "under a column window")
	assert ctx.window_length == e - b
	assert [ctx.splice_rows(rows, unaligned=u) for u in (False, True)] == before
	windows = [(5, 900), (T - 7, T + 9), (3 * T, sg.length)]
	ctx.set_window_set(windows)
	pieces = [ctx.splice_window_set(rows, unaligned=u) for u in (False, True)]
	same_ops(ctx.row_ops(rows, split_match=True), want, "under a window set")
	assert [ctx.splice_window_set(rows, unaligned=u) for u in (False, True)] == pieces
	assert pieces[1] == [[sg.body(r, True, w) for w in windows] for r in rows]
	ctx.set_column_window(0, sg.length)
	same_ops(ctx.row_ops(rows, split_match=True), want, "whole rows again")


# ---- the driver ----------------------------------------------------------------------------------------------------------------------------

def _run(args, cwd=None):
	assert os.path.exists(CLI), "build the host driver first (__graft_entry__.build())"
	return subprocess.run([CLI] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def test_cli_output_paf_haplotypes(v2m, ctx, tmp_path):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	g = oracle.build_variant_graph(fa, vcf, "1")
	paf, chain, alone, out = tmp_path / "out.paf", tmp_path / "out.chain", tmp_path / "alone.chain", tmp_path / "out.fa"
	r = _run(["-H", "-r", fa, "-a", vcf, "-c", "1", "--output-paf=" + str(paf)])
	assert r.returncode == 0, r.stderr.decode()
	assert paf.read_bytes() == E.haplotype_paf(g)
	assert paf.read_bytes().count(b"\n") == g.total_chromosome_copies and b"X" in paf.read_bytes()
	# beside -s and --output-chain, with a chromosome prefix: the same lines, and the chain file --output-chain alone writes
	r = _run(["-H", "-r", fa, "-a", vcf, "-c", "1", "-m", "chrT", "--output-chain=" + str(alone)])
	assert r.returncode == 0, r.stderr.decode()
	r = _run(["-H", "-r", fa, "-a", vcf, "-c", "1", "-s", str(out), "--unaligned", "-m", "chrT", "--output-chain=" + str(chain), "--output-paf=" + str(paf)])
	assert r.returncode == 0, r.stderr.decode()
	assert paf.read_bytes() == E.haplotype_paf(g, "chrT")
	assert chain.read_bytes() == alone.read_bytes() == M.haplotype_chains(g, "chrT")
	assert out.read_bytes().count(b">") == g.total_chromosome_copies + 1
	# Output.output_paf writes the same bytes through the host library's formatter
	ctx.upload_graph(v2m.VariantGraph.from_object(g), g.ref)
	stream = io.BytesIO()
	assert v2m.HaplotypeOutput(ctx, chromosome_id="chrT").output_paf(v2m.VariantGraph.from_object(g), stream) == g.total_chromosome_copies
	assert stream.getvalue() == E.haplotype_paf(g, "chrT")


def test_cli_output_paf_founders(v2m, ctx, tmp_path):
	from vcf2multialign_amd import host
	g = synth.build_case(tmp_path, 44, 40000, 1200, 6)
	fa, vcf = str(tmp_path / "synth.fa"), str(tmp_path / "synth.vcf")
	paf, chain, alone, cuts_file = tmp_path / "f.paf", tmp_path / "f.chain", tmp_path / "alone.chain", tmp_path / "cuts"
	r = _run(["-F", "3", "-d", "10", "-r", fa, "-a", vcf, "-c", "1", "--output-paf=" + str(paf), "--output-chain=" + str(chain), "-t", str(cuts_file), "--verbose"])
	assert r.returncode == 0, r.stderr.decode()
	cuts, _, _ = host.read_cut_positions(cuts_file)
	lines = r.stdout.decode().split("Matchings:\n")[1].splitlines()[:3]
	assigned = [int(x) for line in lines for x in line.split("\t")[1:]]
	assert len(assigned) == 3 * (len(cuts) - 1)
	assert paf.read_bytes() == E.founder_paf(g, cuts, assigned)
	assert paf.read_bytes().count(b"\n") == 3
	r = _run(["-F", "3", "-d", "10", "-r", fa, "-a", vcf, "-c", "1", "--output-chain=" + str(alone), "-p", str(cuts_file)])
	assert r.returncode == 0, r.stderr.decode()
	assert chain.read_bytes() == alone.read_bytes() == M.founder_chains(g, cuts, assigned)
	ctx.upload_graph(v2m.VariantGraph.from_object(g), g.ref)
	stream = io.BytesIO()
	assert v2m.FounderSequenceGreedyOutput(ctx).output_paf(v2m.VariantGraph.from_object(g), cuts, assigned, stream) == 3
	assert stream.getvalue() == E.founder_paf(g, cuts, assigned)


def test_cli_output_paf_refusals(tmp_path):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	bed = tmp_path / "r.bed"
	bed.write_text("1\t0\t4\n")
	common = ["-H", "-r", fa, "-a", vcf, "-c", "1", "--output-paf=" + str(tmp_path / "x.paf")]
	for extra, what in ((["--region=1-4", "-s", str(tmp_path / "x.a2m")], "--region"), (["--regions-file=" + str(bed)], "--regions-file"), (["--device=0,0"], "more than one --device entry")):
		r = _run(common + extra, cwd=str(tmp_path))
		assert r.returncode != 0
		assert ("ERROR: --output-paf cannot be combined with %s.\n" % what).encode() in r.stderr, r.stderr.decode()
	r = _run(common + ["-m", "chr 1"])
	assert r.returncode != 0 and b"holds whitespace" in r.stderr and not (tmp_path / "x.paf").exists()


# ---- the checked build ---------------------------------------------------------------------------------------------------------------------

CHECKED_CORPUS = [
	"tests/test_gpu_row_ops_eqx.py::test_eqx_graphs",
	"tests/test_gpu_row_ops_eqx.py::test_ops_graphs",
	"tests/test_gpu_row_ops_eqx.py::test_literal_dashes",
	"tests/test_gpu_row_ops_eqx.py::test_reference_fixtures",
	"tests/test_gpu_row_ops_eqx.py::test_seam_graph_rows_with_cuts",
	"tests/test_gpu_row_ops_eqx.py::test_more_rows_than_the_cached_words_and_than_a_group",
	"tests/test_gpu_row_ops_eqx.py::test_a_window_in_force_is_neither_used_nor_disturbed",
]


def test_corpus_on_the_checked_build():
	"""The list above with every LDS object, scratch buffer and staging area poisoned before use (tests/test_gpu_checked_build.py), one run per
	seed: a read of unwritten LDS in the carry words of the split changes ops."""
	from test_gpu_checked_build import SEEDS, run_checked_corpus
	from vcf2multialign_amd import build
	assert os.path.exists(build.CHECKED_LIB_PATH) and os.path.exists(build.CHECKED_HOST_LIB_PATH), "build_native() builds them"
	for seed in SEEDS:   # the second seed only once the first has passed
		rc, out = run_checked_corpus(seed, build.CHECKED_LIB_PATH, build.CHECKED_HOST_LIB_PATH, corpus=CHECKED_CORPUS, timeout=600)
		assert rc == 0, "checked build, seed %s: exit %d\n%s" % (seed, rc, out[-6000:])
		assert " passed" in out and "libv2m_hip_checked.so" in out, out[-3000:]
		print(seed, out.strip().splitlines()[-2])
