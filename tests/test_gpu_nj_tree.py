"""The neighbour-joining tree on the GPU (include/v2m_hip.h, "neighbour joining"; csrc/nj_kernels.hpp) against the numpy model of
tests/nj_tree_model.py, byte for byte: every corpus matrix through v2m_nj_tree_of_distances from a guarded upload, the graph items of
tests/pair_distances_model.py through v2m_nj_tree under both definitions, the errors of the raw ABI, the driver, and the corpus again on
the checked build.  The largest matrix has 2 B + 1 taxa (B: nj_join_kernel's workgroup): a few thousand short launches."""

import ctypes as C
import functools
import io
import os

import numpy as np
import pytest

import nj_tree_model as M
import oracle
import pair_distances_model as PM
import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")
PLOIDY_MAX = PM.PLOIDY_MAX
GUARD_ROWS = 2


@pytest.fixture(scope="module")
def v2m():
	import vcf2multialign_amd as v
	from vcf2multialign_amd import _native as N
	assert (N.NJ_ROWS_PER_GROUP, N.NJ_JOIN_THREADS, N.NJ_JOIN_BATCH) == M.kernel_constants() and np.dtype(N.NJ_NODE_DTYPE) == M.NODE_DTYPE
	return v


@pytest.fixture(scope="module")
def ctx(v2m):
	c = v2m.Context(0)
	yield c
	c.close()


def upload(v2m, ctx, g):
	ctx.upload_graph(v2m.VariantGraph.from_object(g), g.ref)


class GuardedMatrix:
	"""The upper triangle of d in a device buffer u32[GUARD_ROWS + n + GUARD_ROWS][pitch], pitch > n: the diagonal, the lower triangle,
	the padding columns and the guard rows hold hostile values that no result may depend on."""

	def __init__(self, d):
		import torch
		n = d.shape[0]
		self.n, self.pitch = n, (n + 1 + 3) // 4 * 4 + 4 * (n % 3)
		rng = np.random.default_rng(n)
		host = rng.integers(1 << 31, 1 << 32, size=(n + 2 * GUARD_ROWS, self.pitch), dtype=np.uint64).astype(np.uint32)
		body = host[GUARD_ROWS:GUARD_ROWS + n]
		upper = np.triu_indices(n, 1)
		body[:, :n][upper] = d[upper]
		self.host = host
		self.device = torch.from_numpy(host.view(np.int32).copy()).cuda()
		self.ptr = self.device.data_ptr() + GUARD_ROWS * self.pitch * 4
		assert self.ptr % 16 == 0 and self.pitch % 4 == 0 and self.pitch > n

	def unchanged(self):
		return np.array_equal(self.device.cpu().numpy().view(np.uint32), self.host)


def same_records(got, want, what):
	assert got.dtype == want.dtype and len(got) == len(want), what
	if got.tobytes() != want.tobytes():
		k = next(i for i in range(len(got)) if got[i:i + 1].tobytes() != want[i:i + 1].tobytes())
		raise AssertionError("%s: the first difference at record %d of %d: got %s, expected %s" % (what, k, len(got), got[k], want[k]))


def check_matrix(ctx, item):
	m = GuardedMatrix(item.d)
	nodes, info = ctx.nj_tree_of_distances(m.ptr, m.n, m.pitch, info=True)
	same_records(nodes, M.expected(item.name), item.name)
	assert m.unchanged(), item.name + ": the input matrix"
	assert (info["n_nodes"], info["n_sites"], info["n_columns"], info["n_passes"]) == (item.n - 2, 0, 0, 0) and info["distances_ms"] == info["tree_ms"] == 0.0      # profiling is off


# ---- the corpus ------------------------------------------------------------------------------------------------------------------------------

SINGLE = [item for item in M.corpus() if not item.name.startswith("six_")]


@pytest.mark.parametrize("item", SINGLE, ids=[i.name for i in SINGLE])
def test_corpus(v2m, ctx, item):
	check_matrix(ctx, item)


def test_the_six_leaf_tree_under_every_relabeling(v2m, ctx):
	six = [item for item in M.corpus() if item.name.startswith("six_")]
	assert len(six) == 720
	for item in six:
		check_matrix(ctx, item)


# ---- beyond one batch of the join kernel ------------------------------------------------------------------------------------------------------

JOIN_BATCH_ITEMS = M.join_batch_items()


@pytest.mark.parametrize("item", JOIN_BATCH_ITEMS, ids=[i.name for i in JOIN_BATCH_ITEMS])
def test_join_batches(v2m, ctx, item):
	"""(J - 1) B + 1, J B and J B + 64 taxa (J B: the live slots nj_join_kernel's loop takes in one trip): the last element of a lane's
	batch, the batch exactly full, and 64 joins whose loop makes a second trip.  tests/test_nj_tree_host.py asserts that those joins move
	slots of the first trip and of the second.  About two launches a taxon, and the model takes a few seconds at these sizes."""
	check_matrix(ctx, item)


@functools.lru_cache(maxsize=None)
def distinct_rows_beyond_a_batch(acgt):
	"""(the item, the model's matrix, the model's records of it): computed once, shared, read-only."""
	_, B, J = M.kernel_constants()
	item = PM.distinct_item(J * B + 64)
	d, V, L = PM.expected(item.g, item.rows, acgt_only=acgt)
	nodes = M.nj(d)
	for a in (d, nodes):
		a.setflags(write=False)
	return item, d, V, L, nodes


@pytest.mark.parametrize("acgt", [False, True], ids=["all", "acgt"])
def test_distinct_rows_beyond_a_join_batch(v2m, ctx, acgt):
	"""J B + 64 rows that all differ, from rows to records: 17 tiles of pack and pair kernels, then the tree of the matrix they left on
	the device, held to the model's records of the model's matrix; ctx.pair_distances of the same rows is that matrix."""
	item, d, V, L, want = distinct_rows_beyond_a_batch(acgt)
	upload(v2m, ctx, item.g)
	nodes, info = ctx.nj_tree(item.rows, acgt_only=acgt, info=True)
	same_records(nodes, want, "%s acgt=%s" % (item.name, acgt))
	assert (info["n_nodes"], info["n_sites"], info["n_columns"]) == (len(item.rows) - 2, V, L), info
	got = ctx.pair_distances(item.rows, acgt_only=acgt)
	assert got.dtype == np.uint32 and np.array_equal(got, d), "%s acgt=%s: pair_distances" % (item.name, acgt)


def test_stage_times_while_profiling(v2m, ctx):
	item = next(i for i in M.corpus() if i.name == "path_noise_101_1")
	m = GuardedMatrix(item.d)
	ctx.profile_enable(True)
	try:
		nodes, info = ctx.nj_tree_of_distances(m.ptr, m.n, m.pitch, info=True)
	finally:
		ctx.profile_enable(False)
		ctx.profile_reset()
	same_records(nodes, M.expected(item.name), item.name)
	assert info["tree_ms"] > 0.0 and info["distances_ms"] == 0.0


# ---- from rows -------------------------------------------------------------------------------------------------------------------------------

def expected_of_rows(item, acgt):
	d, V, L = PM.expected(item.g, item.rows, item.window, acgt_only=acgt)
	return M.nj(d), V, L


GRAPH_ITEMS = M.graph_items()


@pytest.mark.parametrize("item", GRAPH_ITEMS, ids=[i.name for i in GRAPH_ITEMS])
def test_graph_items(v2m, ctx, item):
	upload(v2m, ctx, item.g)
	if item.window:
		ctx.set_column_window(*item.window)
	for acgt in (False, True):
		want, V, L = expected_of_rows(item, acgt)
		nodes, info = ctx.nj_tree(item.rows, acgt_only=acgt, info=True)
		same_records(nodes, want, "%s acgt=%s" % (item.name, acgt))
		_, distances = ctx.pair_distances(item.rows, acgt_only=acgt, info=True)
		assert (info["n_nodes"], info["n_sites"], info["n_columns"], info["n_passes"]) == (len(item.rows) - 2, V, L, distances["n_passes"]), (item.name, info)
		assert (distances["n_sites"], distances["n_columns"]) == (V, L)
		assert info["distances_ms"] == info["tree_ms"] == 0.0


def test_the_views_are_left_as_they_were(v2m, ctx):
	item = next(i for i in GRAPH_ITEMS if i.window)
	g, rows, w = item.g, item.rows, item.window
	upload(v2m, ctx, g)
	sets = [(2, 30), (41, 47), (3, 4)]
	ctx.set_window_set(sets)
	ctx.set_column_window(*w)
	pieces = ctx.splice_window_set(rows)
	before = ctx.column_counts(rows)
	spliced = ctx.splice_rows(rows)
	same_records(ctx.nj_tree(rows), expected_of_rows(item, False)[0], "under a window set and a window")
	assert ctx.window_length == w[1] - w[0] and ctx.window_set_size == len(sets)
	for a, b in zip(before, ctx.column_counts(rows)):
		assert np.array_equal(a, b)
	assert ctx.splice_rows(rows) == spliced and ctx.splice_window_set(rows) == pieces
	ctx.set_column_window(0, g.aligned_length)
	whole = PM.Item("whole", g, rows)
	same_records(ctx.nj_tree(rows, acgt_only=True), expected_of_rows(whole, True)[0], "whole rows again")


# ---- the raw ABI -----------------------------------------------------------------------------------------------------------------------------

def test_errors(v2m):
	import torch
	from vcf2multialign_amd import _native as N
	with v2m.Context(0) as c:
		item = next(i for i in M.corpus() if i.name == "caterpillar_12")
		m = GuardedMatrix(item.d)
		nodes = np.full(16, 7, dtype=M.NODE_DTYPE)
		nodes_before = nodes.tobytes()
		info = N.NjTreeInfo()
		info.n_columns = 77
		of_distances, of_rows = c._lib.v2m_nj_tree_of_distances, c._lib.v2m_nj_tree
		last_error = lambda: c._lib.v2m_last_error(c._h).decode()
		# the matrix form needs no graph
		assert N.V2M_OK == of_distances(c._h, m.ptr, m.n, m.pitch, nodes.ctypes.data, None)
		same_records(nodes[:10], M.expected(item.name), "without a graph")
		nodes[:] = 7
		# n = 0: V2M_OK, nothing touched; n = 1 and n = 2: no tree
		assert N.V2M_OK == of_distances(c._h, m.ptr, 0, m.pitch, nodes.ctypes.data, C.byref(info)) and info.n_columns == 77
		for n in (1, 2):
			assert N.V2M_ERR_INVALID_ARGUMENT == of_distances(c._h, m.ptr, n, m.pitch, nodes.ctypes.data, C.byref(info))
			assert "at least 3 taxa" in last_error()
		# NULL pointers, misalignment, a bad pitch
		assert N.V2M_ERR_INVALID_ARGUMENT == of_distances(c._h, None, m.n, m.pitch, nodes.ctypes.data, None)
		assert N.V2M_ERR_INVALID_ARGUMENT == of_distances(c._h, m.ptr, m.n, m.pitch, None, None)
		for off in (4, 8, 12):
			assert N.V2M_ERR_INVALID_ARGUMENT == of_distances(c._h, m.ptr + off, m.n, m.pitch, nodes.ctypes.data, None) and "16-byte aligned" in last_error()
		for pitch in (m.n - 1, 8, m.pitch + 1, m.pitch + 2):
			assert N.V2M_ERR_INVALID_ARGUMENT == of_distances(c._h, m.ptr, m.n, pitch, nodes.ctypes.data, None) and "pitch" in last_error()
		# more taxa than the limit: refused before anything is allocated or read (the matrix is nowhere near that large)
		free_before = torch.cuda.mem_get_info()[0]
		assert N.V2M_ERR_UNSUPPORTED == of_distances(c._h, m.ptr, N.NJ_MAX_ROWS + 1, N.NJ_MAX_ROWS + 4, nodes.ctypes.data, None) and str(N.NJ_MAX_ROWS) in last_error()
		assert torch.cuda.mem_get_info()[0] == free_before
		assert nodes.tobytes() == nodes_before and info.n_columns == 77 and m.unchanged()
		# from rows: no graph, then NULL rows and nodes, bad flags, too few and too many rows, bad cuts
		graph_item = next(i for i in M.graph_items() if i.name == "sites_64")
		batch = v2m.RowBatch(graph_item.rows)
		assert N.V2M_ERR_STATE == of_rows(c._h, C.byref(batch.struct), 0, nodes.ctypes.data, None)
		upload(v2m, c, graph_item.g)
		assert N.V2M_ERR_INVALID_ARGUMENT == of_rows(c._h, None, 0, nodes.ctypes.data, None)
		assert N.V2M_ERR_INVALID_ARGUMENT == of_rows(c._h, C.byref(batch.struct), 0, None, None)
		for flags in (0x1, 0x2, 0x4, 0x8, 0x10, 0x40, 0x21, 0x80000000):
			assert N.V2M_ERR_INVALID_ARGUMENT == of_rows(c._h, C.byref(batch.struct), flags, nodes.ctypes.data, None) and "v2m_nj_tree" in last_error()
		assert N.V2M_OK == of_rows(c._h, C.byref(v2m.RowBatch([]).struct), 0, nodes.ctypes.data, C.byref(info)) and info.n_columns == 77
		for rows in ([0], [0, PLOIDY_MAX]):
			assert N.V2M_ERR_INVALID_ARGUMENT == of_rows(c._h, C.byref(v2m.RowBatch(rows).struct), 0, nodes.ctypes.data, C.byref(info)) and "at least 3 taxa" in last_error()
		many = v2m.RowBatch([0] * (N.NJ_MAX_ROWS + 1))
		assert N.V2M_ERR_UNSUPPORTED == of_rows(c._h, C.byref(many.struct), 0, nodes.ctypes.data, None) and str(N.NJ_MAX_ROWS) in last_error()
		bad = v2m.RowBatch([0, [(2, 0), (1, 1)], 1])
		assert N.V2M_ERR_PRECONDITION == of_rows(c._h, C.byref(bad.struct), 0, nodes.ctypes.data, None)
		assert nodes.tobytes() == nodes_before and info.n_columns == 77
		# the Python surface: no rows give no records, one row raises
		got, record = c.nj_tree([], info=True)
		assert got.shape == (0,) and got.dtype == M.NODE_DTYPE and record["n_columns"] == graph_item.g.aligned_length
		with pytest.raises(Exception):
			c.nj_tree([0, 1])
		same_records(c.nj_tree(graph_item.rows), expected_of_rows(graph_item, False)[0], "after the errors")


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------

def _run(args, cwd=None):
	import subprocess
	assert os.path.exists(CLI), "build the host driver first (__graft_entry__.build())"
	return subprocess.run([CLI] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def tree_text(g, ids, rows, window=None, acgt_only=False):
	from vcf2multialign_amd import host
	return host.nj_newick_text(M.nj(PM.expected(g, rows, window, acgt_only)[0]), ids)


def test_cli_haplotypes(v2m, ctx, tmp_path):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	g = oracle.build_variant_graph(fa, vcf, "1")
	vg = v2m.VariantGraph.from_object(g)
	ids, rows = PM.haplotype_ids(g)
	assert len(rows) >= 4
	nwk, tsv, a2m = tmp_path / "out.nwk", tmp_path / "out.tsv", tmp_path / "out.fa"
	common = ["-H", "-r", fa, "-a", vcf, "-c", "1"]
	r = _run(common + ["--output-tree=" + str(nwk), "--verbose"])
	assert r.returncode == 0, r.stderr.decode()
	want = tree_text(g, ids, rows)
	d, V, L = PM.expected(g, rows)
	assert nwk.read_bytes() == want == M.newick(M.nj(d), ids) and want.count(b":") == 2 * len(rows) - 3
	assert ("Tree: %d rows, %d columns, %d sites, %d joins." % (len(rows), L, V, len(rows) - 3)).encode() in r.stderr, r.stderr.decode()
	r = _run(common + ["--output-tree=" + str(nwk), "--tree-acgt-only"])
	assert r.returncode == 0, r.stderr.decode()
	assert nwk.read_bytes() == tree_text(g, ids, rows, acgt_only=True)
	s, e = 3, min(len(g.ref), 9)
	w = vg.columns_of_reference_range(s - 1, e)
	for extra in (["--omit-reference"], ["--region=%d-%d" % (s, e)], ["--region=%d-%d" % (s, e), "--omit-reference", "--tree-acgt-only"]):
		r = _run(common + ["--output-tree=" + str(nwk)] + extra)
		assert r.returncode == 0, r.stderr.decode()
		k = 1 if "--omit-reference" in extra else 0
		window = w if any(x.startswith("--region") for x in extra) else None
		assert nwk.read_bytes() == tree_text(g, ids[k:], rows[k:], window, "--tree-acgt-only" in extra), extra
	# beside the other outputs: each is what it is alone; --acgt-only belongs to the distances
	r = _run(common + ["-s", str(a2m), "--output-distances=" + str(tsv), "--acgt-only", "--output-tree=" + str(nwk)])
	assert r.returncode == 0, r.stderr.decode()
	with open(os.path.join(HERE, "golden", "derived", "test-4.haplotypes.a2m"), "rb") as f:
		assert a2m.read_bytes() == f.read()
	assert tsv.read_bytes() == PM.file_text(g, ids, rows, acgt_only=True) and nwk.read_bytes() == want
	# fewer than three sequences: one diploid sample without the reference
	one = tmp_path / "one.vcf"
	with open(vcf) as f:
		lines = f.read().splitlines()
	head = next(i for i, line in enumerate(lines) if line.startswith("#CHROM"))
	one.write_text("\n".join(lines[:head] + ["\t".join(line.split("\t")[:10]) for line in lines[head:]]) + "\n")
	r = _run(["-H", "-r", fa, "-a", str(one), "-c", "1", "--omit-reference", "--output-tree=" + str(tmp_path / "few.nwk")])
	assert r.returncode != 0 and b"ERROR: --output-tree needs at least three sequences (got 2).\n" in r.stderr, r.stderr.decode()
	assert not (tmp_path / "few.nwk").exists()
	# Output.output_tree writes the same bytes
	upload(v2m, ctx, g)
	stream = io.BytesIO()
	info = v2m.HaplotypeOutput(ctx).output_tree(vg, stream)
	assert stream.getvalue() == want and info["n_sites"] == V and info["n_nodes"] == len(rows) - 2
	stream = io.BytesIO()
	v2m.HaplotypeOutput(ctx, should_output_reference=False, region=(s - 1, e)).output_tree(vg, stream, acgt_only=True)
	assert stream.getvalue() == tree_text(g, ids[1:], rows[1:], w, True) and ctx.window_length == g.aligned_length


def test_cli_founders(v2m, ctx, tmp_path):
	from vcf2multialign_amd import host
	g = synth.build_case(tmp_path, 44, 40000, 1200, 6)
	fa, vcf = str(tmp_path / "synth.fa"), str(tmp_path / "synth.vcf")
	nwk, cuts_file = tmp_path / "f.nwk", tmp_path / "cuts"
	r = _run(["-F", "3", "-d", "10", "-r", fa, "-a", vcf, "-c", "1", "--output-tree=" + str(nwk), "-t", str(cuts_file), "--verbose"])
	assert r.returncode == 0, r.stderr.decode()
	cuts, _, _ = host.read_cut_positions(cuts_file)
	lines = r.stdout.decode().split("Matchings:\n")[1].splitlines()[:3]
	assigned = [int(x) for line in lines for x in line.split("\t")[1:]]
	n = len(cuts) - 1
	assert len(assigned) == 3 * n
	rows = [PLOIDY_MAX] + [list(zip(cuts[:-1], assigned[k * n:(k + 1) * n])) for k in range(3)]
	ids = ["REF", "1", "2", "3"]
	want = tree_text(g, ids, rows)
	assert nwk.read_bytes() == want and PM.expected(g, rows)[0].any()
	r = _run(["-F", "3", "-d", "10", "-r", fa, "-a", vcf, "-c", "1", "--output-tree=" + str(nwk), "-p", str(cuts_file), "--omit-reference", "--tree-acgt-only", "--region=1000-30000"])
	assert r.returncode == 0, r.stderr.decode()
	vg = v2m.VariantGraph.from_object(g)
	assert nwk.read_bytes() == tree_text(g, ids[1:], rows[1:], vg.columns_of_reference_range(999, 30000), True)
	upload(v2m, ctx, g)
	stream = io.BytesIO()
	v2m.FounderSequenceGreedyOutput(ctx).output_tree(vg, cuts, assigned, stream)
	assert stream.getvalue() == want


# ---- the checked build -----------------------------------------------------------------------------------------------------------------------

CHECKED_CORPUS = [
	"tests/test_gpu_nj_tree.py::test_corpus",
	"tests/test_gpu_nj_tree.py::test_the_six_leaf_tree_under_every_relabeling",
	"tests/test_gpu_nj_tree.py::test_join_batches[%s]" % M.join_batch_items()[-1].name,      # J B + 64 taxa: a slot nobody updated holds poison
	"tests/test_gpu_nj_tree.py::test_graph_items",
	"tests/test_gpu_nj_tree.py::test_the_views_are_left_as_they_were",
]


def test_corpus_on_the_checked_build():
	"""The list above with every LDS object and every scratch buffer (the working matrix, R, the ids, the row minima and the records
	among them) poisoned before use (tests/test_gpu_checked_build.py), one run per seed: an element of the matrix or a row minimum
	nobody wrote in this call changes the result.  No library is preloaded."""
	from test_gpu_checked_build import SEEDS, run_checked_corpus
	from vcf2multialign_amd import build
	assert os.path.exists(build.CHECKED_LIB_PATH) and os.path.exists(build.CHECKED_HOST_LIB_PATH), "build_native() builds them"
	for seed in SEEDS:   # the second seed only once the first has passed
		rc, out = run_checked_corpus(seed, build.CHECKED_LIB_PATH, build.CHECKED_HOST_LIB_PATH, corpus=CHECKED_CORPUS, timeout=600)
		assert rc == 0, "checked build, seed %s: exit %d\n%s" % (seed, rc, out[-6000:])
		assert " passed" in out and "libv2m_hip_checked.so" in out, out[-3000:]
		print(seed, out.strip().splitlines()[-2])
