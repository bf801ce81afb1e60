"""Parsimony on a tree on the GPU (include/v2m_hip.h, "parsimony"; csrc/parsimony_kernels.hpp) against the numpy model of
tests/tree_parsimony_model.py, byte for byte: every corpus item through v2m_parsimony_of_sites from a guarded upload with a capacity of
0, the exact one and one short; the graph items of tests/variable_sites_model.py through v2m_tree_parsimony on the tree v2m_nj_tree
builds of the same rows, whole and in three site ranges, under both row groupings of the gather; the errors of the raw ABI; the driver;
and the corpus again on the checked build."""

import ctypes as C
import io
import os

import numpy as np
import pytest

import nj_tree_model as NJ
import oracle
import pair_distances_model as PM
import tree_parsimony_model as M
import variable_sites_model as VM

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")
PLOIDY_MAX = PM.PLOIDY_MAX
GUARD_ROWS = 2
FILL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def v2m():
	import vcf2multialign_amd as v
	from vcf2multialign_amd import _native as N
	assert (N.FITCH_SITES, N.FITCH_THREADS, N.FITCH_BATCH) == M.kernel_constants()
	assert np.dtype(N.PARSIMONY_SITE_DTYPE) == M.SITE_DTYPE and np.dtype(N.TREE_SITE_DTYPE) == M.TREE_SITE_DTYPE and np.dtype(N.TREE_MUTATION_DTYPE) == M.MUTATION_DTYPE
	return v


@pytest.fixture(scope="module")
def ctx(v2m):
	c = v2m.Context(0)
	yield c
	c.close()


def upload(v2m, ctx, g):
	ctx.upload_graph(v2m.VariantGraph.from_object(g), g.ref)


class GuardedBytes:
	"""m in a device buffer u8[GUARD_ROWS + n + GUARD_ROWS][pitch], pitch > V: the bytes behind the sites and the guard rows hold
	letters of both cases and everything else, which no result may depend on."""

	def __init__(self, m):
		import torch
		n, V = m.shape
		self.n, self.V, self.pitch = n, V, (V + 15) // 16 * 16 + 16 * (1 + n % 2)
		rng = np.random.default_rng(n * 1000 + V)
		hostile = np.frombuffer(b"ACGTacgtN-" + bytes([1, 0xFF]), dtype=np.uint8)
		host = hostile[rng.integers(0, len(hostile), size=(n + 2 * GUARD_ROWS, self.pitch))]
		host[GUARD_ROWS:GUARD_ROWS + n, :V] = m
		self.host = np.ascontiguousarray(host)
		self.device = torch.from_numpy(self.host.copy()).cuda()
		self.ptr = self.device.data_ptr() + GUARD_ROWS * self.pitch
		assert self.ptr % 16 == 0 and self.pitch % 16 == 0 and self.pitch > V

	def unchanged(self):
		return np.array_equal(self.device.cpu().numpy(), self.host)


class Filled:
	"""A device buffer of `count` records of `dtype` between two guards of 64 bytes, all filled with FILL."""

	def __init__(self, count, dtype):
		import torch
		self.count, self.dtype = count, np.dtype(dtype)
		self.words = 32 + max(1, count) * self.dtype.itemsize // 4
		self.device = torch.full((self.words,), FILL, dtype=torch.int32, device="cuda")
		self.ptr = self.device.data_ptr() + 64
		assert self.ptr % 16 == 0

	def records(self):
		raw = self.device.cpu().numpy().view(np.uint32)
		assert (raw[:16] == FILL).all() and (raw[16 + self.count * self.dtype.itemsize // 4:] == FILL).all(), "written outside the records"
		return raw[16:16 + self.count * self.dtype.itemsize // 4].view(self.dtype)

	def untouched(self):
		return bool((self.device.cpu().numpy().view(np.uint32) == FILL).all())


def same_records(got, want, what):
	assert got.dtype == want.dtype and len(got) == len(want), (what, got.dtype, want.dtype, len(got), len(want))
	if got.tobytes() != want.tobytes():
		k = next(i for i in range(len(got)) if got[i:i + 1].tobytes() != want[i:i + 1].tobytes())
		raise AssertionError("%s: the first difference at record %d of %d: got %s, expected %s" % (what, k, len(got), got[k], want[k]))


def check_item(v2m, ctx, item):
	from vcf2multialign_amd import _native as N
	want_sites, want_branches, want_mutations = M.expected(item.name)
	total = len(want_mutations)
	data = GuardedBytes(item.m)
	modes = [("none", 0), ("exact", total)] + ([("short", total - 1)] if total >= 2 else [])
	for mode, capacity in modes:
		sites, branches, mutations = Filled(item.V, M.SITE_DTYPE), Filled(2 * item.n - 3, np.uint32), Filled(capacity, M.MUTATION_DTYPE)
		call = lambda: ctx.parsimony_of_sites(data.ptr, item.n, item.V, data.pitch, item.nodes, sites.ptr, branches.ptr, mutations.ptr if capacity else None, capacity)
		what = "%s, capacity %s" % (item.name, mode)
		if mode == "short":
			with pytest.raises(v2m.V2MError) as failure:
				call()
			assert failure.value.code == N.V2M_ERR_INVALID_ARGUMENT and str(total) in str(failure.value), failure.value
			assert ctx.parsimony_mutations == total and mutations.untouched() and branches.untouched(), what
		else:
			assert call() == total, what
			same_records(branches.records(), want_branches, what + ": branch changes")
			if capacity:
				same_records(mutations.records(), want_mutations, what + ": mutations")
		same_records(sites.records(), want_sites, what + ": sites")
	assert data.unchanged(), item.name + ": the input bytes"


# ---- the device form --------------------------------------------------------------------------------------------------------------------

CORPUS = M.corpus()


@pytest.mark.parametrize("item", CORPUS, ids=[i.name for i in CORPUS])
def test_device_form(v2m, ctx, item):
	check_item(v2m, ctx, item)


def test_no_site_and_an_exact_pitch(v2m, ctx):
	item = next(i for i in CORPUS if i.name == "taxa_9")
	data = GuardedBytes(item.m)
	branches = Filled(2 * item.n - 3, np.uint32)
	assert 0 == ctx.parsimony_of_sites(data.ptr, item.n, 0, data.pitch, item.nodes, None, branches.ptr)
	assert not branches.records().any()
	# pitch == V: nothing behind the sites
	import torch
	exact = next(i for i in CORPUS if i.V % 16 == 0)
	device = torch.from_numpy(np.ascontiguousarray(exact.m).copy()).cuda()
	sites, branches = Filled(exact.V, M.SITE_DTYPE), Filled(2 * exact.n - 3, np.uint32)
	want = M.expected(exact.name)
	assert len(want[2]) == ctx.parsimony_of_sites(device.data_ptr(), exact.n, exact.V, exact.V, exact.nodes, sites.ptr, branches.ptr)
	same_records(sites.records(), want[0], "exact pitch: sites")
	same_records(branches.records(), want[1], "exact pitch: branch changes")


def test_stage_times_while_profiling(v2m, ctx):
	item = next(i for i in VM.corpus() if i.name == "cuts")
	upload(v2m, ctx, item.g)
	nodes = ctx.nj_tree(item.rows)
	ctx.profile_enable(True)
	try:
		*_, info = ctx.tree_parsimony(item.rows, nodes, info=True)
	finally:
		ctx.profile_enable(False)
		ctx.profile_reset()
	assert info["counts_ms"] > 0.0 and info["gather_ms"] > 0.0 and info["parsimony_ms"] > 0.0


# ---- from rows --------------------------------------------------------------------------------------------------------------------------

GRAPH_ITEMS = M.graph_items()
_expected_of_rows = {}


def expected_of_rows(item, nodes):
	"""The model's results for a graph item on the tree `nodes`: computed once per item and tree, shared, read-only."""
	key = (item.name, nodes.tobytes())
	if key not in _expected_of_rows:
		out = M.expected_of_rows(item.g, item.rows, nodes, item.window)
		for a in out[:3]:
			a.setflags(write=False)
		_expected_of_rows[key] = out
	return _expected_of_rows[key]


def check_graph_item(v2m, ctx, item, ranges=None):
	upload(v2m, ctx, item.g)
	if item.window:
		ctx.set_column_window(*item.window)
	nodes = ctx.nj_tree(item.rows)
	want_sites, want_branches, want_mutations, L = expected_of_rows(item, nodes)
	sites, branches, mutations, info = ctx.tree_parsimony(item.rows, nodes, info=True)
	same_records(sites, want_sites, item.name + ": sites")
	same_records(branches, want_branches, item.name + ": branch changes")
	same_records(mutations, want_mutations, item.name + ": mutations")
	V = len(want_sites)
	assert (info["n_sites"], info["n_columns"], info["n_mutations"]) == (V, L, len(want_mutations)), (item.name, info)
	assert info["n_ranges"] == (ranges if ranges is not None else 1 if V else 0), (item.name, info)
	assert info["counts_ms"] == info["gather_ms"] == info["parsimony_ms"] == 0.0                 # profiling is off
	assert sum(ctx.tree_parsimony_blocks) == len(want_mutations) and len(ctx.tree_parsimony_blocks) <= max(1, info["n_ranges"])
	return info


@pytest.mark.parametrize("item", GRAPH_ITEMS, ids=[i.name for i in GRAPH_ITEMS])
def test_graph_items(v2m, ctx, item):
	check_graph_item(v2m, ctx, item)


def test_graph_items_cover_the_forms():
	assert any(i.window for i in GRAPH_ITEMS) and any(not i.window for i in GRAPH_ITEMS)
	assert any(isinstance(r, (list, tuple)) for i in GRAPH_ITEMS for r in i.rows), "rows with cuts"
	assert any(len(set(r for r in i.rows if not isinstance(r, (list, tuple)))) < len([r for r in i.rows if not isinstance(r, (list, tuple))]) for i in GRAPH_ITEMS), "repeated rows"


def three_range_item():
	"""(item, bytes): the graph item with the most SNP sites and the budget that cuts them into three ranges, the last one ragged."""
	S, _, _ = M.kernel_constants()
	unit = 64 * S
	item = max(GRAPH_ITEMS, key=lambda i: len(VM.expected(i.g, i.rows, i.window, snp_only=True)[0]))
	V, n = len(VM.expected(item.g, item.rows, item.window, snp_only=True)[0]), len(item.rows)
	k = -(-V // (3 * unit))
	assert 2 * unit * k < V <= 3 * unit * k and V % (unit * k), (V, k)
	return item, unit * k * (2 * n - 2) + (2 * n - 2) * unit // 2


def test_three_ranges(v2m, ctx, monkeypatch):
	item, budget = three_range_item()
	monkeypatch.setenv("V2M_PARSIMONY_BYTES", str(budget))
	check_graph_item(v2m, ctx, item, ranges=3)
	assert len(ctx.tree_parsimony_blocks) >= 2
	# a budget below one wave of sites still takes a wave at a time
	monkeypatch.setenv("V2M_PARSIMONY_BYTES", "1")
	V = len(VM.expected(item.g, item.rows, item.window, snp_only=True)[0])
	check_graph_item(v2m, ctx, item, ranges=-(-V // (64 * M.kernel_constants()[0])))


@pytest.mark.parametrize("item", GRAPH_ITEMS, ids=[i.name for i in GRAPH_ITEMS])
def test_graph_items_in_row_groups_of_five(v2m, ctx, monkeypatch, item):
	monkeypatch.setenv("V2M_SITE_ROWS_PER_GROUP", "5")
	check_graph_item(v2m, ctx, item)


def test_three_ranges_in_row_groups_of_five(v2m, ctx, monkeypatch):
	item, budget = three_range_item()
	monkeypatch.setenv("V2M_SITE_ROWS_PER_GROUP", "5")
	monkeypatch.setenv("V2M_PARSIMONY_BYTES", str(budget))
	check_graph_item(v2m, ctx, item, ranges=3)


def test_sinks_may_be_null_and_may_abort(v2m, ctx):
	from vcf2multialign_amd import _native as N
	item = next(i for i in GRAPH_ITEMS if i.name == "cuts")
	upload(v2m, ctx, item.g)
	nodes = ctx.nj_tree(item.rows)
	want_sites, want_branches, want_mutations, _ = expected_of_rows(item, nodes)
	sites, branches, mutations = ctx.tree_parsimony(item.rows, nodes, want_sites=False)
	assert len(sites) == 0
	same_records(mutations, want_mutations, "without a sites sink")
	sites, branches, mutations = ctx.tree_parsimony(item.rows, nodes, want_mutations=False, want_branch_changes=False)
	assert len(mutations) == 0 and len(branches) == 0
	same_records(sites, want_sites, "without a mutations sink")
	batch = v2m.RowBatch(item.rows)
	abort = N.TREE_SINK_FN(lambda user, records, count: 1)
	none = C.cast(None, N.TREE_SINK_FN)
	for sinks in ((abort, none), (none, abort)):
		assert N.V2M_ERR_SINK == ctx._lib.v2m_tree_parsimony(ctx._h, C.byref(batch.struct), nodes.ctypes.data, 0, None, sinks[0], sinks[1], None, None)
	same_records(ctx.tree_parsimony(item.rows, nodes)[1], want_branches, "after the aborts")


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
	nodes = ctx.nj_tree(rows)
	same_records(ctx.tree_parsimony(rows, nodes)[2], expected_of_rows(item, nodes)[2], "under a window set and a window")
	assert ctx.window_length == w[1] - w[0] and ctx.window_set_size == len(sets)
	for a, b in zip(before, ctx.column_counts(rows)):
		assert np.array_equal(a, b)
	assert ctx.splice_rows(rows) == spliced and ctx.splice_window_set(rows) == pieces


# ---- the raw ABI ------------------------------------------------------------------------------------------------------------------------

def test_errors(v2m):
	import torch
	from test_tree_parsimony_host import bad_records
	from vcf2multialign_amd import _native as N
	with v2m.Context(0) as c:
		item = next(i for i in CORPUS if i.name == "taxa_9")
		data = GuardedBytes(item.m)
		sites, branches, mutations = Filled(item.V, M.SITE_DTYPE), Filled(2 * item.n - 3, np.uint32), Filled(8, M.MUTATION_DTYPE)
		of_sites, of_rows = c._lib.v2m_parsimony_of_sites, c._lib.v2m_tree_parsimony
		last_error = lambda: c._lib.v2m_last_error(c._h).decode()
		total = C.c_uint64(77)
		nodes = item.nodes.copy()
		args = lambda n=item.n, V=item.V, pitch=data.pitch, nd=nodes, b=data.ptr, s=sites.ptr, br=branches.ptr, mu=None, cap=0: (c._h, b, n, V, pitch, nd.ctypes.data if nd is not None else None,
			s, br, mu, cap, C.byref(total))
		# n = 0: V2M_OK, nothing touched; n = 1 and n = 2: no tree
		assert N.V2M_OK == of_sites(*args(n=0)) and total.value == 77
		for n in (1, 2):
			assert N.V2M_ERR_INVALID_ARGUMENT == of_sites(*args(n=n)) and "at least 3 taxa" in last_error()
		# more taxa than the limit: refused before anything is allocated or read
		free_before = torch.cuda.mem_get_info()[0]
		assert N.V2M_ERR_UNSUPPORTED == of_sites(*args(n=N.NJ_MAX_ROWS + 1)) and str(N.NJ_MAX_ROWS) in last_error()
		assert torch.cuda.mem_get_info()[0] == free_before
		# NULL pointers, misalignment, a bad pitch, a capacity without a list
		assert N.V2M_ERR_INVALID_ARGUMENT == c._lib.v2m_parsimony_of_sites(c._h, data.ptr, item.n, item.V, data.pitch, nodes.ctypes.data, sites.ptr, branches.ptr, None, 0, None)
		for kw in (dict(nd=None), dict(b=None), dict(s=None), dict(br=None), dict(cap=3)):
			assert N.V2M_ERR_INVALID_ARGUMENT == of_sites(*args(**kw)), kw
		for kw in (dict(b=data.ptr + 4), dict(s=sites.ptr + 8), dict(br=branches.ptr + 4), dict(mu=mutations.ptr + 8, cap=8)):
			assert N.V2M_ERR_INVALID_ARGUMENT == of_sites(*args(**kw)) and "16-byte aligned" in last_error(), kw
		for pitch in (item.V - 1, data.pitch + 8, 16):
			assert N.V2M_ERR_INVALID_ARGUMENT == of_sites(*args(pitch=pitch)) and "pitch" in last_error()
		# records that are no tree, in every form
		for what, bad, n in bad_records():
			assert n == item.n
			assert N.V2M_ERR_INVALID_ARGUMENT == of_sites(*args(nd=bad)) and "v2m_parsimony_of_sites" in last_error(), what
		assert total.value == 77 and sites.untouched() and branches.untouched() and mutations.untouched() and data.unchanged()
		# the device form needs no graph
		assert N.V2M_OK == of_sites(*args()) and total.value == len(M.expected(item.name)[2])
		same_records(sites.records(), M.expected(item.name)[0], "without a graph")
		# from rows: no graph, then NULL rows and nodes, flags, too few and too many rows, bad records, bad cuts
		graph_item = next(i for i in GRAPH_ITEMS if i.name == "sites_64")
		batch = v2m.RowBatch(graph_item.rows)
		n = len(graph_item.rows)
		tree = M.tree("joins", n, 3)
		info = N.TreeParsimonyInfo()
		info.n_columns = 77
		none = C.cast(None, N.TREE_SINK_FN)
		rows_args = lambda b=batch, nd=tree, flags=0: (c._h, C.byref(b.struct) if b is not None else None, nd.ctypes.data if nd is not None else None, flags, None, none, none, None, C.byref(info))
		assert N.V2M_ERR_STATE == of_rows(*rows_args())
		upload(v2m, c, graph_item.g)
		assert N.V2M_ERR_INVALID_ARGUMENT == of_rows(*rows_args(b=None))
		assert N.V2M_ERR_INVALID_ARGUMENT == of_rows(*rows_args(nd=None))
		for flags in (0x1, 0x20, 0x40, 0x80000000):
			assert N.V2M_ERR_INVALID_ARGUMENT == of_rows(*rows_args(flags=flags)) and "v2m_tree_parsimony" in last_error()
		assert N.V2M_OK == of_rows(*rows_args(b=v2m.RowBatch([]))) and info.n_columns == 77
		for rows in ([0], [0, PLOIDY_MAX]):
			assert N.V2M_ERR_INVALID_ARGUMENT == of_rows(*rows_args(b=v2m.RowBatch(rows))) and "at least 3 taxa" in last_error()
		many = v2m.RowBatch([0] * (N.NJ_MAX_ROWS + 1))
		assert N.V2M_ERR_UNSUPPORTED == of_rows(*rows_args(b=many)) and str(N.NJ_MAX_ROWS) in last_error()
		assert N.V2M_ERR_INVALID_ARGUMENT == of_rows(*rows_args(nd=M.tree("joins", n, 3)[::-1].copy()))
		bad = v2m.RowBatch([0, [(2, 0), (1, 1)], 1])
		assert N.V2M_ERR_PRECONDITION == of_rows(*rows_args(b=bad, nd=M.spine(3)))
		assert info.n_columns == 77
		# the Python surface: no rows give nothing
		got = c.tree_parsimony([], np.zeros(0, dtype=M.NODE_DTYPE), info=True)
		assert [len(x) for x in got[:3]] == [0, 0, 0] and got[3]["n_columns"] == graph_item.g.aligned_length
		# any tree of the rows is taken, not only the neighbour-joining one
		want = M.expected_of_rows(graph_item.g, graph_item.rows, tree)
		got = c.tree_parsimony(graph_item.rows, tree)
		for g_, w_, what in zip(got, want, ("sites", "branch changes", "mutations")):
			same_records(g_, w_, "a tree that is no neighbour joining: " + what)


# ---- the driver -------------------------------------------------------------------------------------------------------------------------

def _run(args, cwd=None):
	import subprocess
	assert os.path.exists(CLI), "build the host driver first (__graft_entry__.build())"
	return subprocess.run([CLI] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def test_cli_haplotypes(v2m, ctx, tmp_path):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	g = oracle.build_variant_graph(fa, vcf, "1")
	vg = v2m.VariantGraph.from_object(g)
	ids, rows = PM.haplotype_ids(g)
	nodes = NJ.nj(PM.expected(g, rows)[0])
	sites, branches, mutations, L = M.expected_of_rows(g, rows, nodes)
	assert len(sites) and len(mutations)
	want = (M.newick(nodes, ids, branches), M.mutations_text(g, mutations, sites, ids), M.sites_text(g, sites))
	nwk, pars, muts, tsv = (tmp_path / name for name in ("out.nwk", "out.pars.nwk", "out.mutations.tsv", "out.sites.tsv"))
	common = ["-H", "-r", fa, "-a", vcf, "-c", "1", "--output-tree=" + str(nwk)]
	flags = ["--output-tree-parsimony=" + str(pars), "--output-tree-mutations=" + str(muts), "--output-tree-sites=" + str(tsv)]
	r = _run(common + flags + ["--verbose"])
	assert r.returncode == 0, r.stderr.decode()
	assert (pars.read_bytes(), muts.read_bytes(), tsv.read_bytes()) == want
	assert ("Parsimony: %d rows, %d columns, %d sites, %d mutations, 1 ranges." % (len(rows), L, len(sites), len(mutations))).encode() in r.stderr, r.stderr.decode()
	# one flag alone; the same tree under a bootstrap
	for f in (pars, muts, tsv):
		f.unlink()
	r = _run(common + flags[1:2] + ["--tree-bootstrap=3"])
	assert r.returncode == 0, r.stderr.decode()
	assert muts.read_bytes() == want[1] and not pars.exists() and not tsv.exists()
	# Output.output_tree_parsimony writes the same bytes
	upload(v2m, ctx, g)
	streams = [io.BytesIO() for _ in range(3)]
	info = v2m.HaplotypeOutput(ctx).output_tree_parsimony(vg, *streams)
	assert tuple(s.getvalue() for s in streams) == want and info["n_mutations"] == len(mutations)
	stream = io.BytesIO()
	v2m.HaplotypeOutput(ctx).output_tree_parsimony(vg, parsimony=stream, bootstrap=2)
	assert stream.getvalue() == want[0]


# ---- the checked build ------------------------------------------------------------------------------------------------------------------

CHECKED_CORPUS = [
	"tests/test_gpu_tree_parsimony.py::test_device_form",
	"tests/test_gpu_tree_parsimony.py::test_no_site_and_an_exact_pitch",
	"tests/test_gpu_tree_parsimony.py::test_three_ranges",
]


def test_corpus_on_the_checked_build():
	"""The device-form corpus with every LDS object and every scratch buffer (the sets, the workgroups' steps, the totals, the branch
	counters and the lists among them) poisoned before use (tests/test_gpu_checked_build.py), one child process per seed: a set, an
	offset or a counter nobody wrote in this call changes the result.  No library is preloaded."""
	from test_gpu_checked_build import SEEDS, run_checked_corpus
	from vcf2multialign_amd import build
	assert os.path.exists(build.CHECKED_LIB_PATH) and os.path.exists(build.CHECKED_HOST_LIB_PATH), "build_native() builds them"
	for seed in SEEDS:   # the second seed only once the first has passed
		rc, out = run_checked_corpus(seed, build.CHECKED_LIB_PATH, build.CHECKED_HOST_LIB_PATH, corpus=CHECKED_CORPUS, timeout=600)
		assert rc == 0, "checked build, seed %s: exit %d\n%s" % (seed, rc, out[-6000:])
		assert " passed" in out and "libv2m_hip_checked.so" in out, out[-3000:]
		print(seed, out.strip().splitlines()[-2])
