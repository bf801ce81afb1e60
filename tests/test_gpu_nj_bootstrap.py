"""The bootstrap on the GPU (include/v2m_hip.h, "bootstrap"; csrc/bootstrap_kernels.hpp, csrc/nj_support.hpp) against the model of
tests/nj_bootstrap_model.py, exactly: the weighted pair kernel under explicit weights, the draws through v2m_bootstrap_distances,
v2m_nj_bootstrap against the parent's tree of the model's matrices, the errors of the raw ABI, the driver, and the corpus again on the
checked build."""

import ctypes as C
import io
import os

import numpy as np
import pytest

import nj_bootstrap_model as BM
import nj_tree_model as M
import oracle
import pair_distances_model as PM

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")
PLOIDY_MAX = PM.PLOIDY_MAX
GUARD = 64          # guard elements on either side of a host matrix


@pytest.fixture(scope="module")
def v2m():
	import vcf2multialign_amd as v
	from vcf2multialign_amd import _native as N
	assert (N.PAIR_TILE, N.PAIR_CHUNK_WORDS) == PM.kernel_constants() and (N.BOOT_DRAW_THREADS, N.BOOT_SLICES) == BM.kernel_constants()
	return v


@pytest.fixture(scope="module")
def ctx(v2m):
	c = v2m.Context(0)
	yield c
	c.close()


def upload(v2m, ctx, item):
	ctx.upload_graph(v2m.VariantGraph.from_object(item.g), item.g.ref)
	if item.window:
		ctx.set_column_window(*item.window)


def guarded(ctx, v2m, rows, call):
	"""The host matrix of a raw call between guard elements: call(batch, pointer, info) -> status."""
	from vcf2multialign_amd import _native as N
	n = len(rows)
	buf = np.full(n * n + 2 * GUARD, 0xA5A5A5A5, dtype=np.uint32)
	info = N.PairDistancesInfo()
	batch = v2m.RowBatch(rows)
	rc = call(batch, buf.ctypes.data + 4 * GUARD, info)
	assert rc == N.V2M_OK, ctx._lib.v2m_last_error(ctx._h).decode()
	assert (buf[:GUARD] == 0xA5A5A5A5).all() and (buf[GUARD + n * n:] == 0xA5A5A5A5).all(), "the guard elements"
	return buf[GUARD:GUARD + n * n].reshape(n, n).copy(), info


def weighted(ctx, v2m, rows, w, acgt):
	from vcf2multialign_amd import _native as N
	w = np.ascontiguousarray(w, dtype=np.uint32)
	return guarded(ctx, v2m, rows, lambda batch, dist, info: ctx._lib.v2m_pair_distances_weighted(ctx._h, C.byref(batch.struct), N.DIST_ACGT_ONLY if acgt else 0,
		w.ctypes.data if w.size else None, dist, C.byref(info)))


def replicate(ctx, v2m, rows, seed, r, acgt):
	from vcf2multialign_amd import _native as N
	return guarded(ctx, v2m, rows, lambda batch, dist, info: ctx._lib.v2m_bootstrap_distances(ctx._h, C.byref(batch.struct), N.DIST_ACGT_ONLY if acgt else 0, seed, r, dist, C.byref(info)))


def same_matrix(got, want, what):
	if not np.array_equal(got, want):
		i, j = np.argwhere(got != want)[0]
		raise AssertionError("%s: %d entries differ, the first at [%d][%d]: got %d, expected %d" % (what, int((got != want).sum()), i, j, got[i, j], want[i, j]))


def check_explicit(ctx, v2m, item):
	upload(v2m, ctx, item)
	V, L = int(BM.site_mask(item).sum()), BM._classes(item).shape[1]
	for name, w, K in BM.explicit_patterns(item):
		for acgt in (False, True):
			got, info = weighted(ctx, v2m, item.rows, w, acgt)
			same_matrix(got, BM.expected_weighted(item, w, acgt), "%s %s acgt=%s (K = %d)" % (item.name, name, acgt, K))
			assert (info.n_sites, info.n_columns) == (V, L), (item.name, name)
			if name == "ones":
				same_matrix(got, ctx.pair_distances(item.rows, acgt_only=acgt), "%s: all ones against pair_distances" % item.name)
			if name == "zeros":
				assert not got.any()


# ---- the weighted kernel under explicit weights ------------------------------------------------------------------------------------------------

ROW_ITEMS = [PM.Item("rows_%d" % n, PM.row_count_graph(), PM.row_count_rows(n)) for n in PM.row_counts()]
SITE_ITEMS = [PM.Item("sites_%d" % V, PM.sites_graph_of(V), PM.SITE_ROWS) for V in PM.site_counts()]
WINDOW_ITEMS = [PM.Item("window_%d_%d" % w, PM.window_graph(), PM.SITE_ROWS, w) for w in PM.windows()]


@pytest.mark.parametrize("item", ROW_ITEMS + SITE_ITEMS + WINDOW_ITEMS, ids=repr)
def test_explicit_weights(v2m, ctx, item):
	check_explicit(ctx, v2m, item)


def test_distinct_rows_weighted_and_resampled(v2m, ctx):
	"""Four tiles of rows that all differ (tests/pair_distances_model.py: distinct_items(); the rows of ROW_ITEMS repeat with period 16,
	which hides rows, halves of a tile and tiles taken for one another): the weighted kernel under all ones and under 2^b on site b, and
	one replicate under each definition, every entry held to the model."""
	T, _ = PM.kernel_constants()
	item = PM.distinct_item(3 * T + 1)
	upload(v2m, ctx, item)
	patterns = {name: w for name, w, _ in BM.explicit_patterns(item)}
	for name in ("ones", "powers"):
		for acgt in (False, True):
			got, info = weighted(ctx, v2m, item.rows, patterns[name], acgt)
			same_matrix(got, BM.expected_weighted(item, patterns[name], acgt), "%s %s acgt=%s" % (item.name, name, acgt))
			assert info.n_sites == PM.variable_columns(item.g)
	for seed, r, acgt in ((1, 0, False), (BM.MASK, 1, True)):
		got, _ = replicate(ctx, v2m, item.rows, seed, r, acgt)
		same_matrix(got, BM.expected_replicate(item, seed, r, acgt), "%s seed %d replicate %d acgt=%s" % (item.name, seed, r, acgt))


def test_a_sum_of_two_to_the_32_is_refused(v2m, ctx):
	from vcf2multialign_amd import _native as N
	item = SITE_ITEMS[3]
	upload(v2m, ctx, item)
	L = item.g.aligned_length
	w = np.zeros(L, dtype=np.uint32)
	w[0], w[L - 1] = 0xFFFFFFFF, 1                                      # 2^32 exactly, none of it on a site or all of it: the rule is the sum's
	dist = np.full(len(item.rows) ** 2, 9, dtype=np.uint32)
	batch = v2m.RowBatch(item.rows)
	rc = ctx._lib.v2m_pair_distances_weighted(ctx._h, C.byref(batch.struct), 0, w.ctypes.data, dist.ctypes.data, None)
	assert rc == N.V2M_ERR_INVALID_ARGUMENT and "2^32" in ctx._lib.v2m_last_error(ctx._h).decode() and (dist == 9).all()
	w[L - 1] = 0
	got, _ = weighted(ctx, v2m, item.rows, w, False)
	same_matrix(got, BM.expected_weighted(item, w), "2^32 - 1 on one column")


def _with_env(monkeypatch, **knobs):
	for k, v in knobs.items():
		monkeypatch.setenv(k, str(v))


def test_parts_and_passes_through_the_knobs(v2m, ctx, monkeypatch):
	T, Cw = PM.kernel_constants()
	item = PM.Item("sites_many", PM.sites_graph_of(64 * Cw * 6 + 3), PM.SITE_ROWS)      # seven chunks, the last with three sites
	n_pad = T
	chunk_bytes = Cw * 3 * n_pad * 8
	for knobs, passes in (({"V2M_PAIR_DISTANCES_PARTS": 3}, 1), ({"V2M_PAIR_DISTANCES_PARTS": 1}, 1), ({"V2M_PAIR_DISTANCES_PLANE_BYTES": 4 * chunk_bytes}, 2),
			({"V2M_PAIR_DISTANCES_PLANE_BYTES": 4 * chunk_bytes, "V2M_PAIR_DISTANCES_PARTS": 2}, 2)):      # parts of 3, 3, 1 chunks; one part; passes of 4 and 3 chunks; those in parts of 2, 2 and 2, 1
		with monkeypatch.context() as mp:
			_with_env(mp, **knobs)
			upload(v2m, ctx, item)
			for name, w, K in BM.explicit_patterns(item):
				got, info = weighted(ctx, v2m, item.rows, w, name == "powers")
				same_matrix(got, BM.expected_weighted(item, w, name == "powers"), "%s under %s" % (name, knobs))
				assert info.n_passes == passes, (knobs, info.n_passes)
			got, info = replicate(ctx, v2m, item.rows, 1, 0, False)
			same_matrix(got, BM.expected_replicate(item, 1, 0), "replicate 0 under %s" % (knobs,))


# ---- the draws -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("item", ROW_ITEMS + SITE_ITEMS + WINDOW_ITEMS, ids=repr)
def test_bootstrap_distances(v2m, ctx, item):
	upload(v2m, ctx, item)
	for seed in BM.SEEDS:
		for r in BM.REPLICATES:
			acgt = bool((seed + r) & 1)
			got, info = replicate(ctx, v2m, item.rows, seed, r, acgt)
			same_matrix(got, BM.expected_replicate(item, seed, r, acgt), "%s seed %d replicate %d acgt=%s" % (item.name, seed, r, acgt))
			assert info.n_columns == BM._classes(item).shape[1]


def graph_of_length(L):
	"""A sites_graph cut to a window of exactly L columns by the test: returns (item of the whole graph, window)."""
	g = PM.sites_graph(L // 3 + 2, 7, 31, spacing=3)
	assert g.aligned_length >= L
	return g


@pytest.mark.parametrize("L", BM.draw_lengths())
def test_draw_block_seams(v2m, ctx, L):
	g = graph_of_length(L)
	item = PM.Item("draws_%d" % L, g, PM.SITE_ROWS, (1, 1 + L))
	upload(v2m, ctx, item)
	assert ctx.window_length == L
	for seed, r in ((1, 0), (BM.MASK, (1 << 32) - 1)):
		got, _ = replicate(ctx, v2m, item.rows, seed, r, False)
		same_matrix(got, BM.expected_replicate(item, seed, r), "L = %d seed %d replicate %d" % (L, seed, r))
	assert ctx.bootstrap_distances(item.rows, 1, 0).dtype == np.uint32


def test_a_view_with_no_site(v2m, ctx):
	item = PM.Item("sites_0", PM.sites_graph_of(20), [PLOIDY_MAX] * 3)
	upload(v2m, ctx, item)
	got, info = replicate(ctx, v2m, item.rows, 1, 0, False)
	assert not got.any() and (info.n_sites, info.n_passes) == (0, 0)
	got, info = weighted(ctx, v2m, item.rows, np.full(item.g.aligned_length, 5, dtype=np.uint32), True)
	assert not got.any() and info.n_sites == 0
	nodes, support, trees, info = ctx.nj_bootstrap(item.rows, 4, replicates=True, info=True)
	zero = M.nj(np.zeros((3, 3), dtype=np.uint32))
	assert nodes.tobytes() == zero.tobytes() and support.shape == (0,) and all(t.tobytes() == zero.tobytes() for t in trees)
	four = [PLOIDY_MAX] * 4
	nodes, support = ctx.nj_bootstrap(four, 7)
	assert nodes.tobytes() == M.nj(np.zeros((4, 4), dtype=np.uint32)).tobytes() and support.tolist() == [7]     # every support is B


# ---- v2m_nj_bootstrap --------------------------------------------------------------------------------------------------------------------------

def same_records(got, want, what):
	assert got.dtype == want.dtype and len(got) == len(want), what
	assert got.tobytes() == want.tobytes(), what


@pytest.mark.parametrize("n", BM.tree_row_counts())
def test_nj_bootstrap(v2m, ctx, n):
	from vcf2multialign_amd import host
	item = BM.tree_item(n)
	upload(v2m, ctx, item)
	d, V, L = PM.expected(item.g, item.rows)
	for B in BM.replicates_of(n):
		for seed, acgt in ((1, False), (BM.MASK, True)) if B > 1 or n > 5 else ((1, False),):
			main, trees, counts = BM.bootstrap(item, B, seed, acgt)
			nodes, support, got_trees, info = ctx.nj_bootstrap(item.rows, B, seed=seed, acgt_only=acgt, replicates=True, info=True)
			same_records(nodes, main, "%d rows: the main tree" % n)
			same_records(nodes, ctx.nj_tree(item.rows, acgt_only=acgt), "%d rows: nj_tree" % n)
			assert got_trees.shape == (B, n - 2)
			for r in range(B):
				same_records(got_trees[r], trees[r], "%d rows, seed %d: replicate %d" % (n, seed, r))
			same_records(got_trees[0], host.nj_tree_cpu(BM.expected_replicate(item, seed, 0, acgt)), "the second yardstick")
			assert np.array_equal(support, counts), (n, B, seed, support, counts)
			assert np.array_equal(support, host.nj_split_support(nodes, got_trees))
			assert (info["n_rows"], info["n_sites"], info["n_columns"], info["n_passes"], info["n_pack_passes"], info["n_replicates"]) == (n, V, L, 1, 1, B)
			assert 1 <= info["max_slices"] <= 32 and info["distances_ms"] == info["weights_ms"] == info["pairs_ms"] == info["trees_ms"] == 0.0   # profiling is off
			# without the replicate trees
			nodes2, support2 = ctx.nj_bootstrap(item.rows, B, seed=seed, acgt_only=acgt)
			assert nodes2.tobytes() == nodes.tobytes() and np.array_equal(support2, support)


def test_pack_passes_when_the_budget_is_small(v2m, ctx, monkeypatch):
	T, Cw = PM.kernel_constants()
	n, B = T + 1, 5
	item = PM.Item("passes", PM.sites_graph(64 * Cw * 2 + 5, n, 29), [PLOIDY_MAX] + list(range(n - 1)))     # three chunks of sites, the last nearly empty
	upload(v2m, ctx, item)
	main, trees, counts = BM.bootstrap(item, B, 1)
	nodes, support, got_trees, fit = ctx.nj_bootstrap(item.rows, B, replicates=True, info=True)
	assert (fit["n_passes"], fit["n_pack_passes"]) == (1, 1)
	chunks = (fit["n_sites"] + 64 * Cw - 1) // (64 * Cw)
	assert chunks >= 2
	monkeypatch.setenv("V2M_PAIR_DISTANCES_PLANE_BYTES", str(Cw * 3 * 2 * T * 8))        # one chunk of the two tiles' rows
	nodes2, support2, got_trees2, small = ctx.nj_bootstrap(item.rows, B, replicates=True, info=True)
	assert small["n_passes"] == chunks and small["n_pack_passes"] == B * chunks, small
	assert nodes2.tobytes() == nodes.tobytes() == main.tobytes() and got_trees2.tobytes() == got_trees.tobytes() and np.array_equal(support2, support) and np.array_equal(support, counts)
	assert small["max_slices"] == fit["max_slices"]


def test_stage_times_while_profiling(v2m, ctx):
	item = BM.tree_item(5)
	upload(v2m, ctx, item)
	ctx.profile_enable(True)
	try:
		_, _, info = ctx.nj_bootstrap(item.rows, 3, info=True)
		_, one = ctx.bootstrap_distances(item.rows, 1, 0, info=True)
	finally:
		ctx.profile_enable(False)
		ctx.profile_reset()
	assert min(info["distances_ms"], info["weights_ms"], info["pairs_ms"], info["trees_ms"]) > 0.0 and one["pairs_ms"] > 0.0


def test_the_views_are_left_as_they_were(v2m, ctx):
	item = next(i for i in WINDOW_ITEMS)
	g, rows, w = item.g, item.rows, item.window
	upload(v2m, ctx, PM.Item("whole", g, rows))
	sets = [(2, 30), (41, 47), (3, 4)]
	ctx.set_window_set(sets)
	ctx.set_column_window(*w)
	pieces = ctx.splice_window_set(rows)
	before = ctx.column_counts(rows)
	spliced = ctx.splice_rows(rows)
	main, trees, counts = BM.bootstrap(item, 6, 1)
	nodes, support = ctx.nj_bootstrap(rows, 6)
	same_records(nodes, main, "under a window set and a window")
	assert np.array_equal(support, counts)
	same_matrix(ctx.bootstrap_distances(rows, 1, 2), BM.expected_replicate(item, 1, 2), "bootstrap_distances under a window")
	ones = np.ones(w[1] - w[0], dtype=np.uint32)
	same_matrix(ctx.pair_distances_weighted(rows, ones), PM.expected(g, rows, w)[0], "pair_distances_weighted under a window")
	assert ctx.window_length == w[1] - w[0] and ctx.window_set_size == len(sets)
	for a, b in zip(before, ctx.column_counts(rows)):
		assert np.array_equal(a, b)
	assert ctx.splice_rows(rows) == spliced and ctx.splice_window_set(rows) == pieces


# ---- the raw ABI -----------------------------------------------------------------------------------------------------------------------------------

def test_errors(v2m):
	import torch
	from vcf2multialign_amd import _native as N
	with v2m.Context(0) as c:
		item = SITE_ITEMS[2]
		n, L = len(item.rows), item.g.aligned_length
		batch = v2m.RowBatch(item.rows)
		nodes = np.full(16, 7, dtype=M.NODE_DTYPE)
		support = np.full(16, 7, dtype=np.uint32)
		dist = np.full(n * n, 7, dtype=np.uint32)
		w = np.ones(L, dtype=np.uint32)
		info, binfo = N.PairDistancesInfo(), N.NjBootstrapInfo()
		info.n_columns = binfo.n_columns = 77
		lib = c._lib
		last_error = lambda: lib.v2m_last_error(c._h).decode()
		boot = lambda rows, flags, B, nd=nodes.ctypes.data, sp=support.ctypes.data: lib.v2m_nj_bootstrap(c._h, rows, flags, B, 1, nd, sp, None, C.byref(binfo))
		# no graph
		assert N.V2M_ERR_STATE == lib.v2m_pair_distances_weighted(c._h, C.byref(batch.struct), 0, w.ctypes.data, dist.ctypes.data, None)
		assert N.V2M_ERR_STATE == lib.v2m_bootstrap_distances(c._h, C.byref(batch.struct), 0, 1, 0, dist.ctypes.data, None)
		assert N.V2M_ERR_STATE == boot(C.byref(batch.struct), 0, 3)
		c.upload_graph(v2m.VariantGraph.from_object(item.g), item.g.ref)
		free_before = torch.cuda.mem_get_info()[0]
		# NULL pointers
		assert N.V2M_ERR_INVALID_ARGUMENT == lib.v2m_pair_distances_weighted(c._h, None, 0, w.ctypes.data, dist.ctypes.data, None)
		assert N.V2M_ERR_INVALID_ARGUMENT == lib.v2m_pair_distances_weighted(c._h, C.byref(batch.struct), 0, None, dist.ctypes.data, None) and "weights" in last_error()
		assert N.V2M_ERR_INVALID_ARGUMENT == lib.v2m_pair_distances_weighted(c._h, C.byref(batch.struct), 0, w.ctypes.data, None, None)
		assert N.V2M_ERR_INVALID_ARGUMENT == lib.v2m_bootstrap_distances(c._h, None, 0, 1, 0, dist.ctypes.data, None)
		assert N.V2M_ERR_INVALID_ARGUMENT == lib.v2m_bootstrap_distances(c._h, C.byref(batch.struct), 0, 1, 0, None, None)
		assert N.V2M_ERR_INVALID_ARGUMENT == boot(None, 0, 3)
		assert N.V2M_ERR_INVALID_ARGUMENT == boot(C.byref(batch.struct), 0, 3, nd=None)
		assert N.V2M_ERR_INVALID_ARGUMENT == boot(C.byref(batch.struct), 0, 3, sp=None) and "support" in last_error()
		# flags
		for flags in (0x1, 0x2, 0x4, 0x8, 0x10, 0x40, 0x21, 0x80000000):
			assert N.V2M_ERR_INVALID_ARGUMENT == lib.v2m_pair_distances_weighted(c._h, C.byref(batch.struct), flags, w.ctypes.data, dist.ctypes.data, None) and "v2m_pair_distances_weighted" in last_error()
			assert N.V2M_ERR_INVALID_ARGUMENT == lib.v2m_bootstrap_distances(c._h, C.byref(batch.struct), flags, 1, 0, dist.ctypes.data, None) and "v2m_bootstrap_distances" in last_error()
			assert N.V2M_ERR_INVALID_ARGUMENT == boot(C.byref(batch.struct), flags, 3) and "v2m_nj_bootstrap" in last_error()
		# the replicates' range, and too few rows in v2m_nj_tree's words
		for B in (0, N.NJ_BOOTSTRAP_MAX_REPLICATES + 1, 0xFFFFFFFF):
			assert N.V2M_ERR_INVALID_ARGUMENT == boot(C.byref(batch.struct), 0, B) and str(N.NJ_BOOTSTRAP_MAX_REPLICATES) in last_error()
		for rows in ([0], [0, PLOIDY_MAX]):
			assert N.V2M_ERR_INVALID_ARGUMENT == boot(C.byref(v2m.RowBatch(rows).struct), 0, 3) and "at least 3 taxa" in last_error()
		# no rows: V2M_OK, nothing touched
		empty = v2m.RowBatch([])
		assert N.V2M_OK == boot(C.byref(empty.struct), 0, 3) and binfo.n_columns == 77
		assert N.V2M_OK == lib.v2m_pair_distances_weighted(c._h, C.byref(empty.struct), 0, w.ctypes.data, dist.ctypes.data, C.byref(info)) and info.n_columns == 77
		assert N.V2M_OK == lib.v2m_bootstrap_distances(c._h, C.byref(empty.struct), 0, 1, 0, dist.ctypes.data, C.byref(info)) and info.n_columns == 77
		# too many rows, bad cuts, the sum rule
		many = v2m.RowBatch([0] * (N.PAIR_DISTANCES_MAX_ROWS + 1))
		assert N.V2M_ERR_UNSUPPORTED == boot(C.byref(many.struct), 0, 3) and str(N.NJ_MAX_ROWS) in last_error()
		assert N.V2M_ERR_UNSUPPORTED == lib.v2m_bootstrap_distances(c._h, C.byref(many.struct), 0, 1, 0, dist.ctypes.data, None)
		bad = v2m.RowBatch([0, [(2, 0), (1, 1)], 1])
		assert N.V2M_ERR_PRECONDITION == boot(C.byref(bad.struct), 0, 3)
		assert N.V2M_ERR_PRECONDITION == lib.v2m_bootstrap_distances(c._h, C.byref(bad.struct), 0, 1, 0, dist.ctypes.data, None)
		heavy = w.copy()
		heavy[3] = 0xFFFFFFFF - (L - 1) + 1
		assert N.V2M_ERR_INVALID_ARGUMENT == lib.v2m_pair_distances_weighted(c._h, C.byref(batch.struct), 0, heavy.ctypes.data, dist.ctypes.data, None) and "2^32" in last_error()
		# each before any device work
		assert torch.cuda.mem_get_info()[0] == free_before
		assert (nodes["a"] == 7).all() and (support == 7).all() and (dist == 7).all() and info.n_columns == 77 and binfo.n_columns == 77
		# the Python surface
		got, sup = c.nj_bootstrap([], 3)
		assert got.shape == (0,) and sup.shape == (0,)
		with pytest.raises(Exception):
			c.nj_bootstrap(item.rows, 0)
		with pytest.raises(ValueError):
			c.pair_distances_weighted(item.rows, w[:-1])
		main, trees, counts = BM.bootstrap(item, 4, 1)
		nodes2, sup2 = c.nj_bootstrap(item.rows, 4)
		assert nodes2.tobytes() == main.tobytes() and np.array_equal(sup2, counts)


# ---- the driver --------------------------------------------------------------------------------------------------------------------------------------

def _run(args, cwd=None):
	import subprocess
	assert os.path.exists(CLI), "build the host driver first (__graft_entry__.build())"
	return subprocess.run([CLI] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def texts(g, ids, rows, B, seed, window=None, acgt=False):
	"""(the tree with support, the replicate trees) as the model writes them."""
	item = PM.Item("cli", g, rows, window)
	main, trees, counts = BM.bootstrap(item, B, seed, acgt)
	return BM.newick_support(main, ids, counts), b"".join(M.newick(t, ids) for t in trees)


def test_cli_haplotypes(v2m, ctx, tmp_path):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	g = oracle.build_variant_graph(fa, vcf, "1")
	vg = v2m.VariantGraph.from_object(g)
	ids, rows = PM.haplotype_ids(g)
	assert len(rows) >= 4
	nwk, reps, a2m = tmp_path / "out.nwk", tmp_path / "reps.nwk", tmp_path / "out.fa"
	common = ["-H", "-r", fa, "-a", vcf, "-c", "1"]
	r = _run(common + ["--output-tree=" + str(nwk), "--tree-bootstrap=25", "--output-tree-replicates=" + str(reps), "-s", str(a2m), "--verbose"])
	assert r.returncode == 0, r.stderr.decode()
	want, want_reps = texts(g, ids, rows, 25, 1)
	assert nwk.read_bytes() == want and reps.read_bytes() == want_reps and want_reps.count(b"\n") == 25
	with open(os.path.join(HERE, "golden", "derived", "test-4.haplotypes.a2m"), "rb") as f:
		assert a2m.read_bytes() == f.read()
	assert b"25 replicates, K = " in r.stderr and b"1 pack passes." in r.stderr, r.stderr.decode()
	s, e = 3, min(len(g.ref), 9)
	w = vg.columns_of_reference_range(s - 1, e)
	r = _run(common + ["--output-tree=" + str(nwk), "--tree-bootstrap=7", "--tree-seed=18446744073709551615", "--tree-acgt-only", "--omit-reference", "--region=%d-%d" % (s, e)])
	assert r.returncode == 0, r.stderr.decode()
	assert nwk.read_bytes() == texts(g, ids[1:], rows[1:], 7, BM.MASK, w, True)[0]
	# the Python output class writes the same bytes
	ctx.upload_graph(vg, g.ref)
	stream = io.BytesIO()
	info = v2m.HaplotypeOutput(ctx).output_tree_bootstrap(vg, stream, 25, replicates_path=str(reps))
	assert stream.getvalue() == want and reps.read_bytes() == want_reps and info["n_replicates"] == 25
	stream = io.BytesIO()
	v2m.HaplotypeOutput(ctx, should_output_reference=False, region=(s - 1, e)).output_tree_bootstrap(vg, stream, 7, seed=BM.MASK, acgt_only=True)
	assert stream.getvalue() == texts(g, ids[1:], rows[1:], 7, BM.MASK, w, True)[0] and ctx.window_length == g.aligned_length


def test_cli_founders(v2m, ctx, tmp_path):
	import synth
	from vcf2multialign_amd import host
	g = synth.build_case(tmp_path, 44, 40000, 1200, 6)
	fa, vcf = str(tmp_path / "synth.fa"), str(tmp_path / "synth.vcf")
	nwk, reps, cuts_file = tmp_path / "f.nwk", tmp_path / "f.reps", tmp_path / "cuts"
	r = _run(["-F", "3", "-d", "10", "-r", fa, "-a", vcf, "-c", "1", "--output-tree=" + str(nwk), "--tree-bootstrap=4", "--tree-seed=0", "--output-tree-replicates=" + str(reps), "-t", str(cuts_file), "--verbose"])
	assert r.returncode == 0, r.stderr.decode()
	cuts, _, _ = host.read_cut_positions(cuts_file)
	lines = r.stdout.decode().split("Matchings:\n")[1].splitlines()[:3]
	assigned = [int(x) for line in lines for x in line.split("\t")[1:]]
	n = len(cuts) - 1
	rows = [PLOIDY_MAX] + [list(zip(cuts[:-1], assigned[k * n:(k + 1) * n])) for k in range(3)]
	ids = ["REF", "1", "2", "3"]
	want, want_reps = texts(g, ids, rows, 4, 0)
	assert nwk.read_bytes() == want and reps.read_bytes() == want_reps
	ctx.upload_graph(v2m.VariantGraph.from_object(g), g.ref)
	stream = io.BytesIO()
	v2m.FounderSequenceGreedyOutput(ctx).output_tree_bootstrap(v2m.VariantGraph.from_object(g), cuts, assigned, stream, 4, seed=0)
	assert stream.getvalue() == want


# ---- the checked build -------------------------------------------------------------------------------------------------------------------------------

CHECKED_CORPUS = [
	"tests/test_gpu_nj_bootstrap.py::test_explicit_weights",
	"tests/test_gpu_nj_bootstrap.py::test_distinct_rows_weighted_and_resampled",
	"tests/test_gpu_nj_bootstrap.py::test_parts_and_passes_through_the_knobs",
	"tests/test_gpu_nj_bootstrap.py::test_bootstrap_distances",
	"tests/test_gpu_nj_bootstrap.py::test_draw_block_seams",
	"tests/test_gpu_nj_bootstrap.py::test_a_view_with_no_site",
	"tests/test_gpu_nj_bootstrap.py::test_nj_bootstrap",
	"tests/test_gpu_nj_bootstrap.py::test_pack_passes_when_the_budget_is_small",
	"tests/test_gpu_nj_bootstrap.py::test_the_views_are_left_as_they_were",
]


def test_corpus_on_the_checked_build():
	"""The list above with every LDS object and every scratch buffer (the weights, their slices, the OR word and the replicate's matrix
	among them) poisoned before use (tests/test_gpu_checked_build.py), one run per seed: a slice word, a weight or a matrix element nobody
	wrote in this call changes the result.  No library is preloaded."""
	from test_gpu_checked_build import SEEDS, run_checked_corpus
	from vcf2multialign_amd import build
	assert os.path.exists(build.CHECKED_LIB_PATH) and os.path.exists(build.CHECKED_HOST_LIB_PATH), "build_native() builds them"
	for seed in SEEDS:   # the second seed only once the first has passed
		rc, out = run_checked_corpus(seed, build.CHECKED_LIB_PATH, build.CHECKED_HOST_LIB_PATH, corpus=CHECKED_CORPUS, timeout=600)
		assert rc == 0, "checked build, seed %s: exit %d\n%s" % (seed, rc, out[-6000:])
		assert " passed" in out and "libv2m_hip_checked.so" in out, out[-3000:]
		print(seed, out.strip().splitlines()[-2])
