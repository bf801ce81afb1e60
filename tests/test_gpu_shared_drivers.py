"""What the analyses' host forms share (v2m_hip.hip: in_turn, copy_to_slot, drain) at its seams: v2m_variable_sites with a rows sink,
v2m_site_ld with a pairs sink and v2m_tree_parsimony with a mutations sink, cut by their knobs into exactly two and three units --
three is the smallest count at which buffer k & 1 is taken again while unit k - 1 is still crossing the link -- and with a sink that
aborts at the first, the second and the last of three units: the call returns V2M_ERR_SINK with both streams left idle, and the same
call on the same context then gives the model's result.  The abort cases also run on the checked build.

One graph of 600 sites under 17 rows serves all three calls.  The counts this file does not take are asserted elsewhere: one unit by
every corpus item of tests/test_gpu_variable_sites.py, test_gpu_site_ld.py and test_gpu_tree_parsimony.py (check_forms, check_item,
check_graph_item), two ranges of site LD by test_gpu_site_ld.py::test_emit_ranges, three ranges of parsimony by
test_gpu_tree_parsimony.py::test_three_ranges."""

import ctypes as C
import functools
import os

import numpy as np
import pytest

import site_ld_model as LM
import tree_parsimony_model as TM
import variable_sites_model as VM

pytestmark = pytest.mark.gpu

N_SITES = 600
LD_PARAMS = LM.Params(window_sites=6)


@pytest.fixture(scope="module")
def v2m():
	import vcf2multialign_amd as v
	return v


@pytest.fixture(scope="module")
def ctx(v2m):
	c = v2m.Context(0)
	g, _ = case()
	c.upload_graph(v2m.VariantGraph.from_object(g), g.ref)
	yield c
	c.close()


@functools.lru_cache(maxsize=None)
def case():
	"""(graph, rows): 600 biallelic sites a base apart under the 12 copies, the reference, a repeated row and three rows with cuts."""
	g = LM.random_graph(N_SITES, seed=7)
	rows = LM.all_rows(g)
	assert len(rows) == 17
	return g, rows


def read_only(*arrays):
	for a in arrays:
		a.setflags(write=False)
	return arrays


# ---- the three calls, each with a sink that counts its units and may abort at one ---------------------------------------------------------

class Units:
	"""The units a sink received, and the one at which it returns non-zero (None: never)."""

	def __init__(self, abort_at=None):
		self.abort_at, self.got = abort_at, []

	def take(self, unit):
		self.got.append(unit)
		return 1 if len(self.got) - 1 == self.abort_at else 0


def variable_sites_call(v2m, ctx, abort_at=None):
	"""(status, blocks as (first_row, n_rows), bytes u8[n, V])"""
	from vcf2multialign_amd import _native as N
	_, rows = case()
	units = Units(abort_at)

	def sink(_user, first_row, n_rows, data, pitch, n_sites):
		a = np.frombuffer(C.string_at(data, (n_rows - 1) * pitch + n_sites), dtype=np.uint8)
		return units.take((int(first_row), np.lib.stride_tricks.as_strided(a, shape=(n_rows, n_sites), strides=(pitch, 1)).copy()))

	batch = v2m.RowBatch(rows)
	rc = ctx._lib.v2m_variable_sites(ctx._h, C.byref(batch.struct), 0, C.cast(None, N.SITE_COLUMNS_SINK_FN), N.SITE_ROWS_SINK_FN(sink), None, None)
	return rc, [(first, len(a)) for first, a in units.got], np.concatenate([a for _, a in units.got])


def site_ld_call(v2m, ctx, abort_at=None):
	"""(status, block sizes, pairs)"""
	from vcf2multialign_amd import _native as N
	_, rows = case()
	units = Units(abort_at)

	def sink(_user, records, count):
		return units.take(np.frombuffer(C.string_at(records, 24 * count), dtype=np.dtype(N.LD_PAIR_DTYPE)).copy())

	batch = v2m.RowBatch(rows)
	params = ctx._site_ld_params(**LD_PARAMS.kwargs())
	rc = ctx._lib.v2m_site_ld(ctx._h, C.byref(batch.struct), C.byref(params), C.cast(None, N.LD_SINK_FN), N.LD_SINK_FN(sink), None, None)
	return rc, [len(b) for b in units.got], np.concatenate(units.got)


def tree_parsimony_call(v2m, ctx, abort_at=None):
	"""(status, block sizes, mutations, branch changes)"""
	from vcf2multialign_amd import _native as N
	_, rows = case()
	units = Units(abort_at)

	def sink(_user, records, count):
		return units.take(np.frombuffer(C.string_at(records, 16 * count), dtype=np.dtype(N.TREE_MUTATION_DTYPE)).copy())

	batch = v2m.RowBatch(rows)
	nodes = np.ascontiguousarray(tree(ctx), dtype=np.dtype(N.NJ_NODE_DTYPE))
	branches = np.zeros(2 * len(rows) - 3, dtype=np.uint32)
	rc = ctx._lib.v2m_tree_parsimony(ctx._h, C.byref(batch.struct), nodes.ctypes.data, 0, branches.ctypes.data, C.cast(None, N.TREE_SINK_FN), N.TREE_SINK_FN(sink), None, None)
	return rc, [len(b) for b in units.got], np.concatenate(units.got), branches


# ---- the model's results, computed once ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def expected_bytes():
	g, rows = case()
	columns, data, _ = VM.expected(g, rows)
	assert len(columns) == N_SITES
	return read_only(data)[0]


@functools.lru_cache(maxsize=None)
def expected_pairs():
	g, rows = case()
	_, pairs, _, _ = LM.expected(LM.Item("drivers", g, rows, LD_PARAMS, arrays=True))
	return read_only(pairs)[0]


_tree = []


def tree(ctx):
	"""The rows' neighbour-joining tree, made once (on the GPU: the tree is input here, tests/test_gpu_nj_tree.py checks it)."""
	if not _tree:
		_tree.append(read_only(ctx.nj_tree(case()[1]))[0])
	return _tree[0]


_parsimony = []


def expected_parsimony(ctx):
	if not _parsimony:
		g, rows = case()
		sites, branches, mutations, _ = TM.expected_of_rows(g, rows, tree(ctx))
		assert len(sites) == N_SITES
		_parsimony.append(read_only(branches, mutations))
	return _parsimony[0]


# ---- the knobs that cut a call into k units --------------------------------------------------------------------------------------------------

def slices_of(k):
	"""The (first_row, n_rows) of k row slices of the 17 rows."""
	n = len(case()[1])
	per = -(-n // k)
	return [(r, min(per, n - r)) for r in range(0, n, per)]


def set_row_slices(ctx, monkeypatch, k):
	pitch = int(ctx.min_row_pitch)
	monkeypatch.setenv("V2M_RING_SLOT_BYTES", str(slices_of(k)[0][1] * pitch + pitch // 2))


def ld_ranges_of(per_strip, block_pairs):
	"""site_ld_run's ranges: whole strips while their pairs fit the block, at least one strip, a range without a pair passed over."""
	out, i = [], 0
	while i < len(per_strip):
		j, count = i + 1, per_strip[i]
		while j < len(per_strip) and count + per_strip[j] <= block_pairs:
			count += per_strip[j]
			j += 1
		if count:
			out.append(count)
		i = j
	return out


@functools.lru_cache(maxsize=None)
def ld_block_pairs(k):
	"""(the least block size in pairs that gives exactly k ranges, the ranges' sizes)"""
	T, _ = LM.kernel_constants()
	pairs = expected_pairs()
	per_strip = [int(c) for c in np.bincount(pairs["site_a"] // T, minlength=-(-N_SITES // T))]
	assert sum(1 for c in per_strip if c) >= 3, per_strip
	for block_pairs in range(max(per_strip), len(pairs) + 1):
		ranges = ld_ranges_of(per_strip, block_pairs)
		if len(ranges) == k:
			return block_pairs, ranges
	raise AssertionError("no block size gives %d ranges of %s" % (k, per_strip))


def set_ld_ranges(monkeypatch, k):
	block_pairs, ranges = ld_block_pairs(k)
	monkeypatch.setenv("V2M_SITE_LD_BLOCK_BYTES", str(24 * block_pairs + 23))   # (a record short of one more pair)
	return ranges


def set_parsimony_ranges(monkeypatch, k):
	"""Ranges of whole waves of 64 S sites: 3 waves in k = 2 ranges of (2, 1) waves or k = 3 ranges of a wave."""
	S, _, _ = TM.kernel_constants()
	wave, n = 64 * S, len(case()[1])
	assert 2 * wave < N_SITES <= 3 * wave and k in (2, 3)
	waves = {2: 2, 3: 1}[k]
	monkeypatch.setenv("V2M_PARSIMONY_BYTES", str(waves * wave * (2 * n - 2) + (2 * n - 2) * wave // 2))
	return [min(N_SITES, s + waves * wave) - s for s in range(0, N_SITES, waves * wave)]


def mutations_per_range(ctx, range_sites):
	_, mutations = expected_parsimony(ctx)
	edges = np.r_[0, np.cumsum(range_sites)]
	return [int(((mutations["site"] >= a) & (mutations["site"] < b)).sum()) for a, b in zip(edges[:-1], edges[1:])]


# ---- the overlapped driver at two and three units ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", (2, 3))
def test_variable_sites_in_k_slices(v2m, ctx, monkeypatch, k):
	from vcf2multialign_amd import _native as N
	set_row_slices(ctx, monkeypatch, k)
	rc, blocks, data = variable_sites_call(v2m, ctx)
	assert rc == N.V2M_OK and blocks == slices_of(k) and len(blocks) == k, (rc, blocks)
	assert np.array_equal(data, expected_bytes())


def test_site_ld_in_three_ranges(v2m, ctx, monkeypatch):
	from vcf2multialign_amd import _native as N
	ranges = set_ld_ranges(monkeypatch, 3)
	rc, blocks, pairs = site_ld_call(v2m, ctx)
	assert rc == N.V2M_OK and blocks == ranges and len(blocks) == 3, (rc, blocks, ranges)
	assert np.array_equal(pairs, expected_pairs())


def test_tree_parsimony_in_two_ranges(v2m, ctx, monkeypatch):
	from vcf2multialign_amd import _native as N
	want_branches, want_mutations = expected_parsimony(ctx)
	want_blocks = mutations_per_range(ctx, set_parsimony_ranges(monkeypatch, 2))
	assert len(want_blocks) == 2 and all(want_blocks), want_blocks
	rc, blocks, mutations, branches = tree_parsimony_call(v2m, ctx)
	assert rc == N.V2M_OK and blocks == want_blocks, (rc, blocks, want_blocks)
	assert mutations.tobytes() == want_mutations.tobytes() and np.array_equal(branches, want_branches)


# ---- a sink that aborts at unit 0, 1 and 2 of three ----------------------------------------------------------------------------------------

ABORT_AT = (0, 1, 2)


@pytest.mark.parametrize("abort_at", ABORT_AT)
def test_variable_sites_sink_aborts(v2m, ctx, monkeypatch, abort_at):
	from vcf2multialign_amd import _native as N
	set_row_slices(ctx, monkeypatch, 3)
	rc, blocks, _ = variable_sites_call(v2m, ctx, abort_at)
	assert rc == N.V2M_ERR_SINK and blocks == slices_of(3)[:abort_at + 1], (rc, blocks)
	assert "sink aborted" in ctx._lib.v2m_last_error(ctx._h).decode()
	rc, blocks, data = variable_sites_call(v2m, ctx)
	assert rc == N.V2M_OK and blocks == slices_of(3) and np.array_equal(data, expected_bytes())


@pytest.mark.parametrize("abort_at", ABORT_AT)
def test_site_ld_sink_aborts(v2m, ctx, monkeypatch, abort_at):
	from vcf2multialign_amd import _native as N
	ranges = set_ld_ranges(monkeypatch, 3)
	rc, blocks, _ = site_ld_call(v2m, ctx, abort_at)
	assert rc == N.V2M_ERR_SINK and blocks == ranges[:abort_at + 1], (rc, blocks, ranges)
	assert "sink aborted" in ctx._lib.v2m_last_error(ctx._h).decode()
	rc, blocks, pairs = site_ld_call(v2m, ctx)
	assert rc == N.V2M_OK and blocks == ranges and np.array_equal(pairs, expected_pairs())


@pytest.mark.parametrize("abort_at", ABORT_AT)
def test_tree_parsimony_sink_aborts(v2m, ctx, monkeypatch, abort_at):
	from vcf2multialign_amd import _native as N
	want_branches, want_mutations = expected_parsimony(ctx)
	want_blocks = mutations_per_range(ctx, set_parsimony_ranges(monkeypatch, 3))
	assert len(want_blocks) == 3 and all(want_blocks), want_blocks
	rc, blocks, _, _ = tree_parsimony_call(v2m, ctx, abort_at)
	assert rc == N.V2M_ERR_SINK and blocks == want_blocks[:abort_at + 1], (rc, blocks, want_blocks)
	assert "sink aborted" in ctx._lib.v2m_last_error(ctx._h).decode()
	rc, blocks, mutations, branches = tree_parsimony_call(v2m, ctx)
	assert rc == N.V2M_OK and blocks == want_blocks, (rc, blocks, want_blocks)
	assert mutations.tobytes() == want_mutations.tobytes() and np.array_equal(branches, want_branches)


# ---- the checked build -----------------------------------------------------------------------------------------------------------------------

CHECKED_CORPUS = [
	"tests/test_gpu_shared_drivers.py::test_variable_sites_sink_aborts",
	"tests/test_gpu_shared_drivers.py::test_site_ld_sink_aborts",
	"tests/test_gpu_shared_drivers.py::test_tree_parsimony_sink_aborts",
]


def test_sink_aborts_on_the_checked_build():
	"""The abort cases with every scratch buffer and staging area poisoned before use (tests/test_gpu_checked_build.py), in a child
	process, one run per seed: a call after an aborted one that reads what the aborted call left changes its result.  No library is
	preloaded."""
	from test_gpu_checked_build import SEEDS, run_checked_corpus
	from vcf2multialign_amd import build
	assert os.path.exists(build.CHECKED_LIB_PATH) and os.path.exists(build.CHECKED_HOST_LIB_PATH), "build_native() builds them"
	for seed in SEEDS:   # the second seed only once the first has passed
		rc, out = run_checked_corpus(seed, build.CHECKED_LIB_PATH, build.CHECKED_HOST_LIB_PATH, corpus=CHECKED_CORPUS, timeout=600)
		assert rc == 0, "checked build, seed %s: exit %d\n%s" % (seed, rc, out[-6000:])
		assert " passed" in out and "libv2m_hip_checked.so" in out, out[-3000:]
		print(seed, out.strip().splitlines()[-2])
