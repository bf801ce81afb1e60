"""Window diversity on the GPU (include/v2m_hip.h, "window diversity"; csrc/diversity_kernels.hpp) against the numpy model of
tests/window_diversity_model.py, byte for byte and with no tolerance: the corpus of hand-made counts tables through
v2m_diversity_of_counts from uploads whose every element outside the table's columns is hostile, with guards around the results; the
graph items of tests/variable_sites_model.py through v2m_window_diversity, whole and under a column window, in bins of 1, 7 and all
columns, within and between two row groups; the cross-check against the pair distances; the views; the errors of the raw ABI; the
driver and the Python output classes on the reference fixture test-4, with and without groups and with --region, against the model's
text; and the device corpus and the graph items again on the checked build."""

import ctypes as C
import os

import numpy as np
import pytest

import column_counts_model as CM
import variable_sites_model as VM
import window_diversity_model as M

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FILL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def v2m():
	import vcf2multialign_amd as v
	from vcf2multialign_amd import _native as N
	assert (N.DIVERSITY_COLUMNS, N.DIVERSITY_SFS_LDS_BINS) == M.kernel_constants() and N.DIVERSITY_MAX_ROWS == M.MAX_ROWS
	assert np.dtype(N.DIVERSITY_BIN_DTYPE) == M.BIN_DTYPE and np.dtype(N.DIVERSITY_BETWEEN_BIN_DTYPE) == M.BETWEEN_DTYPE
	return v


@pytest.fixture(scope="module")
def ctx(v2m):
	c = v2m.Context(0)
	yield c
	c.close()


def upload(v2m, ctx, g):
	ctx.upload_graph(v2m.VariantGraph.from_object(g), g.ref)


class Table:
	"""M.table(planes) in device memory, 16-byte aligned."""

	def __init__(self, planes, seed=5):
		import torch
		self.host, self.pitch = M.table(planes, seed)
		self.device = torch.from_numpy(self.host.view(np.int32).copy()).cuda()
		self.ptr = self.device.data_ptr()
		assert self.ptr % 16 == 0 and self.pitch % 4 == 0

	def unchanged(self):
		return np.array_equal(self.device.cpu().numpy().view(np.uint32), self.host)


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


# ---- the device form on hand-made tables ------------------------------------------------------------------------------------------------

CORPUS = M.corpus()


def check_item(ctx, item):
	want_bins, want_sfs, want_many = M.expected(item.name)
	a = Table(item.planes)
	b = Table(item.planes_b, seed=9) if item.planes_b is not None else None
	n_bins = len(item.bounds) - 1
	bins = Filled(n_bins, M.BETWEEN_DTYPE if b else M.BIN_DTYPE)
	sfs = Filled(item.n // 2 + 1, np.uint64) if item.sfs else None
	if b:
		assert b.pitch == a.pitch
	info = ctx.diversity_of_counts(a.ptr, a.pitch, item.L, item.n, item.bounds, bins.ptr, sfs.ptr if sfs else None, b.ptr if b else None, item.n_b)
	same_records(bins.records(), want_bins, item.name + ": bins")
	if sfs:
		assert sfs.records().tobytes() == want_sfs.tobytes(), (item.name, np.flatnonzero(sfs.records() != want_sfs)[:8])
	assert (info["n_columns"], info["n_bins"], info["multiallelic"]) == (item.L, n_bins, want_many), (item.name, info)
	assert info["counts_ms"] == info["bins_ms"] == 0.0                                              # profiling is off
	assert a.unchanged() and (b is None or b.unchanged()), item.name + ": the tables"


@pytest.mark.parametrize("item", CORPUS, ids=[i.name for i in CORPUS])
def test_device_form(ctx, item):
	check_item(ctx, item)


def test_stage_times_while_profiling(ctx):
	item = next(i for i in CORPUS if i.name == "seams")
	a, bins = Table(item.planes), Filled(len(item.bounds) - 1, M.BIN_DTYPE)
	ctx.profile_enable(True)
	try:
		info = ctx.diversity_of_counts(a.ptr, a.pitch, item.L, item.n, item.bounds, bins.ptr)
	finally:
		ctx.profile_enable(False)
	assert info["bins_ms"] > 0.0 and info["counts_ms"] == 0.0
	same_records(bins.records(), M.expected(item.name)[0], "while profiling")


# ---- through rows -----------------------------------------------------------------------------------------------------------------------

GRAPH_ITEMS = VM.corpus()


def bounds_of(L, begin):
	return [np.arange(L + 1, dtype=np.uint64) + np.uint64(begin), np.array(sorted(set(list(range(0, L, 7)) + [L])), dtype=np.uint64) + np.uint64(begin),
		np.array([begin, begin + L], dtype=np.uint64)]


@pytest.mark.parametrize("item", GRAPH_ITEMS, ids=[i.name for i in GRAPH_ITEMS])
def test_graph_items(v2m, ctx, item):
	upload(v2m, ctx, item.g)
	begin = 0
	if item.window:
		ctx.set_column_window(*item.window)
		begin = item.window[0]
	m = CM.matrix(item.g, item.rows, item.window)
	n, L = m.shape
	c = M.letters_of(m)
	half = max(1, n // 2)
	rows_a, rows_b = list(item.rows[:half]), list(item.rows[half:])
	for bounds in bounds_of(L, begin):
		relative = bounds - np.uint64(begin)
		bins, sfs, info = ctx.window_diversity(item.rows, bounds, info=True)
		same_records(bins, M.from_counts(c, n, relative), item.name)
		want_sfs, want_many = M.sfs_from_counts(c, n, relative[0], relative[-1])
		assert sfs.tobytes() == want_sfs.tobytes(), item.name
		assert (info["n_columns"], info["n_bins"], info["multiallelic"]) == (L, len(bounds) - 1, want_many), (item.name, info)
		if rows_b:
			between, none = ctx.window_diversity(rows_a, bounds, rows_b=rows_b)
			same_records(between, M.between_from_counts(M.letters_of(m[:half]), M.letters_of(m[half:]), relative), item.name + ": between")
			assert none is None


def test_graph_items_cover_the_forms():
	assert any(i.window for i in GRAPH_ITEMS) and any(not i.window for i in GRAPH_ITEMS)
	assert any(isinstance(r, (list, tuple)) for i in GRAPH_ITEMS for r in i.rows), "rows with cuts"


CROSS = [i for i in GRAPH_ITEMS if len(i.rows) >= 2][::7]


@pytest.mark.parametrize("item", CROSS, ids=[i.name for i in CROSS])
def test_diffs_equal_the_pair_distances(v2m, ctx, item):
	"""Two independent kernels: one bin over the view sums what the upper triangle of the ACGT-only distances sums."""
	upload(v2m, ctx, item.g)
	begin, end = item.window if item.window else (0, item.g.aligned_length)
	if item.window:
		ctx.set_column_window(*item.window)
	bins, _ = ctx.window_diversity(item.rows, [begin, end], want_sfs=False)
	dist = ctx.pair_distances(item.rows, acgt_only=True)
	assert int(bins["diffs"][0]) == int(np.triu(dist.astype(np.uint64), 1).sum(dtype=np.uint64)), item.name
	assert int(bins["columns"][0]) == end - begin


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
	m = CM.matrix(g, rows, w)
	bounds = np.array([w[0], w[0] + 1, w[1]], dtype=np.uint64)
	bins, sfs = ctx.window_diversity(rows, bounds)
	same_records(bins, M.from_counts(M.letters_of(m), len(rows), bounds - np.uint64(w[0])), "under a window set and a window")
	half = max(1, len(rows) // 2)
	ctx.window_diversity(rows[:half], bounds, rows_b=rows[half:] or rows[:1])
	assert ctx.window_length == w[1] - w[0] and ctx.window_set_size == len(sets)
	for a, b in zip(before, ctx.column_counts(rows)):
		assert np.array_equal(a, b)
	assert ctx.splice_rows(rows) == spliced and ctx.splice_window_set(rows) == pieces


# ---- the raw ABI ------------------------------------------------------------------------------------------------------------------------

def test_errors(v2m):
	from vcf2multialign_amd import _native as N
	with v2m.Context(0) as c:
		item = next(i for i in CORPUS if i.name == "seams")
		other = next(i for i in CORPUS if i.name == "between")
		a, bins, sfs = Table(item.planes), Filled(len(item.bounds) - 1, M.BIN_DTYPE), Filled(item.n // 2 + 1, np.uint64)
		of_counts, of_rows = c._lib.v2m_diversity_of_counts, c._lib.v2m_window_diversity
		last_error = lambda: c._lib.v2m_last_error(c._h).decode()
		info = N.WindowDiversityInfo()
		info.n_bins = 77
		def args(ta=a.ptr, tb=None, pitch=a.pitch, L=item.L, n=item.n, n_b=0, bounds=item.bounds, n_bins=None, d_bins=bins.ptr, d_sfs=None):
			bounds = None if bounds is None else np.ascontiguousarray(bounds, dtype=np.uint64)
			args.keep = bounds
			return (c._h, ta, tb, pitch, L, n, n_b, bounds.ctypes.data if bounds is not None else None, (len(bounds) - 1 if n_bins is None else n_bins) if bounds is not None else 1,
				d_bins, d_sfs, C.byref(info))
		untouched = lambda: bins.untouched() and sfs.untouched() and info.n_bins == 77
		# no bin, no row: V2M_OK and nothing touched
		assert N.V2M_OK == of_counts(*args(n_bins=0)) and untouched()
		assert N.V2M_OK == of_counts(*args(n=0, d_sfs=sfs.ptr)) and untouched()
		assert N.V2M_OK == of_counts(*args(tb=a.ptr, n_b=0)) and untouched()
		assert N.V2M_ERR_INVALID_ARGUMENT == of_counts(None, *args()[1:])
		for bad, word in ((dict(ta=None), "d_counts_a is NULL"), (dict(d_bins=None), "d_bins is NULL"), (dict(bounds=None), "bounds is NULL"),
				(dict(n_b=3), "without a second table"), (dict(tb=a.ptr, n_b=3, d_sfs=sfs.ptr), "no spectrum"),
				(dict(ta=a.ptr + 4), "16-byte aligned"), (dict(d_bins=bins.ptr + 8), "16-byte aligned"), (dict(d_sfs=sfs.ptr + 8), "16-byte aligned"),
				(dict(pitch=a.pitch + 2), "multiple of 4"), (dict(pitch=((item.L + 3) & ~3) - 4), "at least"),
				(dict(bounds=[0, 9, 8, 20]), "descends"), (dict(bounds=[0, item.L + 1]), "leave")):
			assert N.V2M_ERR_INVALID_ARGUMENT == of_counts(*args(**bad)), bad
			assert word in last_error() and untouched(), (bad, last_error())
		for bad, word in ((dict(n=M.MAX_ROWS + 1), "V2M_DIVERSITY_MAX_ROWS"), (dict(tb=a.ptr, n_b=M.MAX_ROWS + 1), "V2M_DIVERSITY_MAX_ROWS"),
				(dict(L=1 << 32, pitch=1 << 32), "2^32")):
			assert N.V2M_ERR_UNSUPPORTED == of_counts(*args(**bad)), bad
			assert word in last_error() and untouched(), (bad, last_error())
		assert a.unchanged()
		# the host form: without a graph, then its own arguments
		rows = v2m.RowBatch([0, 1])
		bounds = np.array([0, 3], dtype=np.uint64)
		out = np.zeros(1, dtype=M.BIN_DTYPE)
		out_sfs = np.zeros(2, dtype=np.uint64)
		call = lambda ra=rows, rb=None, b=bounds, n_bins=1, o=out, s=None: of_rows(c._h, C.byref(ra.struct) if ra is not None else None, C.byref(rb.struct) if rb is not None else None,
			b.ctypes.data if b is not None else None, n_bins, o.ctypes.data if o is not None else None, s.ctypes.data if s is not None else None, C.byref(info))
		assert N.V2M_ERR_STATE == call()
		g = other_graph = next(i for i in GRAPH_ITEMS if not i.window and i.g.aligned_length >= 8).g
		c.upload_graph(v2m.VariantGraph.from_object(g), g.ref)
		L = g.aligned_length
		assert N.V2M_ERR_INVALID_ARGUMENT == of_rows(None, C.byref(rows.struct), None, bounds.ctypes.data, 1, out.ctypes.data, None, None)
		for bad, word in ((dict(ra=None), "rows_a is NULL"), (dict(o=None), "bins is NULL"), (dict(b=None), "bounds is NULL"), (dict(rb=rows, s=out_sfs), "no spectrum"),
				(dict(b=np.array([4, 3], dtype=np.uint64)), "descends"), (dict(b=np.array([0, L + 1], dtype=np.uint64)), "leave")):
			assert N.V2M_ERR_INVALID_ARGUMENT == call(**bad), bad
			assert word in last_error() and info.n_bins == 77 and not out.view(np.uint64).any(), (bad, last_error())
		c.set_column_window(2, 6)
		for b in ([1, 3], [2, 7]):
			assert N.V2M_ERR_INVALID_ARGUMENT == call(b=np.array(b, dtype=np.uint64)) and "leave the view" in last_error()
		inside = np.array([2, 6], dtype=np.uint64)
		assert N.V2M_OK == call(b=inside, n_bins=0) and N.V2M_OK == call(ra=v2m.RowBatch([]), b=inside) and N.V2M_OK == call(rb=v2m.RowBatch([]), b=inside) and info.n_bins == 77
		assert not out.view(np.uint64).any()
		assert N.V2M_OK == call(b=inside, s=out_sfs) and info.n_bins == 1 and int(out["columns"][0]) == 4


# ---- the driver -------------------------------------------------------------------------------------------------------------------------

CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")


def _run(args, cwd=None):
	import subprocess
	assert os.path.exists(CLI), "build the host driver first (__graft_entry__.build())"
	return subprocess.run([CLI] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def test_cli_haplotypes(v2m, ctx, tmp_path, monkeypatch):
	import io
	import oracle
	import pair_distances_model as PM
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	g = oracle.build_variant_graph(fa, vcf, "1")
	vg = v2m.VariantGraph.from_object(g)
	ids, rows = PM.haplotype_ids(g)
	assert len(ids) >= 6
	div, sfs, dvg, grp = (tmp_path / name for name in ("out.div.tsv", "out.sfs.tsv", "out.dxy.tsv", "groups.tsv"))
	common = ["-H", "-r", fa, "-a", vcf, "-c", "1"]
	upload(v2m, ctx, g)
	# one group, `all`: windows of one bin, then sliding windows of three bins, then under --region
	for flags, kw, region in (([], dict(window=10000), None), (["--diversity-window=4"], dict(window=4), None), (["--diversity-window=6", "--diversity-step=2"], dict(window=6, step=2), None),
			(["--diversity-window=4", "--diversity-step=2", "--region=3-16"], dict(window=4, step=2), (2, 16))):
		want = M.driver_texts(g, ids, rows, region=region, **kw)
		r = _run(common + ["--output-diversity=" + str(div), "--diversity-sfs=" + str(sfs), "--verbose"] + flags)
		assert r.returncode == 0, r.stderr.decode()
		assert (div.read_bytes(), sfs.read_bytes()) == want[:2], (flags, div.read_bytes().decode(), want[0].decode())
		assert b"Diversity: %d rows, " % len(rows) in r.stderr and want[2] is None
		streams = [io.BytesIO(), io.BytesIO()]
		v2m.HaplotypeOutput(ctx, region=region).output_diversity(vg, *streams, **kw)
		assert tuple(x.getvalue() for x in streams) == want[:2], flags
	# three groups, a sequence in none of them, the file's order not the rows'
	pairs = [(ids[5], "north"), (ids[0], "south"), (ids[1], "north"), (ids[2], "south"), (ids[4], "east"), (ids[6], "north")]
	grp.write_text("# id, group\n" + "".join("%s\t%s\n" % p for p in pairs))
	for flags, kw, region in ((["--diversity-window=4", "--diversity-step=2"], dict(window=4, step=2), None), (["--diversity-window=5", "--region=2-19"], dict(window=5), (1, 19))):
		want = M.driver_texts(g, ids, rows, groups=pairs, region=region, **kw)
		r = _run(common + ["--output-diversity=" + str(div), "--diversity-sfs=" + str(sfs), "--output-divergence=" + str(dvg), "--diversity-groups=" + str(grp)] + flags)
		assert r.returncode == 0, r.stderr.decode()
		assert (div.read_bytes(), sfs.read_bytes(), dvg.read_bytes()) == want, (flags, dvg.read_bytes().decode(), want[2].decode())
		assert want[0].count(b"\nnorth\t") and want[2].startswith(b"#group_a\tgroup_b\t") and b"\nsouth\teast\t" in want[2]
		streams = [io.BytesIO() for _ in range(3)]
		v2m.HaplotypeOutput(ctx, region=region).output_diversity(vg, *streams, groups=pairs, **kw)
		assert tuple(x.getvalue() for x in streams) == want, flags
	# divergence alone; the tables' budget
	dvg.unlink()
	r = _run(common + ["--output-divergence=" + str(dvg), "--diversity-groups=" + str(grp), "--diversity-window=5", "--region=2-19"])
	assert r.returncode == 0 and dvg.read_bytes() == want[2], r.stderr.decode()
	monkeypatch.setenv("V2M_DIVERSITY_TABLE_BYTES", "1000")
	r = _run(common + ["--output-diversity=" + str(div), "--diversity-groups=" + str(grp)])
	assert r.returncode != 0 and b"more than V2M_DIVERSITY_TABLE_BYTES = 1000" in r.stderr, r.stderr.decode()
	with pytest.raises(ValueError, match="V2M_DIVERSITY_TABLE_BYTES = 1000"):
		v2m.HaplotypeOutput(ctx).output_diversity(vg, io.BytesIO(), groups=pairs)
	assert ctx.window_length == g.aligned_length


# ---- the checked build ------------------------------------------------------------------------------------------------------------------

CHECKED_CORPUS = [
	"tests/test_gpu_window_diversity.py::test_device_form",
	"tests/test_gpu_window_diversity.py::test_graph_items",
]


def test_corpus_on_the_checked_build():
	"""The device-form corpus with every LDS object (the waves' sums, the histogram) and every scratch buffer (the bounds, the
	multiallelic count) poisoned before use (tests/test_gpu_checked_build.py), one child process per seed: a counter or a sum nobody
	wrote in this call changes the result.  No library is preloaded."""
	from test_gpu_checked_build import SEEDS, run_checked_corpus
	from vcf2multialign_amd import build
	assert os.path.exists(build.CHECKED_LIB_PATH) and os.path.exists(build.CHECKED_HOST_LIB_PATH), "build_native() builds them"
	for seed in SEEDS:   # the second seed only once the first has passed
		rc, out = run_checked_corpus(seed, build.CHECKED_LIB_PATH, build.CHECKED_HOST_LIB_PATH, corpus=CHECKED_CORPUS, timeout=600)
		assert rc == 0, "checked build, seed %s: exit %d\n%s" % (seed, rc, out[-6000:])
		assert " passed" in out and "libv2m_hip_checked.so" in out, out[-3000:]
		print(seed, out.strip().splitlines()[-2])
