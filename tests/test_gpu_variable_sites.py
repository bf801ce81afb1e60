"""Context.variable_sites / variable_sites_device (v2m_variable_sites[_device]: the column counts' kernels, the two selections' count and
emit kernels, gather_sites_kernel) and --output-variable-sites against the model of tests/variable_sites_model.py: every item goes through
the host form and through the device form, with guard bytes around and inside its buffers, under both selections, each held equal to the
model byte for byte.

tests/test_variable_sites_host.py asserts, without a GPU, that the corpus holds the site counts, row counts, windows and bytes it is here
for, and that the selected columns carry the pair distances."""

import ctypes as C
import io
import os

import numpy as np
import pytest

import column_counts_model as CM
import oracle
import pair_distances_model as PM
import row_ops_model as M
import synth
import variable_sites_model as VM

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")
PLOIDY_MAX = VM.PLOIDY_MAX
S, THREADS, GROUP = VM.kernel_constants()     # kGatherSites, kGatherThreads, kGatherMinGroupRows
GUARD = 64                                    # guard bytes (and guard columns) on either side of a device buffer


@pytest.fixture(scope="module")
def v2m():
	import vcf2multialign_amd as v
	from vcf2multialign_amd import _native as N
	assert (N.GATHER_SITES, N.GATHER_THREADS, N.GATHER_MIN_GROUP_ROWS) == (S, THREADS, GROUP)
	return v


@pytest.fixture(scope="module")
def ctx(v2m):
	c = v2m.Context(0)
	yield c
	c.close()


def upload(v2m, ctx, g):
	ctx.upload_graph(v2m.VariantGraph.from_object(g), g.ref)


def pattern_bytes(n):
	"""A pre-fill without a zero byte (the bytes written as 0 behind the sites must show) that repeats with no period of a pitch."""
	return ((np.arange(n, dtype=np.uint64) * 2654435761 >> 7) % 251 + 1).astype(np.uint8)


def pattern_words(n):
	return ((np.arange(n, dtype=np.uint64) * 2654435761 + 0x5EEDC0DE) & 0xFFFFFFFF).astype(np.uint32) | np.uint32(0x80000000)


class DeviceBuffers:
	"""u8[n][pitch] and u32[pitch] on the device, each between GUARD guard elements, pre-filled."""

	def __init__(self, n, pitch):
		import torch
		self.n, self.pitch = n, pitch
		self.fill_bytes = pattern_bytes(2 * GUARD + max(n, 1) * pitch)
		self.fill_columns = pattern_words(2 * GUARD + pitch)
		self.bytes = torch.from_numpy(self.fill_bytes.copy()).cuda()
		self.columns = torch.from_numpy(self.fill_columns.view(np.int32).copy()).cuda()
		self.ptr = self.bytes.data_ptr() + GUARD
		self.columns_ptr = self.columns.data_ptr() + 4 * GUARD
		assert self.ptr % 16 == 0 and pitch % 16 == 0

	def read(self):
		return self.bytes.cpu().numpy(), self.columns.cpu().numpy().view(np.uint32)

	def untouched(self):
		b, c = self.read()
		return np.array_equal(b, self.fill_bytes) and np.array_equal(c, self.fill_columns)


def check_device(ctx, rows, want_columns, want_bytes, first, snp_only, what, extra=16, with_columns=True):
	"""The device form into guarded buffers of pitch V rounded up to 16, plus `extra`."""
	n, V = len(rows), len(want_columns)
	pitch = ((V + 15) & ~15) + extra
	buf = DeviceBuffers(n, pitch)
	got_V = ctx.variable_sites_device(rows, buf.ptr, pitch, columns_ptr=buf.columns_ptr if with_columns else None, snp_only=snp_only)
	assert got_V == V, "%s: %d sites, expected %d" % (what, got_V, V)
	b, c = buf.read()
	assert np.array_equal(b[:GUARD], buf.fill_bytes[:GUARD]) and np.array_equal(b[GUARD + n * pitch:], buf.fill_bytes[GUARD + n * pitch:]), what + ": the guards around the bytes"
	assert np.array_equal(c[:GUARD], buf.fill_columns[:GUARD]) and np.array_equal(c[GUARD + V:], buf.fill_columns[GUARD + V:]), what + ": the columns beyond V and their guards"
	if with_columns:
		assert np.array_equal(c[GUARD:GUARD + V].astype(np.uint64) + np.uint64(first), want_columns), what + ": the columns (relative to the view)"
	else:
		assert np.array_equal(c, buf.fill_columns), what + ": no columns asked for"
	if n:
		body = b[GUARD:GUARD + n * pitch].reshape(n, pitch)
		fill = buf.fill_bytes[GUARD:GUARD + n * pitch].reshape(n, pitch)
		pad = (V + 3) & ~3
		if not np.array_equal(body[:, :V], want_bytes):
			bad = np.argwhere(body[:, :V] != want_bytes)
			r, s = bad[0]
			raise AssertionError("%s: %d of %d bytes differ, the first at row %d site %d: got 0x%02x, expected 0x%02x" % (what, len(bad), want_bytes.size, r, s, body[r, s], want_bytes[r, s]))
		if V:
			assert (body[:, V:pad] == 0).all(), what + ": bytes [V, (V + 3) & ~3) are written as 0"
			assert np.array_equal(body[:, pad:], fill[:, pad:]), what + ": nothing beyond (V + 3) & ~3 of a row is touched"
		else:
			assert np.array_equal(body, fill), what + ": no site, nothing written"


def check_forms(ctx, g, rows, window=None, what=""):
	"""Both forms under both selections over the view in force (`window` says which that is) against the model; returns the infos."""
	what = what or getattr(g, "name", "graph")
	infos = []
	for snp_only in (False, True):
		label = "%s%s" % (what, " snp" if snp_only else "")
		want_columns, want_bytes, L = VM.expected(g, rows, window, snp_only)
		assert ctx.window_length == L
		columns, data, info = ctx.variable_sites(rows, snp_only=snp_only, info=True)
		assert columns.dtype == np.uint64 and np.array_equal(columns, want_columns), label + " host form: the columns"
		assert data.dtype == np.uint8 and data.shape == want_bytes.shape and np.array_equal(data, want_bytes), label + " host form: the bytes"
		assert (info["n_sites"], info["n_columns"]) == (len(want_columns), L), (label, info)
		assert info["counts_ms"] == info["gather_ms"] == 0.0      # profiling is off
		blocks = ctx.variable_sites_blocks
		assert blocks == ([(0, len(rows))] if len(want_columns) and len(rows) else []), (label, blocks)
		check_device(ctx, rows, want_columns, want_bytes, window[0] if window else 0, snp_only, label + " device form")
		infos.append(info)
	return infos


# ---- the corpus ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("item", VM.corpus(), ids=[i.name for i in VM.corpus()])
def test_corpus(v2m, ctx, item):
	upload(v2m, ctx, item.g)
	if item.window:
		ctx.set_column_window(*item.window)
	info, _ = check_forms(ctx, item.g, item.rows, item.window, item.name)
	if item.window:
		assert ctx.window_length == item.window[1] - item.window[0]
	assert info["n_sites"] == ctx.pair_distances(item.rows, info=True)[1]["n_sites"]


def test_exact_pitch_and_no_columns(v2m, ctx):
	"""A pitch of exactly V rounded up to 16 (V a multiple of 16: no byte to spare), and a NULL d_columns."""
	V = 4 * 64 * S
	g = PM.sites_graph_of(V)
	upload(v2m, ctx, g)
	want_columns, want_bytes, _ = VM.expected(g, PM.SITE_ROWS)
	assert len(want_columns) == V and V % 16 == 0
	check_device(ctx, PM.SITE_ROWS, want_columns, want_bytes, 0, False, "exact pitch", extra=0)
	check_device(ctx, PM.SITE_ROWS, want_columns, want_bytes, 0, False, "no columns", with_columns=False)


def test_too_small_a_pitch(v2m, ctx):
	"""V > pitch: the error, *n_sites set, nothing written; the caller sizes by it and calls again."""
	from vcf2multialign_amd import _native as N
	g = PM.sites_graph_of(64 * S + 1)
	upload(v2m, ctx, g)
	rows = PM.SITE_ROWS
	for snp_only in (False, True):
		want_columns, want_bytes, _ = VM.expected(g, rows, snp_only=snp_only)
		V = len(want_columns)
		assert V > 16
		for pitch in (0, 16, (V - 1) & ~15):
			buf = DeviceBuffers(len(rows), max(pitch, 16))
			with pytest.raises(v2m.V2MError) as e:
				ctx.variable_sites_device(rows, buf.ptr, pitch, columns_ptr=buf.columns_ptr, snp_only=snp_only)
			assert e.value.code == N.V2M_ERR_INVALID_ARGUMENT and str(V) in str(e.value), str(e.value)
			assert ctx.variable_sites_count == V and buf.untouched()
		check_device(ctx, rows, want_columns, want_bytes, 0, snp_only, "sized by the first call", extra=0)


def test_row_slices(v2m, ctx, monkeypatch):
	"""V2M_RING_SLOT_BYTES small enough for four slices of three rows and one of one: both passes over the rows go slice by slice, the
	row sink receives the five blocks in order, and together they are the whole batch."""
	g = PM.sites_graph_of(THREADS * S + 65)
	upload(v2m, ctx, g)
	rows = [0, 1, PLOIDY_MAX, 2, 3, 4, 5, 6, 3, 0] + PM.cut_rows(g)
	assert len(rows) == 13
	want = check_forms(ctx, g, rows, what="one slice")
	pitch = int(ctx.min_row_pitch)
	monkeypatch.setenv("V2M_RING_SLOT_BYTES", str(3 * pitch + pitch // 2))
	from vcf2multialign_amd import _native as N
	ctx.profile_enable(True)
	ctx.profile_reset()
	try:
		columns, data, info = ctx.variable_sites(rows, info=True)
		launches = ctx.profile_get(N.KERNEL_COLUMN_COUNTS)[0]
		assert launches == 5, launches      # four slices of three rows and a remainder of one
		assert info["counts_ms"] > 0 and info["gather_ms"] > 0
	finally:
		ctx.profile_reset()
		ctx.profile_enable(False)
	assert ctx.variable_sites_blocks == [(0, 3), (3, 3), (6, 3), (9, 3), (12, 1)]
	want_columns, want_bytes, _ = VM.expected(g, rows)
	assert np.array_equal(columns, want_columns) and np.array_equal(data, want_bytes)
	for snp_only in (False, True):
		want_columns, want_bytes, _ = VM.expected(g, rows, snp_only=snp_only)
		columns, data = ctx.variable_sites(rows, snp_only=snp_only)
		assert ctx.variable_sites_blocks == [(0, 3), (3, 3), (6, 3), (9, 3), (12, 1)]
		assert np.array_equal(columns, want_columns) and np.array_equal(data, want_bytes)
		check_device(ctx, rows, want_columns, want_bytes, 0, snp_only, "device form in slices")
	monkeypatch.delenv("V2M_RING_SLOT_BYTES")
	assert check_forms(ctx, g, rows, what="one slice again") == want


# ---- row groups above the floor ----------------------------------------------------------------------------------------------------------------

# V2M_SITE_ROWS_PER_GROUP over the 3 T + 1 distinct rows of tests/pair_distances_model.py: a row a group; one unrolled trip of four and a
# tail row in every group, the groups starting at every residue mod 4; a tail of two, the groups starting at the even residues; 67; exactly one group; one group of more rows than
# there are (what the rule gives when the site blocks alone fill the device)
GROUP_ITEM_ROWS = 3 * PM.kernel_constants()[0] + 1
SITE_ROWS_PER_GROUP = (1, 5, 18, 67, GROUP_ITEM_ROWS, 1000000)


@pytest.mark.parametrize("per_group", SITE_ROWS_PER_GROUP)
def test_row_groups_of_the_gather(v2m, ctx, monkeypatch, per_group):
	"""gather_sites_kernel with groups of other sizes than the rule's floor, over rows that all differ: a group written one group off
	shows in every byte."""
	item = PM.distinct_item(GROUP_ITEM_ROWS)
	assert GROUP not in SITE_ROWS_PER_GROUP and len(VM.expected(item.g, item.rows)[0]) == PM.variable_columns(item.g) == 2 * 64 * PM.kernel_constants()[1] + 5
	upload(v2m, ctx, item.g)
	monkeypatch.setenv("V2M_SITE_ROWS_PER_GROUP", str(per_group))
	check_forms(ctx, item.g, item.rows, what="%s, %d rows a group" % (item.name, per_group))


@pytest.mark.parametrize("per_group", (18, 1000000))
def test_row_groups_of_the_gather_in_slices(v2m, ctx, monkeypatch, per_group):
	"""The same under slices of 50 rows: a slice's first row is neither the batch's first nor a multiple of the group."""
	item = PM.distinct_item(GROUP_ITEM_ROWS)
	upload(v2m, ctx, item.g)
	pitch = int(ctx.min_row_pitch)
	monkeypatch.setenv("V2M_RING_SLOT_BYTES", str(50 * pitch + pitch // 2))
	monkeypatch.setenv("V2M_SITE_ROWS_PER_GROUP", str(per_group))
	for snp_only in (False, True):
		want_columns, want_bytes, _ = VM.expected(item.g, item.rows, snp_only=snp_only)
		columns, data = ctx.variable_sites(item.rows, snp_only=snp_only)
		assert ctx.variable_sites_blocks == [(0, 50), (50, 50), (100, 50), (150, GROUP_ITEM_ROWS - 150)]
		assert np.array_equal(columns, want_columns) and np.array_equal(data, want_bytes)
		check_device(ctx, item.rows, want_columns, want_bytes, 0, snp_only, "device form in slices, %d rows a group" % per_group)


def test_sinks(v2m, ctx):
	"""A sink that returns non-zero gives V2M_ERR_SINK (and the other sink is not called afterwards); NULL sinks are accepted."""
	from vcf2multialign_amd import _native as N
	g = PM.sites_graph_of(70)
	upload(v2m, ctx, g)
	batch = v2m.RowBatch(PM.SITE_ROWS)
	calls = []
	call = ctx._lib.v2m_variable_sites

	def columns_sink(result):
		def cb(_user, _columns, n_sites):
			calls.append(("columns", int(n_sites)))
			return result
		return N.SITE_COLUMNS_SINK_FN(cb)

	def rows_sink(result):
		def cb(_user, first_row, n_rows, _bytes, pitch, n_sites):
			calls.append(("rows", int(first_row), int(n_rows), int(n_sites)))
			assert pitch >= n_sites
			return result
		return N.SITE_ROWS_SINK_FN(cb)

	info = N.VariableSitesInfo()
	assert N.V2M_OK == call(ctx._h, C.byref(batch.struct), 0, columns_sink(0), rows_sink(0), None, C.byref(info))
	assert calls == [("columns", 70), ("rows", 0, len(PM.SITE_ROWS), 70)] and info.n_sites == 70
	del calls[:]
	assert N.V2M_ERR_SINK == call(ctx._h, C.byref(batch.struct), 0, columns_sink(3), rows_sink(0), None, None)
	assert calls == [("columns", 70)]
	del calls[:]
	assert N.V2M_ERR_SINK == call(ctx._h, C.byref(batch.struct), 0, columns_sink(0), rows_sink(-1), None, None)
	assert calls == [("columns", 70), ("rows", 0, len(PM.SITE_ROWS), 70)]
	del calls[:]
	null_columns, null_rows = C.cast(None, N.SITE_COLUMNS_SINK_FN), C.cast(None, N.SITE_ROWS_SINK_FN)
	assert N.V2M_OK == call(ctx._h, C.byref(batch.struct), 0, null_columns, rows_sink(0), None, None)
	assert calls == [("rows", 0, len(PM.SITE_ROWS), 70)]
	del calls[:]
	assert N.V2M_OK == call(ctx._h, C.byref(batch.struct), N.SITES_SNP, columns_sink(0), null_rows, None, C.byref(info))
	n_snp = len(VM.expected(g, PM.SITE_ROWS, snp_only=True)[0])
	assert calls == [("columns", n_snp)] and info.n_sites == n_snp and 0 < n_snp < 70
	del calls[:]
	assert N.V2M_OK == call(ctx._h, C.byref(batch.struct), 0, null_columns, null_rows, None, C.byref(info)) and info.n_sites == 70 and not calls
	# no site: neither sink is called
	upload(v2m, ctx, CM.other_graph())
	three = v2m.RowBatch([PLOIDY_MAX, 0, 1])
	assert N.V2M_OK == call(ctx._h, C.byref(three.struct), 0, columns_sink(1), rows_sink(1), None, C.byref(info)) and not calls and info.n_sites == 0 and info.n_columns == 21
	check_forms(ctx, CM.other_graph(), [PLOIDY_MAX, 0, 1], what="after the sinks")


def test_the_views_are_left_as_they_were(v2m, ctx):
	g = PM.window_graph()
	upload(v2m, ctx, g)
	rows = PM.SITE_ROWS
	w = PM.windows()[1]
	sets = [(2, 30), (41, 47), (3, 4)]
	ctx.set_window_set(sets)
	ctx.set_column_window(*w)
	pieces = ctx.splice_window_set(rows)
	before = ctx.column_counts(rows)
	before_variable = ctx.column_counts(rows, variable_only=True)
	spliced = ctx.splice_rows(rows)
	check_forms(ctx, g, rows, w, "under a window set and a window")
	assert ctx.window_length == w[1] - w[0] and ctx.window_set_size == len(sets)
	for a, b in zip(before + before_variable, ctx.column_counts(rows) + ctx.column_counts(rows, variable_only=True)):
		assert np.array_equal(a, b)
	assert ctx.splice_rows(rows) == spliced and ctx.splice_window_set(rows) == pieces
	# the bytes are those the rows hold at the columns
	columns, data = ctx.variable_sites(rows)
	bodies = np.stack([np.frombuffer(b, dtype=np.uint8) for b in spliced])
	assert np.array_equal(bodies[:, (columns - np.uint64(w[0])).astype(np.int64)], data)
	ctx.set_column_window(0, g.aligned_length)
	check_forms(ctx, g, rows, what="whole rows again")


@pytest.mark.parametrize("stem", ["test-1a", "test-2", "test-4"])
def test_reference_fixtures(v2m, ctx, stem):
	fasta = {"test-1a": "test-1.fa"}.get(stem, stem + ".fa")
	g = oracle.build_variant_graph(os.path.join(FIX, fasta), os.path.join(FIX, stem + ".vcf"), "1")
	upload(v2m, ctx, g)
	check_forms(ctx, g, M.rows_with_cuts(g), what=stem)


# ---- the raw ABI -----------------------------------------------------------------------------------------------------------------------------

def test_errors(v2m):
	import torch
	from vcf2multialign_amd import _native as N
	with v2m.Context(0) as c:
		g = CM.hostile_graph(0)
		batch = v2m.RowBatch(CM.HOSTILE_ROWS)
		n = len(CM.HOSTILE_ROWS)
		t = torch.full((n * 16 + 64,), 7, dtype=torch.uint8, device="cuda")
		cols = torch.full((64,), 7, dtype=torch.int32, device="cuda")
		count = C.c_uint64(77)
		null_columns, null_rows = C.cast(None, N.SITE_COLUMNS_SINK_FN), C.cast(None, N.SITE_ROWS_SINK_FN)
		call, device = c._lib.v2m_variable_sites, c._lib.v2m_variable_sites_device
		# no graph
		assert N.V2M_ERR_STATE == call(c._h, C.byref(batch.struct), 0, null_columns, null_rows, None, None)
		assert N.V2M_ERR_STATE == device(c._h, C.byref(batch.struct), 0, cols.data_ptr(), t.data_ptr(), 16, C.byref(count))
		upload(v2m, c, g)
		# flags: the one bit, and none of the other row calls'
		for flags in (0x1, 0x2, 0x4, 0x8, 0x10, 0x20, 0x41, 0x60, 0x80, 0x80000000):
			assert N.V2M_ERR_INVALID_ARGUMENT == call(c._h, C.byref(batch.struct), flags, null_columns, null_rows, None, None), hex(flags)
			assert N.V2M_ERR_INVALID_ARGUMENT == device(c._h, C.byref(batch.struct), flags, cols.data_ptr(), t.data_ptr(), 16, C.byref(count)), hex(flags)
		# NULL pointers
		assert N.V2M_ERR_INVALID_ARGUMENT == call(c._h, None, 0, null_columns, null_rows, None, None)
		assert N.V2M_ERR_INVALID_ARGUMENT == device(c._h, None, 0, cols.data_ptr(), t.data_ptr(), 16, C.byref(count))
		assert N.V2M_ERR_INVALID_ARGUMENT == device(c._h, C.byref(batch.struct), 0, cols.data_ptr(), None, 16, C.byref(count))
		assert N.V2M_ERR_INVALID_ARGUMENT == device(c._h, C.byref(batch.struct), 0, cols.data_ptr(), t.data_ptr(), 16, None)
		# a misaligned buffer, a pitch that is no multiple of 16
		for ptr, pitch in ((t.data_ptr() + 4, 16), (t.data_ptr() + 8, 16), (t.data_ptr() + 1, 16), (t.data_ptr(), 12), (t.data_ptr(), 8), (t.data_ptr(), 17)):
			assert N.V2M_ERR_INVALID_ARGUMENT == device(c._h, C.byref(batch.struct), 0, cols.data_ptr(), ptr, pitch, C.byref(count)), (ptr % 16, pitch)
		assert (t.cpu().numpy() == 7).all() and (cols.cpu().numpy() == 7).all() and count.value == 77
		want_columns, want_bytes, _ = VM.expected(g, CM.HOSTILE_ROWS)
		V = len(want_columns)
		assert 0 < V <= 16
		assert N.V2M_OK == device(c._h, C.byref(batch.struct), 0, cols.data_ptr(), t.data_ptr(), 16, C.byref(count)) and count.value == V
		assert np.array_equal(t.cpu().numpy()[:n * 16].reshape(n, 16)[:, :V], want_bytes)
		assert np.array_equal(cols.cpu().numpy()[:V].astype(np.uint64), want_columns)
		# no rows: V2M_OK, nothing touched
		empty = v2m.RowBatch([])
		before, before_cols = t.cpu().numpy().copy(), cols.cpu().numpy().copy()
		info = N.VariableSitesInfo()
		info.n_columns = 77
		count.value = 78
		sunk = []
		sink = N.SITE_COLUMNS_SINK_FN(lambda *a: sunk.append(a) or 0)
		assert N.V2M_OK == call(c._h, C.byref(empty.struct), 0, sink, null_rows, None, C.byref(info)) and info.n_columns == 77 and not sunk
		assert N.V2M_OK == device(c._h, C.byref(empty.struct), 0, cols.data_ptr(), t.data_ptr(), 0, C.byref(count)) and count.value == 78
		assert np.array_equal(t.cpu().numpy(), before) and np.array_equal(cols.cpu().numpy(), before_cols)
		columns, data, info_dict = c.variable_sites([], info=True)
		assert columns.shape == (0,) and data.shape == (0, 0) and info_dict["n_columns"] == g.aligned_length
		# one row: no site
		columns, data = c.variable_sites([3])
		assert columns.shape == (0,) and data.shape == (1, 0)
		# bad cuts
		bad = v2m.RowBatch([0, [(2, 0), (1, 1)]])
		assert N.V2M_ERR_PRECONDITION == call(c._h, C.byref(bad.struct), 0, null_columns, null_rows, None, None)
		assert N.V2M_ERR_PRECONDITION == device(c._h, C.byref(bad.struct), 0, cols.data_ptr(), t.data_ptr(), 16, C.byref(count))
		check_forms(c, g, CM.HOSTILE_ROWS, what="after the errors")


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------

def _run(args, cwd=None):
	import subprocess
	assert os.path.exists(CLI), "build the host driver first (__graft_entry__.build())"
	return subprocess.run([CLI] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def cut_fasta(a2m, columns, first=0):
	"""The -s file `a2m` (bytes) with every sequence line cut down to `columns` (absolute; the file's bodies begin at column `first`)."""
	lines = a2m.split(b"\n")
	assert lines[-1] == b"" and len(lines) % 2 == 1
	idx = columns.astype(np.int64) - first
	out = []
	for header, body in zip(lines[0:-1:2], lines[1:-1:2]):
		assert header.startswith(b">")
		out.append(header + b"\n" + np.frombuffer(body, dtype=np.uint8)[idx].tobytes() + b"\n")
	return b"".join(out)


def counts_fields(tsv, columns):
	"""The first two fields of the lines of an --output-column-counts file whose column is among `columns`."""
	keep = set(int(c) for c in columns)
	out = []
	for line in tsv.decode().splitlines():
		if not line.startswith("#") and int(line.split("\t")[0]) in keep:
			out.append("\t".join(line.split("\t")[:2]) + "\n")
	return "".join(out).encode()


def test_cli_haplotypes(v2m, ctx, tmp_path):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	g = oracle.build_variant_graph(fa, vcf, "1")
	vg = v2m.VariantGraph.from_object(g)
	ids, rows = VM.a2m_ids(g)
	sites, pos, a2m, counts = tmp_path / "sites.fa", tmp_path / "pos.tsv", tmp_path / "out.a2m", tmp_path / "counts.tsv"
	common = ["-H", "-r", fa, "-a", vcf, "-c", "1"]
	s, e = 3, min(len(g.ref), 9)
	w = vg.columns_of_reference_range(s - 1, e)
	seen = []
	for extra in ([], ["--snp-sites"], ["--omit-reference"], ["--omit-reference", "--snp-sites"], ["--region=%d-%d" % (s, e)], ["--region=%d-%d" % (s, e), "--omit-reference", "--snp-sites"]):
		k = 1 if "--omit-reference" in extra else 0
		window = w if any(x.startswith("--region") for x in extra) else None
		snp_only = "--snp-sites" in extra
		r = _run(common + ["-s", str(a2m), "--output-variable-sites=" + str(sites), "--output-site-positions=" + str(pos), "--output-column-counts=" + str(counts), "--all-columns", "--verbose"] + extra)
		assert r.returncode == 0, r.stderr.decode()
		columns, data, L = VM.expected(g, rows[k:], window, snp_only)
		# the FASTA is the -s file of the same run cut to the model's columns, and the model's bytes
		assert sites.read_bytes() == cut_fasta(a2m.read_bytes(), columns, window[0] if window else 0) == VM.fasta(ids[k:], data), extra
		# the positions are the first two fields of the matching lines of the column counts of the same run
		assert pos.read_bytes() == counts_fields(counts.read_bytes(), columns) == VM.positions_text(g, columns), extra
		assert ("Variable sites: %d rows, %d columns, %d sites." % (len(rows) - k, L, len(columns))).encode() in r.stderr, r.stderr.decode()
		seen.append(len(columns))
	assert seen[0] > 0 and len(set(seen)) > 1
	# alone, and beside -s --unaligned: the sites are of the aligned form, the A2M file is what it is without the option
	plain = tmp_path / "plain.fa"
	r = _run(common + ["-s", str(plain), "--unaligned"])
	assert r.returncode == 0, r.stderr.decode()
	r = _run(common + ["-s", str(a2m), "--unaligned", "--output-variable-sites=" + str(sites)])
	assert r.returncode == 0, r.stderr.decode()
	columns, data, _ = VM.expected(g, rows)
	assert sites.read_bytes() == VM.fasta(ids, data) and a2m.read_bytes() == plain.read_bytes()
	r = _run(common + ["--output-variable-sites=" + str(sites), "--snp-sites"])
	assert r.returncode == 0, r.stderr.decode()
	assert sites.read_bytes() == VM.fasta(ids, VM.expected(g, rows, snp_only=True)[1])
	# Output.output_variable_sites writes the same bytes
	upload(v2m, ctx, g)
	stream, positions = io.BytesIO(), io.BytesIO()
	info = v2m.HaplotypeOutput(ctx).output_variable_sites(vg, stream, positions=positions)
	assert stream.getvalue() == VM.fasta(ids, data) and positions.getvalue() == VM.positions_text(g, columns) and info["n_sites"] == len(columns)
	stream = io.BytesIO()
	v2m.HaplotypeOutput(ctx, should_output_reference=False, region=(s - 1, e)).output_variable_sites(vg, stream, snp_only=True)
	assert stream.getvalue() == VM.fasta(ids[1:], VM.expected(g, rows[1:], w, True)[1]) and ctx.window_length == g.aligned_length


def test_cli_no_site(v2m, tmp_path):
	"""A window of one column: where it holds no site every sequence line is empty, and so is the positions file."""
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	sites, pos = tmp_path / "sites.fa", tmp_path / "pos.tsv"
	g = oracle.build_variant_graph(fa, vcf, "1")
	ids, rows = VM.a2m_ids(g)
	r = _run(["-H", "-r", fa, "-a", vcf, "-c", "1", "--region=1-1", "--output-variable-sites=" + str(sites), "--output-site-positions=" + str(pos)])
	assert r.returncode == 0, r.stderr.decode()
	columns, data, _ = VM.expected(g, rows, v2m.VariantGraph.from_object(g).columns_of_reference_range(0, 1))
	assert sites.read_bytes() == VM.fasta(ids, data) and pos.read_bytes() == VM.positions_text(g, columns)
	if len(columns) == 0:
		assert sites.read_bytes() == b"".join(b">" + i.encode() + b"\n\n" for i in ids) and pos.read_bytes() == b""


def test_cli_founders(v2m, ctx, tmp_path):
	from vcf2multialign_amd import host
	g = synth.build_case(tmp_path, 44, 40000, 1200, 6)
	fa, vcf = str(tmp_path / "synth.fa"), str(tmp_path / "synth.vcf")
	sites, pos, a2m, counts, cuts_file = tmp_path / "f.fa", tmp_path / "f.pos", tmp_path / "f.a2m", tmp_path / "f.counts", tmp_path / "cuts"
	r = _run(["-F", "3", "-d", "10", "-r", fa, "-a", vcf, "-c", "1", "-s", str(a2m), "--output-variable-sites=" + str(sites), "--output-site-positions=" + str(pos),
		"--output-column-counts=" + str(counts), "-t", str(cuts_file), "--verbose"])
	assert r.returncode == 0, r.stderr.decode()
	cuts, _, _ = host.read_cut_positions(cuts_file)
	lines = r.stdout.decode().split("Matchings:\n")[1].splitlines()[:3]
	assigned = [int(x) for line in lines for x in line.split("\t")[1:]]
	n = len(cuts) - 1
	assert len(assigned) == 3 * n
	rows = [PLOIDY_MAX] + [list(zip(cuts[:-1], assigned[k * n:(k + 1) * n])) for k in range(3)]
	ids = ["REF", "1", "2", "3"]
	columns, data, _ = VM.expected(g, rows)
	assert len(columns) > 0
	assert sites.read_bytes() == cut_fasta(a2m.read_bytes(), columns) == VM.fasta(ids, data)
	assert pos.read_bytes() == counts_fields(counts.read_bytes(), columns) == VM.positions_text(g, columns)
	vg = v2m.VariantGraph.from_object(g)
	w = vg.columns_of_reference_range(999, 30000)
	r = _run(["-F", "3", "-d", "10", "-r", fa, "-a", vcf, "-c", "1", "-s", str(a2m), "--output-variable-sites=" + str(sites), "-p", str(cuts_file), "--omit-reference", "--snp-sites", "--region=1000-30000"])
	assert r.returncode == 0, r.stderr.decode()
	columns_w, data_w, _ = VM.expected(g, rows[1:], w, True)
	assert sites.read_bytes() == cut_fasta(a2m.read_bytes(), columns_w, w[0]) == VM.fasta(ids[1:], data_w)
	upload(v2m, ctx, g)
	stream, positions = io.BytesIO(), io.BytesIO()
	v2m.FounderSequenceGreedyOutput(ctx).output_variable_sites(vg, cuts, assigned, stream, positions=positions)
	assert stream.getvalue() == VM.fasta(ids, data) and positions.getvalue() == VM.positions_text(g, columns)


# ---- the checked build -----------------------------------------------------------------------------------------------------------------------

CHECKED_CORPUS = [
	"tests/test_gpu_variable_sites.py::test_corpus",
	"tests/test_gpu_variable_sites.py::test_exact_pitch_and_no_columns",
	"tests/test_gpu_variable_sites.py::test_too_small_a_pitch",
	"tests/test_gpu_variable_sites.py::test_row_slices",
	"tests/test_gpu_variable_sites.py::test_row_groups_of_the_gather",
	"tests/test_gpu_variable_sites.py::test_row_groups_of_the_gather_in_slices",
	"tests/test_gpu_variable_sites.py::test_sinks",
	"tests/test_gpu_variable_sites.py::test_the_views_are_left_as_they_were",
	"tests/test_gpu_variable_sites.py::test_reference_fixtures",
]


def test_corpus_on_the_checked_build():
	"""The list above with every LDS object, scratch buffer (the site list and the host form's gathered slices among them) and staging
	area poisoned before use (tests/test_gpu_checked_build.py), one run per seed: a site, a column or a byte nobody wrote in this call
	changes the result.  No library is preloaded."""
	from test_gpu_checked_build import SEEDS, run_checked_corpus
	from vcf2multialign_amd import build
	assert os.path.exists(build.CHECKED_LIB_PATH) and os.path.exists(build.CHECKED_HOST_LIB_PATH), "build_native() builds them"
	for seed in SEEDS:   # the second seed only once the first has passed
		rc, out = run_checked_corpus(seed, build.CHECKED_LIB_PATH, build.CHECKED_HOST_LIB_PATH, corpus=CHECKED_CORPUS, timeout=600)
		assert rc == 0, "checked build, seed %s: exit %d\n%s" % (seed, rc, out[-6000:])
		assert " passed" in out and "libv2m_hip_checked.so" in out, out[-3000:]
		print(seed, out.strip().splitlines()[-2])
