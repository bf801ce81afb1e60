"""Context.column_counts / column_counts_device (v2m_column_counts[_device]: column_counts_kernel, count_variable_columns_kernel,
scan_tile_counts_kernel, emit_column_counts_kernel) and --output-column-counts against the model of tests/column_counts_model.py: every
item goes through the device form, the sink form and the sink form with V2M_COUNTS_VARIABLE_ONLY, each held equal to the model.

tests/test_column_counts_host.py asserts, without a GPU, that the hostile-byte graphs hold the bytes and columns they are here for."""

import ctypes as C
import io
import os
import subprocess
import sys

import numpy as np
import pytest

import column_counts_model as CM
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
FIXTURES = [(FIX, "test-1a", "test-1.fa"), (FIX, "test-1b", "test-1.fa"), (FIX, "test-2", "test-2.fa"), (FIX, "test-3", "test-3.fa"), (FIX, "test-4", "test-4.fa"),
	(FOUNDER_FIX, "test-1", "test-1.fa"), (FOUNDER_FIX, "test-2", "test-2.fa"), (FOUNDER_FIX, "test-3", "test-3.fa"), (FOUNDER_FIX, "test-4", "test-4.fa")]
PLOIDY_MAX = CM.PLOIDY_MAX
GUARD = 0x5EEDC0DE
COLUMNS = 4096          # kCountColumns: the columns of a workgroup of column_counts_kernel
RUN = 255               # kCountRun: the rows between two flushes of its byte lanes
MIN_ROWS = 32           # kColumnCountsMinRows: the least rows of a row group
ONE_GROUP = "1000000"   # V2M_COLUMN_COUNTS_ROWS_PER_GROUP: every row in one group -- plain read-modify-writes, a flush every RUN rows


@pytest.fixture(scope="module")
def v2m():
	import vcf2multialign_amd as v
	from vcf2multialign_amd import _native as N
	assert (N.COUNT_COLUMNS, N.COUNT_RUN, N.COLUMN_COUNTS_MIN_ROWS) == (COLUMNS, RUN, MIN_ROWS)
	return v


@pytest.fixture(scope="module")
def ctx(v2m):
	c = v2m.Context(0)
	yield c
	c.close()


def upload(v2m, ctx, g):
	ctx.upload_graph(v2m.VariantGraph.from_object(g), g.ref)


def device_table(ctx, rows, L, extra=8, prefill=None, accumulate=False):
	"""The device form into a table of pitch (L rounded up to 4) + extra: u32[6, pitch] as the call left it."""
	import torch
	pitch = ((L + 3) & ~3) + extra
	if prefill is None:
		prefill = np.full((6, pitch), GUARD, dtype=np.uint32)
	t = torch.from_numpy(prefill.view(np.int32).copy()).cuda()
	assert t.data_ptr() % 16 == 0
	ctx.column_counts_device(rows, t.data_ptr(), pitch, accumulate=accumulate)
	return t.cpu().numpy().view(np.uint32)


def same_counts(got, want, what):
	assert got.shape == want.shape, "%s: shape %s, expected %s" % (what, got.shape, want.shape)
	if not np.array_equal(got, want):
		bad = np.argwhere(got != want)
		i, k = bad[0]
		raise AssertionError("%s: %d of %d counts differ, the first at record %d class %s: got %s, expected %s" % (what, len(bad), want.size, i, CM.CLASSES[k], got[i].tolist(), want[i].tolist()))


def check_forms(ctx, g, rows, window=None, what=""):
	"""The three forms over the view in force (`window` says which that is) against the model."""
	what = what or getattr(g, "name", "graph")
	want = CM.counts(CM.matrix(g, rows, window))
	L, begin = want.shape[0], (window[0] if window else 0)
	assert ctx.window_length == L
	L4 = (L + 3) & ~3
	t = device_table(ctx, rows, L)
	same_counts(t[:, :L].T, want, what + " device form")
	assert (t[:, L:L4] == 0).all(), what + ": the tail up to a multiple of 4 is written as 0"
	assert (t[:, L4:] == GUARD).all(), what + ": nothing beyond the tail is touched"
	cols, c = ctx.column_counts(rows)
	assert cols.dtype == np.uint64 and c.dtype == np.uint32
	assert np.array_equal(cols, np.arange(begin, begin + L, dtype=np.uint64)), what + ": columns are absolute and ascend"
	same_counts(c, want, what + " sink form")
	keep = CM.variable(want, len(rows))
	cols, c = ctx.column_counts(rows, variable_only=True)
	assert np.array_equal(cols, np.flatnonzero(keep).astype(np.uint64) + np.uint64(begin)), what + ": the variable columns"
	same_counts(c, want[keep], what + " variable only")
	return want


def tiny_graph(L):
	"""L columns: a deletion at column 1 and a substitution at the last but one where they fit, reference bytes elsewhere."""
	b = S.Builder(7000 + L)
	b.add_ref(1)
	if L >= 4:
		b.add_site([0], 1)
		b.ref_to(L - 2)
		b.add_site([1], 1)
	b.ref_to(L)
	return b.finish([list(range(b.n_edges)), []], "tiny_%d" % L)


# ---- bytes -----------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shift", CM.HOSTILE_SHIFTS)
def test_hostile_bytes(v2m, ctx, shift):
	g = CM.hostile_graph(shift)
	upload(v2m, ctx, g)
	want = check_forms(ctx, g, CM.HOSTILE_ROWS)
	assert want[28 + shift].tolist() == [0, 0, 0, 0, 0, 6]           # 0x0D is no gap
	assert want[13 + shift:20 + shift].sum() == 0                       # 0x40 0x42 0x60 0xC1 0xE1 0x00 0x0D are of no class
	assert want[shift:8 + shift, 0].tolist() == [9, 0, 0, 9, 9, 0, 0, 9]   # A@@AABBA


def test_every_row_other_is_not_variable(v2m, ctx):
	g = CM.other_graph()
	upload(v2m, ctx, g)
	want = check_forms(ctx, g, [PLOIDY_MAX, 0, 1])
	assert want.sum() == 0
	assert ctx.column_counts([PLOIDY_MAX, 0, 1], variable_only=True)[0].size == 0 and ctx.column_count_blocks == []


def test_literal_dashes_count_as_gaps(v2m, ctx):
	g = M.dash_graph()
	upload(v2m, ctx, g)
	want = check_forms(ctx, g, [PLOIDY_MAX, 0, 1, 2, 3, 4, [(0, 0), (2, 2)]], what="dashes")
	assert want[1, 5] == 7 and want[5, 5] > 0        # the reference's literal '-', and the walk's padding


@pytest.mark.parametrize("where,stem,fasta", FIXTURES, ids=[os.path.basename(f[0])[:7] + "-" + f[1] for f in FIXTURES])
def test_reference_fixtures(v2m, ctx, where, stem, fasta):
	g = oracle.build_variant_graph(os.path.join(where, fasta), os.path.join(where, stem + ".vcf"), "1")
	upload(v2m, ctx, g)
	check_forms(ctx, g, M.rows_with_cuts(g), what=stem)


def test_rows_with_cuts(v2m, ctx):
	sg = S.assemble_graph(5)
	named = S.assemble_rows(5)
	rows = [PLOIDY_MAX, 0, 2] + [list(named[k]) for k in sorted(named)]
	for r in rows:
		assert sg.oracle_body(r) == sg.body(r)
	upload(v2m, ctx, sg.g)
	check_forms(ctx, sg.g, rows, what=sg.name)


# ---- row counts ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("per_group", [None, ONE_GROUP])
def test_row_counts_across_the_byte_lane_flush(v2m, ctx, monkeypatch, per_group):
	"""Default: groups of MIN_ROWS rows that meet with atomics.  One group: the lanes flush after every RUN rows, with plain stores."""
	if per_group:
		monkeypatch.setenv("V2M_COLUMN_COUNTS_ROWS_PER_GROUP", per_group)
	g = CM.hostile_graph(0)
	upload(v2m, ctx, g)
	for n in (1, 2, 254, 255, 256, 257, 510, 511, 512):
		want = check_forms(ctx, g, CM.repeated(CM.HOSTILE_ROWS, n), what="%d rows" % n)
		assert want[0, 0] == n


@pytest.mark.parametrize("per_group", [None, ONE_GROUP])
def test_counts_past_16_bits(v2m, ctx, monkeypatch, per_group):
	if per_group:
		monkeypatch.setenv("V2M_COLUMN_COUNTS_ROWS_PER_GROUP", per_group)
	g = CM.hostile_graph(15)
	assert g.aligned_length == 48
	upload(v2m, ctx, g)
	n = 65793
	want = check_forms(ctx, g, CM.repeated(CM.HOSTILE_ROWS, n), what="65 793 rows")
	assert want[0, 0] == n and want[:, 0].max() > 65535


def test_row_counts_at_the_row_split(v2m, ctx, monkeypatch):
	"""n_rows a multiple of the rows per group and one more: the default split (MIN_ROWS on a one-block view), and forced ones -- 7 rows;
	RUN rows, a group that flushes exactly once; 300 rows, a group that flushes in its middle and leaves 45 or 46 rows."""
	g = CM.hostile_graph(2)
	upload(v2m, ctx, g)
	for forced, counts in ((None, (MIN_ROWS, MIN_ROWS + 1, 2 * MIN_ROWS, 2 * MIN_ROWS + 1)), ("7", (7, 8, 14, 15)), (str(RUN), (2 * RUN, 2 * RUN + 1)), ("300", (600, 601))):
		if forced:
			monkeypatch.setenv("V2M_COLUMN_COUNTS_ROWS_PER_GROUP", forced)
		for n in counts:
			check_forms(ctx, g, CM.repeated(CM.HOSTILE_ROWS, n), what="%d rows in groups of %s" % (n, forced or "the default"))


# ---- view length -----------------------------------------------------------------------------------------------------------------------------

def test_short_views(v2m, ctx):
	"""Every residue of L mod 16 below 16, and the lengths around one and two chunks."""
	for L in list(range(1, 16)) + [16, 17, 31, 32, 33]:
		sg = tiny_graph(L)
		assert sg.length == L
		upload(v2m, ctx, sg.g)
		check_forms(ctx, sg.g, sg.rows + [0], what=sg.name)


@pytest.mark.parametrize("L", [COLUMNS - 1, COLUMNS, COLUMNS + 1, COLUMNS + 15, COLUMNS + 16, COLUMNS + 17, 2 * COLUMNS - 3, 2 * COLUMNS + 5])
def test_views_around_a_workgroups_columns(v2m, ctx, L):
	sg = S.geometry_graph(L)
	upload(v2m, ctx, sg.g)
	check_forms(ctx, sg.g, sg.rows + [1, 0], what=sg.name)


def test_geometry_lengths(v2m, ctx):
	for L in S.geometry_lengths()[:6]:
		sg = S.geometry_graph(L)
		upload(v2m, ctx, sg.g)
		check_forms(ctx, sg.g, sg.rows, what=sg.name)


def test_column_windows(v2m, ctx):
	"""Windows whose begin and whose end take every residue mod 16; the reported columns are absolute; the window stays in force."""
	sg = S.geometry_graph(3 * COLUMNS + 77)
	rows = sg.rows + [0]
	upload(v2m, ctx, sg.g)
	windows = [(COLUMNS - 6 + i, 2 * COLUMNS + 40) for i in range(16)] + [(100, COLUMNS + 100 + i) for i in range(16)]
	windows += [(COLUMNS - 1, COLUMNS), (COLUMNS - 1, COLUMNS + 14), (COLUMNS + 3, COLUMNS + 19), (sg.length - 17, sg.length), (0, 1)]
	assert {b % 16 for b, _ in windows} == set(range(16)) and {e % 16 for _, e in windows} == set(range(16))
	for w in windows:
		ctx.set_column_window(*w)
		check_forms(ctx, sg.g, rows, window=w, what="window %d-%d" % w)
		assert ctx.window_length == w[1] - w[0]
	assert ctx.splice_rows(rows) == [sg.body(r, False, windows[-1]) for r in rows]
	ctx.set_column_window(0, sg.length)
	check_forms(ctx, sg.g, rows, what="whole rows again")


def test_a_window_set_in_force_is_ignored(v2m, ctx):
	sg = S.geometry_graph(COLUMNS + 17)
	rows = sg.rows
	upload(v2m, ctx, sg.g)
	sets = [(5, 900), (COLUMNS - 7, COLUMNS + 9), (3, 4)]
	ctx.set_window_set(sets)
	pieces = ctx.splice_window_set(rows)
	check_forms(ctx, sg.g, rows, what="under a window set")
	w = (COLUMNS - 30, COLUMNS + 2)
	ctx.set_column_window(*w)
	check_forms(ctx, sg.g, rows, window=w, what="under a window set and a window")
	assert ctx.splice_window_set(rows) == pieces and ctx.window_set_size == len(sets)
	assert ctx.splice_rows(rows) == [sg.body(r, False, w) for r in rows]


# ---- the device form's table -----------------------------------------------------------------------------------------------------------------

def test_accumulate(v2m, ctx):
	g = CM.hostile_graph(1)
	upload(v2m, ctx, g)
	rows = CM.repeated(CM.HOSTILE_ROWS, 301)
	L = g.aligned_length
	L4 = (L + 3) & ~3
	assert L4 != L
	want = CM.counts(CM.matrix(g, rows))
	# two half batches into one table
	import torch
	pitch = L4 + 12
	t = torch.from_numpy(np.full((6, pitch), GUARD, dtype=np.uint32).view(np.int32)).cuda()
	ctx.column_counts_device(rows[:150], t.data_ptr(), pitch)
	ctx.column_counts_device(rows[150:], t.data_ptr(), pitch, accumulate=True)
	got = t.cpu().numpy().view(np.uint32)
	same_counts(got[:, :L].T, want, "two halves")
	assert (got[:, L:L4] == 0).all() and (got[:, L4:] == GUARD).all()
	# onto a prefilled table: added to; the tail and everything beyond it are left alone
	prefill = (np.arange(6 * pitch, dtype=np.uint32).reshape(6, pitch) * np.uint32(2654435761)) >> np.uint32(8)
	got = device_table(ctx, rows, L, extra=12, prefill=prefill, accumulate=True)
	same_counts((got[:, :L] - prefill[:, :L]).T, want, "onto a prefilled table")
	assert np.array_equal(got[:, L:], prefill[:, L:])
	# without the flag the same table is overwritten
	got = device_table(ctx, rows, L, extra=12, prefill=prefill)
	same_counts(got[:, :L].T, want, "overwritten")
	assert (got[:, L:L4] == 0).all() and np.array_equal(got[:, L4:], prefill[:, L4:])


# ---- selection -------------------------------------------------------------------------------------------------------------------------------

SELECT_RANGE = 600      # columns per range under V2M_COLUMN_COUNTS_BLOCK_BYTES = 32 * 600: select blocks [0, 256), [256, 512), [512, 600) of each
SELECT_SITES = (0, 255, 256, 511, 512, 599, 600, 601, 855, 856, 1111, 1112, 1199, 1200, 1499)


def selection_graph():
	"""1500 columns with a one-byte deletion at the first and last column of select blocks, either side of the range seams, and at the
	row's first and last column."""
	b = S.Builder(7500)
	for s in SELECT_SITES:
		if s > b.length:
			b.ref_to(s)
		b.add_site([0], 1)
	assert b.length == 1500
	return b.finish([list(range(b.n_edges)), []], "selection")


def test_selection_in_several_blocks(v2m, ctx, monkeypatch):
	monkeypatch.setenv("V2M_COLUMN_COUNTS_BLOCK_BYTES", str(32 * SELECT_RANGE))
	sg = selection_graph()
	upload(v2m, ctx, sg.g)
	rows = sg.rows
	want = check_forms(ctx, sg.g, rows, what=sg.name)
	assert np.flatnonzero(CM.variable(want, len(rows))).tolist() == list(SELECT_SITES)
	ctx.column_counts(rows)
	assert ctx.column_count_blocks == [600, 600, 300]
	ctx.column_counts(rows, variable_only=True)
	assert ctx.column_count_blocks == [6, 7, 2]
	# a range without a variable column gives no call: the blocks of the other ranges arrive
	w = (601, 1400)
	ctx.set_column_window(*w)
	check_forms(ctx, sg.g, rows, window=w, what="selection window")
	ctx.column_counts(rows, variable_only=True)
	assert ctx.column_count_blocks == [7]
	# REF rows only, and one row: no column is variable and the sink is never called
	ctx.set_column_window(0, sg.length)
	for batch in ([PLOIDY_MAX] * 3, [0]):
		check_forms(ctx, sg.g, batch, what="nothing variable")
		assert ctx.column_counts(batch, variable_only=True)[0].size == 0 and ctx.column_count_blocks == []


def test_every_column_variable(v2m, ctx, monkeypatch):
	monkeypatch.setenv("V2M_COLUMN_COUNTS_BLOCK_BYTES", str(32 * 256))
	b = S.Builder(7600)
	b.add_sites(700, 1, 1, 0)
	sg = b.finish([list(range(700)), []], "all_variable")
	upload(v2m, ctx, sg.g)
	want = check_forms(ctx, sg.g, sg.rows, what=sg.name)
	assert CM.variable(want, 3).all()
	ctx.column_counts(sg.rows, variable_only=True)
	assert ctx.column_count_blocks == [256, 256, 188]


def test_a_budget_below_one_record(v2m, ctx, monkeypatch):
	monkeypatch.setenv("V2M_COLUMN_COUNTS_BLOCK_BYTES", "1")
	g = CM.hostile_graph(0)
	upload(v2m, ctx, g)
	check_forms(ctx, g, CM.HOSTILE_ROWS)
	assert ctx.column_count_blocks == [1, 1, 1]


# ---- slices ----------------------------------------------------------------------------------------------------------------------------------

SLICE_CHILD = r"""
import os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np
import torch
import column_counts_model as CM
import seam_graphs as S
import vcf2multialign_amd as v2m
from vcf2multialign_amd import _native as N
sg = S.geometry_graph(4097)
rows = CM.repeated(sg.rows, %(n_rows)d)
out = {}
with v2m.Context(0) as ctx:
	ctx.upload_graph(v2m.VariantGraph.from_object(sg.g), sg.g.ref)
	ctx.profile_enable(True)
	out["cols"], out["counts"] = ctx.column_counts(rows)
	out["launches"] = np.array([ctx.profile_get(N.KERNEL_COLUMN_COUNTS)[0], ctx.profile_get(N.KERNEL_COLUMN_SELECT)[0]])
	out["vcols"], out["vcounts"] = ctx.column_counts(rows, variable_only=True)
	t = torch.zeros((6, 4100), dtype=torch.int32, device="cuda")
	ctx.column_counts_device(rows, t.data_ptr(), 4100)
	out["table"] = t.cpu().numpy().view(np.uint32)
np.savez(%(path)r, **out)
"""


@pytest.mark.parametrize("slot_bytes,n_rows,stage", [("20000", 37, "1"), ("20000", 600, "1"), ("22000", 600, "1"), ("22000", 600, "0")])
def test_several_slices_give_the_one_slice_result(v2m, ctx, tmp_path, slot_bytes, n_rows, stage):
	"""V2M_RING_SLOT_BYTES = 20 000 / 22 000: four / five rows of pitch 4 352 a slice.  Slices that small are one row group each, so the
	byte lanes are carried from slice to slice (the staged form) and widened before they would pass 255 rows: after 252 rows with four
	rows a slice, after exactly 255 with five -- and every row holds the same byte in most columns.  V2M_COLUMN_COUNTS_STAGE = 0: the
	same slices, each flushed into the table."""
	path = str(tmp_path / "sliced.npz")
	env = dict(os.environ, V2M_RING_SLOT_BYTES=slot_bytes, V2M_COLUMN_COUNTS_STAGE=stage)
	r = subprocess.run([sys.executable, "-c", SLICE_CHILD % {"root": ROOT, "path": path, "n_rows": n_rows}], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=env)
	assert r.returncode == 0, r.stdout.decode(errors="replace")[-4000:]
	sliced = np.load(path)
	sg = S.geometry_graph(4097)
	rows = CM.repeated(sg.rows, n_rows)
	upload(v2m, ctx, sg.g)
	want = check_forms(ctx, sg.g, rows, what="one slice")
	per_slice = int(slot_bytes) // 4352
	assert sliced["launches"].tolist() == [(n_rows + per_slice - 1) // per_slice, 1]
	assert want.max() == n_rows and (n_rows < 255 or per_slice * (255 // per_slice) == (255 if per_slice == 5 else 252))
	same_counts(sliced["counts"], want, "in slices")
	cols, c = ctx.column_counts(rows, variable_only=True)
	assert np.array_equal(sliced["vcols"], cols) and np.array_equal(sliced["vcounts"], c) and cols.size
	same_counts(sliced["table"][:, :4097].T, want, "device form in slices")
	assert (sliced["table"][:, 4097:] == 0).all()


def test_profile_ids(v2m, ctx):
	from vcf2multialign_amd import _native as N
	g = CM.hostile_graph(0)
	upload(v2m, ctx, g)
	ctx.profile_enable(True)
	ctx.profile_reset()
	try:
		ctx.column_counts(CM.HOSTILE_ROWS)
		assert ctx.profile_get(N.KERNEL_COLUMN_COUNTS)[0] == 1 and ctx.profile_get(N.KERNEL_COLUMN_SELECT)[0] == 1
		assert ctx.profile_get(N.KERNEL_SPLICE_ALIGNED)[0] >= 1
		with pytest.raises(v2m.V2MError):
			ctx.profile_get(N.KERNEL_LIMIT)
	finally:
		ctx.profile_reset()
		ctx.profile_enable(False)


# ---- the raw ABI -----------------------------------------------------------------------------------------------------------------------------

def test_errors(v2m):
	import torch
	from vcf2multialign_amd import _native as N
	with v2m.Context(0) as c:
		g = CM.hostile_graph(0)
		batch = v2m.RowBatch(CM.HOSTILE_ROWS)
		seen = []
		count = N.COLUMN_COUNTS_SINK_FN(lambda _u, _records, n: seen.append(n) or 0)
		t = torch.zeros(6 * 64 + 4, dtype=torch.int32, device="cuda")
		call, device = c._lib.v2m_column_counts, c._lib.v2m_column_counts_device
		# no graph
		assert N.V2M_ERR_STATE == call(c._h, C.byref(batch.struct), 0, count, None) and not seen
		assert N.V2M_ERR_STATE == device(c._h, C.byref(batch.struct), 0, t.data_ptr(), 64)
		upload(v2m, c, g)
		L = g.aligned_length
		assert L == 33
		assert N.V2M_OK == call(c._h, C.byref(batch.struct), 0, count, None) and seen == [L]
		# flags: only the aligned form exists, and each form has its one flag
		for flags in (0x1, 0x2, 0x4, 0x10, 0x18, 0x20):
			del seen[:]
			assert N.V2M_ERR_INVALID_ARGUMENT == call(c._h, C.byref(batch.struct), flags, count, None) and not seen, hex(flags)
		for flags in (0x1, 0x2, 0x4, 0x8, 0x18, 0x20):
			assert N.V2M_ERR_INVALID_ARGUMENT == device(c._h, C.byref(batch.struct), flags, t.data_ptr(), 64), hex(flags)
		# NULL pointers
		assert N.V2M_ERR_INVALID_ARGUMENT == call(c._h, None, 0, count, None)
		assert N.V2M_ERR_INVALID_ARGUMENT == call(c._h, C.byref(batch.struct), 0, N.COLUMN_COUNTS_SINK_FN(), None)
		assert N.V2M_ERR_INVALID_ARGUMENT == device(c._h, C.byref(batch.struct), 0, None, 64)
		# a misaligned table, a pitch that is no multiple of 4, a short pitch
		for ptr, pitch in ((t.data_ptr() + 4, 64), (t.data_ptr() + 8, 64), (t.data_ptr(), 38), (t.data_ptr(), 32), (t.data_ptr(), 0)):
			assert N.V2M_ERR_INVALID_ARGUMENT == device(c._h, C.byref(batch.struct), 0, ptr, pitch), (ptr % 16, pitch)
		assert (t.cpu().numpy() == 0).all()
		assert N.V2M_OK == device(c._h, C.byref(batch.struct), 0, t.data_ptr(), 36)          # exactly L rounded up to 4
		# no rows: V2M_OK, nothing touched, no call
		empty = v2m.RowBatch([])
		del seen[:]
		assert N.V2M_OK == call(c._h, C.byref(empty.struct), 0, count, None) and not seen
		before = t.cpu().numpy().copy()
		assert N.V2M_OK == device(c._h, C.byref(empty.struct), 0, t.data_ptr(), 36) and np.array_equal(t.cpu().numpy(), before)
		# bad cuts
		bad = v2m.RowBatch([[(2, 0), (1, 1)]])
		assert N.V2M_ERR_PRECONDITION == call(c._h, C.byref(bad.struct), 0, count, None)
		# the sink aborts
		del seen[:]
		abort = N.COLUMN_COUNTS_SINK_FN(lambda _u, _records, n: seen.append(n) or 1)
		assert N.V2M_ERR_SINK == call(c._h, C.byref(batch.struct), 0, abort, None) and seen == [L]
		os.environ["V2M_COLUMN_COUNTS_BLOCK_BYTES"] = str(32 * 10)
		try:
			del seen[:]
			second = N.COLUMN_COUNTS_SINK_FN(lambda _u, _records, n: seen.append(n) or (1 if len(seen) == 2 else 0))
			assert N.V2M_ERR_SINK == call(c._h, C.byref(batch.struct), 0, second, None) and seen == [10, 10]
		finally:
			del os.environ["V2M_COLUMN_COUNTS_BLOCK_BYTES"]
		check_forms(c, g, CM.HOSTILE_ROWS, what="after the errors")


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------

def _run(args, cwd=None):
	assert os.path.exists(CLI), "build the host driver first (__graft_entry__.build())"
	return subprocess.run([CLI] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def test_cli_haplotypes(v2m, ctx, tmp_path):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	g = oracle.build_variant_graph(fa, vcf, "1")
	vg = v2m.VariantGraph.from_object(g)
	copies = list(range(g.total_chromosome_copies))
	tsv, a2m, plain = tmp_path / "out.tsv", tmp_path / "out.fa", tmp_path / "plain.fa"
	common = ["-H", "-r", fa, "-a", vcf, "-c", "1"]
	r = _run(common + ["--output-column-counts=" + str(tsv), "--verbose"])
	assert r.returncode == 0, r.stderr.decode()
	want = CM.file_text(g, [PLOIDY_MAX] + copies)
	assert tsv.read_bytes() == want and want.count(b"\n") > 2
	assert ("Column counts: %d rows, %d columns, %d variable." % (1 + len(copies), g.aligned_length, want.count(b"\n") - 2)).encode() in r.stderr, r.stderr.decode()
	r = _run(common + ["--output-column-counts=" + str(tsv), "--omit-reference"])
	assert r.returncode == 0, r.stderr.decode()
	assert tsv.read_bytes() == CM.file_text(g, copies)
	r = _run(common + ["--output-column-counts=" + str(tsv), "--all-columns", "--verbose"])
	assert r.returncode == 0, r.stderr.decode()
	assert tsv.read_bytes() == CM.file_text(g, [PLOIDY_MAX] + copies, all_columns=True)
	assert ("%d columns, %d variable." % (g.aligned_length, want.count(b"\n") - 2)).encode() in r.stderr
	# --region restricts the columns, which stay absolute
	s, e = 3, min(len(g.ref), 9)
	w = vg.columns_of_reference_range(s - 1, e)
	for extra in ([], ["--all-columns"], ["--omit-reference", "--all-columns"]):
		r = _run(common + ["--output-column-counts=" + str(tsv), "--region=%d-%d" % (s, e)] + extra)
		assert r.returncode == 0, r.stderr.decode()
		rows = copies if "--omit-reference" in extra else [PLOIDY_MAX] + copies
		assert tsv.read_bytes() == CM.file_text(g, rows, window=w, all_columns="--all-columns" in extra)
	# beside -s --unaligned: the counts are of the aligned form, the A2M file is what it is without the option
	r = _run(common + ["-s", str(plain), "--unaligned"])
	assert r.returncode == 0, r.stderr.decode()
	r = _run(common + ["-s", str(a2m), "--unaligned", "--output-column-counts=" + str(tsv), "--output-chain=" + str(tmp_path / "c.chain"), "--output-paf=" + str(tmp_path / "c.paf")])
	assert r.returncode == 0, r.stderr.decode()
	assert tsv.read_bytes() == want and a2m.read_bytes() == plain.read_bytes()
	assert (tmp_path / "c.chain").read_bytes() == M.haplotype_chains(g)
	# Output.output_column_counts writes the same bytes through the host library's formatter
	upload(v2m, ctx, g)
	stream = io.BytesIO()
	assert v2m.HaplotypeOutput(ctx).output_column_counts(vg, stream) == want.count(b"\n") - 2
	assert stream.getvalue() == want
	stream = io.BytesIO()
	v2m.HaplotypeOutput(ctx, should_output_reference=False, region=(s - 1, e)).output_column_counts(vg, stream, all_columns=True)
	assert stream.getvalue() == CM.file_text(g, copies, window=w, all_columns=True) and ctx.window_length == g.aligned_length


def test_cli_founders(v2m, ctx, tmp_path):
	from vcf2multialign_amd import host
	g = synth.build_case(tmp_path, 44, 40000, 1200, 6)
	fa, vcf = str(tmp_path / "synth.fa"), str(tmp_path / "synth.vcf")
	tsv, cuts_file = tmp_path / "f.tsv", tmp_path / "cuts"
	r = _run(["-F", "3", "-d", "10", "-r", fa, "-a", vcf, "-c", "1", "--output-column-counts=" + str(tsv), "-t", str(cuts_file), "--verbose"])
	assert r.returncode == 0, r.stderr.decode()
	cuts, _, _ = host.read_cut_positions(cuts_file)
	lines = r.stdout.decode().split("Matchings:\n")[1].splitlines()[:3]
	assigned = [int(x) for line in lines for x in line.split("\t")[1:]]
	n = len(cuts) - 1
	assert len(assigned) == 3 * n
	rows = [PLOIDY_MAX] + [list(zip(cuts[:-1], assigned[k * n:(k + 1) * n])) for k in range(3)]
	want = CM.file_text(g, rows)
	assert tsv.read_bytes() == want and want.count(b"\n") > 10
	r = _run(["-F", "3", "-d", "10", "-r", fa, "-a", vcf, "-c", "1", "--output-column-counts=" + str(tsv), "-p", str(cuts_file), "--omit-reference", "--region=1000-30000"])
	assert r.returncode == 0, r.stderr.decode()
	vg = v2m.VariantGraph.from_object(g)
	assert tsv.read_bytes() == CM.file_text(g, rows[1:], window=vg.columns_of_reference_range(999, 30000))
	upload(v2m, ctx, g)
	stream = io.BytesIO()
	v2m.FounderSequenceGreedyOutput(ctx).output_column_counts(vg, cuts, assigned, stream)
	assert stream.getvalue() == want


def test_cli_refusals(tmp_path):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	bed = tmp_path / "r.bed"
	bed.write_text("1\t0\t4\n")
	common = ["-H", "-r", fa, "-a", vcf, "-c", "1"]
	for extra, what in ((["--regions-file=" + str(bed)], "--regions-file"), (["--device=0,0"], "more than one --device entry")):
		r = _run(common + ["--output-column-counts=" + str(tmp_path / "x.tsv")] + extra, cwd=str(tmp_path))
		assert r.returncode != 0
		assert ("ERROR: --output-column-counts cannot be combined with %s.\n" % what).encode() in r.stderr, r.stderr.decode()
	r = _run(common + ["--all-columns", "-s", str(tmp_path / "x.a2m")])
	assert r.returncode != 0 and b"ERROR: --all-columns requires --output-column-counts.\n" in r.stderr
	assert not (tmp_path / "x.tsv").exists() and not (tmp_path / "x.a2m").exists()


# ---- the checked build -----------------------------------------------------------------------------------------------------------------------

CHECKED_CORPUS = [
	"tests/test_gpu_column_counts.py::test_hostile_bytes",
	"tests/test_gpu_column_counts.py::test_literal_dashes_count_as_gaps",
	"tests/test_gpu_column_counts.py::test_reference_fixtures",
	"tests/test_gpu_column_counts.py::test_row_counts_across_the_byte_lane_flush",
	"tests/test_gpu_column_counts.py::test_row_counts_at_the_row_split",
	"tests/test_gpu_column_counts.py::test_short_views",
	"tests/test_gpu_column_counts.py::test_views_around_a_workgroups_columns",
	"tests/test_gpu_column_counts.py::test_column_windows",
	"tests/test_gpu_column_counts.py::test_accumulate",
	"tests/test_gpu_column_counts.py::test_selection_in_several_blocks",
	"tests/test_gpu_column_counts.py::test_every_column_variable",
	"tests/test_gpu_column_counts.py::test_several_slices_give_the_one_slice_result[22000-600-1]",   # the staged form: its child inherits the checked libraries
]


def test_corpus_on_the_checked_build():
	"""The list above with every LDS object, scratch buffer and staging area poisoned before use (tests/test_gpu_checked_build.py), one run per
	seed: a count read from a table, a block count or a record nobody wrote in this call changes the result."""
	from test_gpu_checked_build import SEEDS, run_checked_corpus
	from vcf2multialign_amd import build
	assert os.path.exists(build.CHECKED_LIB_PATH) and os.path.exists(build.CHECKED_HOST_LIB_PATH), "build_native() builds them"
	for seed in SEEDS:   # the second seed only once the first has passed
		rc, out = run_checked_corpus(seed, build.CHECKED_LIB_PATH, build.CHECKED_HOST_LIB_PATH, corpus=CHECKED_CORPUS, timeout=600)
		assert rc == 0, "checked build, seed %s: exit %d\n%s" % (seed, rc, out[-6000:])
		assert " passed" in out and "libv2m_hip_checked.so" in out, out[-3000:]
		print(seed, out.strip().splitlines()[-2])
