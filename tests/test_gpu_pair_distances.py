"""Context.pair_distances / pair_distances_device (v2m_pair_distances[_device]: the column counts' kernels, emit_site_columns_kernel,
pack_sites_kernel, pair_distances_kernel) and --output-distances against the model of tests/pair_distances_model.py: every item goes
through the host form and through the device form with a pitch beyond n, under both definitions, each held equal to the model entry for
entry.

tests/test_pair_distances_host.py asserts, without a GPU, that the corpus holds the row counts, site counts, windows and classes it is
here for, and that the model's matrix over all columns equals the one over the variable columns alone."""

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

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")
PLOIDY_MAX = PM.PLOIDY_MAX
GUARD = 0x5EEDC0DE
T, CHUNK = PM.kernel_constants()     # kPairTile, kPairChunkWords
CHUNK_SITES = 64 * CHUNK


@pytest.fixture(scope="module")
def v2m():
	import vcf2multialign_amd as v
	from vcf2multialign_amd import _native as N
	assert (N.PAIR_TILE, N.PAIR_CHUNK_WORDS) == (T, CHUNK)
	return v


@pytest.fixture(scope="module")
def ctx(v2m):
	c = v2m.Context(0)
	yield c
	c.close()


def upload(v2m, ctx, g):
	ctx.upload_graph(v2m.VariantGraph.from_object(g), g.ref)


def pattern(n, pitch):
	"""A pre-fill no entry of which is a plausible distance."""
	return ((np.arange(n * pitch, dtype=np.uint64) * 2654435761 + GUARD) & 0xFFFFFFFF).astype(np.uint32).reshape(n, pitch) | np.uint32(0x80000000)


def device_matrix(ctx, rows, acgt_only, extra=8):
	"""The device form into a buffer of pitch (n rounded up to 4) + extra, pre-filled: (u32[n, pitch] as the call left it, the pre-fill)."""
	import torch
	n = len(rows)
	pitch = ((n + 3) & ~3) + extra
	fill = pattern(max(n, 1), pitch)
	t = torch.from_numpy(fill.view(np.int32).copy()).cuda()
	assert t.data_ptr() % 16 == 0
	ctx.pair_distances_device(rows, t.data_ptr(), pitch, acgt_only=acgt_only)
	return t.cpu().numpy().view(np.uint32)[:n], fill[:n]


def same_matrix(got, want, what):
	assert got.shape == want.shape and got.dtype == np.uint32, "%s: shape %s %s, expected %s" % (what, got.shape, got.dtype, want.shape)
	if not np.array_equal(got, want):
		bad = np.argwhere(got != want)
		i, j = bad[0]
		raise AssertionError("%s: %d of %d entries differ, the first at [%d][%d]: got %d, expected %d" % (what, len(bad), want.size, i, j, got[i, j], want[i, j]))


def check_forms(ctx, g, rows, window=None, what="", passes=None):
	"""Both forms under both definitions over the view in force (`window` says which that is) against the model; returns the info."""
	what = what or getattr(g, "name", "graph")
	n = len(rows)
	info = None
	for acgt in (False, True):
		want, V, L = PM.expected(g, rows, window, acgt)
		assert ctx.window_length == L
		got, info = ctx.pair_distances(rows, acgt_only=acgt, info=True)
		same_matrix(got, want, "%s host form%s" % (what, " acgt" if acgt else ""))
		assert (info["n_sites"], info["n_columns"]) == (V, L), (what, info)
		assert info["n_passes"] == (passes if passes is not None and V else 1 if V else 0), (what, info)
		assert info["counts_ms"] == info["pack_ms"] == info["pairs_ms"] == 0.0      # profiling is off
		buf, fill = device_matrix(ctx, rows, acgt)
		same_matrix(np.ascontiguousarray(buf[:, :n]), want, "%s device form%s" % (what, " acgt" if acgt else ""))
		assert np.array_equal(buf[:, n:], fill[:, n:]), what + ": nothing beyond column n of a row is touched"
	return info


# ---- the corpus ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("item", PM.corpus(), ids=[i.name for i in PM.corpus()])
def test_corpus(v2m, ctx, item):
	upload(v2m, ctx, item.g)
	if item.window:
		ctx.set_column_window(*item.window)
	info = check_forms(ctx, item.g, item.rows, item.window, item.name)
	if item.window:
		assert ctx.window_length == item.window[1] - item.window[0]
	assert info["n_sites"] == len(ctx.column_counts(item.rows, variable_only=True)[0])


def split_of(chunks, parts):
	"""The chunks of each part of a launch, by the library's rule (csrc/v2m_hip.hip: pair_chunks_per_part and the launch): parts of
	ceil(chunks / min(parts, chunks)) chunks, the last one the remainder."""
	per_part = -(-chunks // max(1, min(parts, chunks)))
	return [min(per_part, chunks - b) for b in range(0, chunks, per_part)]


def test_site_split_and_single_part(v2m, ctx, monkeypatch):
	"""Seven chunks of sites (six and five sites more).  By default, with few rows, every chunk is a part of its own and the parts meet
	by atomicAdd on the zeroed matrix.  Two parts asked for: 4 + 3 chunks; four: 2 + 2 + 2 + 1 -- the last part holds the remainder,
	under one tile pair and under the six of three tiles of rows, where both edge tiles are in the launch.  One part: plain stores after
	a loop over all seven chunks, the same with four tiles of rows (one chunk, the plain path by default, is among the corpus)."""
	V = 6 * CHUNK_SITES + 5
	chunks = -(-V // CHUNK_SITES)
	assert chunks == 7 and split_of(chunks, 2) == [4, 3] and split_of(chunks, 4) == [2, 2, 2, 1] and split_of(chunks, 1) == [7] and split_of(chunks, 1024) == [1] * 7
	g = PM.sites_graph_of(V)
	upload(v2m, ctx, g)
	assert PM.expected(g, PM.SITE_ROWS)[1] == V
	three_tiles = CM.repeated(PM.SITE_ROWS[:8], 2 * T + 1)
	for forced in (None, "2", "4", "1"):
		if forced:
			monkeypatch.setenv("V2M_PAIR_DISTANCES_PARTS", forced)
		check_forms(ctx, g, PM.SITE_ROWS, what="%s parts" % (forced or "default"))
		check_forms(ctx, g, three_tiles, what="%s parts, three tiles" % (forced or "default"))
	check_forms(ctx, g, CM.repeated(PM.SITE_ROWS[:8], 3 * T + 1), what="one part, four tiles")
	# five chunks in two parts: 3 + 2
	monkeypatch.setenv("V2M_PAIR_DISTANCES_PARTS", "2")
	g5 = PM.sites_graph_of(4 * CHUNK_SITES + 70)
	assert -(-(4 * CHUNK_SITES + 70) // CHUNK_SITES) == 5 and split_of(5, 2) == [3, 2]
	upload(v2m, ctx, g5)
	check_forms(ctx, g5, PM.SITE_ROWS, what="five chunks in two parts")


def test_row_slices(v2m, ctx, monkeypatch):
	"""V2M_RING_SLOT_BYTES small enough for four slices of three rows and one of one: both passes over the rows go slice by slice, and a
	slice's rows land at their own place in the planes."""
	g = PM.sites_graph_of(CHUNK_SITES + 65)
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
		d, info = ctx.pair_distances(rows, info=True)
		launches = ctx.profile_get(N.KERNEL_COLUMN_COUNTS)[0]
		assert launches == 5, launches      # four slices of three rows and a remainder of one
		assert info["counts_ms"] > 0 and info["pack_ms"] > 0 and info["pairs_ms"] > 0
	finally:
		ctx.profile_reset()
		ctx.profile_enable(False)
	same_matrix(d, PM.expected(g, rows)[0], "in slices, profiling on")
	assert check_forms(ctx, g, rows, what="in slices") == want


def test_passes(v2m, ctx, monkeypatch):
	"""V2M_PAIR_DISTANCES_PLANE_BYTES for two chunks of planes a pass: seven chunks of sites make three passes of two and one of one,
	each adding into the matrix."""
	g = PM.sites_graph_of(6 * CHUNK_SITES + 5)
	upload(v2m, ctx, g)
	rows = PM.SITE_ROWS
	chunk_bytes = CHUNK * 3 * T * 8            # the planes of one chunk of sites for up to T rows
	assert check_forms(ctx, g, rows, what="one pass")["n_passes"] == 1
	monkeypatch.setenv("V2M_PAIR_DISTANCES_PLANE_BYTES", str(2 * chunk_bytes + 100))
	assert check_forms(ctx, g, rows, what="four passes", passes=4)["n_passes"] == 4
	monkeypatch.setenv("V2M_PAIR_DISTANCES_PLANE_BYTES", "1")
	assert check_forms(ctx, g, rows, what="a budget below one chunk", passes=7)["n_passes"] == 7
	# more rows: the chunk of T + 1 rows takes twice the bytes
	monkeypatch.setenv("V2M_PAIR_DISTANCES_PLANE_BYTES", str(6 * chunk_bytes))
	check_forms(ctx, g, CM.repeated(rows[:8], T + 1), what="T + 1 rows in passes", passes=3)


# ---- rows that all differ ----------------------------------------------------------------------------------------------------------------------
#
# The rows of the corpus above repeat with period 16 or 8, which a row group, the halves of pair_row() and a tile are multiples of; in the
# items of PM.distinct_items() no two rows are equal, and tests/test_pair_distances_host.py asserts that a row group written one group off,
# two rows, halves or tiles exchanged each change their expected matrices.

DISTINCT = PM.distinct_items()


@pytest.mark.parametrize("item", DISTINCT, ids=[i.name for i in DISTINCT])
def test_distinct_rows(v2m, ctx, item):
	"""4, 9 and 17 tiles of rows that all differ: 10, 45 and 153 tile pairs decoded from blockIdx.x, every entry held to the model."""
	upload(v2m, ctx, item.g)
	check_forms(ctx, item.g, item.rows, what=item.name)


def test_distinct_rows_in_parts_and_passes(v2m, ctx, monkeypatch):
	"""The 3 T + 1 rows over three chunks of sites: one part (plain stores), two parts (atomics on the zeroed matrix), and a plane budget
	of two chunks (two passes)."""
	item = PM.distinct_item(3 * T + 1)
	upload(v2m, ctx, item.g)
	assert -(-PM.variable_columns(item.g) // CHUNK_SITES) == 3 and split_of(3, 2) == [2, 1]
	for forced in ("1", "2"):
		monkeypatch.setenv("V2M_PAIR_DISTANCES_PARTS", forced)
		check_forms(ctx, item.g, item.rows, what="%s, %s parts" % (item.name, forced))
	monkeypatch.delenv("V2M_PAIR_DISTANCES_PARTS")
	chunk_bytes = CHUNK * 3 * 4 * T * 8            # the planes of one chunk of sites for four tiles of rows
	monkeypatch.setenv("V2M_PAIR_DISTANCES_PLANE_BYTES", str(2 * chunk_bytes))
	check_forms(ctx, item.g, item.rows, what=item.name + ", two passes", passes=2)


# ---- row groups above the floor ----------------------------------------------------------------------------------------------------------------

# V2M_SITE_ROWS_PER_GROUP over the 3 T + 1 distinct rows: a row a group; one unrolled trip of four and a tail row in every group, the groups
# starting at every residue mod 4; a tail of two, the groups starting at the even residues; 67; exactly one group; one group of more rows than there are (what the rule gives when the
# site blocks alone fill the device)
SITE_ROWS_PER_GROUP = (1, 5, 18, 67, 3 * T + 1, 1000000)


@pytest.mark.parametrize("per_group", SITE_ROWS_PER_GROUP)
def test_row_groups_of_the_pack(v2m, ctx, monkeypatch, per_group):
	"""pack_sites_kernel with groups of other sizes than the rule's floor of 16, over two chunks of sites and five more."""
	item = PM.distinct_item(3 * T + 1)
	assert PM.variable_columns(item.g) == 2 * CHUNK_SITES + 5 and {b % 4 for b in range(0, len(item.rows), 5)} == {0, 1, 2, 3}
	upload(v2m, ctx, item.g)
	monkeypatch.setenv("V2M_SITE_ROWS_PER_GROUP", str(per_group))
	check_forms(ctx, item.g, item.rows, what="%s, %d rows a group" % (item.name, per_group))


@pytest.mark.parametrize("per_group", (18, 1000000))
def test_row_groups_of_the_pack_in_slices(v2m, ctx, monkeypatch, per_group):
	"""The same under slices of 50 rows: a slice's first row is neither the batch's first nor a multiple of the group."""
	item = PM.distinct_item(3 * T + 1)
	upload(v2m, ctx, item.g)
	pitch = int(ctx.min_row_pitch)
	monkeypatch.setenv("V2M_RING_SLOT_BYTES", str(50 * pitch + pitch // 2))
	monkeypatch.setenv("V2M_SITE_ROWS_PER_GROUP", str(per_group))
	from vcf2multialign_amd import _native as N
	ctx.profile_enable(True)
	ctx.profile_reset()
	try:
		d = ctx.pair_distances(item.rows)
		launches = ctx.profile_get(N.KERNEL_COLUMN_COUNTS)[0]
	finally:
		ctx.profile_reset()
		ctx.profile_enable(False)
	assert launches == 4, launches      # three slices of 50 rows and one of 43
	same_matrix(d, PM.expected(item.g, item.rows)[0], "in slices, profiling on")
	check_forms(ctx, item.g, item.rows, what="%s, %d rows a group, slices of 50 rows" % (item.name, per_group))


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
		host_buf = np.full((n, n), GUARD, dtype=np.uint32)
		info = N.PairDistancesInfo()
		t = torch.full((n * 16 + 4,), 7, dtype=torch.int32, device="cuda")
		call, device = c._lib.v2m_pair_distances, c._lib.v2m_pair_distances_device
		# no graph
		assert N.V2M_ERR_STATE == call(c._h, C.byref(batch.struct), 0, host_buf.ctypes.data, C.byref(info))
		assert N.V2M_ERR_STATE == device(c._h, C.byref(batch.struct), 0, t.data_ptr(), 16)
		upload(v2m, c, g)
		# flags: the one bit, and none of the other row calls'
		for flags in (0x1, 0x2, 0x4, 0x8, 0x10, 0x21, 0x30, 0x40, 0x80000000):
			assert N.V2M_ERR_INVALID_ARGUMENT == call(c._h, C.byref(batch.struct), flags, host_buf.ctypes.data, None), hex(flags)
			assert N.V2M_ERR_INVALID_ARGUMENT == device(c._h, C.byref(batch.struct), flags, t.data_ptr(), 16), hex(flags)
		# NULL pointers
		assert N.V2M_ERR_INVALID_ARGUMENT == call(c._h, None, 0, host_buf.ctypes.data, None)
		assert N.V2M_ERR_INVALID_ARGUMENT == call(c._h, C.byref(batch.struct), 0, None, None)
		assert N.V2M_ERR_INVALID_ARGUMENT == device(c._h, None, 0, t.data_ptr(), 16)
		assert N.V2M_ERR_INVALID_ARGUMENT == device(c._h, C.byref(batch.struct), 0, None, 16)
		# a misaligned matrix, a pitch that is no multiple of 4, a pitch below n
		for ptr, pitch in ((t.data_ptr() + 4, 16), (t.data_ptr() + 8, 16), (t.data_ptr(), 14), (t.data_ptr(), 8), (t.data_ptr(), 0)):
			assert N.V2M_ERR_INVALID_ARGUMENT == device(c._h, C.byref(batch.struct), 0, ptr, pitch), (ptr % 16, pitch)
		assert (t.cpu().numpy() == 7).all() and (host_buf == GUARD).all()
		assert N.V2M_OK == device(c._h, C.byref(batch.struct), 0, t.data_ptr(), 12)          # exactly n rounded up to 4
		assert np.array_equal(t.cpu().numpy().view(np.uint32)[:n * 12].reshape(n, 12)[:, :n], PM.expected(g, CM.HOSTILE_ROWS)[0])
		# the info may be NULL
		assert N.V2M_OK == call(c._h, C.byref(batch.struct), N.DIST_ACGT_ONLY, host_buf.ctypes.data, None)
		assert np.array_equal(host_buf, PM.expected(g, CM.HOSTILE_ROWS, acgt_only=True)[0])
		# no rows: V2M_OK, nothing touched
		empty = v2m.RowBatch([])
		host_buf[:] = GUARD
		before = t.cpu().numpy().copy()
		info.n_columns = 77
		assert N.V2M_OK == call(c._h, C.byref(empty.struct), 0, host_buf.ctypes.data, C.byref(info)) and (host_buf == GUARD).all() and info.n_columns == 77
		assert N.V2M_OK == device(c._h, C.byref(empty.struct), 0, t.data_ptr(), 0) and np.array_equal(t.cpu().numpy(), before)
		assert c.pair_distances([]).shape == (0, 0)
		# more than V2M_PAIR_DISTANCES_MAX_ROWS rows: refused before anything is allocated or queued -- the matrix pointer is never used
		many = v2m.RowBatch(CM.repeated(CM.HOSTILE_ROWS, N.PAIR_DISTANCES_MAX_ROWS + 1))
		assert N.V2M_ERR_UNSUPPORTED == call(c._h, C.byref(many.struct), 0, host_buf.ctypes.data, None)
		assert "V2M_PAIR_DISTANCES_MAX_ROWS = 32768" in c._lib.v2m_last_error(c._h).decode()
		assert N.V2M_ERR_UNSUPPORTED == device(c._h, C.byref(many.struct), 0, t.data_ptr(), 32772)
		assert "32768" in c._lib.v2m_last_error(c._h).decode() and (host_buf == GUARD).all() and np.array_equal(t.cpu().numpy(), before)
		# bad cuts
		bad = v2m.RowBatch([0, [(2, 0), (1, 1)]])
		assert N.V2M_ERR_PRECONDITION == call(c._h, C.byref(bad.struct), 0, host_buf.ctypes.data, None)
		assert N.V2M_ERR_PRECONDITION == device(c._h, C.byref(bad.struct), 0, t.data_ptr(), 16)
		check_forms(c, g, CM.HOSTILE_ROWS, what="after the errors")


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------

def _run(args, cwd=None):
	import subprocess
	assert os.path.exists(CLI), "build the host driver first (__graft_entry__.build())"
	return subprocess.run([CLI] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def test_cli_haplotypes(v2m, ctx, tmp_path):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	g = oracle.build_variant_graph(fa, vcf, "1")
	vg = v2m.VariantGraph.from_object(g)
	ids, rows = PM.haplotype_ids(g)
	tsv, a2m, plain, paf = tmp_path / "out.tsv", tmp_path / "out.fa", tmp_path / "plain.fa", tmp_path / "out.paf"
	common = ["-H", "-r", fa, "-a", vcf, "-c", "1"]
	r = _run(common + ["--output-distances=" + str(tsv), "--verbose"])
	assert r.returncode == 0, r.stderr.decode()
	want = PM.file_text(g, ids, rows)
	d, V, L = PM.expected(g, rows)
	assert tsv.read_bytes() == want and V > 0 and d.any()
	assert ("Distances: %d rows, %d columns, %d sites, 1 passes." % (len(rows), L, V)).encode() in r.stderr, r.stderr.decode()
	r = _run(common + ["--output-distances=" + str(tsv), "--acgt-only"])
	assert r.returncode == 0, r.stderr.decode()
	assert tsv.read_bytes() == PM.file_text(g, ids, rows, acgt_only=True)
	r = _run(common + ["--output-distances=" + str(tsv), "--omit-reference"])
	assert r.returncode == 0, r.stderr.decode()
	assert tsv.read_bytes() == PM.file_text(g, ids[1:], rows[1:])
	# --region restricts the columns
	s, e = 3, min(len(g.ref), 9)
	w = vg.columns_of_reference_range(s - 1, e)
	for extra in ([], ["--acgt-only"], ["--omit-reference", "--acgt-only"]):
		r = _run(common + ["--output-distances=" + str(tsv), "--region=%d-%d" % (s, e)] + extra)
		assert r.returncode == 0, r.stderr.decode()
		k = 1 if "--omit-reference" in extra else 0
		assert tsv.read_bytes() == PM.file_text(g, ids[k:], rows[k:], window=w, acgt_only="--acgt-only" in extra)
	# beside -s --unaligned and --output-paf: the distances are of the aligned form, the A2M file is what it is without the option, and
	# the names are the PAF's query names
	r = _run(common + ["-s", str(plain), "--unaligned"])
	assert r.returncode == 0, r.stderr.decode()
	r = _run(common + ["-s", str(a2m), "--unaligned", "--output-distances=" + str(tsv), "--output-paf=" + str(paf)])
	assert r.returncode == 0, r.stderr.decode()
	assert tsv.read_bytes() == want and a2m.read_bytes() == plain.read_bytes()
	assert [line.split("\t")[0] for line in paf.read_text().splitlines()] == ids[1:]
	# beside -s: the A2M equals the golden
	r = _run(common + ["-s", str(a2m), "--output-distances=" + str(tsv)])
	assert r.returncode == 0, r.stderr.decode()
	with open(os.path.join(HERE, "golden", "derived", "test-4.haplotypes.a2m"), "rb") as f:
		assert a2m.read_bytes() == f.read()
	assert tsv.read_bytes() == want
	# Output.output_distances writes the same bytes through the host library's formatter
	upload(v2m, ctx, g)
	stream = io.BytesIO()
	info = v2m.HaplotypeOutput(ctx).output_distances(vg, stream)
	assert stream.getvalue() == want and info["n_sites"] == V
	stream = io.BytesIO()
	v2m.HaplotypeOutput(ctx, should_output_reference=False, region=(s - 1, e)).output_distances(vg, stream, acgt_only=True)
	assert stream.getvalue() == PM.file_text(g, ids[1:], rows[1:], window=w, acgt_only=True) and ctx.window_length == g.aligned_length


def test_cli_founders(v2m, ctx, tmp_path):
	from vcf2multialign_amd import host
	g = synth.build_case(tmp_path, 44, 40000, 1200, 6)
	fa, vcf = str(tmp_path / "synth.fa"), str(tmp_path / "synth.vcf")
	tsv, cuts_file = tmp_path / "f.tsv", tmp_path / "cuts"
	r = _run(["-F", "3", "-d", "10", "-r", fa, "-a", vcf, "-c", "1", "--output-distances=" + str(tsv), "-t", str(cuts_file), "--verbose"])
	assert r.returncode == 0, r.stderr.decode()
	cuts, _, _ = host.read_cut_positions(cuts_file)
	lines = r.stdout.decode().split("Matchings:\n")[1].splitlines()[:3]
	assigned = [int(x) for line in lines for x in line.split("\t")[1:]]
	n = len(cuts) - 1
	assert len(assigned) == 3 * n
	rows = [PLOIDY_MAX] + [list(zip(cuts[:-1], assigned[k * n:(k + 1) * n])) for k in range(3)]
	ids = ["REF", "1", "2", "3"]
	want = PM.file_text(g, ids, rows)
	assert tsv.read_bytes() == want and PM.expected(g, rows)[0].any()
	r = _run(["-F", "3", "-d", "10", "-r", fa, "-a", vcf, "-c", "1", "--output-distances=" + str(tsv), "-p", str(cuts_file), "--omit-reference", "--acgt-only", "--region=1000-30000"])
	assert r.returncode == 0, r.stderr.decode()
	vg = v2m.VariantGraph.from_object(g)
	assert tsv.read_bytes() == PM.file_text(g, ids[1:], rows[1:], window=vg.columns_of_reference_range(999, 30000), acgt_only=True)
	upload(v2m, ctx, g)
	stream = io.BytesIO()
	v2m.FounderSequenceGreedyOutput(ctx).output_distances(vg, cuts, assigned, stream)
	assert stream.getvalue() == want


def test_cli_refusals(tmp_path):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	bed = tmp_path / "r.bed"
	bed.write_text("1\t0\t4\n")
	common = ["-H", "-r", fa, "-a", vcf, "-c", "1"]
	for extra, what in ((["--regions-file=" + str(bed)], "--regions-file"), (["--device=0,0"], "more than one --device entry")):
		r = _run(common + ["--output-distances=" + str(tmp_path / "x.tsv")] + extra, cwd=str(tmp_path))
		assert r.returncode != 0
		assert ("ERROR: --output-distances cannot be combined with %s.\n" % what).encode() in r.stderr, r.stderr.decode()
	r = _run(common + ["--acgt-only", "-s", str(tmp_path / "x.a2m")])
	assert r.returncode != 0 and b"ERROR: --acgt-only requires --output-distances.\n" in r.stderr
	assert not (tmp_path / "x.tsv").exists() and not (tmp_path / "x.a2m").exists()


# ---- the checked build -----------------------------------------------------------------------------------------------------------------------

CHECKED_CORPUS = [
	"tests/test_gpu_pair_distances.py::test_corpus",
	"tests/test_gpu_pair_distances.py::test_site_split_and_single_part",
	"tests/test_gpu_pair_distances.py::test_row_slices",
	"tests/test_gpu_pair_distances.py::test_passes",
	"tests/test_gpu_pair_distances.py::test_distinct_rows",
	"tests/test_gpu_pair_distances.py::test_distinct_rows_in_parts_and_passes",
	"tests/test_gpu_pair_distances.py::test_row_groups_of_the_pack",
	"tests/test_gpu_pair_distances.py::test_row_groups_of_the_pack_in_slices",
	"tests/test_gpu_pair_distances.py::test_the_views_are_left_as_they_were",
	"tests/test_gpu_pair_distances.py::test_reference_fixtures",
]


def test_corpus_on_the_checked_build():
	"""The list above with every LDS object, scratch buffer (the planes, the site list and the host form's matrix among them) and staging
	area poisoned before use (tests/test_gpu_checked_build.py), one run per seed: a plane word, a site or a matrix entry nobody wrote in
	this call changes the result.  No library is preloaded."""
	from test_gpu_checked_build import SEEDS, run_checked_corpus
	from vcf2multialign_amd import build
	assert os.path.exists(build.CHECKED_LIB_PATH) and os.path.exists(build.CHECKED_HOST_LIB_PATH), "build_native() builds them"
	for seed in SEEDS:   # the second seed only once the first has passed
		rc, out = run_checked_corpus(seed, build.CHECKED_LIB_PATH, build.CHECKED_HOST_LIB_PATH, corpus=CHECKED_CORPUS, timeout=600)
		assert rc == 0, "checked build, seed %s: exit %d\n%s" % (seed, rc, out[-6000:])
		assert " passed" in out and "libv2m_hip_checked.so" in out, out[-3000:]
		print(seed, out.strip().splitlines()[-2])
