"""Context.site_ld / site_ld_device (v2m_site_ld[_device]: the column counts' kernels, count_ld_columns_kernel, emit_ld_columns_kernel,
ld_pack_kernel, ld_pairs_kernel) and --output-ld against the model of tests/site_ld_model.py: every item goes through the host form and
through the device form, with guard bytes around its buffers, and the site and pair records are held equal to the model's record for
record and in order.

tests/test_site_ld_host.py asserts, without a GPU, that the corpus holds the site counts, bands, row counts, thresholds, windows and
bytes it is here for, that wide_items() (4 160 and 32 768 rows) reach every way the threshold's two 128-bit products can compare, and
that band_items() (581 sites) reach bands of 4 to 10 tiles a strip."""

import ctypes as C
import io
import os

import numpy as np
import pytest

import column_counts_model as CM
import oracle
import site_ld_model as LM
import synth
import variable_sites_model as VM

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")
PLOIDY_MAX = LM.PLOIDY_MAX
T, CHUNK = LM.kernel_constants()              # kLdTile, kLdChunkWords
GUARD = 4                                     # guard records on either side of a device buffer
RECORD = 24


@pytest.fixture(scope="module")
def v2m():
	import vcf2multialign_amd as v
	from vcf2multialign_amd import _native as N
	assert (N.LD_TILE, N.LD_CHUNK_WORDS, N.SITE_LD_MAX_WINDOW) == (T, CHUNK, LM.MAX_WINDOW)
	assert np.dtype(N.LD_SITE_DTYPE) == LM.SITE_DTYPE and np.dtype(N.LD_PAIR_DTYPE) == LM.PAIR_DTYPE
	return v


@pytest.fixture(scope="module")
def ctx(v2m):
	c = v2m.Context(0)
	yield c
	c.close()


def upload(v2m, ctx, g):
	ctx.upload_graph(v2m.VariantGraph.from_object(g), g.ref)


def pattern_bytes(n):
	return ((np.arange(n, dtype=np.uint64) * 2654435761 >> 7) % 251 + 1).astype(np.uint8)


class DeviceBuffers:
	"""v2m_ld_site[site_capacity] and v2m_ld_pair[pair_capacity] on the device, each between GUARD guard records, pre-filled."""

	def __init__(self, site_capacity, pair_capacity):
		import torch
		self.site_capacity, self.pair_capacity = site_capacity, pair_capacity
		self.fill_sites = pattern_bytes(RECORD * (2 * GUARD + site_capacity))
		self.fill_pairs = pattern_bytes(RECORD * (2 * GUARD + pair_capacity))[::-1].copy()
		self.sites = torch.from_numpy(self.fill_sites.copy()).cuda()
		self.pairs = torch.from_numpy(self.fill_pairs.copy()).cuda()
		self.sites_ptr = self.sites.data_ptr() + RECORD * GUARD
		self.pairs_ptr = self.pairs.data_ptr() + RECORD * GUARD
		assert self.sites_ptr % 16 == 0 and self.pairs_ptr % 16 == 0 and (RECORD * GUARD) % 16 == 0

	def read(self):
		return self.sites.cpu().numpy(), self.pairs.cpu().numpy()

	def untouched(self):
		s, p = self.read()
		return np.array_equal(s, self.fill_sites) and np.array_equal(p, self.fill_pairs)


def same_records(got, want, what):
	assert got.dtype == want.dtype, what
	if len(got) != len(want) or not np.array_equal(got, want):
		k = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), min(len(got), len(want)))
		raise AssertionError("%s: %d records, expected %d; the first difference at %d: got %s, expected %s"
			% (what, len(got), len(want), k, got[k] if k < len(got) else None, want[k] if k < len(want) else None))


def check_device(ctx, rows, params, want_sites, want_pairs, what, extra=3):
	"""The device form into guarded buffers with `extra` records to spare: exactly [0, V) and [0, n_pairs) are written."""
	V, P = len(want_sites), len(want_pairs)
	buf = DeviceBuffers(V + extra, P + extra)
	assert ctx.site_ld_device(rows, buf.sites_ptr, V + extra, buf.pairs_ptr, P + extra, **params.kwargs()) == (V, P), what
	s, p = buf.read()
	lo, hi = RECORD * GUARD, RECORD * (GUARD + V)
	assert np.array_equal(s[:lo], buf.fill_sites[:lo]) and np.array_equal(s[hi:], buf.fill_sites[hi:]), what + ": the site records beyond V and their guards"
	same_records(s[lo:hi].view(LM.SITE_DTYPE), want_sites, what + ": the sites")
	hi = RECORD * (GUARD + P)
	assert np.array_equal(p[:lo], buf.fill_pairs[:lo]) and np.array_equal(p[hi:], buf.fill_pairs[hi:]), what + ": the pair records beyond n_pairs and their guards"
	same_records(p[lo:hi].view(LM.PAIR_DTYPE), want_pairs, what + ": the pairs")


def check_item(ctx, item, what=""):
	"""Both forms over the view in force against the model; returns the host form's info."""
	what = what or item.name
	want_sites, want_pairs, n_candidates, L = LM.expected(item)
	assert ctx.window_length == L
	sites, pairs, info = ctx.site_ld(item.rows, info=True, **item.params.kwargs())
	same_records(sites, want_sites, what + " host form: the sites")
	same_records(pairs, want_pairs, what + " host form: the pairs")
	if len(item.rows):
		assert (info["n_sites"], info["n_columns"], info["n_pairs"], info["n_candidates"]) == (len(want_sites), L, len(want_pairs), n_candidates), (what, info)
	assert info["counts_ms"] == info["pack_ms"] == info["pairs_ms"] == 0.0      # profiling is off
	assert ctx.site_ld_blocks == ([len(want_pairs)] if len(want_pairs) else []), (what, ctx.site_ld_blocks)
	check_device(ctx, item.rows, item.params, want_sites, want_pairs, what + " device form")
	return info


# ---- the corpus ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("item", LM.corpus(), ids=[i.name for i in LM.corpus()])
def test_corpus(v2m, ctx, item):
	upload(v2m, ctx, item.g)
	if item.window:
		ctx.set_column_window(*item.window)
	check_item(ctx, item)
	if item.window:
		assert ctx.window_length == item.window[1] - item.window[0]


def item_named(name):
	return next(i for i in LM.corpus() if i.name == name)


def test_n_sites_against_the_snp_sites(v2m, ctx):
	"""The sites are the SNP sites of v2m_variable_sites whose column holds exactly two of A, C, G, T, each often enough."""
	for name in ("pm_sites", "min_count_2", "sites_%d" % (T + 1)):
		item = item_named(name)
		upload(v2m, ctx, item.g)
		columns, data = ctx.variable_sites(item.rows, snp_only=True)
		keep = []
		for k in range(len(columns)):
			present = [int((LM.PM.classes(data[:, k]) == c).sum()) for c in range(4)]
			keep.append(sum(1 for x in present if x) == 2 and all(x >= item.params.min_allele_count for x in present if x))
		sites, _ = ctx.site_ld(item.rows, **item.params.kwargs())
		assert np.array_equal(sites["column"], columns[np.array(keep, dtype=bool)]) and 0 < len(sites) <= len(columns), name


def test_capacities(v2m, ctx):
	"""Capacities one too small: the error names both numbers, both counts are set, nothing is written, and a call sized by them
	succeeds.  Exact capacities.  NULL d_pairs with capacity 0: the counts only."""
	from vcf2multialign_amd import _native as N
	item = item_named("sites_%d" % (T + 1))
	upload(v2m, ctx, item.g)
	want_sites, want_pairs, _, _ = LM.expected(item)
	V, P = len(want_sites), len(want_pairs)
	assert V > 1 and P > 1
	for site_capacity, pair_capacity in ((V - 1, P), (V, P - 1), (0, 0), (V - 1, P - 1)):
		buf = DeviceBuffers(max(site_capacity, 1), max(pair_capacity, 1))
		with pytest.raises(v2m.V2MError) as e:
			ctx.site_ld_device(item.rows, buf.sites_ptr, site_capacity, buf.pairs_ptr, pair_capacity, **item.params.kwargs())
		assert e.value.code == N.V2M_ERR_INVALID_ARGUMENT and str(V) in str(e.value) and str(P) in str(e.value), str(e.value)
		assert ctx.site_ld_counts == (V, P) and buf.untouched()
	buf = DeviceBuffers(V, 1)
	with pytest.raises(v2m.V2MError) as e:
		ctx.site_ld_device(item.rows, buf.sites_ptr, V, None, 0, **item.params.kwargs())
	assert e.value.code == N.V2M_ERR_INVALID_ARGUMENT and ctx.site_ld_counts == (V, P) and buf.untouched()
	check_device(ctx, item.rows, item.params, want_sites, want_pairs, "sized by the first call", extra=0)
	# no pair is reported: NULL d_pairs succeeds and the sites are written
	none = item_named("random_40_r2_1_1")
	upload(v2m, ctx, none.g)
	want_sites, want_pairs, _, _ = LM.expected(none)
	assert len(want_pairs) == 0 and len(want_sites) == 40
	buf = DeviceBuffers(40, 1)
	assert ctx.site_ld_device(none.rows, buf.sites_ptr, 40, None, 0, **none.params.kwargs()) == (40, 0)
	s, p = buf.read()
	same_records(s[RECORD * GUARD:RECORD * (GUARD + 40)].view(LM.SITE_DTYPE), want_sites, "NULL d_pairs: the sites")
	assert np.array_equal(p, buf.fill_pairs)


def test_row_slices(v2m, ctx, monkeypatch):
	"""V2M_RING_SLOT_BYTES small enough for slices of 50 rows: the slices straddle the 64-row words of the planes, which two launches
	of ld_pack_kernel then OR into."""
	from vcf2multialign_amd import _native as N
	item = item_named("rows_%d" % (64 * CHUNK + 1))
	upload(v2m, ctx, item.g)
	want = check_item(ctx, item, "one slice")
	pitch = int(ctx.min_row_pitch)
	monkeypatch.setenv("V2M_RING_SLOT_BYTES", str(50 * pitch + pitch // 2))
	ctx.profile_enable(True)
	ctx.profile_reset()
	try:
		sites, pairs, info = ctx.site_ld(item.rows, info=True, **item.params.kwargs())
		launches = ctx.profile_get(N.KERNEL_COLUMN_COUNTS)[0]
		assert launches == (len(item.rows) + 49) // 50 and launches > 8, launches
		assert info["counts_ms"] > 0 and info["pack_ms"] > 0 and info["pairs_ms"] > 0
	finally:
		ctx.profile_reset()
		ctx.profile_enable(False)
	want_sites, want_pairs, _, _ = LM.expected(item)
	same_records(sites, want_sites, "in slices: the sites")
	same_records(pairs, want_pairs, "in slices: the pairs")
	check_device(ctx, item.rows, item.params, want_sites, want_pairs, "device form in slices")
	monkeypatch.delenv("V2M_RING_SLOT_BYTES")
	assert check_item(ctx, item, "one slice again") == want


# V2M_SITE_LD_WORDS_PER_GROUP over six row words, the last one ragged: groups of two, of three, of four (a full group and a ragged one of
# two) and one group of more words than there are (what the rule gives when the site blocks alone fill the device)
LD_WORDS_PER_GROUP = (2, 3, 4, 1000000)


@pytest.mark.parametrize("per_group", LD_WORDS_PER_GROUP)
def test_word_groups_of_the_pack(v2m, ctx, monkeypatch, per_group):
	"""ld_pack_kernel with more than one word a group: its loop over a group's words makes a second trip and more."""
	item = LM.row_words_item()
	upload(v2m, ctx, item.g)
	monkeypatch.setenv("V2M_SITE_LD_WORDS_PER_GROUP", str(per_group))
	check_item(ctx, item, "%s, %d words a group" % (item.name, per_group))


@pytest.mark.parametrize("per_group", LD_WORDS_PER_GROUP)
def test_word_groups_of_the_pack_in_slices(v2m, ctx, monkeypatch, per_group):
	"""The same under slices of 50 rows: a slice's first word is the previous slice's last, which both launches OR into, and a slice
	of 50 rows spans two words, so a group of two or more holds them both."""
	item = LM.row_words_item()
	upload(v2m, ctx, item.g)
	pitch = int(ctx.min_row_pitch)
	monkeypatch.setenv("V2M_RING_SLOT_BYTES", str(50 * pitch + pitch // 2))
	monkeypatch.setenv("V2M_SITE_LD_WORDS_PER_GROUP", str(per_group))
	check_item(ctx, item, "%s, %d words a group, slices of 50 rows" % (item.name, per_group))


def test_emit_ranges(v2m, ctx, monkeypatch):
	"""The smallest V2M_SITE_LD_BLOCK_BYTES: one strip of T sites per emit range, the blocks in order and together all pairs; and a
	block size that takes two strips."""
	item = item_named("sites_%d" % (2 * T + 1))
	upload(v2m, ctx, item.g)
	want_sites, want_pairs, _, _ = LM.expected(item)
	per_strip = [int(((want_pairs["site_a"] // T) == k).sum()) for k in range(3)]
	assert per_strip[0] and per_strip[1] and not per_strip[2], per_strip      # the last strip holds the last site alone: a range without a pair
	monkeypatch.setenv("V2M_SITE_LD_BLOCK_BYTES", "1")
	sites, pairs = ctx.site_ld(item.rows, **item.params.kwargs())
	assert ctx.site_ld_blocks == per_strip[:2]
	same_records(sites, want_sites, "a strip a range: the sites")
	same_records(pairs, want_pairs, "a strip a range: the pairs")
	monkeypatch.setenv("V2M_SITE_LD_BLOCK_BYTES", str(RECORD * (per_strip[0] + per_strip[1]) - 1))
	sites, pairs = ctx.site_ld(item.rows, **item.params.kwargs())
	assert ctx.site_ld_blocks == per_strip[:2]
	same_records(pairs, want_pairs, "a record short of two strips: the pairs")
	monkeypatch.setenv("V2M_SITE_LD_BLOCK_BYTES", str(RECORD * (per_strip[0] + per_strip[1])))
	sites, pairs = ctx.site_ld(item.rows, **item.params.kwargs())
	assert ctx.site_ld_blocks == [per_strip[0] + per_strip[1]]
	same_records(pairs, want_pairs, "all strips a range: the pairs")
	check_device(ctx, item.rows, item.params, want_sites, want_pairs, "device form under a block size")
	monkeypatch.delenv("V2M_SITE_LD_BLOCK_BYTES")
	check_item(ctx, item, "one range again")


# ---- the threshold beyond 64 bits: batches of 4 160 and 32 768 rows --------------------------------------------------------------------------

def wide_named(name):
	return next(i for i in LM.wide_items() if i.name == name)


@pytest.mark.parametrize("item", LM.wide_items(), ids=[i.name for i in LM.wide_items()])
def test_wide_rows(v2m, ctx, item):
	"""ld_reported() where D^2 min_r2_den and min_r2_num den pass 2^64: the high words decide against the low ones (R1, R2), are equal
	and not 0 (R3, the ties and their neighbours); tests/test_site_ld_host.py names the regime of every item."""
	upload(v2m, ctx, item.g)
	check_item(ctx, item)


def test_wide_rows_in_slices(v2m, ctx, monkeypatch):
	"""V2M_SITE_LD_MAX_ROWS rows in slices of 1 000: 33 launches of ld_pack_kernel into 512 row words, no slice but the first beginning
	on a word."""
	from vcf2multialign_amd import _native as N
	item = wide_named("wide_r1")
	assert len(item.rows) == N.SITE_LD_MAX_ROWS
	upload(v2m, ctx, item.g)
	pitch = int(ctx.min_row_pitch)
	monkeypatch.setenv("V2M_RING_SLOT_BYTES", str(1000 * pitch + pitch // 2))
	ctx.profile_enable(True)
	ctx.profile_reset()
	try:
		sites, pairs = ctx.site_ld(item.rows, **item.params.kwargs())
		launches = ctx.profile_get(N.KERNEL_COLUMN_COUNTS)[0]
		assert launches == (len(item.rows) + 999) // 1000 == 33, launches
	finally:
		ctx.profile_reset()
		ctx.profile_enable(False)
	want_sites, want_pairs, _, _ = LM.expected(item)
	same_records(sites, want_sites, "in slices: the sites")
	same_records(pairs, want_pairs, "in slices: the pairs")
	check_item(ctx, item, "%s in slices of 1000 rows" % item.name)


def test_wide_rows_in_word_groups(v2m, ctx, monkeypatch):
	"""The 512 row words in groups of three: 170 whole groups and one of two words."""
	item = wide_named("wide_r1")
	upload(v2m, ctx, item.g)
	monkeypatch.setenv("V2M_SITE_LD_WORDS_PER_GROUP", "3")
	check_item(ctx, item, "%s, 3 words a group" % item.name)


# ---- bands of 4 to 10 tiles over 10 strips ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("item", LM.band_items(), ids=[i.name for i in LM.band_items()])
def test_bands(v2m, ctx, item):
	"""A strip's cells in one, two and three trips of scan_tile_counts_kernel, ld_pairs_kernel<true>'s cells[cell + 1] across up to ten
	tiles, interior strips whose whole band is live and strips whose band leaves the strips."""
	upload(v2m, ctx, item.g)
	check_item(ctx, item)


def ranges_of(per_strip, block_pairs):
	"""The pairs of the emit ranges as include/v2m_hip.h says them: whole strips while their records fit the block, at least one strip;
	a range without a pair is passed over.  [(first strip, strips, pairs)]."""
	out, i = [], 0
	while i < len(per_strip):
		j, count = i + 1, per_strip[i]
		while j < len(per_strip) and count + per_strip[j] <= block_pairs:
			count += per_strip[j]
			j += 1
		if count:
			out.append((i, j - i, count))
		i = j
	return out


def test_band_emit_ranges(v2m, ctx, monkeypatch):
	"""Emit ranges over ten strips of a band of five tiles: a strip a range, and three strips a range, so that ranges begin at strips
	3 and 6 and ld_pairs_kernel<true> takes strip_bases[ti] - out_base for a strip_first beyond 2."""
	item = next(i for i in LM.band_items() if i.name == "band_w%d_r2_0_1" % (3 * T + 1))
	upload(v2m, ctx, item.g)
	want_sites, want_pairs, _, _ = LM.expected(item)
	per_strip = np.bincount(want_pairs["site_a"] // T, minlength=10).tolist()
	assert len(per_strip) == 10 and all(per_strip) and sum(per_strip) == len(want_pairs)
	three = max(sum(per_strip[i:i + 3]) for i in range(8))
	for block_bytes, strips in ((1, 1), (RECORD * three, 3)):
		ranges = ranges_of(per_strip, max(1, block_bytes // RECORD))
		assert ranges[0][1] == strips and len(ranges) >= 3 and ranges[1][0] == strips and (strips == 1 or ranges[1][1] == 3 and ranges[2][0] == 6), ranges
		monkeypatch.setenv("V2M_SITE_LD_BLOCK_BYTES", str(block_bytes))
		sites, pairs = ctx.site_ld(item.rows, **item.params.kwargs())
		assert ctx.site_ld_blocks == [count for _, _, count in ranges], (ctx.site_ld_blocks, ranges)
		same_records(sites, want_sites, "%d strips a range: the sites" % strips)
		order = pairs["site_a"].astype(np.int64) * len(want_sites) + pairs["site_b"]
		assert (np.diff(order) > 0).all(), "%d strips a range: the pairs are not in the order (s, t)" % strips
		same_records(pairs, want_pairs, "%d strips a range: the pairs" % strips)
		check_device(ctx, item.rows, item.params, want_sites, want_pairs, "device form, %d strips a range" % strips)
	monkeypatch.delenv("V2M_SITE_LD_BLOCK_BYTES")
	check_item(ctx, item, "one range again")


def test_plane_budget(v2m, ctx, monkeypatch):
	"""A plane budget one byte too small is V2M_ERR_UNSUPPORTED with the bytes needed in the message; the exact budget passes."""
	from vcf2multialign_amd import _native as N
	item = item_named("rows_%d" % (64 * CHUNK + 1))
	upload(v2m, ctx, item.g)
	want_sites, want_pairs, _, _ = LM.expected(item)
	V, n = len(want_sites), len(item.rows)
	need = 16 * ((V + T - 1) // T * T) * ((n + 63) // 64)
	monkeypatch.setenv("V2M_SITE_LD_PLANE_BYTES", str(need - 1))
	buf = DeviceBuffers(V, len(want_pairs))
	with pytest.raises(v2m.V2MError) as e:
		ctx.site_ld(item.rows, **item.params.kwargs())
	assert e.value.code == N.V2M_ERR_UNSUPPORTED and str(need) in str(e.value), str(e.value)
	with pytest.raises(v2m.V2MError) as e:
		ctx.site_ld_device(item.rows, buf.sites_ptr, V, buf.pairs_ptr, len(want_pairs), **item.params.kwargs())
	assert e.value.code == N.V2M_ERR_UNSUPPORTED and str(need) in str(e.value) and buf.untouched(), str(e.value)
	monkeypatch.setenv("V2M_SITE_LD_PLANE_BYTES", str(need))
	check_item(ctx, item, "the exact budget")
	monkeypatch.delenv("V2M_SITE_LD_PLANE_BYTES")


def test_sinks(v2m, ctx):
	"""A sink that returns non-zero gives V2M_ERR_SINK (and the other sink is not called afterwards); NULL sinks are accepted."""
	from vcf2multialign_amd import _native as N
	item = item_named("random_40_r2_1_5")
	upload(v2m, ctx, item.g)
	want_sites, want_pairs, n_candidates, _ = LM.expected(item)
	V, P = len(want_sites), len(want_pairs)
	batch = v2m.RowBatch(item.rows)
	params = ctx._site_ld_params(**item.params.kwargs())
	calls = []
	call = ctx._lib.v2m_site_ld

	def sink(kind, result):
		def cb(_user, _records, n):
			calls.append((kind, int(n)))
			return result
		return N.LD_SINK_FN(cb)

	null = C.cast(None, N.LD_SINK_FN)
	info = N.SiteLdInfo()
	assert N.V2M_OK == call(ctx._h, C.byref(batch.struct), C.byref(params), sink("sites", 0), sink("pairs", 0), None, C.byref(info))
	assert calls == [("sites", V), ("pairs", P)] and (info.n_sites, info.n_pairs, info.n_candidates) == (V, P, n_candidates)
	del calls[:]
	assert N.V2M_ERR_SINK == call(ctx._h, C.byref(batch.struct), C.byref(params), sink("sites", 3), sink("pairs", 0), None, None)
	assert calls == [("sites", V)]
	del calls[:]
	assert N.V2M_ERR_SINK == call(ctx._h, C.byref(batch.struct), C.byref(params), sink("sites", 0), sink("pairs", -1), None, None)
	assert calls == [("sites", V), ("pairs", P)]
	del calls[:]
	assert N.V2M_OK == call(ctx._h, C.byref(batch.struct), C.byref(params), null, sink("pairs", 0), None, None)
	assert calls == [("pairs", P)]
	del calls[:]
	assert N.V2M_OK == call(ctx._h, C.byref(batch.struct), C.byref(params), sink("sites", 0), null, None, C.byref(info))
	assert calls == [("sites", V)] and info.n_pairs == P
	del calls[:]
	assert N.V2M_OK == call(ctx._h, C.byref(batch.struct), C.byref(params), null, null, None, C.byref(info)) and (info.n_sites, info.n_pairs) == (V, P) and not calls
	# no pair: the pair sink is not called; no site: neither is
	none = item_named("random_40_r2_1_1")
	params = ctx._site_ld_params(**none.params.kwargs())
	assert N.V2M_OK == call(ctx._h, C.byref(batch.struct), C.byref(params), sink("sites", 0), sink("pairs", 1), None, C.byref(info))
	assert calls == [("sites", V)] and info.n_pairs == 0
	del calls[:]
	upload(v2m, ctx, CM.other_graph())
	three = v2m.RowBatch([PLOIDY_MAX, 0, 1])
	assert N.V2M_OK == call(ctx._h, C.byref(three.struct), C.byref(params), sink("sites", 1), sink("pairs", 1), None, C.byref(info))
	assert not calls and (info.n_sites, info.n_columns, info.n_pairs) == (0, 21, 0)
	check_item(ctx, item_named("all_other"), "after the sinks")


def test_the_views_are_left_as_they_were(v2m, ctx):
	item = next(i for i in LM.corpus() if i.window)
	g, rows, w = item.g, item.rows, item.window
	upload(v2m, ctx, g)
	sets = [(2, 30), (41, 47), (3, 4)]
	ctx.set_window_set(sets)
	ctx.set_column_window(*w)
	pieces = ctx.splice_window_set(rows)
	before = ctx.column_counts(rows)
	spliced = ctx.splice_rows(rows)
	check_item(ctx, item, "under a window set and a window")
	assert ctx.window_length == w[1] - w[0] and ctx.window_set_size == len(sets)
	for a, b in zip(before, ctx.column_counts(rows)):
		assert np.array_equal(a, b)
	assert ctx.splice_rows(rows) == spliced and ctx.splice_window_set(rows) == pieces
	ctx.set_column_window(0, g.aligned_length)
	check_item(ctx, LM.Item("whole", g, rows, item.params), "whole rows again")


# ---- the raw ABI -----------------------------------------------------------------------------------------------------------------------------

def test_errors(v2m):
	import torch
	from vcf2multialign_amd import _native as N
	with v2m.Context(0) as c:
		item = item_named("ld_graph_r2_1_5")
		g = item.g
		batch = v2m.RowBatch(item.rows)
		sites = torch.full((RECORD * 16,), 7, dtype=torch.uint8, device="cuda")
		pairs = torch.full((RECORD * 32,), 7, dtype=torch.uint8, device="cuda")
		ns, np_ = C.c_uint64(77), C.c_uint64(78)
		null = C.cast(None, N.LD_SINK_FN)
		call, device = c._lib.v2m_site_ld, c._lib.v2m_site_ld_device
		good = N.SiteLdParams(4096, 1, 1, 5, 0)

		def both(params, batch_ref=None):
			ref = C.byref(batch.struct) if batch_ref is None else batch_ref
			p = C.byref(params) if params is not None else None
			return (call(c._h, ref, p, null, null, None, None), device(c._h, ref, p, sites.data_ptr(), 16, pairs.data_ptr(), 32, C.byref(ns), C.byref(np_)))

		# no graph
		assert both(good) == (N.V2M_ERR_STATE, N.V2M_ERR_STATE)
		upload(v2m, c, g)
		# NULL rows and params; parameters out of range
		assert call(c._h, None, C.byref(good), null, null, None, None) == N.V2M_ERR_INVALID_ARGUMENT
		assert both(None) == (N.V2M_ERR_INVALID_ARGUMENT,) * 2
		for bad in (N.SiteLdParams(0, 1, 1, 5, 0), N.SiteLdParams(4097, 1, 1, 5, 0), N.SiteLdParams(10, 0, 1, 5, 0), N.SiteLdParams(10, 1, 1, 0, 0),
				N.SiteLdParams(10, 1, 6, 5, 0), N.SiteLdParams(10, 1, 1, 1000001, 0)):
			assert both(bad) == (N.V2M_ERR_INVALID_ARGUMENT,) * 2, [getattr(bad, f) for f, _ in bad._fields_]
			assert "v2m_site_ld" in c._lib.v2m_last_error(c._h).decode()
		# NULL outputs, a NULL d_pairs with a capacity, misaligned buffers
		ref, p = C.byref(batch.struct), C.byref(good)
		assert N.V2M_ERR_INVALID_ARGUMENT == device(c._h, ref, p, None, 16, pairs.data_ptr(), 32, C.byref(ns), C.byref(np_))
		assert N.V2M_ERR_INVALID_ARGUMENT == device(c._h, ref, p, sites.data_ptr(), 16, None, 32, C.byref(ns), C.byref(np_))
		assert N.V2M_ERR_INVALID_ARGUMENT == device(c._h, ref, p, sites.data_ptr(), 16, pairs.data_ptr(), 32, None, C.byref(np_))
		assert N.V2M_ERR_INVALID_ARGUMENT == device(c._h, ref, p, sites.data_ptr(), 16, pairs.data_ptr(), 32, C.byref(ns), None)
		for off in (1, 4, 8):
			assert N.V2M_ERR_INVALID_ARGUMENT == device(c._h, ref, p, sites.data_ptr() + off, 15, pairs.data_ptr(), 32, C.byref(ns), C.byref(np_))
			assert N.V2M_ERR_INVALID_ARGUMENT == device(c._h, ref, p, sites.data_ptr(), 16, pairs.data_ptr() + off, 31, C.byref(ns), C.byref(np_))
		assert (sites.cpu().numpy() == 7).all() and (pairs.cpu().numpy() == 7).all() and (ns.value, np_.value) == (77, 78)
		# more rows than the limit: before any device work
		many = v2m.RowBatch([0] * (N.SITE_LD_MAX_ROWS + 1))
		assert both(good, C.byref(many.struct)) == (N.V2M_ERR_UNSUPPORTED,) * 2 and str(N.SITE_LD_MAX_ROWS) in c._lib.v2m_last_error(c._h).decode()
		# no rows: V2M_OK, nothing touched
		empty = v2m.RowBatch([])
		info = N.SiteLdInfo()
		info.n_columns = 77
		sunk = []
		sink = N.LD_SINK_FN(lambda *a: sunk.append(a) or 0)
		assert N.V2M_OK == call(c._h, C.byref(empty.struct), p, sink, sink, None, C.byref(info)) and info.n_columns == 77 and not sunk
		assert N.V2M_OK == device(c._h, C.byref(empty.struct), p, sites.data_ptr(), 16, pairs.data_ptr(), 32, C.byref(ns), C.byref(np_)) and (ns.value, np_.value) == (77, 78)
		assert (sites.cpu().numpy() == 7).all() and (pairs.cpu().numpy() == 7).all()
		s, pr, info_dict = c.site_ld([], info=True)
		assert s.shape == (0,) and pr.shape == (0,) and info_dict["n_columns"] == g.aligned_length
		# one row: no site
		s, pr = c.site_ld([3])
		assert s.shape == (0,) and pr.shape == (0,)
		# bad cuts
		bad = v2m.RowBatch([0, [(2, 0), (1, 1)]])
		assert both(good, C.byref(bad.struct)) == (N.V2M_ERR_PRECONDITION,) * 2
		check_item(c, item, "after the errors")


# ---- the driver ------------------------------------------------------------------------------------------------------------------------------

def _run(args, cwd=None):
	import subprocess
	assert os.path.exists(CLI), "build the host driver first (__graft_entry__.build())"
	return subprocess.run([CLI] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def test_cli_haplotypes(v2m, ctx, tmp_path):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	g = oracle.build_variant_graph(fa, vcf, "1")
	vg = v2m.VariantGraph.from_object(g)
	ids, rows = VM.a2m_ids(g)
	out = tmp_path / "ld.tsv"
	common = ["-H", "-r", fa, "-a", vcf, "-c", "1"]
	s, e = 3, min(len(g.ref), 9)
	w = vg.columns_of_reference_range(s - 1, e)
	seen = []
	for extra, params in (([], LM.Params(1000, 0, (1, 5), 1)), (["--ld-min-r2=0"], LM.Params(1000, 0, (0, 1), 1)),
			(["--ld-min-r2=0.05", "--ld-window=2", "--omit-reference"], LM.Params(2, 0, (1, 20), 1)),
			(["--ld-min-r2=0.000001", "--ld-window-columns=3", "--ld-min-count=2"], LM.Params(1000, 3, (1, 1000000), 2)),
			(["--ld-min-r2=1", "--region=%d-%d" % (s, e)], LM.Params(1000, 0, (1, 1), 1)),
			(["--ld-min-r2=0.", "--region=%d-%d" % (s, e), "--omit-reference"], LM.Params(1000, 0, (0, 1), 1))):
		k = 1 if "--omit-reference" in extra else 0
		window = w if any(x.startswith("--region") for x in extra) else None
		r = _run(common + ["--output-ld=" + str(out), "--verbose"] + extra)
		assert r.returncode == 0, r.stderr.decode()
		want = LM.file_text(g, rows[k:], window, params)
		assert out.read_bytes() == want, (extra, out.read_bytes().decode(), want.decode())
		header = want.decode().splitlines()[0].split("\t")
		seen.append((int(header[5]), int(header[7])))
		assert ("Site LD: %d rows, %d columns, %d sites," % (len(rows) - k, int(header[3]), int(header[5]))).encode() in r.stderr, r.stderr.decode()
	assert seen[0][0] > 1 and max(p for _, p in seen) > 0 and len(set(seen)) > 1, seen
	# Output.output_ld writes the same bytes
	upload(v2m, ctx, g)
	stream = io.BytesIO()
	info = v2m.HaplotypeOutput(ctx).output_ld(vg, stream)
	assert stream.getvalue() == LM.file_text(g, rows, None, LM.Params(1000, 0, (1, 5), 1)) and info["n_sites"] == seen[0][0]
	stream = io.BytesIO()
	v2m.HaplotypeOutput(ctx, should_output_reference=False, region=(s - 1, e)).output_ld(vg, stream, min_r2=(0, 1))
	assert stream.getvalue() == LM.file_text(g, rows[1:], w, LM.Params(1000, 0, (0, 1), 1)) and ctx.window_length == g.aligned_length


def test_cli_founders(v2m, ctx, tmp_path):
	from vcf2multialign_amd import host
	g = synth.build_case(tmp_path, 44, 40000, 1200, 6)
	fa, vcf = str(tmp_path / "synth.fa"), str(tmp_path / "synth.vcf")
	out, cuts_file = tmp_path / "f.ld", tmp_path / "cuts"
	r = _run(["-F", "3", "-d", "10", "-r", fa, "-a", vcf, "-c", "1", "--output-ld=" + str(out), "--ld-window=50", "--ld-min-r2=0.5", "-t", str(cuts_file), "--verbose"])
	assert r.returncode == 0, r.stderr.decode()
	cuts, _, _ = host.read_cut_positions(cuts_file)
	lines = r.stdout.decode().split("Matchings:\n")[1].splitlines()[:3]
	assigned = [int(x) for line in lines for x in line.split("\t")[1:]]
	n = len(cuts) - 1
	assert len(assigned) == 3 * n
	rows = [PLOIDY_MAX] + [list(zip(cuts[:-1], assigned[k * n:(k + 1) * n])) for k in range(3)]
	params = LM.Params(50, 0, (1, 2), 1)
	want = LM.file_text(g, rows, None, params)
	assert out.read_bytes() == want and len(want.splitlines()) > 3
	vg = v2m.VariantGraph.from_object(g)
	w = vg.columns_of_reference_range(999, 30000)
	r = _run(["-F", "3", "-d", "10", "-r", fa, "-a", vcf, "-c", "1", "--output-ld=" + str(out), "--ld-window=50", "--ld-min-r2=0.5", "-p", str(cuts_file), "--omit-reference", "--region=1000-30000"])
	assert r.returncode == 0, r.stderr.decode()
	assert out.read_bytes() == LM.file_text(g, rows[1:], w, params)
	upload(v2m, ctx, g)
	stream = io.BytesIO()
	v2m.FounderSequenceGreedyOutput(ctx).output_ld(vg, cuts, assigned, stream, window_sites=50, min_r2=(1, 2))
	assert stream.getvalue() == want


# ---- the checked build -----------------------------------------------------------------------------------------------------------------------

CHECKED_CORPUS = [
	"tests/test_gpu_site_ld.py::test_corpus",
	"tests/test_gpu_site_ld.py::test_capacities",
	"tests/test_gpu_site_ld.py::test_row_slices",
	"tests/test_gpu_site_ld.py::test_word_groups_of_the_pack",
	"tests/test_gpu_site_ld.py::test_word_groups_of_the_pack_in_slices",
	"tests/test_gpu_site_ld.py::test_emit_ranges",
	"tests/test_gpu_site_ld.py::test_plane_budget",
	"tests/test_gpu_site_ld.py::test_sinks",
	"tests/test_gpu_site_ld.py::test_the_views_are_left_as_they_were",
	# batches of 4 160 and 32 768 rows (512 row words of planes), strips of up to 640 cells
	"tests/test_gpu_site_ld.py::test_wide_rows",
	"tests/test_gpu_site_ld.py::test_wide_rows_in_slices",
	"tests/test_gpu_site_ld.py::test_wide_rows_in_word_groups",
	"tests/test_gpu_site_ld.py::test_bands",
	"tests/test_gpu_site_ld.py::test_band_emit_ranges",
]


def test_corpus_on_the_checked_build():
	"""The list above with every LDS object, scratch buffer (the site list, the records, the planes, the cells and the pairs of a range
	among them) and staging area poisoned before use (tests/test_gpu_checked_build.py), one run per seed: a site, a plane word or a
	cell nobody wrote in this call changes the result.  No library is preloaded."""
	from test_gpu_checked_build import SEEDS, run_checked_corpus
	from vcf2multialign_amd import build
	assert os.path.exists(build.CHECKED_LIB_PATH) and os.path.exists(build.CHECKED_HOST_LIB_PATH), "build_native() builds them"
	for seed in SEEDS:   # the second seed only once the first has passed
		rc, out = run_checked_corpus(seed, build.CHECKED_LIB_PATH, build.CHECKED_HOST_LIB_PATH, corpus=CHECKED_CORPUS, timeout=600)
		assert rc == 0, "checked build, seed %s: exit %d\n%s" % (seed, rc, out[-6000:])
		assert " passed" in out and "libv2m_hip_checked.so" in out, out[-3000:]
		print(seed, out.strip().splitlines()[-2])
