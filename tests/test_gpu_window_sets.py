"""Window sets (v2m_set_window_set, v2m_splice_window_set[_device], --regions-file) on the GPU.

Piece (row, k) of a set is the body v2m_set_column_window(begin_k, end_k) + a row call gives, so every piece of every row is compared
with test_gpu_window.py's column-tracking walk, sliced (window_bodies), in both modes; every seventh window is compared with the
column-window calls on the same context as well.  The device form is checked for what it may write: a buffer of 0x55 keeps that byte
everywhere outside the pieces (unaligned) or outside the slots' 16-byte chunks (aligned)."""

import os
import subprocess

import numpy as np
import pytest

import oracle
import synth
from test_gpu_window import FIXTURES, PLOIDY_MAX, TILE, _bridges, _fixture_graph, _records, column_walk, oracle_cols, walk_rows, window_bodies, window_classes

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
SEAM_LENGTHS = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49]


@pytest.fixture(scope="module")
def v2m():
	import vcf2multialign_amd as v
	return v


@pytest.fixture(scope="module")
def ctx(v2m):
	c = v2m.Context(0)
	yield c
	c.close()


def model_layout(wins):
	offsets, at = [], 0
	for b, e in wins:
		offsets.append(at)
		at += (e - b + 15) // 16 * 16
	return offsets, (at + 255) // 256 * 256, at


def check_set(v2m, ctx, g, rows, windows, forms=("rows",), walked=None, kind_of_row=None, upload=True):
	"""Every piece of every row of the set `windows` ((begin, end) or (name, begin, end)), aligned and unaligned, against the walk.
	walked / kind_of_row: the walks of the distinct rows and which of them row i is (batches that repeat a few rows many times)."""
	wins = [(int(w[-2]), int(w[-1])) for w in windows]
	if upload:
		ctx.upload_graph(v2m.VariantGraph.from_object(g), g.ref)
	if walked is None:
		walked = walk_rows(g, rows)
	if kind_of_row is None:
		kind_of_row = list(range(len(rows)))
	ctx.set_window_set(wins)
	offsets, pitch, slots_end = model_layout(wins)
	assert ctx.window_set_size == len(wins)
	assert ctx.window_set_layout == (offsets, pitch)
	expected = [[window_bodies(w, b, e) for b, e in wins] for w in walked]
	for unaligned in (False, True):
		want = [[x[1 if unaligned else 0] for x in per_kind] for per_kind in expected]
		if "rows" in forms:
			got = ctx.splice_window_set(rows, unaligned=unaligned)
			assert len(got) == len(rows)
			for i, pieces in enumerate(got):
				if pieces != want[kind_of_row[i]]:   # (name the first piece that differs)
					for k, (a, w) in enumerate(zip(pieces, want[kind_of_row[i]])):
						assert a == w, "window %d [%d, %d) unaligned=%s row %d: %d bytes, expected %d" % (k, wins[k][0], wins[k][1], unaligned, i, len(a), len(w))
					assert len(pieces) == len(wins)
		if "device" in forms:
			import torch
			dpitch = slots_end + (48 if unaligned else 0) if len(wins) % 2 else pitch
			buf = torch.full((len(rows) * dpitch + 64,), 0x55, dtype=torch.uint8, device="cuda")
			lengths = ctx.splice_window_set_device(rows, buf.data_ptr(), dpitch, unaligned=unaligned, want_lengths=True)
			ctx.synchronize()
			host = buf.cpu().numpy()
			assert lengths.shape == (len(rows), len(wins))
			for i in range(len(rows)):
				record = host[i * dpitch:(i + 1) * dpitch]
				untouched = np.ones(dpitch, dtype=bool)
				for k, w in enumerate(want[kind_of_row[i]]):
					assert int(lengths[i, k]) == len(w), "device lengths, window %d row %d unaligned=%s" % (k, i, unaligned)
					assert record[offsets[k]:offsets[k] + len(w)].tobytes() == w, "device, window %d row %d unaligned=%s" % (k, i, unaligned)
					untouched[offsets[k]:offsets[k] + (len(w) if unaligned else (len(w) + 15) // 16 * 16)] = False
				assert (record[untouched] == 0x55).all(), "row %d unaligned=%s: bytes outside the pieces were written" % (i, unaligned)
			assert (host[len(rows) * dpitch:] == 0x55).all()
	# the same context's column-window calls, every seventh window
	for k in range(0, len(wins), 7):
		b, e = wins[k]
		ctx.set_column_window(b, e)
		for unaligned in (False, True):
			got = ctx.splice_rows(rows, unaligned=unaligned)
			for i, a in enumerate(got):
				assert a == expected[kind_of_row[i]][k][1 if unaligned else 0], "column window %d [%d, %d) unaligned=%s row %d" % (k, b, e, unaligned, i)
	ctx.set_column_window(0, int(g.aligned_positions[-1]))


def edge_geometry(g):
	ap = np.asarray(g.aligned_positions, dtype=np.int64)
	csum = np.asarray(g.alt_edge_count_csum, dtype=np.int64)
	src = np.repeat(np.arange(len(ap) - 1), np.diff(csum)[:len(ap) - 1])
	begin, end = ap[src], ap[np.asarray(g.alt_edge_targets, dtype=np.int64)]
	llen = np.diff(np.asarray(g.label_offsets, dtype=np.int64))
	return begin, end, llen


def back_to_back(start, lengths, L):
	out, at = [], max(0, start)
	for n in lengths:
		if at + n <= L:
			out.append((at, at + n))
		at += n
	return out


def seam_windows(g):
	"""Case 3: the slot-seam lengths back to back from column 0, over a label, over padding and inside the longest deletion's span,
	with one window three times."""
	L = int(g.aligned_positions[-1])
	begin, end, llen = edge_geometry(g)
	wins = back_to_back(0, SEAM_LENGTHS, L)
	lab = int(np.argmax(llen))
	wins += back_to_back(int(begin[lab]) - 20, SEAM_LENGTHS, L)
	padded = int(np.argmax((end - begin) - llen))
	wins += back_to_back(int(begin[padded]) + int(llen[padded]) - 20, SEAM_LENGTHS, L)
	d = int(np.argmax(end - begin))
	wins += back_to_back(int(begin[d]) + int(end[d] - begin[d]) // 3, SEAM_LENGTHS, L)
	return wins + [wins[7]] * 3


def tile_seam_windows(L):
	"""Case 4: windows of a tile +- 1 and of two tiles + 1, from a tile boundary and from 37 before one, with one-column windows between
	them (a short tile follows a full one in tile order)."""
	wins = []
	for start in (TILE, 2 * TILE - 37):
		for n in (TILE - 1, TILE, TILE + 1, 2 * TILE + 1):
			wins.append((start, min(L, start + n)))
			wins.append((start + n // 2, start + n // 2 + 1))
	return wins


def many_short_windows(L, n=3000, seed=5):
	rng = np.random.default_rng(seed)
	begins = rng.integers(0, L - 40, size=n)
	return [(int(b), int(b) + int(k)) for b, k in zip(begins, rng.integers(1, 41, size=n))]


def founder_rows(g, rng, counts):
	bridges = _bridges(g)
	H = g.total_chromosome_copies
	rows = []
	for k in counts:
		cuts = [0] + sorted(int(x) for x in rng.choice(bridges, size=min(k, len(bridges)), replace=False))
		copies = [int(x) for x in rng.integers(0, H, size=len(cuts))]
		copies[1] = PLOIDY_MAX
		rows.append(list(zip(cuts, copies)))
	return rows


# ---- 1: reference fixtures -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stem,fasta", FIXTURES)
def test_reference_fixtures_all_windows(v2m, ctx, stem, fasta):
	g = _fixture_graph(stem, fasta)
	L = int(g.aligned_positions[-1])
	rows = [PLOIDY_MAX] + list(range(g.total_chromosome_copies))
	check_set(v2m, ctx, g, rows, [(b, e) for b in range(L) for e in range(b + 1, L + 1)], forms=("rows", "device"))


# ---- 2: synthetic seeds ----------------------------------------------------------------------------------------------------------

def _synthetic(tmp_path, seed):
	rng = np.random.default_rng(900 + seed)
	ref_len = int(rng.integers(2000, 70000))
	g = synth.build_case(tmp_path, 7000 + seed, ref_len, int(rng.integers(1, max(2, ref_len // 40))), int(rng.integers(1, 4)),
		multi_allelic=float(rng.choice([0.0, 0.2])), long_every=int(rng.choice([0, 13, 50])), max_indel=int(rng.choice([8, 64])))
	g = synth.with_random_paths(g, seed, float(rng.choice([0.05, 0.3, 0.8])))
	return g, rng


@pytest.mark.parametrize("seed", range(32))
def test_synthetic_random_paths(v2m, ctx, tmp_path, seed):
	g, rng = _synthetic(tmp_path, seed)
	rows = [PLOIDY_MAX] + list(range(g.total_chromosome_copies))
	check_set(v2m, ctx, g, rows, window_classes(g, rng), forms=("rows", "device") if seed % 8 == 0 else ("rows",))


# ---- 3, 4, 5: seams and many short tiles -----------------------------------------------------------------------------------------

def _seam_case(tmp_path):
	return synth.with_random_paths(synth.build_case(tmp_path, 41, 60000, 1500, 3, multi_allelic=0.2, long_every=30, max_indel=64), 6, 0.3)


def test_slot_seams(v2m, ctx, tmp_path):
	g = _seam_case(tmp_path)
	rows = [PLOIDY_MAX] + list(range(g.total_chromosome_copies))
	check_set(v2m, ctx, g, rows, seam_windows(g), forms=("rows", "device"))


def test_tile_seams_within_a_window(v2m, ctx, tmp_path):
	g = synth.with_random_paths(synth.build_case(tmp_path, 31, 90000, 4000, 4, multi_allelic=0.2, long_every=40), 3, 0.3)
	rows = [PLOIDY_MAX] + list(range(g.total_chromosome_copies))
	check_set(v2m, ctx, g, rows, tile_seam_windows(int(g.aligned_positions[-1])), forms=("rows", "device"))


def _many_case(tmp_path):
	g = synth.with_random_paths(synth.build_case(tmp_path, 43, 70000, 2500, 4, multi_allelic=0.2, long_every=25), 7, 0.3)
	rows = [PLOIDY_MAX] + list(range(g.total_chromosome_copies)) + founder_rows(g, np.random.default_rng(43), (4, 40))
	return g, rows


def test_many_short_tiles(v2m, ctx, tmp_path):
	g, rows = _many_case(tmp_path)
	check_set(v2m, ctx, g, rows, many_short_windows(int(g.aligned_positions[-1])), forms=("rows", "device"))


# ---- 6, 7: one window, windows no edge reaches -----------------------------------------------------------------------------------

def test_a_set_of_one_window(v2m, ctx, tmp_path):
	g, rng = _synthetic(tmp_path, 3)
	rows = [PLOIDY_MAX] + list(range(g.total_chromosome_copies))
	ctx.upload_graph(v2m.VariantGraph.from_object(g), g.ref)
	walked = walk_rows(g, rows)
	for w in window_classes(g, rng):
		check_set(v2m, ctx, g, rows, [w], walked=walked, upload=False)   # (window 0 is also compared with set_column_window)


def test_only_windows_no_edge_reaches(v2m, ctx, tmp_path):
	g = synth.with_random_paths(synth.build_case(tmp_path, 12, 50000, 300, 3, long_every=30), 2, 0.5)
	begin, end, _ = edge_geometry(g)
	order = np.argsort(begin, kind="stable")
	reach = np.maximum.accumulate(end[order])
	gaps = np.nonzero(begin[order][1:] > reach[:-1] + 2)[0]
	assert gaps.size >= 5
	wins = [(int(reach[i]) + 1, int(begin[order][i + 1]) - 1) for i in gaps[::max(1, gaps.size // 20)]]
	rows = [PLOIDY_MAX] + list(range(g.total_chromosome_copies))
	ref_row = column_walk(g)[0]
	check_set(v2m, ctx, g, rows, wins, forms=("rows", "device"))
	for pieces in ctx.splice_window_set(rows):
		assert pieces == [ref_row[b:e] for b, e in wins]   # nothing to resolve: every piece is the REF row's


# ---- 8: serial resolve -----------------------------------------------------------------------------------------------------------

def test_serial_resolve_under_sets(v2m, ctx, tmp_path, monkeypatch):
	monkeypatch.setenv("V2M_MAX_BACK_WORDS", "0")
	g = synth.with_random_paths(synth.build_case(tmp_path, 55, 200000, 12000, 4, long_every=9, max_indel=200, multi_allelic=0.3), 8, 0.5)
	rows = [PLOIDY_MAX] + list(range(g.total_chromosome_copies))
	L = int(g.aligned_positions[-1])
	walked = walk_rows(g, rows)
	check_set(v2m, ctx, g, rows, [(100, 400), (L - 500, L - 100)], walked=walked)                    # the hull is about the whole row
	check_set(v2m, ctx, g, rows, [(L // 2, L // 2 + 300), (L // 2 + 300, L // 2 + 900), (L // 2 - 50, L // 2 + 10)], walked=walked, upload=False)


# ---- 9: founder rows -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("max_back", [None, "0"])
def test_founder_rows_with_cuts(v2m, ctx, tmp_path, monkeypatch, max_back):
	if max_back is not None:
		monkeypatch.setenv("V2M_MAX_BACK_WORDS", max_back)
	g = synth.with_random_paths(synth.build_case(tmp_path, 31, 90000, 4000, 6, multi_allelic=0.2, long_every=40), 3, 0.3)
	rng = np.random.default_rng(4)
	bridges = _bridges(g)
	rows = [PLOIDY_MAX] + list(range(g.total_chromosome_copies)) + founder_rows(g, rng, (5, 40, 400)) + [[(bridges[len(bridges) // 2], 1)]]
	check_set(v2m, ctx, g, rows, window_classes(g, rng, n_random=10), forms=("rows", "device"))


# ---- 10: row groups and stores ---------------------------------------------------------------------------------------------------

def _many_rows(tmp_path):
	g, kinds = _many_case(tmp_path)
	return g, kinds, [i % len(kinds) for i in range(311)]


@pytest.mark.parametrize("rows_per_group,count_rows", [("1", "7"), ("17", "1"), ("256", None)])
def test_row_groups(v2m, ctx, tmp_path, monkeypatch, rows_per_group, count_rows):
	monkeypatch.setenv("V2M_ROWS_PER_GROUP", rows_per_group)
	if count_rows is not None:
		monkeypatch.setenv("V2M_COUNT_ROWS_PER_GROUP", count_rows)
	g, kinds, kind_of_row = _many_rows(tmp_path)
	walked = walk_rows(g, kinds)
	rows = [kinds[k] for k in kind_of_row]
	check_set(v2m, ctx, g, rows, seam_windows(g), walked=walked, kind_of_row=kind_of_row)
	check_set(v2m, ctx, g, rows, many_short_windows(int(g.aligned_positions[-1])), walked=walked, kind_of_row=kind_of_row, upload=False)


def test_default_row_groups_of_many_rows(v2m, ctx, tmp_path):
	"""No knob: the set's own choice of rows per group (from the mean tile length) over 311 rows."""
	g, kinds, kind_of_row = _many_rows(tmp_path)
	rows = [kinds[k] for k in kind_of_row]
	check_set(v2m, ctx, g, rows, many_short_windows(int(g.aligned_positions[-1]), n=500), walked=walk_rows(g, kinds), kind_of_row=kind_of_row)


@pytest.mark.parametrize("nt,unaligned_store", [("0", "plain"), ("1", "nt")])
def test_store_flavours_forced(v2m, ctx, tmp_path, monkeypatch, nt, unaligned_store):
	monkeypatch.setenv("V2M_NT_STORES", nt)
	monkeypatch.setenv("V2M_UNALIGNED_STORE", unaligned_store)
	g = _seam_case(tmp_path)
	rows = [PLOIDY_MAX] + list(range(g.total_chromosome_copies))
	walked = walk_rows(g, rows)
	check_set(v2m, ctx, g, rows, seam_windows(g), forms=("rows", "device"), walked=walked)
	check_set(v2m, ctx, g, rows, many_short_windows(int(g.aligned_positions[-1]), n=700), forms=("rows", "device"), walked=walked, upload=False)
	check_set(v2m, ctx, g, rows, window_classes(g, np.random.default_rng(41)), forms=("rows", "device"), walked=walked, upload=False)


# ---- 11: cache limits ------------------------------------------------------------------------------------------------------------

def test_cache_limits(v2m, ctx, tmp_path, monkeypatch):
	g = synth.extreme_spans_case(tmp_path, dense_tile=True)
	begin, end, llen = edge_geometry(g)
	dense = int(np.argmax(np.bincount(begin // TILE)))
	d, i = int(np.argmax(end - begin)), int(np.argmax(llen))
	j = int(np.nonzero((llen > 1024) & (llen < 2000))[0][0])
	L = int(g.aligned_positions[-1])
	db, de, ib, jb = int(begin[d]), int(end[d]), int(begin[i]), int(begin[j])
	wins = [(db + 5000, db + 90000), (db - 100, db + 20000), (db + 70000, de - 70000), (ib + 1000, ib + int(llen[i]) + 500), (ib - 50, ib + 40000),
		(dense * TILE + 100, min(L, (dense + 2) * TILE + 9)), (dense * TILE - 3000, dense * TILE + 9000), (jb + 10, jb + 1400), (0, L)]
	wins += back_to_back(dense * TILE + 500, SEAM_LENGTHS * 3, L) + [(dense * TILE + 3000, dense * TILE + 3300), (dense * TILE + 16000, dense * TILE + 16700)]
	wins += back_to_back(ib + 30000, SEAM_LENGTHS, L) + [(ib + 20000, ib + 20300)]
	rows = [PLOIDY_MAX] + list(range(6)) + [[(0, 0), (g.node_count - 3, 3)]]
	walked = walk_rows(g, rows)
	check_set(v2m, ctx, g, rows, wins, forms=("rows", "device"), walked=walked)
	monkeypatch.setenv("V2M_ROWS_PER_GROUP", "40")                  # 48 rows in one group of 40: rows 16.. use the uncached path
	check_set(v2m, ctx, g, rows * 6, wins[:1] + wins[5:7] + wins[9:], walked=walked, kind_of_row=list(range(len(rows))) * 6, upload=False)


# ---- 12: small ring slices -------------------------------------------------------------------------------------------------------

def test_small_ring_slices(v2m, ctx, tmp_path, monkeypatch):
	monkeypatch.setenv("V2M_RING_SLOT_BYTES", str(1 << 18))
	g = _seam_case(tmp_path)
	kinds = [PLOIDY_MAX] + list(range(g.total_chromosome_copies))
	kind_of_row = [i % len(kinds) for i in range(45)]
	rows = [kinds[k] for k in kind_of_row]
	wins = [(1000, 1000 + TILE + 5)] + seam_windows(g) + [(30000, 33000)]     # ~21 KB a record: a dozen rows a slice
	_, pitch, _ = model_layout(wins)
	assert 3 * pitch < (1 << 18) < len(rows) * pitch // 3
	check_set(v2m, ctx, g, rows, wins, walked=walk_rows(g, kinds), kind_of_row=kind_of_row)


# ---- 13: state -------------------------------------------------------------------------------------------------------------------

def test_state_and_errors(v2m, tmp_path):
	import vcf2multialign_amd._native as N
	g = synth.with_random_paths(synth.build_case(tmp_path, 12, 50000, 2000, 3, long_every=30), 2, 0.3)
	rows = [PLOIDY_MAX] + list(range(g.total_chromosome_copies))
	vg = v2m.VariantGraph.from_object(g)
	L = int(g.aligned_positions[-1])
	wins = [(100, 200), (L - 5000, L), (150, 170), (20000, 20000 + TILE + 3)]
	walked = walk_rows(g, rows)
	want = {u: [[window_bodies(w, b, e)[u] for b, e in wins] for w in walked] for u in (0, 1)}
	arr = lambda xs: np.ascontiguousarray(xs, dtype=np.uint64)
	with v2m.Context(0) as plain, v2m.Context(0) as c:
		one = arr([0]), arr([1])
		assert c._lib.v2m_set_window_set(c._h, 1, one[0].ctypes.data, one[1].ctypes.data) == N.V2M_ERR_STATE
		assert c.window_set_size == 0
		plain.upload_graph(vg, g.ref)
		c.upload_graph(vg, g.ref)
		with pytest.raises(v2m.V2MError) as err:
			c.splice_window_set(rows)
		assert err.value.code == N.V2M_ERR_STATE
		assert c._lib.v2m_set_window_set(c._h, 0, None, None) == N.V2M_ERR_INVALID_ARGUMENT
		for bad, b, e in ((1, 5, 5), (2, 9, 3), (0, 0, L + 1), (3, L, L + 1)):
			begins, ends = arr([10, 10, 10, 10]), arr([20, 20, 20, 20])
			begins[bad], ends[bad] = b, e
			assert c._lib.v2m_set_window_set(c._h, 4, begins.ctypes.data, ends.ctypes.data) == N.V2M_ERR_INVALID_ARGUMENT
			assert ("window %d" % bad) in c._lib.v2m_last_error(c._h).decode()
		assert c.window_set_size == 0

		whole = {u: plain.splice_rows(rows, unaligned=bool(u)) for u in (0, 1)}
		c.set_window_set(wins)
		assert c.window_set_size == len(wins)
		# the row calls never see the set; a column window does not change the set
		for u in (0, 1):
			assert c.splice_rows(rows, unaligned=bool(u)) == whole[u]
			assert c.splice_window_set(rows, unaligned=bool(u)) == want[u]
		assert c.window_length == L and c.min_row_pitch == plain.min_row_pitch and c.max_unaligned_length == plain.max_unaligned_length
		c.set_column_window(300, 900)
		plain.set_column_window(300, 900)
		for u in (0, 1):
			assert c.splice_window_set(rows, unaligned=bool(u)) == want[u]
			assert c.splice_rows(rows, unaligned=bool(u)) == plain.splice_rows(rows, unaligned=bool(u))
		c.set_window_set(wins[:2])                                  # a new set does not touch the column window
		assert c.window_length == 600
		for u in (0, 1):
			assert c.splice_window_set(rows, unaligned=bool(u)) == [p[:2] for p in want[u]]
			assert c.splice_rows(rows, unaligned=bool(u)) == plain.splice_rows(rows, unaligned=bool(u))
		# BGZF through the set call, bad pitches
		with pytest.raises(v2m.V2MError) as err:
			c.splice_window_set(rows, bgzf=True)
		assert err.value.code == N.V2M_ERR_UNSUPPORTED
		import torch
		buf = torch.zeros(1 << 20, dtype=torch.uint8, device="cuda")
		_, _, slots_end = model_layout(wins[:2])
		for pitch in (slots_end - 16, slots_end + 8):
			with pytest.raises(v2m.V2MError) as err:
				c.splice_window_set_device(rows, buf.data_ptr(), pitch)
			assert err.value.code == N.V2M_ERR_INVALID_ARGUMENT
		c.upload_graph(vg, g.ref)                                   # a new upload drops the set (and the window)
		assert c.window_set_size == 0 and c._lib.v2m_window_set_pitch(c._h) == 0
		with pytest.raises(v2m.V2MError) as err:
			c.splice_window_set(rows)
		assert err.value.code == N.V2M_ERR_STATE


def test_unaligned_refuses_a_nul_byte(v2m, tmp_path):
	import vcf2multialign_amd._native as N
	g = _fixture_graph("test-4", "test-4.fa")
	ref = bytearray(g.ref)
	ref[2] = 0
	with v2m.Context(0) as c:
		c.upload_graph(v2m.VariantGraph.from_object(g), bytes(ref))
		c.set_window_set([(0, 3), (1, 5)])
		assert [[len(x) for x in p] for p in c.splice_window_set([PLOIDY_MAX])] == [[3, 4]]   # aligned mode keeps such bytes
		with pytest.raises(v2m.V2MError) as err:
			c.splice_window_set([PLOIDY_MAX], unaligned=True)
		assert err.value.code == N.V2M_ERR_UNSUPPORTED


# ---- 14: the checked build -------------------------------------------------------------------------------------------------------

CHECKED_CORPUS = ["tests/test_gpu_window_sets.py::" + name for name in (
	"test_reference_fixtures_all_windows", "test_synthetic_random_paths", "test_slot_seams", "test_tile_seams_within_a_window",
	"test_many_short_tiles", "test_founder_rows_with_cuts", "test_cache_limits")]


def test_sets_on_the_checked_build():
	"""No chunk past a short tile's end is read from LDS nobody filled: the poisoned build gives the same pieces under both seeds."""
	from test_gpu_checked_build import SEEDS, run_checked_corpus
	from vcf2multialign_amd import build
	assert os.path.exists(build.CHECKED_LIB_PATH) and os.path.exists(build.CHECKED_HOST_LIB_PATH), "build_native() builds them"
	for seed in SEEDS:   # the second seed only once the first has passed
		rc, out = run_checked_corpus(seed, build.CHECKED_LIB_PATH, build.CHECKED_HOST_LIB_PATH, corpus=CHECKED_CORPUS)
		assert rc == 0, "checked build, seed %s: exit %d\n%s" % (seed, rc, out[-6000:])
		assert " passed" in out, out[-3000:]


# ---- 15: the CLI -----------------------------------------------------------------------------------------------------------------

def _run(args, cwd, env=None):
	return subprocess.run([CLI] + args, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)


def _bed(R, seed=15, n=40):
	"""~40 regions, overlapping and unsorted, every other one named, one line of another chromosome, one comment line, one range twice."""
	rng = np.random.default_rng(seed)
	regions, lines = [], [b"# regions of the test", b"track name=test"]
	for i in range(n):
		s = int(rng.integers(0, R - 1))
		e = int(min(R, s + 1 + rng.integers(0, [40, 3000, 20000][i % 3])))
		if i == 5:
			s, e = regions[2][1], regions[2][2]
		name = "gene_%d" % i if i % 2 == 0 else "1_%d_%d" % (s, e)
		if name in [r[0] for r in regions]:
			continue
		regions.append((name, s, e))
		lines.append(b"1\t%d\t%d" % (s, e) + (b"\t%s\t0\t+" % name.encode() if i % 2 == 0 else b""))
		if i == 9:
			lines.append(b"2\t10\t500\tother_chromosome")
		if i == 20:
			lines.append(b"")
	regions += [("first_base", 0, 1), ("last_base", R - 1, R), ("whole", 0, R)]
	lines += [b"1\t0\t1\tfirst_base", b"1\t%d\t%d\tlast_base" % (R - 1, R), b"1\t0\t%d\twhole" % R]
	return regions, b"\n".join(lines) + b"\n"


def _check_regions_against_region_runs(tmp_path, tag, input_args, mode, flags, regions, bed_path, suffix):
	from concurrent.futures import ThreadPoolExecutor
	out = tmp_path / ("regions_" + tag)
	out.mkdir()
	env = dict(os.environ, V2M_REGIONS_PER_PASS="7")                                  # several passes
	r = _run(input_args + mode + flags + ["--device=0", "--regions-file=" + str(bed_path), "--verbose"], out, env=env)
	assert r.returncode == 0, r.stderr.decode()
	assert sorted(os.listdir(out)) == sorted(name + suffix for name, _, _ in regions)
	single = tmp_path / ("single_" + tag)
	single.mkdir()

	def one(region):
		name, s, e = region
		return _run(input_args + mode + flags + ["--device=0", "-s", str(single / (name + suffix)), "--region=%d-%d" % (s + 1, e)], single)
	with ThreadPoolExecutor(8) as pool:
		for region, rr in zip(regions, pool.map(one, regions)):
			assert rr.returncode == 0, rr.stderr.decode()
	headers = None
	for name, s, e in regions:
		got, want = (out / (name + suffix)).read_bytes(), (single / (name + suffix)).read_bytes()
		assert got == want, "%s: %s [%d, %d)" % (tag, name, s, e)
		assert headers is None or [h for h, _ in _records(got)] == headers
		headers = [h for h, _ in _records(got)]
	return r, headers


@pytest.mark.parametrize("omit", [False, True], ids=["with_ref", "omit_reference"])
@pytest.mark.parametrize("unaligned", [False, True], ids=["aligned", "unaligned"])
@pytest.mark.parametrize("founders", [False, True], ids=["haplotypes", "founders"])
def test_cli_regions_file(tmp_path, founders, unaligned, omit):
	g = synth.build_case(tmp_path, 41, 60000, 1500, 5, long_every=25, multi_allelic=0.1)
	fa, vcf = str(tmp_path / "synth.fa"), str(tmp_path / "synth.vcf")
	regions, bed = _bed(len(g.ref))
	bed_path = tmp_path / "regions.bed"
	bed_path.write_bytes(bed)
	mode = ["-F", "3", "-d", "10"] if founders else ["-H"]
	flags = (["--unaligned"] if unaligned else []) + (["--omit-reference"] if omit else []) + ["-m", "chrT"]
	suffix = ".fa" if unaligned else ".a2m"
	r, headers = _check_regions_against_region_runs(tmp_path, "vcf", ["-r", fa, "-a", vcf, "-c", "1"], mode, flags, regions, bed_path, suffix)
	assert ("%d regions taken, 1 lines of other chromosomes skipped" % len(regions)).encode() in r.stderr
	assert b"passes of at most 7 regions" in r.stderr
	ids = [] if omit else ["chrT\tREF"]
	if founders:
		ids += ["chrT\t%d" % (1 + k) for k in range(3)]
	else:
		ids += ["chrT\t%s-%d" % (s, 1 + c) for si, s in enumerate(g.sample_names) for c in range(int(g.ploidy_csum[si + 1]) - int(g.ploidy_csum[si]))]
	assert headers == [i.encode() for i in ids]
	if not founders and not omit:
		# the bodies themselves, against the column-tracking walk
		rows = [PLOIDY_MAX] + list(range(g.total_chromosome_copies))
		walked = walk_rows(g, rows)
		for name, s, e in regions[::5]:
			b, en = oracle_cols(g, s, e)
			got = _records((tmp_path / "regions_vcf" / (name + suffix)).read_bytes())
			assert [x for _, x in got] == [window_bodies(w, b, en)[1 if unaligned else 0] for w in walked], name
	if not omit:
		# the same from a graph checkpoint; without --chromosome every line of the BED file is taken
		graph = str(tmp_path / "graph.bin")
		w = _run(["-H", "-r", fa, "-a", vcf, "-c", "1", "-f", graph, "--device=0", "-s", "/dev/null"], tmp_path)
		assert w.returncode == 0, w.stderr.decode()
		_check_regions_against_region_runs(tmp_path, "graph", ["-r", fa, "-g", graph], mode, flags, regions + [("other_chromosome", 10, 500)], bed_path, suffix)
