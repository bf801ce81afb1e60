"""The row kernels at every cache limit and every chunk mask: splice_aligned_kernel, count_unaligned_kernel, splice_unaligned_kernel, their
window forms and resolve_effective_edges_kernel in front of them, on the hand-made graphs of tests/seam_graphs.py.

Every case is compared with the numpy model of seam_graphs.py and with the oracle's output_sequence, aligned and unaligned, through
splice_rows; where the case is about stores also through splice_rows_device into a buffer filled with a guard byte, at a pitch wider
than the row (aligned: nothing written past the length rounded up to 16; unaligned: nothing past the row's bytes; the lengths are the
model's).  That the graphs put the named values in front of the kernels is what tests/test_seam_graphs_host.py asserts, without a GPU.

Groups (the issue's letters):  a  every 16-bit keep-mask of a chunk x 16 destination phases x both routes to pack_chunk_and_store_exact
(the workgroup's queue, packed a row later by a rotating wave; slots packed in place), whole rows and column windows, both store
flavours;  b  short-chunk counts per row tile around the queue's size and the slots' ends, an all-padding tile, an empty window row, a
one-row group;  c  the patch cache: n_range and n_cross + n_range at the tables' sizes, the label slice, spans at the 16-bit limit,
patch lengths at kLongPatch, the long-patch queue, edges at tile boundaries, the row groups' sizes;  d  tile geometry and tile runs;
e  resolve: restart distances at V2M_MAX_BACK_WORDS, blocker / blocked pairs across word, thread and workgroup boundaries, the last word's
tail;  f  a, b, c and e again on the checked build.

Left out, by name:
  * resolve's blocker "as bit 0 of the word after its blocked edge": edges are ordered by source node and a blocker precedes what it
    blocks, so no graph v2m_upload_graph accepts has it; the pairs are (bit 63, bit 0 of the next word) and (bit 0, bit 63 of one word).
  * kCountRowsMax rows per group through splice_rows: a call's rows are cut into slices of at most 128 MB, fewer than kCountRowsMax rows of
    the cache graph; the case runs through splice_rows_device, which launches all rows at once."""

import os

import numpy as np
import pytest

import seam_graphs as S

pytestmark = pytest.mark.gpu

K = S.kernel_constants()
T = K.kTileBytes
GUARD = 0xA5                    # in no reference byte, label byte or padding


@pytest.fixture(scope="module")
def v2m():
	import vcf2multialign_amd as v
	return v


@pytest.fixture(scope="module")
def ctx(v2m):
	c = v2m.Context(0)
	yield c
	c.close()


def _same(got, want, what):
	if got == want:
		return
	a, w = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
	n = min(a.size, w.size)
	d = np.flatnonzero(a[:n] != w[:n])
	at = int(d[0]) if d.size else n
	raise AssertionError("%s: %d bytes, %d expected, %d differ, the first at %d (tile %d, chunk %d): got %r, expected %r" % (
		what, a.size, w.size, d.size, at, at // T, at % T // 16, got[max(0, at - 8):at + 24], want[max(0, at - 8):at + 24]))


def _row_name(row):
	"""A copy's number; a row with cuts by its first cuts."""
	return str(row) if isinstance(row, (int, np.integer)) else "%d cuts: %s ..." % (len(row), list(row[:3]))


def _expected(sg, rows, unaligned, window):
	"""The model's bodies, held equal to the oracle's."""
	by_row = {}
	for r in rows:
		key = sg.row_key(r)
		if key not in by_row:
			by_row[key] = sg.body(r, unaligned, window)
			assert by_row[key] == sg.oracle_body(r, unaligned, window), "model and oracle differ: %s row %s" % (sg.name, r)
	return [by_row[sg.row_key(r)] for r in rows]


def check(v2m, ctx, sg, rows, windows=(None,), device=False, modes=(False, True), upload=True):
	if upload:
		ctx.upload_graph(v2m.VariantGraph.from_object(sg.g), sg.g.ref)
	for window in windows:
		name = "%s %s" % (sg.name, "whole" if window is None else "%s [%d, %d)" % window)
		b, e = (0, sg.length) if window is None else window[1:]
		ctx.set_column_window(b, e)
		for unaligned in modes:
			want = _expected(sg, rows, unaligned, None if window is None else (b, e))
			got = ctx.splice_rows(rows, unaligned=unaligned)
			assert len(got) == len(want)
			for i, (a, w) in enumerate(zip(got, want)):
				_same(a, w, "%s unaligned=%s row %d (%s)" % (name, unaligned, i, _row_name(rows[i])))
			if device:
				_check_device(ctx, rows, want, unaligned, name)
	ctx.set_column_window(0, sg.length)


def _check_device(ctx, rows, want, unaligned, name):
	import torch
	need = ctx.max_unaligned_length if unaligned else ctx.window_length
	pitch = (need + 15) // 16 * 16 + 64                 # wider than any row
	buf = torch.full((len(rows) * pitch + 64,), GUARD, dtype=torch.uint8, device="cuda")
	lengths = ctx.splice_rows_device(rows, buf.data_ptr(), pitch, unaligned=unaligned, want_lengths=True)
	ctx.synchronize()
	host = buf.cpu().numpy()
	del buf
	for i, w in enumerate(want):
		row = host[i * pitch:(i + 1) * pitch]
		assert int(lengths[i]) == len(w), "%s device unaligned=%s row %d: length %d, expected %d" % (name, unaligned, i, int(lengths[i]), len(w))
		_same(row[:len(w)].tobytes(), w, "%s device unaligned=%s row %d (%s)" % (name, unaligned, i, _row_name(rows[i])))
		written_to = len(w) if unaligned else (len(w) + 15) // 16 * 16
		stray = np.flatnonzero(row[written_to:] != GUARD)
		assert 0 == stray.size, "%s device unaligned=%s row %d: %d bytes written past the row, the first at %d (row length %d)" % (name, unaligned, i, stray.size, written_to + int(stray[0]), len(w))
	assert np.all(host[len(rows) * pitch:] == GUARD)


# ---- a. every chunk mask -------------------------------------------------------------------------------------------------------------------

MASK_GRAPHS = {"s0": (0, 0), "s0_rotated": (0, K.kTileChunks // 4), "s7": (7, 0)}
MASK_ROWS_PER_GROUP = 8          # 2 x 8 + 1 = 17 rows = REF, the 15 phase copies, the copy with no bit set: two full groups and a ragged one


@pytest.mark.parametrize("store", ["plain", "nt"])
@pytest.mark.parametrize("which", sorted(MASK_GRAPHS))
def test_every_chunk_mask(v2m, ctx, monkeypatch, which, store):
	"""All 65 536 keep-masks of a 16-byte chunk at all 16 destination phases through pack_chunk_and_store_exact (the census: through the queue
	in s7, in place in s0 and s0_rotated together), in rows that begin at 16 different phases.  17 rows in groups of 8: every wave takes the
	packing turn ((row + pass) & 3), and the extra round after a group's last row runs for a full group and for a group of one row."""
	monkeypatch.setenv("V2M_UNALIGNED_STORE", store)
	monkeypatch.setenv("V2M_NT_STORES", "1" if "nt" == store else "0")
	monkeypatch.setenv("V2M_ROWS_PER_GROUP", str(MASK_ROWS_PER_GROUP))
	sg = S.mask_graph(*MASK_GRAPHS[which])
	rows = S.mask_rows(MASK_ROWS_PER_GROUP)
	assert len(rows) == 2 * MASK_ROWS_PER_GROUP + 1 and set(rows) == set(sg.rows)
	check(v2m, ctx, sg, rows, device=True, modes=(True,) if "nt" == store else (True, False))


@pytest.mark.parametrize("which,store", [("s0", "nt"), ("s0_rotated", "plain"), ("s7", "nt"), ("s7", "plain")])
def test_every_chunk_mask_under_windows(v2m, ctx, monkeypatch, which, store):
	"""splice_unaligned_window_kernel on the same graphs: a window whose first column is a multiple of 16 but not of the tile, one that is odd
	(every chunk of it straddles two masks), one that ends in the middle of a chunk."""
	monkeypatch.setenv("V2M_UNALIGNED_STORE", store)
	monkeypatch.setenv("V2M_ROWS_PER_GROUP", str(MASK_ROWS_PER_GROUP))
	sg = S.mask_graph(*MASK_GRAPHS[which])
	check(v2m, ctx, sg, S.mask_rows(MASK_ROWS_PER_GROUP), windows=sg.notes["windows"], device="s0" == which)


# ---- b. short chunks per row tile -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("rows_per_group", [None, "1", "3"])
def test_short_chunk_counts(v2m, ctx, monkeypatch, rows_per_group):
	"""Row tiles with exactly 0, 1, 63, 64, 65, kQueue - 1, kQueue and kQueue + 1 short chunks, in a tile's first and last chunk and either side of
	a slot's end; the first slot that does not fit the queue with empty and with full slots after it; a tile that is all padding in one row;
	a window in which that row is empty; groups of one row."""
	if rows_per_group:
		monkeypatch.setenv("V2M_ROWS_PER_GROUP", rows_per_group)
	sg = S.short_count_graph()
	rows = [S.PLOIDY_MAX, 0, 1, 0, 0, S.PLOIDY_MAX, 1]
	check(v2m, ctx, sg, rows, windows=[None] + sg.notes["windows"], device=True)


# ---- c. the patch cache ----------------------------------------------------------------------------------------------------------------------

G = K.kGroupRowsLds


@pytest.mark.parametrize("rows_per_group", [1, G - 1, G, G + 1, 2 * G + 1])
def test_patch_cache_limits(v2m, ctx, monkeypatch, rows_per_group):
	"""A tile per limit of the workgroup's patch cache (seam_graphs.cache_graph), in groups of 1, kGroupRowsLds - 1, kGroupRowsLds,
	kGroupRowsLds + 1 and 2 x kGroupRowsLds + 1 rows (the cached effective-edge words are reloaded every kGroupRowsLds rows), a full group and
	a ragged one.  Consecutive rows differ in every limit; the rows with kLongQueueLds - 1, kLongQueueLds and kLongQueueLds + 1 long patches in
	one tile follow one another."""
	monkeypatch.setenv("V2M_ROWS_PER_GROUP", str(rows_per_group))
	sg = S.cache_graph()
	rows = S.cache_rows(max(len(sg.rows), rows_per_group + max(1, rows_per_group // 2)))
	check(v2m, ctx, sg, rows, device=rows_per_group in (1, G + 1))


def test_patch_cache_limits_at_the_count_kernels_group_size(v2m, ctx, monkeypatch):
	"""kCountRowsMax rows per group and one row more in the call, through splice_rows_device (one launch for all rows)."""
	monkeypatch.setenv("V2M_ROWS_PER_GROUP", str(K.kCountRowsMax))
	sg = S.cache_graph()
	rows = S.cache_rows(K.kCountRowsMax + 1)
	ctx.upload_graph(v2m.VariantGraph.from_object(sg.g), sg.g.ref)
	for unaligned in (True, False):
		_check_device(ctx, rows, _expected(sg, rows, unaligned, None), unaligned, sg.name + " %d rows" % len(rows))


def test_patch_cache_limits_under_windows(v2m, ctx, monkeypatch):
	"""Windows that begin inside, at and one column after each of the limit tiles (the window kernels, and the tile tables that
	v2m_set_column_window builds with code of its own)."""
	monkeypatch.setenv("V2M_ROWS_PER_GROUP", str(G + 1))
	sg = S.cache_graph()
	rows = S.cache_rows(G + 3)
	check(v2m, ctx, sg, rows, windows=sg.notes["windows"])
	check(v2m, ctx, sg, rows[:5], windows=sg.notes["windows"][::7], device=True, upload=False)


# ---- d. tile geometry -----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("length", S.geometry_lengths())
def test_tile_geometry(v2m, ctx, length):
	"""Aligned lengths of k tiles + {-1, 0, 1, 15, 16, 17} columns; 63, 64, 65, 71 and 72 tiles (the default run of 64 tiles; a last run that the
	unaligned kernels remap over the XCDs, 72 - 64 = 8 tiles, and ones they do not)."""
	sg = S.geometry_graph(length)
	check(v2m, ctx, sg, sg.rows, device=True)


@pytest.mark.parametrize("tile_run", ["1", "8", "9"])
def test_tile_runs(v2m, ctx, monkeypatch, tile_run):
	monkeypatch.setenv("V2M_TILE_RUN", tile_run)
	for length in S.geometry_lengths()[-5:]:
		sg = S.geometry_graph(length)
		check(v2m, ctx, sg, sg.rows + [0, 1])


# ---- e. resolve ------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("back_words", [str(S.RESOLVE_BACK_WORDS), None, "0"])
@pytest.mark.parametrize("tail", [0, 1, 63])
def test_resolve_seams(v2m, ctx, monkeypatch, tail, back_words):
	"""With V2M_MAX_BACK_WORDS = b: a deletion whose restart point lies exactly b and b + 1 words back from a set edge under it (decided per word;
	handed to the serial kernel); blocker and blocked edge as bits 63 / 0 of neighbouring words at the boundaries between two words, two of a
	thread's words and two workgroups' pieces, and as bits 0 / 63 of one word; n_edges % 64 in {0, 1, 63} with the last edge set."""
	if back_words is not None:
		monkeypatch.setenv("V2M_MAX_BACK_WORDS", back_words)
	sg = S.resolve_graph(tail)
	check(v2m, ctx, sg, sg.rows)
	p, q = next(pair for pair in sg.notes["pairs"] if pair[1] == 64 * 256 * K.kResolveWordsPerThread)
	check(v2m, ctx, sg, sg.rows, windows=[("across_pieces", int(sg.begin[p]) - 700, int(sg.end[q]) + 300), ("under_deletion", int(sg.begin[sg.notes["under"][0]]) - 30, int(sg.begin[sg.notes["under"][1]]) + 9)], upload=False)


# ---- f. the checked build ---------------------------------------------------------------------------------------------------------------------

CHECKED_CORPUS = [
	"tests/test_gpu_splice_seams.py::test_every_chunk_mask[s7-plain]",
	"tests/test_gpu_splice_seams.py::test_every_chunk_mask[s0-nt]",
	"tests/test_gpu_splice_seams.py::test_every_chunk_mask_under_windows[s0-nt]",
	"tests/test_gpu_splice_seams.py::test_short_chunk_counts",
	"tests/test_gpu_splice_seams.py::test_patch_cache_limits",
	"tests/test_gpu_splice_seams.py::test_patch_cache_limits_under_windows",
	"tests/test_gpu_splice_seams.py::test_resolve_seams",
]


def test_corpus_on_the_checked_build():
	"""Groups a, b, c and e with every LDS object, scratch buffer and slot poisoned before use (tests/test_gpu_checked_build.py), both seeds."""
	from test_gpu_checked_build import SEEDS, run_checked_corpus
	from vcf2multialign_amd import build
	assert os.path.exists(build.CHECKED_LIB_PATH) and os.path.exists(build.CHECKED_HOST_LIB_PATH), "build_native() builds them"
	for seed in SEEDS:   # the second seed only once the first has passed
		rc, out = run_checked_corpus(seed, build.CHECKED_LIB_PATH, build.CHECKED_HOST_LIB_PATH, corpus=CHECKED_CORPUS, timeout=600)
		assert rc == 0, "checked build, seed %s: exit %d\n%s" % (seed, rc, out[-6000:])
		assert " passed" in out and "libv2m_hip_checked.so" in out, out[-3000:]
		print(seed, out.strip().splitlines()[-2])
