"""The transpose kernels at every column phase and span seam: transpose_bits_lines_kernel (lines8, lines16), transpose_bits_kernel (8x8) and
transpose_bits_stream_kernel (stream16), bit for bit against the plain transpose of tests/transpose_shapes.py, on that module's shape lists
(tests/test_seam_shapes_host.py asserts, without a GPU, what the lists reach).

Groups (the issue's letters); A - D call v2m_transpose_bits_device on a destination with 4096 guard words in front and behind, refilled with
the guard pattern before every launch, so a word no kernel wrote is a wrong word:
  A  phase x span seam: q whole 16-word blocks and r words more for every r, spans of 1, 2 and 3 blocks (a forward and a backward neighbour at
     every seam, last spans of one partial block), one ragged panel and whole panels plus a ragged one.  360 + 3 x 384 = 1512 launches.
  B  merged column ends: every width the host's rule accepts (17 .. 127, no multiple of 16: every overlay position DW - 16 e) and the widths
     either side of the rule, whole columns forced and the spans the host chooses.  3 x 444 = 1332 launches.
  C  ragged source panels: every fill of the last panel.  2 x 132 = 264 launches.
  D  item order: 1 .. 17 items in XCD chunks, in plain order and with either dimension fastest.  136 + 80 launches.
  E  pitch forms through the calls that make them: dense -> line-aligned (v2m_bind_path_matrix_device), line-aligned -> line-aligned (a part
     of the copies through v2m_upload_path_slice), every row spliced and compared with the bits; line-aligned -> dense (edge_major_paths in
     front of both pBWT kernels, against tests/pbwt_ref.py).  15 graphs x 8 kernels x 2 forms = 240 binds; 8 founder cases.
  F  calibration: one matrix just over launch_transpose's threshold, what ctx.info says it remembered, V2M_TRANSPOSE_CANDIDATES.
  G  one q of A, all of B and E's two row forms on the checked build (slab and input stage poisoned: a slab word nobody wrote becomes
     wrong output), both seeds."""

import os
import re

import numpy as np
import pytest

import oracle
import pbwt_ref as R
import seam_graphs as S
import transpose_shapes as T

pytestmark = pytest.mark.gpu

PANEL = "V2M_TRANSPOSE_PANEL"


@pytest.fixture(scope="module")
def v2m():
	import vcf2multialign_amd as v
	return v


@pytest.fixture(scope="module")
def ctx(v2m):
	c = v2m.Context(0)
	yield c
	c.close()


class Device:
	"""One shape on the device: the source uploaded once, the reference computed once, the guarded destination refilled before each kernel."""

	def __init__(self, ctx, SW, DW, want=None):
		import torch
		self.ctx, self.SW, self.DW = ctx, SW, DW
		self.rows, self.cols = 64 * SW, 64 * DW
		src = T.source(SW, DW)
		self.src = src
		self.want = T.transpose_ref(src, self.rows, self.cols) if want is None else want(src, self.rows, self.cols)
		self.d_src = torch.from_numpy(src.view(np.int64)).cuda()
		self.d_dst = torch.empty(self.want.size + 2 * T.GUARD_WORDS, dtype=torch.int64, device="cuda")

	def run(self, monkeypatch, kernel):
		import torch
		if kernel is None:
			monkeypatch.delenv(PANEL, raising=False)
		else:
			monkeypatch.setenv(PANEL, kernel)
		self.d_dst.fill_(T.GUARD)
		torch.cuda.synchronize()
		self.ctx.transpose_bits_device(self.d_src.data_ptr(), self.rows, self.cols, self.d_dst.data_ptr() + 8 * T.GUARD_WORDS)
		self.ctx.synchronize()
		compare(self.d_dst.cpu().numpy().view(np.uint64), self.want, kernel, self.SW, self.DW)


def compare(host, want, kernel, SW, DW):
	g, n = T.GUARD_WORDS, want.size
	what = "%s, SW %d, DW %d" % (kernel or "(calibrated)", SW, DW)
	body = host[g:g + n]
	if not np.array_equal(body, want):
		bad = np.flatnonzero(body != want)
		col, word = divmod(int(bad[0]), DW)
		raise AssertionError("%s: %d of %d words wrong, the first in destination column %d, word %d of the column (block %d, DW mod 16 = %d, the column's lines begin at word %d): %016x, expected %016x%s" % (
			what, bad.size, n, col, word, word // 16, DW % 16, -col * DW % 16, int(body[bad[0]]), int(want[bad[0]]), ", which is the guard pattern: never written" if int(body[bad[0]]) == T.GUARD else ""))
	for name, part, base in (("in front of", host[:g], -g), ("behind", host[g + n:], n)):
		stray = np.flatnonzero(part != T.GUARD)
		assert 0 == stray.size, "%s: %d guard words %s the destination overwritten, the first at word %d of the destination (DW mod 16 = %d)" % (what, stray.size, name, base + int(stray[0]), DW % 16)


# ---- A. phase x span seam ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("q", T.A_WHOLE_BLOCKS)
def test_phase_and_span_seams(ctx, monkeypatch, q):
	"""DW = 16 q + r for every r: the slab read position s_r = (-r DW) mod 16 takes every step from column to column, with q whole blocks
	carried in front of a partial one; spans of 1, 2 and 3 blocks put a forward and a backward neighbour at the seams and leave last spans
	of one partial block; the panel kernels run the same shapes."""
	for DW in T.a_widths(q):
		for SW in T.A_HEIGHTS:
			d = Device(ctx, SW, DW)
			for kernel in T.A_KERNELS:
				d.run(monkeypatch, kernel)


# ---- B. merged column ends -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("SW", T.B_HEIGHTS)
def test_merged_column_ends(ctx, monkeypatch, SW):
	"""Every width that reaches the kMerge instantiation (tests/test_seam_shapes_host.py: exactly these): the next column's first words are
	overlaid at slab position DW - 16 e, clamped to the pad word, for every DW mod 16 at 2 .. 8 blocks; and the widths the rule excludes,
	which must take the plain instantiation."""
	for DW in list(T.B_WIDTHS) + list(T.B_BOUNDARY_WIDTHS):
		d = Device(ctx, SW, DW)
		for kernel in T.B_KERNELS:
			d.run(monkeypatch, kernel)


# ---- C. ragged source panels ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("DW,kernels", T.C_CASES, ids=["%d_words" % c[0] for c in T.C_CASES])
def test_ragged_source_panels(ctx, monkeypatch, DW, kernels):
	"""Every height of 1 .. 33 words: the last panel of either geometry holds 1 .. 8 / 1 .. 16 row-words, the rest are loaded from a clamped
	address and must not be stored (21 words: merged column ends; 37: three spans of one block)."""
	for SW in T.C_HEIGHTS:
		d = Device(ctx, SW, DW)
		for kernel in kernels:
			d.run(monkeypatch, kernel)


# ---- D. item order -------------------------------------------------------------------------------------------------------------------------

def test_item_order_of_the_line_kernels(ctx, monkeypatch):
	"""n = 1 .. 17 spans of one block (every n mod 8, fewer items than XCD chunks among them), XCD chunks and plain order, panels or spans
	fastest."""
	for n in T.D_ITEMS:
		d = Device(ctx, *T.d_lines_shape(n))
		for kernel in T.D_LINES_KERNELS:
			for suffix in T.D_SUFFIXES:
				d.run(monkeypatch, kernel + suffix)


def test_item_order_of_the_panel_kernels(ctx, monkeypatch):
	for kernel in ("8x8", "stream16"):
		for grid in T.D_PANEL_GRIDS:
			d = Device(ctx, *T.d_panel_shape(kernel, grid))
			for suffix in T.D_SUFFIXES:
				d.run(monkeypatch, kernel + suffix)


# ---- E. pitch forms ------------------------------------------------------------------------------------------------------------------------

def snv_graph(k, n_copies):
	"""64 k - 5 single-column SNV sites (upper-case reference, lower-case labels, nothing overlappable): row c's byte at column e is lower
	case exactly where bit (c, e) is set.  Returns (SeamGraph, bits[copy, edge], every copy's row as the bits give it)."""
	E = T.e_edges(k)
	bits = np.random.default_rng([k, n_copies]).random((n_copies, E)) < 1 / 3
	b = S.Builder(1000 * k + n_copies)
	b.add_sites(E, 1, 1, 1)
	sg = b.finish([np.flatnonzero(row) for row in bits], name="%d SNV sites, %d copies" % (E, n_copies))
	assert sg.length == E and np.array_equal(sg.label_offsets, np.arange(E + 1))
	rows = np.where(bits, sg.label_bytes[None, :], sg.ref[None, :])
	for c in range(n_copies):
		assert rows[c].tobytes() == sg.body(c), c
		assert np.array_equal(rows[c] >= ord("a"), bits[c]), c
	assert sg.body(S.PLOIDY_MAX) == sg.ref.tobytes()
	return sg, bits, rows


def edge_major_words(bits, hp, ep):
	"""paths_by_edge_and_chrom_copy, dense: one column of hp / 64 words per edge."""
	full = np.zeros((ep, hp), dtype=bool)
	full[:bits.shape[1], :bits.shape[0]] = bits.T
	return np.packbits(full, axis=1, bitorder="little").view("<u8").reshape(-1).copy()


def same_rows(got, want, what):
	assert len(got) == want.shape[0]
	a = np.frombuffer(b"".join(got), dtype=np.uint8)
	assert a.size == want.size, "%s: %d bytes, %d expected" % (what, a.size, want.size)
	bad = np.flatnonzero(a.reshape(want.shape) != want)
	if bad.size:
		r, e = divmod(int(bad[0]), want.shape[1])
		raise AssertionError("%s: %d bytes differ, the first in row %d at edge %d (path word %d, bit %d): %r, expected %r" % (what, bad.size, r, e, e // 64, e % 64, chr(a[bad[0]]), chr(want[r, e])))


@pytest.mark.parametrize("n_copies", T.E_COPIES)
@pytest.mark.parametrize("k", T.E_PATH_WORDS)
def test_pitch_forms_through_the_path_matrix(v2m, ctx, monkeypatch, k, n_copies):
	"""(i) v2m_bind_path_matrix_device: dense source, line-aligned destination (pitch 16, 32 or 48 for 1 .. 33 path words).
	(ii) v2m_upload_path_slice of copies [8, n - 16): the packed share has a line-aligned SOURCE pitch above its word count as well.
	The context's matrix buffer is kept from one bind to the next, so before every kernel another kernel binds the complement: a word the
	kernel under test leaves out is then a wrong bit, not the previous kernel's right one."""
	import torch
	sg, bits, want = snv_graph(k, n_copies)
	E, hp, ep = T.e_edges(k), R.round64(n_copies), R.round64(T.e_edges(k))
	words = edge_major_words(bits, hp, ep)
	vg = v2m.VariantGraph.from_object(sg.g)
	vg.paths_by_chrom_copy_and_edge = None
	ctx.upload_graph(vg, sg.g.ref)
	d_words = torch.from_numpy(words.view(np.int64)).cuda()
	d_complement = torch.from_numpy((~words).view(np.int64)).cuda()
	torch.cuda.synchronize()
	ref_row = sg.ref[None, :]
	first, part = T.E_SLICE_FIRST, n_copies - T.E_SLICE_FIRST - T.E_SLICE_LEFT_OUT
	assert R.round64(part) == hp
	for kernel in T.E_KERNELS:
		scrub = "stream16" if kernel.startswith("8x8") else "8x8"
		# (i)
		monkeypatch.setenv(PANEL, scrub)
		ctx.bind_path_matrix_device(d_complement.data_ptr(), hp, ep)
		monkeypatch.setenv(PANEL, kernel)
		ctx.bind_path_matrix_device(d_words.data_ptr(), hp, ep)
		got = ctx.splice_rows(list(range(n_copies)) + [hp - 1])
		same_rows(got, np.concatenate([want, ref_row]), "%s, bound from the device under %s" % (sg.name, kernel))
		# (ii)
		monkeypatch.setenv(PANEL, scrub)
		ctx.bind_path_matrix_device(d_complement.data_ptr(), hp, ep)
		monkeypatch.setenv(PANEL, kernel)
		ctx.upload_path_slice(words, hp, ep, first, part)
		got = ctx.splice_rows(list(range(part)) + [part, hp - 1])                  # (the copies after the part are another GPU's: REF here)
		same_rows(got, np.concatenate([want[first:first + part], ref_row, ref_row]), "%s, copies [%d, %d) uploaded under %s" % (sg.name, first, first + part, kernel))
	ctx.synchronize()


@pytest.mark.parametrize("kernel", ["lines16", "lines8:1"])
@pytest.mark.parametrize("n_copies,path_words", [(130, 17), (130, 33), (1100, 17), (1100, 33)])
def test_founder_kernels_behind_a_line_aligned_matrix(v2m, ctx, monkeypatch, n_copies, path_words, kernel):
	"""(iii) After v2m_bind_path_matrix_device the context's matrix has a pitch of 32 or 48 words for 17 or 33: edge_major_paths transposes it
	back, line-aligned source, dense destination (3 or 18 words), for both pBWT kernels, whose every output is compared with the plain pBWT."""
	from test_gpu_founder_kernels import Bound, _both_kernels
	monkeypatch.setenv(PANEL, kernel)
	n_edges = 64 * path_words - 5
	b = Bound(v2m, ctx, R.family("dense", n_copies, n_edges, seed=6), device_bind=True)
	_both_kernels(b, n_copies, np.random.default_rng([n_copies, path_words]))


# ---- F. calibration ------------------------------------------------------------------------------------------------------------------------

NOTE = re.compile(r"transpose (\d+)x(\d+) bits: (\S+) \(([^)]*)\)")


def test_calibration_remembers_one_candidate_per_shape(v2m, monkeypatch):
	"""257 x 259 words, 34.1 MB: launch_transpose times every candidate (lines16 with the span rule that depends on the CU count among them),
	remembers one and says so in ctx.info, once per shape; V2M_TRANSPOSE_CANDIDATES replaces the list."""
	SW, DW = T.F_SHAPE
	monkeypatch.delenv("V2M_TRANSPOSE_CANDIDATES", raising=False)
	with v2m.Context(0) as first:
		d = Device(first, SW, DW, want=oracle.transpose_matrix)
		before = NOTE.findall(first.info)
		d.run(monkeypatch, None)
		notes = NOTE.findall(first.info)
		assert len(notes) == len(before) + 1, first.info
		rows, cols, picked, timings = notes[-1]
		assert (int(rows), int(cols)) == (64 * SW, 64 * DW) and picked in T.F_CANDIDATES, first.info
		assert [t.rsplit(" ", 2)[0] for t in timings.split(", ")] == list(T.F_CANDIDATES), first.info
		d.run(monkeypatch, None)                                               # the remembered kernel: right again, nothing timed
		assert NOTE.findall(first.info) == notes, first.info

		monkeypatch.setenv("V2M_TRANSPOSE_CANDIDATES", "lines16;lines8:3")
		with v2m.Context(0) as fresh:
			d2 = Device(fresh, SW, DW, want=lambda *a: d.want)
			d2.run(monkeypatch, None)
			(rows, cols, picked, timings), = NOTE.findall(fresh.info)
			assert (int(rows), int(cols)) == (64 * SW, 64 * DW) and picked in ("lines16", "lines8:3"), fresh.info
			assert [t.rsplit(" ", 2)[0] for t in timings.split(", ")] == ["lines16", "lines8:3"], fresh.info
			del d2
		monkeypatch.delenv("V2M_TRANSPOSE_CANDIDATES")

		inverse = Device(first, DW, SW, want=oracle.transpose_matrix)             # 259 x 257 words: a shape of its own
		inverse.run(monkeypatch, None)
		more = NOTE.findall(first.info)
		assert more[:-1] == notes and (int(more[-1][0]), int(more[-1][1])) == (64 * DW, 64 * SW) and more[-1][2] in T.F_CANDIDATES, first.info


# ---- G. the checked build --------------------------------------------------------------------------------------------------------------------

CHECKED_CORPUS = [
	"tests/test_gpu_transpose_seams.py::test_phase_and_span_seams[5]",
	"tests/test_gpu_transpose_seams.py::test_merged_column_ends",
	"tests/test_gpu_transpose_seams.py::test_pitch_forms_through_the_path_matrix",
]


def test_corpus_on_the_checked_build():
	"""One q of A, all of B and E (i) - (ii) with the slab, the input stage and the context's scratch poisoned before use
	(tests/test_gpu_checked_build.py), both seeds."""
	from test_gpu_checked_build import SEEDS, run_checked_corpus
	from vcf2multialign_amd import build
	assert os.path.exists(build.CHECKED_LIB_PATH) and os.path.exists(build.CHECKED_HOST_LIB_PATH), "build_native() builds them"
	for seed in SEEDS:   # the second seed only once the first has passed
		rc, out = run_checked_corpus(seed, build.CHECKED_LIB_PATH, build.CHECKED_HOST_LIB_PATH, corpus=CHECKED_CORPUS, timeout=600)
		assert rc == 0, "checked build, seed %s: exit %d\n%s" % (seed, rc, out[-6000:])
		assert " passed" in out and "libv2m_hip_checked.so" in out, out[-3000:]
		print(seed, out.strip().splitlines()[-2])
