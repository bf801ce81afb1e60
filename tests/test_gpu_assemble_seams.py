"""Founder rows at every segment and word seam: assemble_row_bits_kernel, and resolve_effective_edges_kernel, resolve_queued_words_kernel and
resolve_rows_serial_kernel where they read a row from the assembled bit column instead of from one chromosome copy.

The rows are hand-made cuts on two graphs of tests/seam_graphs.py.  assemble_graph(tail) is a chain of one-edge, one-column sites in
which no edge overlaps another: every assembled bit is one visible column.  resolve_graph(tail) has the overlapping edges: there the
assembled row is what resolve decides from.  Every case is compared byte for byte with the model's assembled column (a plain loop over
the edges) and with the oracle's output_sequence(cuts=...), aligned and unaligned, through splice_rows; the whole-row cases also through
splice_rows_device into a guard-filled buffer.  That the cuts put the named values in front of the kernel -- and that at every cut the
copies either side differ in the bit before it and the bit after it, without which a wrong mask shows nowhere -- is what
tests/test_seam_graphs_host.py asserts (SegmentCensus), without a GPU.

Classes (the issue's letters):  a  cuts either side of a word's first and last edge, at the words beside wave span and workgroup edges
(from in {0, 1, 63}, to in {1, 63, 64}, one-bit segments);  b  segments of one word, one wave span, 65 words across a span edge, across
the workgroup edge, longer than a workgroup;  c  64, 65, 66, 129 and 130 segments for one wave's lane loop, 64 lanes into one LDS word;
d  REF segments: before a late first cut, one bit, one word, up to a span edge, last;  e  a last segment of the last edge alone, and
one that begins past every edge, for n_edges % 64 in {0, 1, 63};  f  empty segments (two cuts, one first edge) at an ordinary edge, a
span's and a workgroup's first edge;  g  batches: alone, between plain and REF rows, twice, kGroupRowsLds + 1 rows;  h  column windows
whose first edge word is 1, 63, 64, 65, 257, with cuts laid against the shifted wave spans, a window no edge reaches, a window set.
v2m_row_ops on the rows of a, c, d and f: on this graph's twin with empty labels, where every set bit is a D of one byte (one-byte
substitutions leave the ops one M run whatever the bits), and on the cut rows of resolve_graph.
Resolve on assembled rows: the blocker / blocked pairs and the deletion of resolve_graph with the copies switching around them, as it is,
with the serial kernel, with the queue at 0 and 1 entries per shard, and under windows (one in which a word is assembled that is not
resolved).  All of it again on the checked build, where the assembled column's scratch and the kernel's LDS are poisoned.

Left out, by name:
  * the `<=` of the kernel's binary search: with `<` the walk begins at an earlier segment, and a segment that ends at or before the
    span's first edge is clipped to nothing, so the words are the same; only the number of segments walked differs.  Segments that begin
    exactly on a span's first edge (one, and two with an empty one) are placed all the same.
  * a row of two segments each longer than a workgroup's 256 words: the graph has 323 words; the row placed has one segment of 260
    words and one of the rest (every wave of the first workgroup sees a single segment, the first wave of the second sees both).
  * more than two cuts with one first edge: the nodes that share a first edge are an edge's target and the next site's own node, two."""

import os

import pytest

import row_ops_model as M
import seam_graphs as S
from test_gpu_splice_seams import _expected, _same, check

pytestmark = pytest.mark.gpu

K = S.kernel_constants()
R = S.PLOIDY_MAX
TAILS = (0, 1, 63)


@pytest.fixture(scope="module")
def v2m():
	import vcf2multialign_amd as v
	return v


@pytest.fixture(scope="module")
def ctx(v2m):
	c = v2m.Context(0)
	yield c
	c.close()


# ---- a - f: whole rows ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tail", TAILS)
def test_segment_and_word_seams(v2m, ctx, tail):
	"""Every row of classes a - f in one batch, through splice_rows and splice_rows_device."""
	sg = S.assemble_graph(tail)
	rows = list(S.assemble_rows(tail).values())
	check(v2m, ctx, sg, rows, device=True)


# ---- g: batches ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("tail", TAILS)
def test_batches(v2m, ctx, tail):
	"""A cut row alone; cut rows between plain and REF rows (the workgroups of those rows leave at once, and a cut row's words lie at
	row x the words' stride whatever the rows before it were); the same cut row twice; kGroupRowsLds + 1 rows."""
	sg = S.assemble_graph(tail)
	by_name = S.assemble_rows(tail)
	cut = list(by_name.values())
	for name in ("a_word_edges_45", "c_129", "f_empty_45", "e_past_every_edge_45"):
		check(v2m, ctx, sg, [by_name[name]], upload="a_word_edges_45" == name)
	check(v2m, ctx, sg, [0, by_name["a_word_edges_01"], R, by_name["c_129"], 3, R, by_name["f_empty_10"], 5, by_name["d_ref"], 1], upload=False)
	check(v2m, ctx, sg, [by_name["c_65_45"], by_name["c_65_45"]], upload=False)
	many = [(R, 4, 2)[i % 3] if i % 2 else cut[(i // 2) % len(cut)] for i in range(K.kGroupRowsLds + 1)]
	assert len(many) == K.kGroupRowsLds + 1 and isinstance(many[0], list) and isinstance(many[-1], list)
	check(v2m, ctx, sg, many, upload=False)


# ---- h: column windows ---------------------------------------------------------------------------------------------------------------------

def _window_rows(rows):
	cut = list(rows.values())
	return [R, cut[0], 4, cut[1], cut[0]]


@pytest.mark.parametrize("tail", TAILS)
def test_column_windows(v2m, ctx, tail):
	"""v2m_set_column_window with the window's first edge word at 1, 63, 64, 65 and 257: the wave spans begin at that word, and the cuts lie
	on the shifted spans' first edges, an edge before and after, with 65 one-edge segments under the second span; and a window that no
	edge reaches, in which rows with cuts are the REF row's columns."""
	sg = S.assemble_graph(tail)
	ctx.upload_graph(v2m.VariantGraph.from_object(sg.g), sg.g.ref)
	for name, b, e, rows in S.assemble_windows(tail):
		check(v2m, ctx, sg, _window_rows(rows), windows=[(name, b, e)], device=name in ("lo_63", "no_edge"), upload=False)


@pytest.mark.parametrize("tail", [0, 63])
def test_window_set(v2m, ctx, tail):
	"""Three of the windows as one window set: the words put together run from the first window's first edge word to the last one's end."""
	sg = S.assemble_graph(tail)
	ctx.upload_graph(v2m.VariantGraph.from_object(sg.g), sg.g.ref)
	chosen = [w for w in S.assemble_windows(tail) if w[0] in ("lo_257", "lo_1", "lo_64")]
	assert 3 == len(chosen)
	windows = [(b, e) for _, b, e, _ in chosen]
	rows = [R] + [row for w in chosen for row in w[3].values()] + [5]
	ctx.set_window_set(windows)
	for unaligned in (False, True):
		want = [_expected(sg, rows, unaligned, w) for w in windows]
		got = ctx.splice_window_set(rows, unaligned=unaligned)
		assert len(got) == len(rows)
		for i, pieces in enumerate(got):
			assert len(pieces) == len(windows)
			for k, piece in enumerate(pieces):
				_same(piece, want[k][i], "%s window set, window %d [%d, %d) unaligned=%s row %d" % ((sg.name, k) + windows[k] + (unaligned, i)))


# ---- row ops -------------------------------------------------------------------------------------------------------------------------------

def _same_row_ops(ctx, sg, rows):
	from test_gpu_row_ops import same_ops
	got = ctx.row_ops(rows)
	same_ops(got, [M.seam_ops(sg, r) for r in rows], sg.name)
	for r, (ops, length) in zip(rows, got):
		M.check_invariants(ops, int(sg.kept.sum()), length, is_ref_row=not isinstance(r, list) and r == R)
	return got


@pytest.mark.parametrize("tail", TAILS)
def test_row_ops(v2m, ctx, tail):
	"""v2m_row_ops resolves the rows itself (always whole rows): the rows of classes a, c, d and f give the model's ops.  On the graph of
	substitutions every row is one M run; on its twin with empty labels every set bit is a D of one byte, so the ops spell the
	assembled column out."""
	rows = [row for name, row in S.assemble_rows(tail).items() if name[0] in "acdf"] + [R, 4]
	for sg in (S.assemble_graph(tail), S.assemble_graph(tail, 0)):
		ctx.upload_graph(v2m.VariantGraph.from_object(sg.g), sg.g.ref)
		got = _same_row_ops(ctx, sg, rows)
		assert all(len(ops) == 1 for ops, _ in got) == (sg is S.assemble_graph(tail))


@pytest.mark.parametrize("tail", [0, 63])
def test_row_ops_on_resolved_rows(v2m, ctx, tail):
	"""The same through resolve: the cut rows of resolve_graph, whose labels of two bytes are I runs and whose stretched edges D runs."""
	sg = S.resolve_graph(tail)
	ctx.upload_graph(v2m.VariantGraph.from_object(sg.g), sg.g.ref)
	_same_row_ops(ctx, sg, _resolve_rows(tail))


# ---- resolve on assembled rows ---------------------------------------------------------------------------------------------------------------

RESOLVE_KNOBS = {
	"as_it_is": {},
	"serial": {"V2M_MAX_BACK_WORDS": str(S.RESOLVE_BACK_WORDS)},      # the edge bw + 1 words under the deletion sends its row to resolve_rows_serial_kernel
	"queue_0": {"V2M_RESOLVE_QUEUE_CAPACITY": "0"},                    # every hard word is decided in the streaming pass, walking back over the assembled row
	"queue_1": {"V2M_RESOLVE_QUEUE_CAPACITY": "1"},                    # one word per shard in the queued pass, the rest in the streaming pass
}


def _resolve_rows(tail):
	cut = list(S.resolve_cut_rows(tail).values())
	return cut[:2] + [0, R] + cut[2:] + [2]


@pytest.mark.parametrize("knobs", sorted(RESOLVE_KNOBS))
@pytest.mark.parametrize("tail", TAILS)
def test_resolve_reads_the_assembled_row(v2m, ctx, monkeypatch, tail, knobs):
	"""Rows that switch copy at the source node of every blocker and right after its blocked edge, at the deletion's source node and at the
	first bridge after its end: what resolve decides depends on bits of two copies, and on none of the first segment's."""
	for name, value in RESOLVE_KNOBS[knobs].items():
		monkeypatch.setenv(name, value)
	sg = S.resolve_graph(tail)
	check(v2m, ctx, sg, _resolve_rows(tail))


@pytest.mark.parametrize("knobs", ["as_it_is", "queue_0"])
@pytest.mark.parametrize("tail", [0, 63])
def test_resolve_reads_the_assembled_row_under_windows(v2m, ctx, monkeypatch, tail, knobs):
	"""A window that begins under the deletion, and one whose first resolved word begins with an overlappable edge: the words put together
	begin a word earlier than the words resolved."""
	for name, value in RESOLVE_KNOBS[knobs].items():
		monkeypatch.setenv(name, value)
	sg = S.resolve_graph(tail)
	check(v2m, ctx, sg, _resolve_rows(tail), windows=S.resolve_cut_windows(tail))


# ---- the checked build ------------------------------------------------------------------------------------------------------------------------

CHECKED_CORPUS = [
	"tests/test_gpu_assemble_seams.py::test_segment_and_word_seams",
	"tests/test_gpu_assemble_seams.py::test_batches",
	"tests/test_gpu_assemble_seams.py::test_column_windows",
	"tests/test_gpu_assemble_seams.py::test_window_set",
	"tests/test_gpu_assemble_seams.py::test_row_ops",
	"tests/test_gpu_assemble_seams.py::test_row_ops_on_resolved_rows",
	"tests/test_gpu_assemble_seams.py::test_resolve_reads_the_assembled_row",
	"tests/test_gpu_assemble_seams.py::test_resolve_reads_the_assembled_row_under_windows",
]


def test_corpus_on_the_checked_build():
	"""The list above with every LDS object, scratch buffer and staging area poisoned before use (tests/test_gpu_checked_build.py), one run per seed."""
	from test_gpu_checked_build import SEEDS, run_checked_corpus
	from vcf2multialign_amd import build
	assert os.path.exists(build.CHECKED_LIB_PATH) and os.path.exists(build.CHECKED_HOST_LIB_PATH), "build_native() builds them"
	for seed in SEEDS:   # the second seed only once the first has passed
		rc, out = run_checked_corpus(seed, build.CHECKED_LIB_PATH, build.CHECKED_HOST_LIB_PATH, corpus=CHECKED_CORPUS, timeout=600)
		assert rc == 0, "checked build, seed %s: exit %d\n%s" % (seed, rc, out[-6000:])
		assert " passed" in out and "libv2m_hip_checked.so" in out, out[-3000:]
		print(seed, out.strip().splitlines()[-2])
