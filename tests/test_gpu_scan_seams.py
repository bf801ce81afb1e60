"""The one-workgroup scan kernels that stitch a row's per-tile results together, at their own seams: scan_row_ops_kernel and
scan_row_ops_eqx_kernel (the class of the last non-skipped column and the op count so far), scan_tile_counts_kernel (the bytes so far) and,
on top of it, count_variable_columns_kernel + emit_column_counts_kernel (ranks inside a block of 256 columns).  All of them run 256 threads in
4 waves and walk a row in rounds of 256 items: item i is lane i % 64 of scan wave (i % 256) / 64 of scan block i / 256.

The graphs are row_ops_model.scan_graphs() and their retouched forms of row_ops_eqx_model.scan_graphs(): 513 to 578 tiles with every column
of tiles 63, 64, 255 and 256 a breakpoint, runs of every class across a wave seam (127|128) and a block seam (511|512), and all-padding
stretches that cover a whole scan wave with live waves either side of it in its block, a stretch from lane 0 of a wave to the middle of it,
a whole scan block, and a scan block with the first wave of the next.  tests/test_row_ops_model_host.py and tests/test_row_ops_eqx_host.py
assert without a GPU that the graphs place these (scan_reach()) and hold the op lists that are written down by hand there and here.

  row ops        ops and lengths against the models, the invariants, the split form folded against the unsplit call in both orders; the same
                 rows with V2M_OPS_SLICE_BYTES = 72 (six records a piece) in a child process;
  tile counts    splice_rows aligned and unaligned against the model and the oracle, splice_rows_device into a guarded buffer, whole rows and
                 two column windows a graph: one that begins inside a skipped stretch, one whose own tile 255|256 lies between an empty and a
                 full tile;
  selection      65 836 columns (257 blocks of 256 and 44 columns) with one-byte deletions either side of the wave seams of one block, at
                 columns 65 535 and 65 536 and at both ends; one range, and ranges of 65 536 columns (a range that ends at block 256);
  checked build  all of the above and tests/test_checksum_rows.py with LDS and scratch poisoned, both seeds.

Wall times on an MI355X, graph builds and models included: the module without the checked build 7 s together with
tests/test_checksum_rows.py (the slices' child process 2.2 s, the first test's graphs and context 1.9 s, every other test below 1 s); the
checked build's two runs 19 s together.

What the tests are worth was measured once on three builds with one line of a scan kernel changed (values only): the `if (c)` of
scan_row_ops_kernel's wave loop dropped; block_last of scan_row_ops_eqx_kernel started at 0; wave_last given precedence over wave_carry.
test_row_ops / test_row_ops_split fail on each (the REF row of a block graph comes out as two M ops, the dense row of the wave graph with
an op per tile), while every graph of tests/test_gpu_row_ops.py::test_ops_graphs and tests/test_gpu_row_ops_eqx.py passes on all three.

Not as the list of situations has it:
  * a skipped scan block followed by a COMPLETE scan block: the smallest such row has 768 tiles.  The block after the skipped one holds one
    full tile and a ragged one here, so the scan's last round is a short one.
  * the checked build runs these tests as a corpus of this module's own and not as entries of the row ops modules' corpora, whose time
    stays what it was."""

import os
import subprocess
import sys

import numpy as np
import pytest

import column_counts_model as CM
import row_ops_eqx_model as E
import row_ops_model as M
import seam_graphs as S
from test_gpu_column_counts import check_forms
from test_gpu_row_ops import check_seam as check_plain, same_ops
from test_gpu_row_ops_eqx import check_seam as check_split
from test_gpu_splice_seams import check as check_splice

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
K = S.kernel_constants()
T = K.kTileBytes
PLOIDY_MAX = M.PLOIDY_MAX
GRAPHS = ["scan_waves", "scan_block_0", "scan_block_1"]


@pytest.fixture(scope="module")
def v2m():
	import vcf2multialign_amd as v
	return v


@pytest.fixture(scope="module")
def ctx(v2m):
	c = v2m.Context(0)
	yield c
	c.close()


# ---- row ops -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", range(3), ids=GRAPHS)
def test_row_ops(v2m, ctx, which):
	sg = M.scan_graphs()[which]
	assert sg.name == GRAPHS[which] and len(sg.rows) <= 8
	got = check_plain(v2m, ctx, sg, sg.rows)
	R = int(sg.kept.sum())
	m, i, d = M.OP_M, M.OP_I, M.OP_D
	assert got[0][0].tolist() == [[m, R]]                                         # the REF row is one M op
	if which:
		n_skipped = 256 + 64 * (which - 1)
		assert R == 256 * T + 1 + 8 + T + 300
		for copy in (3, 4, 5):                                                    # M ... a skipped scan block (and a wave) ... M: one op
			assert got[1 + copy][0].tolist() == [[m, R]], copy
		assert got[1][0].tolist() == [[m, 256 * T], [i, n_skipped * T], [m, 1 + 8 + T + 300]]
		assert got[2][0].tolist() == [[m, 256 * T - 6], [d, 11], [m, R - 256 * T - 5]]      # D ... skipped ... D: one op
		assert got[3][0].tolist() == [[m, 256 * T - 6], [d, 6], [m, R - 256 * T]]          # D ... skipped ... M
	else:
		ops = got[1][0]                                                          # copy 0: tiles 63, 64, 255 and 256 give an op a column
		assert len(ops) == 4 * T + 3 and ops[0].tolist() == [m, 63 * T + 1] and ops[1:2 * T, 1].max() == 1
		assert ops[2 * T].tolist() == [m, 185 * T - 100 + 1] and ops[2 * T + 1:4 * T, 1].max() == 1
		assert ops[-2].tolist() == [i, 64 * T]                                   # the insertion over the skipped wave
		for copy in (3, 4, 6):                                                    # M ... a skipped wave ... M, and the stretch from lane 0
			assert got[1 + copy][0].tolist() == [[m, R]], copy


@pytest.mark.parametrize("which", range(3), ids=GRAPHS)
def test_row_ops_split(v2m, ctx, which):
	sg = E.scan_graphs()[which]
	got = check_split(v2m, ctx, sg, sg.rows, split_first=bool(which & 1))
	R = int(sg.kept.sum())
	eq, x, d = E.OP_EQ, E.OP_X, E.OP_D
	assert got[0][0].tolist() == [[eq, R]]
	if which:
		assert got[4][0].tolist() == [[eq, 256 * T - 1], [x, 2], [eq, T + 308]]             # X ... a skipped scan block (and a wave) ... X: one X op of length 2
		assert got[5][0].tolist() == [[eq, 256 * T], [x, 1], [eq, T + 308]]                 # = ... skipped ... X
		assert got[6][0].tolist() == [[eq, 256 * T - 1], [x, 1], [eq, T + 309]]             # X ... skipped ... =
		assert got[2][0].tolist() == [[eq, 256 * T - 6], [d, 11], [eq, R - 256 * T - 5]]
	else:
		assert len(got[1][0]) > 65535 and got[1][0][:5, 0].tolist() == [eq, E.OP_I, x, E.OP_I, eq]
		assert got[4][0][:, 0].tolist() == [eq, x, eq] and got[4][0][1, 1] == 2             # X ... a skipped wave ... X
		assert got[5][0][:, 0].tolist() == [eq, x, eq] and got[5][0][1, 1] == 1
		assert got[7][0].tolist()[1:] == [[x, 2], [eq, int(got[7][0][2, 1])], [x, 40], [eq, 700]]   # X ... skipped from lane 0 ... X; the X run across 511|512


SLICE_CHILD = r"""
import os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import numpy as np
import row_ops_model as M
import row_ops_eqx_model as E
import vcf2multialign_amd as v2m
out = {}
with v2m.Context(0) as ctx:
	for which in (0, 2):
		for split, sg in ((False, M.scan_graphs()[which]), (True, E.scan_graphs()[which])):
			ctx.upload_graph(v2m.VariantGraph.from_object(sg.g), sg.g.ref)
			for i, (ops, length) in enumerate(ctx.row_ops(sg.rows, split_match=split)):
				out["%%s_%%d_ops" %% (sg.name, i)] = ops
				out["%%s_%%d_length" %% (sg.name, i)] = np.array([length])
np.savez(%(path)r, **out)
"""


def test_several_slices_give_the_one_slice_result(v2m, ctx, tmp_path):
	"""V2M_OPS_SLICE_BYTES = 72 (six records): the rows of the wave graph and of the longer block graph, counted once, are emitted in pieces
	that begin at a row that is not the slice's first, from per-row tables of 513 and 578 entries."""
	path = str(tmp_path / "sliced.npz")
	env = dict(os.environ, V2M_OPS_SLICE_BYTES="72")
	r = subprocess.run([sys.executable, "-c", SLICE_CHILD % {"root": ROOT, "path": path}], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300, env=env)
	assert r.returncode == 0, r.stdout.decode(errors="replace")[-4000:]
	sliced = np.load(path)
	for which in (0, 2):
		for split, sg in ((False, M.scan_graphs()[which]), (True, E.scan_graphs()[which])):
			ctx.upload_graph(v2m.VariantGraph.from_object(sg.g), sg.g.ref)
			whole = ctx.row_ops(sg.rows, split_match=split)
			counts = [len(ops) for ops, _ in whole]
			assert sum(counts) > 12 and any(a + b <= 6 for a, b in zip(counts, counts[1:]))          # several pieces, one of them of two rows or more
			got = [(sliced["%s_%d_ops" % (sg.name, i)], int(sliced["%s_%d_length" % (sg.name, i)][0])) for i in range(len(sg.rows))]
			same_ops(got, whole, sg.name + " in slices")


# ---- tile counts: the unaligned splice and its window form ---------------------------------------------------------------------------------

@pytest.mark.parametrize("which", range(3), ids=GRAPHS)
def test_splice(v2m, ctx, which):
	"""scan_tile_counts_kernel under the unaligned splice: tiles of 0 and of 16 384 surviving bytes either side of the scan's wave and block
	seams.  Whole rows through splice_rows and splice_rows_device (the lengths are the model's, nothing is written past a row's bytes), then
	the graph's two windows, in which the scan's tile 0 is not the row's."""
	sg = M.scan_graphs()[which]
	check_splice(v2m, ctx, sg, sg.rows, device=True)
	windows = sg.notes["windows"]
	b, e = windows[1][1:]
	census = S.RowCensus(sg, PLOIDY_MAX, S.TileTables(sg, (b, e)))
	assert (0, T) == (int(census.tile_bytes[255]), int(census.tile_bytes[256])), "the second window's tile 255 is empty and its tile 256 full"
	assert 0 == S.RowCensus(sg, PLOIDY_MAX, S.TileTables(sg, windows[0][1:])).tile_bytes[:20].sum()
	check_splice(v2m, ctx, sg, sg.rows, windows=windows, device=0 == which, upload=False)


# ---- the column selection ------------------------------------------------------------------------------------------------------------------

SELECT_BLOCK = 3            # the select block whose wave seams hold sites
SELECT_SITES = [0] + [256 * SELECT_BLOCK + c for c in (63, 64, 127, 128, 191, 192)] + [256 * 256 - 1, 256 * 256, 256 * 256 + 299]


def selection_graph():
	"""256 x 256 + 300 columns with a one-byte deletion at the first and the last column, either side of the three wave seams of one block of
	256 columns, and at column 255 of block 255 and column 0 of block 256: the scan over the blocks' counts crosses its round of 256 there."""
	b = S.Builder(7700)
	for s in SELECT_SITES:
		if s > b.length:
			b.ref_to(s)
		b.add_site([0], 1)
	assert b.length == 256 * 256 + 300
	return b.finish([list(range(b.n_edges)), []], "selection_wide")


@pytest.mark.parametrize("range_columns", [None, 256 * 256], ids=["one_range", "range_ends_at_block_256"])
def test_selection(v2m, ctx, monkeypatch, range_columns):
	if range_columns:
		monkeypatch.setenv("V2M_COLUMN_COUNTS_BLOCK_BYTES", str(32 * range_columns))
	sg = selection_graph()
	ctx.upload_graph(v2m.VariantGraph.from_object(sg.g), sg.g.ref)
	rows = sg.rows
	want = check_forms(ctx, sg.g, rows, what=sg.name)
	assert np.flatnonzero(CM.variable(want, len(rows))).tolist() == SELECT_SITES
	assert SELECT_SITES == [0, 831, 832, 895, 896, 959, 960, 65535, 65536, 65835]
	cols, counts = ctx.column_counts(rows, variable_only=True)
	assert cols.tolist() == SELECT_SITES and counts[:, 5].tolist() == [1] * len(SELECT_SITES)      # one row of three holds a gap there
	assert ctx.column_count_blocks == ([8, 2] if range_columns else [10])
	ctx.column_counts(rows)
	assert ctx.column_count_blocks == ([256 * 256, 300] if range_columns else [256 * 256 + 300])


# ---- the checked build ---------------------------------------------------------------------------------------------------------------------

CHECKED_CORPUS = [
	"tests/test_gpu_scan_seams.py::test_row_ops",
	"tests/test_gpu_scan_seams.py::test_row_ops_split",
	"tests/test_gpu_scan_seams.py::test_several_slices_give_the_one_slice_result",          # its child inherits the checked libraries
	"tests/test_gpu_scan_seams.py::test_splice",
	"tests/test_gpu_scan_seams.py::test_selection",
	"tests/test_checksum_rows.py::test_device_is_the_model",
	"tests/test_checksum_rows.py::test_device_many_rows",
	"tests/test_checksum_rows.py::test_device_twice_on_one_context",
]


def test_corpus_on_the_checked_build():
	"""The list above with every LDS object, scratch buffer and staging area poisoned before use (tests/test_gpu_checked_build.py), one run per
	seed: wave_last, wave_sums and carry_s are LDS, and the skipped-wave path is where a read of an entry nobody wrote this round would hide in
	the product build.  A corpus of its own: the row ops modules' corpora keep their time."""
	from test_gpu_checked_build import SEEDS, run_checked_corpus
	from vcf2multialign_amd import build
	assert os.path.exists(build.CHECKED_LIB_PATH) and os.path.exists(build.CHECKED_HOST_LIB_PATH), "build_native() builds them"
	for seed in SEEDS:   # the second seed only once the first has passed
		rc, out = run_checked_corpus(seed, build.CHECKED_LIB_PATH, build.CHECKED_HOST_LIB_PATH, corpus=CHECKED_CORPUS, timeout=600)
		assert rc == 0, "checked build, seed %s: exit %d\n%s" % (seed, rc, out[-6000:])
		assert " passed" in out and "libv2m_hip_checked.so" in out, out[-3000:]
		print(seed, out.strip().splitlines()[-2])
