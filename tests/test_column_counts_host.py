"""Column counts without a GPU: the host library's column_counts_text against the model's text (tests/column_counts_model.py), the header's
constants, and assertions that the corpus of tests/test_gpu_column_counts.py really holds the bytes and columns it is there for."""

import os
import re

import numpy as np

import column_counts_model as CM
import row_ops_model as M
import seam_graphs as S

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _header():
	with open(os.path.join(ROOT, "include", "v2m_hip.h")) as f:
		return f.read()


def _host_text(g, n_rows, columns, counts):
	from vcf2multialign_amd import host
	return host.column_counts_text(n_rows, columns, counts, g.reference_positions, g.aligned_positions)


# ---- the text ------------------------------------------------------------------------------------------------------------------------------

def test_text_of_the_hostile_graph():
	"""Both header lines, `.` in the padding column, the position of a literal '-' of the reference, the first and the last column."""
	g = CM.hostile_graph(0)
	rows = CM.HOSTILE_ROWS
	cols, c = CM.expected(g, rows)
	text = _host_text(g, len(rows), cols, c)
	assert text == CM.text(g, len(rows), cols, c)
	lines = text.decode().split("\n")
	assert lines[0] == "#rows\t9" and lines[1] == "#column\tref_pos\tA\tC\tG\tT\tN\tgap\tother" and lines[-1] == ""
	assert lines[2] == "0\t1\t9\t0\t0\t0\t0\t0\t0"                 # the first column
	assert lines[2 + 12] == "12\t13\t0\t0\t0\t0\t0\t9\t0"          # a literal '-' of the reference has a position
	assert lines[2 + 28] == "28\t.\t0\t0\t0\t0\t0\t6\t3"           # the REF row's padding has none
	assert lines[2 + 32] == "32\t32\t0\t0\t0\t0\t9\t0\t0"          # the last column
	assert len(lines) == 2 + 33 + 1
	# the variable columns alone, and no record at all
	vcols, vc = CM.expected(g, rows, variable_only=True)
	assert vcols.tolist() == [25, 26, 28]
	assert _host_text(g, len(rows), vcols, vc) == CM.text(g, len(rows), vcols, vc) == CM.file_text(g, rows)
	assert _host_text(g, 3, [], np.zeros((0, 6), np.uint32)) == b"#rows\t3\n#column\tref_pos\tA\tC\tG\tT\tN\tgap\tother\n"


def test_text_of_graphs_with_padding_runs():
	"""Every column of the dash graph (literal '-' in the reference and in labels, padding columns) and of a seam graph; records in
	descending order too (the formatter looks a record up afresh when it does not ascend)."""
	import vcf2multialign_amd as v2m
	g = M.dash_graph()
	rows = [CM.PLOIDY_MAX, 0, 1, 2, 3, 4]
	cols, c = CM.expected(g, rows)
	assert _host_text(g, len(rows), cols, c) == CM.text(g, len(rows), cols, c)
	assert b"\n5\t.\t" in CM.text(g, len(rows), cols, c) and b"\n8\t6\t" in CM.text(g, len(rows), cols, c)
	assert _host_text(g, len(rows), cols[::-1], c[::-1]) == CM.text(g, len(rows), cols[::-1], c[::-1])
	vg = v2m.VariantGraph.from_object(g)
	assert [vg.reference_position_of_column(i) for i in range(g.aligned_length)] == [CM.reference_position(g, i) for i in range(g.aligned_length)]
	assert vg.reference_position_of_column(g.aligned_length) is None
	sg = M.boundary_graph()
	pick = np.r_[0:40, sg.length - 40:sg.length].astype(np.uint64)
	c = CM.counts(CM.matrix(sg.g, sg.rows))[pick.astype(np.int64)]
	assert _host_text(sg.g, len(sg.rows), pick, c) == CM.text(sg.g, len(sg.rows), pick, c)
	vg = v2m.VariantGraph.from_object(sg.g)
	for col in pick.tolist():
		p = vg.reference_position_of_column(col)
		assert p == CM.reference_position(sg.g, col) and (p is not None) == bool(sg.kept[col])
		if p is not None:
			assert sg.g.ref[p - 1] == sg.ref_row[col]


def test_the_model_rows_are_the_seam_graphs_rows():
	"""SeamGraph.oracle_body, which the model reads, equals SeamGraph.body."""
	for sg in (M.boundary_graph(), S.geometry_graph(4097)):
		for r in sg.rows:
			assert sg.oracle_body(r) == sg.body(r) == CM.aligned_row(sg.g, r).tobytes()


# ---- the header ----------------------------------------------------------------------------------------------------------------------------

def test_header_constants():
	from vcf2multialign_amd import _native as N
	header = _header()
	assert "#define V2M_COUNT_CLASSES 6" in header and N.COUNT_CLASSES == 6
	assert re.search(r"#define V2M_COUNTS_VARIABLE_ONLY\s+0x8u", header) and N.COUNTS_VARIABLE_ONLY == 0x8
	assert re.search(r"#define V2M_COUNTS_ACCUMULATE\s+0x10u", header) and N.COUNTS_ACCUMULATE == 0x10
	assert "V2M_KERNEL_END = 15" in header and "V2M_KERNEL_COLUMN_COUNTS = 15" in header and "V2M_KERNEL_COLUMN_SELECT = 16" in header and "V2M_KERNEL_LIMIT = 17" in header
	assert (N.KERNEL_COLUMN_COUNTS, N.KERNEL_COLUMN_SELECT, N.KERNEL_LIMIT) == (15, 16, 17)
	assert "#define V2M_ABI_VERSION 5" in header and "V2M_COLUMN_COUNTS_BLOCK_BYTES" in header
	assert np.dtype(N.COLUMN_COUNT_DTYPE).itemsize == 32
	for name in ("v2m_column_counts", "v2m_column_counts_device"):
		assert re.search(r"\bint %s\(" % name, header) and name in N.SIGNATURES


def test_python_constants_are_the_sources():
	from vcf2multialign_amd import _native as N
	with open(S.KERNELS_HPP) as f:
		kernels = f.read()
	with open(os.path.join(ROOT, "vcf2multialign_amd", "csrc", "v2m_hip.hip")) as f:
		library = f.read()
	assert re.search(r"constexpr int kCountThreads = 256;", kernels) and re.search(r"constexpr u32 kCountColumns = kCountThreads \* 16;", kernels) and N.COUNT_COLUMNS == 4096
	assert re.search(r"constexpr u32 kCountRun = %d;" % N.COUNT_RUN, kernels) and N.COUNT_RUN == 255
	assert re.search(r"constexpr int kSelectColumns = %d;" % N.SELECT_COLUMNS, kernels)
	assert re.search(r"constexpr u64 kColumnCountsMinRows = %d;" % N.COLUMN_COUNTS_MIN_ROWS, library)


# ---- reach: what the GPU corpus holds ------------------------------------------------------------------------------------------------------

def test_hostile_graphs_hold_what_they_are_for():
	g = CM.hostile_graph(0)
	rows = CM.HOSTILE_ROWS
	m = CM.matrix(g, rows)
	n = len(rows)
	c = CM.counts(m).astype(np.int64)
	oth = CM.other(CM.counts(m), n)
	# a column whose only non-gap byte is 0x0D
	col = [i for i in range(m.shape[1]) if set(m[:, i].tolist()) == {0x0D, 0x2D}]
	assert col == [28] and c[28].tolist() == [0, 0, 0, 0, 0, 6] and oth[28] == 3
	present = set(m.reshape(-1).tolist())
	assert {0xC1, 0xE1, 0x40, 0x42, 0x60, 0x00, 0x0D} <= present
	# neither 0xC1 / 0xE1 nor 0x40 / 0x42 / 0x60 is counted as a letter, 0x0D is no gap
	for i in range(m.shape[1]):
		if set(m[:, i].tolist()) <= {0xC1, 0xE1, 0x40, 0x42, 0x60, 0x00, 0x0D}:
			assert c[i].sum() == 0 and oth[i] == n
	# the pairs inside one 32-bit word of a row
	ref_row = m[0].tobytes()
	for pair in (b"A@", b"@A", b"AB", b"BA"):
		at = [i for i in range(len(ref_row) - 1) if ref_row[i:i + 2] == pair and i // 4 == (i + 1) // 4]
		assert at, pair
	# each of the seven classes holds all rows of some column
	for k in range(6):
		assert (c[:, k] == n).any(), CM.CLASSES[k]
	assert (oth == n).any()
	# a column split between "other" and one class, and nothing else
	assert any(oth[i] and (c[i] > 0).sum() == 1 and oth[i] + c[i].max() == n for i in range(m.shape[1]))
	assert CM.variable(CM.counts(m), n).sum() == 3
	# the shifted graphs hold the same columns one, two and three byte lanes on
	for s in CM.HOSTILE_SHIFTS[1:]:
		ms = CM.matrix(CM.hostile_graph(s), rows)
		assert np.array_equal(ms[:, s:], m) and (ms[:, :s] == ord("A")).all()
	# all-other: not variable
	go = CM.other_graph()
	mo = CM.matrix(go, [CM.PLOIDY_MAX, 0, 1])
	assert CM.counts(mo).sum() == 0 and not CM.variable(CM.counts(mo), 3).any()
