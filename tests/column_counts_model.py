"""The model of the column counts (include/v2m_hip.h, "column counts"): numpy over the CPU oracle's aligned rows.

matrix(g, rows) stacks the oracle's aligned bodies (oracle.OracleGraph.output_sequence; for a seam graph that is SeamGraph.oracle_body, held
equal to SeamGraph.body by tests/test_column_counts_host.py); counts() applies the header's rule to its bytes; variable() and text() follow.
The hostile-byte graphs are made here from flat arrays (oracle.graph_from_arrays): the oracle carries every byte value, 0x00 and 0x0D included."""

import functools

import numpy as np

import oracle

PLOIDY_MAX = oracle.PLOIDY_MAX
CLASSES = ("A", "C", "G", "T", "N", "gap", "other")


def aligned_row(g, row):
	"""The oracle's aligned row: an int is a chromosome copy (PLOIDY_MAX = REF), a list is (cut node, copy) pairs."""
	body = g.output_sequence(g.ref, cuts=[(int(n), int(c)) for n, c in row]) if isinstance(row, (list, tuple)) else g.output_sequence(g.ref, copy_index=int(row))
	return np.frombuffer(body, dtype=np.uint8)


def matrix(g, rows, window=None):
	"""[len(rows), L] bytes: the rows' aligned bodies (every occurrence of a repeated row), cut to the column window."""
	cache = {}
	def one(row):
		key = tuple(row) if isinstance(row, (list, tuple)) else int(row)
		if key not in cache:
			cache[key] = aligned_row(g, row)
		return cache[key]
	L = g.aligned_length
	m = np.stack([one(r) for r in rows]) if len(rows) else np.zeros((0, L), dtype=np.uint8)
	assert m.shape[1] == L
	return m if window is None else m[:, window[0]:window[1]]


def counts(m):
	"""u32[L, 6]: per column the rows whose byte is A, C, G, T, N (either case: exactly the two ASCII letters) or '-' (exactly)."""
	low = m | 0x20
	return np.stack([(low == ord(c)).sum(axis=0) for c in "acgtn"] + [(m == 0x2D).sum(axis=0)], axis=1).astype(np.uint32)


def other(c, n_rows):
	return n_rows - c.astype(np.int64).sum(axis=1)


def variable(c, n_rows):
	"""bool[L]: none of the seven classes holds all n_rows rows."""
	return np.maximum(c.astype(np.int64).max(axis=1), other(c, n_rows)) != n_rows


def reference_position(g, column):
	"""The 1-based reference position whose byte the REF row holds at `column`, or None where it holds padding."""
	aln, ref = g.aligned_positions.astype(np.int64), g.reference_positions.astype(np.int64)
	n = int(np.searchsorted(aln, column, side="right")) - 1
	k = column - int(aln[n])
	return int(ref[n]) + k + 1 if n + 1 < len(aln) and k < int(ref[n + 1]) - int(ref[n]) else None


def text(g, n_rows, columns, c):
	lines = ["#rows\t%d" % n_rows, "#column\tref_pos\tA\tC\tG\tT\tN\tgap\tother"]
	for col, row in zip([int(x) for x in columns], np.asarray(c).astype(np.int64).tolist()):
		p = reference_position(g, col)
		lines.append("\t".join([str(col), "." if p is None else str(p)] + [str(x) for x in row] + [str(n_rows - sum(row))]))
	return ("\n".join(lines) + "\n").encode()


def expected(g, rows, window=None, variable_only=False):
	"""(columns, counts) as Context.column_counts returns them."""
	c = counts(matrix(g, rows, window))
	cols = np.arange(c.shape[0], dtype=np.uint64) + np.uint64(window[0] if window else 0)
	if variable_only:
		keep = variable(c, len(rows))
		return cols[keep], c[keep]
	return cols, c


def file_text(g, rows, window=None, all_columns=False):
	"""What --output-column-counts writes for `rows`."""
	cols, c = expected(g, rows, window, variable_only=not all_columns)
	return text(g, len(rows), cols, c)


# ---- hostile bytes ------------------------------------------------------------------------------------------------------------------------

HOSTILE_REF = b"A@@AABBA" + b"CGTN-" + bytes([0x40, 0x42, 0x60, 0xC1, 0xE1, 0x00, 0x0D]) + b"acgtn" + b"AGC" + b"TTAN"
HOSTILE_LABELS = [bytes([0xC1]), b"t", bytes([0x00]), b"C\r"]
HOSTILE_COPIES = [[0], [1], [2], [3], [0, 1, 3], [], [0, 2, 3]]


@functools.lru_cache(maxsize=None)
def hostile_graph(shift=0):
	"""32 reference bytes (after `shift` leading 'A's, which move everything to another byte lane) that hold every byte the rule has to
	tell apart: the pairs A@, @A, AB, BA inside one 32-bit word (columns 0-7: a byte next to a matching one that differs from it in
	the low bits, where a borrow-propagating zero-byte test miscounts); C, G, T, N and a literal '-' (8-12); 0x40, 0x42, 0x60, 0xC1, 0xE1,
	0x00, 0x0D (13-19); lower case (20-24).  Then three sites: column 25 'A' under the label 0xC1, column 26 'G' under 't' and under 0x00,
	column 27 'C' with a padding column 28 under the two-byte label 'C' 0x0D -- so column 28 holds 0x0D or '-' and nothing else."""
	s = shift
	reference_positions = [0, 25 + s, 26 + s, 27 + s, 28 + s, 32 + s]
	aligned_positions = [0, 25 + s, 26 + s, 27 + s, 29 + s, 33 + s]
	targets = [2, 3, 3, 4]
	csum = [0, 0, 1, 3, 4, 4, 4]
	label_offsets = np.r_[0, np.cumsum([len(x) for x in HOSTILE_LABELS])]
	bits = np.zeros((64, 64), dtype=bool)
	for c, edges in enumerate(HOSTILE_COPIES):
		bits[c, edges] = True
	words = np.packbits(bits, axis=1, bitorder="little").view("<u8").reshape(-1).copy()
	g = oracle.graph_from_arrays(reference_positions, aligned_positions, targets, csum, label_offsets, b"".join(HOSTILE_LABELS), words, 64, 64, ["S"], [0, len(HOSTILE_COPIES)])
	g.ref = b"A" * s + HOSTILE_REF
	g.name = "hostile_%d" % s
	return g


HOSTILE_ROWS = [PLOIDY_MAX] + list(range(len(HOSTILE_COPIES))) + [[(0, 0), (2, 2), (3, 5)]]
HOSTILE_SHIFTS = (0, 1, 2, 3)


def other_graph():
	"""Every row is "other" in every column: a reference of '@' and 0x00 without edges."""
	g = oracle.graph_from_arrays([0, 21], [0, 21], [], [0, 0, 0], [0], b"", np.zeros(64, dtype=np.uint64), 64, 64, ["S"], [0, 2])
	g.ref = b"@" * 20 + b"\0"
	g.name = "all_other"
	return g


def repeated(rows, n):
	"""n rows that cycle through `rows`."""
	return [rows[i % len(rows)] for i in range(n)]
