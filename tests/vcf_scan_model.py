"""A model of the VCF scan rule, written from the "VCF scan" section of include/v2m_hip.h alone (test infrastructure): what v2m_vcf_scan
and scan_lines_host must say of a text, line by line, and what the header promises of any chunking of it.  Plain Python over
bytes.split, startswith and integer sets: no tab positions, no steps, nothing shared with the package but the dtype of a record.

The model also names why a line is declined (`reason`), which the rule does not ask of a scanner; the seam census uses it.

Where the header was silent it has been amended, not the model bent to the code:
  - "column_begin = the columns of the chunk's lines before it" holds for words_per_column == 0 too (a layout that excludes every copy):
    the columns then have no words, but they are still counted, and n_columns is their number."""

import numpy as np

REASONS = ("tabs<7", "a", "b", "c", "d", "e:missing", "e:empty", "e:long", "e:nondigit", "e:value")
DIGITS = frozenset(b"0123456789")


def split_lines(text):
	"""Lines: the bytes between '\\n's; a last line without '\\n' counts, a trailing '\\n' adds no empty line."""
	lines = bytes(text).split(b"\n")
	if lines[-1] == b"":
		lines.pop()
	return lines


def first_column(line):
	"""Column 1 for the layout test: up to the first tab; without a tab the whole line less a final '\\r'."""
	if b"\t" in line:
		return line.split(b"\t")[0]
	return line[:-1] if line.endswith(b"\r") else line


def is_kind_0(line):
	return line == b"" or line.startswith(b"#")


def token_reason(token, n_alts):
	"""None when the token is "." or 1 - 3 decimal digits of value <= n_alts; else why not."""
	if token == b".":
		return None
	if token == b"":
		return "e:empty"
	if not set(token) <= DIGITS:
		return "e:nondigit"
	if len(token) > 3:
		return "e:long"
	return None if int(token) <= n_alts else "e:value"


def classify(line, wanted, layout):
	"""(kind, n_alts, head, columns, reason); reason is None unless the kind is 3.  layout is None before the layout line."""
	words = int(layout["words_per_column"]) if layout is not None else 0
	none = np.zeros((0, words), np.uint64)
	if is_kind_0(line):
		return 0, 0, (line if line.startswith(b"#CHROM") else b""), none, None
	fields = line.split(b"\t")
	n_tabs = len(fields) - 1
	if n_tabs < 7:
		return 3, 0, line, none, "tabs<7"
	if fields[0] != wanted:
		return 1, 0, b"", none, None
	assert layout is not None, "a line on the wanted chromosome with 7 tabs or more is the layout line or comes after it"

	def declined(reason):
		return 3, 0, line, none, reason

	if line.endswith(b"\r"):
		return declined("a")
	if n_tabs < 9 or not (fields[8] == b"GT" or fields[8].startswith(b"GT:")):
		return declined("b")
	n_alts = len(fields[4].split(b","))
	if not 1 <= n_alts <= 8:
		return declined("c")
	n_samples = int(layout["n_samples"])
	if n_tabs != 8 + n_samples:
		return declined("d")
	copy_begin, row_lookup = layout["copy_begin"], layout["row_lookup"]
	columns = np.zeros((n_alts, words), np.uint64)
	for s in range(n_samples):
		tokens = fields[9 + s].split(b":")[0].replace(b"/", b"|").split(b"|")
		for c in range(int(copy_begin[s + 1]) - int(copy_begin[s])):
			if c >= len(tokens):
				return declined("e:missing")
			why = token_reason(tokens[c], n_alts)
			if why is not None:
				return declined(why)
			allele = 0 if tokens[c] == b"." else int(tokens[c])
			row = int(row_lookup[int(copy_begin[s]) + c])
			if allele >= 1 and row >= 0:
				columns[allele - 1, row >> 6] |= np.uint64(1 << (row & 63))
	return 2, n_alts, b"\t".join(fields[:9]), columns, None


def scan_line(line, wanted, layout):
	"""(kind, n_alts, head, columns); columns: [n_alts, words_per_column] uint64."""
	return classify(line, wanted, layout)[:4]


def layout_line_of(lines, wanted):
	"""The first line that is not of kind 0 and whose column 1 is the wanted name, or None."""
	for i, line in enumerate(lines):
		if not is_kind_0(line) and first_column(line) == wanted:
			return i
	return None


def scan_text(text, wanted, layout_fn, with_reasons=False):
	"""([(kind, n_alts, head, columns)] per line, the layout line's index or None).  layout_fn(line index, line) gives the layout (a dict
	of the header's fields); it is called once, for the layout line, or never.  with_reasons: a third result, the reasons per line."""
	wanted = wanted.encode() if isinstance(wanted, str) else bytes(wanted)
	lines = split_lines(text) if len(text) else []
	at = layout_line_of(lines, wanted)
	layout = layout_fn(at, lines[at]) if at is not None else None
	full = [classify(line, wanted, layout if at is not None and i >= at else None) for i, line in enumerate(lines)]
	out = [f[:4] for f in full]
	return (out, at, [f[4] for f in full]) if with_reasons else (out, at)


def check_chunks(chunks, model_lines, layout_line, what=""):
	"""What the header promises of any chunking, and per line the model's record, head and columns."""
	at = 0
	for c in chunks:
		n = len(c["lines"])
		assert n > 0, (what, "an empty chunk", at)
		assert int(c["first_line"]) == at, (what, "first_line", int(c["first_line"]), at)
		before = layout_line is None or at + n <= layout_line
		assert before or at >= layout_line, (what, "a chunk straddles the layout line", at, n, layout_line)
		words = int(c["words_per_column"])
		heads, columns, head_at, column_at = c["heads"], c["columns"], 0, 0
		if before:
			assert words == 0, (what, "words_per_column before the layout line", at, words)
		assert columns.ndim == 2 and columns.shape[1] == words, (what, at, columns.shape, words)
		for k in range(n):
			l = c["lines"][k]
			kind, n_alts, head, cols = model_lines[at + k]
			where = (what, "line", at + k)
			assert (int(l["kind"]), int(l["n_alts"])) == (kind, n_alts), (where, int(l["kind"]), int(l["n_alts"]), kind, n_alts)
			assert int(l["head_offset"]) == head_at and int(l["head_length"]) == len(head), (where, int(l["head_offset"]), int(l["head_length"]), head_at, len(head))
			assert heads[head_at:head_at + len(head)] == head, (where, heads[head_at:head_at + len(head)], head)
			assert int(l["column_begin"]) == column_at, (where, int(l["column_begin"]), column_at)
			if n_alts:
				assert cols.shape[1] == words, (where, cols.shape, words)
				if words:
					assert columns[column_at:column_at + n_alts].tobytes() == cols.tobytes(), (where, columns[column_at:column_at + n_alts], cols)
			head_at += len(head)
			column_at += n_alts
		assert len(heads) == head_at, (what, "the head pool is the concatenation of the heads", at, len(heads), head_at)
		assert int(c["n_columns"]) == column_at, (what, "n_columns", at, int(c["n_columns"]), column_at)
		if words:
			assert columns.shape[0] == column_at, (what, "the column pool", at, columns.shape, column_at)
		at += n
	assert at == len(model_lines), (what, "lines", at, len(model_lines))
