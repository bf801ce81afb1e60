"""One GPU context = one v2m_ctx (include/v2m_hip.h): graph resident in HBM, kernels on its stream."""

import ctypes as C

import numpy as np

from . import _native as N


class V2MError(RuntimeError):
	def __init__(self, code, message):
		super().__init__("%s: %s" % (N.ERROR_NAMES.get(code, "V2M_ERR_%d" % code), message))
		self.code = code


class RowBatch:
	"""v2m_row_batch: per row either a constant chromosome copy (PLOIDY_MAX = REF row) or a list of
	(cut node, copy) pairs (the founder delegate, founder_sequence_greedy_output.cc:78-115)."""

	def __init__(self, rows):
		copy_index, cut_offsets, cut_nodes, cut_copies = [], [0], [], []
		any_cuts = False
		for r in rows:
			if isinstance(r, (int, np.integer)):
				copy_index.append(int(r))
			else:
				any_cuts = True
				copy_index.append(N.V2M_PLOIDY_MAX)
				for node, copy in r:
					cut_nodes.append(int(node))
					cut_copies.append(int(copy))
			cut_offsets.append(len(cut_nodes))
		self.n_rows = len(copy_index)
		self.copy_index = np.ascontiguousarray(copy_index, dtype=np.uint32)
		self.cut_offsets = np.ascontiguousarray(cut_offsets, dtype=np.uint64) if any_cuts else None
		self.cut_nodes = np.ascontiguousarray(cut_nodes, dtype=np.uint64)
		self.cut_copies = np.ascontiguousarray(cut_copies, dtype=np.uint32)
		self.struct = N.RowBatchStruct(
			self.n_rows,
			self.copy_index.ctypes.data if self.n_rows else None,
			self.cut_offsets.ctypes.data if any_cuts else None,
			self.cut_nodes.ctypes.data if len(cut_nodes) else None,
			self.cut_copies.ctypes.data if len(cut_copies) else None,
		)

	@classmethod
	def haplotypes(cls, copies, include_reference=False):
		rows = ([N.V2M_PLOIDY_MAX] if include_reference else []) + [int(c) for c in copies]
		return cls(rows)


def first_record_layout(line, excluded=(), path_alignment=64):
	"""The layout the host's first-record code derives from a VCF record (bytes): every sample's ploidy from the width of its GT, rows
	numbered over the included copies in order; excluded: (sample index, copy index) pairs.  For Context.vcf_scan and host.scan_lines_host."""
	fields = bytes(line).rstrip(b"\r").split(b"\t")
	gt_index = fields[8].split(b":").index(b"GT")
	copy_begin, row_lookup, row = [0], [], 0
	for s, field in enumerate(fields[9:]):
		gt = field.split(b":")[gt_index]
		for c in range(1 + gt.count(b"|") + gt.count(b"/")):
			if (s, c) in excluded:
				row_lookup.append(-1)
			else:
				row_lookup.append(row)
				row += 1
		copy_begin.append(len(row_lookup))
	return dict(n_samples=len(fields) - 9, n_rows=row, words_per_column=(row + path_alignment - 1) // path_alignment * (path_alignment // 64),
		copy_begin=copy_begin, row_lookup=row_lookup)


def collect_vcf_scan(call, layout):
	"""Runs call(layout_fn, chunk_fn) -- v2m_vcf_scan or the host scanner, which share their callbacks -- and returns (code, chunks, layout
	line index or None).  A chunk is a dict: first_line, lines (structured array, N.VCF_LINE_DTYPE), heads (bytes), columns (uint64 array
	[n_columns, words_per_column]), words_per_column, n_columns.  layout(line_index, line) returns what first_record_layout returns."""
	chunks, keep, seen = [], [], []

	def on_layout(_user, line_index, line, length, out):
		try:
			d = layout(line_index, C.string_at(line, length))
			cb = np.ascontiguousarray(d["copy_begin"], dtype=np.uint32)
			rl = np.ascontiguousarray(d["row_lookup"] if len(d["row_lookup"]) else [0], dtype=np.int32)
			keep.extend([cb, rl])
			out[0].n_samples, out[0].n_rows, out[0].words_per_column = d["n_samples"], d["n_rows"], d["words_per_column"]
			out[0].copy_begin, out[0].row_lookup = cb.ctypes.data, rl.ctypes.data
			seen.append(line_index)
			return 0
		except Exception as e:   # nothing may cross the C boundary
			keep.append(e)
			return 1

	def on_chunk(_user, c):
		c = c[0]
		lines = np.frombuffer(C.string_at(c.lines, c.n_lines * C.sizeof(N.VcfLine)), dtype=N.VCF_LINE_DTYPE).copy()
		heads = C.string_at(c.heads, c.head_bytes) if c.head_bytes else b""
		n_words = c.n_columns * c.words_per_column
		columns = np.frombuffer(C.string_at(c.columns, 8 * n_words), dtype=np.uint64).copy() if n_words else np.zeros(0, np.uint64)
		chunks.append(dict(first_line=c.first_line, lines=lines, heads=heads, columns=columns.reshape(c.n_columns, c.words_per_column) if n_words else columns.reshape(0, c.words_per_column),
			words_per_column=c.words_per_column, n_columns=c.n_columns))
		return 0

	rc = call(N.VCF_LAYOUT_FN(on_layout), N.VCF_CHUNK_FN(on_chunk))
	for k in keep:
		if isinstance(k, Exception):
			raise k
	return rc, chunks, (seen[0] if seen else None)


class Context:
	def __init__(self, device=0):
		self._lib = N.load()
		h = C.c_void_p()
		rc = self._lib.v2m_ctx_create(device, C.byref(h))
		if rc != N.V2M_OK:
			raise V2MError(rc, self._lib.v2m_last_error(None).decode())
		self._h = h
		self._keepalive = None

	def close(self):
		if getattr(self, "_h", None):
			self._lib.v2m_ctx_destroy(self._h)
			self._h = None

	def __del__(self):
		try:
			self.close()
		except Exception:
			pass

	def __enter__(self):
		return self

	def __exit__(self, *exc):
		self.close()

	def _check(self, rc):
		if rc != N.V2M_OK:
			raise V2MError(rc, self._lib.v2m_last_error(self._h).decode())

	@property
	def stream(self):
		return self._lib.v2m_ctx_stream(self._h)

	@property
	def info(self):
		return self._lib.v2m_ctx_info(self._h).decode()

	def synchronize(self):
		self._check(self._lib.v2m_ctx_synchronize(self._h))

	# ---- VCF scan --------------------------------------------------------------------------------
	def vcf_scan(self, data, wanted_chr, layout=first_record_layout):
		"""v2m_vcf_scan over `data` (bytes: BGZF or plain VCF text).  Returns the chunks as collect_vcf_scan describes them; for tests and
		tools.  layout(line_index, line) -> the layout of the first record on wanted_chr (default: first_record_layout, nothing excluded)."""
		data = bytes(data)
		fn = layout if layout is not first_record_layout else (lambda _i, line: first_record_layout(line))
		rc, chunks, self.vcf_layout_line = collect_vcf_scan(
			lambda lf, cf: self._lib.v2m_vcf_scan(self._h, C.cast(C.c_char_p(data), C.c_void_p), len(data), wanted_chr.encode(), lf, cf, None), fn)
		self._check(rc)
		return chunks

	# ---- transpose_matrix (transpose_matrix.hh:14) --------------------------------------------
	def transpose_matrix(self, words, n_rows, n_cols):
		"""Host form: column-major u64 words of an n_rows x n_cols bit matrix -> words of its transpose."""
		src = np.ascontiguousarray(words, dtype=np.uint64)
		dst = np.zeros(src.size, dtype=np.uint64)
		self._check(self._lib.v2m_transpose_bits(self._h, src.ctypes.data if src.size else None, n_rows, n_cols, dst.ctypes.data if dst.size else None))
		return dst

	def transpose_bits_device(self, d_src, n_rows, n_cols, d_dst):
		self._check(self._lib.v2m_transpose_bits_device(self._h, d_src, n_rows, n_cols, d_dst))

	# ---- graph ---------------------------------------------------------------------------------
	def upload_graph(self, graph, ref_seq):
		ref = bytes(ref_seq)
		lb = graph.label_bytes
		view = N.GraphView(
			graph.node_count, graph.edge_count,
			graph.reference_positions.ctypes.data, graph.aligned_positions.ctypes.data,
			graph.alt_edge_targets.ctypes.data if graph.edge_count else None,
			graph.alt_edge_count_csum.ctypes.data,
			graph.label_offsets.ctypes.data if graph.edge_count else None,
			C.cast(C.c_char_p(lb), C.c_void_p) if lb else None,
			graph.paths_by_chrom_copy_and_edge.ctypes.data if graph.paths_by_chrom_copy_and_edge is not None and graph.paths_by_chrom_copy_and_edge.size else None,
			graph.path_rows, graph.path_cols,
		)
		self._check(self._lib.v2m_upload_graph(self._h, C.byref(view), C.cast(C.c_char_p(ref), C.c_void_p) if ref else None, len(ref)))

	def set_paths_device(self, d_words, path_rows, path_cols):
		self._check(self._lib.v2m_set_paths_device(self._h, d_words, path_rows, path_cols))

	def bind_path_matrix_device(self, d_paths_by_edge_and_chrom_copy, n_rows, n_cols):
		"""v2m_bind_path_matrix_device: transposes a device-resident transpose input (n_rows copies x n_cols edges) into the
		context's own, line-aligned path matrix and binds it.  Asynchronous."""
		self._check(self._lib.v2m_bind_path_matrix_device(self._h, d_paths_by_edge_and_chrom_copy, n_rows, n_cols))

	def upload_path_slice(self, paths_by_edge_and_chrom_copy, n_rows, n_cols, first_copy=0, n_copies=None):
		"""v2m_upload_path_slice: this GPU's chromosome copies [first_copy, first_copy + n_copies) out of the whole host-resident
		transpose input (n_rows copies x n_cols edges), transposed on the GPU and bound as the uploaded graph's path matrix."""
		words = np.ascontiguousarray(paths_by_edge_and_chrom_copy, dtype=np.uint64)
		assert words.size == n_rows // 64 * n_cols
		n_copies = n_rows - first_copy if n_copies is None else n_copies
		self._check(self._lib.v2m_upload_path_slice(self._h, words.ctypes.data if words.size else None, n_rows, n_cols, first_copy, n_copies))

	def upload_path_blocks(self, paths_by_edge_and_chrom_copy, n_rows, n_cols, first_copy, block_copies, stride_copies, copy_end=None):
		"""v2m_upload_path_blocks: every stride_copies-th block of block_copies chromosome copies from first_copy on (up to copy_end):
		the share of one of several GPUs whose rows have to leave in row order.  Local copy l = global copy
		first_copy + (l // block_copies) * stride_copies + l % block_copies."""
		words = np.ascontiguousarray(paths_by_edge_and_chrom_copy, dtype=np.uint64)
		assert words.size == n_rows // 64 * n_cols
		self._check(self._lib.v2m_upload_path_blocks(self._h, words.ctypes.data if words.size else None, n_rows, n_cols, first_copy, block_copies, stride_copies,
			n_rows if copy_end is None else copy_end))

	@property
	def aligned_length(self):
		return self._lib.v2m_aligned_length(self._h)

	@property
	def min_row_pitch(self):
		return self._lib.v2m_min_row_pitch(self._h)

	@property
	def max_unaligned_length(self):
		return self._lib.v2m_max_unaligned_length(self._h)

	def set_column_window(self, col_begin, col_end):
		"""v2m_set_column_window: every following row call produces columns [col_begin, col_end) of the rows (aligned: exactly those
		bytes; unaligned: the emitted bytes whose column lies there).  (0, aligned_length) is the whole row again, as is a new upload."""
		self._check(self._lib.v2m_set_column_window(self._h, int(col_begin), int(col_end)))

	@property
	def window_length(self):
		"""v2m_window_length: col_end - col_begin of the column window, the aligned length without one."""
		return self._lib.v2m_window_length(self._h)

	# ---- window sets ---------------------------------------------------------------------------
	def set_window_set(self, windows):
		"""v2m_set_window_set: `windows`, an iterable of (begin, end) column ranges in any order, overlapping or repeated, become the
		context's window set, which splice_window_set[_device] splice in one launch per row batch.  Independent of set_column_window;
		a new upload drops it."""
		begin, end = _window_arrays(windows)
		self._check(self._lib.v2m_set_window_set(self._h, begin.size, begin.ctypes.data if begin.size else None, end.ctypes.data if end.size else None))
		self._window_set = (begin, end)

	@property
	def window_set_size(self):
		return self._lib.v2m_window_set_size(self._h)

	@property
	def window_set_layout(self):
		"""(slot offsets, record pitch) of the window set: piece k of a row sits at offsets[k] of the row's record."""
		if not self.window_set_size:
			raise V2MError(N.V2M_ERR_STATE, "no window set")
		offsets, _ = window_set_layout(zip(*self._window_set))
		return offsets, int(self._lib.v2m_window_set_pitch(self._h))

	def splice_window_set(self, rows, unaligned=False, bgzf=False):
		"""v2m_splice_window_set: per row a list of bytes, one per window of the set, each what set_column_window + splice_rows gives
		for that window.  (bgzf exists to be refused: V2M_ERR_UNSUPPORTED.)"""
		if not isinstance(rows, RowBatch):
			rows = RowBatch(rows)
		n = self.window_set_size
		offsets = self.window_set_layout[0] if n else []
		collected, error = [], []

		def _cb(_user, _row_index, record, lengths):
			try:
				base = record or 0
				collected.append([C.string_at(base + offsets[k], lengths[k]) if lengths[k] else b"" for k in range(n)])
				return 0
			except BaseException as e:  # propagate through the C frame as V2M_ERR_SINK
				error.append(e)
				return 1

		flags = (N.V2M_SPLICE_UNALIGNED if unaligned else 0) | (N.V2M_SPLICE_BGZF if bgzf else 0)
		rc = self._lib.v2m_splice_window_set(self._h, C.byref(rows.struct), flags, N.WINDOW_SINK_FN(_cb), None)
		if error:
			raise error[0]
		self._check(rc)
		return collected

	def splice_window_set_device(self, rows, d_out, record_pitch, unaligned=False, want_lengths=False):
		"""v2m_splice_window_set_device: records of record_pitch bytes at d_out; returns the [n_rows, n_windows] lengths when asked."""
		if not isinstance(rows, RowBatch):
			rows = RowBatch(rows)
		lengths = np.zeros((rows.n_rows, self.window_set_size), dtype=np.uint32) if want_lengths else None
		self._check(self._lib.v2m_splice_window_set_device(self._h, C.byref(rows.struct), N.V2M_SPLICE_UNALIGNED if unaligned else 0,
			d_out, record_pitch, lengths.ctypes.data if want_lengths and lengths.size else None))
		return lengths

	def splice_window_set_distinct(self, rows, unaligned=False, want_pieces=True, bgzf=False, on_class=None):
		"""v2m_splice_window_set_distinct: (pieces, class_of).  pieces[k] is the list of window k's distinct bodies (bytes) in class order,
		or pieces is None with want_pieces=False (a NULL sink: no piece crosses the link); class_of is a uint32 array [n_rows, n_windows],
		class_of[r, k] the class of piece (r, k).  self.distinct_class_counts is the call's n_classes_out.  on_class(window, class_index,
		first_row, body) sees every sink call in order.  (bgzf exists to be refused: V2M_ERR_UNSUPPORTED.)"""
		if not isinstance(rows, RowBatch):
			rows = RowBatch(rows)
		n = self.window_set_size
		class_of = np.zeros((rows.n_rows, n), dtype=np.uint32)
		counts = np.zeros(max(1, n), dtype=np.uint32)
		pieces, error = [[] for _ in range(n)], []

		def _cb(_user, window, class_index, first_row, ptr, length):
			try:
				body = C.string_at(ptr, length) if length else b""
				if class_index != len(pieces[window]):
					raise AssertionError("class %d of window %d arrived after %d classes" % (class_index, window, len(pieces[window])))
				pieces[window].append(body)
				if on_class is not None:
					on_class(int(window), int(class_index), int(first_row), body)
				return 0
			except BaseException as e:  # propagate through the C frame as V2M_ERR_SINK
				error.append(e)
				return 1

		flags = (N.V2M_SPLICE_UNALIGNED if unaligned else 0) | (N.V2M_SPLICE_BGZF if bgzf else 0)
		sink = N.DISTINCT_SINK_FN(_cb) if want_pieces else C.cast(None, N.DISTINCT_SINK_FN)
		buf = np.zeros(max(1, class_of.size), dtype=np.uint32)   # (never a NULL pointer for an empty table)
		rc = self._lib.v2m_splice_window_set_distinct(self._h, C.byref(rows.struct), flags, sink, None, buf.ctypes.data, counts.ctypes.data)
		if error:
			raise error[0]
		self._check(rc)
		class_of[...] = buf[:class_of.size].reshape(class_of.shape)
		self.distinct_class_counts = counts[:n].copy()
		return (pieces if want_pieces else None), class_of

	# ---- rows ----------------------------------------------------------------------------------
	def splice_rows(self, rows, sink=None, unaligned=False, bgzf=False):
		"""v2m_splice_rows.  sink(row_index, body: bytes) is called per row in order; without a sink the
		bodies are collected and returned as a list.  bgzf=True: each row's body arrives as its BGZF members
		(V2M_SPLICE_BGZF; gzip.decompress() of them is the body, b"" for an empty body)."""
		if not isinstance(rows, RowBatch):
			rows = RowBatch(rows)
		collected = []
		error = []

		def _cb(_user, row_index, ptr, length):
			try:
				body = C.string_at(ptr, length) if length else b""
				if sink is None:
					collected.append(body)
				else:
					sink(row_index, body)
				return 0
			except BaseException as e:  # propagate through the C frame as V2M_ERR_SINK
				error.append(e)
				return 1

		cb = N.SINK_FN(_cb)
		flags = (N.V2M_SPLICE_UNALIGNED if unaligned else 0) | (N.V2M_SPLICE_BGZF if bgzf else 0)
		rc = self._lib.v2m_splice_rows(self._h, C.byref(rows.struct), flags, cb, None)
		if error:
			raise error[0]
		self._check(rc)
		return collected if sink is None else None

	def splice_rows_held(self, rows, on_row, n_slots=4, unaligned=False):
		"""v2m_splice_rows_held: on_row(row_index, address, length, hold) is called per row in order on this thread and may return
		before it is done with the row; the bytes at `address` stay valid until release_row(hold) is called (any thread, once per
		accepted row).  A callback that raises, or returns a true value, refuses the row and ends the call."""
		if not isinstance(rows, RowBatch):
			rows = RowBatch(rows)
		error = []

		def _cb(_user, row_index, ptr, length, hold):
			try:
				return 1 if on_row(row_index, ptr, length, hold) else 0
			except BaseException as e:
				error.append(e)
				return 1

		cb = N.HOLD_SINK_FN(_cb)
		rc = self._lib.v2m_splice_rows_held(self._h, C.byref(rows.struct), N.V2M_SPLICE_UNALIGNED if unaligned else 0, n_slots, cb, None)
		if error:
			raise error[0]
		self._check(rc)

	def release_row(self, hold):
		self._lib.v2m_row_release(hold)

	def splice_rows_device(self, rows, d_out, row_pitch, unaligned=False, want_lengths=False):
		if not isinstance(rows, RowBatch):
			rows = RowBatch(rows)
		lengths = np.zeros(rows.n_rows, dtype=np.uint64) if want_lengths else None
		self._check(self._lib.v2m_splice_rows_device(self._h, C.byref(rows.struct), N.V2M_SPLICE_UNALIGNED if unaligned else 0,
			d_out, row_pitch, lengths.ctypes.data if want_lengths and rows.n_rows else None))
		return lengths

	def row_ops(self, rows, split_match=False):
		"""v2m_row_ops: per row ((n, 2) uint32 array of (op, length) with op 0 = M, 1 = I, 2 = D; the row's unaligned length) -- the row's
		alignment to the reference, always of the whole row whatever column window or window set is in force.  split_match
		(V2M_OPS_SPLIT_MATCH): 7 = '=' and 8 = X in place of M -- the row's byte equals the REF row's, letters compared without case, or not."""
		if not isinstance(rows, RowBatch):
			rows = RowBatch(rows)
		collected, error = [], []

		def _cb(_user, _row_index, ops, n_ops, row_length):
			try:
				a = np.frombuffer(C.string_at(ops, 8 * n_ops), dtype=np.uint32).reshape(n_ops, 2).copy() if n_ops else np.zeros((0, 2), np.uint32)
				collected.append((a, int(row_length)))
				return 0
			except BaseException as e:  # propagate through the C frame as V2M_ERR_SINK
				error.append(e)
				return 1

		rc = self._lib.v2m_row_ops(self._h, C.byref(rows.struct), N.OPS_SPLIT_MATCH if split_match else 0, N.OPS_SINK_FN(_cb), None)
		if error:
			raise error[0]
		self._check(rc)
		return collected

	def column_counts(self, rows, variable_only=False):
		"""v2m_column_counts: (columns u64[n], counts u32[n, 6]) -- per column of the view in force (the whole row, or the column window)
		how many rows of the batch hold A, C, G, T, N (either case) or '-' there; `columns` are absolute and ascend.  variable_only
		(V2M_COUNTS_VARIABLE_ONLY): only the columns where no class -- "other", rows minus the six, included -- holds every row."""
		if not isinstance(rows, RowBatch):
			rows = RowBatch(rows)
		blocks, error = [], []

		def _cb(_user, records, n):
			try:
				blocks.append(np.frombuffer(C.string_at(records, 32 * n), dtype=np.dtype(N.COLUMN_COUNT_DTYPE)).copy())
				return 0
			except BaseException as e:  # propagate through the C frame as V2M_ERR_SINK
				error.append(e)
				return 1

		rc = self._lib.v2m_column_counts(self._h, C.byref(rows.struct), N.COUNTS_VARIABLE_ONLY if variable_only else 0, N.COLUMN_COUNTS_SINK_FN(_cb), None)
		if error:
			raise error[0]
		self._check(rc)
		self.column_count_blocks = [len(b) for b in blocks]   # the sizes of the blocks the records arrived in
		records = np.concatenate(blocks) if blocks else np.zeros(0, dtype=np.dtype(N.COLUMN_COUNT_DTYPE))
		return records["column"].copy(), records["count"].copy()

	def column_counts_device(self, rows, ptr, plane_pitch, accumulate=False):
		"""v2m_column_counts_device: the counts into device memory at `ptr`, u32[6][plane_pitch] (16-byte aligned, plane_pitch a multiple
		of 4 and at least the view's length rounded up to 4); accumulate (V2M_COUNTS_ACCUMULATE) adds to what is there."""
		if not isinstance(rows, RowBatch):
			rows = RowBatch(rows)
		self._check(self._lib.v2m_column_counts_device(self._h, C.byref(rows.struct), N.COUNTS_ACCUMULATE if accumulate else 0, ptr, plane_pitch))

	def pair_distances(self, rows, acgt_only=False, info=False):
		"""v2m_pair_distances: np.uint32[n, n], the number of columns of the view in force (the whole row, or the column window) in which
		two rows of the batch differ by class (A, C, G, T, N, gap, other) -- with acgt_only (V2M_DIST_ACGT_ONLY) the columns where both hold
		one of A, C, G, T and differ.  With info=True: (matrix, dict of v2m_pair_distances_info's fields)."""
		if not isinstance(rows, RowBatch):
			rows = RowBatch(rows)
		n = int(rows.struct.n_rows)
		dist = np.zeros(max(1, n * n), dtype=np.uint32)   # (never a NULL pointer: no rows is no error)
		record = N.PairDistancesInfo()
		self._check(self._lib.v2m_pair_distances(self._h, C.byref(rows.struct), N.DIST_ACGT_ONLY if acgt_only else 0, dist.ctypes.data, C.byref(record)))
		dist = dist[:n * n].reshape(n, n)
		if n == 0:
			record.n_columns = self.window_length   # (with no rows the call returns before it writes the info)
		if info:
			return dist, {name: getattr(record, name) for name, _ in N.PairDistancesInfo._fields_}
		return dist

	def _weighted_result(self, n, dist, record, info):
		dist = dist[:n * n].reshape(n, n)
		if n == 0:
			record.n_columns = self.window_length   # (with no rows the call returns before it writes the info)
		if info:
			return dist, {name: getattr(record, name) for name, _ in N.PairDistancesInfo._fields_}
		return dist

	def pair_distances_weighted(self, rows, weights, acgt_only=False, info=False):
		"""v2m_pair_distances_weighted: np.uint32[n, n], the pair distances with column c of the view in force counted weights[c] times
		(one u32 per column of the view; their sum must be below 2^32).  With info=True: (matrix, dict of v2m_pair_distances_info's
		fields)."""
		if not isinstance(rows, RowBatch):
			rows = RowBatch(rows)
		weights = np.ascontiguousarray(weights, dtype=np.uint32)
		if weights.ndim != 1 or weights.size != self.window_length:
			raise ValueError("weights holds %d values and the view %d columns" % (weights.size, self.window_length))
		n = int(rows.struct.n_rows)
		dist = np.zeros(max(1, n * n), dtype=np.uint32)
		record = N.PairDistancesInfo()
		self._check(self._lib.v2m_pair_distances_weighted(self._h, C.byref(rows.struct), N.DIST_ACGT_ONLY if acgt_only else 0,
			weights.ctypes.data if weights.size else None, dist.ctypes.data, C.byref(record)))
		return self._weighted_result(n, dist, record, info)

	def bootstrap_distances(self, rows, seed, replicate, acgt_only=False, info=False):
		"""v2m_bootstrap_distances: np.uint32[n, n], the weighted pair distances of bootstrap replicate `replicate` (any u32) under
		`seed` (any u64): the columns of the view in force drawn with replacement as include/v2m_hip.h, "bootstrap", defines the draws."""
		if not isinstance(rows, RowBatch):
			rows = RowBatch(rows)
		n = int(rows.struct.n_rows)
		dist = np.zeros(max(1, n * n), dtype=np.uint32)
		record = N.PairDistancesInfo()
		self._check(self._lib.v2m_bootstrap_distances(self._h, C.byref(rows.struct), N.DIST_ACGT_ONLY if acgt_only else 0, int(seed), int(replicate),
			dist.ctypes.data, C.byref(record)))
		return self._weighted_result(n, dist, record, info)

	def pair_distances_device(self, rows, ptr, pitch, acgt_only=False):
		"""v2m_pair_distances_device: the matrix into device memory at `ptr`, u32[n][pitch] (16-byte aligned, pitch a multiple of 4 and at
		least n); elements [i][j < n] are overwritten, nothing else is touched."""
		if not isinstance(rows, RowBatch):
			rows = RowBatch(rows)
		self._check(self._lib.v2m_pair_distances_device(self._h, C.byref(rows.struct), N.DIST_ACGT_ONLY if acgt_only else 0, ptr, pitch))

	def variable_sites(self, rows, snp_only=False, info=False):
		"""v2m_variable_sites: (columns np.uint64[V], bytes np.uint8[n, V]) -- the rows of the batch cut down to the variable columns of
		the view in force (the whole row, or the column window), byte for byte; `columns` are absolute and ascend.  snp_only
		(V2M_SITES_SNP): only the columns where at least two of A, C, G, T occur.  With info=True: (columns, bytes, dict of
		v2m_variable_sites_info's fields).  self.variable_sites_blocks: the (first_row, n_rows) of the blocks the rows arrived in."""
		if not isinstance(rows, RowBatch):
			rows = RowBatch(rows)
		n = int(rows.struct.n_rows)
		columns, blocks, error = [], [], []

		def _columns(_user, cols, n_sites):
			try:
				columns.append(np.frombuffer(C.string_at(cols, 8 * n_sites), dtype=np.uint64).copy())
				return 0
			except BaseException as e:  # propagate through the C frame as V2M_ERR_SINK
				error.append(e)
				return 1

		def _rows(_user, first_row, n_rows, data, pitch, n_sites):
			try:
				if not columns:
					raise AssertionError("rows before the columns")
				a = np.frombuffer(C.string_at(data, (n_rows - 1) * pitch + n_sites), dtype=np.uint8)
				a = np.lib.stride_tricks.as_strided(a, shape=(n_rows, n_sites), strides=(pitch, 1)).copy()
				blocks.append((int(first_row), a))
				return 0
			except BaseException as e:
				error.append(e)
				return 1

		record = N.VariableSitesInfo()
		rc = self._lib.v2m_variable_sites(self._h, C.byref(rows.struct), N.SITES_SNP if snp_only else 0, N.SITE_COLUMNS_SINK_FN(_columns), N.SITE_ROWS_SINK_FN(_rows), None, C.byref(record))
		if error:
			raise error[0]
		self._check(rc)
		if len(columns) > 1:
			raise AssertionError("the columns arrived %d times" % len(columns))
		self.variable_sites_blocks = [(first, len(a)) for first, a in blocks]
		cols = columns[0] if columns else np.zeros(0, dtype=np.uint64)
		data = np.concatenate([a for _, a in blocks]) if blocks else np.zeros((n, 0), dtype=np.uint8)
		if n == 0:
			record.n_columns = self.window_length   # (with no rows the call returns before it writes the info)
		if info:
			return cols, data, {name: getattr(record, name) for name, _ in N.VariableSitesInfo._fields_}
		return cols, data

	def variable_sites_device(self, rows, ptr, pitch, columns_ptr=None, snp_only=False):
		"""v2m_variable_sites_device: the rows' bytes at the sites into device memory at `ptr`, u8[n][pitch] (16-byte aligned, pitch a
		multiple of 16), and the view-relative columns into u32[pitch] at `columns_ptr` when given.  Returns V, the number of sites; with
		V > pitch the call raises (self.variable_sites_count then holds V) and has written nothing."""
		if not isinstance(rows, RowBatch):
			rows = RowBatch(rows)
		count = C.c_uint64(0)
		self.variable_sites_count = None
		rc = self._lib.v2m_variable_sites_device(self._h, C.byref(rows.struct), N.SITES_SNP if snp_only else 0, columns_ptr, ptr, pitch, C.byref(count))
		self.variable_sites_count = int(count.value)
		self._check(rc)
		return int(count.value)

	@staticmethod
	def _site_ld_params(window_sites, window_columns, min_r2, min_allele_count):
		num, den = min_r2
		return N.SiteLdParams(int(window_sites), int(min_allele_count), int(num), int(den), int(window_columns))

	def site_ld(self, rows, window_sites=1000, window_columns=0, min_r2=(1, 5), min_allele_count=1, info=False, want_sites=True, want_pairs=True):
		"""v2m_site_ld: (sites, pairs), numpy structured arrays of v2m_ld_site and v2m_ld_pair records -- the biallelic sites of the view
		in force (the whole row, or the column window) and, of the site pairs (s, t) with t - s <= window_sites and, unless window_columns
		is 0, a column distance of at most window_columns, those whose r^2 = D^2 / den reaches min_r2 = (numerator, denominator), compared
		exactly in integers; ascending by (s, t).  With info=True: (sites, pairs, dict of v2m_site_ld_info's fields).  want_sites /
		want_pairs = False pass a NULL sink.  self.site_ld_blocks: the sizes of the blocks the pairs arrived in."""
		if not isinstance(rows, RowBatch):
			rows = RowBatch(rows)
		n = int(rows.struct.n_rows)
		sites, blocks, error = [], [], []

		def _sites(_user, records, count):
			try:
				if blocks:
					raise AssertionError("the sites after a pair")
				sites.append(np.frombuffer(C.string_at(records, 24 * count), dtype=np.dtype(N.LD_SITE_DTYPE)).copy())
				return 0
			except BaseException as e:  # propagate through the C frame as V2M_ERR_SINK
				error.append(e)
				return 1

		def _pairs(_user, records, count):
			try:
				if count == 0:
					raise AssertionError("a block of no pairs")
				blocks.append(np.frombuffer(C.string_at(records, 24 * count), dtype=np.dtype(N.LD_PAIR_DTYPE)).copy())
				return 0
			except BaseException as e:
				error.append(e)
				return 1

		params = self._site_ld_params(window_sites, window_columns, min_r2, min_allele_count)
		record = N.SiteLdInfo()
		no_sink = C.cast(None, N.LD_SINK_FN)
		rc = self._lib.v2m_site_ld(self._h, C.byref(rows.struct), C.byref(params), N.LD_SINK_FN(_sites) if want_sites else no_sink,
			N.LD_SINK_FN(_pairs) if want_pairs else no_sink, None, C.byref(record))
		if error:
			raise error[0]
		self._check(rc)
		if len(sites) > 1:
			raise AssertionError("the sites arrived %d times" % len(sites))
		self.site_ld_blocks = [len(b) for b in blocks]
		site_records = sites[0] if sites else np.zeros(0, dtype=np.dtype(N.LD_SITE_DTYPE))
		pair_records = np.concatenate(blocks) if blocks else np.zeros(0, dtype=np.dtype(N.LD_PAIR_DTYPE))
		if n == 0:
			record.n_columns = self.window_length   # (with no rows the call returns before it writes the info)
		if info:
			return site_records, pair_records, {name: getattr(record, name) for name, _ in N.SiteLdInfo._fields_}
		return site_records, pair_records

	def site_ld_device(self, rows, sites_ptr, site_capacity, pairs_ptr, pair_capacity, window_sites=1000, window_columns=0, min_r2=(1, 5), min_allele_count=1):
		"""v2m_site_ld_device: the site records into device memory at `sites_ptr` (v2m_ld_site[site_capacity]) and the reported pairs at
		`pairs_ptr` (v2m_ld_pair[pair_capacity]; None with capacity 0 asks for the counts only), both 16-byte aligned.  Returns
		(n_sites, n_pairs); when either exceeds its capacity the call raises (self.site_ld_counts then holds both) and has written
		nothing."""
		if not isinstance(rows, RowBatch):
			rows = RowBatch(rows)
		params = self._site_ld_params(window_sites, window_columns, min_r2, min_allele_count)
		n_sites, n_pairs = C.c_uint64(0), C.c_uint64(0)
		self.site_ld_counts = None
		rc = self._lib.v2m_site_ld_device(self._h, C.byref(rows.struct), C.byref(params), sites_ptr, site_capacity, pairs_ptr, pair_capacity, C.byref(n_sites), C.byref(n_pairs))
		self.site_ld_counts = (int(n_sites.value), int(n_pairs.value))
		self._check(rc)
		return self.site_ld_counts

	@staticmethod
	def _nj_result(n, nodes, record, info):
		nodes = nodes[:max(0, n - 2)] if n >= 3 else nodes[:0]
		if info:
			return nodes, {name: getattr(record, name) for name, _ in N.NjTreeInfo._fields_}
		return nodes

	def nj_tree(self, rows, acgt_only=False, info=False):
		"""v2m_nj_tree: the neighbour-joining tree of the batch's rows over the view in force, from their pair distances (acgt_only:
		V2M_DIST_ACGT_ONLY), as a structured array of the n - 2 v2m_nj_node records (a, b, c, reserved, len_a, len_b, len_c): the joins in
		order, node n + t made at join t, then the trifurcation.  No rows give no records; one or two raise.  With info=True: (records,
		dict of v2m_nj_tree_info's fields)."""
		if not isinstance(rows, RowBatch):
			rows = RowBatch(rows)
		n = int(rows.struct.n_rows)
		nodes = np.zeros(max(1, n - 2), dtype=np.dtype(N.NJ_NODE_DTYPE))   # (never a NULL pointer: no rows is no error)
		record = N.NjTreeInfo()
		self._check(self._lib.v2m_nj_tree(self._h, C.byref(rows.struct), N.DIST_ACGT_ONLY if acgt_only else 0, nodes.ctypes.data, C.byref(record)))
		if n == 0:
			record.n_columns = self.window_length   # (with no rows the call returns before it writes the info)
		return self._nj_result(n, nodes, record, info)

	def nj_bootstrap(self, rows, n_replicates, seed=1, acgt_only=False, replicates=False, info=False):
		"""v2m_nj_bootstrap: (nodes, support) -- nj_tree's records and, per join record, the number of the n_replicates bootstrap
		replicates under `seed` whose tree holds the record's split (np.uint32[n - 3]).  replicates=True adds the replicate trees, a
		structured array [n_replicates, n - 2]; info=True adds the dict of v2m_nj_bootstrap_info's fields."""
		if not isinstance(rows, RowBatch):
			rows = RowBatch(rows)
		n = int(rows.struct.n_rows)
		n_replicates = int(n_replicates)
		if not 0 <= n_replicates < 1 << 32 or not 0 <= int(seed) < 1 << 64:
			raise ValueError("n_replicates is a u32 and seed a u64 (got %d and %d)" % (n_replicates, int(seed)))
		nodes = np.zeros(max(1, n - 2), dtype=np.dtype(N.NJ_NODE_DTYPE))   # (never a NULL pointer: no rows is no error)
		support = np.zeros(max(1, n - 3), dtype=np.uint32)
		keep = replicates and 1 <= n_replicates <= N.NJ_BOOTSTRAP_MAX_REPLICATES
		trees = np.zeros((n_replicates if keep else 1, max(1, n - 2)), dtype=np.dtype(N.NJ_NODE_DTYPE))
		record = N.NjBootstrapInfo()
		self._check(self._lib.v2m_nj_bootstrap(self._h, C.byref(rows.struct), N.DIST_ACGT_ONLY if acgt_only else 0, n_replicates, int(seed),
			nodes.ctypes.data, support.ctypes.data, trees.ctypes.data if keep else None, C.byref(record)))
		result = [nodes[:max(0, n - 2)] if n >= 3 else nodes[:0], support[:max(0, n - 3)]]
		if replicates:
			result.append(trees[:, :n - 2] if n >= 3 else trees[:0, :0])
		if info:
			result.append({name: getattr(record, name) for name, _ in N.NjBootstrapInfo._fields_})
		return tuple(result)

	def nj_tree_of_distances(self, ptr, n, pitch, info=False):
		"""v2m_nj_tree_of_distances: the tree of the n taxa whose distances lie in device memory at `ptr`, u32[n][pitch] (16-byte aligned,
		pitch a multiple of 4 and at least n; only the upper triangle is read, nothing is written): the records of nj_tree."""
		n = int(n)
		nodes = np.zeros(max(1, n - 2 if n <= N.NJ_MAX_ROWS else 1), dtype=np.dtype(N.NJ_NODE_DTYPE))
		record = N.NjTreeInfo()
		self._check(self._lib.v2m_nj_tree_of_distances(self._h, ptr, n, int(pitch), nodes.ctypes.data, C.byref(record)))
		return self._nj_result(n, nodes, record, info)

	def tree_parsimony(self, rows, nodes, info=False, want_sites=True, want_mutations=True, want_branch_changes=True):
		"""v2m_tree_parsimony: Fitch's parsimony of the SNP sites of the view in force on the tree of `nodes` (n - 2 v2m_nj_node records
		over the batch's rows as leaves, as nj_tree returns them): (sites, branch_changes, mutations) -- structured arrays of
		v2m_tree_site (column, steps, present) and v2m_tree_mutation (site, node, from, to) records and np.uint32[2 n - 3].  With
		info=True: (..., dict of v2m_tree_parsimony_info's fields).  want_* = False pass a NULL sink or pointer (an empty array comes
		back).  self.tree_parsimony_blocks: the sizes of the blocks the mutations arrived in."""
		if not isinstance(rows, RowBatch):
			rows = RowBatch(rows)
		n = int(rows.struct.n_rows)
		nodes = np.ascontiguousarray(nodes, dtype=np.dtype(N.NJ_NODE_DTYPE))
		sites, blocks, error = [], [], []

		def _sites(_user, records, count):
			try:
				if count == 0:
					raise AssertionError("a call with no site")
				sites.append(_records(records, count, N.TREE_SITE_DTYPE))
				return 0
			except BaseException as e:  # propagate through the C frame as V2M_ERR_SINK
				error.append(e)
				return 1

		def _mutations(_user, records, count):
			try:
				if count == 0:
					raise AssertionError("a block of no mutations")
				if sites:
					raise AssertionError("a mutation after the sites")
				blocks.append(_records(records, count, N.TREE_MUTATION_DTYPE))
				return 0
			except BaseException as e:
				error.append(e)
				return 1

		def _records(ptr, count, dtype):
			out = np.empty(count, dtype=np.dtype(dtype))                     # (a block of mutations may hold more than 2^31 bytes)
			C.memmove(out.ctypes.data, ptr, out.nbytes)
			return out

		branch_changes = np.zeros(max(1, 2 * n - 3), dtype=np.uint32)
		record = N.TreeParsimonyInfo()
		no_sink = C.cast(None, N.TREE_SINK_FN)
		rc = self._lib.v2m_tree_parsimony(self._h, C.byref(rows.struct), nodes.ctypes.data if len(nodes) else None, 0,
			branch_changes.ctypes.data if want_branch_changes else None, N.TREE_SINK_FN(_sites) if want_sites else no_sink,
			N.TREE_SINK_FN(_mutations) if want_mutations else no_sink, None, C.byref(record))
		if error:
			raise error[0]
		self._check(rc)
		if len(sites) > 1:
			raise AssertionError("the sites arrived %d times" % len(sites))
		self.tree_parsimony_blocks = [len(b) for b in blocks]
		result = [sites[0] if sites else np.zeros(0, dtype=np.dtype(N.TREE_SITE_DTYPE)),
			branch_changes[:2 * n - 3] if n >= 3 and want_branch_changes else branch_changes[:0],
			np.concatenate(blocks) if blocks else np.zeros(0, dtype=np.dtype(N.TREE_MUTATION_DTYPE))]
		if n == 0:
			record.n_columns = self.window_length   # (with no rows the call returns before it writes the info)
		if info:
			result.append({name: getattr(record, name) for name, _ in N.TreeParsimonyInfo._fields_})
		return tuple(result)

	def parsimony_of_sites(self, bytes_ptr, n, n_sites, pitch, nodes, sites_ptr, branch_changes_ptr, mutations_ptr=None, capacity=0):
		"""v2m_parsimony_of_sites: the parsimony of the n_sites sites of the n rows in device memory at `bytes_ptr`, u8[n][pitch] (16-byte
		aligned, pitch a multiple of 16 and at least n_sites; nothing is written there), on the tree of `nodes` (host, n - 2 records):
		v2m_parsimony_site[n_sites] to `sites_ptr`, u32[2 n - 3] to `branch_changes_ptr` and the mutations to `mutations_ptr`
		(v2m_tree_mutation[capacity]; None with capacity 0 asks for everything but the list), all device memory.  Returns the number of
		mutations; when they exceed a non-zero capacity the call raises (self.parsimony_mutations then holds their number) and has
		written neither the list nor the branch counts."""
		nodes = np.ascontiguousarray(nodes, dtype=np.dtype(N.NJ_NODE_DTYPE))
		n_mutations = C.c_uint64(0)
		self.parsimony_mutations = None
		rc = self._lib.v2m_parsimony_of_sites(self._h, bytes_ptr, int(n), int(n_sites), int(pitch), nodes.ctypes.data if len(nodes) else None, sites_ptr, branch_changes_ptr,
			mutations_ptr, int(capacity), C.byref(n_mutations))
		self.parsimony_mutations = int(n_mutations.value)
		self._check(rc)
		return self.parsimony_mutations

	def window_diversity(self, rows, bounds, rows_b=None, want_sfs=True, info=False):
		"""v2m_window_diversity: the bin records of include/v2m_hip.h's "window diversity" for the rows of the batch over the bins
		[bounds[k], bounds[k + 1]) -- absolute columns inside the view in force, ascending.  Within form (rows_b None): (bins, sfs), a
		structured array of v2m_diversity_bin and np.uint64[n / 2 + 1] (None with want_sfs=False).  Between form: (bins, None), bins of
		v2m_diversity_between_bin.  info=True: (..., dict of v2m_window_diversity_info's fields)."""
		if not isinstance(rows, RowBatch):
			rows = RowBatch(rows)
		if rows_b is not None and not isinstance(rows_b, RowBatch):
			rows_b = RowBatch(rows_b)
		bounds = np.ascontiguousarray(bounds, dtype=np.uint64)
		n_bins = max(0, len(bounds) - 1)
		n = int(rows.struct.n_rows)
		bins = np.zeros(max(1, n_bins), dtype=np.dtype(N.DIVERSITY_BIN_DTYPE if rows_b is None else N.DIVERSITY_BETWEEN_BIN_DTYPE))
		sfs = np.zeros(n // 2 + 1, dtype=np.uint64) if (want_sfs and rows_b is None) else None
		record = N.WindowDiversityInfo()
		self._check(self._lib.v2m_window_diversity(self._h, C.byref(rows.struct), C.byref(rows_b.struct) if rows_b is not None else None,
			bounds.ctypes.data if len(bounds) else None, n_bins, bins.ctypes.data, sfs.ctypes.data if sfs is not None else None, C.byref(record)))
		result = (bins[:n_bins], sfs)
		if info:
			result += ({name: getattr(record, name) for name, _ in N.WindowDiversityInfo._fields_},)
		return result

	def diversity_of_counts(self, counts_ptr, plane_pitch, length, n, bounds, bins_ptr, sfs_ptr=None, counts_b_ptr=None, n_b=0):
		"""v2m_diversity_of_counts: the bin records, and with `sfs_ptr` the folded spectrum, of the counts table in device memory at
		`counts_ptr` (u32[6][plane_pitch] over `length` columns, counted over n rows) -- with `counts_b_ptr`, a second table over n_b
		rows, the between form -- over the bins of `bounds` (host, relative to the tables), into device memory at `bins_ptr` and
		`sfs_ptr`.  Returns the dict of v2m_window_diversity_info's fields."""
		bounds = np.ascontiguousarray(bounds, dtype=np.uint64)
		record = N.WindowDiversityInfo()
		self._check(self._lib.v2m_diversity_of_counts(self._h, counts_ptr, counts_b_ptr, int(plane_pitch), int(length), int(n), int(n_b),
			bounds.ctypes.data if len(bounds) else None, max(0, len(bounds) - 1), bins_ptr, sfs_ptr, C.byref(record)))
		return {name: getattr(record, name) for name, _ in N.WindowDiversityInfo._fields_}

	def bgzf_compress(self, data):
		"""v2m_bgzf_compress: `data` as BGZF members, compressed on the GPU by the kernels of splice_rows(bgzf=True) (no EOF member)."""
		src = bytes(data)
		cap = bgzf_bound(len(src))
		dst = C.create_string_buffer(cap)
		n = C.c_uint64()
		self._check(self._lib.v2m_bgzf_compress(self._h, src if src else None, len(src), dst, cap, C.byref(n)))
		return dst.raw[:n.value]

	def bgzf_decompress(self, data):
		"""v2m_bgzf_decompress: the bytes of BGZF `data`, inflated on the GPU (framing checked on the host first)."""
		src = bytes(data)
		_, n_bytes, _ = bgzf_scan(src)
		dst = C.create_string_buffer(max(1, n_bytes))
		n = C.c_uint64(0)
		self._check(self._lib.v2m_bgzf_decompress(self._h, src if src else None, len(src), dst, n_bytes, C.byref(n)))
		return dst.raw[:n.value]

	def alloc_output(self, nbytes, candidates=3):
		"""v2m_alloc_output: device memory for row output, picked among `candidates` allocations by measured write rate."""
		p = C.c_void_p()
		self._check(self._lib.v2m_alloc_output(self._h, nbytes, candidates, C.byref(p)))
		return p.value

	def free_output(self, ptr):
		self._check(self._lib.v2m_free_output(self._h, ptr))

	def read_output(self, ptr, count, dtype=np.uint8):
		"""v2m_read_output: `count` elements of `dtype` from device memory at `ptr`, after everything queued on the context's stream."""
		out = np.zeros(max(1, int(count)), dtype=np.dtype(dtype))
		self._check(self._lib.v2m_read_output(self._h, ptr, int(count) * out.dtype.itemsize, out.ctypes.data))
		return out[:int(count)]

	def checksum_rows_device(self, d_rows, row_pitch, n_rows, length=0, lengths=None):
		out = np.zeros(n_rows, dtype=np.uint64)
		la = None if lengths is None else np.ascontiguousarray(lengths, dtype=np.uint64)
		self._check(self._lib.v2m_checksum_rows_device(self._h, d_rows, row_pitch, n_rows, length, la.ctypes.data if la is not None else None, out.ctypes.data if n_rows else None))
		return out

	# ---- profiling -----------------------------------------------------------------------------
	def profile_enable(self, enabled=True):
		self._check(self._lib.v2m_profile_enable(self._h, int(enabled)))

	def profile_reset(self):
		self._check(self._lib.v2m_profile_reset(self._h))

	def profile_get(self, kernel):
		n, ms = C.c_uint64(), C.c_double()
		self._check(self._lib.v2m_profile_get(self._h, kernel, C.byref(n), C.byref(ms)))
		return n.value, ms.value


def _profile_launches(self, kernel):
	"""Per-launch device times (ms) of `kernel` since the last profile_reset()."""
	n = C.c_uint64()
	self._check(self._lib.v2m_profile_get_launches(self._h, kernel, None, 0, C.byref(n)))
	out = np.zeros(n.value, dtype=np.float64)
	if n.value:
		self._check(self._lib.v2m_profile_get_launches(self._h, kernel, out.ctypes.data, n.value, C.byref(n)))
	return out


Context.profile_launches = _profile_launches


def _window_arrays(windows):
	pairs = [(int(b), int(e)) for b, e in windows]
	begin = np.ascontiguousarray([b for b, _ in pairs], dtype=np.uint64)
	end = np.ascontiguousarray([e for _, e in pairs], dtype=np.uint64)
	return begin, end


def window_set_layout(windows):
	"""v2m_window_set_layout (host only, no context): (slot offsets, record pitch) of the windows as a set."""
	lib = N.load()
	begin, end = _window_arrays(windows)
	offsets = np.zeros(begin.size, dtype=np.uint64)
	pitch = C.c_uint64(0)
	rc = lib.v2m_window_set_layout(begin.size, begin.ctypes.data if begin.size else None, end.ctypes.data if end.size else None,
		offsets.ctypes.data if begin.size else None, C.byref(pitch))
	if rc != N.V2M_OK:
		raise V2MError(rc, lib.v2m_last_error(None).decode(errors="replace"))
	return [int(o) for o in offsets], pitch.value


def bgzf_bound(n):
	"""v2m_bgzf_bound: the most bytes bgzf_frame_stored / Context.bgzf_compress write for n input bytes."""
	return int(N.load().v2m_bgzf_bound(n))


def bgzf_frame_stored(data):
	"""v2m_bgzf_frame_stored: `data` as stored-block BGZF members (host only); b"" gives exactly the 28-byte EOF member."""
	lib = N.load()
	src = bytes(data)
	cap = bgzf_bound(len(src))
	dst = C.create_string_buffer(cap)
	n = C.c_uint64()
	rc = lib.v2m_bgzf_frame_stored(src if src else None, len(src), dst, cap, C.byref(n))
	if rc != N.V2M_OK:
		raise V2MError(rc, "v2m_bgzf_frame_stored failed")
	return dst.raw[:n.value]


def bgzf_scan(data):
	"""v2m_bgzf_scan (host only): (members, decompressed bytes, ends with the EOF member) of BGZF `data`; V2MError for gzip that is not
	BGZF (V2M_ERR_UNSUPPORTED) and for broken framing (V2M_ERR_INVALID_ARGUMENT)."""
	lib = N.load()
	src = bytes(data)
	m, n, eof = C.c_uint64(0), C.c_uint64(0), C.c_int(0)
	rc = lib.v2m_bgzf_scan(src if src else None, len(src), C.byref(m), C.byref(n), C.byref(eof))
	if rc != N.V2M_OK:
		raise V2MError(rc, lib.v2m_last_error(None).decode(errors="replace"))
	return m.value, n.value, bool(eof.value)


def checksum_rows_host(rows_bytes):
	"""The checksum of v2m_checksum_rows_device computed with numpy (for comparisons in tests/bench)."""
	out = []
	golden = np.uint64(0x9E3779B97F4A7C15)
	for body in rows_bytes:
		n = len(body)
		pad = (-n) % 8
		words = np.frombuffer(bytes(body) + b"\0" * pad, dtype="<u8")
		idx = np.arange(1, words.size + 1, dtype=np.uint64)
		with np.errstate(over="ignore"):
			acc = _mix64(idx * golden ^ words).sum(dtype=np.uint64) if words.size else np.uint64(0)
			acc = acc + _mix64(np.array([n], dtype=np.uint64))[0]
		out.append(int(acc))
	return np.array(out, dtype=np.uint64)


def _mix64(z):
	z = z.astype(np.uint64, copy=True)
	with np.errstate(over="ignore"):
		z ^= z >> np.uint64(30)
		z *= np.uint64(0xBF58476D1CE4E5B9)
		z ^= z >> np.uint64(27)
		z *= np.uint64(0x94D049BB133111EB)
		z ^= z >> np.uint64(31)
	return z
