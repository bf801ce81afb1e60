"""Hand-made graphs for the row kernels' seams, with a plain model of the rows and a census of what the kernels see.  TEST INFRASTRUCTURE ONLY.

The graphs of synth.py come out of a VCF writer and a random generator: nothing decides where a byte, an edge or a 16-byte chunk lands
relative to the kernels' own constants.  Here a graph is described column by column -- which aligned columns hold a reference byte, which
are padding, where nodes and ALT edges begin and end -- turned into the flat arrays of a variant graph with numpy, and handed to
oracle.graph_from_arrays / VariantGraph.from_object.  Three independent things then describe the same rows:

  the model     SeamGraph.body(): the REF row's columns with the spans of the row's effective edges overwritten (label, then padding);
                numpy over the builder's own column description, no oracle call;
  the oracle    OracleGraph.output_sequence(), the restatement of the reference's node walk;
  the kernels   through splice_rows / splice_rows_device (tests/test_gpu_splice_seams.py).

tests/test_seam_graphs_host.py holds the first two equal on a machine without a GPU and runs the census: from the arrays, with the kernels'
own definitions of tile, range, crossing edge, slot and chunk, it recomputes the quantities the kernels branch on and asserts that every
seam value a graph is meant to reach is reached.  Every number comes from csrc/kernels.hpp (kernel_constants()): a changed constant moves
the graphs with it, a renamed one fails loudly.

A row is a chromosome copy (or PLOIDY_MAX, the REF row) or a founder row, a list of (cut node, copy) pairs.  The model of a founder row
is its assembled bit column: per edge the bit of the copy in force at the edge's source node (SeamGraph.assembled, a plain loop).
SegmentCensus recomputes what assemble_row_bits_kernel sees of such a row: the segment table, and per wave span and word what the
kernel's search, lane loop and masks come to (tests/test_gpu_assemble_seams.py)."""

import functools
import os
import re

import numpy as np

import oracle

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KERNELS_HPP = os.path.join(ROOT, "vcf2multialign_amd", "csrc", "kernels.hpp")
PLOIDY_MAX = oracle.PLOIDY_MAX
GAP = ord("-")

CONSTANT_NAMES = ("kTileBytes", "kSpliceThreads", "kLongPatch", "kCandLds", "kLabelLds", "kGroupRowsLds", "kLongQueueLds", "kCandDeltaLds",
	"kCountRowsMax", "kMaxBackWords", "kResolveWordsPerThread")


class Constants(dict):
	__getattr__ = dict.__getitem__


@functools.lru_cache(maxsize=None)
def kernel_constants():
	"""The kernels' constants, read from csrc/kernels.hpp.  kQueue: splice_unaligned_kernel's template default and the literal the window
	kernel instantiates splice_unaligned_tiles with, which must agree."""
	with open(KERNELS_HPP) as f:
		text = f.read()
	out = Constants()
	for name in CONSTANT_NAMES:
		found = re.findall(r"^constexpr\s+(?:int|u32)\s+%s\s*=\s*(\d+)\s*;" % name, text, re.M)
		assert len(found) == 1, "%s: %d definitions of the form `constexpr int|u32 %s = value;` in kernels.hpp" % (name, len(found), name)
		out[name] = int(found[0])
	whole = re.search(r"template\s*<bool kNonTemporal,\s*u32 kQueue\s*=\s*(\d+)>\s*__global__[^{;]*\bsplice_unaligned_kernel\(", text)
	window = re.search(r"\bsplice_unaligned_window_kernel\([^{]*\{\s*splice_unaligned_tiles<kNonTemporal,\s*(\d+),\s*true>", text)
	assert whole and window, "kQueue: splice_unaligned_kernel's default or the window kernel's literal was not found in kernels.hpp"
	assert whole.group(1) == window.group(1), "kQueue differs between the whole-row kernel (%s) and the window kernel (%s)" % (whole.group(1), window.group(1))
	out["kQueue"] = int(whole.group(1))
	out["kTileChunks"] = out["kTileBytes"] // 16
	out["kSlots"] = out["kTileChunks"] // 64            # 1-KiB slots of a tile: 64 lanes x 16 bytes
	assert out["kTileBytes"] % 1024 == 0 and out["kSpliceThreads"] % 64 == 0 and out["kSlots"] * 64 * 16 == out["kTileBytes"]
	return out


# ---- the builder ------------------------------------------------------------------------------------------------------------------------

class Builder:
	"""Columns are appended left to right: kept (a reference byte) or padding.  A node begins at every kept column that follows a padding
	column, and at every column an edge begins or ends at (which must be kept; an edge may also end at the row's end).  So a kept run with
	the padding run after it is one node interval, as in a graph made from a VCF.  Edges are (begin column, end column, label length); add
	them in the order of their begin columns (the end may lie in columns not appended yet).  Reference and label bytes are drawn at
	finish(): ACGT for the reference, acgt for labels, so a misplaced byte of one kind never looks like the other."""

	def __init__(self, seed):
		self.seed = seed
		self._kept = []
		self.length = 0
		self._begin, self._end, self._label_len = [], [], []

	@property
	def n_edges(self):
		return len(self._begin)

	def add_kept(self, flags):
		flags = np.asarray(flags, dtype=bool)
		self._kept.append(flags)
		self.length += flags.size
		return self.length - flags.size

	def add_ref(self, k, pad=0):
		"""k reference bytes, then pad padding columns.  Returns the first column."""
		assert k >= 0 and pad >= 0 and (self.length > 0 or k > 0 or 0 == pad)
		return self.add_kept(np.r_[np.ones(k, bool), np.zeros(pad, bool)])

	def ref_to(self, column):
		assert column >= self.length
		return self.add_ref(column - self.length)

	def pad_to(self, column):
		assert column >= self.length > 0
		return self.add_ref(0, column - self.length)

	def edge(self, begin, end, label_len):
		assert 0 <= begin < end and 0 <= label_len <= end - begin and (not self._begin or begin >= self._begin[-1]), (begin, end, label_len)
		self._begin.append(begin)
		self._end.append(end)
		self._label_len.append(label_len)
		return len(self._begin) - 1

	def add_site(self, label_lens, span, ref_bytes=1):
		"""A node interval of `span` columns, the first ref_bytes of them kept, with one ALT edge per label over exactly that interval.
		The column after it must be kept (or the row's end).  Returns the edges' indices."""
		assert 1 <= ref_bytes <= span
		begin = self.add_ref(ref_bytes, span - ref_bytes)
		return [self.edge(begin, begin + span, n) for n in label_lens]

	def add_sites(self, n, span, ref_bytes, label_len):
		"""n equal sites one after the other, one edge each; returns the first edge's index."""
		first = self.n_edges
		begin = self.add_kept(np.tile(np.r_[np.ones(ref_bytes, bool), np.zeros(span - ref_bytes, bool)], n))
		assert not self._begin or begin >= self._begin[-1]
		self._begin.extend(range(begin, begin + n * span, span))
		self._end.extend(range(begin + span, begin + (n + 1) * span, span))
		self._label_len.extend([label_len] * n)
		return first

	def finish(self, copies, name=""):
		"""copies: per chromosome copy the indices of the edges whose path bit is set."""
		rng = np.random.default_rng(self.seed)
		kept = np.concatenate(self._kept)
		L = kept.size
		begin = np.asarray(self._begin, dtype=np.int64).reshape(-1)
		end = np.asarray(self._end, dtype=np.int64).reshape(-1)
		label_len = np.asarray(self._label_len, dtype=np.int64).reshape(-1)
		E = begin.size
		assert kept[0] and (E == 0 or (end.max() <= L and np.all(np.diff(begin) >= 0)))
		is_node = kept & ~np.r_[False, kept[:-1]]
		for cols in (begin, end[end < L]):
			assert np.all(kept[cols]), "an edge begins or ends in a padding column"
			is_node[cols] = True
		node_cols = np.flatnonzero(is_node)
		aligned_positions = np.r_[node_cols, L]
		kept_before = np.r_[0, np.cumsum(kept)]
		reference_positions = kept_before[aligned_positions]
		assert np.all(np.diff(reference_positions) > 0)
		N = aligned_positions.size
		src = np.searchsorted(aligned_positions, begin)
		tgt = np.searchsorted(aligned_positions, end)
		assert np.array_equal(aligned_positions[src], begin) and np.array_equal(aligned_positions[tgt], end) and np.all(tgt > src)
		csum = np.r_[0, np.cumsum(np.bincount(src, minlength=N))]
		label_offsets = np.r_[0, np.cumsum(label_len)]
		ref = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, size=int(kept_before[-1]))]
		label_bytes = np.frombuffer(b"acgt", np.uint8)[rng.integers(0, 4, size=int(label_offsets[-1]))]

		n_copies = len(copies)
		ep, hp = max(64, (E + 63) // 64 * 64), max(64, (n_copies + 63) // 64 * 64)
		bits = np.zeros((hp, ep), dtype=bool)
		for c, edges in enumerate(copies):
			if len(edges):
				bits[c, np.asarray(edges, dtype=np.int64)] = True
		assert not bits[:, E:].any()
		words = np.packbits(bits, axis=1, bitorder="little").view("<u8").reshape(-1).copy()
		g = oracle.graph_from_arrays(reference_positions, aligned_positions, tgt, csum, label_offsets, label_bytes.tobytes(), words, ep, hp, ["S"], [0, n_copies])
		g.ref = ref.tobytes()
		return SeamGraph(name, g, kept, ref, begin, end, label_offsets, label_len, label_bytes, src, tgt, [np.sort(np.asarray(c, dtype=np.int64)) for c in copies])


class SeamGraph:
	def __init__(self, name, g, kept, ref, begin, end, label_offsets, label_len, label_bytes, src, tgt, copies):
		self.name, self.g, self.kept, self.ref = name, g, kept, ref
		self.begin, self.end, self.label_offsets, self.label_len, self.label_bytes, self.src, self.tgt = begin, end, label_offsets, label_len, label_bytes, src, tgt
		self.copies = copies
		self.length = kept.size
		self.n_edges = begin.size
		self.ref_row = np.full(self.length, GAP, dtype=np.uint8)
		self.ref_row[kept] = ref
		self._aligned, self._oracle, self._bits, self._assembled = {}, {}, {}, {}
		self.notes = {}          # what a graph's maker wants its tests to know: tiles, edges, windows by name

	@property
	def rows(self):
		"""REF and every copy."""
		return [PLOIDY_MAX] + list(range(len(self.copies)))

	# -- the model ---------------------------------------------------------------------------------------------------------------------
	# A row is an int (a chromosome copy, or PLOIDY_MAX for REF) or a list of (cut node, copy) pairs, as Context.splice_rows takes them.
	@staticmethod
	def row_key(row):
		return int(row) if isinstance(row, (int, np.integer)) else tuple((int(node), int(copy)) for node, copy in row)

	def copy_bits(self, copy):
		"""Copy `copy`'s path bits, one bool per edge."""
		if copy not in self._bits:
			b = np.zeros(self.n_edges, dtype=bool)
			b[self.copies[copy]] = True
			self._bits[copy] = b
		return self._bits[copy]

	def assembled(self, row):
		"""The bit column of a row: a copy's own bits; for a row with cuts, per edge the bit of the copy in force at the edge's source node
		(the copy of the last cut at or before that node; PLOIDY_MAX, which sets nothing, before the first cut)."""
		key = self.row_key(row)
		if isinstance(key, int):
			return np.zeros(self.n_edges, dtype=bool) if key == PLOIDY_MAX else self.copy_bits(key)
		if key not in self._assembled:
			bits = np.zeros(self.n_edges, dtype=bool)
			k, copy = 0, PLOIDY_MAX
			for e, node in enumerate(self.src.tolist()):
				while k < len(key) and key[k][0] <= node:
					copy = key[k][1]
					k += 1
				if copy != PLOIDY_MAX:
					bits[e] = self.copy_bits(copy)[e]
			self._assembled[key] = bits
		return self._assembled[key]

	def effective(self, row):
		"""The model's walk: of the row's set edges, in order, those that begin at or after the node the walk stands on."""
		out, cur = [], 0
		for e in np.flatnonzero(self.assembled(row)).tolist():
			if self.src[e] >= cur:
				out.append(e)
				cur = self.tgt[e]
		return out

	def aligned(self, row):
		"""The row's aligned columns (kept per row: the callers slice it many times)."""
		key = self.row_key(row)
		if key not in self._aligned:
			self._aligned[key] = self._aligned_uncached(row)
		return self._aligned[key]

	def _aligned_uncached(self, row):
		a = self.ref_row.copy()
		for e in self.effective(row):
			b, n = int(self.begin[e]), int(self.label_len[e])
			a[b:int(self.end[e])] = GAP
			a[b:b + n] = self.label_bytes[int(self.label_offsets[e]):int(self.label_offsets[e]) + n]
		return a

	def body(self, row, unaligned=False, window=None):
		a = self.aligned(row)
		if window is not None:
			a = a[window[0]:window[1]]
		return (a[a != GAP] if unaligned else a).tobytes()

	def oracle_body(self, row, unaligned=False, window=None):
		"""The oracle's row; a window of it is cut from its aligned row (a column window is defined on aligned columns)."""
		key = (self.row_key(row), bool(unaligned and window is None))
		if key not in self._oracle:
			if isinstance(key[0], int):
				self._oracle[key] = self.g.output_sequence(self.g.ref, copy_index=key[0], unaligned=key[1])
			else:
				self._oracle[key] = self.g.output_sequence(self.g.ref, cuts=list(key[0]), unaligned=key[1])
		if window is None:
			return self._oracle[key]
		a = np.frombuffer(self._oracle[key], dtype=np.uint8)[window[0]:window[1]]
		return (a[a != GAP] if unaligned else a).tobytes()

	# -- cuts ------------------------------------------------------------------------------------------------------------------------------
	def first_edge_of_node(self, node):
		"""The host's h_csum[node]: the first edge that begins at `node` or after it."""
		return int(np.searchsorted(self.src, node, side="left"))

	def is_bridge(self, node):
		"""No edge jumps over the node: every edge that begins before it ends at or before it (where v2m_splice_rows lets a row cut)."""
		first = self.first_edge_of_node(node)
		return 0 == first or int(self.tgt[:first].max()) <= node


# ---- the census: what the kernels see ------------------------------------------------------------------------------------------------

class TileTables:
	"""Per tile of the whole row or of a column window, by the kernels' definitions (kernels.hpp: tile_tables, load_patch_cache): tile t is
	columns [base + t * kTileBytes, ...) clipped to the end; its range = the edges that begin in it; its crossing edges = those with
	begin < tile base < end; the label base = the label offset of the range's first edge."""

	def __init__(self, sg, window=None):
		K = kernel_constants()
		T = K.kTileBytes
		b, e = window if window is not None else (0, sg.length)
		self.col_begin, self.col_end = b, e
		self.n_tiles = max(1, (e - b + T - 1) // T)
		self.base = b + np.arange(self.n_tiles + 1, dtype=np.int64) * T
		self.tile_end = np.minimum(self.base[1:], e)
		self.edge_begin = np.searchsorted(sg.begin, np.minimum(self.base, e), side="left")
		self.range_begin = self.edge_begin[:-1]
		self.n_range = np.diff(self.edge_begin)
		self.cross = [[] for _ in range(self.n_tiles)]
		first = np.where(sg.begin < b, 0, (sg.begin - b) // T + 1)            # first tile whose base lies after the edge's begin
		last = np.minimum((sg.end - 1 - b) // T, self.n_tiles - 1)           # last tile whose base lies before the edge's end
		for ed in np.flatnonzero(last >= first).tolist():
			for t in range(int(first[ed]), int(last[ed]) + 1):
				assert sg.begin[ed] < self.base[t] < sg.end[ed]
				self.cross[t].append(ed)
		self.n_cross = np.array([len(c) for c in self.cross], dtype=np.int64)

	def tile_of(self, column):
		return (column - self.col_begin) // kernel_constants().kTileBytes

	def label_end_in_slice(self, sg, t):
		"""label_begin - label_base + label_len of the cached candidates of tile t (the first kCandLds of its range)."""
		K = kernel_constants()
		r0, n = int(self.range_begin[t]), int(min(self.n_range[t], K.kCandLds))
		base = sg.label_offsets[r0] if n else 0
		return sg.label_offsets[r0:r0 + n] - base + sg.label_len[r0:r0 + n]

	def clipped(self, sg, e, t):
		return int(min(sg.end[e], self.tile_end[t]) - max(sg.begin[e], self.base[t]))


class RowCensus:
	"""One row of the whole graph or of a window, as the unaligned kernels cut it: per tile the surviving bytes, the destination offset, the
	short chunks (1 ... 15 surviving bytes) of each 1-KiB slot, how many leading slots fit the workgroup's queue (the later ones are packed
	in place: "dense"); per chunk its keep-mask, destination phase and route; per tile the effective patches longer than kLongPatch."""

	def __init__(self, sg, row, tables):
		K = kernel_constants()
		T = K.kTileBytes
		tt = tables
		a = sg.aligned(row)[tt.col_begin:tt.col_end]
		kept = np.zeros(tt.n_tiles * T, dtype=bool)         # past the end: padding (the template holds zeros there)
		kept[:a.size] = a != GAP
		chunks = kept.reshape(-1, 16)
		self.count = chunks.sum(axis=1)
		self.mask = np.packbits(chunks, axis=1, bitorder="little").view("<u2").reshape(-1)
		self.short = (self.count >= 1) & (self.count <= 15)
		before = np.r_[0, np.cumsum(self.count)]
		self.phase = before[:-1] & 15                       # destination address mod 16 (rows are a multiple of 16 apart)
		self.length = int(before[-1])
		self.tile_offset = before[:-1:K.kTileChunks]
		self.tile_bytes = self.count.reshape(tt.n_tiles, -1).sum(axis=1)
		self.slot_short = self.short.reshape(tt.n_tiles, K.kSlots, 64).sum(axis=2)
		self.tile_short = self.slot_short.sum(axis=1)
		self.n_fit = (np.cumsum(self.slot_short, axis=1) <= K.kQueue).sum(axis=1)      # the kernel's ballot: a prefix of the slots
		self.queued = self.short & np.repeat(np.arange(K.kSlots)[None, :] < self.n_fit[:, None], 64, axis=1).reshape(-1)
		self.dense = self.short & ~self.queued
		self.n_long = np.zeros(tt.n_tiles, dtype=np.int64)
		self.effective = sg.effective(row)
		for e in self.effective:
			if sg.end[e] <= tt.col_begin or sg.begin[e] >= tt.col_end:
				continue
			for t in range(max(0, int(tt.tile_of(sg.begin[e]))), min(tt.n_tiles - 1, int(tt.tile_of(sg.end[e] - 1))) + 1):
				self.n_long[t] += tt.clipped(sg, e, t) > K.kLongPatch


class SegmentCensus:
	"""One row as assemble_row_bits_kernel sees it.  The segment table is the one prepare_rows (csrc/v2m_hip.hip) builds: a row without cuts is
	one segment (edge 0, its copy); a row with cuts has one segment per cut, (the first edge at or after the cut node, the cut's copy), and a
	leading (edge 0, PLOIDY_MAX) one unless its first cut is node 0.  Segment s covers the edges from its first edge to the next segment's;
	the last one goes on to the end.  The kernel puts words [word_base, n_words) together, one wave per 64 of them from word_base on.

	spans        per wave span (first word, segments that begin on its first edge, segments the lane loop walks, rounds of the lane loop):
	             the walk begins at the last segment whose first edge is <= the span's first edge and ends before the first segment that
	             begins at or after the span's end; 64 segments per round
	masks        {(from, to)}: per (segment, word) the first bit of the word in the segment and one past the last, REF segments left out
	mask_at      {(segment, word): (from, to)}
	writers      per word the number of segments that OR bits into it
	empty        the segments that hold no edge (their first edge is the next segment's too)
	ref          the PLOIDY_MAX segments"""

	def __init__(self, sg, row, word_base=0, n_words=None):
		key = sg.row_key(row)
		if isinstance(key, int):
			table = [(0, key)]
		else:
			table = [] if key[0][0] == 0 else [(0, PLOIDY_MAX)]
			table += [(sg.first_edge_of_node(node), copy) for node, copy in key]
		self.seg_begin = np.array([b for b, _ in table], dtype=np.int64)
		self.seg_copy = [c for _, c in table]
		assert np.all(np.diff(self.seg_begin) >= 0) and 0 == self.seg_begin[0]
		n_seg = len(table)
		self.n_words = n_words = (sg.n_edges + 63) // 64 if n_words is None else n_words
		self.word_base = word_base
		seg_end = np.r_[self.seg_begin[1:], np.iinfo(np.int64).max]
		self.empty = [s for s in range(n_seg) if seg_end[s] == self.seg_begin[s]]
		self.ref = [s for s in range(n_seg) if self.seg_copy[s] == PLOIDY_MAX]
		self.spans = []
		for w0 in range(word_base, n_words, 64):
			e_lo, e_hi = 64 * w0, 64 * min(w0 + 64, n_words)
			first = int(np.flatnonzero(self.seg_begin <= e_lo)[-1])
			walked = int(np.count_nonzero(self.seg_begin[first:] < e_hi))
			self.spans.append((w0, int(np.count_nonzero(self.seg_begin == e_lo)), walked, (walked + 63) // 64))
		self.masks, self.mask_at, self.writers = set(), {}, np.zeros(n_words, dtype=np.int64)
		lo_edge, hi_edge = 64 * word_base, 64 * n_words
		for s in range(n_seg):
			b, e = max(int(self.seg_begin[s]), lo_edge), min(int(seg_end[s]), hi_edge)
			if b >= e or self.seg_copy[s] == PLOIDY_MAX:
				continue
			for w in range(b >> 6, ((e - 1) >> 6) + 1):
				ft = (max(b - 64 * w, 0), min(e - 64 * w, 64))
				if ft != (0, 64):                   # (whole words are counted, not listed: a long segment has thousands)
					self.mask_at[(s, w)] = ft
				self.masks.add(ft)
			self.writers[b >> 6:((e - 1) >> 6) + 1] += 1

	def neighbours(self):
		"""(cut edge, copy before, copy after) at every change from a segment that holds edges to the next one that does."""
		held = [s for s in range(len(self.seg_copy)) if s not in self.empty]
		return [(int(self.seg_begin[t]), self.seg_copy[s], self.seg_copy[t]) for s, t in zip(held, held[1:])]


def window_words(sg, col_begin, col_end):
	"""(restart, lo, hi) of a column window, by the host's rule (csrc/v2m_hip.hip: first_edge_reaching_past, words_of_edges): the edges from
	the first one whose span, or an earlier edge's, reaches past col_begin to the last one that begins before col_end; lo and hi are
	their words, restart the last word at or before lo whose first edge is not overlappable.  (0, 0, 0): no edge reaches the window."""
	e_hi = int(np.searchsorted(sg.begin, col_end, side="left"))
	reach = np.maximum.accumulate(sg.end[:e_hi]) if e_hi else np.zeros(0, dtype=np.int64)
	e_lo = int(np.searchsorted(reach, col_begin, side="right"))
	if e_lo >= e_hi:
		return 0, 0, 0
	furthest = np.r_[0, np.maximum.accumulate(sg.tgt)][:-1]
	overlappable = sg.src < furthest
	lo = restart = e_lo // 64
	while restart > 0 and overlappable[64 * restart]:
		restart -= 1
	return restart, lo, (e_hi + 63) // 64


def mask_phase_coverage(censuses):
	"""(queued, dense): bool [65536][16], which (keep-mask, destination phase) pairs reach pack_chunk_and_store_exact by either route."""
	queued, dense = np.zeros((65536, 16), dtype=bool), np.zeros((65536, 16), dtype=bool)
	for c in censuses:
		queued[c.mask[c.queued], c.phase[c.queued]] = True
		dense[c.mask[c.dense], c.phase[c.dense]] = True
	return queued, dense


def packable_masks():
	"""The keep-masks the pack sees: 1 ... 15 surviving bytes (an empty chunk writes nothing, a full one is one 16-byte store)."""
	n = np.array([bin(m).count("1") for m in range(65536)])
	return (n >= 1) & (n <= 15)


# ---- group a: every chunk mask ---------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def mask_graph(full_after, rotate=0):
	"""One leading interval (1 reference byte, 15 padding columns) with 15 ALT edges node 0 -> node 1 whose labels are 2 ... 16 bytes, then
	every 16-bit keep-mask as one 16-column chunk, in the order (m + rotate) mod 65536, each followed by `full_after` chunks without padding;
	one full chunk closes the row.  Copy c (0 ... 14) takes edge c, copy 15 takes nothing: with REF the rows begin at all 16 phases."""
	b = Builder(1000 + full_after)
	b.add_ref(1, 15)
	order = (np.arange(65536, dtype=np.int64) + rotate) & 0xFFFF
	cols = ((order[:, None] >> np.arange(16)) & 1).astype(bool)
	cols = np.concatenate([cols, np.ones((65536, 16 * full_after), dtype=bool)], axis=1).reshape(-1)
	b.add_kept(cols)
	b.add_ref(16)
	first_node = 16 + int(np.argmax(cols))              # where the leading interval ends: the first kept column after it
	for n in range(2, 17):
		b.edge(0, first_node, n)
	sg = b.finish([[c] for c in range(15)] + [[]], "masks_s%d_r%d" % (full_after, rotate))
	K = kernel_constants()
	T = K.kTileBytes
	sg.notes["windows"] = [
		("16_not_tile", 5 * T + 16 * 37, 9 * T + 16 * 37 + 16 * 11),      # first column a multiple of 16, not of the tile
		("odd", 3 * T + 4099, 8 * T + 4099),                              # every chunk of the window straddles two of the row's
		("ends_mid_chunk", 2 * T, 6 * T + 16 * 5 + 7),
	]
	return sg


def mask_rows(rows_per_group):
	"""REF, the 15 phase copies, the copy with no bit set; repeated to 2 x rows-per-group + 1 rows (a full group, a full group, a ragged one)."""
	base = [PLOIDY_MAX] + list(range(16))
	return [base[i % len(base)] for i in range(max(len(base), 2 * rows_per_group + 1))]


# ---- group b: short-chunk counts per row tile -------------------------------------------------------------------------------------------

def _tile_with_short_chunks(positions):
	"""A tile's columns with a short chunk (k kept bytes, then padding; k cycles through 1 ... 15) at each of the chunk positions."""
	K = kernel_constants()
	kept = np.ones(K.kTileBytes, dtype=bool)
	for i, p in enumerate(positions):
		kept[16 * p + 1 + i % 15:16 * p + 16] = False
	return kept


@functools.lru_cache(maxsize=None)
def short_count_graph():
	K = kernel_constants()
	T, Q, S, C = K.kTileBytes, K.kQueue, K.kSlots, K.kTileChunks
	assert Q + 1 <= 3 * 64 and Q >= 65
	plan = [
		("none", []),
		("one_first", [0]),
		("one_last", [C - 1]),
		("63", list(range(63))),
		("64_slot_end", list(range(64))),                              # the whole first slot
		("65", list(range(65))),
		("either_side", [63, 64, 127, 128]),                           # the last chunk of a slot and the first of the next
		("q_minus_1", list(range(Q - 1))),
		("q", list(range(Q))),
		("q_plus_1", list(range(Q + 1))),                               # the slot that holds chunk Q is the first that does not fit; the later ones hold none
		("q_over_all_slots", [64 * s + j for s in range(S) for j in range(Q // S)]),    # Q short chunks, the last slot completes them
		("later_slots_dense", [64 * s + j for s in range(S) for j in range(Q // 4 - 2)]),   # the fifth slot is the first that does not fit, every later one holds more
		("q_last_chunks", list(range(C - Q, C))),
		("deleted_before", []),
		("deleted", list(range(0, C, 9))),                              # all padding in copy 0
		("deleted_after", [5, 70]),
		("tail", [1, 2, 3]),
	]
	b = Builder(2000)
	names = [p[0] for p in plan]
	for _, positions in plan:
		b.add_kept(_tile_with_short_chunks(positions))
	b.add_ref(16 * 3 + 5)                                                # a ragged last tile
	t = names.index("deleted")
	# copy 0: a deletion from the last chunk of the tile before to the third chunk of the tile after: the tile between is all padding
	deletion = b.edge(t * T - 16, (t + 1) * T + 32, 1)
	sg = b.finish([[deletion], []], "short_counts")
	sg.notes["tiles"] = {n: i for i, n in enumerate(names)}
	sg.notes["plan"] = dict(plan)
	sg.notes["windows"] = [
		("empty_in_copy_0", t * T + 100, t * T + 5000),                  # inside the deletion: copy 0's unaligned body is empty
		("from_deleted_tile", t * T + 48, (t + 2) * T - 3),
		("counts_shifted", 3 * T + 16 * 3, 12 * T + 16 * 3),
	]
	return sg


# ---- group c: the patch cache -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cache_graph():
	"""A tile per limit of the workgroup's patch cache.  notes["tiles"][name] = the tile; notes["edges"][name] = edge indices."""
	K = kernel_constants()
	T = K.kTileBytes
	b = Builder(3000)
	tiles, edges, copies = {}, {}, {k: [] for k in range(12)}

	def next_tile(name):
		b.ref_to((b.length + T - 1) // T * T if b.length else 0)
		tiles[name] = b.length // T
		return b.length

	def fillers_until(residue):
		"""Sites in the current tile until the number of edges is `residue` mod 64 (at least two); returns the last one's edge."""
		n = (residue - b.n_edges - 2) % 64 + 2
		return b.add_sites(n, 3, 2, 3) + n - 1

	next_tile("start")
	b.add_ref(40)

	# n_range at kCandLds - 1 / kCandLds / kCandLds + 1, the range beginning at bit 0 / 1 / 63 of an effective-edge word; sites of 2 columns whose
	# label fills both (the unaligned rows grow by a byte per edge taken)
	for which, (n, bit) in enumerate(((K.kCandLds - 1, 0), (K.kCandLds, 1), (K.kCandLds + 1, 63))):
		next_tile("before_range_%d" % which)
		b.add_ref(30)
		before = fillers_until(bit)
		base = next_tile("range_%d" % which)
		b.add_ref(7)
		first = b.add_sites(n, 2, 1, 2)
		assert b.length < base + T and b.n_edges == first + n and first % 64 == bit
		b.add_ref(5)
		next_tile("after_range_%d" % which)
		after = b.add_sites(3, 4, 1, 2)
		edges["range_%d" % which] = (before, first, n, after)
		copies[0] += [first, after + 2]                                  # candidate 0
		copies[1] += [first + K.kCandLds - 2]                            # the last candidate all three ranges cache
		copies[2] += [before, first + n - 1, after]                      # just before the range, its last candidate (cached end - 1, the cached end, one past it), just after
		copies[3] += [before, first, first + K.kCandLds - 2, first + n - 1, after]
		if n > K.kCandLds:
			copies[1] += [first + K.kCandLds]                            # the first candidate past the cache
			copies[4] += [first + K.kCandLds - 1, first + K.kCandLds]
		else:
			copies[4] += [first + n - 2]

	# n_cross + n_range at kCandDeltaLds - 1 / kCandDeltaLds / kCandDeltaLds + 1: nested long deletions that begin in the tile before and all end in this
	# one, then more sites than the cache holds
	n_range = K.kCandLds + 88
	for which, total in enumerate((K.kCandDeltaLds - 1, K.kCandDeltaLds, K.kCandDeltaLds + 1)):
		n_cross = total - n_range
		assert 0 < n_cross and 3 * n_cross + 3 * n_range + 200 < T
		base = next_tile("before_delta_%d" % which)
		b.add_ref(100)
		first_cross = b.n_edges
		for i in range(n_cross):                                             # begins ascend, ends descend: nested
			b.edge(base + 100 + 2 * i, base + T + 10 + 2 * (n_cross - i), 1)
		assert next_tile("delta_%d" % which) == base + T
		b.add_ref(10 + 2 * n_cross + 30)
		first = b.add_sites(n_range, 3, 2, 3)
		b.add_ref(9)
		edges["delta_%d" % which] = (first_cross, n_cross, first, n_range)
		copies[0] += [first_cross, first + n_range - 1]                      # the first of the crossing list; the last candidate of all
		copies[1] += [first_cross + n_cross - 1, first + n_range - 2]       # the last of the crossing list; the candidate before the last
		copies[2] += [first_cross + n_cross // 2, first, first + n_range - 1]
		copies[3] += [first + n_range - 2, first + n_range - 1]
		copies[4] += [first_cross + 1, first_cross + 2, first + K.kCandLds - 1, first + K.kCandLds]   # the second blocks the third: one crossing edge is effective

	# the cached label slice: a label that ends at byte kLabelLds - 1 / kLabelLds / kLabelLds + 1 of the tile's slice, an empty label at that offset, the edge after
	for which, end_at in enumerate((K.kLabelLds - 1, K.kLabelLds, K.kLabelLds + 1)):
		next_tile("label_%d" % which)
		b.add_ref(20)
		e0, = b.add_site([end_at - 10], end_at - 10)                         # an insertion: one reference byte, the label fills the interval
		b.add_ref(3)
		e1, = b.add_site([10], 12, 2)
		b.add_ref(3)
		e2, = b.add_site([0], 5, 5)                                          # an empty label: five reference bytes become padding
		b.add_ref(3)
		e3, = b.add_site([3], 3, 3)
		b.add_ref(3)
		edges["label_%d" % which] = (e0, e1, e2, e3)
		copies[5] += [e0, e1, e2, e3]
		copies[6] += [e1, e3]
		copies[7] += [e0, e2]

	# spans of 0xFFFE / 0xFFFF / 0x10000 columns for an edge that begins in the tile (each crosses into the next three or four tiles)
	for which, span in enumerate((0xFFFE, 0xFFFF, 0x10000)):
		base = next_tile("span_%d" % which)
		b.add_ref(1000 + which)
		e0, = b.add_site([7], span, span)                                    # every column kept in REF; the edge leaves 7 bytes and padding
		b.add_ref(11)
		e1, = b.add_site([2], 2, 1)
		edges["span_%d" % which] = (e0, e1)
		copies[5] += [e0, e1]
		copies[6] += [e1]
		copies[8] += [e0]

	# patches of exactly kLongPatch and kLongPatch + 1 columns: whole, and clipped to that by the tile's end
	base = next_tile("long_patch")
	b.add_ref(50)
	p0, = b.add_site([K.kLongPatch - 6], K.kLongPatch)
	b.add_ref(5)
	p1, = b.add_site([K.kLongPatch - 6], K.kLongPatch + 1)
	b.ref_to(base + T - K.kLongPatch)
	p2, = b.add_site([2 * K.kLongPatch - 1], 2 * K.kLongPatch)              # kLongPatch columns in this tile, as many in the next: its label goes on there
	base = next_tile("long_patch_clipped")
	b.ref_to(base + T - K.kLongPatch - 1)
	p3, = b.add_site([2 * K.kLongPatch + 1], 2 * K.kLongPatch + 1)          # kLongPatch + 1 columns here
	edges["long_patch"] = (p0, p1, p2, p3)
	copies[5] += [p0, p1, p2, p3]
	copies[6] += [p0, p2]
	copies[7] += [p1, p3]

	# kLongQueueLds - 1 / kLongQueueLds / kLongQueueLds + 1 long patches effective in one (row, tile), in consecutive rows
	base = next_tile("long_queue")
	b.add_ref(64)
	first = b.add_sites(K.kLongQueueLds + 1, 2 * K.kLongPatch, 3, 2 * K.kLongPatch - 9)
	b.add_ref(5)
	edges["long_queue"] = (first, K.kLongQueueLds + 1)
	copies[9] += list(range(first, first + K.kLongQueueLds - 1))
	copies[10] += list(range(first, first + K.kLongQueueLds))
	copies[11] += list(range(first, first + K.kLongQueueLds + 1))

	# an edge that begins on the last column of a tile (its label goes on in the next); one that ends exactly on a tile boundary
	base = next_tile("last_column")
	b.ref_to(base + T - 1)
	q0, = b.add_site([30], 40)
	b.add_ref(5)
	base = next_tile("ends_on_boundary")
	b.ref_to(base + T - 50)
	q1, = b.add_site([20], 50, 4)
	assert b.length == base + T
	tiles["after_boundary"] = b.length // T
	b.add_ref(100)
	q2, = b.add_site([1], 1)
	b.add_ref(333)
	edges["tile_edges"] = (q0, q1, q2)
	copies[5] += [q0, q1, q2]
	copies[9] += [q0]
	copies[10] += [q1]

	sg = b.finish([sorted(copies[k]) for k in sorted(copies)], "cache_limits")
	sg.notes["tiles"], sg.notes["edges"] = tiles, edges
	limit_tiles = [t for n, t in tiles.items() if not n.startswith(("start", "before_range", "after_", "before_delta"))]
	windows = []
	for n, t in sorted(tiles.items(), key=lambda x: x[1]):
		if t in limit_tiles:
			end = min(sg.length, (t + 1) * T + 3000)
			windows += [(n + "_inside", t * T + 4321, end), (n + "_at", t * T, end), (n + "_after", t * T + 1, end)]
	sg.notes["windows"] = windows
	return sg


def cache_rows(n):
	"""n rows over REF and the cache graph's copies such that consecutive rows differ in every limit (the long queue's rows side by side)."""
	base = [PLOIDY_MAX, 9, 10, 11, 0, 1, 2, 3, 4, 5, 6, 7, 8]
	return [base[i % len(base)] for i in range(n)]


# ---- group d: tile geometry -------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def geometry_graph(length):
	"""`length` aligned columns with a handful of edges: substitutions, insertions and deletions spread over the row, one deletion across
	every sixth tile boundary.  Copy 0 takes the even edges, copy 1 the odd ones."""
	K = kernel_constants()
	T = K.kTileBytes
	b = Builder(4000 + length % 9973)
	b.add_ref(3)
	spots = sorted(set([length * i // 8 for i in range(1, 8)] + [t * T - 20 for t in range(1, length // T + 1, 6)]))
	n = 0
	for s in spots:
		if s < b.length + 2 or s + 60 > length:
			continue
		b.ref_to(s)
		kind = n % 3
		if kind == 0:
			b.add_site([1], 1)
		elif kind == 1:
			b.add_site([9], 9)
		else:
			b.add_site([1], 40, 40)
		b.add_ref(1)
		n += 1
	b.ref_to(length)
	return b.finish([list(range(0, b.n_edges, 2)), list(range(1, b.n_edges, 2))], "geometry_%d" % length)


def geometry_lengths():
	K = kernel_constants()
	T = K.kTileBytes
	out = [k * T + d for k in (1, 5) for d in (-1, 0, 1, 15, 16, 17)]
	out += [n * T - 5 for n in (63, 64, 65, 71, 72)]            # tile counts around the default run of 64 tiles; 72 - 64 = a last run of 8
	return out


# ---- group e: resolve -------------------------------------------------------------------------------------------------------------------

RESOLVE_BACK_WORDS = 2          # the V2M_MAX_BACK_WORDS the resolve graphs are laid out for


@functools.lru_cache(maxsize=None)
def resolve_graph(tail_edges):
	"""A chain of two-column sites, one edge each (edge i = site i), in which some edges are stretched over the sites after them, which makes
	those sites' edges overlappable.  tail_edges in {0, 1, 63}: the edge count mod 64.
	A blocker always precedes the edge it blocks (edges are ordered by source node), so the pairs at a word boundary are: blocker = bit 63 of
	word k - 1 and blocked = bit 0 of word k; and blocker = bit 0, blocked = bit 63 of one word.  k: 1, kResolveWordsPerThread, 256 (a thread's
	next word), 256 x kResolveWordsPerThread (the next workgroup's piece)."""
	K = kernel_constants()
	bw = RESOLVE_BACK_WORDS
	piece = 256 * K.kResolveWordsPerThread
	n = 64 * (piece + 4) + tail_edges
	stretch = {}                                                   # edge -> the last site it covers
	pairs = []
	for k in (1, K.kResolveWordsPerThread, 256, piece):
		stretch[64 * k - 1] = 64 * k
		pairs.append((64 * k - 1, 64 * k))
	for w in (3, piece + 2):
		stretch[64 * w] = 64 * w + 63
		pairs.append((64 * w, 64 * w + 63))
	# a deletion at bit 0 of word 16 over the sites of the next bw + 1 words and a few more: from a set edge in word 16 + bw the restart point
	# (the deletion: the nearest earlier edge no other can skip) lies bw words back, from one in word 16 + bw + 1, bw + 1 words back
	deletion = 64 * 16
	stretch[deletion] = deletion + 64 * (bw + 1) + 40
	under = (deletion + 64 * bw + 5, deletion + 64 * (bw + 1) + 5)
	b = Builder(5000 + tail_edges)
	b.add_ref(2)
	b.add_kept(np.tile(np.array([True, False]), n))
	b.add_ref(6)
	for i in range(n):
		b.edge(2 + 2 * i, 2 + 2 * (stretch.get(i, i) + 1), 1 + (i & 1))
	copies = [
		[x for p in pairs for x in p] + [deletion, under[0]],      # every blocker with its blocked edge
		[p[1] for p in pairs] + [under[0], under[1]],               # the blocked edges alone: effective
		[deletion, under[1], n - 1],
		[p[0] for p in pairs] + [deletion + 1, under[0], n - 1],
		list(range(deletion - 3, deletion + 64 * (bw + 2), 7)) + [n - 1],
		list(range(0, n, 5)),
	]
	sg = b.finish(copies, "resolve_%d" % tail_edges)
	sg.notes.update(pairs=pairs, deletion=deletion, under=under, back_words=bw)
	return sg


# ---- group f: founder rows: assemble_row_bits_kernel, and resolve on assembled rows -------------------------------------------------------

ASSEMBLE_GAPS = (64 * 10 + 17, 64 * 64, 64 * 256)        # an ordinary edge, a wave span's first edge, a workgroup's first edge
ASSEMBLE_PAIRS = ((0, 1), (2, 3), (4, 5))                # complementary copies: all-one / all-zero, even / odd edges, a random half / the rest
ASSEMBLE_WINDOW_WORDS = (1, 63, 64, 65, 257)             # wr.lo of the column windows


@functools.lru_cache(maxsize=None)
def assemble_graph(tail_edges, label_len=1):
	"""A chain of one-column sites with one edge each (edge i = site i; the label is one byte, which is never the reference's: acgt against
	ACGT).  No edge overlaps another and every node is a bridge, so the effective edges are the assembled bits and aligned column
	begin[i] shows bit i: every bit assemble_row_bits_kernel writes is visible.  64 x (256 + 64 + 3) + tail_edges edges: a workgroup's
	four wave spans, one more wave span, a short last one.  The sites of ASSEMBLE_GAPS follow a reference byte without an edge: the edge
	before ends on that byte's node, the site has its own, both can be cut and both have the same first edge.
	label_len = 0: the same graph with empty labels.  A set bit is then a deleted reference byte, which the row's alignment ops show (a
	one-byte substitution leaves them one M run whatever the bits are); nodes, edges, copies and so the cut rows are the same."""
	n = 64 * (256 + 64 + 3) + tail_edges
	b = Builder(6000 + tail_edges)
	at = 0
	for g in ASSEMBLE_GAPS:
		b.add_sites(g - at, 1, 1, label_len)
		b.add_ref(1)
		at = g
	b.add_sites(n - at, 1, 1, label_len)
	b.add_ref(40)
	every = np.arange(n)
	half = np.sort(np.random.default_rng(6100 + tail_edges).choice(n, size=n // 2, replace=False))
	copies = [every, [], every[0::2], every[1::2], half, np.setdiff1d(every, half)]
	sg = b.finish(copies, "assemble_%d%s" % (tail_edges, "" if label_len else "_deletions"))
	assert sg.n_edges == n
	return sg


def cut_row(sg, segments):
	"""[(where, copy)] -> [(cut node, copy)].  where: the segment's first edge (the cut is at the edge's own node; n_edges: at the node
	the last edge ends on), or ("gap", e): the node before edge e's, which must hold no edge (so the segment is empty)."""
	out = []
	for where, copy in segments:
		if isinstance(where, tuple):
			node = int(sg.src[where[1]]) - 1
			assert "gap" == where[0] and sg.first_edge_of_node(node) == where[1] and not np.any(sg.src == node)
		else:
			node = int(sg.tgt[-1]) if where == sg.n_edges else int(sg.src[where])
			assert sg.first_edge_of_node(node) == where
		assert sg.is_bridge(node) and (not out or node > out[-1][0]), (where, node)
		out.append((node, copy))
	return out


def _alternate(edges, pair, first=0):
	return [(e, pair[(i + first) & 1]) for i, e in enumerate(edges)]


def _differing(sg, copy, edge, among):
	"""The copy of `among` whose bit at `edge` is not `copy`'s."""
	return next(c for c in among if sg.copy_bits(c)[edge] != sg.copy_bits(copy)[edge])


@functools.lru_cache(maxsize=None)
def assemble_rows(tail_edges):
	"""{name: row} for the whole-row cases; the first letter of a name is its class (the issue's letters a - f)."""
	sg = assemble_graph(tail_edges)
	n, R = sg.n_edges, PLOIDY_MAX
	seg = {}
	# a. cuts either side of a word's first and last edge, for words at the limits of a wave span and of a workgroup
	edges = sorted({0} | {64 * k + d for k in (1, 63, 64, 65, 255, 256, 257) for d in (-1, 0, 1, 63)})
	for i, pair in enumerate(ASSEMBLE_PAIRS):
		seg["a_word_edges_%d%d" % pair] = _alternate(edges, pair, i)
	# b. segment lengths against the spans
	seg["b_word_span_65"] = _alternate([0, 64 * 20, 64 * 21, 64 * 100, 64 * 165, 64 * 192, 64 * 256], (4, 5))   # one word; 65 words across word 128; the span [192, 256)
	seg["b_across_workgroups"] = _alternate([0, 64 * 250 + 7, 64 * 262 + 9], (2, 3))
	seg["b_two_long_01"] = _alternate([0, 64 * 260 + 13], (0, 1))
	seg["b_two_long_45"] = _alternate([0, 64 * 260 + 13], (5, 4))
	# c. runs of one-edge segments under one wave span: 64 / 65 / 66 / 129 / 130 segments for the lane loop to walk
	for name, first, count, pair in (("c_63", 64 * 3 + 1, 63, (0, 1)), ("c_64", 64 * 3, 64, (4, 5)), ("c_65_01", 64 * 70, 65, (0, 1)), ("c_65_45", 64 * 70, 65, (4, 5)),
			("c_128", 64 * 130 + 3, 128, (2, 3)), ("c_129", 64 * 200 + 60, 129, (4, 5))):
		seg[name] = _alternate([0] + list(range(first, first + count)), pair)
	# d. REF segments beside the all-one copy (copy 0: a REF segment read as a copy would show too): before the first cut, one bit, one word, up to a wave span's first edge, the last segment
	seg["d_ref"] = [(64 * 5 + 2, 0), (64 * 30 + 7, R), (64 * 30 + 8, 0), (64 * 40, R), (64 * 41, 0), (64 * 120 + 5, R), (64 * 128, 0), (64 * 300 + 1, R)]
	seg["d_first_cut_late"] = [(64 * 63 + 9, 0)]
	# e. last segments
	seg["e_last_edge_45"] = [(0, 4), (n - 1, 5)]
	seg["e_last_edge_01"] = [(0, 0), (n - 1, 1)]
	seg["e_last_edge_10"] = [(0, 1), (n - 1, 0)]
	seg["e_past_every_edge_45"] = [(0, 4), (64 * 322 + 1, 5), (n, 4)]
	seg["e_past_every_edge_10"] = [(0, 1), (n, 0)]
	seg["e_past_every_edge_01"] = [(0, 0), (n, 1)]
	# f. empty segments: two cuts with one first edge; the second one's copy holds from there, the first one's differs from it at that edge
	for name, pair, others in (("f_empty_45", (4, 5), (0, 1)), ("f_empty_10", (1, 0), (4, 5))):
		s = [(0, pair[0])]
		for i, g in enumerate(ASSEMBLE_GAPS):
			winner = pair[(i + 1) & 1]
			s += [(("gap", g), _differing(sg, winner, g, others)), (g, winner)]
		seg[name] = s
	return {name: cut_row(sg, s) for name, s in seg.items()}


@functools.lru_cache(maxsize=None)
def assemble_windows(tail_edges):
	"""[(name, first column, end column, {name: row})]: windows whose first edge word is k, for k in ASSEMBLE_WINDOW_WORDS, each with cuts
	against the wave spans as the window shifts them (first words k + 64 j): either side of the first and of the second span's first
	edge, and 65 one-edge segments under the second span; and a window no edge reaches."""
	sg = assemble_graph(tail_edges)
	out = []
	for k in ASSEMBLE_WINDOW_WORDS:
		last = 64 * (k + 130) + 9
		end = int(sg.begin[last]) + 1 if last < sg.n_edges else sg.length - 10
		second = 64 * (k + 64)
		edges = [0, 64 * k - 30, 64 * k - 1, 64 * k, 64 * k + 1, second - 1, second, second + 1] + list(range(second + 3, second + 3 + 65))
		rows = {"h_w%d_%d%d" % ((k,) + pair): cut_row(sg, _alternate(edges, pair, k)) for pair in ((4, 5), (0, 1))}
		out.append(("lo_%d" % k, int(sg.begin[64 * k + 5]), end, rows))
	rows = {"h_none_45": out[0][3]["h_w1_45"], "h_none_past": assemble_rows(tail_edges)["e_past_every_edge_45"]}
	out.append(("no_edge", sg.length - 30, sg.length - 2, rows))
	return out


@functools.lru_cache(maxsize=None)
def resolve_cut_rows(tail_edges):
	"""{name: row} on resolve_graph(tail_edges): rows that switch copy at the source node of every blocker of notes["pairs"] and at the node
	right after its blocked edge, at the deletion's source node and at the first bridge after its end.  `inside` names the copy between
	such a pair of cuts, `outside` the copy elsewhere (the first segment's).  Copy 0 sets every blocker with its blocked edge, the
	deletion and the edge bw words under it; 1 the blocked edges and both edges under the deletion, not the deletion; 2 the deletion and
	the edge bw + 1 words under it, no pair's edge; 3 the blockers alone; 4 every seventh edge around the deletion; 5 every fifth edge."""
	sg = resolve_graph(tail_edges)
	d = sg.notes["deletion"]
	after = int(sg.tgt[d])
	while not sg.is_bridge(after):
		after += 1
	places = sorted([(int(sg.src[p]), int(sg.tgt[q])) for p, q in sg.notes["pairs"]] + [(int(sg.src[d]), after)])
	rows = {}
	for name, outside, inside in (("both_inside", 2, 0), ("both_outside", 0, 2), ("blocked_alone_inside", 0, 1), ("blocked_alone_outside", 1, 0),
			("blockers_inside", 5, 3), ("sevenths_inside", 1, 4)):
		row = [(0, outside)]
		for begin, end in places:
			assert sg.is_bridge(begin) and sg.is_bridge(end) and row[-1][0] < begin < end
			row += [(begin, inside), (end, outside)]
		rows[name] = row
	return rows


def resolve_cut_windows(tail_edges):
	"""A window that begins under the deletion (restart == lo: the deletion is its word's first edge and nothing reaches over it), and one
	that begins on the column the blocked edge at bit 0 of word kResolveWordsPerThread ends on: the first edge that reaches into it is bit
	1 of that word, whose first edge is overlappable, so the words assembled begin a word before the words resolved (restart < lo)."""
	sg = resolve_graph(tail_edges)
	under = sg.notes["under"]
	q = 64 * kernel_constants().kResolveWordsPerThread
	assert (q - 1, q) in sg.notes["pairs"]
	return [("under_deletion", int(sg.begin[under[0]]) - 30, int(sg.begin[under[1]]) + 9), ("after_blocked_bit_0", int(sg.end[q]), int(sg.end[q]) + 3000)]
