"""A model of v2m_splice_window_set_distinct (include/v2m_hip.h, "distinct pieces of a window set") and the corpus its GPU tests run.

The model takes the expected pieces from test_gpu_window.py's column-tracking walk (walk_rows / window_bodies) and groups them with a plain
dictionary loop: class_of, the per-window class bodies, the class counts and the order and arguments of the sink calls.  piece_key is the
key hash_pieces_kernel gives a piece: the checksum of v2m_checksum_rows_device, spelled out with Python integers.

The corpus (cases()) is shared by tests/test_gpu_distinct.py, which runs it on the GPU, and tests/test_distinct_model_host.py, which
asserts on the CPU that it reaches what it is meant to reach."""

import os

import numpy as np

import synth
from test_gpu_window import FIXTURES, PLOIDY_MAX, TILE, _fixture_graph, walk_rows, window_bodies, window_classes
from test_gpu_window_sets import _many_case, _seam_case, back_to_back, founder_rows, many_short_windows, model_layout, seam_windows, tile_seam_windows

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
KERNELS_HPP = os.path.join(ROOT, "vcf2multialign_amd", "csrc", "kernels.hpp")
M64 = 2 ** 64 - 1
GOLDEN = 0x9E3779B97F4A7C15
SMALL_RING = 1 << 18
TABLE_BYTES_PER_PIECE = 40      # v2m_hip.hip, distinct_run: what a piece takes in device tables, counted against the slot


def kernel_constants():
	"""kDistinctChunkBytes and kDistinctLongBytes as csrc/kernels.hpp defines them."""
	import re
	with open(KERNELS_HPP) as f:
		text = f.read()
	out = {}
	for name in ("kDistinctChunkBytes", "kDistinctLongBytes"):
		found = re.findall(r"^constexpr\s+u32\s+%s\s*=\s*(\d+)\s*;" % name, text, re.M)
		assert len(found) == 1, name
		out[name] = int(found[0])
	return out


def mix64(z):
	z &= M64
	z ^= z >> 30
	z = z * 0xBF58476D1CE4E5B9 & M64
	z ^= z >> 27
	z = z * 0x94D049BB133111EB & M64
	return z ^ z >> 31


def piece_key(body):
	"""The key of a piece: its zero-padded little-endian 8-byte words w, sum of mix64((w + 1) * golden ^ word), plus mix64(length)."""
	body = bytes(body)
	acc = mix64(len(body))
	padded = body + b"\0" * (-len(body) % 8)
	for w in range(len(padded) // 8):
		acc += mix64((w + 1) * GOLDEN & M64 ^ int.from_bytes(padded[8 * w:8 * w + 8], "little"))
	return acc & M64


def classes_of(expected):
	"""expected[r][k] = the bytes of piece (r, k).  Returns (class_of [n_rows, n_windows] uint32, bodies[k] = the class bodies of window k
	in class order, first_rows[k], calls = [(window, class index, first row, body)] in the order the sink is called)."""
	n_rows = len(expected)
	n_windows = len(expected[0]) if n_rows else 0
	class_of = np.zeros((n_rows, n_windows), dtype=np.uint32)
	bodies, first_rows, seen = [[] for _ in range(n_windows)], [[] for _ in range(n_windows)], [{} for _ in range(n_windows)]
	calls = []
	for r, pieces in enumerate(expected):
		for k, body in enumerate(pieces):
			c = seen[k].get(body)
			if c is None:
				c = seen[k][body] = len(bodies[k])
				bodies[k].append(body)
				first_rows[k].append(r)
				calls.append((k, c, r, body))
			class_of[r, k] = c
	return class_of, bodies, first_rows, calls


class Case:
	"""One input of the corpus: a graph, the distinct rows (kinds), which kind row i of the batch is, the windows, and the environment
	the call runs under.  expected(unaligned) is the pieces of every batch row."""

	def __init__(self, name, g, kinds, windows, kind_of_row=None, env=None):
		self.name, self.g, self.kinds, self.env = name, g, kinds, dict(env or {})
		self.windows = [(int(w[-2]), int(w[-1])) for w in windows]
		self.kind_of_row = list(range(len(kinds))) if kind_of_row is None else list(kind_of_row)
		self.rows = [kinds[k] for k in self.kind_of_row]
		self._walked = None

	@property
	def walked(self):
		if self._walked is None:
			self._walked = walk_rows(self.g, self.kinds)
		return self._walked

	def expected(self, unaligned):
		per_kind = [[window_bodies(w, b, e)[1 if unaligned else 0] for b, e in self.windows] for w in self.walked]
		return [per_kind[k] for k in self.kind_of_row]


def _all_rows(g):
	return [PLOIDY_MAX] + list(range(g.total_chromosome_copies))


def length_windows(g):
	"""Windows of every length at which a kernel takes another path: around 8 and 16 (the masked word, the 16-byte chunk), around the
	chunk of a long piece and around the short / long threshold -- as window lengths (the aligned pieces), and again as windows in which
	the REF row emits that many bytes (unaligned pieces end inside a chunk of the window's)."""
	K = kernel_constants()
	chunk, long_bytes = K["kDistinctChunkBytes"], K["kDistinctLongBytes"]
	L = int(g.aligned_positions[-1])
	wins = back_to_back(100, [1, 7, 8, 9, 15, 16, 17], L)
	emitted = np.concatenate([[0], np.cumsum(column_positions(g) >= 0)])      # REF bytes before column c
	for i, n in enumerate([chunk - 1, chunk, chunk + 1, 2 * chunk + 1, long_bytes - 8, long_bytes, long_bytes + 8]):
		begin = 300 + 977 * i
		assert begin + n <= L
		wins.append((begin, begin + n))
		end = int(np.searchsorted(emitted, emitted[begin] + n, side="left"))
		assert end <= L and emitted[end] - emitted[begin] == n
		wins.append((begin, end))
	return wins


def column_positions(g):
	"""ref_pos_of[c] = the reference position whose byte the REF row holds in column c, or -1 for the REF row's padding."""
	rp, ap = np.asarray(g.reference_positions, dtype=np.int64), np.asarray(g.aligned_positions, dtype=np.int64)
	out = np.full(int(ap[-1]), -1, dtype=np.int64)
	for n in range(len(rp) - 1):
		k = int(rp[n + 1] - rp[n])
		out[ap[n]:ap[n] + k] = np.arange(rp[n], rp[n + 1])
	return out


def crafted_case(tmp_path):
	"""The seam graph with a literal '-' in the reference at a base one row deletes, and windows found in the walks: one that is padding in
	every row (all pieces empty when unaligned), one in which two rows are equal while they differ within 15 columns after its end, and
	the column of the literal '-' (two rows' aligned pieces are equal, '-' and padding, their unaligned pieces are not)."""
	g = _seam_case(tmp_path)
	kinds = [PLOIDY_MAX] + list(range(6))
	walked = walk_rows(g, kinds)
	pads = np.array([pad for _, pad in walked])
	ref_pos_of = column_positions(g)
	deleted = np.nonzero(~pads[0] & pads[1:].any(axis=0) & (ref_pos_of >= 0))[0]
	assert deleted.size, "no row deletes a reference base"
	dash_col = int(deleted[len(deleted) // 2])
	ref = bytearray(g.ref)
	ref[int(ref_pos_of[dash_col])] = ord("-")
	g.ref = bytes(ref)
	walked = walk_rows(g, kinds)
	rows = np.array([np.frombuffer(r, dtype=np.uint8) for r, _ in walked])
	L = rows.shape[1]
	special = {"dash": (dash_col, dash_col + 1)}
	all_pad = np.logical_and.reduce(pads, axis=0)
	cols = np.nonzero(all_pad)[0]
	assert cols.size, "no column is padding in every row"
	c = int(cols[0])
	e = c
	while e < L and all_pad[e]:
		e += 1
	special["all_empty"] = (c, e)
	for r in range(1, len(kinds)):
		diff = np.nonzero(rows[0] != rows[r])[0]
		gaps = np.nonzero(np.diff(diff) > 40)[0]
		if gaps.size:
			d = int(diff[gaps[0] + 1])              # the first difference after more than 40 equal columns
			special["differ_after"] = (d - 25, d - 6)   # equal inside, different in the 6th column after the end
			special["differ_after_rows"] = (0, r)
			break
	assert "differ_after" in special
	wins = [special["dash"], special["all_empty"], special["differ_after"]] + seam_windows(g)[:20] + [(0, 64), (L - 70, L)]
	case = Case("crafted", g, kinds, wins)
	case._walked = walked
	case.special = special
	return case


def small_case(tmp_path):
	"""At most 24 rows and 40 windows, for V2M_DISTINCT_HASH_BITS = 0, 1, 3: every key of a window collides."""
	g = _seam_case(tmp_path)
	L = int(g.aligned_positions[-1])
	kinds = _all_rows(g)[:8]
	kind_of_row = [i % len(kinds) for i in range(21)]
	wins = seam_windows(g)[:30] + [(200, 1200), (L // 2, L // 2 + 3000), (L - 900, L), (40, 41)]
	return Case("small", g, kinds, wins, kind_of_row=kind_of_row)


def small_ring_case(tmp_path):
	"""V2M_RING_SLOT_BYTES = 256 KiB with 45 rows of ~21 KB records: a handful of rows a slice, classes span slices."""
	g = _seam_case(tmp_path)
	kinds = _all_rows(g)
	kind_of_row = [i % 6 for i in range(20)] + [i % len(kinds) for i in range(25)]     # (classes that begin in a later slice, too)
	wins = [(1000, 1000 + TILE + 5)] + seam_windows(g) + [(30000, 33000)]
	return Case("small_ring", g, kinds, wins, kind_of_row=kind_of_row, env={"V2M_RING_SLOT_BYTES": str(SMALL_RING)})


def rows_per_slice(case, slot_bytes):
	"""The rows of a slice as distinct_run plans them."""
	_, pitch, _ = model_layout(case.windows)
	return max(1, min(len(case.rows), slot_bytes // (pitch + TABLE_BYTES_PER_PIECE * len(case.windows))))


def fixture_case(stem, fasta):
	g = _fixture_graph(stem, fasta)
	return Case("fixture_" + stem, g, _all_rows(g), window_classes(g, np.random.default_rng(1)))


def seam_case(tmp_path):
	g = _seam_case(tmp_path)
	return Case("slot_seams", g, _all_rows(g), seam_windows(g))


def tile_seam_case(tmp_path):
	g = synth.with_random_paths(synth.build_case(tmp_path, 31, 90000, 4000, 4, multi_allelic=0.2, long_every=40), 3, 0.3)
	return Case("tile_seams", g, _all_rows(g), tile_seam_windows(int(g.aligned_positions[-1])))


def many_short_case(tmp_path):
	g, rows = _many_case(tmp_path)                       # (the REF row, every copy and two founder rows with cuts)
	return Case("many_short", g, rows, many_short_windows(int(g.aligned_positions[-1]), n=700))


def many_rows_case(tmp_path):
	g, kinds = _many_case(tmp_path)
	L = int(g.aligned_positions[-1])
	return Case("many_rows", g, kinds, seam_windows(g)[:25] + many_short_windows(L, n=120, seed=9) + [(500, 9500)], kind_of_row=[i % len(kinds) for i in range(311)])


def founder_case(tmp_path):
	g = synth.with_random_paths(synth.build_case(tmp_path, 31, 90000, 4000, 6, multi_allelic=0.2, long_every=40), 3, 0.3)
	rng = np.random.default_rng(4)
	rows = [PLOIDY_MAX] + list(range(4)) + founder_rows(g, rng, (5, 40, 400)) + founder_rows(g, np.random.default_rng(4), (5,))
	return Case("founders", g, rows, window_classes(g, rng, n_random=4))


def lengths_case(tmp_path):
	g = _seam_case(tmp_path)
	return Case("lengths", g, _all_rows(g), length_windows(g))


CASE_BUILDERS = [seam_case, tile_seam_case, many_short_case, many_rows_case, founder_case, lengths_case, crafted_case, small_case, small_ring_case]


def cases(tmp_path):
	"""Every case of the corpus, the reference fixtures first."""
	out = [fixture_case(stem, fasta) for stem, fasta in FIXTURES]
	for i, build in enumerate(CASE_BUILDERS):
		d = tmp_path / ("case_%d" % i)
		d.mkdir()
		out.append(build(d))
	return out
