"""A plain transpose with column pitches, the source generator and the shape lists of tests/test_gpu_transpose_seams.py.  TEST
INFRASTRUCTURE ONLY; no GPU.

transpose_ref() is numpy's unpackbits / packbits around a transposition: the source's columns to bits, the bit matrix turned, the
destination's columns packed again.  tests/test_seam_shapes_host.py holds it equal to the oracle's naive transpose (dense form, and
column by column where there are pitches) and asserts by computation what the lists below claim to reach, with the host's own rules for
the whole-line kernel (lines_geometry() restates launch_transpose_lines of csrc/v2m_hip.hip: P panels, NB blocks of 16 words, NS spans,
merged column ends or not).

Shapes are (SW, DW): the source's words per column (n_rows / 64) and the destination's (n_cols / 64).  The destination column r begins
at word r * DW of a dense destination, so its 128-byte lines begin at its words s_r, s_r + 16, ... with s_r = (-r * DW) mod 16: DW mod 16
is the phase step from one column to the next."""

import numpy as np

GUARD_WORDS = 4096
GUARD = 0x5A5A5A5A5A5A5A5A
MI355X_CUS = 256


# ---- the reference -----------------------------------------------------------------------------------------------------------------------

def transpose_ref(src_words, n_rows, n_cols, src_pitch=0, dst_pitch=0, fill=GUARD):
	"""src_words: n_cols columns of src_pitch words (0 = dense: n_rows / 64), the first n_rows / 64 of each are the column's bits, bit i
	of word w = row 64 w + i.  Returns n_rows columns of dst_pitch words (0 = dense: n_cols / 64) with the transposed bits; the words
	between a column's n_cols / 64 words and its pitch hold `fill`."""
	assert 0 == n_rows % 64 and 0 == n_cols % 64
	SW, DW = n_rows // 64, n_cols // 64
	SP, DP = src_pitch or SW, dst_pitch or DW
	assert SP >= SW and DP >= DW
	src = np.ascontiguousarray(src_words, dtype="<u8")
	assert src.size == n_cols * SP, (src.size, n_cols, SP)
	out = np.full((n_rows, DP), fill, dtype=np.uint64)
	if SW and DW:
		bits = np.unpackbits(src.view(np.uint8).reshape(n_cols, SP * 8)[:, :SW * 8], axis=1, bitorder="little")         # [source column, source row]
		out[:, :DW] = np.packbits(np.ascontiguousarray(bits.T), axis=1, bitorder="little").view("<u8")                    # [source row, word of the destination column]
	return out.reshape(-1)


def random_words(rng, n):
	"""The generator of test_transpose_random: two random words and-ed together (a quarter of the bits set in the low 63), bit 63 set at
	random -- every word has both values in both halves."""
	w = rng.integers(0, 2 ** 63, size=n, dtype=np.uint64) & rng.integers(0, 2 ** 63, size=n, dtype=np.uint64)
	w |= rng.integers(0, 2, size=n, dtype=np.uint64) << np.uint64(63)
	return w


def source(SW, DW, src_pitch=0, pad=None):
	"""A (SW x DW words) source, dense or with a column pitch; `pad` fills the words between a column's SW words and its pitch (default:
	random words as well: nothing may depend on them)."""
	SP = src_pitch or SW
	rng = np.random.default_rng([SW, DW, SP])
	w = random_words(rng, DW * 64 * SP)
	if pad is not None and SP > SW:
		w.reshape(DW * 64, SP)[:, SW:] = pad
	return w


# ---- launch_transpose_lines, restated -------------------------------------------------------------------------------------------------------

def parse_kernel(name):
	"""'lines16:2/sf' -> ('lines16', 2, ['/sf']); K = 0 where the name gives none."""
	suffixes = []
	while len(name) > 3 and name[-3:] in ("/rr", "/pf", "/sf"):
		suffixes.insert(0, name[-3:])
		name = name[:-3]
	family, _, k = name.partition(":")
	return family, int(k) if k else 0, suffixes


def lines_geometry(kernel, SW, DW, SP=0, DP=0, n_cus=MI355X_CUS):
	"""(P, NB, NS, span_blocks, merged) of a lines8 / lines16 launch, as launch_transpose_lines computes them."""
	family, span_blocks, _ = parse_kernel(kernel)
	kTsR = {"lines8": 8, "lines16": 16}[family]
	SP, DP = SP or SW, DP or DW
	P, NB = (SW + kTsR - 1) // kTsR, (DW + 15) // 16
	if 0 == span_blocks and 16 == kTsR:
		max_spans = max(1, min(NB // 4, 4 * n_cus // max(1, P) + 1))
		best = -1.0
		for ns in range(1, max_spans + 1):
			k = (NB + ns - 1) // ns
			wgs = P * ((NB + k - 1) // k)
			score = wgs / ((wgs + n_cus - 1) // n_cus * n_cus) * k / (k + 1)
			if score > best * 1.005:
				best, span_blocks = score, k
	if 0 == span_blocks:
		if NB <= 32 and P >= 1024:
			span_blocks = NB
		else:
			span_blocks = 32
			while span_blocks > 4 and P * ((NB + span_blocks - 1) // span_blocks) < 1024:
				span_blocks //= 2
	NS = (NB + span_blocks - 1) // span_blocks
	return P, NB, NS, span_blocks, merges(NS, NB, DW, DP)


def merges(NS, NB, DW, DP):
	"""The host's rule for the merged column ends (kMerge)."""
	return 1 == NS and NB <= 8 and DP == DW and DW >= 16 and 0 != DP % 16


def items(kernel, SW, DW):
	"""Work items (workgroups with work) of a launch: panels x spans, or panels x panels."""
	family = parse_kernel(kernel)[0]
	if family in ("8x8", "stream16"):
		t = 8 if "8x8" == family else 16
		return ((SW + t - 1) // t) * ((DW + t - 1) // t)
	P, _, NS, _, _ = lines_geometry(kernel, SW, DW)
	return P * NS


# ---- the lists ------------------------------------------------------------------------------------------------------------------------------

# A. phase x span seam: q whole blocks and r words more, every r; heights = one ragged panel, and one or two whole panels plus a ragged
# one for both geometries (8 and 16 row-words); spans of 1, 2 and 3 blocks (forwards, backwards, forwards) and the two panel kernels
A_WHOLE_BLOCKS = (0, 1, 2, 5)
A_HEIGHTS = (1, 3, 17)
A_KERNELS = ("lines8:1", "lines8:2", "lines8:3", "lines16:1", "lines16:2", "lines16:3", "8x8", "stream16")


def a_widths(q):
	return [16 * q + r for r in range(16) if 16 * q + r >= 1]


# B. merged column ends: every width the host's rule accepts (one span, at most 8 blocks, dense, DW >= 16, not a multiple of 16), whole
# columns asked for (:400) and with the spans the host chooses, and the widths either side of the rule
B_WIDTHS = [DW for DW in range(17, 128) if DW % 16]
B_BOUNDARY_WIDTHS = (15, 16, 64, 128, 129, 144)
B_HEIGHTS = (1, 9, 17)
B_KERNELS = ("lines8:400", "lines16:400", "lines8", "lines16")

# C. ragged source panels: every fill of the last panel of both geometries (the clamped source row-word, rw_ok)
C_HEIGHTS = list(range(1, 34))
C_CASES = ((21, ("8x8", "stream16", "lines8", "lines16")), (37, ("8x8", "stream16", "lines8:1", "lines16:1")))

# D. item order: n items (SW = 1, spans of one block) in the eight XCD chunks, in plain order, with either dimension fastest
D_ITEMS = list(range(1, 18))
D_SUFFIXES = ("", "/rr", "/pf", "/sf")
D_LINES_KERNELS = ("lines8:1", "lines16:1")
D_PANEL_GRIDS = ((1, 1), (1, 3), (2, 2), (1, 7), (2, 3), (1, 8), (3, 3), (2, 5), (1, 13), (1, 17))   # (row panels, column panels) of 8x8 and stream16


def d_lines_shape(n):
	return 1, 16 * n - 3


def d_panel_shape(kernel, grid):
	t = 8 if "8x8" == kernel else 16
	return t * (grid[0] - 1) + 1, t * grid[1] - 3


# E. pitch forms: 64 k - 5 edges (k path words: pitch 16, 16, 16, 32 and 48), copies that pad to 1, 3 and 17 words
E_PATH_WORDS = (1, 15, 16, 17, 33)
E_COPIES = (59, 190, 1085)
E_KERNELS = ("8x8", "stream16", "lines8:1", "lines8:2/sf", "lines8:400", "lines16", "lines16:1", "lines16:2")
E_SLICE_FIRST, E_SLICE_LEFT_OUT = 8, 16


def e_edges(k):
	return 64 * k - 5


# F. calibration: just over launch_transpose's 32 MiB threshold, phase 3, 17 blocks
F_SHAPE = (257, 259)
F_CANDIDATES = ("8x8", "stream16", "lines8", "lines16")
