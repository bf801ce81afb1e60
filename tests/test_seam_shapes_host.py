"""tests/transpose_shapes.py without a GPU: its plain transpose against the oracle's naive one, and what its shape lists claim to reach,
recomputed with the host's own rules (launch_transpose_lines, restated in transpose_shapes.lines_geometry): a later edit that thins a list
fails here, not silently on the GPU."""

import os
import re

import numpy as np
import pytest

import oracle
import transpose_shapes as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- transpose_ref ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("SW,DW", [(1, 1), (1, 2), (2, 1), (3, 5), (9, 33), (17, 95), (5, 16), (16, 17), (1, 79), (33, 3), (2, 31), (7, 64)])
def test_transpose_ref_is_the_oracles_naive_transpose(SW, DW):
	rows, cols = 64 * SW, 64 * DW
	src = T.source(SW, DW)
	want = oracle.transpose_matrix(src, rows, cols, naive=True)
	assert np.array_equal(T.transpose_ref(src, rows, cols), want)
	assert np.array_equal(T.transpose_ref(T.transpose_ref(src, rows, cols), cols, rows), src)


@pytest.mark.parametrize("SW,DW,SP,DP", [(1, 1, 16, 16), (3, 5, 16, 0), (3, 5, 0, 16), (9, 33, 16, 48), (17, 21, 32, 32), (2, 17, 3, 18), (17, 95, 32, 0), (1, 40, 0, 48)])
def test_transpose_ref_with_pitches(SW, DW, SP, DP):
	"""Column by column against the dense result: the data words of every destination column are the dense column, the pad words keep
	the fill, and the source's pad words change nothing."""
	rows, cols = 64 * SW, 64 * DW
	dense = T.source(SW, DW)
	want = oracle.transpose_matrix(dense, rows, cols, naive=True).reshape(rows, DW)
	sp, dp = SP or SW, DP or DW
	for pad in (None, 0, 0xFFFFFFFFFFFFFFFF):
		src = T.source(SW, DW, SP, pad=pad)                                     # pad words: random, zeros, ones
		src.reshape(cols, sp)[:, :SW] = dense.reshape(cols, SW)
		got = T.transpose_ref(src, rows, cols, SP, DP, fill=0x1122334455667788).reshape(rows, dp)
		for r in range(rows):
			assert np.array_equal(got[r, :DW], want[r]), (r, pad)
		assert (got[:, DW:] == 0x1122334455667788).all()


def test_source_words_have_both_values_in_both_halves():
	w = T.source(3, 17)
	lo, hi = w & np.uint64(0xFFFFFFFF), w >> np.uint64(32)
	assert (lo != 0).all() and (hi != 0).all() and (lo != 0xFFFFFFFF).all() and (hi != 0xFFFFFFFF).all()
	assert 0 < int((w >> np.uint64(63)).sum()) < w.size


# ---- launch_transpose_lines, restated -----------------------------------------------------------------------------------------------------------

def test_lines_geometry_follows_the_launch_code():
	"""The restated rules name what csrc/v2m_hip.hip says: the merge condition and the two span rules, literally."""
	with open(os.path.join(ROOT, "vcf2multialign_amd", "csrc", "v2m_hip.hip")) as f:
		text = f.read()
	assert "if (kMayMerge && 1 == NS && NB <= 8 && DP == DW && DW >= 16 && 0 != DP % 16)" in text
	assert "u64 const P((SW + kTsR - 1) / kTsR), NB((DW + 15) / 16);" in text
	assert "while (span_blocks > 4 && P * ((NB + span_blocks - 1) / span_blocks) < 1024) span_blocks /= 2;" in text
	assert "max_spans(std::max<u64>(1, std::min<u64>(NB / 4, 4 * n_cus / std::max<u64>(1, P) + 1)))" in text
	assert re.search(r'"lines16"\).*\n(.*\n){3}\s*return launch_transpose_lines<8, 4, 16, 32, true>', text)
	assert "if (8 == V) return launch_transpose_lines<8, 4, 8, 32, true>" in text
	assert "if (SW * DW * 512 < (u64(32) << 20))" in text
	assert re.search(r'kTransposeCandidates\[\] = \{%s\}' % ", ".join('"%s"' % c for c in T.F_CANDIDATES), text)
	# a few values by hand
	assert (1, 2, 2, 1, False) == T.lines_geometry("lines8:1", 1, 21)
	assert (1, 2, 1, 400, True) == T.lines_geometry("lines8:400", 3, 21)
	assert (3, 2, 1, 4, True) == T.lines_geometry("lines8", 17, 21)
	assert (2, 8, 2, 4, False) == T.lines_geometry("lines16", 17, 127)             # the host cuts 8 blocks into two spans
	assert (2, 7, 1, 7, True) == T.lines_geometry("lines16", 17, 111)
	assert not T.lines_geometry("lines16:400", 17, 21, DP=32)[4]                     # a line-aligned destination never merges
	assert ("lines8", 2, ["/sf"]) == T.parse_kernel("lines8:2/sf") and ("8x8", 0, ["/rr"]) == T.parse_kernel("8x8/rr")


# ---- the lists ------------------------------------------------------------------------------------------------------------------------------------

def test_group_a_reaches_every_phase_at_each_block_count():
	n = 0
	for q in T.A_WHOLE_BLOCKS:
		widths = T.a_widths(q)
		assert {DW // 16 for DW in widths} == {q}
		assert {DW % 16 for DW in widths} == set(range(16)) - ({0} if 0 == q else set())
		n += len(widths)
		for kernel in T.A_KERNELS:
			if kernel.startswith("lines"):
				K = T.parse_kernel(kernel)[1]
				for SW in T.A_HEIGHTS:
					for DW in widths:
						P, NB, NS, span_blocks, merged = T.lines_geometry(kernel, SW, DW)
						assert span_blocks == K and NS == (NB + K - 1) // K and NB == q + (DW % 16 != 0)
	assert 63 == n
	# spans: with q = 5 (5 or 6 blocks) spans of 1, 2 and 3 blocks give a backward span between two forward ones, a forward last span, a
	# backward last span, and a last span of one partial block; q = 1 and 2 give one and two spans
	assert {T.lines_geometry("lines8:%d" % K, 1, 16 * 5 + 3)[2] for K in (1, 2, 3)} == {6, 3, 2}
	assert {T.lines_geometry("lines8:%d" % K, 1, 80)[2] for K in (1, 2, 3)} == {5, 3, 2}
	# heights: one ragged panel, whole panels and a ragged one, for both geometries
	assert [T.lines_geometry("lines8:1", SW, 17)[0] for SW in T.A_HEIGHTS] == [1, 1, 3]
	assert [T.lines_geometry("lines16:1", SW, 17)[0] for SW in T.A_HEIGHTS] == [1, 1, 2]
	assert max(SW * DW * 512 for SW in T.A_HEIGHTS for q in T.A_WHOLE_BLOCKS for DW in T.a_widths(q)) <= 830 * 1000


def test_group_b_reaches_every_merged_width_and_no_other():
	rule = [DW for DW in range(1, 200) if T.merges(1, (DW + 15) // 16, DW, DW)]
	assert rule == T.B_WIDTHS and 105 == len(rule)
	for nb in range(2, 9):
		assert {DW % 16 for DW in T.B_WIDTHS if (DW + 15) // 16 == nb} == set(range(1, 16))
	for SW in T.B_HEIGHTS:
		for kernel in ("lines8:400", "lines16:400"):
			assert all(T.lines_geometry(kernel, SW, DW)[4] for DW in T.B_WIDTHS)
			assert not any(T.lines_geometry(kernel, SW, DW)[4] for DW in T.B_BOUNDARY_WIDTHS)
		# the spans the host chooses: one span and merged up to 4 blocks (lines8) / 7 blocks (lines16), two unmerged spans above
		assert [DW for DW in T.B_WIDTHS if T.lines_geometry("lines8", SW, DW)[4]] == [DW for DW in T.B_WIDTHS if DW < 64]
		assert [DW for DW in T.B_WIDTHS if T.lines_geometry("lines16", SW, DW)[4]] == [DW for DW in T.B_WIDTHS if DW < 112]
		assert {T.lines_geometry(k, SW, DW)[2] for k in ("lines8", "lines16") for DW in T.B_WIDTHS} == {1, 2}
	# the boundary widths: one word and one block either side of every clause of the rule
	assert not T.merges(1, 1, 15, 15) and not T.merges(1, 1, 16, 16) and not T.merges(1, 4, 64, 64) and not T.merges(1, 8, 128, 128)
	assert not T.merges(1, 9, 129, 129) and not T.merges(1, 9, 144, 144) and T.merges(1, 8, 127, 127) and T.merges(1, 2, 17, 17)
	assert max(SW * DW * 512 for SW in T.B_HEIGHTS for DW in T.B_WIDTHS) == 17 * 127 * 512


def test_group_c_fills_the_last_panel_in_every_way():
	for tsr in (8, 16):
		assert {SW % tsr for SW in T.C_HEIGHTS} == set(range(tsr))
		assert {(SW + tsr - 1) // tsr for SW in T.C_HEIGHTS} >= {1, 2, 3}
	(w_merged, k_merged), (w_spans, k_spans) = T.C_CASES
	for SW in T.C_HEIGHTS:
		assert all(T.lines_geometry(k, SW, w_merged)[4] for k in k_merged if k.startswith("lines"))
		assert all((3, False) == T.lines_geometry(k, SW, w_spans)[2::2] for k in k_spans if k.startswith("lines"))
	for _, kernels in T.C_CASES:
		assert {T.parse_kernel(k)[0] for k in kernels} == {"8x8", "stream16", "lines8", "lines16"}


def test_group_d_reaches_every_item_count_mod_8():
	for kernel in T.D_LINES_KERNELS:
		counts = [T.items(kernel, *T.d_lines_shape(n)) for n in T.D_ITEMS]
		assert counts == T.D_ITEMS and {c % 8 for c in counts} == set(range(8)) and min(counts) < 8 < max(counts)
		assert {T.d_lines_shape(n)[1] % 16 for n in T.D_ITEMS} == {13}
	for kernel in ("8x8", "stream16"):
		counts = [T.items(kernel, *T.d_panel_shape(kernel, g)) for g in T.D_PANEL_GRIDS]
		assert counts == [p * q for p, q in T.D_PANEL_GRIDS]
		assert {c % 8 for c in counts} == set(range(8)) and min(counts) < 8 < max(counts)
		assert set(counts) <= set(T.D_ITEMS)
	assert set(T.D_SUFFIXES) == {"", "/rr", "/pf", "/sf"}


def test_group_e_pitches():
	"""The library's path matrix has a pitch of the path words rounded up to 16: all but k = 16 leave pad words; a part of the copies
	is sent with a source pitch above its word count."""
	pitch = lambda words: (words + 15) // 16 * 16
	assert [pitch((T.e_edges(k) + 63) // 64) for k in T.E_PATH_WORDS] == [16, 16, 16, 32, 48]
	assert [(T.e_edges(k) + 63) // 64 for k in T.E_PATH_WORDS] == list(T.E_PATH_WORDS)
	assert [(c + 63) // 64 for c in T.E_COPIES] == [1, 3, 17]
	for c in T.E_COPIES:
		part = c - T.E_SLICE_FIRST - T.E_SLICE_LEFT_OUT
		assert part > 0 and part % 8 and pitch((part + 63) // 64) > (part + 63) // 64 == (c + 63) // 64
	assert {T.parse_kernel(k)[0] for k in T.E_KERNELS} == {"8x8", "stream16", "lines8", "lines16"}


def test_group_f_is_just_over_the_calibration_threshold():
	SW, DW = T.F_SHAPE
	assert 32 << 20 <= SW * DW * 512 < 35 << 20 and 3 == DW % 16 and 17 == (DW + 15) // 16 and 1 == SW % 16
	assert SW * DW * 512 < 1.02 * (32 << 20)                                        # (256 x 256 words are the threshold itself)
