"""The distinct-pieces model on the CPU (tests/distinct_model.py): its key against the checksum helper, its grouping on a hand-made
table, and reach assertions on the corpus tests/test_gpu_distinct.py runs -- a corpus that exercises nothing must not pass.  Also the
new symbol's prototype and the CLI's refusal of --distinct without --regions-file, which needs no device."""

import os
import subprocess

import numpy as np
import pytest

import distinct_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
	return M.cases(tmp_path_factory.mktemp("distinct"))


def test_key_is_the_checksum_of_the_header():
	import vcf2multialign_amd as v2m
	rng = np.random.default_rng(3)
	rows = [b"ACGT-ACGTACG", b"", b"A" * 8, b"ACGTACGTT"]          # test_host_cpu.py's reference rows
	rows += [bytes(rng.integers(0, 256, size=n, dtype=np.uint8)) for n in (1, 7, 8, 9, 15, 16, 17, 4097)]
	assert [M.piece_key(r) for r in rows] == v2m.checksum_rows_host(rows).tolist()
	assert M.piece_key(b"") == M.mix64(0) and M.piece_key(b"A") != M.piece_key(b"A\0")     # the length is part of the key


def test_constants_are_the_kernels():
	from vcf2multialign_amd import _native as N
	K = M.kernel_constants()
	assert (N.DISTINCT_CHUNK_BYTES, N.DISTINCT_LONG_BYTES) == (K["kDistinctChunkBytes"], K["kDistinctLongBytes"])
	assert N.DISTINCT_CHUNK_BYTES % 16 == 0 and N.DISTINCT_LONG_BYTES >= N.DISTINCT_CHUNK_BYTES
	assert (N.KERNEL_DISTINCT_HASH, N.KERNEL_DISTINCT_GATHER, N.KERNEL_DISTINCT_VERIFY) == (12, 13, 14) and len(N.KERNEL_NAMES) == 15
	header = open(os.path.join(ROOT, "include", "v2m_hip.h")).read()
	assert "V2M_KERNEL_DISTINCT_HASH = 12" in header and "V2M_KERNEL_DISTINCT_VERIFY = 14" in header and "V2M_KERNEL_END = 15" in header
	with open(os.path.join(ROOT, "vcf2multialign_amd", "csrc", "v2m_hip.hip")) as f:
		assert ("%d * W" % M.TABLE_BYTES_PER_PIECE) in f.read()


def test_grouping_on_a_hand_made_table():
	expected = [[b"AA", b"", b"x"], [b"AB", b"", b"x"], [b"AA", b"-", b"x"], [b"AC", b"", b"x"], [b"AB", b"-", b"x"]]
	class_of, bodies, first_rows, calls = M.classes_of(expected)
	assert class_of.tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [1, 1, 0]]
	assert bodies == [[b"AA", b"AB", b"AC"], [b"", b"-"], [b"x"]] and first_rows == [[0, 1, 3], [0, 2], [0]]
	assert calls == [(0, 0, 0, b"AA"), (1, 0, 0, b""), (2, 0, 0, b"x"), (0, 1, 1, b"AB"), (1, 1, 2, b"-"), (0, 2, 3, b"AC")]
	assert M.classes_of([])[0].shape == (0, 0)


def test_symbol_and_prototype():
	import ctypes as C
	from vcf2multialign_amd import _native as N, build
	lib = C.CDLL(build.LIB_PATH)
	assert hasattr(lib, "v2m_splice_window_set_distinct") and "v2m_splice_window_set_distinct" in N.SIGNATURES
	header = " ".join(open(os.path.join(ROOT, "include", "v2m_hip.h")).read().split())
	assert "typedef int (*v2m_distinct_sink_fn)(void *user, uint64_t window, uint64_t class_index, uint64_t first_row, const char *bytes, uint64_t length);" in header
	assert ("int v2m_splice_window_set_distinct(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags /* 0 or V2M_SPLICE_UNALIGNED */, "
		"v2m_distinct_sink_fn sink /* may be NULL */, void *user, uint32_t *class_of_out /* host, [n_rows][n_windows] */, "
		"uint32_t *n_classes_out /* host, optional, [n_windows] */);") in header
	assert "#define V2M_ABI_VERSION 5" in header and "V2M_DISTINCT_POOL_BYTES" in header and "V2M_KERNEL_COUNT = 9" in header
	assert header.index("---- window sets") < header.index("---- distinct pieces of a window set") < header.index("---- row alignment ops")


def test_corpus_reaches_what_it_is_meant_to(corpus):
	K = M.kernel_constants()
	chunk, long_bytes = K["kDistinctChunkBytes"], K["kDistinctLongBytes"]
	one_class = all_classes = between = 0
	lengths = {False: set(), True: set()}
	for case in corpus:
		assert len({w for w in case.windows}) >= 1 and len(case.rows) >= 1
		for unaligned in (False, True):
			expected = case.expected(unaligned)
			class_of, bodies, first_rows, calls = M.classes_of(expected)
			assert calls == sorted(calls, key=lambda c: (c[2], c[0])) and len(calls) == sum(len(b) for b in bodies)
			for k, b in enumerate(bodies):
				assert class_of[:, k].max() + 1 == len(b) and [expected[r][k] for r in first_rows[k]] == b
				one_class += len(b) == 1
				all_classes += len(b) == len(case.rows) > 1
				between += 1 < len(b) < len(case.rows)
				lengths[unaligned].update(len(x) for x in b)
	assert one_class >= 10 and all_classes >= 2 and between >= 10, (one_class, all_classes, between)
	for mode in (False, True):
		have = lengths[mode]
		assert {1, 7, 8, 9, 15, 16, 17} <= have, sorted(have)[:40]
		# both sides of the chunk, of two chunks and of the short / long threshold (unaligned: what the REF row emits in a longer window)
		assert {chunk - 1, chunk, chunk + 1, 2 * chunk + 1, long_bytes - 8, long_bytes, long_bytes + 8} <= have, mode
	assert 0 in lengths[True] and 0 not in lengths[False]


def test_crafted_windows(corpus):
	case = next(c for c in corpus if c.name == "crafted")
	aligned, unaligned = case.expected(False), case.expected(True)
	k_dash, k_empty, k_after = 0, 1, 2
	assert case.windows[:3] == [case.special["dash"], case.special["all_empty"], case.special["differ_after"]]
	# the literal '-' of the reference against another row's padding: equal aligned pieces, different unaligned pieces
	pairs = [(a, b) for a in range(len(case.rows)) for b in range(a)
		if aligned[a][k_dash] == aligned[b][k_dash] == b"-" and {unaligned[a][k_dash], unaligned[b][k_dash]} == {b"-", b""}]
	assert pairs
	assert M.classes_of(aligned)[0][:, k_dash].tolist() != M.classes_of(unaligned)[0][:, k_dash].tolist()
	# padding in every row: one class of length 0 when unaligned
	assert all(p[k_empty] == b"" for p in unaligned) and all(set(p[k_empty]) == {ord("-")} for p in aligned)
	# equal inside the window, different within the 15 columns after its end
	a, b = case.special["differ_after_rows"]
	begin, end = case.windows[k_after]
	assert aligned[a][k_after] == aligned[b][k_after]
	assert case.walked[a][0][end:end + 15] != case.walked[b][0][end:end + 15] and case.walked[a][0][begin:end] == case.walked[b][0][begin:end]


def test_small_case_fits_the_hash_bits_runs(corpus):
	case = next(c for c in corpus if c.name == "small")
	assert len(case.rows) <= 24 and len(case.windows) <= 40
	for unaligned in (False, True):
		_, bodies, _, _ = M.classes_of(case.expected(unaligned))
		assert max(len(b) for b in bodies) >= 3                     # more than one verify round at 0 bits


def test_classes_span_slices_under_the_small_ring(corpus):
	case = next(c for c in corpus if c.name == "small_ring")
	per_slice = M.rows_per_slice(case, M.SMALL_RING)
	assert 2 <= per_slice and 3 * per_slice < len(case.rows)
	for unaligned in (False, True):
		class_of, _, first_rows, _ = M.classes_of(case.expected(unaligned))
		spanning = sum(1 for k in range(len(case.windows)) for r in range(len(case.rows))
			if first_rows[k][class_of[r, k]] // per_slice < r // per_slice)
		assert spanning >= len(case.windows)
		# and a class that begins in a later slice than the first
		assert any(r // per_slice >= 1 for k in range(len(case.windows)) for r in first_rows[k])


# ---- the CLI, without a device ----------------------------------------------------------------------------------------------------

def _cli(tmp_path, extra):
	args = [CLI, "-H", "-r", os.path.join(FIX, "test-4.fa"), "-a", os.path.join(FIX, "test-4.vcf"), "-c", "1", "--device=99"]
	return subprocess.run(args + list(extra), cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


@pytest.mark.parametrize("extra", [["--distinct"], ["--distinct", "-s", "out.a2m"], ["--distinct", "--region=1-3", "-s", "out.a2m"], ["--distinct", "--output-sequences-separate"]])
def test_cli_distinct_requires_regions_file(tmp_path, extra):
	r = _cli(tmp_path, extra)
	assert r.returncode != 0
	assert b"ERROR: --distinct requires --regions-file." in r.stderr, r.stderr.decode()
	assert b"GPU" not in r.stderr and b"device" not in r.stderr.lower().replace(b"--device", b"")
	assert not os.listdir(tmp_path)


def test_cli_usage_names_distinct():
	r = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
	assert b"--distinct" in r.stderr and b".classes.tsv" in r.stderr
