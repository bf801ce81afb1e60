"""Window sets on the CPU: the layout of a set through the context-free v2m_window_set_layout, the new symbols and their prototypes, and
--regions-file's BED parsing and refusals through the CLI (reported before any device is opened)."""

import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
LENGTHS = [1, 15, 16, 17, 31, 32, 33, 16383, 16384, 16385, 32769]


def model(windows):
	offsets, at = [], 0
	for b, e in windows:
		offsets.append(at)
		at += (e - b + 15) // 16 * 16
	return offsets, (at + 255) // 256 * 256


def _raw_layout(begins, ends):
	from vcf2multialign_amd import _native as N
	lib = N.load()
	b, e = np.ascontiguousarray(begins, dtype=np.uint64), np.ascontiguousarray(ends, dtype=np.uint64)
	offsets, pitch = np.zeros(max(1, b.size), dtype=np.uint64), C.c_uint64(0)
	rc = lib.v2m_window_set_layout(b.size, b.ctypes.data if b.size else None, e.ctypes.data if e.size else None, offsets.ctypes.data, C.byref(pitch))
	return rc, lib.v2m_last_error(None).decode()


@pytest.mark.parametrize("lengths", [LENGTHS, LENGTHS[::-1]], ids=["ascending", "reversed"])
def test_layout_is_the_model(lengths):
	import vcf2multialign_amd as v2m
	rng = np.random.default_rng(len(lengths))
	windows = [(int(b), int(b) + n) for b, n in zip(rng.integers(0, 100000, size=len(lengths)), lengths)]
	offsets, pitch = v2m.window_set_layout(windows)
	assert (offsets, pitch) == model(windows)
	ends = [o + (e - b + 15) // 16 * 16 for o, (b, e) in zip(offsets, windows)]
	assert offsets[0] == 0 and all(o % 16 == 0 for o in offsets)
	assert all(ends[k] <= offsets[k + 1] for k in range(len(windows) - 1))           # slots never overlap
	assert pitch == (ends[-1] + 255) // 256 * 256 and pitch % 256 == 0 and pitch >= ends[-1]


def test_repeated_and_overlapping_windows_get_their_own_slots():
	import vcf2multialign_amd as v2m
	windows = [(100, 140), (100, 140), (90, 150), (100, 140), (139, 141), (0, 1), (100, 140)]
	offsets, pitch = v2m.window_set_layout(windows)
	assert (offsets, pitch) == model(windows)
	assert offsets == [0, 48, 96, 160, 208, 224, 240] and pitch == 512
	assert len(set(offsets)) == len(windows)


def test_layout_errors():
	import vcf2multialign_amd as v2m
	from vcf2multialign_amd import _native as N
	rc, _ = _raw_layout([], [])
	assert rc == N.V2M_ERR_INVALID_ARGUMENT
	for bad, (b, e) in ((0, (5, 5)), (2, (9, 3))):
		begins, ends = [10, 10, 10], [20, 20, 20]
		begins[bad], ends[bad] = b, e
		rc, message = _raw_layout(begins, ends)
		assert rc == N.V2M_ERR_INVALID_ARGUMENT and ("window %d" % bad) in message, message
	with pytest.raises(v2m.V2MError) as err:
		v2m.window_set_layout([(3, 3)])
	assert err.value.code == N.V2M_ERR_INVALID_ARGUMENT
	# the slots reach 2^32: the unaligned kernels keep per-tile destinations in 32 bits.  No graph is needed for the layout.
	rc, message = _raw_layout([0, 0], [1 << 31, 1 << 31])
	assert rc == N.V2M_ERR_UNSUPPORTED and "2^32" in message
	assert _raw_layout([0, 7], [1 << 31, (1 << 31) - 16 + 7])[0] == N.V2M_OK            # 2^32 - 16: the last layout that fits
	assert _raw_layout([0], [1 << 32])[0] == N.V2M_ERR_UNSUPPORTED
	assert _raw_layout([0, 0, 0], [(1 << 64) - 1, (1 << 64) - 1, 40])[0] == N.V2M_ERR_UNSUPPORTED   # (the sum must not wrap)


def test_symbols_and_prototypes():
	from vcf2multialign_amd import _native as N, build
	lib = C.CDLL(build.LIB_PATH)
	names = ("v2m_window_set_layout", "v2m_set_window_set", "v2m_window_set_size", "v2m_window_set_pitch", "v2m_splice_window_set", "v2m_splice_window_set_device")
	for name in names:
		assert hasattr(lib, name) and name in N.SIGNATURES
	header = " ".join(open(os.path.join(ROOT, "include", "v2m_hip.h")).read().split())
	for prototype in (
			"int v2m_window_set_layout(uint64_t n_windows, const uint64_t *col_begin, const uint64_t *col_end, uint64_t *slot_offset /* [n_windows] */, uint64_t *record_pitch);",
			"int v2m_set_window_set(v2m_ctx *ctx, uint64_t n_windows, const uint64_t *col_begin, const uint64_t *col_end);",
			"uint64_t v2m_window_set_size(const v2m_ctx *ctx);",
			"uint64_t v2m_window_set_pitch(const v2m_ctx *ctx);",
			"typedef int (*v2m_window_sink_fn)(void *user, uint64_t row_index, const char *record, const uint32_t *lengths /* [n_windows] */);",
			"int v2m_splice_window_set(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, v2m_window_sink_fn sink, void *user);",
			"int v2m_splice_window_set_device(v2m_ctx *ctx, const v2m_row_batch *rows, uint32_t flags, void *d_out, uint64_t record_pitch, uint32_t *lengths_out /* host, optional, [n_rows][n_windows] */);"):
		assert prototype in header, prototype
	assert "#define V2M_ABI_VERSION 5" in header and N.ABI_VERSION == 5
	assert header.index("---- column windows") < header.index("---- window sets") < header.index("---- founder search")
	assert lib.v2m_window_set_size(None) == 0 and lib.v2m_window_set_pitch(None) == 0


# ---- --regions-file -----------------------------------------------------------------------------------------------------------------

def _cli(tmp_path, bed, extra=(), chromosome="1"):
	path = tmp_path / "regions.bed"
	path.write_bytes(bed)
	args = [CLI, "-H", "-r", os.path.join(FIX, "test-4.fa"), "-a", os.path.join(FIX, "test-4.vcf"), "--regions-file=" + str(path), "--device=99"]
	if chromosome is not None:
		args += ["-c", chromosome]
	return subprocess.run(args + list(extra), cwd=str(tmp_path), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def _refused(r, *messages):
	assert r.returncode == 1, r.stderr.decode()
	for m in messages:
		assert m in r.stderr, r.stderr.decode()
	assert b"GPU" not in r.stderr and b"device" not in r.stderr.lower().replace(b"--device", b"")


def _ref_length():
	with open(os.path.join(FIX, "test-4.fa"), "rb") as f:
		return sum(len(line.strip()) for line in f if not line.startswith(b">"))


@pytest.mark.parametrize("bed,line,message", [
	(b"1\tx\t5\n", 1, b"decimal integers"),
	(b"# genes\n1\t0\t3\tok\n1\t2\t-5\n", 3, b"decimal integers"),
	(b"1\t1.5\t5\n", 1, b"decimal integers"),
	(b"1\t0\t3\n\n1\t4\t4\tempty\n", 3, b"not less than end"),
	(b"track name=x\n1\t5\t2\n", 2, b"not less than end"),
	(b"1\t0\t2\ta\n1\t1\t3\tb\n1\t0\t2\ta\n", 3, b"duplicate region name \"a\" (first on line 1)"),
	(b"1\t0\t2\n1\t0\t2\n", 2, b"duplicate region name \"1_0_2\""),
	(b"1\t0\t2\tgenes/a\n", 1, b"cannot name a file"),
	(b"1\t0\t2\t..\n", 1, b"cannot name a file"),
	(b"1\t0\t2\t.\n", 1, b"cannot name a file"),
	(b"1\t0\t2\t\n", 1, b"cannot name a file"),
	(b"1\t0\t2\ta\0b\n", 1, b"cannot name a file"),
	(b"browser position\n1\t0\n", 2, b"at least three tab-separated fields"),
	(b"1 0 2\n", 1, b"at least three tab-separated fields"),
])
def test_cli_bed_errors_name_their_line(tmp_path, bed, line, message):
	_refused(_cli(tmp_path, bed), b"--regions-file", ("regions.bed line %d:" % line).encode(), message)
	assert not [f for f in os.listdir(tmp_path) if f.endswith((".a2m", ".fa"))]


def test_cli_bed_end_past_the_reference(tmp_path):
	R = _ref_length()
	_refused(_cli(tmp_path, b"1\t0\t%d\tfits\n1\t1\t%d\tlong\n" % (R, R + 1)), b"regions.bed line 2:", b"past the end of the reference sequence (%d)" % R)


def test_cli_bed_no_region_on_the_chromosome(tmp_path):
	_refused(_cli(tmp_path, b"# only other chromosomes\n2\t0\t3\n3\t0\t3\tx\n"), b"holds no region on chromosome \"1\"")
	_refused(_cli(tmp_path, b"# nothing\n\ntrack x\n"), b"holds no region")
	_refused(_cli(tmp_path, b"2\t0\t3\n2\t5\t1\n", chromosome="2"), b"regions.bed line 2:")      # taken once it is the chromosome's
	r = _cli(tmp_path, b"2\t5\t1\n1\t0\t3\n")                                                    # a bad line of another chromosome is skipped
	assert b"regions.bed line" not in r.stderr


@pytest.mark.parametrize("extra,named", [
	(["--region=1-3"], b"--region"), (["-s", "out.a2m"], b"-s / --output-sequences-a2m"), (["--output-sequences-separate"], b"--output-sequences-separate"),
	(["--pipe=cat"], b"--pipe"), (["-s", "out.a2m.gz", "--bgzf"], b"-s / --output-sequences-a2m"), (["--device=0,1"], b"more than one --device entry")])
def test_cli_refuses_conflicting_options(tmp_path, extra, named):
	_refused(_cli(tmp_path, b"1\t0\t3\n", extra=extra), b"--regions-file cannot be combined with " + named)


def test_cli_refuses_bgzf(tmp_path):
	r = _cli(tmp_path, b"1\t0\t3\n", extra=["--bgzf"])
	assert r.returncode == 1 and b"--bgzf" in r.stderr


def test_cli_usage_names_regions_file():
	r = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
	assert b"--regions-file=FILE.bed" in r.stderr
