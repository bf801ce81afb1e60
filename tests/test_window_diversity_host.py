"""Window diversity without a GPU (include/v2m_hip.h, "window diversity"): the numpy model from counts against a brute force over the
rows' pairs, the worked Tajima value, the model against the host library's plain loops and doubles bit for bit on the graph items of
tests/variable_sites_model.py, the texts, the header, the exported symbols, the kernels' source, windows as sums of bins, the driver's argument
errors, and the census of the seams the GPU corpus reaches."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import column_counts_model as CM
import variable_sites_model as VM
import window_diversity_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def same_records(got, want, what):
	assert got.dtype == want.dtype and len(got) == len(want), (what, got.dtype, want.dtype, len(got), len(want))
	if got.tobytes() != want.tobytes():
		k = next(i for i in range(len(got)) if got[i:i + 1].tobytes() != want[i:i + 1].tobytes())
		raise AssertionError("%s: the first difference at record %d of %d: got %s, expected %s" % (what, k, len(got), got[k], want[k]))


# ---- the model against the brute force --------------------------------------------------------------------------------------------------

SMALL = [(n, L, seed) for seed, (n, L) in enumerate([(1, 5), (2, 9), (3, 12), (4, 16), (5, 23), (8, 31), (13, 40)])]


@pytest.mark.parametrize("n,L,seed", SMALL)
def test_counts_model_equals_the_brute_force(n, L, seed):
	m = M.random_alignment(n, L, seed)
	c = M.letters_of(m)
	for bounds in (np.array([0, L], dtype=np.uint64), np.arange(L + 1, dtype=np.uint64), M.random_bounds(L, 6, seed)):
		bins, sfs, many = M.brute_within(m, bounds)
		same_records(M.from_counts(c, n, bounds), bins, "within")
		want_sfs, want_many = M.sfs_from_counts(c, n, bounds[0], bounds[-1])
		assert sfs.tobytes() == want_sfs.tobytes() and many == want_many
		assert int(sfs.sum()) + many == int(bins["complete"].sum())
		mb = M.random_alignment(n + 2, L, seed + 100)
		same_records(M.between_from_counts(c, M.letters_of(mb), bounds), M.brute_between(m, mb, bounds), "between")


def test_the_small_alignments_hold_every_kind_of_byte():
	kinds = set(b"".join(M.random_alignment(n, L, seed).tobytes() for n, L, seed in SMALL))
	assert set(b"ACGTacgtNn-") <= kinds and kinds - set(b"ACGTacgtNn-"), "both cases, N, gap, other bytes"


def test_the_worked_tajima_value():
	a1, a2 = M.harmonics(10)
	assert float(a1) == 2.8289682539682537 and float(a2) == 1.5397677311665408
	assert float(M.tajima_of(10, 16, 3.888889)) == -1.4461719856148525
	assert "%.6f" % M.tajima_of(10, 16, 3.888889) == "-1.446172"


def test_values_that_do_not_exist():
	rec = np.zeros(1, dtype=M.BIN_DTYPE)[0]
	assert all(x != x for x in M.values(rec, 1))
	pi, theta, tajima = M.values(rec, 5)
	assert pi != pi and theta == 0.0 and tajima != tajima          # S = 0: v = 0, no D
	between = np.zeros(1, dtype=M.BETWEEN_DTYPE)[0]
	assert all(x != x for x in M.divergence_values(between, rec, rec))


# ---- the model against the host library's plain loops -----------------------------------------------------------------------------------

GRAPH_ITEMS = VM.corpus()


def bounds_of(L):
	return [np.arange(L + 1, dtype=np.uint64), np.array(sorted(set(list(range(0, L, 7)) + [L])), dtype=np.uint64), np.array([0, L], dtype=np.uint64)]


@pytest.mark.parametrize("item", GRAPH_ITEMS, ids=[i.name for i in GRAPH_ITEMS])
def test_model_equals_the_restatement(item):
	from vcf2multialign_amd import host
	m = np.ascontiguousarray(CM.matrix(item.g, item.rows, item.window))
	n, L = m.shape
	c = M.letters_of(m)
	half = max(1, n // 2)
	ma, mb = np.ascontiguousarray(m[:half]), np.ascontiguousarray(m[half:])
	for bounds in bounds_of(L) if L else []:
		bins, sfs, many = host.window_diversity_cpu(m, bounds)
		want = M.from_counts(c, n, bounds)
		same_records(bins, want, item.name)
		want_sfs, want_many = M.sfs_from_counts(c, n, bounds[0], bounds[-1])
		assert sfs.tobytes() == want_sfs.tobytes() and many == want_many, item.name
		assert host.window_diversity_values(bins, n).tobytes() == M.values_array(want, n).tobytes(), item.name
		if len(mb):
			between, none, zero = host.window_diversity_cpu(ma, bounds, rows_b=mb)
			want_between = M.between_from_counts(M.letters_of(ma), M.letters_of(mb), bounds)
			same_records(between, want_between, item.name + ": between")
			assert none is None and zero == 0
			wa, wb = M.from_counts(M.letters_of(ma), len(ma), bounds), M.from_counts(M.letters_of(mb), len(mb), bounds)
			assert host.window_divergence_values(between, wa, wb).tobytes() == M.divergence_array(want_between, wa, wb).tobytes(), item.name


def test_the_restatement_on_small_alignments_and_its_errors():
	from vcf2multialign_amd import host
	m = M.random_alignment(6, 40, 3)
	bounds = np.array([2, 2, 9, 30, 30, 38], dtype=np.uint64)
	bins, sfs, many = host.window_diversity_cpu(m, bounds)
	want, want_sfs, want_many = M.brute_within(m, bounds)
	same_records(bins, want, "brute")
	assert sfs.tobytes() == want_sfs.tobytes() and many == want_many
	bins, sfs, many = host.window_diversity_cpu(m, bounds, want_sfs=False)
	same_records(bins, want, "no spectrum")
	assert sfs is None and many == 0
	with pytest.raises(ValueError):
		host.window_diversity_cpu(m, [3, 2])
	with pytest.raises(ValueError):
		host.window_diversity_cpu(m, [0, 41])
	assert len(host.window_diversity_cpu(m, [])[0]) == 0


def test_the_doubles_on_windows_of_every_kind():
	from vcf2multialign_amd import host
	rng = np.random.default_rng(7)
	for n in (1, 2, 3, 10, 501, 32768):
		recs = np.zeros(40, dtype=M.BIN_DTYPE)
		for name in M.BIN_DTYPE.names:
			recs[name] = rng.integers(0, 1 << int(rng.integers(1, 61)), size=len(recs), dtype=np.uint64)
		recs[:4] = 0
		recs["complete_segregating"][4:8] = 1
		assert host.window_diversity_values(recs, n).tobytes() == M.values_array(recs, n).tobytes(), n
		between = np.zeros(len(recs), dtype=M.BETWEEN_DTYPE)
		for name in M.BETWEEN_DTYPE.names:
			between[name] = rng.integers(0, 1 << 40, size=len(recs), dtype=np.uint64)
		between[::5] = 0
		assert host.window_divergence_values(between, recs, recs[::-1].copy()).tobytes() == M.divergence_array(between, recs, recs[::-1]).tobytes(), n


# ---- the texts ------------------------------------------------------------------------------------------------------------------------

def test_texts():
	from vcf2multialign_amd import host
	m = M.random_alignment(10, 60, 1)
	bounds = np.array([0, 10, 10, 35, 60], dtype=np.uint64)
	bins = M.from_counts(M.letters_of(m), 10, bounds)
	starts, ends = bounds[:-1] + np.uint64(1), bounds[1:]
	for header in (False, True):
		assert host.window_diversity_text("all", 10, bins, starts, ends, header=header) == M.diversity_text("all", 10, bins, starts, ends, header=header)
	text = M.diversity_text("all", 10, bins, starts, ends, header=True).decode().splitlines()
	assert text[0].split("\t") == ["#group", "start", "end", "columns", "called", "diffs", "pairs", "pi", "segregating", "complete", "theta_w", "tajima_d"]
	assert text[2].split("\t")[3:8] == ["0", "0", "0", "0", "NA"] and len(text) == 5
	ma, mb = m[:4], m[4:]
	between = M.between_from_counts(M.letters_of(ma), M.letters_of(mb), bounds)
	wa, wb = M.from_counts(M.letters_of(ma), 4, bounds), M.from_counts(M.letters_of(mb), 6, bounds)
	for header in (False, True):
		assert host.window_divergence_text("a", "b", between, wa, wb, starts, ends, header=header) == M.divergence_text("a", "b", between, wa, wb, starts, ends, header=header)
	assert b"\tNA\tNA\n" in M.divergence_text("a", "b", between, wa, wb, starts, ends)
	sfs, many = M.sfs_from_counts(M.letters_of(m), 10, 0, 60)
	for header in (False, True):
		assert host.diversity_sfs_text("all", 10, sfs, many, header=header) == M.sfs_text("all", 10, sfs, many, header=header)
	assert M.sfs_text("g", 3, [5, 2], 1) == b"g\t3\t0\t5\ng\t3\t1\t2\ng\t3\tmultiallelic\t1\n"
	with pytest.raises(ValueError):
		host.window_diversity_text("a\tb", 10, bins, starts, ends)
	with pytest.raises(ValueError):
		host.diversity_sfs_text("all", 10, sfs[:-1], many)


# ---- the header, the symbols, the source ----------------------------------------------------------------------------------------------

def test_header_constants_layouts_and_prototypes():
	from vcf2multialign_amd import _native as N
	with open(os.path.join(ROOT, "include", "v2m_hip.h")) as f:
		header = f.read()
	assert "#define V2M_ABI_VERSION 5" in header and "V2M_KERNEL_END = 15" in header and "V2M_KERNEL_LIMIT = 17" in header
	assert header.index("---- parsimony") < header.index("---- window diversity") < header.index("---- founder search")
	assert "#define V2M_DIVERSITY_MAX_ROWS 32768u" in header and N.DIVERSITY_MAX_ROWS == M.MAX_ROWS == 32768
	assert (N.DIVERSITY_COLUMNS, N.DIVERSITY_SFS_LDS_BINS) == M.kernel_constants()
	for name, dtype, size, model in (("v2m_diversity_bin", N.DIVERSITY_BIN_DTYPE, 64, M.BIN_DTYPE), ("v2m_diversity_between_bin", N.DIVERSITY_BETWEEN_BIN_DTYPE, 32, M.BETWEEN_DTYPE)):
		body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, header).group(1)
		assert re.findall(r"\b(\w+)\s*[,;]", body) == [f for f, *_ in dtype], name
		assert np.dtype(dtype).itemsize == size and np.dtype(dtype) == model
		assert "uint64_t" in body and "uint32_t" not in body
	info = re.search(r"typedef struct \{([^}]*)\} v2m_window_diversity_info;", header).group(1)
	assert re.findall(r"(\w+);", info) == [f for f, _ in N.WindowDiversityInfo._fields_] == ["n_columns", "n_bins", "multiallelic", "counts_ms", "bins_ms"]
	assert C.sizeof(N.WindowDiversityInfo) == 40
	assert re.search(r"\bint v2m_diversity_of_counts\(v2m_ctx \*ctx, const void \*d_counts_a, const void \*d_counts_b[^;]*?, uint64_t plane_pitch, uint64_t L,\s*"
		r"uint64_t n_a, uint64_t n_b, const uint64_t \*bounds[^;]*?, uint64_t n_bins, void \*d_bins,\s*void \*d_sfs[^;]*?, v2m_window_diversity_info \*info[^;]*?\);", header)
	assert re.search(r"\bint v2m_window_diversity\(v2m_ctx \*ctx, const v2m_row_batch \*rows_a, const v2m_row_batch \*rows_b[^;]*?,\s*const uint64_t \*bounds[^;]*?, "
		r"uint64_t n_bins, void \*bins[^;]*?,\s*uint64_t \*sfs[^;]*?, v2m_window_diversity_info \*info[^;]*?\);", header)
	assert len(N.SIGNATURES["v2m_diversity_of_counts"][1]) == 12 and len(N.SIGNATURES["v2m_window_diversity"][1]) == 8
	# every operation of the doubles is spelled out
	for line in ("pi       = d(diffs) / d(pairs)", "theta_w  = S / a1", "tajima_d = (k - S / a1) / sqrt(v)", "fst      = 1 - (pi_A + pi_B) / (2 * dxy)"):
		assert line in header, line


def test_exported_symbols():
	from vcf2multialign_amd import build
	for path in (build.LIB_PATH, build.CHECKED_LIB_PATH):
		out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, check=True).stdout.decode()
		assert " T v2m_diversity_of_counts\n" in out and " T v2m_window_diversity\n" in out and " T v2m_read_output\n" in out, path
	for path in (build.HOST_LIB_PATH, build.CHECKED_HOST_LIB_PATH):
		out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, check=True).stdout.decode()
		for name in ("v2mh_window_diversity_cpu", "v2mh_window_diversity_values", "v2mh_window_divergence_values", "v2mh_window_diversity_text", "v2mh_window_divergence_text",
				"v2mh_diversity_sfs_text"):
			assert " T %s\n" % name in out, (path, name)


def test_the_kernels_are_in_the_library_source():
	from vcf2multialign_amd import build
	with open(M.DIVERSITY_KERNELS_HPP) as f:
		text = f.read()
	for kernel in ("diversity_init_kernel", "diversity_bins_kernel"):
		assert re.search(r"__global__[^;{]*\b%s\(" % kernel, text), kernel
	code = re.sub(r"//[^\n]*", "", text)
	assert "V2M_POISON_LDS(wave_sums)" in code and "V2M_POISON_LDS(histogram)" in code
	assert "float" not in code and "double" not in code, "integers only"
	with open(os.path.join(ROOT, "vcf2multialign_amd", "csrc", "v2m_hip.hip")) as f:
		library = f.read()
	assert library.index('#include "parsimony_kernels.hpp"') < library.index('#include "diversity_kernels.hpp"')
	assert M.DIVERSITY_KERNELS_HPP in build.deps("HIP_DEPS")
	assert "hipLaunchCooperativeKernel" not in library and "d_diversity_bounds" in library


def test_python_surface():
	import inspect
	import vcf2multialign_amd as v2m
	from vcf2multialign_amd import host
	assert list(inspect.signature(v2m.Context.window_diversity).parameters) == ["self", "rows", "bounds", "rows_b", "want_sfs", "info"]
	assert list(inspect.signature(v2m.Context.diversity_of_counts).parameters) == ["self", "counts_ptr", "plane_pitch", "length", "n", "bounds", "bins_ptr", "sfs_ptr",
		"counts_b_ptr", "n_b"]
	assert list(inspect.signature(host.window_diversity_cpu).parameters) == ["rows", "bounds", "rows_b", "length", "want_sfs"]
	from vcf2multialign_amd import output
	assert list(inspect.signature(output.HaplotypeOutput.output_diversity).parameters) == ["self", "graph", "diversity", "sfs", "divergence", "window", "step", "groups"]
	assert list(inspect.signature(output.FounderSequenceGreedyOutput.output_diversity).parameters) == ["self", "graph", "cut_positions", "assigned_samples_column_major",
		"diversity", "sfs", "divergence", "window", "step", "groups"]
	assert list(inspect.signature(v2m.Context.read_output).parameters) == ["self", "ptr", "count", "dtype"]
	for name in ("window_diversity_text", "window_divergence_text", "diversity_sfs_text", "window_diversity_values", "window_divergence_values"):
		assert callable(getattr(host, name))


# ---- windows of several bins, and the driver's argument errors (reported before a device is opened) -----------------------------------

def test_windows_are_bins_summed_as_integers():
	m = M.random_alignment(9, 50, 2)
	bounds = np.arange(0, 51, 5, dtype=np.uint64)
	bins = M.from_counts(M.letters_of(m), 9, bounds)
	for width in (1, 2, 5, 10):
		windows = M.summed(bins, width)
		coarse = M.from_counts(M.letters_of(m), 9, bounds[::width])
		same_records(windows, coarse, "width %d" % width)           # disjoint windows of `width` bins are the bins of the coarser bounds
	assert int(M.summed(bins, 10)["columns"][0]) == 50 and len(M.summed(bins, 3)) == 4


CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")


def _run(args, cwd=None):
	assert os.path.exists(CLI), "build the host driver first (__graft_entry__.build())"
	return subprocess.run([CLI] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_cli_argument_errors(tmp_path):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	out = tmp_path / "x.tsv"
	common = ["-H", "-r", fa, "-a", vcf, "-c", "1", "--output-diversity=" + str(out)]
	r = _run(common + ["--diversity-window=10", "--diversity-step=4"], cwd=str(tmp_path))
	assert r.returncode != 0 and b"ERROR: --diversity-step must divide --diversity-window (10 is no multiple of 4).\n" in r.stderr, r.stderr.decode()
	r = _run(common + ["--output-divergence=" + str(tmp_path / "d.tsv")], cwd=str(tmp_path))
	assert r.returncode != 0 and b"ERROR: --output-divergence requires --diversity-groups.\n" in r.stderr, r.stderr.decode()
	groups = tmp_path / "groups.tsv"
	groups.write_text("REF\ta\nnobody.1\tb\n")
	r = _run(common + ["--diversity-groups=" + str(groups)], cwd=str(tmp_path))
	assert r.returncode != 0 and b"\"nobody.1\" names no output sequence.\n" in r.stderr, r.stderr.decode()
	groups.write_text("".join("id%d\tgroup%d\n" % (k, k) for k in range(17)))
	r = _run(common + ["--diversity-groups=" + str(groups)], cwd=str(tmp_path))
	assert r.returncode != 0 and b"line 17: more than 16 groups.\n" in r.stderr, r.stderr.decode()
	for flag in ("--diversity-window=5", "--diversity-step=5", "--diversity-groups=" + str(groups)):
		r = _run(["-H", "-r", fa, "-a", vcf, "-c", "1", "-s", str(tmp_path / "x.a2m"), flag], cwd=str(tmp_path))
		assert r.returncode != 0 and b"requires --output-diversity, --diversity-sfs or --output-divergence.\n" in r.stderr, r.stderr.decode()
	assert not out.exists() and not (tmp_path / "d.tsv").exists() and not (tmp_path / "x.a2m").exists()
	r = _run(["--help"])
	text = r.stdout + r.stderr
	assert r.returncode == 0 and all(flag in text for flag in (b"--output-diversity=FILE", b"--diversity-window=BP", b"--diversity-step=BP", b"--diversity-sfs=FILE",
		b"--diversity-groups=FILE", b"--output-divergence=FILE"))


# ---- the census of the GPU corpus -----------------------------------------------------------------------------------------------------

def test_every_seam_is_reached_by_an_item():
	reached = {}
	for item in M.corpus():
		for seam in M.census(item):
			reached.setdefault(seam, []).append(item.name)
	missing = [s for s in M.SEAMS if s not in reached]
	assert not missing, missing
	assert set(reached) <= set(M.SEAMS)


def test_the_corpus_items_are_tables_a_count_could_make():
	T, H = M.kernel_constants()
	for item in M.corpus():
		lo, hi = int(item.bounds[0]), int(item.bounds[-1])
		assert 0 <= lo <= hi <= item.L and (np.diff(item.bounds.astype(np.int64)) >= 0).all(), item.name
		assert int(item.planes[:, lo:hi].astype(np.uint64).sum(axis=0).max(initial=0)) <= item.n, item.name
		if item.planes_b is not None:
			assert int(item.planes_b[:, lo:hi].astype(np.uint64).sum(axis=0).max(initial=0)) <= item.n_b and item.planes_b.shape == item.planes.shape, item.name
		assert item.n <= M.MAX_ROWS and item.n_b <= M.MAX_ROWS
