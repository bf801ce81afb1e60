"""Variable sites without a GPU: the model of tests/variable_sites_model.py held to the fact that ties it to the pair distances (the distances
over the selected columns alone are the distances over all columns), the conditions that keep the corpus of
tests/test_gpu_variable_sites.py from hiding a failure, the host library's site_positions_text against the column counts' text, the header's
constants and prototypes, the exported symbols, and the driver's argument errors."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import column_counts_model as CM
import pair_distances_model as PM
import variable_sites_model as VM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")


def _header():
	with open(os.path.join(ROOT, "include", "v2m_hip.h")) as f:
		return f.read()


@pytest.fixture(scope="module")
def modelled():
	"""Per corpus item: (item, the alignment, the mask of flags 0, the mask of the SNP selection)."""
	out = []
	for item in VM.corpus():
		m = CM.matrix(item.g, item.rows, item.window)
		out.append((item, m, VM.selection(m), VM.selection(m, snp_only=True)))
	return out


# ---- the model -----------------------------------------------------------------------------------------------------------------------------

def test_the_selected_columns_carry_the_distances(modelled):
	"""The one property that ties the selections to what is merged: on every item the pair distances over the selected columns alone
	equal those over all columns -- flags 0 under the all-classes definition, the SNP selection under acgt_only."""
	for item, m, variable, snp in modelled:
		cls = PM.classes(m)
		columns, data, L = VM.expected(item.g, item.rows, item.window)
		assert L == m.shape[1] and np.array_equal(data, m[:, variable]), item.name
		assert np.array_equal(PM.distances(PM.classes(data)), PM.distances(cls)), item.name
		columns, data, _ = VM.expected(item.g, item.rows, item.window, snp_only=True)
		assert np.array_equal(data, m[:, snp]), item.name
		assert np.array_equal(PM.distances(PM.classes(data), acgt_only=True), PM.distances(cls, acgt_only=True)), item.name
		# and no column left out could have added to them
		assert PM.distances(cls[:, ~variable]).sum() == 0 and PM.distances(cls[:, ~snp], acgt_only=True).sum() == 0, item.name
		assert not (snp & ~variable).any(), item.name      # a SNP column is a variable column
		if len(item.rows) <= 1:
			assert not variable.any() and not snp.any(), item.name


def test_the_columns_are_absolute_and_ascend(modelled):
	for item, m, variable, snp in modelled:
		first = item.window[0] if item.window else 0
		for snp_only, mask in ((False, variable), (True, snp)):
			columns, data, _ = VM.expected(item.g, item.rows, item.window, snp_only)
			assert columns.dtype == np.uint64 and data.dtype == np.uint8 and data.shape == (len(item.rows), len(columns)), item.name
			assert (np.diff(columns.astype(np.int64)) > 0).all() and np.array_equal(columns, np.flatnonzero(mask) + first), item.name
			whole = CM.matrix(item.g, item.rows)
			assert np.array_equal(whole[:, columns.astype(np.int64)], data), item.name


def test_the_snp_rule_spelled_out():
	"""By hand over every pair of bytes: only pairs of two different letters of ACGT (either case) make a SNP column."""
	for a in b"AaCcGgTtNn-R@":
		for b in b"AaCcGgTtNn-R@":
			m = np.array([[a], [b]], dtype=np.uint8)
			la, lb = chr(a).lower(), chr(b).lower()
			assert bool(VM.snp(m)[0]) == (la in "acgt" and lb in "acgt" and la != lb), (a, b)
			assert bool(VM.selection(m)[0]) == (PM.classes(m)[0, 0] != PM.classes(m)[1, 0]), (a, b)
	assert not VM.snp(np.array([[ord("A")]], dtype=np.uint8)).any() and VM.snp(np.zeros((0, 3), dtype=np.uint8)).shape == (3,)


# ---- reach: what the GPU corpus holds --------------------------------------------------------------------------------------------------------

def test_the_corpus_cannot_hide_a_failure(modelled):
	S, T, G = VM.kernel_constants()
	W, B = 64 * S, T * S
	names = [item.name for item, *_ in modelled]
	assert len(set(names)) == len(names) and set(i.name for i in PM.corpus()) <= set(names)
	# the two selections differ somewhere, and the SNP selection is a non-empty strict subset somewhere
	assert any(not np.array_equal(v, s) for _, _, v, s in modelled)
	assert any(s.any() and (v & ~s).any() and not (s & ~v).any() for _, _, v, s in modelled)
	# both spellings occur among the selected bytes
	selected = set()
	for _, m, v, _ in modelled:
		selected.update(m[:, v].reshape(-1).tolist())
	assert {ord("c"), ord("C"), ord("t"), ord("T"), ord("n"), ord("N"), ord("-"), ord("R"), 0xC1} <= selected
	# every residue of V mod S and every seam value, as the number of sites of flags 0
	counts = {int(v.sum()) for _, _, v, _ in modelled}
	assert {c % S for c in counts if c} == set(range(S))
	assert set(range(1, S + 2)) | {W - 1, W, W + 1, B - 1, B, B + 1, 2 * B + 1} <= counts and 0 in counts
	assert set(VM.seam_site_counts()) <= counts
	by_name = {item.name: (item, v) for item, _, v, _ in modelled}
	for V in VM.seam_site_counts():
		assert int(by_name["sites_%d" % V][1].sum()) == V
	# the SNP selection too leaves words of one, two and three sites at the end
	assert {int(s.sum()) % S for _, _, _, s in modelled} == set(range(S))
	# the row counts: 1 ... 9 and around the row group
	rows = {len(item.rows) for item, *_ in modelled}
	assert set(range(1, 10)) | {G - 1, G, G + 1, 2 * G + 1} <= rows
	item, v = by_name["two_blocks_three_groups"]
	assert len(item.rows) == 2 * G + 1 and B < int(v.sum()) <= 2 * B
	# a repeated row, and rows with cuts
	item, _ = by_name["cuts"]
	assert item.rows[4] == item.rows[8] and sum(isinstance(r, list) for r in item.rows) == 3


def test_the_sites_graph_pairs_split_as_the_issue_says():
	"""In a sites_graph a site's column holds 'A' and a pair of the six other classes: the pairs (N, -), (N, R) and (-, R) make it variable
	but not SNP; every pair with C, G or T makes it SNP."""
	g = PM.sites_graph_of(64)
	m = CM.matrix(g, PM.SITE_ROWS)
	v, s = VM.selection(m), VM.selection(m, snp_only=True)
	cls = PM.classes(m)
	seen_not_snp = set()
	for col in (int(c) for c in g.site_columns[~g.two_byte]):      # (a two-byte label's padding column holds no 'A': '-' and one class)
		present = set(cls[:, col].tolist())
		assert v[col] and 0 in present
		if s[col]:
			assert len(present & {0, 1, 2, 3}) >= 2
		else:
			seen_not_snp.add(tuple(sorted(present - {0})))
	assert {(4, 5), (4, 6), (5, 6)} <= seen_not_snp
	assert all(not (set(p) & {1, 2, 3}) for p in seen_not_snp)


def test_the_windows(modelled):
	g = PM.window_graph()
	whole = VM.selection(CM.matrix(g, PM.SITE_ROWS))
	ws = [item.window for item, *_ in modelled if item.window]
	assert ws == PM.windows()
	assert any(whole[b] for b, e in ws) and any(whole[e - 1] for b, e in ws) and any(not whole[b:e].any() for b, e in ws)
	for item, m, v, s in modelled:
		if item.window:
			b, e = item.window
			assert np.array_equal(v, whole[b:e]) or len(item.rows) != len(PM.SITE_ROWS)


# ---- the positions text ----------------------------------------------------------------------------------------------------------------------

def test_site_positions_text():
	from vcf2multialign_amd import host
	g = CM.hostile_graph(1)
	rows = CM.HOSTILE_ROWS
	for snp_only in (False, True):
		columns, _, _ = VM.expected(g, rows, snp_only=snp_only)
		got = host.site_positions_text(columns, g.reference_positions, g.aligned_positions)
		assert got == VM.positions_text(g, columns)
		# the first two fields of the column counts' lines of the same columns, made by the same code
		cols, c = CM.expected(g, rows)
		keep = np.isin(cols, columns)
		lines = host.column_counts_text(len(rows), cols[keep], c[keep], g.reference_positions, g.aligned_positions).decode().splitlines()[2:]
		assert got.decode().splitlines() == ["\t".join(line.split("\t")[:2]) for line in lines]
	assert b"\t.\n" in host.site_positions_text(VM.expected(g, rows)[0], g.reference_positions, g.aligned_positions)      # a padding column
	assert host.site_positions_text([], g.reference_positions, g.aligned_positions) == b""


def test_fasta_text():
	data = np.array([[65, 99], [45, 0xC1]], dtype=np.uint8)
	assert VM.fasta(["a", "1\tb"], data) == b">a\nAc\n>1\tb\n-\xc1\n"
	assert VM.fasta(["a", "b"], np.zeros((2, 0), dtype=np.uint8)) == b">a\n\n>b\n\n"


# ---- the header and the library --------------------------------------------------------------------------------------------------------------

def test_header_constants_and_prototypes():
	from vcf2multialign_amd import _native as N
	header = _header()
	assert re.search(r"#define V2M_SITES_SNP\s+0x40u", header) and N.SITES_SNP == 0x40
	flags = [int(x, 16) for x in re.findall(r"^#define V2M_(?:SPLICE|OPS|COUNTS|DIST|SITES)_\w+\s+(0x[0-9a-fA-F]+)u", header, re.M)]
	assert len(flags) == 7 and len(set(flags)) == 7                     # collides with no flag of the row, counts or distance calls
	assert "#define V2M_ABI_VERSION 5" in header and "V2M_KERNEL_END = 15" in header and "V2M_KERNEL_LIMIT = 17" in header
	assert header.index("---- pair distances") < header.index("---- variable sites") < header.index("---- founder search")
	assert re.search(r"\bint v2m_variable_sites\(v2m_ctx \*ctx, const v2m_row_batch \*rows, uint32_t flags[^;]*?,\s*v2m_site_columns_sink_fn columns_sink[^;]*?,"
		r"\s*v2m_site_rows_sink_fn rows_sink[^;]*?, void \*user,\s*v2m_variable_sites_info \*info", header)
	assert re.search(r"\bint v2m_variable_sites_device\(v2m_ctx \*ctx, const v2m_row_batch \*rows, uint32_t flags[^;]*?,\s*void \*d_columns[^;]*?, void \*d_bytes, uint64_t pitch, uint64_t \*n_sites\)", header)
	assert re.search(r"typedef int \(\*v2m_site_columns_sink_fn\)\(void \*user, const uint64_t \*columns, uint64_t n_sites\);", header)
	assert re.search(r"typedef int \(\*v2m_site_rows_sink_fn\)\(void \*user, uint64_t first_row, uint64_t n_rows, const char \*bytes, uint64_t pitch, uint64_t n_sites\);", header)
	for name in ("v2m_variable_sites", "v2m_variable_sites_device"):
		assert name in N.SIGNATURES
	fields = re.search(r"typedef struct \{([^}]*)\} v2m_variable_sites_info;", header).group(1)
	assert re.findall(r"(\w+);", fields) == [f for f, _ in N.VariableSitesInfo._fields_] == ["n_sites", "n_columns", "counts_ms", "gather_ms"]
	assert C.sizeof(N.VariableSitesInfo) == 32
	assert (N.GATHER_SITES, N.GATHER_THREADS, N.GATHER_MIN_GROUP_ROWS) == VM.kernel_constants()


def test_exported_symbols():
	from vcf2multialign_amd import build
	hip = C.CDLL(build.LIB_PATH)
	for name in ("v2m_variable_sites", "v2m_variable_sites_device"):
		assert hasattr(hip, name), name
	host = C.CDLL(build.HOST_LIB_PATH)
	assert hasattr(host, "v2mh_site_positions_text")
	out = subprocess.run(["nm", "-D", "--defined-only", build.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
	assert " T v2m_variable_sites\n" in out and " T v2m_variable_sites_device\n" in out


def test_the_kernels_are_in_the_library_source():
	with open(VM.SITE_KERNELS_HPP) as f:
		text = f.read()
	for kernel in ("count_snp_columns_kernel", "emit_snp_columns_kernel", "gather_sites_kernel"):
		assert re.search(r"__global__[^;{]*\b%s\(" % kernel, text), kernel
	assert text.count("__shared__") == text.count("V2M_POISON_LDS(") == 2         # every LDS object goes through V2M_POISON_LDS
	with open(os.path.join(ROOT, "vcf2multialign_amd", "csrc", "v2m_hip.hip")) as f:
		library = f.read()
	assert library.index('#include "distance_kernels.hpp"') < library.index('#include "site_kernels.hpp"')
	# the row-group rule the corpus' row counts are chosen for
	assert "std::max<u64>({u64(v2m::kGatherMinGroupRows), (nr + want_groups - 1) / want_groups, (nr + 65534) / 65535})" in library
	# and the knob that replaces it in tests/test_gpu_variable_sites.py, read once per call in either form
	assert "forced_site_group(forced_rows, std::max<u64>({u64(v2m::kGatherMinGroupRows)," in library
	assert library.count('u64 const forced_rows(env_u64("V2M_SITE_ROWS_PER_GROUP", 0));') == 2
	from vcf2multialign_amd import build
	assert VM.SITE_KERNELS_HPP in build.deps("HIP_DEPS")


def test_python_surface():
	import inspect
	import vcf2multialign_amd as v
	assert list(inspect.signature(v.Context.variable_sites).parameters) == ["self", "rows", "snp_only", "info"]
	assert list(inspect.signature(v.Context.variable_sites_device).parameters) == ["self", "rows", "ptr", "pitch", "columns_ptr", "snp_only"]
	assert list(inspect.signature(v.HaplotypeOutput.output_variable_sites).parameters) == ["self", "graph", "stream", "snp_only", "positions"]
	assert list(inspect.signature(v.FounderSequenceGreedyOutput.output_variable_sites).parameters) == ["self", "graph", "cut_positions", "assigned_samples_column_major", "stream", "snp_only", "positions"]


# ---- the driver's argument errors (reported before a device is opened) ---------------------------------------------------------------------

def _run(args, cwd=None):
	assert os.path.exists(CLI), "build the host driver first (__graft_entry__.build())"
	return subprocess.run([CLI] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_cli_argument_errors(tmp_path):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	bed = tmp_path / "r.bed"
	bed.write_text("1\t0\t4\n")
	common = ["-H", "-r", fa, "-a", vcf, "-c", "1"]
	for extra, what in ((["--regions-file=" + str(bed)], "--regions-file"), (["--device=0,0"], "more than one --device entry")):
		r = _run(common + ["--output-variable-sites=" + str(tmp_path / "x.fa")] + extra, cwd=str(tmp_path))
		assert r.returncode != 0
		assert ("ERROR: --output-variable-sites cannot be combined with %s.\n" % what).encode() in r.stderr, r.stderr.decode()
	r = _run(common + ["--snp-sites", "-s", str(tmp_path / "x.a2m")], cwd=str(tmp_path))
	assert r.returncode != 0 and b"ERROR: --snp-sites requires --output-variable-sites.\n" in r.stderr
	r = _run(common + ["--output-site-positions=" + str(tmp_path / "x.tsv"), "-s", str(tmp_path / "x.a2m")], cwd=str(tmp_path))
	assert r.returncode != 0 and b"ERROR: --output-site-positions requires --output-variable-sites.\n" in r.stderr
	assert not (tmp_path / "x.fa").exists() and not (tmp_path / "x.a2m").exists() and not (tmp_path / "x.tsv").exists()
	r = _run(["--help"])
	text = r.stdout + r.stderr
	assert r.returncode == 0 and b"--output-variable-sites=FILE" in text and b"--snp-sites" in text and b"--output-site-positions=FILE" in text
