"""Pair distances without a GPU: the model of tests/pair_distances_model.py held to the fact the library's design rests on (only the variable
columns count), the conditions that keep the corpus of tests/test_gpu_pair_distances.py from hiding a failure, the host library's
distances_text against the model's text, the header's constants and prototypes, the exported symbols, and the driver's argument errors."""

import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import column_counts_model as CM
import pair_distances_model as PM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")


def _header():
	with open(os.path.join(ROOT, "include", "v2m_hip.h")) as f:
		return f.read()


@pytest.fixture(scope="module")
def modelled():
	"""Per corpus item: (item, the class matrix, both distance matrices over all columns)."""
	out = []
	for item in PM.corpus():
		cls = PM.classes(CM.matrix(item.g, item.rows, item.window))
		out.append((item, cls, PM.distances(cls), PM.distances(cls, acgt_only=True)))
	return out


# ---- the model -----------------------------------------------------------------------------------------------------------------------------

def test_only_the_variable_columns_count(modelled):
	"""Dropping the non-variable columns changes no entry, under both definitions, on every corpus item."""
	for item, cls, d_all, d_acgt in modelled:
		keep = PM.sites(CM.matrix(item.g, item.rows, item.window))
		assert np.array_equal(keep, (cls != cls[0]).any(axis=0)), item.name     # the column counts' "variable" is "not every class equal"
		assert np.array_equal(PM.distances(cls[:, keep]), d_all), item.name
		assert np.array_equal(PM.distances(cls[:, keep], acgt_only=True), d_acgt), item.name
		assert PM.distances(cls[:, ~keep]).sum() == 0, item.name


def test_the_model_is_a_distance(modelled):
	"""Symmetric with a zero diagonal; acgt <= all entry for entry; the definition spelled out pair by pair on a small item."""
	for item, cls, d_all, d_acgt in modelled:
		for d in (d_all, d_acgt):
			assert d.dtype == np.uint32 and np.array_equal(d, d.T) and (np.diag(d) == 0).all(), item.name
		assert (d_acgt <= d_all).all(), item.name
	item, cls, d_all, d_acgt = modelled[0]
	for i, j in itertools.product(range(len(item.rows)), repeat=2):
		assert d_all[i, j] == sum(1 for a, b in zip(cls[i], cls[j]) if a != b)
		assert d_acgt[i, j] == sum(1 for a, b in zip(cls[i], cls[j]) if a != b and a < 4 and b < 4)


def test_classes_follow_the_header():
	m = np.arange(256, dtype=np.uint8).reshape(1, 256)
	cls = PM.classes(m)[0]
	want = {ord("A"): 0, ord("a"): 0, ord("C"): 1, ord("c"): 1, ord("G"): 2, ord("g"): 2, ord("T"): 3, ord("t"): 3, ord("N"): 4, ord("n"): 4, ord("-"): 5}
	assert all(cls[b] == want.get(b, 6) for b in range(256))
	assert cls[0xC1] == cls[0xE1] == cls[0x0D] == cls[0x00] == 6
	# the counts of the column counts' model are the histogram of these classes
	g = CM.hostile_graph(0)
	mm = CM.matrix(g, CM.HOSTILE_ROWS)
	hist = np.stack([(PM.classes(mm) == k).sum(axis=0) for k in range(6)], axis=1)
	assert np.array_equal(hist, CM.counts(mm))


# ---- reach: what the GPU corpus holds --------------------------------------------------------------------------------------------------------

def test_the_corpus_cannot_hide_a_failure(modelled):
	differ = 0
	for item, cls, d_all, d_acgt in modelled:
		n, V = cls.shape[0], int((cls != cls[0]).any(axis=0).sum())
		if n >= 2 and V >= 1:
			off = d_all[~np.eye(n, dtype=bool)]
			assert off.any(), item.name
		differ += int(not np.array_equal(d_all, d_acgt))
	assert differ >= 1
	names = [item.name for item, *_ in modelled]
	assert len(set(names)) == len(names)
	# repeated rows occur, and both of a pair's entries are 0
	item, cls, d_all, _ = next(x for x in modelled if x[0].name == "sites_64")
	assert item.rows[4] == item.rows[8] and d_all[4, 8] == 0 and d_all[8, 4] == 0 and d_all[4].any()


def test_the_sites_graphs_hold_every_pair_of_classes():
	"""Every unordered pair of the seven classes stands in some column of the row-count graph and of the 64C-site graph."""
	T, C_ = PM.kernel_constants()
	for g, rows in ((PM.row_count_graph(), PM.row_count_rows(T)), (PM.sites_graph_of(64 * C_), PM.SITE_ROWS)):
		cls = PM.classes(CM.matrix(g, rows))
		seen = set()
		for col in cls.T:
			present = sorted(set(col.tolist()))
			seen.update(itertools.combinations(present, 2))
		assert seen == set(itertools.combinations(range(7), 2)), sorted(set(itertools.combinations(range(7), 2)) - seen)
		# a padding column: the REF row holds '-' where a two-byte label holds a class
		ref = CM.matrix(g, [PM.PLOIDY_MAX])[0]
		assert (ref == 0x2D).sum() == int(g.two_byte.sum()) > 0
		raw = set(CM.matrix(g, rows).reshape(-1).tolist())
		assert {ord("N"), ord("n"), ord("c"), ord("R"), 0xC1, ord("-")} <= raw


def test_the_corpus_reaches_the_counts_it_names():
	T, C_ = PM.kernel_constants()
	by_name = {item.name: item for item in PM.corpus()}
	for n in PM.row_counts():
		item = by_name["rows_%d" % n]
		assert len(item.rows) == n
		if n > 15:
			assert any(isinstance(r, list) for r in item.rows)          # rows with cuts among them
	assert max(PM.row_counts()) > 3 * T                                  # four tiles: an edge tile in both dimensions, ten tile pairs
	for V in PM.site_counts():
		item = by_name["sites_%d" % V]
		assert PM.expected(item.g, item.rows)[1] == V == PM.variable_columns(item.g)
	assert PM.expected(by_name["sites_0"].g, by_name["sites_0"].rows)[1] == 0
	assert {64 * C_ - 1, 64 * C_, 64 * C_ + 1, 63, 64, 65, 1} <= set(PM.site_counts())
	# the windows
	g = PM.window_graph()
	ws = PM.windows()
	assert {b % 4 for b, _ in ws} == set(range(4)) and {e % 4 for _, e in ws} == set(range(4))
	site = PM.sites(CM.matrix(g, PM.SITE_ROWS))
	assert any(site[b] for b, e in ws) and any(site[e - 1] for b, e in ws) and any(site[b] and site[e - 1] for b, e in ws)
	assert any(not site[b:e].any() for b, e in ws) and any(site[b:e].any() and not site[b] and not site[e - 1] for b, e in ws)


# ---- reach: the rows that all differ ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def distinct():
	"""Per distinct item: (item, the class matrix, both distance matrices)."""
	out = []
	for item in PM.distinct_items():
		cls = PM.classes(CM.matrix(item.g, item.rows))
		out.append((item, cls, PM.distances(cls), PM.distances(cls, acgt_only=True)))
	return out


def conjugated(d, perm):
	"""d with rows and columns taken through perm: what a kernel gives that takes row perm[i] for row i throughout."""
	return d[np.ix_(perm, perm)]


def near_miss_permutations(n):
	"""(name, perm) over n rows, each the identity beyond the full tiles: the row mix-ups a kernel can make that a corpus of period 16
	cannot see, and two of a shorter reach."""
	T, _ = PM.kernel_constants()
	full = n // T * T
	i = np.arange(n)
	out = []
	for bit in (1, 2, 16, 32):                                       # neighbouring rows, a lane's pair for its other pair, a row group for the next, the halves pair_row() splits a tile into
		out.append(("i ^ %d" % bit, np.where(i < full, i ^ bit, i)))
	for a, b in ((0, 1), (1, 2)):                                    # tile a taken for tile b and back
		p = i.copy()
		p[a * T:(a + 1) * T], p[b * T:(b + 1) * T] = i[b * T:(b + 1) * T], i[a * T:(a + 1) * T]
		out.append(("tiles %d and %d exchanged" % (a, b), p))
	out.append(("shifted by a row group of 16", np.where(i < full, (i + 16) % full, i)))
	for name, p in out:
		assert sorted(p.tolist()) == list(range(n)) and (p != i).any(), name
	return out


def test_the_distinct_rows_all_differ(distinct):
	T, C_ = PM.kernel_constants()
	import nj_tree_model
	_, B, J = nj_tree_model.kernel_constants()
	assert [len(item.rows) for item, *_ in distinct] == [3 * T + 1, 8 * T + 1, J * B + 64] == [193, 513, 1088]
	assert [(len(item.rows) + T - 1) // T for item, *_ in distinct] == [4, 9, 17]            # tiles: 10, 45 and 153 tile pairs
	for item, cls, d_all, d_acgt in distinct:
		n = len(item.rows)
		assert len(np.unique(cls, axis=0)) == n, item.name
		for d in (d_all, d_acgt):
			assert len(np.unique(d, axis=0)) == n, item.name
			assert np.array_equal(d, d.T) and (np.diag(d) == 0).all(), item.name
		assert d_all[~np.eye(n, dtype=bool)].all() and not np.array_equal(d_all, d_acgt), item.name
		assert item.rows[0] == PM.PLOIDY_MAX and 1 not in item.rows and sum(isinstance(r, list) for r in item.rows) == 3, item.name
	# the 3 T + 1 item lies over two chunks of sites and five more (the sites of the row-group tests)
	item = PM.distinct_item(3 * T + 1)
	assert PM.expected(item.g, item.rows)[1] == 2 * 64 * C_ + 5 == PM.variable_columns(item.g)
	assert 50 <= PM.expected(distinct[2][0].g, distinct[2][0].rows)[1] <= 70


def test_the_distinct_rows_tell_the_row_mix_ups_apart(distinct):
	"""Conjugating the expected matrix by each near-miss permutation changes it, under both definitions -- while the matrix of
	row_count_rows(3 T + 1), whose rows repeat with period 16, is the same bit for bit under i ^ 16 and i ^ 32: why these items exist."""
	T, _ = PM.kernel_constants()
	for item, cls, d_all, d_acgt in distinct[:2]:
		n = len(item.rows)
		for name, perm in near_miss_permutations(n):
			for d in (d_all, d_acgt):
				assert not np.array_equal(conjugated(d, perm), d), (item.name, name)
	n = 3 * T + 1
	rows = PM.row_count_rows(n)
	cls = PM.classes(CM.matrix(PM.row_count_graph(), rows))
	blind = dict(near_miss_permutations(n))
	for acgt in (False, True):
		d = PM.distances(cls, acgt)
		for name in ("i ^ 16", "i ^ 32", "tiles 1 and 2 exchanged"):
			assert np.array_equal(conjugated(d, blind[name]), d), name
		assert not np.array_equal(conjugated(d, blind["i ^ 1"]), d)


# ---- the text ------------------------------------------------------------------------------------------------------------------------------

def test_text():
	from vcf2multialign_amd import host
	g = CM.hostile_graph(0)
	rows = CM.HOSTILE_ROWS
	ids = ["REF"] + ["S.%d" % (1 + i) for i in range(len(rows) - 2)] + ["1"]
	for acgt in (False, True):
		d, V, L = PM.expected(g, rows, acgt_only=acgt)
		got = host.distances_text(ids, d, L, V, acgt)
		assert got == PM.text(ids, d, L, V, acgt) == PM.file_text(g, ids, rows, acgt_only=acgt)
		lines = got.decode().split("\n")
		assert lines[0] == "#rows\t9\tcolumns\t33\tsites\t3\tmodel\t%s" % ("acgt" if acgt else "all")
		assert lines[1] == "id\t" + "\t".join(ids) and lines[-1] == "" and len(lines) == 2 + 9 + 1
		assert lines[2].split("\t")[:2] == ["REF", "0"]
	# no rows, one row, the largest entry a u32 holds
	assert host.distances_text([], np.zeros((0, 0), np.uint32), 7, 0) == b"#rows\t0\tcolumns\t7\tsites\t0\tmodel\tall\nid\n" == PM.text([], np.zeros((0, 0)), 7, 0)
	assert host.distances_text(["x"], [[0]], 1, 0, True) == b"#rows\t1\tcolumns\t1\tsites\t0\tmodel\tacgt\nid\tx\nx\t0\n"
	big = np.array([[0, 4294967295], [4294967295, 0]], dtype=np.uint32)
	assert host.distances_text(["a", "b"], big, 4294967295, 4294967295) == PM.text(["a", "b"], big, 4294967295, 4294967295)
	with pytest.raises(ValueError):
		host.distances_text(["a\tb"], [[0]], 1, 0)


# ---- the header and the library --------------------------------------------------------------------------------------------------------------

def test_header_constants_and_prototypes():
	from vcf2multialign_amd import _native as N
	header = _header()
	assert re.search(r"#define V2M_DIST_ACGT_ONLY\s+0x20u", header) and N.DIST_ACGT_ONLY == 0x20
	assert re.search(r"#define V2M_PAIR_DISTANCES_MAX_ROWS\s+32768u", header) and N.PAIR_DISTANCES_MAX_ROWS == 32768 >= 20001
	assert "#define V2M_ABI_VERSION 5" in header and "V2M_KERNEL_END = 15" in header and "V2M_KERNEL_LIMIT = 17" in header
	assert "V2M_PAIR_DISTANCES_PLANE_BYTES" in header and "---- pair distances" in header
	assert header.index("---- column counts") < header.index("---- pair distances") < header.index("---- founder search")
	assert re.search(r"\bint v2m_pair_distances\(v2m_ctx \*ctx, const v2m_row_batch \*rows, uint32_t flags[^;]*?,\s*uint32_t \*dist[^;]*?, v2m_pair_distances_info \*info", header)
	assert re.search(r"\bint v2m_pair_distances_device\(v2m_ctx \*ctx, const v2m_row_batch \*rows, uint32_t flags[^;]*?,\s*void \*d_dist, uint64_t pitch\)", header)
	for name in ("v2m_pair_distances", "v2m_pair_distances_device"):
		assert name in N.SIGNATURES
	fields = re.search(r"typedef struct \{([^}]*)\} v2m_pair_distances_info;", header).group(1)
	assert re.findall(r"(\w+);", fields) == [f for f, _ in N.PairDistancesInfo._fields_] == ["n_sites", "n_columns", "n_passes", "counts_ms", "pack_ms", "pairs_ms"]
	assert C.sizeof(N.PairDistancesInfo) == 48
	assert (N.PAIR_TILE, N.PAIR_CHUNK_WORDS) == PM.kernel_constants()


def test_exported_symbols():
	from vcf2multialign_amd import build
	hip = C.CDLL(build.LIB_PATH)
	for name in ("v2m_pair_distances", "v2m_pair_distances_device"):
		assert hasattr(hip, name), name
	host = C.CDLL(build.HOST_LIB_PATH)
	assert hasattr(host, "v2mh_distances_text")
	out = subprocess.run(["nm", "-D", "--defined-only", build.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
	assert " T v2m_pair_distances\n" in out and " T v2m_pair_distances_device\n" in out


def test_the_kernels_are_in_the_library_source():
	with open(PM.DISTANCE_KERNELS_HPP) as f:
		text = f.read()
	for kernel in ("emit_site_columns_kernel", "pack_sites_kernel", "pair_distances_kernel"):
		assert re.search(r"__global__[^;{]*\b%s\(" % kernel, text), kernel
	with open(os.path.join(ROOT, "vcf2multialign_amd", "csrc", "v2m_hip.hip")) as f:
		assert '#include "distance_kernels.hpp"' in f.read()
	from vcf2multialign_amd import build
	assert PM.DISTANCE_KERNELS_HPP in build.deps("HIP_DEPS")


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
		r = _run(common + ["--output-distances=" + str(tmp_path / "x.tsv")] + extra, cwd=str(tmp_path))
		assert r.returncode != 0
		assert ("ERROR: --output-distances cannot be combined with %s.\n" % what).encode() in r.stderr, r.stderr.decode()
	r = _run(common + ["--acgt-only", "-s", str(tmp_path / "x.a2m")], cwd=str(tmp_path))
	assert r.returncode != 0 and b"ERROR: --acgt-only requires --output-distances.\n" in r.stderr
	assert not (tmp_path / "x.tsv").exists() and not (tmp_path / "x.a2m").exists()
	r = _run(["--help"])
	assert r.returncode == 0 and b"--output-distances=FILE" in r.stdout + r.stderr and b"--acgt-only" in r.stdout + r.stderr


def test_the_site_split_rule_the_gpu_test_assumes():
	"""tests/test_gpu_pair_distances.py: split_of() restates pair_chunks_per_part and the launch's part count; the header names the knob."""
	with open(os.path.join(ROOT, "vcf2multialign_amd", "csrc", "v2m_hip.hip")) as f:
		library = f.read()
	body = re.search(r"u64 pair_chunks_per_part\([^)]*\)\s*\{(.*?)\n\}", library, re.S).group(1)
	assert "std::min<u64>({n_chunks, forced ? forced : spread, 65535})" in body and "return (n_chunks + want_parts - 1) / want_parts;" in body
	assert "parts((chunks + per_part - 1) / per_part)" in library
	assert library.count('env_u64("V2M_PAIR_DISTANCES_PARTS"') == 1          # read once per call
	assert "V2M_PAIR_DISTANCES_PARTS" in _header()
	# the rows of a row group of pack_sites_kernel: the rule, and the knob that replaces it, read once per call
	assert "forced_site_group(forced_site_rows, std::max<u64>({16, (nr + want_groups - 1) / want_groups, (nr + 65534) / 65535}), nr)" in library
	assert library.count('u64 const forced_site_rows(env_u64("V2M_SITE_ROWS_PER_GROUP", 0));') == 1
	assert "return forced ? std::max<u64>(forced, (n + 65534) / 65535) : rule;" in library
	with open(PM.DISTANCE_KERNELS_HPP) as f:
		kernel = f.read()
	assert "n_chunks - chunk_begin < chunks_per_part ? n_chunks : chunk_begin + chunks_per_part" in kernel
