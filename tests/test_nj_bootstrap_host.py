"""The bootstrap without a GPU (include/v2m_hip.h, "bootstrap"): the draws of tests/nj_bootstrap_model.py against known values of
splitmix64 and against Python integers, the host library's split counting (csrc/nj_support.hpp) against the model's frozensets, the
support text, the header, the symbols, the Python surface, the driver's argument errors, and what the GPU tests' corpus holds."""

import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import nj_bootstrap_model as BM
import nj_tree_model as M
import pair_distances_model as PM

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")


# ---- the draws -------------------------------------------------------------------------------------------------------------------------------

def test_mix_is_splitmix64s_finaliser():
	# splitmix64 seeded with 0 returns mix(G), mix(2 G), mix(3 G), mix(4 G): the published first outputs
	assert [BM.mix(k * BM.G) for k in (1, 2, 3, 4)] == [0xE220A8397B1DCDAF, 0x6E789E6AA1B965F4, 0x06C45D188009454F, 0xF88BB8A8724C81EC]
	assert BM.mix(0) == 0 and BM.key_of(0) == 0xE220A8397B1DCDAF and BM.key_of(BM.MASK) == BM.mix(BM.G - 1)
	# one step by hand: z = 1 -> (1 ^ 0) * c1 = c1; then (c1 ^ (c1 >> 27)) * c2; then ^ (>> 31)
	c1, c2 = 0xBF58476D1CE4E5B9, 0x94D049BB133111EB
	z = ((c1 ^ (c1 >> 27)) * c2) % (1 << 64)
	assert BM.mix(1) == z ^ (z >> 31)


@pytest.mark.parametrize("seed", BM.SEEDS)
@pytest.mark.parametrize("r", BM.REPLICATES)
def test_draws_by_halves_equal_python_integers(seed, r):
	for L in (1, 2, 3, 255, 256, 257, 1000):
		got = BM.draws(seed, r, L)
		assert got.dtype == np.uint64 and got.shape == (L,) and int(got.max()) < L
		assert [int(x) for x in got] == [BM.draw_int(seed, r, k, L) for k in range(L)], (seed, r, L)
		w = BM.weights(seed, r, L)
		assert w.dtype == np.uint32 and w.shape == (L,) and int(w.sum()) == L
	assert not BM.draws(seed, r, 1).any() and BM.weights(seed, r, 1).tolist() == [1] and BM.weights(seed, r, 0).shape == (0,)
	# L = 2^32 - 1: the product by halves at the top of its range, on the draws the definition allows (k < L), first and last
	L = (1 << 32) - 1
	with np.errstate(over="ignore"):
		k = np.array([0, 1, 2, L - 2, L - 1], dtype=np.uint64)
		x = BM._mix_np(np.uint64(BM.key_of(seed)) + ((np.uint64(r << 32) | k) + np.uint64(1)) * np.uint64(BM.G))
		got = ((x >> np.uint64(32)) * np.uint64(L) + (((x & np.uint64(0xFFFFFFFF)) * np.uint64(L)) >> np.uint64(32))) >> np.uint64(32)
	assert [int(v) for v in got] == [BM.draw_int(seed, r, int(i), L) for i in k]


def test_replicates_and_seeds_differ():
	L = 500
	seen = {BM.draws(seed, r, L).tobytes() for seed in BM.SEEDS for r in BM.REPLICATES}
	assert len(seen) == len(BM.SEEDS) * len(BM.REPLICATES)


# ---- the split counting ------------------------------------------------------------------------------------------------------------------------

def _trees(n, seeds):
	return [M.nj(M.path_noise(n, s)) for s in seeds]


def _support(main, trees):
	from vcf2multialign_amd import host
	return host.nj_split_support(main, np.stack(trees) if trees else np.zeros((0, len(main)), dtype=M.NODE_DTYPE))


@pytest.mark.parametrize("n", (3, 4, 5, 63, 64, 65, 129))
def test_split_support_against_the_model(n):
	main, *others = _trees(n, range(100, 106))
	trees = others + [main]
	got = _support(main, trees)
	want = BM.support(main, trees, n)
	assert got.dtype == np.uint32 and got.shape == (max(0, n - 3),) and np.array_equal(got, want)
	if n > 3:
		assert int(got.min()) >= 1                                       # (the main tree is among them)
	assert np.array_equal(_support(main, [main] * 7), np.full(n - 3, 7))    # a replicate equal to the main tree: all B
	assert np.array_equal(_support(main, []), np.zeros(n - 3))


def test_additive_trees_share_their_splits_under_noise():
	# the corpus cannot hide a failure: a support strictly between 0 and B, one of B and one of 0 occur
	n = 40
	base = M.random_insertion(n, 5, top=1000).astype(np.int64)
	rng = np.random.default_rng(9)
	trees = []
	for _ in range(12):
		noise = np.triu(rng.integers(0, 220, size=(n, n)), 1)
		trees.append(M.nj((base + noise + noise.T).astype(np.uint32)))
	main = M.nj(base.astype(np.uint32))
	got = _support(main, trees)
	assert np.array_equal(got, BM.support(main, trees, n))
	assert (got == 12).any() and ((got > 0) & (got < 12)).any() and (got == 0).any(), got


def _records(n, joins, last):
	nodes = np.zeros(n - 2, dtype=M.NODE_DTYPE)
	for t, (a, b) in enumerate(joins):
		nodes[t] = (a, b, M.NONE, 0, 1.0, 1.0, 0.0)
	nodes[n - 3] = (*last, 0, 1.0, 1.0, 1.0)
	return nodes


def test_a_split_is_one_value_on_either_side_and_in_any_order():
	# six leaves; splits {0,1} | rest and {4,5} | rest.  One tree holds {0,1} as a join node, the other as the complement {2,3,4,5}.
	a = _records(6, [(0, 1), (4, 5), (2, 6)], (3, 7, 8))                  # nodes: 6 = {0,1}; 7 = {4,5}; 8 = {0,1,2}
	b = _records(6, [(4, 5), (3, 6), (2, 7)], (0, 1, 8))                  # nodes: 6 = {4,5}; 7 = {3,4,5}; 8 = {2,3,4,5} = not {0,1}
	assert BM.splits(a, 6) == [frozenset({2, 3, 4, 5}), frozenset({4, 5}), frozenset({3, 4, 5})]
	assert set(BM.splits(b, 6)) == set(BM.splits(a, 6))
	assert _support(a, [b]).tolist() == [1, 1, 1] and _support(b, [a, a]).tolist() == [2, 2, 2]
	# the same tree with its joins in another order
	c = _records(6, [(4, 5), (0, 1), (2, 7)], (3, 6, 8))
	assert _support(a, [c]).tolist() == [1, 1, 1] == BM.support(a, [c], 6).tolist()
	# a tree sharing no split: {0,2}, {1,4}, {0,2,3}... against a's
	d = _records(6, [(0, 2), (1, 4), (3, 6)], (5, 7, 8))
	assert not set(BM.splits(d, 6)) & set(BM.splits(a, 6))
	assert _support(a, [d, d]).tolist() == [0, 0, 0] and _support(a, [d, b, c]).tolist() == [2, 2, 2]


def test_malformed_records_are_refused():
	from vcf2multialign_amd import host
	good = _records(6, [(0, 1), (4, 5), (2, 6)], (3, 7, 8))
	for bad in (
		_records(6, [(0, 1), (4, 5), (2, 9)], (3, 7, 8)),       # a node that is not made yet
		_records(6, [(0, 1), (0, 5), (2, 6)], (3, 7, 8)),       # a leaf joined twice
		_records(6, [(0, 1), (4, 5), (2, 6)], (3, 7, 7)),       # a node joined twice
		_records(6, [(0, 1), (4, 5), (2, 6)], (3, 7, M.NONE)),  # the last record has two children
	):
		for main, reps in ((bad, [good]), (good, [good, bad])):
			with pytest.raises(ValueError):
				_support(main, reps)
	early = good.copy()
	early[1]["c"] = 3                                            # three children before the last record
	with pytest.raises(ValueError):
		_support(early, [good])
	lib = host._load()
	s = np.zeros(3, dtype=np.uint32)
	assert -1 == lib.v2mh_nj_split_support(6, None, good.ctypes.data, 1, s.ctypes.data)
	assert -1 == lib.v2mh_nj_split_support(6, good.ctypes.data, None, 1, s.ctypes.data)
	assert -1 == lib.v2mh_nj_split_support(6, good.ctypes.data, good.ctypes.data, 1, None)
	assert -1 == lib.v2mh_nj_split_support(2, good.ctypes.data, good.ctypes.data, 1, s.ctypes.data)
	assert 0 == lib.v2mh_nj_split_support(6, good.ctypes.data, good.ctypes.data, 1, s.ctypes.data) and s.tolist() == [1, 1, 1]


# ---- the text --------------------------------------------------------------------------------------------------------------------------------

def test_support_text_and_its_quoting():
	from vcf2multialign_amd import host
	a = _records(6, [(0, 1), (4, 5), (2, 6)], (3, 7, 8))
	labels = ["REF", "s.1", "it's", "a_b", "", "x-2"]
	got = host.nj_newick_support_text(a, labels, [87, 0, 4294967295])
	assert got == b"('a_b':1,('':1,x-2:1)0:1,('it''s':1,(REF:1,s.1:1)87:1)4294967295:1);\n"
	assert got == BM.newick_support(a, labels, [87, 0, 4294967295])
	assert re.sub(rb"\)\d+:", b"):", got) == host.nj_newick_text(a, labels) == M.newick(a, labels)
	three = _records(3, [], (0, 1, 2))
	assert host.nj_newick_support_text(three, ["a", "b", "c"], []) == host.nj_newick_text(three, ["a", "b", "c"]) == b"(a:1,b:1,c:1);\n"
	for n in (4, 33):
		nodes = M.nj(M.path_noise(n, n))
		counts = np.arange(n - 3, dtype=np.uint32) * 7
		labels = ["t%d" % k for k in range(n)]
		assert host.nj_newick_support_text(nodes, labels, counts) == BM.newick_support(nodes, labels, counts)
	with pytest.raises(ValueError):
		host.nj_newick_support_text(a, labels[:5], [1, 2, 3])
	with pytest.raises(ValueError):
		host.nj_newick_support_text(a, ["a"] * 6, [1, 2])
	bad = _records(6, [(0, 1), (0, 5), (2, 6)], (3, 7, 8))
	with pytest.raises(ValueError):
		host.nj_newick_support_text(bad, ["a"] * 6, [1, 2, 3])


# ---- the header, the libraries, the Python surface ---------------------------------------------------------------------------------------------

def _header():
	with open(os.path.join(ROOT, "include", "v2m_hip.h")) as f:
		return f.read()


def test_header_constants_types_and_prototypes():
	from vcf2multialign_amd import _native as N
	header = _header()
	assert re.search(r"#define V2M_NJ_BOOTSTRAP_MAX_REPLICATES\s+100000u", header) and N.NJ_BOOTSTRAP_MAX_REPLICATES == 100000
	assert "#define V2M_ABI_VERSION 5" in header and "V2M_KERNEL_END = 15" in header and "V2M_KERNEL_LIMIT = 17" in header and N.ABI_VERSION == 5
	assert header.index("---- neighbour joining") < header.index("---- bootstrap") < header.index("---- founder search")
	assert re.search(r"\bint v2m_pair_distances_weighted\(v2m_ctx \*ctx, const v2m_row_batch \*rows, uint32_t flags[^;]*?,\s*const uint32_t \*weights[^;]*?, uint32_t \*dist[^;]*?,\s*v2m_pair_distances_info \*info[^;]*?\);", header)
	assert re.search(r"\bint v2m_bootstrap_distances\(v2m_ctx \*ctx, const v2m_row_batch \*rows, uint32_t flags[^;]*?, uint64_t seed, uint32_t replicate,\s*uint32_t \*dist[^;]*?, v2m_pair_distances_info \*info[^;]*?\);", header)
	assert re.search(r"\bint v2m_nj_bootstrap\(v2m_ctx \*ctx, const v2m_row_batch \*rows, uint32_t flags[^;]*?, uint32_t n_replicates, uint64_t seed,\s*v2m_nj_node \*nodes[^;]*?, uint32_t \*support[^;]*?,\s*v2m_nj_node \*replicate_nodes[^;]*?, v2m_nj_bootstrap_info \*info[^;]*?\);", header)
	for name in ("v2m_pair_distances_weighted", "v2m_bootstrap_distances", "v2m_nj_bootstrap"):
		assert name in N.SIGNATURES
	info = re.search(r"typedef struct \{([^}]*)\} v2m_nj_bootstrap_info;", header).group(1)
	assert re.findall(r"(\w+);", info) == [f for f, _ in N.NjBootstrapInfo._fields_] == ["n_rows", "n_sites", "n_columns", "n_passes", "n_pack_passes",
		"n_replicates", "max_slices", "distances_ms", "weights_ms", "pairs_ms", "trees_ms"]
	assert C.sizeof(N.NjBootstrapInfo) == 88
	assert "0x9E3779B97F4A7C15" in header and "0xBF58476D1CE4E5B9" in header and "0x94D049BB133111EB" in header
	assert (N.BOOT_DRAW_THREADS, N.BOOT_SLICES) == BM.kernel_constants() and N.BOOT_SLICES == 32


def test_exported_symbols():
	from vcf2multialign_amd import build
	hip = C.CDLL(build.LIB_PATH)
	for name in ("v2m_pair_distances_weighted", "v2m_bootstrap_distances", "v2m_nj_bootstrap"):
		assert hasattr(hip, name), name
	out = subprocess.run(["nm", "-D", "--defined-only", build.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
	assert " T v2m_pair_distances_weighted\n" in out and " T v2m_bootstrap_distances\n" in out and " T v2m_nj_bootstrap\n" in out
	out = subprocess.run(["nm", "-D", "--defined-only", build.HOST_LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
	assert " T v2mh_nj_split_support\n" in out and " T v2mh_nj_newick_support_text\n" in out


def test_the_kernels_are_in_the_library_source():
	with open(BM.BOOTSTRAP_KERNELS_HPP) as f:
		text = f.read()
	for kernel in ("bootstrap_weights_kernel", "gather_site_weights_kernel", "weight_slices_kernel", "pair_distances_weighted_kernel"):
		assert re.search(r"__global__[^;{]*\b%s\(" % kernel, text), kernel
	# every LDS object of the header goes through the checked build's poison
	for name in re.findall(r"__shared__[^;]*?\b(\w+)\[", text):
		assert "V2M_POISON_LDS(%s);" % name in text, name
	with open(os.path.join(ROOT, "vcf2multialign_amd", "csrc", "v2m_hip.hip")) as f:
		library = f.read()
	assert library.index('#include "distance_kernels.hpp"') < library.index('#include "bootstrap_kernels.hpp"')
	assert '#include "nj_support.hpp"' in library
	buffers = re.search(r"scratch_buf (d_boot_[^;]*);", library).group(1)
	assert sorted(b.strip() for b in buffers.split(",")) == sorted({m for m in re.findall(r"\bd_boot_\w+", library)})   # every new device buffer is a scratch_buf
	with open(os.path.join(ROOT, "vcf2multialign_amd", "csrc", "nj_support.hpp")) as f:
		support = f.read()
	assert "hip" not in re.sub(r"//[^\n]*", "", support).replace("v2m_hip.h", "").lower()        # plain C++
	from vcf2multialign_amd import build
	assert BM.BOOTSTRAP_KERNELS_HPP in build.deps("HIP_DEPS") and os.path.join(ROOT, "vcf2multialign_amd", "csrc", "nj_support.hpp") in build.deps("HIP_DEPS")
	assert os.path.join(ROOT, "vcf2multialign_amd", "csrc", "nj_support.hpp") in build.deps("HOST_DEPS")


def test_python_surface():
	import vcf2multialign_amd as v2m
	from vcf2multialign_amd import host, output
	assert list(inspect.signature(v2m.Context.pair_distances_weighted).parameters) == ["self", "rows", "weights", "acgt_only", "info"]
	assert list(inspect.signature(v2m.Context.bootstrap_distances).parameters) == ["self", "rows", "seed", "replicate", "acgt_only", "info"]
	assert list(inspect.signature(v2m.Context.nj_bootstrap).parameters) == ["self", "rows", "n_replicates", "seed", "acgt_only", "replicates", "info"]
	assert list(inspect.signature(host.nj_split_support).parameters) == ["main_nodes", "replicate_nodes"]
	assert list(inspect.signature(host.nj_newick_support_text).parameters) == ["nodes", "labels", "support"]
	assert list(inspect.signature(output.HaplotypeOutput.output_tree_bootstrap).parameters) == ["self", "graph", "stream", "bootstrap", "seed", "replicates_path", "acgt_only"]
	assert list(inspect.signature(output.FounderSequenceGreedyOutput.output_tree_bootstrap).parameters) == ["self", "graph", "cut_positions", "assigned_samples_column_major",
		"stream", "bootstrap", "seed", "replicates_path", "acgt_only"]


# ---- the driver's argument errors (reported before a device is opened) ---------------------------------------------------------------------------

def _run(args, cwd=None):
	assert os.path.exists(CLI), "build the host driver first (__graft_entry__.build())"
	return subprocess.run([CLI] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_cli_argument_errors(tmp_path):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	bed = tmp_path / "r.bed"
	bed.write_text("1\t0\t4\n")
	common = ["-H", "-r", fa, "-a", vcf, "-c", "1"]
	tree = "--output-tree=" + str(tmp_path / "x.nwk")
	r = _run(common + ["--tree-bootstrap=10", "-s", str(tmp_path / "x.a2m")], cwd=str(tmp_path))
	assert r.returncode != 0 and b"ERROR: --tree-bootstrap requires --output-tree.\n" in r.stderr
	r = _run(common + [tree, "--tree-seed=3"], cwd=str(tmp_path))
	assert r.returncode != 0 and b"ERROR: --tree-seed requires --tree-bootstrap.\n" in r.stderr
	r = _run(common + [tree, "--output-tree-replicates=" + str(tmp_path / "r.nwk")], cwd=str(tmp_path))
	assert r.returncode != 0 and b"ERROR: --output-tree-replicates requires --tree-bootstrap.\n" in r.stderr
	for value in ("0", "100001", "-1", "ten", "", "1.5"):
		r = _run(common + [tree, "--tree-bootstrap=" + value], cwd=str(tmp_path))
		assert r.returncode != 0 and b"ERROR: --tree-bootstrap must be a number of replicates from 1 to 100000" in r.stderr, (value, r.stderr.decode())
	for value in ("18446744073709551616", "-1", "x", ""):
		r = _run(common + [tree, "--tree-bootstrap=10", "--tree-seed=" + value], cwd=str(tmp_path))
		assert r.returncode != 0 and b"ERROR: --tree-seed must be a number from 0 to 18446744073709551615" in r.stderr, (value, r.stderr.decode())
	# each flag is refused where --output-tree is
	for extra, what in ((["--regions-file=" + str(bed)], "--regions-file"), (["--device=0,0"], "more than one --device entry")):
		r = _run(common + [tree, "--tree-bootstrap=10", "--tree-seed=18446744073709551615", "--output-tree-replicates=" + str(tmp_path / "r.nwk")] + extra, cwd=str(tmp_path))
		assert r.returncode != 0 and ("ERROR: --output-tree cannot be combined with %s.\n" % what).encode() in r.stderr, r.stderr.decode()
	r = _run(["-F", "1", "-r", fa, "-a", vcf, "-c", "1", tree, "--tree-bootstrap=10"], cwd=str(tmp_path))
	assert r.returncode != 0 and b"ERROR: --output-tree needs at least three sequences (got 2).\n" in r.stderr
	assert not (tmp_path / "x.nwk").exists() and not (tmp_path / "r.nwk").exists() and not (tmp_path / "x.a2m").exists()
	r = _run(["--help"])
	assert r.returncode == 0 and all(flag in r.stdout + r.stderr for flag in (b"--tree-bootstrap=B", b"--tree-seed=S", b"--output-tree-replicates=FILE"))


# ---- what the GPU tests' corpus holds ----------------------------------------------------------------------------------------------------------

def test_the_corpus_cannot_hide_a_failure():
	n, B, seed = 5, 36, 1
	item = BM.tree_item(n)
	main, trees, counts = BM.bootstrap(item, B, seed)
	plain = PM.expected(item.g, item.rows)[0]
	matrices = [BM.expected_replicate(item, seed, r) for r in range(B)]
	assert all(not np.array_equal(m, plain) for m in matrices[:6]) and len({m.tobytes() for m in matrices}) == B
	L = item.g.aligned_length
	is_site = BM.site_mask(item)
	w = BM.weights(seed, 0, L)
	assert int(w[is_site].max()) >= 2 and int(w[is_site].min()) == 0
	# over the tree items: a support strictly between 0 and B, one of B and one of 0
	seen = []
	for n in BM.tree_row_counts():
		for B in BM.replicates_of(n):
			if n > 3:
				seen += [(int(c), B) for c in BM.bootstrap(BM.tree_item(n), B, seed)[2]]
	assert any(0 < c < B for c, B in seen) and any(c == B for c, B in seen) and any(c == 0 for c, B in seen), seen
	# the explicit-weight items reach K = 1, 2, 31, 32 (and 0)
	reached = set()
	for V in PM.site_counts():
		reached |= {K for _, _, K in BM.explicit_patterns(PM.Item("sites_%d" % V, PM.sites_graph_of(V), PM.SITE_ROWS))}
	assert {0, 1, 2, 31, 32} <= reached, reached
	# all-ones weights are the plain distances, and a non-site column's weight adds nothing
	item = PM.Item("sites_65", PM.sites_graph_of(65), PM.SITE_ROWS)
	for acgt in (False, True):
		assert np.array_equal(BM.expected_weighted(item, np.ones(item.g.aligned_length, dtype=np.uint32), acgt), PM.expected(item.g, item.rows, None, acgt)[0])
	item = PM.Item("window_graph", PM.window_graph(), PM.SITE_ROWS)              # (a site every five columns)
	name, w, K = next(p for p in BM.explicit_patterns(item) if p[0] == "non_sites")
	on_sites = np.where(BM.site_mask(item), w, 0)
	assert (w != on_sites).any() and np.array_equal(BM.expected_weighted(item, w), BM.expected_weighted(item, on_sites))
