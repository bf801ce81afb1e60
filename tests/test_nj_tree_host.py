"""The neighbour-joining tree without a GPU: the host library's plain-loop restatement (v2mh_nj_tree_cpu) held to the numpy model of
tests/nj_tree_model.py byte for byte, the model held to exact arithmetic and to the additive matrices themselves, the conditions that keep
the corpus of tests/test_gpu_nj_tree.py from hiding a failure, the Newick text, the header's constants, types and prototypes, the
exported symbols, the Python surface and the driver's argument errors."""

import ctypes as C
import io
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import nj_tree_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")


def _header():
	with open(os.path.join(ROOT, "include", "v2m_hip.h")) as f:
		return f.read()


# ---- the restatement and the models ----------------------------------------------------------------------------------------------------------

def test_the_restatement_equals_the_model_byte_for_byte():
	from vcf2multialign_amd import host
	differing = [item.name for item in M.corpus() if host.nj_tree_cpu(item.d).tobytes() != M.expected(item.name).tobytes()]
	assert not differing, differing
	# only the upper triangle is read, and a pitch of its own is honoured
	item = next(i for i in M.corpus() if i.name == "path_noise_101_1")
	hostile = np.full((item.n, item.n + 3), 0xDEADBEEF, dtype=np.uint32)
	upper = np.triu_indices(item.n, 1)
	hostile[upper] = item.d[upper]
	nodes = np.zeros(item.n - 2, dtype=M.NODE_DTYPE)
	lib = host._load()
	assert 0 == lib.v2mh_nj_tree_cpu(hostile.ctypes.data, item.n, item.n + 3, nodes.ctypes.data)
	assert nodes.tobytes() == M.expected(item.name).tobytes()
	assert -1 == lib.v2mh_nj_tree_cpu(hostile.ctypes.data, 2, 5, nodes.ctypes.data) and -1 == lib.v2mh_nj_tree_cpu(hostile.ctypes.data, 5, 4, nodes.ctypes.data)
	with pytest.raises(ValueError):
		host.nj_tree_cpu(np.zeros((2, 2)))


def test_the_records_have_the_headers_shape():
	for item in M.corpus():
		nodes, n = M.expected(item.name), item.n
		assert len(nodes) == n - 2 and nodes.dtype.itemsize == 40
		assert (nodes["reserved"] == 0).all() and (nodes["c"][:-1] == M.NONE).all() and (nodes["len_c"][:-1] == 0).all()
		assert (nodes["a"] < nodes["b"]).all() and nodes["b"][-1] < nodes["c"][-1] < 2 * n - 3
		children = sorted(nodes["a"].tolist() + nodes["b"].tolist() + [int(nodes["c"][-1])])
		assert children == list(range(2 * n - 3)), item.name               # every node but the last is joined exactly once
		assert all(max(nd["a"], nd["b"]) < n + t for t, nd in enumerate(nodes[:-1]))


def test_additive_matrices_come_back_exactly():
	"""On an additive matrix the float model equals the exact model (every operation is exact there), and, with no model at all, the
	branch lengths of the result add up to the matrix between every two leaves."""
	additive = [item for item in M.corpus() if item.additive]
	assert len(additive) >= 720 + 8 and {"caterpillar_12", "balanced_16", "inserted_20"} <= {i.name for i in additive}
	for item in additive:
		nodes = M.expected(item.name)
		if item.n <= 40:
			assert M.records_of_exact(M.nj_exact(item.d)).tobytes() == nodes.tobytes(), item.name
		back = M.leaf_distances(nodes, item.n)
		assert all(back[i][j] == int(item.d[i, j]) for i in range(item.n) for j in range(item.n)), item.name
	# branches of length 0 are among them, at a leaf and inside
	six = M.expected("six_000")
	assert 0.0 in (six["len_a"].tolist() + six["len_b"].tolist()) and six["len_c"][-1] == 0.0
	# and the exact model is not the float model everywhere: the noise rounds
	item = next(i for i in M.corpus() if i.name == "path_noise_101_1")
	back = M.leaf_distances(M.expected(item.name), item.n)
	assert any(back[0][j] != int(item.d[0, j]) for j in range(item.n))


def test_the_six_leaf_tree_puts_the_joined_slots_everywhere():
	"""Under the 720 relabelings of the six-leaf tree either joined slot of the first join is the first slot, the last live slot, or
	neither; every relabeling gives the same tree."""
	places = set()
	for k in range(720):
		nodes = M.expected("six_%03d" % k)
		a, b = int(nodes["a"][0]), int(nodes["b"][0])
		places.add(("first" if a == 0 else "inside", "last" if b == 5 else "inside"))
	assert places == {("first", "last"), ("first", "inside"), ("inside", "last"), ("inside", "inside")}


# ---- reach: what the corpus holds --------------------------------------------------------------------------------------------------------------

def test_the_corpus_reaches_the_counts_it_names():
	W, B, J = M.kernel_constants()
	from vcf2multialign_amd import _native as N
	assert (W, B, J) == (N.NJ_ROWS_PER_GROUP, N.NJ_JOIN_THREADS, N.NJ_JOIN_BATCH)
	by_n = {item.n for item in M.corpus()}
	assert {3, 4, 5, W - 1, W, W + 1, B - 1, B, B + 1, 2 * B + 1} <= by_n and max(by_n) == 2 * B + 1
	names = [item.name for item in M.corpus()]
	assert len(set(names)) == len(names)
	for n, seed in M.PATH_NOISE_SEEDS:
		assert 100 <= n <= 180
		d = M.path_noise(n, seed)
		assert np.array_equal(d, d.T) and int(d.max()) < (1 << 31) + (1 << 12)
	for item in M.corpus():
		assert item.d.dtype == np.uint32 and np.array_equal(item.d, item.d.T) and not np.diag(item.d).any(), item.name
	assert graph_items_hold_what_the_issue_names()


def graph_items_hold_what_the_issue_names():
	import pair_distances_model as PM
	items = M.graph_items()
	assert any(item.window for item in items) and any(item.window is None for item in items)
	assert all(len(item.rows) >= 3 for item in items)
	assert any(PM.PLOIDY_MAX in [r for r in item.rows if not isinstance(r, list)] for item in items)
	assert any(len({repr(r) for r in item.rows}) < len(item.rows) for item in items)      # repeated rows
	return True


# ---- beyond one batch of the join kernel ---------------------------------------------------------------------------------------------------------

def replay_slots(nodes, n):
	"""Per join of the records, in order: (r, p, q) -- the live slots before it and the two joined slots, p < q -- by the library's rule
	for the slots: the new node takes the lower slot, the taxon of the last live slot moves into the other."""
	slot_of = {k: k for k in range(n)}
	taxon_in = list(range(n))
	out = []
	for t in range(n - 3):
		r = n - t
		sa, sb = slot_of.pop(int(nodes["a"][t])), slot_of.pop(int(nodes["b"][t]))
		p, q, last = min(sa, sb), max(sa, sb), r - 1
		assert q <= last
		out.append((r, p, q))
		taxon_in[p] = n + t
		slot_of[n + t] = p
		if q != last:
			taxon_in[q] = taxon_in[last]
			slot_of[taxon_in[q]] = q
	assert sorted(slot_of.values()) == [0, 1, 2]
	return out


def test_the_join_batch_items_fill_a_batch_and_pass_it():
	"""nj_join_kernel takes the live slots J B at a time, slot e B + lane element e of a lane's batch.  The three sizes, the
	restatement against the model at each, and on the largest the joins the GPU test is there for: in the second trip slots of the
	first trip are updated and moved into, and a slot of the second trip is joined."""
	from vcf2multialign_amd import host
	_, B, J = M.kernel_constants()
	items = M.join_batch_items()
	assert [item.n for item in items] == [(J - 1) * B + 1, J * B, J * B + 64] == [769, 1024, 1088]
	assert not {item.name for item in items} & {item.name for item in M.corpus()}
	for item in items:
		assert item.d.dtype == np.uint32 and np.array_equal(item.d, item.d.T) and not np.diag(item.d).any(), item.name
		assert host.nj_tree_cpu(item.d).tobytes() == M.expected(item.name).tobytes(), item.name
	large = items[-1]
	joins = replay_slots(M.expected(large.name), large.n)
	second_trip = [(r, p, q) for r, p, q in joins if r > J * B]
	assert len(second_trip) == 64
	both_below = sum(1 for r, p, q in second_trip if q < J * B and q != r - 1)          # every lane of the second trip updates column p and moves into column q
	one_above = sum(1 for r, p, q in second_trip if q >= J * B)
	last_element = [(r, p, q) for r, p, q in joins if J * B >= r > (J - 1) * B]
	last_above = sum(1 for r, p, q in last_element if q >= (J - 1) * B)
	print("joins with r > J B: %d with both slots below J B and q not the last, %d with a slot at or above J B; with J B >= r > (J - 1) B: %d with a slot at or above (J - 1) B"
		% (both_below, one_above, last_above))
	assert both_below >= 1 and one_above >= 1 and len(last_element) == B and last_above >= 1


def test_every_step_of_the_equal_matrix_is_a_full_tie():
	trace = []
	M.nj(next(i for i in M.corpus() if i.name == "all_equal_9").d, trace=trace)
	assert [len(pairs) for pairs in trace] == [r * (r - 1) // 2 for r in range(9, 3, -1)]
	trace = []
	M.nj(next(i for i in M.corpus() if i.name == "all_zero_10").d, trace=trace)
	assert [len(pairs) for pairs in trace] == [r * (r - 1) // 2 for r in range(10, 3, -1)]
	# a leaf pair ties with a pair that holds an internal node, and the pair of the lower id wins
	trace = []
	nodes = M.nj(M.TIE_LEAF_INTERNAL, trace=trace)
	assert trace[1] == [(0, 1), (4, 5)] and (int(nodes["a"][1]), int(nodes["b"][1])) == (0, 1)
	# groups of identical taxa tie as well
	trace = []
	M.nj(next(i for i in M.corpus() if i.name == "groups_4_4_4").d, trace=trace)
	assert max(len(pairs) for pairs in trace) > 1


@pytest.mark.parametrize("variant", [dict(tie="slot"), dict(ru="fma"), dict(rk="alt"), dict(qsum="alt")], ids=lambda v: "%s=%s" % next(iter(v.items())))
def test_the_corpus_cannot_hide_a_failure(variant):
	"""Each near miss of the definition changes the records of at least one corpus item (of the items up to 300 taxa: enough, and
	quick).  A contracted product in Q is not among them: nj(qsum="fma") changed no record of the 48 items up to 180 taxa it was
	tried on, which is why tests/test_nj_kernel_isa.py looks for it in the instructions."""
	items = [item for item in M.corpus() if item.n <= 300 and not (item.name.startswith("six_") and int(item.name[4:]) % 60)]
	changed = [item.name for item in items if M.nj(item.d, **variant).tobytes() != M.expected(item.name).tobytes()]
	assert changed, variant
	if "ru" in variant:          # the family and the sizes the check was made on
		assert sum(name.startswith("path_noise_1") for name in changed) >= 4
	if "tie" in variant:
		assert any(name.startswith("all_equal") for name in changed)


# ---- the text ---------------------------------------------------------------------------------------------------------------------------------

def test_newick_text():
	from vcf2multialign_amd import host
	nodes = M.expected("caterpillar_12")
	labels = ["REF", "S.1", "S-2", "a_b", "it's", "", "x y", "(p)", "q:r", "s,t", "u;v", "Z9"]
	text = host.nj_newick_text(nodes, labels)
	assert text == M.newick(nodes, labels)
	s = text.decode()
	assert s.endswith(");\n") and s.count("(") == s.count(")") == 10 + 3 - 2
	for bare in ("REF:", "S.1:", "S-2:", "Z9:"):
		assert bare in s and "'" + bare[:-1] + "'" not in s
	for quoted in ("'a_b':", "'it''s':", "'':", "'x y':", "'(p)':", "'q:r':", "'s,t':", "'u;v':"):
		assert quoted in s
	# three taxa, and negative lengths kept
	three = np.zeros(1, dtype=M.NODE_DTYPE)
	three[0] = (0, 1, 2, 0, -1.5, 0.1, 1e-20)
	assert host.nj_newick_text(three, ["a", "b", "c"]) == b"(a:-1.5,b:0.1,c:1e-20);\n" == M.newick(three, ["a", "b", "c"])
	d = np.array([[0, 10, 1], [10, 0, 1], [1, 1, 0]], dtype=np.uint32)
	assert host.nj_newick_text(M.nj(d), ["a", "b", "c"]) == b"(a:5,b:5,c:-4);\n"
	# %.10g
	three[0] = (0, 1, 2, 0, 1 / 3, 123456789012.0, 2.5)
	assert host.nj_newick_text(three, ["a", "b", "c"]) == b"(a:0.3333333333,b:1.23456789e+11,c:2.5);\n"
	# depth 2 000: a caterpillar joined from one end, without recursion on either side
	n = 2003
	deep = np.zeros(n - 2, dtype=M.NODE_DTYPE)
	deep[0] = (0, 1, M.NONE, 0, 1.0, 2.0, 0.0)
	for t in range(1, n - 3):
		deep[t] = (t + 1, n + t - 1, M.NONE, 0, 1.0, 2.0, 0.0)          # the next leaf and the node made before
	deep[n - 3] = (n - 2, n - 1, 2 * n - 4, 0, 1.0, 1.0, 3.0)
	labels = ["L%d" % k for k in range(n)]
	text = host.nj_newick_text(deep, labels)
	assert text == M.newick(deep, labels) and text.count(b"(") == n - 2
	assert text.startswith(b"(L2001:1,L2002:1,(L2000:1,(L1999:1,(") and text.endswith(b",(L0:1,L1:2)" + b":2)" * (n - 4) + b":3);\n")
	# what is no tree is refused
	bad = M.expected("caterpillar_12").copy()
	bad["a"][3] = bad["a"][2]
	with pytest.raises(ValueError):
		host.nj_newick_text(bad, ["x"] * 12)
	bad = M.expected("caterpillar_12").copy()
	bad["b"][0] = 12                                                        # its own node
	with pytest.raises(ValueError):
		host.nj_newick_text(bad, ["x"] * 12)
	with pytest.raises(ValueError):
		host.nj_newick_text(M.expected("caterpillar_12"), ["x"] * 11)


# ---- the header and the libraries ----------------------------------------------------------------------------------------------------------------

def test_header_constants_types_and_prototypes():
	from vcf2multialign_amd import _native as N
	header = _header()
	assert re.search(r"#define V2M_NJ_NONE\s+0xFFFFFFFFu", header) and N.NJ_NONE == M.NONE == 0xFFFFFFFF
	assert re.search(r"#define V2M_NJ_MAX_ROWS\s+32768u", header) and N.NJ_MAX_ROWS == 32768
	assert "#define V2M_ABI_VERSION 5" in header and "V2M_KERNEL_END = 15" in header and "V2M_KERNEL_LIMIT = 17" in header
	assert header.index("---- site LD") < header.index("---- neighbour joining") < header.index("---- founder search")
	assert re.search(r"\bint v2m_nj_tree_of_distances\(v2m_ctx \*ctx, const void \*d_dist, uint64_t n, uint64_t pitch, v2m_nj_node \*nodes[^;]*?,\s*v2m_nj_tree_info \*info[^;]*?\);", header)
	assert re.search(r"\bint v2m_nj_tree\(v2m_ctx \*ctx, const v2m_row_batch \*rows, uint32_t flags[^;]*?, v2m_nj_node \*nodes[^;]*?,\s*v2m_nj_tree_info \*info[^;]*?\);", header)
	for name in ("v2m_nj_tree", "v2m_nj_tree_of_distances"):
		assert name in N.SIGNATURES
	node = re.search(r"typedef struct \{([^}]*)\} v2m_nj_node;", header).group(1)
	node = re.sub(r"/\*.*?\*/", "", node)
	assert re.findall(r"\b(\w+)\s*[,;]", node) == list(M.NODE_DTYPE.names) == [f for f, *_ in N.NJ_NODE_DTYPE]
	assert "uint32_t a, b, c, reserved;" in node and "double len_a, len_b, len_c;" in node
	assert M.NODE_DTYPE.itemsize == np.dtype(N.NJ_NODE_DTYPE).itemsize == 40 and M.NODE_DTYPE == np.dtype(N.NJ_NODE_DTYPE)
	info = re.search(r"typedef struct \{([^}]*)\} v2m_nj_tree_info;", header).group(1)
	assert re.findall(r"(\w+);", info) == [f for f, _ in N.NjTreeInfo._fields_] == ["n_nodes", "n_sites", "n_columns", "n_passes", "distances_ms", "tree_ms"]
	assert C.sizeof(N.NjTreeInfo) == 48


def test_exported_symbols():
	from vcf2multialign_amd import build
	hip = C.CDLL(build.LIB_PATH)
	for name in ("v2m_nj_tree", "v2m_nj_tree_of_distances"):
		assert hasattr(hip, name), name
	out = subprocess.run(["nm", "-D", "--defined-only", build.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
	assert " T v2m_nj_tree\n" in out and " T v2m_nj_tree_of_distances\n" in out
	out = subprocess.run(["nm", "-D", "--defined-only", build.HOST_LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
	assert " T v2mh_nj_tree_cpu\n" in out and " T v2mh_nj_newick_text\n" in out


def test_the_kernels_are_in_the_library_source():
	with open(M.NJ_KERNELS_HPP) as f:
		text = f.read()
	for kernel in ("nj_init_kernel", "nj_rowmin_kernel", "nj_join_kernel"):
		assert re.search(r"__global__[^;{]*\b%s\(" % kernel, text), kernel
	# every function that computes holds the pragma
	bodies = re.split(r"\n(?=__global__|__device__)", re.sub(r"//[^\n]*", "", text))
	for body in bodies[1:]:
		if re.search(r"\bdouble\b[^;]*=[^;]*[-+*/]", body.split("{", 1)[1]):
			assert "#pragma clang fp contract(off)" in body, body[:80]
	with open(os.path.join(ROOT, "vcf2multialign_amd", "csrc", "v2m_hip.hip")) as f:
		library = f.read()
	assert library.index('#include "ld_kernels.hpp"') < library.index('#include "nj_kernels.hpp"')
	assert "cooperative" not in library.lower() and "hipGraph" not in text
	from vcf2multialign_amd import build
	assert M.NJ_KERNELS_HPP in build.deps("HIP_DEPS")
	assert "-march" not in " ".join(build.CXX_FLAGS) and "-std=c++20" in build.CXX_FLAGS     # ISO, no FMA to contract into


def test_python_surface():
	import inspect
	import vcf2multialign_amd as v2m
	from vcf2multialign_amd import host, output
	assert list(inspect.signature(v2m.Context.nj_tree).parameters) == ["self", "rows", "acgt_only", "info"]
	assert list(inspect.signature(v2m.Context.nj_tree_of_distances).parameters) == ["self", "ptr", "n", "pitch", "info"]
	assert list(inspect.signature(host.nj_tree_cpu).parameters) == ["dist"]
	assert list(inspect.signature(host.nj_newick_text).parameters) == ["nodes", "labels"]
	assert list(inspect.signature(output.HaplotypeOutput.output_tree).parameters) == ["self", "graph", "stream", "acgt_only"]
	assert list(inspect.signature(output.FounderSequenceGreedyOutput.output_tree).parameters) == ["self", "graph", "cut_positions", "assigned_samples_column_major", "stream", "acgt_only"]
	assert host.nj_tree_cpu(M.TIE_LEAF_INTERNAL).dtype == M.NODE_DTYPE


# ---- the driver's argument errors (reported before a device is opened) ---------------------------------------------------------------------------

def _run(args, cwd=None):
	assert os.path.exists(CLI), "build the host driver first (__graft_entry__.build())"
	return subprocess.run([CLI] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_cli_argument_errors(tmp_path):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	bed = tmp_path / "r.bed"
	bed.write_text("1\t0\t4\n")
	common = ["-H", "-r", fa, "-a", vcf, "-c", "1"]
	for extra, what in ((["--regions-file=" + str(bed)], "--regions-file"), (["--device=0,0"], "more than one --device entry")):
		r = _run(common + ["--output-tree=" + str(tmp_path / "x.nwk")] + extra, cwd=str(tmp_path))
		assert r.returncode != 0
		assert ("ERROR: --output-tree cannot be combined with %s.\n" % what).encode() in r.stderr, r.stderr.decode()
	r = _run(common + ["--tree-acgt-only", "-s", str(tmp_path / "x.a2m")], cwd=str(tmp_path))
	assert r.returncode != 0 and b"ERROR: --tree-acgt-only requires --output-tree.\n" in r.stderr
	# --acgt-only keeps its meaning and its error
	r = _run(common + ["--acgt-only", "--output-tree=" + str(tmp_path / "x.nwk")], cwd=str(tmp_path))
	assert r.returncode != 0 and b"ERROR: --acgt-only requires --output-distances.\n" in r.stderr
	# fewer than three sequences: known from the arguments for founders
	for extra, count in ((["-F", "1"], 2), (["-F", "2", "--omit-reference"], 2), (["-F", "1", "--omit-reference"], 1)):
		r = _run(extra + ["-r", fa, "-a", vcf, "-c", "1", "--output-tree=" + str(tmp_path / "x.nwk")], cwd=str(tmp_path))
		assert r.returncode != 0 and ("ERROR: --output-tree needs at least three sequences (got %d).\n" % count).encode() in r.stderr, r.stderr.decode()
	assert not (tmp_path / "x.nwk").exists() and not (tmp_path / "x.a2m").exists()
	r = _run(["--help"])
	assert r.returncode == 0 and b"--output-tree=FILE" in r.stdout + r.stderr and b"--tree-acgt-only" in r.stdout + r.stderr
