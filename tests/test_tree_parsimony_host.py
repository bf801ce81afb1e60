"""Parsimony on a tree without a GPU: the numpy model of tests/tree_parsimony_model.py held to an independent Sankoff minimum and to
its own invariants, the host library's plain-loop restatement (v2mh_tree_parsimony_cpu) held to the model byte for byte, the sites and
spellings a port gets wrong, every form of records that is no tree, the Newick text, the header's constants, types and prototypes, the
exported symbols, the Python surface and the driver's argument errors."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import tree_parsimony_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")
CORPUS = M.corpus()


def _header():
	with open(os.path.join(ROOT, "include", "v2m_hip.h")) as f:
		return f.read()


# ---- the model --------------------------------------------------------------------------------------------------------------------------

def test_the_models_steps_are_the_least_on_every_item():
	for item in CORPUS:
		sites, _, _ = M.expected(item.name)
		assert np.array_equal(sites["steps"], M.sankoff(item.m, item.nodes)), item.name


def test_mutations_number_the_steps_and_branches_sum_to_them():
	for item in CORPUS:
		sites, branch_changes, mutations = M.expected(item.name)
		assert np.array_equal(np.bincount(mutations["site"], minlength=item.V), sites["steps"]), item.name
		assert int(branch_changes.sum()) == int(sites["steps"].sum()) == len(mutations), item.name
		assert np.array_equal(np.bincount(mutations["node"], minlength=2 * item.n - 3), branch_changes), item.name
		assert (np.diff(mutations["site"].astype(np.int64)) >= 0).all() and (mutations["from"] != mutations["to"]).all() and mutations["to"].max(initial=0) < 4
		# a mutation ends in a state the branch's lower node can take; a leaf that carries one holds exactly that letter
		leaf = mutations[mutations["node"] < item.n]
		assert np.array_equal(M.leaf_sets(item.m)[leaf["node"], leaf["site"]], 1 << leaf["to"]), item.name


def test_the_corpus_can_tell():
	"""The conditions that keep the corpus from hiding a failure: steps above one letter's worth, homoplasies, sites without a step,
	missing bytes in every spelling, mutations on leaves and on internal branches, both cases."""
	S, T, J = M.kernel_constants()
	assert (S, T, J) == (4, 256, 4)
	assert set(M.seam_taxa_counts()) >= set(range(3, 12)) | {65, 257}
	assert set(M.seam_site_counts()) >= set(range(1, S + 2)) | {64 * S - 1, 64 * S, 64 * S + 1, T * S - 1, T * S, T * S + 1, 2 * T * S + 1}
	assert {i.V for i in CORPUS} >= set(M.seam_site_counts()) and {i.n for i in CORPUS} >= set(M.seam_taxa_counts())
	item = next(i for i in CORPUS if i.name == "spine_34")
	sites, branch_changes, mutations = M.expected(item.name)
	popcount = np.array([bin(int(p)).count("1") for p in sites["present"]])
	assert (sites["steps"] > popcount - 1).any() and (sites["steps"] == 0).any() and sites["steps"].max() > 3
	assert (mutations["node"] < item.n).any() and (mutations["node"] >= item.n).any()
	few = M.expected("spine_257")[1]
	assert (few == 0).any() and (few > 0).any()                              # branches without a change: nothing is added for them
	for byte in b"ACGTacgtN-nR" + bytes([0, 0xC1]):
		assert (item.m == byte).any(), byte
	# in the spine every record but the first reads the node the record before it made
	assert all(int(item.nodes["b"][t]) == item.n + t - 1 for t in range(1, item.n - 3)) and int(item.nodes["c"][-1]) == 2 * item.n - 4
	# the join orders that are no neighbour joining: the model's tree of the same bytes' distances differs
	assert not M.is_tree(M.tree("joins", 35, 7)[:-1], 35) and M.is_tree(M.tree("joins", 35, 7), 35)


def test_steps_do_not_depend_on_the_root():
	"""The same unrooted tree written with another last node: the steps stay, and so does the tree's length."""
	# ((0,1)5,(2,3)6,4) and ((2,3)5,4)6 joined with 0 and 1 at the end: the same five-leaf tree
	one = np.zeros(3, dtype=M.NODE_DTYPE)
	one[0], one[1], one[2] = (0, 1, M.NONE, 0, 0, 0, 0), (2, 3, M.NONE, 0, 0, 0, 0), (4, 5, 6, 0, 0, 0, 0)
	other = np.zeros(3, dtype=M.NODE_DTYPE)
	other[0], other[1], other[2] = (2, 3, M.NONE, 0, 0, 0, 0), (4, 5, M.NONE, 0, 0, 0, 0), (0, 1, 6, 0, 0, 0, 0)
	m = M.evolved(one, 5, 300, 3, change=0.3)
	a, b = M.fitch(m, one), M.fitch(m, other)
	assert np.array_equal(a[0], b[0]) and a[0]["steps"].max() >= 2 and a[1].sum() == b[1].sum()


# ---- the restatement --------------------------------------------------------------------------------------------------------------------

def test_the_restatement_equals_the_model_byte_for_byte():
	from vcf2multialign_amd import host
	for item in CORPUS:
		want = M.expected(item.name)
		got = host.tree_parsimony_cpu(item.m, item.nodes)
		for g, w, what in zip(got, want, ("sites", "branch changes", "mutations")):
			assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (item.name, what)
	# a pitch of its own, with bytes behind the sites that no result may depend on
	item = next(i for i in CORPUS if i.name == "inserted_33")
	wide = np.full((item.n, item.V + 7), ord("T"), dtype=np.uint8)
	wide[:, :item.V] = item.m
	got = host.tree_parsimony_cpu(wide, item.nodes, n_sites=item.V)
	assert all(g.tobytes() == w.tobytes() for g, w in zip(got, M.expected(item.name)))
	# the counts without the list; a list that does not fit is not written
	sites, branch_changes, mutations = host.tree_parsimony_cpu(item.m, item.nodes, want_mutations=False)
	assert len(mutations) == 0 and sites.tobytes() == M.expected(item.name)[0].tobytes()
	lib = host._load()
	total = len(M.expected(item.name)[2])
	short = np.full(total, 0xAB, dtype=np.uint8).repeat(16).view(M.MUTATION_DTYPE)
	err = C.create_string_buffer(256)
	assert total == lib.v2mh_tree_parsimony_cpu(item.m.ctypes.data, item.n, item.V, item.V, item.nodes.ctypes.data, sites.ctypes.data, branch_changes.ctypes.data,
		short.ctypes.data, total - 1, err, len(err))
	assert short[:total - 1].tobytes() == M.expected(item.name)[2][:total - 1].tobytes() and short[total - 1:].tobytes() == b"\xab" * 16


def test_missing_one_state_and_four_state_sites():
	from vcf2multialign_amd import host
	nodes = M.spine(5)
	columns = [b"N-n" + bytes([0, 0xC1]), b"ggGgG", b"ACGTa", b"A-C-A", b"acgtN"]
	m = np.ascontiguousarray(np.array([np.frombuffer(c, dtype=np.uint8) for c in columns]).T)
	sites, branch_changes, mutations = M.fitch(m, nodes)
	assert sites["steps"].tolist() == [0, 0, 3, 1, 3] and sites["present"].tolist() == [0, 4, 15, 3, 15]
	assert np.array_equal(sites["steps"], M.sankoff(m, nodes))
	got = host.tree_parsimony_cpu(m, nodes)
	assert got[0].tobytes() == sites.tobytes() and got[1].tobytes() == branch_changes.tobytes() and got[2].tobytes() == mutations.tobytes()
	# the all-missing site puts the root in state A and no mutation anywhere; a missing leaf never carries one
	assert not (mutations["site"] == 0).any()
	missing_leaves = {(r, s) for r in range(5) for s in range(5) if M.leaf_sets(m)[r, s] == 0xF}
	assert not {(int(mu["node"]), int(mu["site"])) for mu in mutations} & missing_leaves
	# lower case is the same letter
	upper = np.frombuffer(bytes(m.tobytes()).upper(), dtype=np.uint8).reshape(m.shape)
	assert all(a.tobytes() == b.tobytes() for a, b in zip(host.tree_parsimony_cpu(upper, nodes), got))


def bad_records():
	"""(what, records, n): every form of records the header refuses."""
	good = M.tree("inserted", 9, 3)
	out = []
	def changed(what, edit, n=9):
		nodes = good.copy()
		edit(nodes)
		assert not M.is_tree(nodes, n), what
		out.append((what, nodes, n))
	changed("a child joined twice", lambda x: x["a"].__setitem__(3, x["a"][2]))
	changed("a node that is not made yet", lambda x: x["b"].__setitem__(0, 9))
	changed("its own node", lambda x: x["b"].__setitem__(2, 11))
	changed("an id beyond the tree", lambda x: x["b"].__setitem__(1, 40))
	changed("a third child before the last record", lambda x: x["c"].__setitem__(0, 8))
	changed("no third child in the last record", lambda x: x["c"].__setitem__(6, M.NONE))
	changed("a and b in descending order", lambda x: x.__setitem__(0, (x["b"][0], x["a"][0], M.NONE, 0, 0, 0, 0)))
	changed("b and c in descending order", lambda x: x.__setitem__(6, (x["a"][6], x["c"][6], x["b"][6], 0, 0, 0, 0)))
	changed("a equal to b", lambda x: x["b"].__setitem__(0, x["a"][0]))
	return out


def test_every_invalid_record_form_is_refused():
	from vcf2multialign_amd import host
	for what, nodes, n in bad_records():
		with pytest.raises(ValueError):
			host.tree_parsimony_cpu(np.full((n, 4), ord("A"), dtype=np.uint8), nodes)
	with pytest.raises(ValueError):
		host.tree_parsimony_cpu(np.zeros((2, 4), dtype=np.uint8), np.zeros(0, dtype=M.NODE_DTYPE))
	with pytest.raises(ValueError):
		host.tree_parsimony_cpu(np.zeros((9, 4), dtype=np.uint8), M.tree("inserted", 9, 3)[:-1])


# ---- the text ---------------------------------------------------------------------------------------------------------------------------

def test_newick_text():
	from vcf2multialign_amd import host
	three = M.spine(3)
	assert host.nj_newick_parsimony_text(three, ["a", "b", "c"], [3, 0, 7]) == b"(a:3,b:0,c:7)node0;\n" == M.newick(three, ["a", "b", "c"], [3, 0, 7])
	five = M.spine(5)
	counts = [1, 2, 3, 4, 5, 6, 7]
	assert host.nj_newick_parsimony_text(five, ["a", "b", "c_d", "", "e'f"], counts) == b"('':4,'e''f':5,('c_d':3,(a:1,b:2)node0:6)node1:7)node2;\n"
	for item in CORPUS:
		labels = ["L%d" % k for k in range(item.n)]
		branch_changes = M.expected(item.name)[1]
		text = host.nj_newick_parsimony_text(item.nodes, labels, branch_changes)
		assert text == M.newick(item.nodes, labels, branch_changes), item.name
		assert text.count(b":") == 2 * item.n - 3 and text.endswith(b")node%d;\n" % (item.n - 3))
	# the topology is nj_newick_text's: with the lengths and the labels taken out the two texts are one
	item = next(i for i in CORPUS if i.name == "balanced_32")
	labels = ["L%d" % k for k in range(item.n)]
	strip = lambda text: re.sub(rb"\)node\d+", b")", re.sub(rb":[-+.e\d]+", b"", text))
	assert strip(host.nj_newick_parsimony_text(item.nodes, labels, M.expected(item.name)[1])) == strip(host.nj_newick_text(item.nodes, labels))
	# depth 2 000 without recursion
	n = 2003
	deep = M.spine(n)
	labels = ["L%d" % k for k in range(n)]
	counts = np.arange(2 * n - 3, dtype=np.uint32)
	text = host.nj_newick_parsimony_text(deep, labels, counts)
	assert text == M.newick(deep, labels, counts) and text.count(b"(") == n - 2
	assert text.startswith(b"(L2001:2001,L2002:2002,(L2000:2000,(L1999:1999,(") and b",(L0:0,L1:1)node0:2003)node1:2004)node2:2005)" in text
	assert text.endswith(b")node1998:4001)node1999:4002)node2000;\n")
	# what is no tree, or no count per branch, is refused
	for what, nodes, k in bad_records()[:6]:
		with pytest.raises(ValueError):
			host.nj_newick_parsimony_text(nodes, ["x"] * k, np.zeros(2 * k - 3, dtype=np.uint32))
	with pytest.raises(ValueError):
		host.nj_newick_parsimony_text(five, ["x"] * 5, counts[:6])


def test_mutation_and_site_texts():
	import oracle
	import pair_distances_model as PM
	import nj_tree_model as NJ
	from vcf2multialign_amd import host
	g = oracle.build_variant_graph(os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf"), "1")
	ids, rows = PM.haplotype_ids(g)
	nodes = NJ.nj(PM.expected(g, rows)[0])
	sites, branch_changes, mutations, L = M.expected_of_rows(g, rows, nodes)
	assert len(sites) and len(mutations) and L == g.aligned_length
	assert host.tree_sites_text(sites, g.reference_positions, g.aligned_positions) == M.sites_text(g, sites)
	assert host.tree_mutations_text(mutations, sites, ids, g.reference_positions, g.aligned_positions) == M.mutations_text(g, mutations, sites, ids)
	assert host.tree_sites_text(sites[:0], g.reference_positions, g.aligned_positions) == b""
	one = np.zeros(1, dtype=M.TREE_SITE_DTYPE)
	one[0] = (0, 5, 0b1011)
	assert host.tree_sites_text(one, g.reference_positions, g.aligned_positions).endswith(b"\tACT\t5\t3\n")
	bad = mutations[:1].copy()
	bad["site"] = len(sites)
	with pytest.raises(ValueError):
		host.tree_mutations_text(bad, sites, ids, g.reference_positions, g.aligned_positions)


# ---- the header and the libraries -------------------------------------------------------------------------------------------------------

def test_header_constants_types_and_prototypes():
	from vcf2multialign_amd import _native as N
	header = _header()
	assert "#define V2M_ABI_VERSION 5" in header and "V2M_KERNEL_END = 15" in header and "V2M_KERNEL_LIMIT = 17" in header
	assert header.index("---- bootstrap") < header.index("---- parsimony") < header.index("---- founder search")
	assert (N.FITCH_SITES, N.FITCH_THREADS, N.FITCH_BATCH) == M.kernel_constants()
	for name, dtype, size in (("v2m_parsimony_site", N.PARSIMONY_SITE_DTYPE, 8), ("v2m_tree_site", N.TREE_SITE_DTYPE, 16), ("v2m_tree_mutation", N.TREE_MUTATION_DTYPE, 16)):
		body = re.search(r"typedef struct \{([^}]*)\} %s;" % name, header).group(1)
		assert re.findall(r"\b(\w+)\s*[,;]", body) == [f for f, *_ in dtype], name
		assert np.dtype(dtype).itemsize == size
	assert np.dtype(N.PARSIMONY_SITE_DTYPE) == M.SITE_DTYPE and np.dtype(N.TREE_SITE_DTYPE) == M.TREE_SITE_DTYPE and np.dtype(N.TREE_MUTATION_DTYPE) == M.MUTATION_DTYPE
	assert "uint64_t column; uint32_t steps, present;" in header and "uint32_t site, node, from, to;" in header
	info = re.search(r"typedef struct \{([^}]*)\} v2m_tree_parsimony_info;", header).group(1)
	assert re.findall(r"(\w+);", info) == [f for f, _ in N.TreeParsimonyInfo._fields_] == ["n_sites", "n_columns", "n_mutations", "n_ranges", "counts_ms", "gather_ms", "parsimony_ms"]
	assert C.sizeof(N.TreeParsimonyInfo) == 56
	assert re.search(r"\bint v2m_parsimony_of_sites\(v2m_ctx \*ctx, const void \*d_bytes, uint64_t n, uint64_t n_sites, uint64_t pitch, const v2m_nj_node \*nodes[^;]*?,\s*"
		r"void \*d_sites, void \*d_branch_changes[^;]*?, void \*d_mutations[^;]*?, uint64_t capacity,\s*uint64_t \*n_mutations\);", header)
	assert re.search(r"\bint v2m_tree_parsimony\(v2m_ctx \*ctx, const v2m_row_batch \*rows, const v2m_nj_node \*nodes[^;]*?, uint32_t flags[^;]*?,\s*uint32_t \*branch_changes[^;]*?, "
		r"v2m_tree_sites_sink_fn sites_sink[^;]*?,\s*v2m_tree_mutations_sink_fn mutations_sink[^;]*?, void \*user, v2m_tree_parsimony_info \*info[^;]*?\);", header)
	for name in ("v2m_parsimony_of_sites", "v2m_tree_parsimony"):
		assert name in N.SIGNATURES
	assert len(N.SIGNATURES["v2m_parsimony_of_sites"][1]) == 11 and len(N.SIGNATURES["v2m_tree_parsimony"][1]) == 9


def test_exported_symbols():
	from vcf2multialign_amd import build
	out = subprocess.run(["nm", "-D", "--defined-only", build.LIB_PATH], stdout=subprocess.PIPE, check=True).stdout.decode()
	assert " T v2m_parsimony_of_sites\n" in out and " T v2m_tree_parsimony\n" in out
	for path in (build.HOST_LIB_PATH, build.CHECKED_HOST_LIB_PATH):
		out = subprocess.run(["nm", "-D", "--defined-only", path], stdout=subprocess.PIPE, check=True).stdout.decode()
		for name in ("v2mh_tree_parsimony_cpu", "v2mh_nj_newick_parsimony_text", "v2mh_tree_mutations_text", "v2mh_tree_sites_text"):
			assert " T %s\n" % name in out, (path, name)


def test_the_kernels_are_in_the_library_source():
	from vcf2multialign_amd import build
	with open(M.PARSIMONY_KERNELS_HPP) as f:
		text = f.read()
	for kernel in ("fitch_up_kernel", "fitch_down_kernel"):
		assert re.search(r"__global__[^;{]*\b%s\(" % kernel, text), kernel
	# the sets are read and written through one pointer that is not __restrict__, by plain loads and stores
	for kernel in ("fitch_up_kernel", "fitch_down_kernel"):
		signature = re.search(r"void %s\((.*?)\)\n\{" % kernel, text, re.S).group(1)
		assert re.search(r"unsigned char \*sets,", signature) and "__restrict__ sets" not in signature, kernel
	code = re.sub(r"//[^\n]*", "", text)
	assert "nontemporal" not in code and "__builtin_amdgcn_raw_buffer" not in code and "asm volatile(\"global" not in code
	with open(os.path.join(ROOT, "vcf2multialign_amd", "csrc", "v2m_hip.hip")) as f:
		library = f.read()
	assert library.index('#include "bootstrap_kernels.hpp"') < library.index('#include "parsimony_kernels.hpp"')
	assert M.PARSIMONY_KERNELS_HPP in build.deps("HIP_DEPS")


def test_python_surface():
	import inspect
	import vcf2multialign_amd as v2m
	from vcf2multialign_amd import host, output
	assert list(inspect.signature(v2m.Context.tree_parsimony).parameters) == ["self", "rows", "nodes", "info", "want_sites", "want_mutations", "want_branch_changes"]
	assert list(inspect.signature(v2m.Context.parsimony_of_sites).parameters) == ["self", "bytes_ptr", "n", "n_sites", "pitch", "nodes", "sites_ptr", "branch_changes_ptr",
		"mutations_ptr", "capacity"]
	assert list(inspect.signature(host.tree_parsimony_cpu).parameters) == ["rows", "nodes", "n_sites", "want_mutations"]
	assert list(inspect.signature(host.nj_newick_parsimony_text).parameters) == ["nodes", "labels", "branch_changes"]
	assert list(inspect.signature(output.HaplotypeOutput.output_tree_parsimony).parameters) == ["self", "graph", "parsimony", "mutations", "sites", "acgt_only", "bootstrap", "seed"]
	assert list(inspect.signature(output.FounderSequenceGreedyOutput.output_tree_parsimony).parameters) == ["self", "graph", "cut_positions", "assigned_samples_column_major",
		"parsimony", "mutations", "sites", "acgt_only", "bootstrap", "seed"]
	# output_tree keeps its parameters
	assert list(inspect.signature(output.HaplotypeOutput.output_tree).parameters) == ["self", "graph", "stream", "acgt_only"]


# ---- the driver's argument errors (reported before a device is opened) ------------------------------------------------------------------

def _run(args, cwd=None):
	assert os.path.exists(CLI), "build the host driver first (__graft_entry__.build())"
	return subprocess.run([CLI] + args, cwd=cwd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


def test_cli_argument_errors(tmp_path):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	common = ["-H", "-r", fa, "-a", vcf, "-c", "1", "-s", str(tmp_path / "x.a2m")]
	for flag in ("--output-tree-parsimony", "--output-tree-mutations", "--output-tree-sites"):
		r = _run(common + ["%s=%s" % (flag, tmp_path / "x.out")], cwd=str(tmp_path))
		assert r.returncode != 0 and ("ERROR: %s requires --output-tree.\n" % flag).encode() in r.stderr, r.stderr.decode()
	assert not (tmp_path / "x.out").exists() and not (tmp_path / "x.a2m").exists()
	r = _run(["--help"])
	text = r.stdout + r.stderr
	assert r.returncode == 0 and all(flag in text for flag in (b"--output-tree-parsimony=FILE", b"--output-tree-mutations=FILE", b"--output-tree-sites=FILE"))
