"""The VCF scan rule on the host (csrc/host/readers.cc: scan_lines_host) and the assembler behind it: graphs built through the scanner
equal the text path's, array by array and message by message, and the scanner declines exactly the lines outside the rule.  No GPU."""

import ctypes as C
import os
import re

import numpy as np
import pytest

import synth
import vcf_scan_cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")
FIXTURES = [("test-1a", "test-1.fa"), ("test-1b", "test-1.fa"), ("test-2", "test-2.fa"), ("test-3", "test-3.fa"), ("test-4", "test-4.fa")]
THREADS = (1, 2, 5)


def graph_arrays(g):
	return dict(ref=g.ref, rp=g.reference_positions.tolist(), ap=g.aligned_positions.tolist(), tg=g.alt_edge_targets.tolist(), cs=g.alt_edge_count_csum.tolist(),
		lo=g.label_offsets.tolist(), lb=g.label_bytes, sn=g.sample_names, pc=g.ploidy_csum.tolist(), pdims=g.paths_by_edge_and_chrom_copy_dims,
		paths=g.paths_by_edge_and_chrom_copy.tobytes(), hv=g.handled_variants, cm=g.chr_id_mismatches, ov=g.overlaps)


def same_graph(fa, vcf, declined=0, **kw):
	"""The scanned build on 1, 2 and 5 threads against the text path; returns the scanned graph."""
	from vcf2multialign_amd import host
	want = graph_arrays(host.HostGraph(fa, vcf, "1", **kw))
	for threads in THREADS:
		h = host.HostGraph(fa, vcf, "1", host_scan=True, threads=threads, **kw)
		assert graph_arrays(h) == want, (vcf, threads)
		assert h.declined_lines == declined, (vcf, h.declined_lines)
		assert h.scanned_lines == len(open(vcf, "rb").read().split(b"\n")) - (1 if open(vcf, "rb").read().endswith(b"\n") else 0)
	return h


@pytest.mark.parametrize("stem,fasta", FIXTURES)
def test_reference_fixtures(stem, fasta):
	# GT first, LF-terminated, at most 8 ALTs: nothing is declined
	same_graph(os.path.join(FIX, fasta), os.path.join(FIX, stem + ".vcf"))


def test_mini3(tmp_path):
	from vcf2multialign_amd import synth as vsynth
	fa, vcf = tmp_path / "m.fa", tmp_path / "m.vcf"
	vsynth.dataset("mini3").write_fasta_and_vcf(fa, vcf)
	h = same_graph(str(fa), str(vcf))
	assert h.handled_variants > 100


@pytest.mark.parametrize("seed,kw", [
	(101, {}), (102, {"mix": (1.0, 0.0, 0.0)}), (103, {"long_every": 25}), (104, {"multi_allelic": 0.4, "density": 0.4}),
	(105, {"ploidy": 1}), (106, {"ploidy": 3}),
])
def test_synthetic_vcfs(tmp_path, seed, kw):
	rng = np.random.default_rng(seed)
	ref = synth.random_reference(rng, 30000)
	n_samples = 70 if seed == 101 else 9
	recs = synth.random_records(rng, ref, 700, n_samples, **kw)
	fa, vcf = synth.write_inputs(str(tmp_path), ref, recs, n_samples, phased=(seed % 2 == 0))
	same_graph(fa, vcf)


@pytest.mark.parametrize("case", vcf_scan_cases.cases() + [vcf_scan_cases.padded_case(range(0, 64, 9)), vcf_scan_cases.copies_case(129)], ids=lambda c: c.name)
def test_hand_made_vcfs(tmp_path, case):
	fa, vcf = case.write(tmp_path)
	same_graph(fa, vcf, declined=len(case.declined), **case.kwargs())


@pytest.mark.parametrize("case", vcf_scan_cases.cases(), ids=lambda c: c.name)
@pytest.mark.parametrize("small_slices", [False, True])
def test_scanner_declines_exactly_the_marked_lines(case, small_slices):
	from vcf2multialign_amd import context, host
	slice_bytes = max(map(len, case.lines)) + 150 if small_slices else 0     # two or three lines a slice
	ex = case.excluded_pairs()
	rc, chunks = host.scan_lines_host(case.vcf, "1", layout=lambda _i, line: context.first_record_layout(line, excluded=ex), slice_bytes=slice_bytes)
	assert rc == 0
	kinds = np.concatenate([c["lines"]["kind"] for c in chunks])
	assert len(kinds) == len(case.lines)
	assert set(np.flatnonzero(kinds == 3).tolist()) == case.declined
	assert [c["first_line"] for c in chunks] == np.cumsum([0] + [len(c["lines"]) for c in chunks])[:-1].tolist()
	for c in chunks:                                                  # allocation in line order, nothing between the heads
		assert c["lines"]["head_offset"].tolist() == np.concatenate([[0], np.cumsum(c["lines"]["head_length"])[:-1]]).tolist()
		assert c["lines"]["column_begin"].tolist() == np.concatenate([[0], np.cumsum(c["lines"]["n_alts"])[:-1]]).tolist()
		assert len(c["heads"]) == int(c["lines"]["head_length"].sum()) and len(c["columns"]) == int(c["lines"]["n_alts"].sum())


def test_a_line_longer_than_a_slice_is_unsupported():
	from vcf2multialign_amd import host
	case = vcf_scan_cases.cases()[0]
	longest = max(map(len, case.lines))
	rc, _ = host.scan_lines_host(case.vcf, "1", slice_bytes=longest)      # the line and its '\n' do not fit
	assert rc == 3
	rc, chunks = host.scan_lines_host(case.vcf, "1", slice_bytes=longest + 1)
	assert rc == 0 and sum(len(c["lines"]) for c in chunks) == len(case.lines)


def test_a_delegate_that_stops_at_a_ref_mismatch_ends_the_scan(tmp_path, monkeypatch):
	"""The graph of the text path (tests/test_host_builder.py: test_delegate_that_stops_at_a_ref_mismatch), and nothing scanned after the
	chunk the build stopped in."""
	from vcf2multialign_amd import host
	L = host._load()
	L.v2mh_set_stop_at_ref_mismatch.argtypes = [C.c_int]
	case = vcf_scan_cases.Case("stops", ["S0", "S1", "S2"])
	for k in range(40):
		case.rec([b"0|1", b"1|0", b"1|1"])
	bad = len(case.lines) - 30
	f = case.lines[bad].split(b"\t")
	f[3] = vcf_scan_cases.other(f[3])                                 # the REF column of the 11th record is not the reference's
	case.lines[bad] = b"\t".join(f)
	fa, vcf = case.write(tmp_path)
	try:
		L.v2mh_set_stop_at_ref_mismatch(1)
		want = graph_arrays(host.HostGraph(fa, vcf, "1"))
		assert 10 <= want["hv"] <= 11 and len(want["tg"]) == 10     # the records before it; nothing after it
		whole = host.HostGraph(fa, vcf, "1", host_scan=True)
		assert graph_arrays(whole) == want
		monkeypatch.setenv("V2M_RING_SLOT_BYTES", "200")             # a few lines a slice
		h = host.HostGraph(fa, vcf, "1", host_scan=True)
		assert graph_arrays(h) == want
		assert bad < h.scanned_lines <= bad + 8 < len(case.lines)
	finally:
		L.v2mh_set_stop_at_ref_mismatch(0)


damaged, ERRORS = vcf_scan_cases.damaged, vcf_scan_cases.ERRORS


@pytest.fixture(scope="module")
def mini3(tmp_path_factory):
	from vcf2multialign_amd import synth as vsynth
	d = tmp_path_factory.mktemp("mini3")
	fa, vcf = d / "m.fa", d / "m.vcf"
	vsynth.dataset("mini3").write_fasta_and_vcf(fa, vcf)
	return str(fa), open(vcf, "rb").read().split(b"\n")


@pytest.mark.parametrize("how", ERRORS)
def test_errors_equal_the_text_paths(mini3, tmp_path, how):
	from vcf2multialign_amd import host
	fa, good = mini3
	lines = list(good)
	k = len(lines) * 3 // 4
	damaged(lines, k, how)
	bad = tmp_path / "bad.vcf"
	bad.write_bytes(b"\n".join(lines))
	with pytest.raises(ValueError) as text:
		host.HostGraph(fa, str(bad), "1")
	# (an error found before the record has claimed its columns -- the column count, POS -- rolls the chunk back to before the PREVIOUS
	# record in the text parser, whose message is then the merge stage's; the scanned path shares that code and says the same)
	if how not in ("fewer than 8 columns", "POS must be 1-based"):
		assert str(text.value) == "VCF line %d: %s" % (k + 1, how)
	for threads in THREADS:
		with pytest.raises(ValueError) as scanned:
			host.HostGraph(fa, str(bad), "1", host_scan=True, threads=threads)
		assert str(scanned.value) == str(text.value)


def test_every_symbol_of_the_scan_section_is_exported_and_bound():
	from vcf2multialign_amd import _native, build
	header = open(os.path.join(ROOT, "include", "v2m_hip.h")).read()
	section = header[header.index("---- VCF scan ----"):header.index("---- verification helper ----")]
	declared = re.findall(r"^\w[\w \*]*?\b(v2m_\w+)\(", section, re.M)
	assert "v2m_vcf_scan" in declared
	lib = C.CDLL(build.LIB_PATH) if os.path.exists(build.LIB_PATH) else None
	assert lib is not None, "build the library first (__graft_entry__.build())"
	for name in declared:
		assert name in _native.SIGNATURES, name
		assert getattr(lib, name) is not None
	assert "V2M_KERNEL_VCF = 8" in header and "V2M_KERNEL_COUNT = 9" in header and _native.KERNEL_VCF == 8
	assert "#define V2M_ABI_VERSION 5" in header
