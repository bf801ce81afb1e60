"""VCF genotype columns parsed on the GPU (v2m_vcf_scan, csrc/vcf_kernels.hpp): the kernels' line records, head pool and bit columns
against the host's implementation of the same rule byte for byte, at the seams of rows, steps, slices and members; graphs and driver
runs through --gpu-parse against the text path; the launch counts; and all of it again on the checked build."""

import os
import subprocess

import numpy as np
import pytest

import vcf_scan_cases
from bgzf_input_util import bgzf, deflate_raw, member
from vcf2multialign_amd.context import first_record_layout   # (the scan's entry point: this file does not import on a tree without it)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")
DERIVED = os.path.join(HERE, "golden", "derived")
FIXTURES = [("test-1a", "test-1.fa"), ("test-1b", "test-1.fa"), ("test-2", "test-2.fa"), ("test-3", "test-3.fa"), ("test-4", "test-4.fa")]
V2M_ERR_UNSUPPORTED = 3
CASES = vcf_scan_cases.cases()
ROW_COUNTS = [1, 2, 63, 64, 65, 127, 128, 129, 4097]


@pytest.fixture(scope="module")
def ctx():
	import vcf2multialign_amd as v2m
	with v2m.Context(0) as c:
		yield c


def small_slot(case):
	"""A ring slot in which every slice holds two or three of the case's lines (one to four where their lengths differ much): room for the
	longest line, since a longer one is unsupported, and for a typical one beside it."""
	lengths = sorted(map(len, case.lines))
	return lengths[-1] + lengths[len(lengths) // 2] + 2


def layout_of(case):
	ex = case.excluded_pairs()
	return lambda _i, line: first_record_layout(line, excluded=ex)


def host_chunks(case, slice_bytes=0):
	from vcf2multialign_amd import host
	rc, chunks = host.scan_lines_host(case.vcf, "1", layout=layout_of(case), slice_bytes=slice_bytes)
	assert rc == 0
	return chunks


def assert_same_chunks(got, want, what):
	"""Byte for byte: the same chunks, and in each the same records, head pool and columns."""
	assert [(c["first_line"], len(c["lines"])) for c in got] == [(c["first_line"], len(c["lines"])) for c in want], what
	for g, w in zip(got, want):
		assert g["lines"].tobytes() == w["lines"].tobytes(), (what, g["first_line"], g["lines"], w["lines"])
		assert g["heads"] == w["heads"], (what, g["first_line"])
		assert g["words_per_column"] == w["words_per_column"] and g["columns"].tobytes() == w["columns"].tobytes(), (what, g["first_line"])


def per_line(chunks):
	"""What the chunks say line by line, whatever the slices were: (kind, n_alts, head, columns)."""
	out = []
	for c in chunks:
		for l in c["lines"]:
			cols = c["columns"][int(l["column_begin"]):int(l["column_begin"]) + int(l["n_alts"])]
			out.append((int(l["kind"]), int(l["n_alts"]), c["heads"][int(l["head_offset"]):int(l["head_offset"]) + int(l["head_length"])], cols.tobytes()))
	return out


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_hand_made_vcfs_equal_the_host_scanner(ctx, case):
	want = host_chunks(case)
	assert_same_chunks(ctx.vcf_scan(case.vcf, "1", layout_of(case)), want, "plain")
	kinds = np.concatenate([c["lines"]["kind"] for c in want])
	assert set(np.flatnonzero(kinds == 3).tolist()) == case.declined
	for piece in (7, 100, 65280):
		assert_same_chunks(ctx.vcf_scan(bgzf(case.vcf, piece=piece), "1", layout_of(case)), want, "pieces of %d" % piece)


@pytest.mark.parametrize("n_copies", ROW_COUNTS)
def test_row_counts_at_the_word_seams(ctx, n_copies):
	case = vcf_scan_cases.copies_case(n_copies)
	want = host_chunks(case)
	assert want[-1]["words_per_column"] == (n_copies + 63) // 64
	assert want[0]["words_per_column"] == 0 and want[0]["columns"].size == 0 and len(want) == 2   # the header lines, before the layout: a chunk without columns
	assert any(int(w) >> ((n_copies - 1) & 63) & 1 for w in want[-1]["columns"][:, (n_copies - 1) >> 6]), "the last row's bit is set somewhere"
	assert_same_chunks(ctx.vcf_scan(case.vcf, "1"), want, n_copies)


@pytest.mark.parametrize("sep", [b"|", b"/"])
def test_every_byte_phase_of_a_step(ctx, sep):
	# 64 pads, two lines of 2.7 KB each: every byte of a line -- two-digit alleles, separators, colons, tabs -- meets every phase of the
	# genotype pass's 64-byte steps, the last and the first byte of a step among them
	case = vcf_scan_cases.padded_case(range(64), sep=sep)
	want = host_chunks(case)
	assert not any((c["lines"]["kind"] == 3).any() for c in want)
	assert_same_chunks(ctx.vcf_scan(case.vcf, "1"), want, "padded")


@pytest.mark.parametrize("case", CASES + [vcf_scan_cases.padded_case(range(0, 64, 21))], ids=lambda c: c.name)
def test_lines_straddle_slices_and_members(ctx, case, monkeypatch):
	slot = small_slot(case)
	monkeypatch.setenv("V2M_RING_SLOT_BYTES", str(slot))
	want = host_chunks(case, slice_bytes=slot)
	assert len(want) > 2 or len(case.lines) < 6
	assert_same_chunks(ctx.vcf_scan(case.vcf, "1", layout_of(case)), want, "plain")
	for piece in (7, 100, 65280):                                      # (whole members: the slices are cut elsewhere, the lines say the same)
		got = ctx.vcf_scan(bgzf(case.vcf, piece=piece), "1", layout_of(case))
		assert per_line(got) == per_line(want), piece
		assert [c["first_line"] for c in got] == np.cumsum([0] + [len(c["lines"]) for c in got])[:-1].tolist()


def test_a_line_longer_than_a_slice_is_unsupported(ctx, monkeypatch):
	from vcf2multialign_amd.context import V2MError
	case = CASES[0]
	longest = max(map(len, case.lines))
	monkeypatch.setenv("V2M_RING_SLOT_BYTES", str(longest))
	with pytest.raises(V2MError) as e:
		ctx.vcf_scan(case.vcf, "1")
	assert e.value.code == V2M_ERR_UNSUPPORTED and "longer than a slice can hold" in str(e.value)
	# BGZF slices are whole members, so a slice's text may exceed the slot by a member's 64 KiB: the same slot holds the same lines ...
	assert per_line(ctx.vcf_scan(bgzf(case.vcf, piece=100), "1")) == per_line(host_chunks(case))
	monkeypatch.setenv("V2M_RING_SLOT_BYTES", str(longest + 1))
	assert per_line(ctx.vcf_scan(case.vcf, "1")) == per_line(host_chunks(case))
	# ... and a line is too long for it once it exceeds the slot and a member together
	lines = list(case.lines)
	lines.insert(2, b"#" + b"x" * 140000)
	data = b"\n".join(lines) + b"\n"
	monkeypatch.setenv("V2M_RING_SLOT_BYTES", "1000")
	for d in (data, bgzf(data, piece=65280), bgzf(data, piece=100)):
		with pytest.raises(V2MError) as e:
			ctx.vcf_scan(d, "1")
		assert e.value.code == V2M_ERR_UNSUPPORTED and "longer than a slice can hold" in str(e.value)


def test_bgzf_damage_reads_as_in_bgzf_decompress(ctx):
	from vcf2multialign_amd.context import V2MError
	data = CASES[8].vcf
	good = bgzf(data, piece=300)
	first = 18 + len(deflate_raw(data[:300])) + 8
	flipped = bytearray(good)
	flipped[first + 18 + 5] ^= 0x10                                    # a payload bit of the second member
	pieces = [data[i:i + 300] for i in range(0, len(data), 300)]
	bad_crc = b"".join(member(deflate_raw(p), p, crc=0x12345678 if k == 2 else None) for k, p in enumerate(pieces))
	for f in (bytes(flipped), bad_crc):
		with pytest.raises(V2MError) as want:
			ctx.bgzf_decompress(f)
		with pytest.raises(V2MError) as got:
			ctx.vcf_scan(f, "1")
		assert (got.value.code, str(got.value)) == (want.value.code, str(want.value))


# ---- graphs ------------------------------------------------------------------------------------

def graph_arrays(g):
	return dict(ref=g.ref, rp=g.reference_positions.tolist(), ap=g.aligned_positions.tolist(), tg=g.alt_edge_targets.tolist(), cs=g.alt_edge_count_csum.tolist(),
		lo=g.label_offsets.tolist(), lb=g.label_bytes, sn=g.sample_names, pc=g.ploidy_csum.tolist(), pdims=g.paths_by_edge_and_chrom_copy_dims,
		paths=g.paths_by_edge_and_chrom_copy.tobytes(), hv=g.handled_variants, cm=g.chr_id_mismatches, ov=g.overlaps)


def gz_copy(src, dst, piece=65280):
	with open(src, "rb") as f:
		data = f.read()
	with open(dst, "wb") as f:
		f.write(bgzf(data, piece=piece))
	return str(dst)


def test_graphs_of_the_fixtures(ctx, tmp_path):
	from vcf2multialign_amd import host
	for stem, fasta in FIXTURES:
		fa, vcf = os.path.join(FIX, fasta), os.path.join(FIX, stem + ".vcf")
		fa_gz, vcf_gz = gz_copy(fa, tmp_path / (fasta + ".gz"), piece=7), gz_copy(vcf, tmp_path / (stem + ".vcf.gz"), piece=100)
		want = graph_arrays(host.HostGraph(fa, vcf, "1"))
		for f, v in ((fa_gz, vcf_gz), (fa, vcf)):
			h = host.HostGraph(f, v, "1", ctx=ctx, gpu_parse=True)
			assert graph_arrays(h) == want, stem
			assert h.declined_lines == 0 and h.scanned_lines == len(open(vcf, "rb").read().splitlines())


def test_graphs_of_the_hand_made_vcfs(ctx, tmp_path, monkeypatch):
	from vcf2multialign_amd import host
	for case in CASES:
		fa, vcf = case.write(tmp_path)
		vcf_gz = gz_copy(vcf, tmp_path / (case.name + ".vcf.gz"), piece=100)
		want = graph_arrays(host.HostGraph(fa, vcf, "1", **case.kwargs()))
		for small in (False, True):
			if small:
				monkeypatch.setenv("V2M_RING_SLOT_BYTES", str(small_slot(case)))
			else:
				monkeypatch.delenv("V2M_RING_SLOT_BYTES", raising=False)
			for v in (vcf, vcf_gz):
				h = host.HostGraph(fa, v, "1", ctx=ctx, gpu_parse=True, **case.kwargs())
				assert graph_arrays(h) == want, (case.name, small, v)
				assert h.declined_lines == len(case.declined), case.name


def test_graph_of_mini3_and_the_error_messages(ctx, tmp_path):
	from vcf2multialign_amd import host, synth
	fa, vcf = tmp_path / "m.fa", tmp_path / "m.vcf"
	synth.dataset("mini3").write_fasta_and_vcf(fa, vcf)
	fa_gz, vcf_gz = gz_copy(fa, tmp_path / "m.fa.gz"), gz_copy(vcf, tmp_path / "m.vcf.gz")
	h = host.HostGraph(fa_gz, vcf_gz, "1", ctx=ctx, gpu_parse=True)
	assert graph_arrays(h) == graph_arrays(host.HostGraph(str(fa), str(vcf), "1")) and h.declined_lines == 0
	good = open(vcf, "rb").read().split(b"\n")
	for how in vcf_scan_cases.ERRORS:
		lines = list(good)
		vcf_scan_cases.damaged(lines, len(lines) * 3 // 4, how)
		bad, bad_gz = tmp_path / "bad.vcf", tmp_path / "bad.vcf.gz"
		bad.write_bytes(b"\n".join(lines))
		gz_copy(bad, bad_gz)
		with pytest.raises(ValueError) as text:
			host.HostGraph(str(fa), str(bad), "1")
		for v in (bad, bad_gz):
			with pytest.raises(ValueError) as scanned:
				host.HostGraph(str(fa), str(v), "1", ctx=ctx, gpu_parse=True)
			assert str(scanned.value) == str(text.value), how


def test_a_delegate_that_stops_at_a_ref_mismatch_ends_the_scan(ctx, tmp_path, monkeypatch):
	import ctypes
	from vcf2multialign_amd import host
	L = host._load()
	L.v2mh_set_stop_at_ref_mismatch.argtypes = [ctypes.c_int]
	case = vcf_scan_cases.Case("stops", ["S0", "S1", "S2"])
	for k in range(40):
		case.rec([b"0|1", b"1|0", b"1|1"])
	bad = len(case.lines) - 30
	f = case.lines[bad].split(b"\t")
	f[3] = vcf_scan_cases.other(f[3])                                 # the REF column of the 11th record is not the reference's
	case.lines[bad] = b"\t".join(f)
	fa, vcf = case.write(tmp_path)
	vcf_gz = gz_copy(vcf, tmp_path / "stops.vcf.gz", piece=100)
	try:
		L.v2mh_set_stop_at_ref_mismatch(1)
		want = graph_arrays(host.HostGraph(fa, vcf, "1"))
		monkeypatch.setenv("V2M_RING_SLOT_BYTES", "200")             # a few lines a slice
		for v in (vcf, vcf_gz):
			h = host.HostGraph(fa, v, "1", ctx=ctx, gpu_parse=True)
			assert graph_arrays(h) == want
			assert bad < h.scanned_lines <= bad + 8 < len(case.lines), v
	finally:
		L.v2mh_set_stop_at_ref_mismatch(0)
	assert per_line(ctx.vcf_scan(case.vcf, "1")) == per_line(host_chunks(case))   # the context is as usable as before


# ---- the driver --------------------------------------------------------------------------------

def run(args, check=True):
	assert os.path.exists(CLI), "build the host driver first (__graft_entry__.build())"
	r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
	if check:
		assert r.returncode == 0, r.stderr.decode()
	return r


def test_cli_gpu_parse_gives_the_goldens(tmp_path):
	for stem, fasta in FIXTURES:
		fa, vcf = os.path.join(FIX, fasta), os.path.join(FIX, stem + ".vcf")
		vcf_gz = gz_copy(vcf, tmp_path / "v.vcf.gz", piece=64)
		out = tmp_path / "out.a2m"
		for v in (vcf, vcf_gz):
			r = run(["-H", "-r", fa, "-a", v, "-c", "1", "--gpu-parse", "--verbose", "-s", str(out)])
			assert out.read_bytes() == open(os.path.join(DERIVED, stem + ".haplotypes.a2m"), "rb").read(), (stem, v)
			assert b"lines scanned, 0 declined" in r.stderr, r.stderr
			assert b"inflated on the GPU" not in r.stderr                # the text was never on the host
			run(["-H", "-r", fa, "-a", v, "-c", "1", "--gpu-parse", "--unaligned", "-s", str(out)])
			assert out.read_bytes() == open(os.path.join(DERIVED, stem + ".haplotypes.unaligned.fa"), "rb").read(), (stem, v)


def test_cli_gpu_parse_refuses_a_graph_input(tmp_path):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	run(["-H", "-r", fa, "-a", vcf, "-c", "1", "-f", str(tmp_path / "g.graph"), "-s", str(tmp_path / "o.a2m")])
	r = run(["-H", "-r", fa, "-g", str(tmp_path / "g.graph"), "--gpu-parse", "-s", str(tmp_path / "o2.a2m")], check=False)
	assert r.returncode != 0 and b"--gpu-parse parses --input-variants; it cannot be combined with --input-graph" in r.stderr


def test_cli_reports_no_declined_line_on_test_4(tmp_path):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	r = run(["-H", "-r", fa, "-a", vcf, "-c", "1", "--gpu-parse", "--verbose", "-s", str(tmp_path / "o.a2m")])
	n = len(open(vcf, "rb").read().splitlines())
	assert ("%d lines scanned, 0 declined" % n).encode() in r.stderr


# ---- launches ----------------------------------------------------------------------------------

def test_one_launch_group_per_slice(ctx, monkeypatch):
	from vcf2multialign_amd import _native as N
	case = next(c for c in CASES if c.name == "no_record")              # no layout line: a chunk per slice
	ctx.profile_enable(True)
	try:
		for small in (False, True):
			if small:
				monkeypatch.setenv("V2M_RING_SLOT_BYTES", str(small_slot(case)))
			ctx.profile_reset()
			chunks = ctx.vcf_scan(case.vcf, "1")
			assert len(chunks) > 2 if small else len(chunks) == 1
			assert ctx.profile_get(N.KERNEL_VCF)[0] == len(chunks) and ctx.profile_get(N.KERNEL_INFLATE)[0] == 0
			ctx.profile_reset()
			chunks = ctx.vcf_scan(bgzf(case.vcf, piece=100), "1")
			assert ctx.profile_get(N.KERNEL_VCF)[0] == len(chunks) == ctx.profile_get(N.KERNEL_INFLATE)[0]
	finally:
		ctx.profile_enable(False)


# ---- the checked build -------------------------------------------------------------------------

CHECKED_CORPUS = [
	"tests/test_gpu_vcf_scan.py::test_hand_made_vcfs_equal_the_host_scanner",
	"tests/test_gpu_vcf_scan.py::test_row_counts_at_the_word_seams",
	"tests/test_gpu_vcf_scan.py::test_every_byte_phase_of_a_step",
	"tests/test_gpu_vcf_scan.py::test_lines_straddle_slices_and_members",
	"tests/test_gpu_vcf_scan.py::test_graphs_of_the_fixtures",
	"tests/test_gpu_vcf_scan.py::test_graphs_of_the_hand_made_vcfs",
	"tests/test_gpu_vcf_scan.py::test_graph_of_mini3_and_the_error_messages",
]


def test_corpus_on_the_checked_build():
	# the same output under two poison seeds: nothing read that this call did not write
	from test_gpu_checked_build import SEEDS, run_checked_corpus
	from vcf2multialign_amd import build
	assert os.path.exists(build.CHECKED_LIB_PATH) and os.path.exists(build.CHECKED_HOST_LIB_PATH), "build_native() builds them"
	for seed in SEEDS:   # the second seed only once the first has passed
		rc, out = run_checked_corpus(seed, build.CHECKED_LIB_PATH, build.CHECKED_HOST_LIB_PATH, corpus=CHECKED_CORPUS, timeout=600)
		assert rc == 0, "checked build, seed %s: exit %d\n%s" % (seed, rc, out[-6000:])
