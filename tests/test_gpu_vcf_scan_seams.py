"""The VCF scan kernels (csrc/vcf_kernels.hpp) and their slice driver (v2m_vcf_scan) against a model of the rule written from the header
alone (tests/vcf_scan_model.py), at every seam of their passes (tests/vcf_scan_seams.py: tiles and leads of the line index, the steps of
the head and the genotype pass, the blocks of the scans, the widths of the column instances).  tests/test_vcf_scan_model_host.py
asserts on the CPU that the texts reach those seams.  Every comparison is bit for bit; the host's scanner is compared as well, chunk by
chunk."""

import os

import pytest

import vcf_scan_model as model
import vcf_scan_seams as seams
from bgzf_input_util import bgzf
from test_gpu_vcf_scan import assert_same_chunks

pytestmark = pytest.mark.gpu

V2M_ERR_UNSUPPORTED = 3
PIECES = (7, 100, 65280)


@pytest.fixture(scope="module")
def ctx():
	import vcf2multialign_amd as v2m
	with v2m.Context(0) as c:
		yield c


def set_slot(monkeypatch, slot):
	if slot:
		monkeypatch.setenv("V2M_RING_SLOT_BYTES", str(slot))
	else:
		monkeypatch.delenv("V2M_RING_SLOT_BYTES", raising=False)


def check(ctx, monkeypatch, t):
	"""The plain text at slot 0 and at the group's slot: the model's lines in the header's chunking, and the host scanner's chunks."""
	from vcf2multialign_amd import host
	lines, at = model.scan_text(t.text, t.wanted, t.layout_fn)
	for slot in (0, t.slot):
		set_slot(monkeypatch, slot)
		got = ctx.vcf_scan(t.text, t.wanted, t.layout_fn)
		assert ctx.vcf_layout_line == at, (t.name, slot)
		model.check_chunks(got, lines, at, (t.name, slot))
		rc, want = host.scan_lines_host(t.text, t.wanted, layout=t.layout_fn, slice_bytes=slot)
		assert rc == 0
		assert_same_chunks(got, want, (t.name, slot))
		assert [c["n_columns"] for c in got] == [c["n_columns"] for c in want], (t.name, slot)


def check_bgzf(ctx, monkeypatch, t):
	"""The text as BGZF in pieces of 7, 100 and 65 280 bytes: whole members, so the slices are cut elsewhere; the lines say the same."""
	lines, at = model.scan_text(t.text, t.wanted, t.layout_fn)
	for piece in PIECES:
		set_slot(monkeypatch, 0 if piece > 100 else t.slot)
		got = ctx.vcf_scan(bgzf(t.text, piece=piece), t.wanted, t.layout_fn)
		model.check_chunks(got, lines, at, (t.name, "pieces of %d" % piece))


def thinned(t, every, keep=3):
	"""The first lines and every `every`-th line after them."""
	lines = model.split_lines(t.text)
	return t._replace(name=t.name + "_thinned", text=seams.joined(lines[:keep] + lines[keep::every]))


# ---- A: the line index ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("part", ["leads", "edges"])
def test_line_index(ctx, monkeypatch, part):
	for t in seams.group_a():
		if t.name.startswith("A_lead") == ("leads" == part):
			check(ctx, monkeypatch, t)


def test_more_than_1024_tiles_and_lines(ctx, monkeypatch):
	check(ctx, monkeypatch, seams.a_big())


def test_a_slice_without_a_whole_line(ctx, monkeypatch):
	from vcf2multialign_amd import _native as N
	t, piece = seams.no_whole_line_then_one()
	lines, at = model.scan_text(t.text, t.wanted, t.layout_fn)
	set_slot(monkeypatch, t.slot)
	ctx.profile_enable(True)
	try:
		ctx.profile_reset()
		got = ctx.vcf_scan(bgzf(t.text, piece=piece), t.wanted, t.layout_fn)
		n_slices = ctx.profile_get(N.KERNEL_VCF)[0]
	finally:
		ctx.profile_enable(False)
	model.check_chunks(got, lines, at, t.name)
	slices = seams.bgzf_slices(t.text, piece, t.slot)
	assert b"\n" not in t.text[:slices[0][1]] and n_slices == len(slices)   # the first slice gave no chunk; the second holds line 0 and the layout line
	assert [(c["first_line"], len(c["lines"])) for c in got[:2]] == [(0, 1), (1, 1)]


# ---- B: the head pass -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [t.name for t in seams.group_b()])
def test_head_pass(ctx, monkeypatch, name):
	(t,) = [t for t in seams.group_b() if t.name == name]
	check(ctx, monkeypatch, t)


# ---- C: the genotype pass ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("quarter", range(4))
def test_genotype_pass(ctx, monkeypatch, quarter):
	(t,) = seams.group_c(pads=range(16 * quarter, 16 * quarter + 16))
	check(ctx, monkeypatch, t)


# ---- D: the layout's widths -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", [t.name for t in seams.group_d()])
def test_layout_widths(ctx, monkeypatch, name):
	(t,) = [t for t in seams.group_d() if t.name == name]
	check(ctx, monkeypatch, t)


def test_unsupported_widths(ctx, monkeypatch):
	from vcf2multialign_amd.context import V2MError
	set_slot(monkeypatch, 0)
	for t in seams.d_unsupported():
		with pytest.raises(V2MError) as e:
			ctx.vcf_scan(t.text, t.wanted, t.layout_fn)
		assert e.value.code == V2M_ERR_UNSUPPORTED and "at most 32768 (512 words) are supported" in str(e.value), str(e.value)
		check(ctx, monkeypatch, seams.group_d()[0])                       # the context works as before


# ---- E: the grammar ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seed", seams.E_SEEDS)
def test_grammar(ctx, monkeypatch, seed):
	(t,) = [t for t in seams.group_e() if t.name == "E_seed_%d" % seed]
	check(ctx, monkeypatch, t)


# ---- BGZF -------------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["head", "genotypes", "grammar"])
def test_bgzf_pieces(ctx, monkeypatch, which):
	if "head" == which:
		texts = [thinned(t, 23) for t in seams.group_b() if t.name in ("B_info", "B_alts", "B_formats", "B_tabs")] + [t for t in seams.group_b() if t.name == "B_name_65"]
	elif "genotypes" == which:
		texts = seams.group_c(pads=(0, 21, 42, 63))
	else:
		texts = [thinned(seams.group_e()[0], 17)]
	for t in texts:
		check_bgzf(ctx, monkeypatch, t)


# ---- the checked build ------------------------------------------------------------------------------------------------------------------

CHECKED_CORPUS = [
	"tests/test_gpu_vcf_scan_seams.py::test_line_index",
	"tests/test_gpu_vcf_scan_seams.py::test_more_than_1024_tiles_and_lines",
	"tests/test_gpu_vcf_scan_seams.py::test_a_slice_without_a_whole_line",
	"tests/test_gpu_vcf_scan_seams.py::test_head_pass[B_alts]",
	"tests/test_gpu_vcf_scan_seams.py::test_head_pass[B_tabs]",
	"tests/test_gpu_vcf_scan_seams.py::test_head_pass[B_name_65]",
	"tests/test_gpu_vcf_scan_seams.py::test_head_pass[B_name_130]",
	"tests/test_gpu_vcf_scan_seams.py::test_genotype_pass[0]",
	"tests/test_gpu_vcf_scan_seams.py::test_genotype_pass[3]",
	"tests/test_gpu_vcf_scan_seams.py::test_layout_widths",
	"tests/test_gpu_vcf_scan_seams.py::test_unsupported_widths",
	"tests/test_gpu_vcf_scan_seams.py::test_grammar[1]",
	"tests/test_gpu_vcf_scan_seams.py::test_bgzf_pieces[genotypes]",
]


def test_corpus_on_the_checked_build():
	# the same output under two poison seeds: nothing read that this call did not write
	from test_gpu_checked_build import SEEDS, run_checked_corpus
	from vcf2multialign_amd import build
	assert os.path.exists(build.CHECKED_LIB_PATH) and os.path.exists(build.CHECKED_HOST_LIB_PATH), "build_native() builds them"
	for seed in SEEDS:   # the second seed only once the first has passed
		rc, out = run_checked_corpus(seed, build.CHECKED_LIB_PATH, build.CHECKED_HOST_LIB_PATH, corpus=CHECKED_CORPUS, timeout=600)
		assert rc == 0, "checked build, seed %s: exit %d\n%s" % (seed, rc, out[-6000:])
