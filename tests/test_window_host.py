"""Column windows on the CPU: the reference-range -> column mapping (Python and C++ agree, the REF row has ref[p] at col(p)), the
CLI's --region errors (reported before any device is opened) and the new C ABI symbols."""

import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import oracle
import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIX = os.path.join(HERE, "golden", "reference-fixtures")
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
PLOIDY_MAX = 0xFFFFFFFF


def _fixture_cases():
	cases = []
	for sub in ("variant-graph", "founder-sequences"):
		d = os.path.join(FIX, sub)
		for vcf in sorted(f for f in os.listdir(d) if f.endswith(".vcf")):
			fa = re.sub(r"[ab]?\.vcf$", ".fa", vcf)
			if os.path.exists(os.path.join(d, fa)):
				cases.append((os.path.join(d, fa), os.path.join(d, vcf)))
	return cases


def _check_mapping(fa, vcf, g):
	from vcf2multialign_amd.host import HostGraph
	from vcf2multialign_amd.variant_graph import VariantGraph
	hg = HostGraph(fa, vcf, "1")
	vg = VariantGraph.from_object(g)
	R, L = len(g.ref), int(g.aligned_positions[-1])
	assert int(g.reference_positions[-1]) == R
	ref_row = g.output_sequence(g.ref, copy_index=PLOIDY_MAX)
	assert len(ref_row) == L
	ends = list(range(1, R + 1)) if R <= 400 else sorted(set([1, R] + list(np.random.default_rng(R).integers(1, R + 1, size=300))))
	for p in range(R):
		b, _ = vg.columns_of_reference_range(p, p + 1)
		assert ref_row[b:b + 1] == g.ref[p:p + 1], p                # col(p) holds ref[p]
	for s in ends[:50] + [0]:
		for e in ends:
			if s < e:
				assert vg.columns_of_reference_range(s, e) == hg.columns_of_reference_range(s, e), (s, e)
	assert vg.columns_of_reference_range(0, R) == (0, L) == hg.columns_of_reference_range(0, R)   # col(0) = 0, col(R) = L
	for s, e in ((0, 0), (3, 2), (0, R + 1), (R, R + 1)):
		with pytest.raises(ValueError):
			vg.columns_of_reference_range(s, e)
		with pytest.raises(ValueError):
			hg.columns_of_reference_range(s, e)


@pytest.mark.parametrize("fa,vcf", _fixture_cases(), ids=lambda x: os.path.basename(x))
def test_mapping_on_reference_fixtures(fa, vcf):
	_check_mapping(fa, vcf, oracle.build_variant_graph(fa, vcf, "1"))


@pytest.mark.parametrize("seed", range(6))
def test_mapping_on_synthetic_graphs(tmp_path, seed):
	g = synth.build_case(tmp_path, 300 + seed, 3000 + 2000 * seed, 200 + 50 * seed, 3, long_every=7, multi_allelic=0.2)
	_check_mapping(str(tmp_path / "synth.fa"), str(tmp_path / "synth.vcf"), g)


def test_unaligned_ref_window_is_the_reference_range(tmp_path):
	"""The REF row's unaligned bytes whose columns lie in [col(s), col(e)) are ref[s:e] (what --region --unaligned gives for REF)."""
	from vcf2multialign_amd.variant_graph import columns_of_reference_range
	g = synth.build_case(tmp_path, 5, 5000, 400, 2, long_every=5)
	row = g.output_sequence(g.ref, copy_index=PLOIDY_MAX)
	col = np.full(len(row), -1)
	rp, ap = [int(x) for x in g.reference_positions], [int(x) for x in g.aligned_positions]
	for n in range(len(rp) - 1):
		col[ap[n]:ap[n] + rp[n + 1] - rp[n]] = np.arange(rp[n], rp[n + 1])
	rng = np.random.default_rng(0)
	for _ in range(200):
		s = int(rng.integers(0, len(g.ref)))
		e = int(rng.integers(s + 1, len(g.ref) + 1))
		b, en = columns_of_reference_range(g.reference_positions, g.aligned_positions, s, e)
		keep = col[b:en] >= 0
		assert bytes(np.frombuffer(row[b:en], np.uint8)[keep]) == g.ref[s:e]


@pytest.mark.parametrize("value,message", [
	("abc", b"--region must be START-END"), ("10", b"--region must be START-END"), ("0-5", b"--region must be START-END"),
	("7-3", b"--region must be START-END"), ("1-", b"--region must be START-END"), ("-5", b"--region must be START-END"),
	("1-99999999", b"past the end of the reference sequence")])
def test_cli_region_errors(value, message):
	d = os.path.join(FIX, "variant-graph")
	r = subprocess.run([CLI, "-H", "-r", os.path.join(d, "test-4.fa"), "-a", os.path.join(d, "test-4.vcf"), "-c", "1", "-s", "/dev/null",
		"--region=" + value, "--device=99"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
	assert r.returncode == 1, r.stderr.decode()
	assert message in r.stderr, r.stderr.decode()
	assert b"GPU" not in r.stderr and b"device" not in r.stderr.lower().replace(b"--device", b"")


def test_cli_usage_names_region():
	r = subprocess.run([CLI, "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
	assert b"--region=START-END" in r.stderr


def test_symbols_exported():
	from vcf2multialign_amd import build
	lib = C.CDLL(build.LIB_PATH)
	for name in ("v2m_set_column_window", "v2m_window_length"):
		assert hasattr(lib, name)
	host = C.CDLL(build.HOST_LIB_PATH)
	assert hasattr(host, "v2mh_columns_of_reference_range")
	header = open(os.path.join(ROOT, "include", "v2m_hip.h")).read()
	assert "int v2m_set_column_window(v2m_ctx *ctx, uint64_t col_begin, uint64_t col_end);" in header
	assert "uint64_t v2m_window_length(const v2m_ctx *ctx);" in header
	assert "#define V2M_ABI_VERSION 5" in header
