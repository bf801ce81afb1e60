"""The gfx950 instructions of the neighbour-joining kernels (csrc/nj_kernels.hpp), cross-compiled as tests/test_kernel_isa.py compiles
the library, in the product and the checked build: no GPU needed.

The tree is defined with every operation rounded on its own.  At -O3 hipcc fuses a product and a sum into v_fma_f64 unless the function
says `#pragma clang fp contract(off)`; a contracted Q changed no record of the corpus items it was tried on
(tests/test_nj_tree_host.py), so no run pins it: the instructions do."""

import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD_FLAGS = {"product": [], "checked": ["-DV2M_CHECKED_BUILD"]}          # as tests/test_kernel_isa.py
KERNELS = ("nj_init_kernel", "nj_rowmin_kernel", "nj_join_kernel", "nj_last_kernel")


@pytest.fixture(scope="module", params=["product", "checked"])
def nj_isa(request, tmp_path_factory):
	"""{kernel: its lines} of the four kernels, and the whole text under "__text__"."""
	from vcf2multialign_amd import build
	hipcc = build.find_hipcc()
	if hipcc is None:
		pytest.skip("hipcc not found")
	out = tmp_path_factory.mktemp("nj_isa") / "v2m_hip.s"
	subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only"] + BUILD_FLAGS[request.param] + ["-o", str(out), build.HIP_SOURCES[0]], cwd=ROOT)
	text = out.read_text()
	kernels, name, cur = {}, None, []
	for line in text.split("\n"):
		m = re.match(r"^(_ZN3v2m\w+):", line)
		if m:
			name, cur = m.group(1), []
		elif name:
			cur.append(line.split(";")[0].strip())
			if "s_endpgm" in line:
				for k in KERNELS:
					if re.match(r"_ZN3v2m\d+%sE" % k, name):
						kernels[k] = cur
				name = None
	assert sorted(kernels) == sorted(KERNELS)
	kernels["__text__"] = text
	return kernels


def test_the_rowmin_kernel_holds_no_fused_multiply_add(nj_isa):
	lines = nj_isa["nj_rowmin_kernel"]
	assert not [l for l in lines if re.search(r"fma|v_ma[dc]_(f|legacy|mix)", l)]          # (v_mad_u64_u32 is address arithmetic)
	assert any(l.startswith("v_mul_f64") for l in lines) and any(l.startswith("v_add_f64") for l in lines)
	# the hot loop reads 16 bytes at a time
	assert any(l.startswith("global_load_dwordx4") for l in lines)


def test_no_nj_kernel_uses_scratch(nj_isa):
	text = nj_isa["__text__"]
	sizes = dict(re.findall(r"\.amdhsa_kernel (_ZN3v2m\w+).*?\.amdhsa_private_segment_fixed_size (\d+)", text, flags=re.S))
	mine = {k: int(v) for k, v in sizes.items() if any(re.match(r"_ZN3v2m\d+%sE" % name, k) for name in KERNELS)}
	assert len(mine) == len(KERNELS) and not any(mine.values()), mine
	for name in KERNELS:
		assert not [l for l in nj_isa[name] if l.startswith(("scratch_", "buffer_"))], name


def test_the_only_fused_multiply_adds_belong_to_the_division(nj_isa):
	"""`/` on doubles is the correctly rounded v_div_scale / v_rcp / v_fma ... / v_div_fmas / v_div_fixup sequence: its v_fma_f64 are
	part of one IEEE operation.  The join kernel has no other, and the other kernels have none at all."""
	for name in ("nj_init_kernel", "nj_last_kernel"):
		assert not [l for l in nj_isa[name] if "fma" in l], name
	lines = nj_isa["nj_join_kernel"]
	inside, divisions, outside = False, 0, []
	for l in lines:
		if l.startswith("v_div_scale_f64") and not inside:
			inside = True
			divisions += 1
		elif l.startswith("v_div_fixup_f64"):
			inside = False
		elif "fma" in l and not l.startswith("v_div_fmas_f64") and not inside:
			outside.append(l)
	assert divisions == 1 and not inside and not outside, (divisions, outside)
	assert any(l.startswith("v_fma_f64") for l in lines)                     # (the sequence is there: the test would see one outside it)
