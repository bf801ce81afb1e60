"""Checks on the gfx950 ISA hipcc emits for the product's kernels (cross-compiled here, no GPU needed).

Why: round 2 found transposes with a few hundred wrong words out of 79 M, now and then.  The cause was in the generated code,
not in the source: the s_barrier at the head of a software-pipelined loop had no `s_waitcnt lgkmcnt(0)` on the path from the
previous iteration's ds_write (the wait __syncthreads() implies had been dropped on the loop's back edge), so a wave could pass
the barrier before another wave's LDS store had landed.  The kernel now carries an explicit wait; this test keeps every barrier
of every kernel honest."""

import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


BUILD_FLAGS = {"product": [], "tuning": ["-DV2M_TUNING_BUILD"], "checked": ["-DV2M_CHECKED_BUILD"]}


@pytest.fixture(scope="module", params=["product", "tuning", "checked"])
def isa(request, tmp_path_factory):
	"""The emitted ISA of the product build, of the tuning build (-DV2M_TUNING_BUILD: every transpose variant that can be timed) and of
	the checked build (-DV2M_CHECKED_BUILD: LDS poisoned before use, tests only)."""
	from vcf2multialign_amd import build
	hipcc = build.find_hipcc()
	if hipcc is None:
		pytest.skip("hipcc not found")
	out = tmp_path_factory.mktemp("isa") / "v2m_hip.s"
	extra = BUILD_FLAGS[request.param]
	subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only"] + extra + ["-o", str(out), build.HIP_SOURCES[0]], cwd=ROOT)
	kernels, name, cur = {}, None, []
	for line in out.read_text().split("\n"):
		m = re.match(r"^(_ZN3v2m\w+):", line)
		if m:
			if name:
				kernels[name] = cur
			name, cur = m.group(1), []
		elif name:
			cur.append(line)
			if "s_endpgm" in line:
				kernels[name] = cur
				name = None
	assert len(kernels) > (20 if request.param == "tuning" else 12)
	if request.param == "product":   # the measured-only shapes are not in the product library
		# 8x8 panel, stream16, lines8 and lines16 (each plain and with merged column ends)
		assert sum("transpose_bits" in k for k in kernels) == 6 and not any("ring" in k for k in kernels), sorted(k for k in kernels if "transpose_bits" in k)
	kernels["__text__"] = out.read_text()
	return kernels


def test_every_barrier_waits_for_lds_first(isa):
	"""Walking back from each s_barrier inside its basic block, an `s_waitcnt ... lgkmcnt(0)` must come before any LDS
	instruction or the block's label."""
	offenders = []
	n_barriers = 0
	for name, lines in isa.items():
		if name == "__text__":
			continue
		for i, line in enumerate(lines):
			if "s_barrier" not in line:
				continue
			n_barriers += 1
			found = None
			for prev in reversed(lines[:i]):
				s = prev.strip()
				if s.startswith(".LBB"):
					break
				if s.startswith("s_waitcnt") and "lgkmcnt(0)" in s:
					found = True
					break
				if s.startswith("ds_"):
					break
			if not found:
				offenders.append(name)
	assert n_barriers > 50
	assert not offenders, "s_barrier without a preceding LDS wait in: " + ", ".join(sorted(set(offenders)))


def test_no_scratch_and_no_mfma(isa):
	"""Integer copy / index work: no kernel spills to scratch memory, none uses the matrix cores."""
	text = isa["__text__"]
	sizes = re.findall(r"\.amdhsa_kernel (_ZN3v2m\w+).*?\.amdhsa_private_segment_fixed_size (\d+)", text, flags=re.S)
	assert len(sizes) >= 16 and len(sizes) == len(isa) - 1
	assert [n for n, size in sizes if int(size) != 0] == []
	assert "v_mfma" not in text


def test_no_kernel_touches_m0(isa):
	"""Nothing in the library needs M0 (no LDS-direct loads, no movrel, no GWS); an inline-assembly experiment that does would have to say so here."""
	for name, lines in isa.items():
		if name == "__text__":
			continue
		uses = [l.strip() for l in lines if re.search(r"\bm0\b", l.split(";")[0])]
		assert not uses, (name, uses[:3])


def test_poison_only_in_the_checked_build(isa, request):
	"""The checked build's LDS and scratch poison (kernels.hpp: V2M_POISON_LDS, v2m_lds_poison_seed, poison_fill_kernel) leaves no trace in
	the product's or the tuning build's device code; the checked build has it."""
	text = isa["__text__"]
	if request.node.callspec.params["isa"] == "checked":
		assert "v2m_lds_poison_seed" in text and "poison_fill_kernel" in text
	else:
		assert "poison" not in text.lower()


def _strip_comments(text):
	text = re.sub(r"/\*.*?\*/", lambda m: re.sub(r"[^\n]", " ", m.group(0)), text, flags=re.S)
	return re.sub(r"//[^\n]*", "", text)


def _drop_tuning_only(text):
	"""The text outside `#ifdef V2M_TUNING_BUILD ... #endif` (nested conditionals counted)."""
	out, depth, skip = [], 0, None
	for line in text.split("\n"):
		s = line.strip()
		if s.startswith("#if"):
			depth += 1
			if skip is None and re.match(r"#\s*ifdef\s+V2M_TUNING_BUILD\b", s):
				skip = depth
		elif s.startswith("#endif"):
			if skip == depth:
				skip = None
				depth -= 1
				continue
			depth -= 1
		out.append("" if skip is not None else line)
	return "\n".join(out)


def _functions(text):
	"""The text cut at every line that begins a function or kernel at column 0 (`template`, `__global__`, `__device__`): each piece holds
	one function's head and body (and whatever follows it up to the next one)."""
	return re.split(r"\n(?=template\b|__global__|__device__)", text)


def _shared_names(decl):
	"""The object names a `__shared__ ... ;` declaration declares."""
	decl = re.sub(r"__attribute__\s*\(\(.*?\)\)", " ", decl)
	decl = re.sub(r"\[[^\]]*\]", "[]", decl.replace("__shared__", " "))
	parts = [p.strip() for p in decl.split(",")]
	names = [re.findall(r"(\w+)\s*(?:\[\]\s*)*;?$", parts[0])[0]]
	names += [re.match(r"(\w+)", p).group(1) for p in parts[1:]]
	return names


def test_every_lds_object_is_poisoned_in_the_checked_build():
	"""Lint: every __shared__ object in csrc/*.hpp, outside tuning-only code, is passed to V2M_POISON_LDS in the same function (so that the
	checked build fills it with garbage before the kernel's first LDS access)."""
	import glob
	csrc = os.path.join(ROOT, "vcf2multialign_amd", "csrc")
	seen, missing = 0, []
	for path in sorted(glob.glob(os.path.join(csrc, "*.hpp"))):
		with open(path) as f:
			text = _drop_tuning_only(_strip_comments(f.read()))
		for body in _functions(text):
			for decl in re.findall(r"__shared__[^;]*;", body):
				for name in _shared_names(decl):
					seen += 1
					if not re.search(r"V2M_POISON_LDS\(\s*%s\s*\)" % re.escape(name), body):
						missing.append("%s: %s" % (os.path.basename(path), name))
	assert seen >= 40, seen
	assert not missing, "LDS objects never passed to V2M_POISON_LDS: " + ", ".join(missing)
