"""bgzf_inflate_kernel (csrc/bgzf_kernels.hpp) through v2m_bgzf_decompress at every seam of its bit reader, its tables, its match copy and
its copy-out (tests/inflate_seams.py), against a plain bit-by-bit walker of RFC 1951, byte for byte; and the refusal reason of every
single-fault member.  tests/test_inflate_seams_host.py proves on the CPU that the members reach the seams and that the walker equals zlib
and tests/deflate_ref.py on them; here the census is taken again for the slices each run really made (the greedy cut is mirrored and
its slice count held against the profile's launch count), so reach is asserted for what ran."""

import os

import pytest

import inflate_seams as S
from bgzf_input_util import EOF_MEMBER

pytestmark = pytest.mark.gpu

V2M_ERR_INVALID_ARGUMENT = 1
# the ring slot: the default (one slice), the smallest (64 KiB a slice: members start again at slice offset 0, output phase 0), one between
SLOTS = {"default": None, "smallest": 1, "between": 70000}


@pytest.fixture(scope="module")
def ctx():
	import vcf2multialign_amd as v2m
	with v2m.Context(0) as c:
		yield c


def decompress_counting(ctx, monkeypatch, f, slot):
	import vcf2multialign_amd as v2m
	if slot is None:
		monkeypatch.delenv("V2M_RING_SLOT_BYTES", raising=False)
	else:
		monkeypatch.setenv("V2M_RING_SLOT_BYTES", str(slot))
	ctx.profile_enable(True)
	ctx.profile_reset()
	try:
		got = ctx.bgzf_decompress(f)
		launches, _ = ctx.profile_get(v2m._native.KERNEL_INFLATE)
	finally:
		ctx.profile_enable(False)
	return got, launches


@pytest.mark.parametrize("setting", list(SLOTS))
@pytest.mark.parametrize("group", S.GROUPS)
def test_accepted_groups(ctx, monkeypatch, group, setting):
	members, seams = S.groups()[group]
	blobs = [m for _, m in members]
	want = [S.walk_member(m).data for m in blobs]
	c, pairs, n_slices, where = S.file_census(blobs, SLOTS[setting])
	got, launches = decompress_counting(ctx, monkeypatch, b"".join(blobs) + EOF_MEMBER, SLOTS[setting])
	assert launches == n_slices, "the mirror of the greedy cut says %d slices, the kernel ran %d times" % (n_slices, launches)
	if got != b"".join(want):
		at = 0
		for (name, _), w in zip(members, want):
			assert got[at:at + len(w)] == w, "%s, %s: member %r (output bytes %d..%d) differs" % (group, setting, name, at, at + len(w))
			at += len(w)
		assert len(got) == at, (group, setting, len(got), at)
	# reach, for the slices that ran
	if "default" == setting:
		assert 1 == n_slices
		missing = [s for s in seams if c[s] < 1]
	else:
		one_slice = S.file_census(blobs)[3]
		if sum(map(len, blobs)) > S.SLOT:
			assert n_slices > 1 and where != one_slice, "the setting moves members to other leads and phases"
		missing = [s for s in seams if S.placement_free(s) and c[s] < 1]
	assert missing == [], (group, setting, missing[:20])
	if group.startswith("matches"):
		assert pairs == S.file_census(blobs)[1]


def test_the_match_crosses_ran_whole(ctx):
	"""(What the groups above ran: the union of their matches is the two crosses.)"""
	pairs = set()
	for part in range(S.MATCH_PARTS):
		pairs |= S.file_census([m for _, m in S.match_group(part)])[1]
	assert set(S.SMALL_CROSS + S.LARGE_CROSS) <= pairs


def test_refused_members(ctx):
	import vcf2multialign_amd as v2m
	seen = set()
	for k, (name, status, build) in enumerate(S.refusals()):
		prefix = S.spacer(10 + k % 7, k % 4, salt=k)                          # a valid member first; its size moves the lead
		lead = (len(prefix) + S.HEADER) % 4
		m = build(lead)
		assert S.walk_member(m, lead).status == status, name
		with pytest.raises(v2m.V2MError) as e:
			ctx.bgzf_decompress(prefix + m + EOF_MEMBER)
		assert e.value.code == V2M_ERR_INVALID_ARGUMENT, (name, str(e.value))
		assert "BGZF member 1 at compressed offset %d: %s" % (len(prefix), S.STATUS_TEXT[status]) in str(e.value), (name, status, str(e.value))
		seen.add((status, lead))
	assert {s for s, _ in seen} == set(S.GPU_STATUSES) and {lead for _, lead in seen} == {0, 1, 2, 3}


# ---- the checked build -------------------------------------------------------------------------

CHECKED_CORPUS = [
	"tests/test_gpu_inflate_seams.py::test_accepted_groups",
	"tests/test_gpu_inflate_seams.py::test_refused_members",
]


def test_seams_on_the_checked_build():
	from test_gpu_checked_build import SEEDS, run_checked_corpus
	from vcf2multialign_amd import build
	assert os.path.exists(build.CHECKED_LIB_PATH) and os.path.exists(build.CHECKED_HOST_LIB_PATH), "build_native() builds them"
	for seed in SEEDS:   # the second seed only once the first has passed
		rc, out = run_checked_corpus(seed, build.CHECKED_LIB_PATH, build.CHECKED_HOST_LIB_PATH, corpus=CHECKED_CORPUS, timeout=600)
		assert rc == 0, "checked build, seed %s: exit %d\n%s" % (seed, rc, out[-6000:])
		assert " passed" in out and "libv2m_hip_checked.so" in out, out[-3000:]
