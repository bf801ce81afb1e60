"""tests/inflate_seams.py without a GPU: its walker against zlib and tests/deflate_ref.py on every member the builders make and on a
zlib corpus, the status it names for every refused member, and the census: every seam of bgzf_inflate_kernel that the GPU test
(tests/test_gpu_inflate_seams.py) relies on is reached by the members, proved from their bytes alone.  A seam nobody reaches fails."""

import pytest

import deflate_ref
import inflate_seams as S
from bgzf_input_util import EOF_MEMBER, bgzf, deflate_raw, member, member_accepted, zlib_inflate


def test_constants_and_status_names():
	assert (S.LIT_ROOT, S.DIST_ROOT, S.CL_ROOT, S.LANES, S.WINDOW_BITS, S.CRC_LANE, S.SLOT, S.HEADER, S.FOOTER) == (10, 8, 7, 64, 2048, 1024, 65536, 18, 8)
	assert S.STATUS[0] == "Ok" and S.STATUS[-1] == "BadFraming" and len(set(S.STATUS)) == 17
	assert S.STATUS_TEXT["PastPayload"] == "the deflate stream reads past the payload" and S.STATUS_TEXT["BadCrc"] == "CRC-32 mismatch"
	assert len(set(S.STATUS_TEXT.values())) == 17   # a message names one status


@pytest.mark.parametrize("group", S.GROUPS)
def test_walker_zlib_and_deflate_ref_agree(group):
	members, _ = S.groups()[group]
	assert len({name for name, _ in members}) == len(members)
	for name, m in members:
		w = S.walk_member(m)
		payload = m[S.HEADER:len(m) - S.FOOTER]
		assert w.status == "Ok", (name, w.status)
		assert w.data == member_accepted(m), name                                       # zlib, CRC-32 and ISIZE
		assert w.data == deflate_ref.detokenize(deflate_ref.inflate_tokens(payload)), name
		assert [r for r in w.records if r.kind != "seek" and r.n < 1] == [], name
		for a, b in zip(w.records, w.records[1:]):                                      # the records tile the stream: only padding between them
			assert a.bit + a.n <= b.bit < a.bit + a.n + 8 or "seek" == b.kind, (name, a, b)
		if group.startswith("matches"):
			assert S.sources_are_distinct(m), "%s: a match copies bytes of which two within 256 are equal" % name


def test_neighbours_differ():
	"""An overrun into the next member's output changes a byte: neighbours in a file do not begin alike."""
	for group in S.GROUPS:
		prev = None
		for name, m in S.groups()[group][0]:
			data = S.walk_member(m).data
			if data:
				assert prev is None or data[:16] != prev[:16], (group, name)
				prev = data


def test_refused_members():
	statuses = set()
	for name, status, build in S.refusals():
		for lead in range(4):
			m = build(lead)
			assert zlib_inflate(m[S.HEADER:len(m) - S.FOOTER]) is None or member_accepted(m) is None, name   # the construction is what it claims
			assert S.walk_member(m, lead).status == status, (name, lead)
		statuses.add(status)
	assert statuses == set(S.GPU_STATUSES) and len(S.GPU_STATUSES) == 15
	# the sixteenth: framing, which the host's scan refuses before any kernel runs
	assert S.walk(b"\x03\x00", isize=S.SLOT + 1).status == "BadFraming" and S.walk(bytes(S.SLOT - S.HEADER - S.FOOTER + 1)).status == "BadFraming"


def test_refusals_at_the_payload_bound():
	"""The two end-of-block cases differ from an accepted member in the payload bound alone."""
	by_name = {name: build for name, _, build in S.refusals()}
	for lead in range(4):
		m = by_name["end-of-block code supplied by the footer"](lead)
		plen = len(m) - S.HEADER - S.FOOTER
		assert len(S.visible_tail(m, lead)) == 3 and 0 == m[len(m) - S.FOOTER] & 0x7f
		longer = S.walk(m[S.HEADER:len(m) - S.FOOTER + 1])   # with the footer's first byte as payload the stream is whole
		assert longer.status == "Ok" and S.walk_member(m, lead).bits == 8 * plen + 7
		assert member_accepted(member(m[S.HEADER:len(m) - S.FOOTER + 1], longer.data)) == longer.data
		m = by_name["end-of-block code one bit short of the padding"](lead)
		plen = len(m) - S.HEADER - S.FOOTER
		assert S.visible_tail(m, lead) == b"" and S.walk_member(m, lead).bits == 8 * plen + 1


@pytest.mark.parametrize("group", S.GROUPS)
def test_every_seam_is_reached(group):
	members, seams = S.groups()[group]
	c, pairs, n_slices, where = S.file_census([m for _, m in members])
	assert n_slices == 1 and len(where) == len(members) + 1
	missing = [s for s in seams if c[s] < 1]
	assert missing == [], "%s: %d of %d seams are not reached: %s" % (group, len(missing), len(seams), missing[:20])


def test_the_match_crosses_are_whole():
	pairs = set()
	for part in range(S.MATCH_PARTS):
		pairs |= S.file_census([m for _, m in S.match_group(part)])[1]
	assert len(S.SMALL_CROSS) == 66 * 256 and len(S.LARGE_CROSS) == 81
	missing = [p for p in S.SMALL_CROSS + S.LARGE_CROSS if p not in pairs]
	assert missing == [], missing[:20]
	offsets = {p % 64 for part in range(S.MATCH_PARTS) for _, m in S.match_group(part) for p, _, _ in S.walk_member(m).matches}
	assert len(offsets) == 64   # p at every phase of the wave


def test_seam_lists_name_everything():
	"""What the issue lists, by count: 10 kinds x 2, 12 leads, 32 phases, 12 seeks; 320 small outputs; every length of every code."""
	assert len(S.BITS_SEAMS) == len(set(S.BITS_SEAMS)) == 20 + 12 + 5 + 32 + 12
	assert len(S.OUTPUT_SEAMS) == len(set(S.OUTPUT_SEAMS)) == 20 * 16 + 2 + 11
	assert len(S.TABLES_SEAMS) == len(set(S.TABLES_SEAMS)) == 22 + 2 * (15 + 15 + 7) + 8 + 2
	# HCLEN 4 describes zero lengths only, so it is reached by a refused stream (NoEndOfBlock), not by a member
	m = {name: build for name, _, build in S.refusals()}["HCLEN 4"](0)
	assert S.census(m, 0, 0)[0]["hclen_4"] == 1


def test_the_census_follows_the_placement():
	"""A member built for one lead misses its seam at another, and a phase moves with the output offset: the census reads the placement."""
	m = S.mk(S.placed(2, "counts", "end_on"))
	assert S.census(m, 0, 0)[0]["end_on_counts"] == 1 and S.census(m, 1, 0)[0]["end_on_counts"] == 0
	m = S.mk(S.small_output(5, 1))
	assert S.census(m, 0, 7)[0]["isize_5_phase_7"] == 1 and S.census(m, 0, 8)[0]["isize_5_phase_7"] == 0
	m = S.mk(S.chain(1))
	for offset in range(4):   # (a byte more of lead turns the phases by 8: every phase once, wherever the member lies)
		assert [S.census(m, offset, 0)[0]["chain_phase%d" % ph] for ph in range(32)] == [1] * 32


def test_slices_mirror_the_greedy_cut():
	data = bytes(range(256)) * 2000
	f = bgzf(data, level=0)                                                              # 8 members (a stored block and an empty final one each) and the EOF member
	sizes, isizes = [65280 + 10 + 26] * 7 + [len(data) - 7 * 65280 + 10 + 26, 28], [65280] * 7 + [len(data) - 7 * 65280, 0]
	assert sum(sizes) == len(f)
	assert S.slices(sizes, isizes) == [0, 9]
	assert S.slices(sizes, isizes, 1) == list(range(8)) + [9]                            # (the EOF member rides with the last)
	assert S.slices(sizes, isizes, 200000) == [0, 3, 6, 9]


@pytest.mark.parametrize("strategy", ["default", "filtered", "huffman", "rle", "fixed"])
def test_walker_on_the_zlib_corpus(strategy):
	from test_gpu_bgzf_input import KINDS
	for level in range(10):
		for kind in KINDS:
			data = KINDS[kind](1500 + 37 * level)
			payload = deflate_raw(data, level=level, strategy=strategy)
			w = S.walk(payload)
			assert w.status == "Ok" and w.data == data == zlib_inflate(payload), (strategy, level, kind)
	data = KINDS["vcf"](30000)
	assert S.walk(deflate_raw(data, strategy=strategy, mem_level=1)).data == data            # many blocks
	assert EOF_MEMBER[S.HEADER:-S.FOOTER] == b"\x03\x00" and S.walk(b"\x03\x00").data == b""
