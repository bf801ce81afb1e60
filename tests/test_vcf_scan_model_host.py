"""The host's scanner (csrc/host/readers.cc: scan_lines_host) against a model of the rule written from the header alone
(tests/vcf_scan_model.py), on the texts of tests/vcf_scan_seams.py and the hand-made VCFs; and the census of those texts: every seam the
GPU tests of the scan rely on is asserted present here, by name, and a text that has drifted off its seam fails.  No GPU."""

import re

import pytest

import vcf_scan_cases
import vcf_scan_model as model
import vcf_scan_seams as seams

CASES = vcf_scan_cases.cases() + [vcf_scan_cases.padded_case(range(0, 64, 9)), vcf_scan_cases.copies_case(129)]


def host_scan(t, slot):
	from vcf2multialign_amd import host
	rc, chunks = host.scan_lines_host(t.text, t.wanted, layout=t.layout_fn, slice_bytes=slot)
	assert rc == 0, (t.name, rc)
	return chunks


def check(t):
	lines, at = model.scan_text(t.text, t.wanted, t.layout_fn)
	for slot in (0, t.slot):
		chunks = host_scan(t, slot)
		model.check_chunks(chunks, lines, at, (t.name, slot))
		assert len(chunks) <= len(seams.plain_slices(t.text, slot)) + 1


def case_text(case):
	from vcf2multialign_amd.context import first_record_layout
	ex = case.excluded_pairs()
	lengths = sorted(map(len, case.lines))
	return seams.Text(case.name, case.vcf, "1", lambda _i, line: first_record_layout(line, excluded=ex), lengths[-1] + lengths[len(lengths) // 2] + 2)


# ---- the host scanner says what the model says ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_hand_made_vcfs(case):
	t = case_text(case)
	check(t)
	kinds = [k for k, _, _, _ in model.scan_text(t.text, t.wanted, t.layout_fn)[0]]
	assert {i for i, k in enumerate(kinds) if 3 == k} == case.declined           # the model declines what the cases mark


@pytest.mark.parametrize("group", ["a", "b", "c", "d", "e"])
def test_seam_texts(group):
	for t in getattr(seams, "group_" + group)():
		check(t)


def test_the_big_slice():
	check(seams.a_big())


def test_no_included_copy_still_counts_columns():
	"""words_per_column == 0: column_begin and n_columns are the running sums the header promises (the scanner used to say 0)."""
	(t,) = [t for t in seams.group_d() if "D_no_rows" == t.name]
	chunks = host_scan(t, 0)
	assert chunks[-1]["words_per_column"] == 0 and chunks[-1]["n_columns"] == int(chunks[-1]["lines"]["n_alts"].sum()) > 8
	assert chunks[-1]["lines"]["column_begin"].max() > 8


def test_unsupported_widths():
	from vcf2multialign_amd import host
	for t in seams.d_unsupported():
		rc, _ = host.scan_lines_host(t.text, t.wanted, layout=t.layout_fn)
		assert rc == 3, t.name


def test_graph_with_every_copy_excluded(tmp_path):
	"""One haploid sample, excluded: a graph without rows.  The scanned build takes such chunks (columns without words) and gives the text
	path's graph."""
	from vcf2multialign_amd import host
	from test_vcf_scan_host import graph_arrays
	case = vcf_scan_cases.Case("nobody", ["S0"])
	case.exclude = ("S0", 0)
	for k in range(5):
		case.rec([b"%d" % (k & 1)])
	fa, vcf = case.write(tmp_path)
	want = graph_arrays(host.HostGraph(fa, vcf, "1", **case.kwargs()))
	assert want["pdims"][0] == 0 or 0 == len(want["paths"])
	h = host.HostGraph(fa, vcf, "1", host_scan=True, **case.kwargs())
	assert graph_arrays(h) == want and h.declined_lines == 0
	check(case_text(case))


# ---- the census: every seam by name ------------------------------------------------------------------------------------------------------

def test_census_a():
	seams.census_a(seams.group_a())
	seams.census_a_big(seams.a_big())
	t, piece = seams.no_whole_line_then_one()
	slices = seams.bgzf_slices(t.text, piece, t.slot)
	first = t.text[:slices[0][1]]
	assert b"\n" not in first and len(first) < t.slot and b"\n" in t.text[slices[0][1]:slices[0][1] + slices[1][1]], "a slice without a whole line, then one with"


def test_census_b():
	seams.census_b(seams.group_b())


def test_census_c():
	seams.census_c(seams.group_c())


def test_census_d():
	seams.census_d(seams.group_d())
	for t in seams.d_unsupported():
		d = t.layout_fn(0, b"")
		assert d["n_rows"] == seams.K["kVcfMaxRows"] + 1 or d["words_per_column"] == seams.K["kVcfMaxWordsPerColumn"] + 1


def test_census_e():
	seams.census_e(seams.group_e())


# ---- a text that drifts off its seam fails the census --------------------------------------------------------------------------------------

def swapped(texts, name, change):
	out = [t._replace(text=change(t.text)) if t.name == name else t for t in texts]
	assert [t.text for t in out] != [t.text for t in texts]
	return out


def test_census_a_misses_a_shifted_newline():
	with pytest.raises(AssertionError, match="newline offsets per lead.*\\(5, 8192\\)"):
		seams.census_a(swapped(seams.group_a(), "A_lead_5", lambda s: s[:20000] + s[20001:] + b"\n"))   # one byte less before the second slice's third tile
	big = seams.a_big()
	with pytest.raises(AssertionError, match="kind 2 or 3 at chunk line"):
		at = big.text.index(b"\n", 3000)                                  # two lines after the layout line become one
		seams.census_a_big(big._replace(text=big.text[:at] + big.text[at + 1:]))


def test_census_b_misses_a_pad():
	with pytest.raises(AssertionError, match="info64.*tab"):
		seams.census_b(swapped(seams.group_b(), "B_info", lambda s: s.replace(b"info64.ppppp\t", b"info64.pppp\t")))
	with pytest.raises(AssertionError, match="eighth comma"):
		seams.census_b(swapped(seams.group_b(), "B_alts", lambda s: re.sub(rb"(eighth8_63\.\tA\t[A,]*)AA,A\t", rb"\1A,AA\t", s, count=1)))


def test_census_c_misses_a_condition_that_no_longer_stands_alone():
	with pytest.raises(AssertionError, match="empty"):
		seams.census_c([t._replace(text=t.text.replace(b"0||1", b"0|0|1", 1)) for t in seams.group_c()])
	with pytest.raises(AssertionError, match="every phase"):
		seams.census_c(seams.group_c(pads=range(63)))


def test_census_d_misses_rows_off_the_word_seams():
	plain = seams.fixed_layout([1] * 12, n_rows=320, words_per_column=5)
	with pytest.raises(AssertionError, match="rows at the word seams"):
		seams.census_d([t._replace(layout_fn=plain) if "D_words_5" == t.name else t for t in seams.group_d()])


def test_census_e_misses_a_reason():
	with pytest.raises(AssertionError, match="every declining reason"):
		seams.census_e([t._replace(text=t.text.replace(b"\r\n", b"\n")) for t in seams.group_e()[:1]])
