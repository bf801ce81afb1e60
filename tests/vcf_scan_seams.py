"""Texts that put the VCF scan (csrc/vcf_kernels.hpp, v2m_vcf_scan) on every seam of its passes, and a census that recomputes from a
text alone which seams it reaches (test infrastructure).  What the scan must say of a text is vcf_scan_model's business; this file only
knows where the kernels' steps, tiles and blocks fall:

  line index    4-KiB tiles (kVcfTileBytes) of 16-byte loads, cut from the slice's text rounded down to 16 bytes.  Plain text is cut
                into slices of fresh = slot - carry new bytes behind the carried line; both slice buffers come from hipMalloc and the
                new bytes begin at a multiple of 16 in them (v2m_vcf_scan: `front`), so lead = (-carry) mod 16.  A carried line holds no
                '\\n', so the first '\\n' of a slice lies at lead + carry or later: offset 15 is met with lead 0 only.
  head pass     64-byte steps from the line's first byte (tabs), from the byte after tab 3 (commas), from the name's first byte.
  genotype pass 64-byte steps from the byte after tab 8.
  scans         kVcfScanThreads entries a block, with a carry between blocks.

Every builder is deterministic and returns a Text: the text, the wanted name, the layout function and the slot of the group."""

import collections
import functools
import os
import re

import numpy as np

import vcf_scan_model as model

HERE = os.path.dirname(os.path.abspath(__file__))
VCF_KERNELS_HPP = os.path.join(os.path.dirname(HERE), "vcf2multialign_amd", "csrc", "vcf_kernels.hpp")
STEP = 64                     # a wave's lanes: one byte each a step

Text = collections.namedtuple("Text", "name text wanted layout_fn slot")


def constants(path=VCF_KERNELS_HPP):
	with open(path) as f:
		text = f.read()
	out = {}
	for name in ("kVcfTileBytes", "kVcfThreads", "kVcfScanThreads", "kVcfMaxAlts", "kVcfMaxRows", "kVcfMaxWordsPerColumn"):
		found = re.findall(r"^constexpr\s+u32\s+%s\s*=\s*(\d+)\s*;" % name, text, re.M)
		assert len(found) == 1, "%s: %d definitions of the form `constexpr u32 %s = value;` in vcf_kernels.hpp" % (name, len(found), name)
		out[name] = int(found[0])
	assert out["kVcfTileBytes"] == 16 * out["kVcfThreads"] and re.search(r"p \+= 64\)", text), "the tiles are 16 bytes a thread, the passes step by a wave"
	return out


K = constants()
TILE, BLOCK = K["kVcfTileBytes"], K["kVcfScanThreads"]


# ---- layouts -----------------------------------------------------------------------------------

def fixed_layout(ploidies, row_lookup=None, n_rows=None, words_per_column=None):
	"""A layout function that ignores the line: samples of the given ploidies; row_lookup defaults to the rows in copy order."""
	copy_begin = np.concatenate([[0], np.cumsum(ploidies)]).astype(np.int64).tolist()
	rows = list(range(copy_begin[-1])) if row_lookup is None else list(row_lookup)
	assert len(rows) == copy_begin[-1]
	n = (max(rows) + 1 if rows and max(rows) >= 0 else 0) if n_rows is None else n_rows
	words = (n + 63) // 64 if words_per_column is None else words_per_column
	d = dict(n_samples=len(ploidies), n_rows=n, words_per_column=words, copy_begin=copy_begin, row_lookup=rows)
	return lambda _i, _line: d


def record(chrom=b"1", pos=100, ident=b"v", ref=b"A", alt=b"C", qual=b".", filt=b"PASS", info=b".", fmt=b"GT", samples=()):
	return b"\t".join([chrom, b"%d" % pos, ident, ref, alt, qual, filt, info, fmt] + list(samples))


HEADER = [b"##fileformat=VCFv4.2", b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tS0\tS1"]
TWO_DIPLOID = fixed_layout([2, 2])
GT2 = [b"0|1", b"1/1"]


def joined(lines, final_eol=True):
	return b"\n".join(lines) + (b"\n" if final_eol else b"")


# ---- the plain-text cut and what it means for the line index -----------------------------------------------------------------------

def plain_slices(text, slot):
	"""[(begin, carry, fresh, last)]: the slices of plain text as the header documents them -- the carried line, then as many new bytes
	as the slot still holds.  begin = the text offset of the slice's first byte (the carried line's)."""
	slot = max(16, min(slot if slot else 64 << 20, 256 << 20))
	out, pos, taken = [], 0, 0
	while pos < len(text):
		carry = taken - pos
		fresh = min(len(text) - taken, slot - min(slot, carry))
		taken += fresh
		last = taken == len(text)
		assert fresh or last, "a line longer than a slice"
		out.append((pos, carry, fresh, last))
		nl = text.rfind(b"\n", pos, taken)
		if last:
			break
		assert nl >= 0 or taken - pos < slot, "a line longer than a slice"
		pos = nl + 1 if nl >= 0 else pos
	return out


def line_index_census(text, slot):
	"""Per slice: lead, the tiles, the '\\n' offsets from the aligned base, the whole lines."""
	out = []
	for begin, carry, fresh, last in plain_slices(text, slot):
		lead = -carry % 16
		s = text[begin:begin + carry + fresh]
		newlines = np.flatnonzero(np.frombuffer(s, np.uint8) == 10) + lead
		n_tiles = (lead + len(s) + TILE - 1) // TILE
		per_tile = np.bincount(newlines // TILE, minlength=n_tiles)
		n_lines = len(newlines) + (1 if last and not s.endswith(b"\n") else 0)
		out.append(dict(lead=lead, carry=carry, length=len(s), newlines=newlines, n_tiles=n_tiles, per_tile=per_tile, n_lines=n_lines, last=last))
	return out


NEWLINE_OFFSETS = (15, 16, 17, 4095, 4096, 4097, 8191, 8192)
assert NEWLINE_OFFSETS == (15, 16, 17, TILE - 1, TILE, TILE + 1, 2 * TILE - 1, 2 * TILE)


def filler(n, k):
	"""A line of n bytes of kind 0 or 1, by turns."""
	if 0 == n:
		return b""
	if n < 8 or k % 2:
		return b"#" + b"c" * (n - 1)
	return b"2" + b"\t" * 7 + b"y" * (n - 8)


def lines_with_newlines_at(positions, total):
	"""A text of `total` bytes with '\\n' exactly at `positions` (ascending text offsets), lines of kinds 0 and 1 between them."""
	out, at = [], 0
	for k, p in enumerate(positions):
		out.append(filler(p - at, k) + b"\n")
		at = p + 1
	out.append(filler(total - at, 1))
	text = b"".join(out)
	assert len(text) == total and [i for i in range(total) if text[i] == 10] == list(positions)
	return text


A_SLOT = 3 * TILE


def a_lead_text(lead):
	"""Three slices of a 12-KiB slot: the first with lead 0, the second with the lead asked for (the carried line has 16 - lead bytes and
	its '\\n' is the slice's first new byte, at offset 16), both with '\\n' at every offset of NEWLINE_OFFSETS."""
	carry = 16 - lead
	first = list(NEWLINE_OFFSETS) + [10000, A_SLOT - carry - 1]
	second_begin = A_SLOT - carry                                       # the carried line's first byte; offset o of the slice is here - lead + o
	second = [second_begin - lead + o for o in NEWLINE_OFFSETS if o >= 16] + [second_begin - lead + 11000]
	third = [2 * A_SLOT + 500, 2 * A_SLOT + 900]
	text = lines_with_newlines_at(first + second + third, 2 * A_SLOT + 901)
	return Text("A_lead_%d" % lead, text, "1", TWO_DIPLOID, A_SLOT)


def a_newline_run():
	return Text("A_newline_run", b"#a\n" + b"\n" * (3 * TILE) + b"#b\n2" + b"\t" * 7 + b"\n", "1", TWO_DIPLOID, A_SLOT)


def a_no_final_newline(length):
	lines, left = [], length
	while left > 120:
		lines.append(filler(99, len(lines)))
		left -= 100
	lines.append(filler(left, 0))
	text = joined(lines, final_eol=False)
	assert len(text) == length
	return Text("A_no_final_newline_%d" % length, text, "1", TWO_DIPLOID, A_SLOT)


def a_tiny(text):
	return Text("A_tiny_%s" % text.hex(), text, "1", TWO_DIPLOID, A_SLOT)


BIG_LAYOUT_LINE = 5
BIG_MARKS = (1023, 1024, 1025, 2047, 2048)                          # chunk-relative lines of kinds 2 and 3 at the allocation scan's block edges
BIG_SLOT = (1 << 20) + 3 * TILE + 5


@functools.lru_cache(maxsize=None)
def a_big():
	"""One slice of more than 1024 tiles: about 70 000 short lines of kinds 0 and 1, the layout line at line 5, and lines of kinds 2 and 3
	around the block edges of the chunk from the layout line on (the chunk's first line is of kind 2, so both carries are non-zero)."""
	rng = np.random.default_rng(20)
	n_lines = 70000
	pads = rng.integers(0, 90, n_lines)
	lines = []
	for i in range(n_lines):
		rel = i - BIG_LAYOUT_LINE
		if i < BIG_LAYOUT_LINE:
			line = HEADER[min(i, 1)] if i < 2 else filler(20 + int(pads[i]), i)
		elif 0 == rel or rel in BIG_MARKS or 0 == rel % 997:
			if rel % 2:
				line = record(pos=i, ident=b"k3", alt=b"C,G", samples=[b"0|2", b"3|1"])      # allele 3 of 2: declined
			else:
				line = record(pos=i, ident=b"k2", alt=b"C,G,T"[:1 + 2 * (rel % 3)], samples=[b"0|1", b"1|0"])
		else:
			line = filler(16 + int(pads[i]), i)
		lines.append(line)
	return Text("A_big", joined(lines), "1", TWO_DIPLOID, BIG_SLOT)


@functools.lru_cache(maxsize=None)
def group_a():
	out = [a_lead_text(lead) for lead in range(16)]
	out.append(a_newline_run())
	out += [a_no_final_newline(TILE * k + d) for k in (1, 2) for d in (-1, 0, 1)]
	out += [a_tiny(t) for t in (b"\n", b"x", b"x\n")]
	return out


def census_a(texts):
	"""Asserts the seams of group A (all but the big text's) by name."""
	met, final_lengths, tile_of_newlines, run = set(), set(), False, 0
	for t in texts:
		slices = line_index_census(t.text, t.slot)
		if t.name.startswith("A_lead"):
			assert len(slices) == 3, (t.name, "three slices", len(slices))
		for s in slices:
			met |= {(s["lead"], int(o)) for o in s["newlines"] if o in NEWLINE_OFFSETS}
			tile_of_newlines = tile_of_newlines or bool((s["per_tile"] == TILE).any())
		kinds = {k for k, _, _, _ in model.scan_text(t.text, t.wanted, t.layout_fn)[0]}
		if t.name.startswith("A_lead"):
			assert kinds == {0, 1}, (t.name, "kinds 0 and 1 only", kinds)
		if not t.text.endswith(b"\n"):
			final_lengths.add(len(t.text))
		run = max(run, max(len(m) for m in re.findall(rb"\n+", t.text)) if b"\n" in t.text else 0)
	missing = [(lead, o) for lead in range(16) for o in NEWLINE_OFFSETS if (lead, o) not in met and not (15 == o and lead)]
	assert not missing, ("newline offsets per lead", missing)
	assert run >= TILE and tile_of_newlines, ("a whole tile of newlines", run)
	assert {TILE * k + d for k in (1, 2) for d in (-1, 0, 1)} <= final_lengths, ("final lines without a newline", sorted(final_lengths))
	assert {b"\n", b"x", b"x\n"} <= {t.text for t in texts}, "the tiny texts"


def census_a_big(t):
	whole = line_index_census(t.text, 0)
	assert len(whole) == 1 and whole[0]["n_tiles"] > BLOCK, ("more than %d tiles in one slice" % BLOCK, whole[0]["n_tiles"])
	lines, at = model.scan_text(t.text, t.wanted, t.layout_fn)
	assert at == BIG_LAYOUT_LINE and len(lines) - at > 2 * BLOCK
	kinds = [k for k, _, _, _ in lines]
	assert sum(k in (0, 1) for k in kinds) > 0.9 * len(kinds) and len(kinds) >= 60000
	for rel in BIG_MARKS:
		assert kinds[at + rel] in (2, 3), ("a line of kind 2 or 3 at chunk line", rel, kinds[at + rel])
	assert {kinds[at + rel] for rel in BIG_MARKS} == {2, 3}
	for edge in (BLOCK, 2 * BLOCK):
		before = lines[at:at + edge]
		assert sum(len(h) for _, _, h, _ in before) and sum(n for _, n, _, _ in before), ("both carries non-zero at block edge", edge)
	assert len(line_index_census(t.text, t.slot)) >= 4


# ---- group B: the head pass -----------------------------------------------------------------------------------------------------------

PADS = range(STEP)
B_SLOT = 3000


def b_text(name, make, pads=PADS, wanted="1", layout_fn=TWO_DIPLOID, first=True):
	"""make(pad) -> [(shape tag, keyword arguments of record() | a raw line)]; the ID column of a record is the tag, '.' and `pad` bytes."""
	lines = list(HEADER)
	if first:
		lines.append(record(chrom=wanted.encode(), pos=1, ident=b"first", samples=GT2))
	for pad in pads:
		for tag, what in make(pad):
			if isinstance(what, bytes):
				lines.append(what)
			else:
				kw = dict(chrom=wanted.encode(), pos=1000 + pad, ident=tag.encode() + b"." + b"p" * pad, samples=GT2)
				kw.update(what)
				lines.append(record(**kw))
	return Text(name, joined(lines), wanted, layout_fn, B_SLOT)


INFO_LENGTHS = (0, 1, 63, 64, 65, 500)
FORMATS = (b"GT", b"GT:", b"GT:DP", b"G", b"GTX", b"TG", b"gt", b"", b"DP:GT")
TAB_COUNTS = (0, 6, 7, 8, 9)
NAME_LENGTHS = (1, 4, 64, 65, 130)


def alt_list(n_commas, n_bytes, eighth_at=None):
	"""An ALT column of n_commas commas and about n_bytes bytes; eighth_at: the offset of the eighth comma in the column."""
	entries = [b"A"] * (n_commas + 1)
	if eighth_at is not None:
		assert n_commas >= 8
		entries[7] = b"A" * (eighth_at - 14)                            # seven entries and their commas before it: 14 bytes
	else:
		entries[-1] = b"A" * max(1, n_bytes - 2 * n_commas)
	col = b",".join(entries)
	assert col.count(b",") == n_commas and (eighth_at is None or [i for i, ch in enumerate(col) if ch == 44][7] == eighth_at)
	return col


def b_info():
	return b_text("B_info", lambda pad: [("info%d" % n, dict(info=b"I" * n)) for n in INFO_LENGTHS])


def b_alts():
	def make(pad):
		out = [("alt%d_%d" % (c, n), dict(alt=alt_list(c, n), samples=[b"7|1", b"0/5"])) for c in (7, 8, 9) for n in (20, 100, 170)]
		out += [("eighth%d_%d" % (c, at), dict(alt=alt_list(c, 0, eighth_at=at))) for c in (8, 9) for at in (STEP - 1, STEP)]
		out.append(("emptyalt", dict(alt=b",C", samples=[b"2|1", b"0/2"])))
		return out
	return b_text("B_alts", make)


def b_formats():
	return b_text("B_formats", lambda pad: [("fmt%d" % k, dict(fmt=f, samples=[b"0|1:5", b"1/1:7"])) for k, f in enumerate(FORMATS)])


def b_tabs():
	def make(pad):
		out = []
		for n in TAB_COUNTS:
			for chrom in (b"1", b"2"):
				for cr in (b"", b"\r"):
					fields = record(chrom=chrom, ident=b"tabs%d." % n + b"p" * pad, samples=[b"0|1"]).split(b"\t")[:n + 1]
					out.append(("tabs", b"\t".join(fields) + cr))
		return out
	return b_text("B_tabs", make)


def b_hash_lines():
	def make(pad):
		return [("h", b"#CHRO"), ("h", b"#CHROM"), ("h", b"#CHROMX"), ("h", b""), ("h", b"#" + b"h" * (STEP + pad)), ("h", b"#CHROM\t" + b"n" * (STEP + pad)),
			("rec", dict())]
	return b_text("B_hash_lines", make, pads=range(0, STEP, 7))


def name_of(n):
	return bytes(b"abcdefghijklmnopqrstuvwxyz0123456789"[i % 36] for i in range(n)).decode()


def other_names(wanted):
	"""A proper prefix, an extension, a change of the last byte, and changes of bytes 63 and 64 (the step's last and the next one's first)."""
	w = wanted.encode()
	out = {"prefix": w[:-1], "extension": w + b"0", "last": w[:-1] + bytes([w[-1] ^ 1])}
	for at in (STEP - 1, STEP):
		if len(w) > at:
			out["byte%d" % at] = w[:at] + bytes([w[at] ^ 1]) + w[at + 1:]
	return out


def b_names(n):
	wanted = name_of(n)
	others = other_names(wanted)
	def make(pad):
		return [("same", dict())] + [(tag, dict(chrom=name)) for tag, name in sorted(others.items())]
	return b_text("B_name_%d" % n, make, pads=range(0, STEP, 9), wanted=wanted)


def b_short_layout_line(line):
	"""The layout line has fewer than 7 tabs: kind 3, yet it fixes the layout (a layout function that does not read the line)."""
	lines = list(HEADER) + [record(chrom=b"2", samples=GT2), line, record(samples=GT2), record(samples=[b"0|1"]), record(chrom=b"2", samples=GT2)]
	return Text("B_short_layout_%s" % line.hex(), joined(lines), "1", TWO_DIPLOID, B_SLOT)


@functools.lru_cache(maxsize=None)
def group_b():
	return [b_info(), b_alts(), b_formats(), b_tabs(), b_hash_lines()] + [b_names(n) for n in NAME_LENGTHS] + [b_short_layout_line(l) for l in (b"1\tfoo", b"1", b"1\r")]


def tab_phases(line):
	return [i % STEP for i, ch in enumerate(line) if ch == 9][:9]


def census_b(texts):
	by_name = {t.name: t for t in texts}

	def tagged(t):
		"""{shape tag: [(line, kind, reason)]} of the text's records."""
		lines, _, reasons = model.scan_text(t.text, t.wanted, t.layout_fn, with_reasons=True)
		out = collections.defaultdict(list)
		for line, (kind, _, _, _), why in zip(model.split_lines(t.text), lines, reasons):
			f = line.split(b"\t")
			if len(f) > 2 and b"." in f[2]:
				out[f[2].split(b".")[0].decode()].append((line, kind, why))
		return out

	def every_phase(t, tag, kind, why=None, tabs=9):
		"""The shape occurs with every pad, as the kind asked for, and each of its tabs after the ID column meets every phase of a step."""
		got = tagged(t)[tag]
		assert len(got) == STEP and all((k, r) == (kind, why) for _, k, r in got), (t.name, tag, kind, why, [(k, r) for _, k, r in got][:3], len(got))
		for which in range(2, tabs):
			assert {tab_phases(line)[which] for line, _, _ in got} == set(range(STEP)), (t.name, tag, "tab", which)

	t = by_name["B_info"]
	for n in INFO_LENGTHS:
		every_phase(t, "info%d" % n, 2)
		assert all(len(line.split(b"\t")[7]) == n for line, _, _ in tagged(t)["info%d" % n])
	t = by_name["B_alts"]
	for c in (7, 8, 9):
		for n, steps in ((20, 1), (100, 2), (170, 3)):
			every_phase(t, "alt%d_%d" % (c, n), 2 if 7 == c else 3, None if 7 == c else "c")
			assert all((len(line.split(b"\t")[4]) + STEP - 1) // STEP == steps and line.split(b"\t")[4].count(b",") == c for line, _, _ in tagged(t)["alt%d_%d" % (c, n)])
	for c in (8, 9):
		for at in (STEP - 1, STEP):
			every_phase(t, "eighth%d_%d" % (c, at), 3, "c")
			for line, _, _ in tagged(t)["eighth%d_%d" % (c, at)]:
				alt = line.split(b"\t")[4]
				assert [i for i, ch in enumerate(alt) if ch == 44][7] == at, ("the eighth comma", at)
	every_phase(t, "emptyalt", 2)
	assert all(line.split(b"\t")[4].startswith(b",") for line, _, _ in tagged(t)["emptyalt"])
	t = by_name["B_formats"]
	for k, f in enumerate(FORMATS):
		ok = f in (b"GT", b"GT:", b"GT:DP")
		every_phase(t, "fmt%d" % k, 2 if ok else 3, None if ok else "b")
		assert all(line.split(b"\t")[8] == f for line, _, _ in tagged(t)["fmt%d" % k])
	# 'G' on the last byte of a step, 'T' on the first of the next
	assert any(line.split(b"\t")[8] == b"GT" and (tab_phases(line)[7] + 1) % STEP == STEP - 1 for line, _, _ in tagged(t)["fmt0"]), "G on byte 63"
	t = by_name["B_tabs"]
	seen = collections.Counter()
	lines, _ = model.scan_text(t.text, t.wanted, t.layout_fn)
	for line, (kind, _, _, _) in list(zip(model.split_lines(t.text), lines))[3:]:                 # (after the header and the first record)
		seen[(line.count(b"\t"), line.split(b"\t")[0].rstrip(b"\r"), line.endswith(b"\r"), kind)] += 1
	for n in TAB_COUNTS:
		for chrom in (b"1", b"2"):
			for cr in (False, True):
				kind = 3 if n < 7 else 1 if chrom == b"2" else 3                # 7 to 9 tabs and one sample of two: a, b or d decline it
				assert seen[(n, chrom, cr, kind)] == STEP, ("tabs", n, chrom, cr, kind, seen)
	t = by_name["B_hash_lines"]
	heads = {line: head for line, (_, _, head, _) in zip(model.split_lines(t.text), model.scan_text(t.text, t.wanted, t.layout_fn)[0])}
	assert heads[b"#CHRO"] == b"" and heads[b"#CHROM"] == b"#CHROM" and heads[b"#CHROMX"] == b"#CHROMX" and b"" in heads
	assert any(len(l) > STEP and l.startswith(b"#h") for l in heads) and any(len(l) > STEP and h == l for l, h in heads.items() if l.startswith(b"#CHROM\t"))
	for n in NAME_LENGTHS:
		t = by_name["B_name_%d" % n]
		assert len(t.wanted) == n
		got = tagged(t)
		want = {"same", "prefix", "extension", "last"} | ({"byte63"} if n > 63 else set()) | ({"byte64"} if n > 64 else set())
		assert set(got) - {"first"} == want, (n, sorted(got))
		for tag in want:
			assert {k for _, k, _ in got[tag]} == ({2} if "same" == tag else {1}), (n, tag)
			for line, _, _ in got[tag]:
				name, w = line.split(b"\t")[0], t.wanted.encode()
				differ = [i for i in range(min(len(name), len(w))) if name[i] != w[i]]
				assert {"same": name == w, "prefix": name == w[:-1], "extension": name[:-1] == w, "last": differ == [n - 1] and len(name) == n,
					"byte63": differ == [63] and len(name) == n, "byte64": differ == [64] and len(name) == n}[tag], (n, tag)
	for t in texts:
		if t.name.startswith("B_short_layout"):
			lines, at = model.scan_text(t.text, t.wanted, t.layout_fn)
			assert lines[at][0] == 3 and model.split_lines(t.text)[at].count(b"\t") < 7 and 2 in {k for k, _, _, _ in lines[at + 1:]}, t.name
	assert sum(t.name.startswith("B_short_layout") for t in texts) == 3


# ---- group C: the genotype pass ----------------------------------------------------------------------------------------------------

C_PLOIDIES = [1, 1, 2, 3, 4, 20]                                    # the pad's carrier, then ploidy 1, 2, 3, 4 and 20
C_SLOT = 2500


def c_layout():
	"""Three copies excluded, the others' rows in a shuffled order."""
	n = sum(C_PLOIDIES)
	rng = np.random.default_rng(3)
	excluded = {2, 7, 20}
	rows = rng.permutation(n - len(excluded)).tolist()
	lookup = [-1 if i in excluded else rows.pop() for i in range(n)]
	return fixed_layout(C_PLOIDIES, row_lookup=lookup, n_rows=n - len(excluded))


C_LAYOUT = c_layout()
X3 = b"|".join(b"%03d" % (k % 4) for k in range(20))                # 79 bytes: a GT subfield longer than a step
X3_TAIL = X3 + b":" + b"5" * 70
assert len(X3) == 79
C_BASE = [b"1", b"0|1", b"1/2/3", b".|0|3|1", X3_TAIL]              # the sample fields after the carrier, alleles up to 3 (n_alts = 3)

# tag -> (sample field index after the carrier or None, the field, the model's reason or None when the line stays of kind 2)
C_VALID = {
	"base": (None, None),
	"dots": (3, b".|./.|."),
	"dot1": (0, b"."),
	"zeros": (2, b"01/003/000"),
	"nalts": (1, b"3|03"),
	"past": (1, b"0|1|zz|9999||"),
	"past1": (0, b"1|x/"),
	"colon": (1, b"0|1:0|1/2:9|9/x"),
	"long": (1, b"1|1:" + b"7" * 140),
	"x1": (4, b"|".join(b"%d" % (k % 4) for k in range(20))),
	"x_past": (4, X3 + b"|abc/4444"),
}
C_DECLINED = {
	"value": (1, b"0|4", "e:value"),
	"value3": (4, X3[:-3] + b"004" + b":9", "e:value"),
	"four": (2, b"1/0001/2", "e:long"),
	"empty": (2, b"0||1", "e:empty"),
	"nondigit": (1, b"0|x", "e:nondigit"),
	"dotdigit": (0, b".1", "e:nondigit"),
	"short_tab": (3, b"0|1|2", "e:missing"),
	"short_colon": (3, b"0|1|2:7|7", "e:missing"),
	"empty_column": (1, b"", "e:empty"),
	"empty_last": (4, b"", "e:empty"),
	"x_short": (4, X3[:-4], "e:missing"),
	"x_bad": (4, X3[:60] + b"x" + X3[61:], "e:nondigit"),
	"x_bad_late": (4, X3[:-1] + b"x", "e:nondigit"),
}
C_COLUMNS = {"too_many": (lambda f: f + [b"0"], "d"), "too_many_empty": (lambda f: f + [b""], "d"), "too_few": (lambda f: f[:-1], "d")}


def c_line(tag, pad):
	fields = list(C_BASE)
	if tag in C_COLUMNS:
		fields = C_COLUMNS[tag][0](fields)
	else:
		at, field = (C_VALID.get(tag) or C_DECLINED[tag])[:2]
		if at is not None:
			fields[at] = field
	return record(pos=2000 + pad, ident=tag.encode() + b"." + b"%d" % pad, alt=b"C,G,T", fmt=b"GT:DP", samples=[b"0:" + b"9" * pad] + fields)


def c_tags():
	return list(C_VALID) + list(C_DECLINED) + list(C_COLUMNS)


@functools.lru_cache(maxsize=None)
def group_c(pads=PADS, tags=None):
	tags = c_tags() if tags is None else list(tags)
	lines = list(HEADER[:1]) + [b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\tP\tH\tD\tT\tQ\tX"]
	lines += [c_line(tag, pad) for pad in pads for tag in tags]
	return [Text("C_genotypes", joined(lines), "1", C_LAYOUT, C_SLOT)]


def census_c(texts):
	(t,) = texts
	lines, _, reasons = model.scan_text(t.text, t.wanted, t.layout_fn, with_reasons=True)
	got = collections.defaultdict(dict)
	for line, (kind, _, _, _), why in zip(model.split_lines(t.text), lines, reasons):
		f = line.split(b"\t")
		if len(f) > 9 and not line.startswith(b"#"):
			tag, pad = f[2].split(b".")
			assert len(f[9]) == 2 + int(pad)
			got[tag.decode()][int(pad)] = (f, kind, why)
	carried = False
	for tag in c_tags():
		assert sorted(got[tag]) == list(PADS), (tag, "every phase of a step", sorted(got[tag]))
		want = C_DECLINED[tag][2] if tag in C_DECLINED else C_COLUMNS[tag][1] if tag in C_COLUMNS else None
		for pad, (f, kind, why) in got[tag].items():
			assert (kind, why) == ((2, None) if want is None else (3, want)), (tag, pad, kind, why)
			base = got["base"][pad][0]
			if tag in C_DECLINED:
				# the condition stands alone on the line: with that one sample field as in the base line, the line is of kind 2
				assert len(f) == len(base) and sum(a != b for a, b in zip(f[9:], base[9:])) == 1, (tag, pad)
			elif tag in C_COLUMNS:
				m = min(len(f), len(base))
				assert abs(len(f) - len(base)) == 1 and f[9:m] == base[9:m], (tag, pad)
			# a step that begins inside the 80-byte GT subfield behind two separators or more, and so does the next: the copy is carried twice
			x_at = sum(len(x) + 1 for x in f[9:14])
			gt = f[14].split(b":")[0] if len(f) > 14 else b""
			for q in range(-x_at % STEP, len(gt) - STEP, STEP):
				seps = gt[:q].count(b"|") + gt[:q].count(b"/")
				carried = carried or (seps >= 2 and q + STEP < len(gt) and len(f) == 15 and kind == 2)
	assert carried, "a copy carry above 1 across a whole step"
	assert {r for r in reasons if r} >= {"d", "e:missing", "e:empty", "e:long", "e:nondigit", "e:value"}
	d = t.layout_fn(0, b"")
	assert -1 in d["row_lookup"] and sorted(r for r in d["row_lookup"] if r >= 0) != [r for r in d["row_lookup"] if r >= 0], "excluded copies, rows out of order"
	assert sorted({int(b) - int(a) for a, b in zip(d["copy_begin"], d["copy_begin"][1:])}) == [1, 2, 3, 4, 20]
	assert any(len(x) > 128 for f, _, _ in got["long"].values() for x in f[9:])


# ---- group D: layout widths -------------------------------------------------------------------------------------------------------

D_WIDTHS = (1, 4, 5, 32, 33, 128, 129, 512)
D_SLOT = 400


def d_layout(n_rows, words_per_column, all_excluded=False):
	"""A dozen haploid samples on the rows at the word seams."""
	picks = [0, 31, 32, 63, 64, n_rows - 1, 1, 33, 65, n_rows - 2, n_rows // 2, 62]
	rows, seen = [], set()
	for r in picks:
		ok = 0 <= r < n_rows and r not in seen and not all_excluded
		rows.append(r if ok else -1)
		seen.add(r)
	return fixed_layout([1] * 12, row_lookup=rows, n_rows=n_rows, words_per_column=words_per_column)


def d_text():
	lines = list(HEADER[:1]) + [b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT" + b"".join(b"\tS%d" % s for s in range(12))]
	rng = np.random.default_rng(4)
	for n_alts in (1, 8, 3, 8, 2):
		gts = [b"%d" % a for a in rng.integers(0, n_alts + 1, 12)]
		gts[5] = b"%d" % n_alts                                           # the last row carries the last ALT
		lines.append(record(alt=b",".join([b"C"] * n_alts), samples=gts))
	lines.insert(4, record(alt=b"C", samples=[b"2"] * 12))                # declined
	lines.insert(5, record(chrom=b"2", samples=[b"0"]))
	return joined(lines)


@functools.lru_cache(maxsize=None)
def group_d():
	text = d_text()
	out = [Text("D_words_%d" % w, text, "1", d_layout(64 * w, w), D_SLOT) for w in D_WIDTHS]
	out.append(Text("D_rows_32768", text, "1", d_layout(K["kVcfMaxRows"], K["kVcfMaxWordsPerColumn"]), D_SLOT))
	out += [Text("D_padded_%d_%d" % (n, w), text, "1", d_layout(n, w), D_SLOT) for n, w in ((65, 4), (1, 5), (130, 33), (12, 512))]
	out.append(Text("D_no_rows", text, "1", d_layout(0, 0, all_excluded=True), D_SLOT))
	return out


def d_unsupported():
	text = d_text()
	return [Text("D_rows_32769", text, "1", d_layout(K["kVcfMaxRows"] + 1, K["kVcfMaxWordsPerColumn"] + 1), D_SLOT),
		Text("D_words_513", text, "1", d_layout(64, K["kVcfMaxWordsPerColumn"] + 1), D_SLOT)]


def census_d(texts):
	widths, padded = set(), 0
	for t in texts:
		d = t.layout_fn(0, b"")
		lines, _ = model.scan_text(t.text, t.wanted, t.layout_fn)
		assert d["n_samples"] == 12 and {2, 3} <= {k for k, _, _, _ in lines}
		widths.add(d["words_per_column"])
		want = {r for r in (0, 31, 32, 63, 64, d["n_rows"] - 1) if 0 <= r < d["n_rows"]}
		assert want <= set(d["row_lookup"]), (t.name, "rows at the word seams", want)
		if d["words_per_column"] > (d["n_rows"] + 63) // 64:
			padded += 1
		if d["n_rows"]:
			last = d["n_rows"] - 1
			assert any(n and ((c[:, last >> 6] >> np.uint64(last & 63)) & np.uint64(1)).any() for _, n, _, c in lines), (t.name, "the last row's bit")
		if d["words_per_column"] == K["kVcfMaxWordsPerColumn"]:
			assert any(n == K["kVcfMaxAlts"] for _, n, _, _ in lines), "8 ALTs at 512 words"
	assert set(D_WIDTHS) | {0} <= widths and padded >= 3
	assert any(t.layout_fn(0, b"")["n_rows"] == K["kVcfMaxRows"] for t in texts)
	assert any(t.layout_fn(0, b"")["n_rows"] == 0 and t.layout_fn(0, b"")["words_per_column"] == 0 for t in texts)
	assert (4, 32, 128, 512) == (4, 32, 128, K["kVcfMaxWordsPerColumn"]), "the instances' thresholds (v2m_vcf_scan)"


# ---- group E: a grammar over all of it ----------------------------------------------------------------------------------------------

E_SEEDS = (1, 2, 3, 4)
E_LINES = 2500
E_PLOIDIES = [1, 2, 3, 4, 2, 20]
E_SLOT = 5000


def e_layout():
	n = sum(E_PLOIDIES)
	rows = np.random.default_rng(5).permutation(100)[:n].tolist()
	rows[4] = rows[17] = -1
	return fixed_layout(E_PLOIDIES, row_lookup=rows, n_rows=100, words_per_column=2)


E_LAYOUT = e_layout()
E_REASONS = model.REASONS


def e_text(seed, n_lines=E_LINES):
	rng = np.random.default_rng(1000 + seed)
	pick = lambda seq: seq[int(rng.integers(0, len(seq)))]
	junk = lambda n, alphabet=b"ab|/:.019;=": bytes(alphabet[int(i)] for i in rng.integers(0, len(alphabet), n))

	def token(n_alts):
		a = int(rng.integers(0, n_alts + 1))
		return pick([b".", b"%d" % a, b"%02d" % a, b"%03d" % a, b"%d" % a])

	def sample(ploidy, n_alts, extra=True):
		out = token(n_alts)
		for _ in range(ploidy - 1):
			out += pick([b"|", b"/"]) + token(n_alts)
		if extra and rng.random() < 0.2:
			out += pick([b"|", b"/"]) + junk(int(rng.integers(0, 6)), b"x9|/.")
		if rng.random() < 0.5:
			out += b":" + junk(int(rng.integers(0, pick([4, 30, 150]))))
		return out

	def on_chromosome(why):
		n_alts = int(rng.integers(1, 9))
		fmt = pick([b"GT", b"GT:DP", b"GT:", b"GT:PGT:X"])
		info = junk(int(rng.integers(0, pick([2, 70, 300]))), b"AB=;0123")
		samples = [sample(p, n_alts) for p in E_PLOIDIES]
		cr = b""
		if "a" == why:
			cr = b"\r"
		elif "b" == why:
			fmt = pick([b"G", b"GTX", b"DP:GT", b"", b"gt", b"TG"])
		elif "c" == why:
			n_alts = int(rng.integers(9, 12))
		elif "d" == why:
			samples = pick([samples[:-1], samples + [b"0"], samples + [b""], samples[:1]])
		elif why and why.startswith("e:"):
			s = int(rng.integers(0, len(E_PLOIDIES)))
			p = E_PLOIDIES[s]
			tokens = [token(n_alts) for _ in range(p)]
			c = int(rng.integers(0, p))
			if "e:missing" == why:
				if 1 == p:
					s, p, c = 1, 2, 1
					tokens = [token(n_alts)] * 2
				tokens = tokens[:int(rng.integers(1, p))]
			else:
				tokens[c] = {"e:empty": b"", "e:long": b"%04d" % int(rng.integers(0, n_alts + 1)), "e:nondigit": pick([b"x", b"1x", b".1", b"-1", b"1."]),
					"e:value": b"%d" % (n_alts + int(rng.integers(1, 990 - n_alts)))}[why]
			samples[s] = pick([b"|", b"/"]).join(tokens) + pick([b"", b":", b":1|2"])
		line = record(pos=int(rng.integers(1, 10 ** 6)), ident=junk(int(rng.integers(0, 70)), b"rs0123"), alt=b",".join(pick([b"A", b"<DEL>", b"", b"ACGT" * 20]) for _ in range(n_alts)),
			info=info, fmt=fmt, samples=samples)
		if "tabs<7" == why:
			line = b"\t".join(line.split(b"\t")[:int(rng.integers(1, 8))])
		return line + cr

	lines = list(HEADER[:1]) + [b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT" + b"".join(b"\tS%d" % s for s in range(len(E_PLOIDIES)))]
	while len(lines) < n_lines:
		u = rng.random()
		if u < 0.15:
			lines.append(pick([b"", b"#" + junk(int(rng.integers(0, 200))), b"#CHROM" + junk(int(rng.integers(0, 90)), b"\tab"), b"##" + junk(5)]))
		elif u < 0.35:
			line = on_chromosome(pick([None, "d", "tabs<7", "a", "e:value"]))
			lines.append(pick([b"2", b"11", b"10", b"", b"1 ", b"chr1", b"X"]) + line[1:])
		elif u < 0.65:
			lines.append(on_chromosome(None))
		else:
			lines.append(on_chromosome(pick(E_REASONS)))
	return Text("E_seed_%d" % seed, joined(lines, final_eol=bool(seed % 2)), "1", E_LAYOUT, E_SLOT)


@functools.lru_cache(maxsize=None)
def group_e():
	return [e_text(seed) for seed in E_SEEDS]


def census_e(texts):
	for t in texts:
		lines, _, reasons = model.scan_text(t.text, t.wanted, t.layout_fn, with_reasons=True)
		kinds = collections.Counter(k for k, _, _, _ in lines)
		assert len(lines) >= 2000 and all(kinds[k] >= len(lines) / 10 for k in range(4)), (t.name, "every kind a tenth of the lines", kinds)
		assert set(reasons) - {None} == set(model.REASONS), (t.name, "every declining reason", set(model.REASONS) - set(reasons))
		on = [(k, line) for (k, _, _, _), line in zip(lines, model.split_lines(t.text)) if k in (2, 3) and model.first_column(line) == t.wanted.encode() and line.count(b"\t") >= 7]
		declined = sum(3 == k for k, _ in on)
		assert 4 * declined >= len(on), (t.name, "a quarter of the records on the chromosome declined", declined, len(on))


# ---- BGZF slices (whole members) -------------------------------------------------------------------------------------------------------

def no_whole_line_then_one():
	"""BGZF only: with members of 150 bytes and a slot of 200, the first slice (one member: the second does not fit) holds no '\\n', the
	next one does.  Plain text cannot do this: a plain slice without a whole line is as long as the slot, which is unsupported."""
	lines = [b"#" + b"q" * 179, record(samples=GT2), b"#" + b"r" * 170, record(chrom=b"2", samples=GT2)]
	return Text("A_no_whole_line", joined(lines), "1", TWO_DIPLOID, 200), 150


def bgzf_slices(text, piece, slot):
	"""[(carry, fresh)] of a BGZF input whose members hold `piece` bytes each: whole members while the slice's text stays within the slot,
	one member in any case."""
	sizes = [len(text[i:i + piece]) for i in range(0, len(text), piece)]
	out, carry, k, at = [], 0, 0, 0
	while k < len(sizes):
		fresh, k0 = 0, k
		while k < len(sizes) and (carry + fresh + sizes[k] <= slot or k == k0):
			fresh += sizes[k]
			k += 1
		out.append((carry, fresh))
		s = text[at - carry:at + fresh]
		at += fresh
		nl = s.rfind(b"\n")
		carry = len(s) - (nl + 1) if nl >= 0 else len(s)
	return out
