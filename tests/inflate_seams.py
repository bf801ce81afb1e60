"""The seams of bgzf_inflate_kernel (csrc/bgzf_kernels.hpp), as test infrastructure without a GPU: a plain bit-by-bit RFC 1951 walker that
records every element it reads, a census that lays the kernel's geometry over those records (the 64-word windows of inflate_bits and
where seek re-anchors them, the root tables, the 64-lane loops, the 16-byte copy-out, the 1-KiB CRC lanes), and deterministic builders
of members that land on each of those boundaries.  tests/test_inflate_seams_host.py asserts on the CPU that every seam is reached;
tests/test_gpu_inflate_seams.py runs the members.

The walker knows the rule and the order of the kernel's refusals only; its bits past the payload are whatever `tail` holds, then zeros,
as the kernel's words past the payload are the footer's bytes up to the next multiple of four, then zeros.  The kernel's constants are
read from its source (constants()), so a retuned kernel fails here rather than drifting away from its tests."""

import functools
import os
import re
import struct
import zlib
from collections import Counter, namedtuple

import numpy as np

from bgzf_input_util import (EOF_MEMBER, BitWriter, fixed_lengths, member, write_dynamic_block, write_fixed_block, write_stored_block,
	write_tokens, zlib_inflate)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BGZF_KERNELS_HPP = os.path.join(ROOT, "vcf2multialign_amd", "csrc", "bgzf_kernels.hpp")
V2M_HIP = os.path.join(ROOT, "vcf2multialign_amd", "csrc", "v2m_hip.hip")


def constants(hpp=BGZF_KERNELS_HPP, hip=V2M_HIP):
	with open(hpp) as f:
		text = f.read()
	with open(hip) as f:
		host = f.read()
	out = {}
	roots = re.findall(r"^constexpr\s+u32\s+kInflateLitRoot\s*=\s*(\d+),\s*kInflateDistRoot\s*=\s*(\d+),\s*kInflateClRoot\s*=\s*(\d+)\s*;", text, re.M)
	assert len(roots) == 1, "the three root sizes in one `constexpr u32 kInflateLitRoot = .., kInflateDistRoot = .., kInflateClRoot = ..;`"
	out["lit_root"], out["dist_root"], out["cl_root"] = map(int, roots[0])
	for key, name in (("lanes", "kInflateThreads"), ("slot", "kBgzfSlotBytes"), ("header", "kBgzfHeaderBytes"), ("footer", "kBgzfFooterBytes")):
		found = re.findall(r"^constexpr\s+u32\s+%s\s*=\s*(\d+)\s*;" % name, text, re.M)
		assert len(found) == 1, "%s: %d definitions of the form `constexpr u32 %s = value;`" % (name, len(found), name)
		out[key] = int(found[0])
	win = re.findall(r"if \(next - base >= (\d+)\) \{ cur = ahead; base \+= (\d+); ahead = load\(base \+ (\d+)\); \}", text)
	assert len(win) == 1 and len(set(win[0])) == 1, "the window switch of inflate_bits::refill"
	out["window_words"] = int(win[0][0])
	assert out["window_words"] == out["lanes"], "a window is one word per lane"
	assert re.search(r"next = base = a >> 2;", text) and re.search(r"while \(nb <= 32\)", text), "seek re-anchors the windows at the word of the byte; refill leaves 33 bits"
	crc = re.findall(r"s0\(min\(lane \* (\d+)u, isize\)\), s1\(min\(s0 \+ (\d+)u, isize\)\)", text)
	assert len(crc) == 1 and crc[0][0] == crc[0][1], "the CRC lanes"
	out["crc_lane"] = int(crc[0][0])
	assert re.search(r"unsigned char out\[kBgzfSlotBytes \+ 16\];", text) and re.search(r"ob\(s\.out \+ \(o0 & 15\)\)", text), "the output's phase in LDS"
	assert re.search(r"if \(dist >= 64\) \{", text) and re.search(r"step\(64 % dist\)", text), "the two forms of the match copy"
	assert re.search(r"for \(u32 b\(0\); b < n; b \+= 64\)", text) and re.search(r"for \(u32 k\(lane\); k < rep; k \+= 64\)", text), "the ballot and the repeat loops"
	enum = re.search(r"enum : u32 \{\s*(kInflateOk = 0,.*?kInflateStatusCount)\s*\};", text, re.S)
	assert enum, "the status enum"
	names = [n.strip().replace(" = 0", "") for n in enum.group(1).split(",")]
	assert names[0] == "kInflateOk" and names[-1] == "kInflateStatusCount" and all(n.startswith("kInflate") for n in names)
	out["status"] = [n[len("kInflate"):] for n in names[:-1]]
	texts = re.search(r"text\[v2m::kInflateStatusCount\] = \{(.*?)\};", host, re.S)
	assert texts, "inflate_status_text"
	out["text"] = re.findall(r'"([^"]*)"', texts.group(1))
	assert len(out["text"]) == len(out["status"]) == 17, (len(out["text"]), len(out["status"]))
	return out


K = constants()
LIT_ROOT, DIST_ROOT, CL_ROOT = K["lit_root"], K["dist_root"], K["cl_root"]
LANES, WINDOW_BITS, CRC_LANE, SLOT = K["lanes"], 32 * K["window_words"], K["crc_lane"], K["slot"]
HEADER, FOOTER = K["header"], K["footer"]
STATUS = K["status"]
STATUS_TEXT = dict(zip(STATUS, K["text"]))

CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)

KINDS = ("hdr", "stored_len", "counts", "cl_triple", "cl_sym", "cl_extra", "lit", "len_extra", "dist", "dist_extra")


# ---- the walker ----------------------------------------------------------------------------------

# kind: one of KINDS, or "seek" (after a stored block's bytes: bit = where the next block starts); bit: first payload bit; n: bits;
# length: the code's length (codes only); index, count: which of the `count` codes of that length, in symbol order; sym: the symbol
Rec = namedtuple("Rec", "kind bit n length index count sym")
Walk = namedtuple("Walk", "data status records blocks matches bits")


class _Refused(Exception):
	pass


class Code:
	"""A canonical code (RFC 1951 section 3.2.2) and zlib's verdict on it: over-subscribed and incomplete codes are refused, except a
	single code of length 1 and (not for the code-length code) no code at all."""

	def __init__(self, lens, is_cl=False):
		self.count, self.first, self.offs, self.sorted = [0] * 16, [0] * 16, [0] * 16, []
		for L in lens:
			if L:
				self.count[L] += 1
		code, left, self.max = 0, 1, 0
		for L in range(1, 16):
			self.first[L], self.offs[L] = code, len(self.sorted)
			self.sorted += [s for s, l in enumerate(lens) if l == L]
			left = 2 * left - self.count[L]
			if self.count[L]:
				self.max = L
			code = (code + self.count[L]) << 1
		self.ok = (not is_cl) if 0 == self.max else (0 == left or (left > 0 and not is_cl and 1 == self.max))

	def decode(self, bits, pos):
		"""(symbol, length, index among the codes of that length) of the code that starts at bits[pos], or None."""
		code = 0
		for L in range(1, self.max + 1):
			code = (code << 1) | bits[pos + L - 1]
			i = code - self.first[L]
			if 0 <= i < self.count[L]:
				return self.sorted[self.offs[L] + i], L, i
		return None


FIXED_LIT, FIXED_DIST = fixed_lengths()


def walk(payload, isize=None, crc=None, tail=b""):
	"""Inflates one raw deflate payload bit by bit.  Walk.data: the bytes (None when refused); status: "Ok" or the first refusal, in the
	order in which the kernel checks; records: a Rec per element read; blocks: a dict per block; matches: (p, length, distance).
	isize / crc: the member's footer (None: unbounded output / no CRC check); tail: the bytes that follow the payload where the reader
	can see them."""
	plen = len(payload)
	pbits = 8 * plen
	bits = np.unpackbits(np.frombuffer(bytes(payload) + bytes(tail) + bytes(640), np.uint8), bitorder="little").tolist()
	out, recs, blocks, matches = bytearray(), [], [], []
	limit = SLOT if isize is None else isize
	pos = 0

	def get(n):
		nonlocal pos
		v = 0
		for i in range(n):
			v |= bits[pos + i] << i
		pos += n
		return v

	def refuse(status):
		raise _Refused(status)

	status = "Ok"
	try:
		if (isize is not None and isize > SLOT) or plen + HEADER + FOOTER > SLOT:
			refuse("BadFraming")
		last = False
		while not last:
			recs.append(Rec("hdr", pos, 3, 0, 0, 0, 0))
			hdr = get(3)
			last, btype = bool(hdr & 1), hdr >> 1
			blk = {"type": btype, "final": last, "bit": pos - 3}
			blocks.append(blk)
			if 3 == btype:
				refuse("BadBlockType")
			if 0 == btype:
				pos = (pos + 7) & ~7
				recs.append(Rec("stored_len", pos, 32, 0, 0, 0, 0))
				n, nn = get(16), get(16)
				if pos > pbits:
					refuse("PastPayload")
				if n != (~nn & 0xffff):
					refuse("StoredLengths")
				at = pos // 8
				if n > plen - at:
					refuse("PastPayload")
				if n > limit - len(out):
					refuse("OutputTooLong")
				out += payload[at:at + n]
				pos += 8 * n
				blk.update(pos=at, len=n)
				recs.append(Rec("seek", pos, 0, 0, 0, 0, 0))
				continue
			if 1 == btype:
				lit, dist = Code(FIXED_LIT), Code(FIXED_DIST)
				blk.update(lit_lens=FIXED_LIT, dist_lens=FIXED_DIST)
			else:
				recs.append(Rec("counts", pos, 14, 0, 0, 0, 0))
				hlit, hdist, hclen = get(5) + 257, get(5) + 1, get(4) + 4
				blk.update(hlit=hlit, hdist=hdist, hclen=hclen)
				if hlit > 286 or hdist > 30:
					refuse("TooManySymbols")
				cl_lens = [0] * 19
				for i in range(hclen):
					recs.append(Rec("cl_triple", pos, 3, 0, 0, 0, 0))
					cl_lens[CL_ORDER[i]] = get(3)
				cl = Code(cl_lens, is_cl=True)
				blk.update(cl_lens=cl_lens, cl=cl)
				if not cl.ok:
					refuse("BadCodeLengthCode")
				lens, seq, total = [], [], hlit + hdist
				blk.update(seq=seq)
				while len(lens) < total:
					d = cl.decode(bits, pos)
					if d is None:
						refuse("BadCodeLengthCode")
					sym, L, i = d
					recs.append(Rec("cl_sym", pos, L, L, i, cl.count[L], sym))
					pos += L
					if sym < 16:
						seq.append((sym, None, len(lens), sym))
						lens.append(sym)
						continue
					val = 0
					if 16 == sym:
						if not lens:
							refuse("BadRepeat")
						val, eb, base = lens[-1], 2, 3
					else:
						eb, base = (3, 3) if 17 == sym else (7, 11)
					recs.append(Rec("cl_extra", pos, eb, 0, 0, 0, sym))
					rep = base + get(eb)
					if rep > total - len(lens):
						refuse("BadRepeat")
					seq.append((sym, rep, len(lens), val))
					lens += [val] * rep
				if pos > pbits:
					refuse("PastPayload")
				if 0 == lens[256]:
					refuse("NoEndOfBlock")
				lit, dist = Code(lens[:hlit]), Code(lens[hlit:])
				blk.update(lit_lens=lens[:hlit], dist_lens=lens[hlit:])
				if not lit.ok:
					refuse("BadLitLenCode")
				if not dist.ok:
					refuse("BadDistCode")
			blk.update(lit=lit, dist=dist)
			lit_count, dist_count = lit.count, dist.count
			while True:
				d = lit.decode(bits, pos)
				if d is None or d[0] >= 286:
					refuse("BadLitLenSymbol")
				sym, L, i = d
				recs.append(Rec("lit", pos, L, L, i, lit_count[L], sym))
				pos += L
				if sym < 256:
					if len(out) >= limit:
						refuse("OutputTooLong")
					out.append(sym)
				elif 256 == sym:
					break
				else:
					li = sym - 257
					if LEN_EXTRA[li]:
						recs.append(Rec("len_extra", pos, LEN_EXTRA[li], 0, 0, 0, sym))
					mlen = LEN_BASE[li] + get(LEN_EXTRA[li])
					d = dist.decode(bits, pos)
					if d is None or d[0] >= 30:
						refuse("BadDistSymbol")
					dsym, L, i = d
					recs.append(Rec("dist", pos, L, L, i, dist_count[L], dsym))
					pos += L
					if DIST_EXTRA[dsym]:
						recs.append(Rec("dist_extra", pos, DIST_EXTRA[dsym], 0, 0, 0, dsym))
					distance = DIST_BASE[dsym] + get(DIST_EXTRA[dsym])
					if pos > pbits:
						refuse("PastPayload")
					p = len(out)
					if distance > p:
						refuse("TooFarBack")
					if mlen > limit - p:
						refuse("OutputTooLong")
					matches.append((p, mlen, distance))
					if distance >= mlen:
						out += out[p - distance:p - distance + mlen]
					else:
						for k in range(mlen):
							out.append(out[p - distance + k])
				if pos > pbits:
					refuse("PastPayload")
			if pos > pbits:
				refuse("PastPayload")
		if isize is not None and len(out) != isize:
			refuse("ShortOutput")
		if crc is not None and zlib.crc32(bytes(out)) != crc:
			refuse("BadCrc")
	except _Refused as e:
		status = e.args[0]
	return Walk(bytes(out) if "Ok" == status else None, status, recs, blocks, matches, pos)


@functools.lru_cache(maxsize=None)
def _walk_cached(payload, isize, crc, tail):
	return walk(payload, isize, crc, tail)


def visible_tail(m, lead):
	"""The footer bytes that share the payload's last word: what the kernel's reader sees past the payload before its zeros."""
	plen = len(m) - HEADER - FOOTER
	return m[len(m) - FOOTER:len(m) - FOOTER + (-(lead + plen)) % 4]


def walk_member(m, lead=0):
	crc, isize = struct.unpack_from("<II", m, len(m) - FOOTER)
	return _walk_cached(m[HEADER:len(m) - FOOTER], isize, crc, visible_tail(m, lead))


def member_isize(m):
	return struct.unpack_from("<I", m, len(m) - 4)[0]


# ---- the census ----------------------------------------------------------------------------------

SMALL_ISIZES = tuple(range(1, 18)) + (31, 32, 33)
CRC_ISIZES = (CRC_LANE - 1, CRC_LANE, CRC_LANE + 1, 2 * CRC_LANE - 1, 2 * CRC_LANE, 2 * CRC_LANE + 1, SLOT - CRC_LANE - 1, SLOT - CRC_LANE, SLOT - CRC_LANE + 1,
	SLOT - 1, SLOT)
TYPE_NAME = {0: "stored", 1: "fixed", 2: "dynamic"}
ROOT_OF = {"lit": LIT_ROOT, "dist": DIST_ROOT, "cl_sym": CL_ROOT}


def census(m, offset, out_offset):
	"""The seams member `m` reaches when it lies at byte `offset` of its slice and its output at `out_offset`: (Counter by seam name,
	set of (distance, length) of its matches).  Words count from the payload's address rounded down to 4; a window is WINDOW_BITS from
	the words' base; the base moves to the word of the next block's first byte after every stored block."""
	lead = (offset + HEADER) % 4
	plen = len(m) - HEADER - FOOTER
	n_words = (lead + plen + 3) // 4
	w = walk_member(m, lead)
	c = Counter()
	base_bits, seeks, reach = 0, 0, 0
	recs = w.records
	for k, r in enumerate(recs):
		if "seek" == r.kind:
			a = lead + r.bit // 8
			base_bits, seeks = 32 * (a >> 2), seeks + 1
			left = n_words - (a >> 2)
			blk = [b for b in w.blocks if 0 == b["type"] and "pos" in b and 8 * (b["pos"] + b["len"]) == r.bit][-1]
			if r.bit // 8 == plen:
				c["seek_phase%d_at_end" % (a & 3)] += 1
				if blk["final"]:
					c["seek_at_end_final_stored" if blk["len"] else "seek_at_end_empty_final_stored"] += 1
			elif left < WINDOW_BITS // 32:
				c["seek_phase%d_lt64_words" % (a & 3)] += 1
			elif left < 2 * WINDOW_BITS // 32:
				c["seek_phase%d_lt128_words" % (a & 3)] += 1
			else:
				c["seek_phase%d_ge128_words" % (a & 3)] += 1
			continue
		r0 = 8 * lead + r.bit - base_bits
		r1 = r0 + r.n
		if (r1 - 1) // WINDOW_BITS > r0 // WINDOW_BITS:
			c["straddle_" + r.kind] += 1
		if r1 >= WINDOW_BITS and 0 == r1 % WINDOW_BITS:
			c["end_on_" + r.kind] += 1
		if 0 == seeks:
			reach = r1
		if r.kind in ROOT_OF:
			name = "cl" if "cl_sym" == r.kind else r.kind
			for which, hit in (("first", 0 == r.index), ("last", r.index == r.count - 1)):
				if hit:
					c["%s_L%d_%s" % (name, r.length, which)] += 1
					if r.count > 1:
						c["%s_L%d_%s_of_many" % (name, r.length, which)] += 1
		if "lit" == r.kind and 15 == r.length and r.sym >= 257 and 5 == LEN_EXTRA[r.sym - 257] and k + 3 < len(recs):
			e, d, x = recs[k + 1], recs[k + 2], recs[k + 3]
			if ("len_extra", 5) == (e.kind, e.n) and ("dist", 15) == (d.kind, d.length) and ("dist_extra", 13) == (x.kind, x.n):
				c["chain_phase%d" % ((8 * lead + r.bit) % 32)] += 1
	if 0 == seeks and reach > 3 * WINDOW_BITS + 64:   # (the reader fetches up to 64 bits ahead of what is used)
		c["three_switches_no_seek"] += 1
	if w.blocks:
		c["lead%d_first_%s" % (lead, TYPE_NAME[w.blocks[0]["type"]])] += 1
	if len(m) == SLOT:
		c["member_65536"] += 1
		if 1 == len(w.blocks) and 0 == w.blocks[0]["type"] and w.blocks[0].get("len") == SLOT - HEADER - FOOTER - 5:
			c["member_65536_one_stored_block"] += 1
	for k, b in enumerate(w.blocks):
		if 2 == b["type"]:
			for name, root in (("lit", LIT_ROOT), ("dist", DIST_ROOT), ("cl", CL_ROOT)):
				code = b.get(name)
				if code is None:
					continue
				top = 7 if "cl" == name else 15
				if all(code.count[L] for L in range(1, top + 1)):
					c["%s_lengths_1_to_%d" % (name, top)] += 1
				if code.max == root:
					c["%s_max_eq_root" % name] += 1
			if "lit" in b:
				if max(b["lit"].count) > LANES:
					c["more_than_64_of_one_length"] += 1
				if max(b["lit"].count) > 2 * LANES:
					c["more_than_128_of_one_length"] += 1
			for field, values in (("hlit", (257, 286)), ("hdist", (1, 30)), ("hclen", (4, 19))):
				if b.get(field) in values:
					c["%s_%d" % (field, b[field])] += 1
			total, seq = b.get("hlit", 0) + b.get("hdist", 0), b.get("seq", [])
			for j, (sym, rep, n, val) in enumerate(seq):
				if rep is None:
					continue
				if 16 == sym and n < b["hlit"] < n + rep:
					c["repeat_16_across_the_border"] += 1
				if 16 == sym and 0 == val and j and seq[j - 1][0] in (17, 18):
					c["repeat_16_of_a_zero_left_by_17_18"] += 1
				if (18, 138) == (sym, rep):
					c["repeat_18_with_138"] += 1
				if (17, 10) == (sym, rep):
					c["repeat_17_with_10"] += 1
				if n + rep == total:
					c["repeat_ends_at_hlit_plus_hdist"] += 1
				if rep > LANES:
					c["repeat_of_more_than_64"] += 1
		types = tuple(x["type"] for x in w.blocks[k:k + 3])
		if (1, 2, 1) == types:
			c["blocks_fixed_dynamic_fixed"] += 1
		if (1, 0, 1) == types:
			c["blocks_fixed_stored_fixed"] += 1
		if (2, 2) == types[:2] and "lit" in w.blocks[k + 1]:
			first, second = b, w.blocks[k + 1]
			if first["lit"].max > LIT_ROOT and first["dist"].max > DIST_ROOT and second["lit"].max <= 2 and second["dist"].max <= 1:
				c["blocks_dynamic_long_then_short"] += 1
	pairs = set()
	for p, mlen, dist in w.matches:
		pairs.add((dist, mlen))
		if dist < LANES and mlen > LANES and LANES % dist:
			c["copy_rounds_with_a_wrapping_step"] += 1
	if "Ok" == w.status:
		isize, phase = len(w.data), out_offset % 16
		if isize in SMALL_ISIZES:
			c["isize_%d_phase_%d" % (isize, phase)] += 1
		if isize == SLOT and 15 == phase:
			c["isize_65536_phase_15"] += 1
		if isize in CRC_ISIZES:
			c["crc_isize_%d" % isize] += 1
	return c, pairs


def slices(sizes, isizes, slot_env=None):
	"""The greedy cut of v2m_bgzf_decompress: the first member of every slice, then the member count."""
	n, total = sum(sizes), sum(isizes)
	target = (64 << 20) if slot_env is None else slot_env
	slot = max(SLOT, min(target, (max(n, total) + 0xffff) & ~0xffff))
	cut, cin, cout = [0], 0, 0
	for k, (size, isize) in enumerate(zip(sizes, isizes)):
		if k > cut[-1] and (cin + size > slot or cout + isize > slot):
			cut.append(k)
			cin = cout = 0
		cin += size
		cout += isize
	return cut + [len(sizes)]


def file_census(members, slot_env=None):
	"""The census of a file of `members` (bytes each; the EOF member is added) under a ring slot setting: (Counter, pairs, slice count,
	[(lead, output phase) per member])."""
	ms = list(members) + [EOF_MEMBER]
	sizes, isizes = [len(m) for m in ms], [member_isize(m) for m in ms]
	cut = slices(sizes, isizes, slot_env)
	total, pairs, where = Counter(), set(), []
	for s in range(len(cut) - 1):
		off = out = 0
		for k in range(cut[s], cut[s + 1]):
			c, p = census(ms[k], off, out)
			total += c
			pairs |= p
			where.append(((off + HEADER) % 4, out % 16))
			off += sizes[k]
			out += isizes[k]
	for k in range(1, len(ms) - 2):   # (the EOF member is not a member of the group)
		if 0 == isizes[k] and isizes[k - 1] and isizes[k + 1]:
			total["isize_0_between_two_members"] += 1
	return total, pairs, len(cut) - 1, where


# ---- what the builders share ---------------------------------------------------------------------

PERM = [(167 * i + 13) & 255 for i in range(256)]   # a fixed permutation of 0..255: any 256 consecutive bytes of its walk are distinct


def perm_bytes(start, n):
	return bytes(PERM[(start + i) & 255] for i in range(n))


def mk(payload, trailing=b""):
	"""The member of an accepted payload (zlib's bytes make the footer; the host test holds the walker against them)."""
	data = zlib_inflate(payload + trailing)
	assert data is not None, "zlib refuses a payload that was built to be accepted"
	return member(payload + trailing, data)


def spacer(j, t, salt=0):
	"""A member of one final stored block of j bytes with t bytes after it: moves the next member's lead and output phase independently."""
	w = BitWriter()
	write_stored_block(w, bytes((0xC1 + 29 * salt + 3 * i) & 255 for i in range(j)))
	return mk(w.bytes(), bytes((0xA5 + i) & 255 for i in range(t)))


class Group:
	"""Members in file order, with the lead and the output phase the next one gets in a file that is one slice."""

	def __init__(self):
		self.members, self.off, self.out = [], 0, 0

	@property
	def lead(self):
		return (self.off + HEADER) % 4

	@property
	def phase(self):
		return self.out % 16

	def add(self, name, m):
		self.members.append((name, m))
		self.off += len(m)
		self.out += member_isize(m)

	def align(self, lead=None, phase=None):
		j = 0 if phase is None else (phase - self.phase) % 16
		t = 0 if lead is None else (lead - (self.off + HEADER + 5 + FOOTER + j + HEADER)) % 4
		if j or t or (lead is not None and lead != self.lead):
			self.add("spacer %d+%d before member %d" % (j, t, len(self.members) + 1), spacer(j, t, salt=len(self.members)))
		assert (lead is None or self.lead == lead) and (phase is None or self.phase == phase)


def pad_to(w, target, salt=0):
	"""A non-final fixed block of literals, after which the writer holds exactly `target` bits."""
	n = target - len(w.bits)
	assert n >= 10 + 63, "room for a padding block (%d bits)" % n
	b = (n - 10) % 8   # 3 + 8 a + 9 b + 7 = n
	a = (n - 10 - 9 * b) // 8
	write_fixed_block(w, [(7 * i + 11 * salt) % 144 for i in range(a)] + [144 + (5 * i) % 112 for i in range(b)] + [256], final=False)
	assert len(w.bits) == target


def lens_of(n, pairs):
	out = [0] * n
	for s, L in pairs.items():
		out[s] = L
	return out


A, B = ord("a"), ord("b")
GOOD_LIT = {256: 2, A: 2, B: 2, 257: 2}


def all_lengths_codes():
	"""A literal/length and a distance code with every length 1..15 in use: one symbol each of lengths 1..14, two of 15."""
	lit = lens_of(286, {**{65 + i: i + 1 for i in range(13)}, 256: 14, 284: 15, 285: 15})
	dist = lens_of(30, {**{i: i + 1 for i in range(14)}, 28: 15, 29: 15})
	return lit, dist


# ---- the bit reader -------------------------------------------------------------------------------

REPEAT_SEQ = [(18, 97 - 11), (3, 0), (16, 5 - 3), (18, 138 - 11), (17, 10 - 3), (17, 5 - 3), (3, 0), (3, 0), (1, 0)]
REPEAT_LIT = {**{s: 3 for s in range(97, 103)}, 256: 3, 257: 3}


def _emit_for(kind):
	"""(a writer function of one final block that holds an element of `kind`, which of its records of that kind to place)."""
	def fixed(tokens):
		return lambda w: write_fixed_block(w, tokens)
	if "hdr" == kind:
		return fixed([A, B, 256]), 0
	if "stored_len" == kind:
		return (lambda w: write_stored_block(w, b"stored bytes")), 0
	if "counts" == kind:
		return (lambda w: write_dynamic_block(w, lens_of(258, GOOD_LIT), [1], [A, ("match", 3, 1), B, 256])), 0
	if "cl_triple" == kind:
		return (lambda w: write_dynamic_block(w, lens_of(258, GOOD_LIT), [1], [A, ("match", 3, 1), B, 256])), 5
	if "cl_sym" == kind:
		return (lambda w: write_dynamic_block(w, lens_of(258, GOOD_LIT), [1], [A, ("match", 3, 1), B, 256])), 100
	if "cl_extra" == kind:
		return (lambda w: write_dynamic_block(w, lens_of(258, REPEAT_LIT), [1], [A, ("match", 3, 1), 256], cl_seq=REPEAT_SEQ)), 0
	if "lit" == kind:
		return fixed([A, B, A, B, 200, 256]), 2
	if "len_extra" == kind:
		return fixed([A, B, ("match", 100, 2), 256]), 0
	if "dist" == kind:
		return fixed([A, B, ("match", 100, 2), 256]), 0
	assert "dist_extra" == kind
	return fixed(list(perm_bytes(0, 40)) + [("match", 10, 37), 256]), 0


def placed(lead, kind, mode, k=1):
	"""A payload whose element of `kind` straddles ("straddle") or ends on ("end_on") the k-th window switch of a member at `lead`."""
	emit, which = _emit_for(kind)
	w0 = BitWriter()
	emit(w0)
	r = [r for r in walk(w0.bytes()).records if r.kind == kind][which]
	switch = k * WINDOW_BITS - 8 * lead
	start = switch - r.n if "end_on" == mode else switch - max(1, r.n // 2)
	w = BitWriter()
	pad_to(w, start - r.bit, salt=2 * KINDS.index(kind) + ("end_on" == mode))
	emit(w)
	return w.bytes()


def first_block(kind, salt):
	w = BitWriter()
	data = perm_bytes(31 * salt, 20 + salt)
	if "stored" == kind:
		write_stored_block(w, data)
	else:
		write_fixed_block(w, list(data) + [("match", 9, 7), 256])
	return w.bytes()


def first_dynamic(salt):
	"""A dynamic first block: 128 literals of 8 bits, the end-of-block code and one length of 2 bits."""
	lit = lens_of(258, {**{s: 8 for s in range(128)}, 256: 2, 257: 2})   # 128 / 256 + 1/4 + 1/4
	data = bytes(b & 127 for b in perm_bytes(31 * salt, 20 + salt))
	w = BitWriter()
	write_dynamic_block(w, lit, [1], list(data) + [("match", 3, 1), 256])
	return w.bytes()


def largest_fixed():
	"""65 536 bytes of member: 58 000 nine-bit and 258 eight-bit fixed literals (a 65 510-byte payload)."""
	w = BitWriter()
	write_fixed_block(w, [144 + (i * 37) % 112 for i in range(58000)] + [(i * 11) % 144 for i in range(258)] + [256])
	return w.bytes()


def largest_stored():
	w = BitWriter()
	data = (perm_bytes(5, 256) * 256)[:SLOT - HEADER - FOOTER - 5]
	write_stored_block(w, data)
	return w.bytes()


def chain(lead):
	"""The longest token at every bit phase of its first bit: a 15-bit length code, 5 extra bits, a 15-bit distance code, 13 extra bits;
	and every code of the two all-lengths codes decoded once.  A stored block of 32 768 bytes first, for the distances to reach."""
	lit, dist = all_lengths_codes()
	w = BitWriter()
	write_stored_block(w, (perm_bytes(0, 256) * 128), final=False)
	write_dynamic_block(w, lit, dist, [], final=False)
	toks = [65 + i for i in range(13)] + [("match", 258, DIST_BASE[d]) for d in range(14)] + [("match", 258, DIST_BASE[28] + 4097)]
	write_tokens(w, toks, lit, dist)
	for ph in range(32):
		while (8 * lead + len(w.bits)) % 32 != ph:
			write_tokens(w, [65], lit, dist)   # a one-bit literal
		write_tokens(w, [("match", 227 + (7 * ph) % 31, DIST_BASE[29] + (0 if 0 == ph else 8191 if 31 == ph else (263 * ph) % 8192))], lit, dist)
	write_tokens(w, [256], lit, dist)
	write_fixed_block(w, [A, 256])
	return w.bytes()


def seek_case(lead, phase, form):
	"""A stored block whose end (where seek re-anchors the windows) lies on byte phase `phase` of the kernel's words, with fewer than 64
	words after it ("lt64"), 64 to 127 ("lt128"), none as the final block ("end") or none as an empty final block ("empty_end")."""
	salt = 4 * ("lt64", "lt128", "end", "empty_end").index(form) + phase
	w = BitWriter()
	q = (phase - lead - 6) % 4 + 1           # q eight-bit literals put LEN at byte q + 2 and the stored bytes at byte q + 6
	write_fixed_block(w, [b % 144 for b in perm_bytes(9 * salt, q)] + [256], final=False)
	if "empty_end" == form:
		write_stored_block(w, b"")
		return w.bytes()
	data = perm_bytes(17 * salt, 8)           # (8 bytes keep the phase)
	if "end" == form:
		write_stored_block(w, data)
		return w.bytes()
	write_stored_block(w, data, final=False)
	write_fixed_block(w, [b % 144 for b in perm_bytes(5 * salt, 100 if "lt64" == form else 300)] + [256])
	return w.bytes()


@functools.lru_cache(maxsize=None)
def bits_group():
	g = Group()
	for kind in KINDS:
		for mode in ("straddle", "end_on"):
			g.add("%s %s" % (kind, mode), mk(placed(g.lead, kind, mode)))
	salt = 0
	for kind in ("stored", "fixed", "dynamic"):
		for lead in range(4):
			g.align(lead=lead)
			salt += 1
			g.add("first block %s, lead %d" % (kind, lead), mk(first_dynamic(salt) if "dynamic" == kind else first_block(kind, salt)))
	w = BitWriter()
	write_fixed_block(w, [b % 144 for b in perm_bytes(3, 1000)] + [256])
	g.add("three window switches", mk(w.bytes()))
	g.add("largest member", mk(largest_fixed()))
	g.add("largest member, one stored block", mk(largest_stored()))
	for phase in range(4):
		for form in ("lt64", "lt128", "end", "empty_end"):
			g.add("seek phase %d %s" % (phase, form), mk(seek_case(g.lead, phase, form)))
	g.add("chain at every phase", mk(chain(g.lead)))
	return tuple(g.members)


BITS_SEAMS = (["%s_%s" % (mode, kind) for kind in KINDS for mode in ("straddle", "end_on")]
	+ ["lead%d_first_%s" % (lead, kind) for lead in range(4) for kind in ("stored", "fixed", "dynamic")]
	+ ["three_switches_no_seek", "member_65536", "member_65536_one_stored_block", "seek_at_end_final_stored", "seek_at_end_empty_final_stored"]
	+ ["chain_phase%d" % ph for ph in range(32)]
	+ ["seek_phase%d_%s" % (ph, form) for ph in range(4) for form in ("lt64_words", "lt128_words", "at_end")])


# ---- the tables ----------------------------------------------------------------------------------

def dyn(lit_pairs, dist_pairs, tokens, n_lit=258, n_dist=1, **kw):
	w = BitWriter()
	write_dynamic_block(w, lens_of(n_lit, lit_pairs), lens_of(n_dist, dist_pairs), tokens, **kw)
	return w.bytes()


def cl_1_to_7():
	"""A code-length code with lengths 1..7 in use (1..6 and two of 7), every one of its eight symbols decoded."""
	cl = lens_of(19, {0: 1, 18: 2, 17: 3, 16: 4, 1: 5, 2: 6, 3: 7, 4: 7})
	lit = {65: 1, 66: 2, 67: 3, 68: 4, 256: 4}
	seq = [(18, 65 - 11), (1, 0), (2, 0), (3, 0), (4, 0), (18, 138 - 11), (17, 10 - 3), (0, 0), (18, 38 - 11), (4, 0), (2, 0), (16, 0)]
	return dyn(lit, {0: 2, 1: 2, 2: 2, 3: 2}, [65, 66, 67, 68, 65, 256], n_lit=257, n_dist=4, cl_lens=cl, cl_seq=seq)


def lit_root_walk():
	"""Literal/length codes around the root: 100 of 10 bits (the root) and 56 of 11 (the first length that walks), first and last of each."""
	lit = {0: 1, 1: 2, 2: 3, **{3 + i: 10 for i in range(100)}, **{103 + i: 11 for i in range(55)}, 256: 11}
	return dyn(lit, {0: 1}, [0, 1, 2, 3, 102, 103, 157, 50, 130, 256], n_lit=257)


def lit_130_of_8():
	lit = {**{i: 8 for i in range(130)}, 200: 2, 201: 3, 202: 4, 203: 5, 204: 6, 256: 7}
	return dyn(lit, {0: 1}, [0, 129, 64, 65, 200, 201, 202, 203, 204, 256], n_lit=257)


def dist_root_walk():
	"""Distance codes around the root: 8 of 8 bits and 16 of 9, first and last of each."""
	dist = {0: 1, 1: 2, 2: 3, 3: 4, **{4 + i: 8 for i in range(8)}, **{12 + i: 9 for i in range(16)}}
	lit = {**{s: 9 for s in range(256)}, 256: 2, 257: 2}
	toks = list(perm_bytes(9, 40)) + [("match", 3, DIST_BASE[d]) for d in (4, 11, 12, 27, 0, 3, 7, 20)]
	w = BitWriter()
	write_stored_block(w, perm_bytes(0, 256) * 49, final=False)   # room for distance symbol 27
	write_dynamic_block(w, lens_of(258, lit), lens_of(28, dist), toks + [256])
	return w.bytes()


def max_equals_root():
	lit = {**{65 + i: i + 1 for i in range(LIT_ROOT - 1)}, 256: LIT_ROOT, 257: LIT_ROOT}
	dist = {**{i: i + 1 for i in range(DIST_ROOT - 1)}, 8: DIST_ROOT, 9: DIST_ROOT}
	toks = [65] * 40 + [65 + i for i in range(LIT_ROOT - 1)] + [("match", 3, DIST_BASE[d]) for d in (0, 6, 8, 9)]
	return dyn(lit, dist, toks + [256], n_lit=258, n_dist=10)


def header_counts():
	"""HLIT 286 with HDIST 30 (HCLEN 19), and HLIT 257 with HDIST 1."""
	lit = {**{s: 9 for s in range(256)}, 256: 2, 285: 2}
	dist = {**{i: 5 for i in range(28)}, 28: 4, 29: 4}                      # 28 / 32 + 2 / 16
	big = dyn(lit, dist, list(perm_bytes(1, 40)) + [("match", 258, 3), ("match", 258, 40), 256], n_lit=286, n_dist=30)
	small = dyn({65: 1, 256: 1}, {}, [65, 65, 256], n_lit=257, n_dist=1)
	return big, small


def repeats():
	"""18 with 138, 16 repeating the zero that 18 left, 17 with 10, 16 across the literal/distance border and ending at HLIT + HDIST."""
	cl = lens_of(19, {2: 2, 16: 2, 17: 2, 18: 2})
	seq = [(18, 127), (16, 3), (17, 7), (18, 46 - 11), (2, 0), (2, 0), (18, 53 - 11), (2, 0), (16, 5 - 3)]
	return dyn({200: 2, 201: 2, 255: 2, 256: 2}, {0: 2, 1: 2, 2: 2, 3: 2}, [200, 201, 255, 200, 256], n_lit=257, n_dist=4, cl_lens=cl, cl_seq=seq, hclen=18)


def long_then_short(bad=None):
	"""A dynamic block with long codes, then one with few short ones: the second block's tables must not keep entries of the first.
	bad: "dist" / "lit" make the refused variants, whose second block uses a code that only the first block has."""
	lit, dist = all_lengths_codes()
	w = BitWriter()
	write_stored_block(w, perm_bytes(0, 256) * 65, final=False)
	toks = [65 + i for i in range(13)] + [("match", 258, DIST_BASE[d]) for d in (0, 9, 13, 28)]
	write_dynamic_block(w, lit, dist, toks + [256], final=False)
	if "lit" == bad:     # '10' is literal 66 in the first block; the second has the one code '0'
		write_dynamic_block(w, lens_of(257, {256: 1}), [0], [("bits", 0b01, 2)])
	elif "dist" == bad:  # '10' is distance symbol 1 in the first block; the second has the one code '0'
		write_dynamic_block(w, lens_of(258, GOOD_LIT), [1], [A, 257, ("bits", 0b01, 2), 256])
	else:
		write_dynamic_block(w, lens_of(258, GOOD_LIT), [1], [A, ("match", 3, 1), B, 256])
	return w.bytes()


def block_sequences():
	out = []
	w = BitWriter()
	write_fixed_block(w, [A, B, ("match", 5, 2), 256], final=False)
	write_dynamic_block(w, lens_of(258, GOOD_LIT), [1], [A, ("match", 3, 1), B, 256], final=False)
	write_fixed_block(w, [200, A, ("match", 7, 3), 143, 144, 256])
	out.append(("fixed, dynamic, fixed", w.bytes()))
	w = BitWriter()
	write_fixed_block(w, [A, B, ("match", 5, 2), 256], final=False)
	write_stored_block(w, b"between", final=False)
	write_fixed_block(w, [200, A, ("match", 7, 3), 143, 144, 256])
	out.append(("fixed, stored, fixed", w.bytes()))
	out.append(("dynamic long, dynamic short", long_then_short()))
	return out


@functools.lru_cache(maxsize=None)
def tables_group():
	g = Group()
	g.add("all lengths and the chain", mk(chain(g.lead)))
	for name, payload in [("code-length code 1..7", cl_1_to_7()), ("literal/length root and root + 1", lit_root_walk()), ("130 codes of 8 bits", lit_130_of_8()),
			("distance root and root + 1", dist_root_walk()), ("max = root", max_equals_root()), ("HLIT 286, HDIST 30", header_counts()[0]),
			("HLIT 257, HDIST 1", header_counts()[1]), ("repeats", repeats())] + block_sequences():
		g.add(name, mk(payload))
	return tuple(g.members)


TABLES_SEAMS = (["lit_lengths_1_to_15", "dist_lengths_1_to_15", "cl_lengths_1_to_7", "lit_max_eq_root", "dist_max_eq_root", "cl_max_eq_root",
	"more_than_64_of_one_length", "more_than_128_of_one_length", "hlit_257", "hlit_286", "hdist_1", "hdist_30", "hclen_19",
	"repeat_16_across_the_border", "repeat_16_of_a_zero_left_by_17_18", "repeat_18_with_138", "repeat_17_with_10", "repeat_ends_at_hlit_plus_hdist",
	"repeat_of_more_than_64", "blocks_fixed_dynamic_fixed", "blocks_fixed_stored_fixed", "blocks_dynamic_long_then_short"]
	+ ["%s_L%d_%s" % (name, L, which) for name, top in (("lit", 15), ("dist", 15), ("cl", 7)) for L in range(1, top + 1) for which in ("first", "last")]
	+ ["%s_L%d_%s_of_many" % (name, L, which) for name, root in (("lit", LIT_ROOT), ("dist", DIST_ROOT)) for L in (root, root + 1) for which in ("first", "last")]
	+ ["cl_L7_first_of_many", "cl_L7_last_of_many"])
# HCLEN 4 lists the lengths of 16, 17, 18 and 0 only, so every length it can describe is 0 and the block has no end-of-block code: it
# can be reached by a refused stream alone (refusals(): "HCLEN 4"), where the host test asserts it.


# ---- the match copy ------------------------------------------------------------------------------

SMALL_CROSS = [(d, n) for n in range(3, 259) for d in range(1, 67)]
LARGE_DISTS, LARGE_LENS = (127, 128, 129, 191, 192, 193, 256, 4096, 32768), (3, 63, 64, 65, 127, 128, 129, 257, 258)
LARGE_CROSS = [(d, n) for d in LARGE_DISTS for n in LARGE_LENS]


def _cross_members(pairs, budget=52000):
	"""Fixed-block members of (distance, length) matches, each behind `distance` fresh literals of the permutation's walk."""
	out, toks, size, at = [], [], 0, 0
	for d, n in pairs:
		if size + d + n > budget:
			out.append(toks + [256])
			toks, size = [], 0
		toks += list(perm_bytes(at, d)) + [("match", n, d)]
		at = (at + d) & 255
		size += d + n
	out.append(toks + [256])
	members = []
	for t in out:
		w = BitWriter()
		write_fixed_block(w, t)
		members.append(mk(w.bytes()))
	return members


MATCH_PARTS = 4


@functools.lru_cache(maxsize=None)
def match_group(part):
	"""Part `part` of the small cross (the lengths dealt in quarters); the last part carries the large cross as well."""
	g = Group()
	n = len(SMALL_CROSS) // MATCH_PARTS
	for k, m in enumerate(_cross_members(SMALL_CROSS[part * n:] if part == MATCH_PARTS - 1 else SMALL_CROSS[part * n:(part + 1) * n])):
		g.add("distances 1..66, part %d.%d" % (part, k), m)
	if part < MATCH_PARTS - 1:
		return tuple(g.members)
	for k, m in enumerate(_cross_members([(d, n) for d, n in LARGE_CROSS if d <= 256])):
		g.add("distances 127..256, part %d" % k, m)
	for d in (4096, 32768):
		w = BitWriter()
		write_stored_block(w, perm_bytes(d >> 8, 256) * (d // 256), final=False)
		write_fixed_block(w, [("match", n, d) for n in LARGE_LENS] + [256])
		g.add("distance %d" % d, mk(w.bytes()))
	return tuple(g.members)


MATCH_SEAMS = ["copy_rounds_with_a_wrapping_step"]


def sources_are_distinct(m):
	"""Every match of the member copies from bytes of which any 256 consecutive ones are distinct."""
	w = walk_member(m)
	for p, mlen, dist in w.matches:
		src = w.data[p - dist:p - dist + min(mlen, dist)]
		for i in range(max(1, len(src) - 255)):
			win = src[i:i + 256]
			if len(set(win)) != len(win):
				return False
	return True


# ---- the output ----------------------------------------------------------------------------------

def sized(n, salt):
	"""A member of exactly n bytes: the permutation's walk as fixed literals, then matches at distance 256."""
	toks = list(perm_bytes(salt, min(n, 256)))
	r = n - len(toks)
	while r:
		if r < 3:
			toks += list(perm_bytes(salt + 100, r))
			break
		k = r if r <= 258 else min(258, r - 3)
		toks.append(("match", k, 256))
		r -= k
	w = BitWriter()
	write_fixed_block(w, toks + [256])
	return w.bytes()


def small_output(n, salt):
	w = BitWriter()
	if salt % 3:
		write_fixed_block(w, list(perm_bytes(7 * salt, n)) + [256])
	else:
		write_stored_block(w, perm_bytes(7 * salt, n))
	return w.bytes()


@functools.lru_cache(maxsize=None)
def output_group():
	g = Group()
	salt = 0
	for phase in range(16):
		for n in SMALL_ISIZES:
			g.align(phase=phase)
			salt += 1
			g.add("ISIZE %d at phase %d" % (n, phase), mk(small_output(n, salt)))
	g.align(phase=15)
	g.add("ISIZE 65536 at phase 15", mk(sized(SLOT, 1)))
	g.add("ISIZE 3", mk(small_output(3, 1)))
	g.add("ISIZE 0", mk(small_output(0, 0)))
	g.add("ISIZE 5", mk(small_output(5, 2)))
	for k, n in enumerate(CRC_ISIZES):
		g.add("ISIZE %d" % n, mk(sized(n, 2 + k)))
	return tuple(g.members)


OUTPUT_SEAMS = (["isize_%d_phase_%d" % (n, ph) for n in SMALL_ISIZES for ph in range(16)] + ["isize_65536_phase_15", "isize_0_between_two_members"]
	+ ["crc_isize_%d" % n for n in CRC_ISIZES])


def groups():
	"""name -> (members as (name, bytes), the seams the group must reach in a file that is one slice)."""
	out = {"bits": (bits_group(), BITS_SEAMS), "tables": (tables_group(), TABLES_SEAMS), "output": (output_group(), OUTPUT_SEAMS)}
	for part in range(MATCH_PARTS):
		out["matches %d" % part] = (match_group(part), MATCH_SEAMS if part == MATCH_PARTS - 1 else [])
	return out


GROUPS = ["bits", "tables", "output"] + ["matches %d" % part for part in range(MATCH_PARTS)]


def placement_free(seam):
	"""Seams that do not depend on where the member lies in its slice: they are reached under every ring slot setting."""
	return not seam.startswith(("straddle_", "end_on_", "lead", "chain_phase", "seek_phase", "isize_"))


# ---- refusals -------------------------------------------------------------------------------------

def fixed(tokens, final=True):
	w = BitWriter()
	write_fixed_block(w, tokens, final=final)
	return w.bytes()


def _eob_short_of_padding(lead):
	"""The end-of-block code cut one bit short, the payload ending on a word of the kernel's: only the zeros past it complete the code."""
	a = (-(lead + 9)) % 4 + 4
	lits = [144 + i for i in range(7)] + [65 + i for i in range(a)]
	w = BitWriter()
	write_fixed_block(w, lits + [("bits", 0, 6)])
	assert len(w.bits) == 8 * (9 + a) and 0 == (lead + 9 + a) % 4
	return member(w.bytes(), bytes(lits))


def _eob_from_the_footer(lead):
	"""No end-of-block code at all, and a CRC-32 whose first byte has seven zero bits where the code would be: all but the payload's
	bound says the member is fine."""
	a = (1 - lead - 6) % 4 + 4
	head = [144 + i for i in range(5)] + [65 + i for i in range(a - 2)]
	for x in range(144):
		for y in range(144):
			data = bytes(head + [x, y])
			if 0 == zlib.crc32(data) & 0x7f:
				w = BitWriter()
				write_fixed_block(w, list(data))
				assert len(w.bits) == 8 * (6 + a) and 1 == (lead + 6 + a) % 4
				return member(w.bytes(), data)
	raise AssertionError("no trailing literals give a CRC-32 with seven low zero bits")


def refusals():
	"""(name, status, function of the lead -> member): single-fault members and the status each must get.  "BadFraming" is the host
	scan's to refuse (a member the kernel would call that never gets past v2m_bgzf_decompress's walk), so only the walker sees it."""
	claim = b"a" * 10
	out = []

	def add(name, status, payload, data=claim, **kw):
		out.append((name, status, lambda lead, m=member(payload, data, **kw): m))

	w = BitWriter(); w.put(1, 1); w.put(3, 2)
	add("block type 3", "BadBlockType", w.bytes())
	w = BitWriter(); write_stored_block(w, b"hello", nlen=0)
	add("LEN != ~NLEN", "StoredLengths", w.bytes())
	add("HLIT 287", "TooManySymbols", dyn(GOOD_LIT, {0: 1}, [A, 256], n_lit=287))
	add("HDIST 31", "TooManySymbols", dyn(GOOD_LIT, {0: 1}, [A, 256], n_dist=31))
	add("incomplete code-length code", "BadCodeLengthCode", dyn({256: 1}, {0: 1}, [], cl_lens=lens_of(19, {1: 1, 2: 2, 0: 3}), cl_seq=[(0, 0)] * 256 + [(1, 0), (1, 0)]))
	add("over-subscribed code-length code", "BadCodeLengthCode", dyn({256: 1}, {0: 1}, [], cl_lens=lens_of(19, {0: 1, 1: 1, 2: 1}), cl_seq=[(0, 0)] * 256 + [(1, 0), (1, 0)]))
	add("no code-length codes", "BadCodeLengthCode", dyn({256: 1}, {0: 1}, [], cl_lens=[0] * 19, cl_seq=[]))
	add("repeat with no previous length", "BadRepeat", dyn(GOOD_LIT, {0: 1}, [], cl_seq=[(16, 0)]))
	add("repeat past HLIT + HDIST", "BadRepeat", dyn({256: 1}, {0: 1}, [], cl_seq=[(18, 127), (18, 127), (1, 0), (16, 3)]))
	add("over-subscribed literal/length code", "BadLitLenCode", dyn({256: 1, A: 1, B: 1}, {0: 1}, []))
	add("incomplete literal/length code", "BadLitLenCode", dyn({256: 2, A: 2}, {0: 1}, []))
	add("over-subscribed distance code", "BadDistCode", dyn(GOOD_LIT, {0: 1, 1: 1, 2: 1}, [], n_dist=3))
	add("incomplete distance code", "BadDistCode", dyn(GOOD_LIT, {0: 2, 1: 2}, [], n_dist=2))
	add("no end-of-block code", "NoEndOfBlock", dyn({A: 1, B: 1}, {0: 1}, [], n_lit=257))
	add("HCLEN 4", "NoEndOfBlock", dyn({}, {}, [], n_lit=257, n_dist=1, cl_lens=lens_of(19, {0: 1, 18: 2, 17: 3, 16: 3}), cl_seq=[(18, 127), (18, 119 - 11), (0, 0)], hclen=4))
	add("literal/length symbol 286", "BadLitLenSymbol", fixed([A, 286]))
	add("a literal/length code of the block before", "BadLitLenSymbol", long_then_short("lit"), data=bytes(40000))
	add("distance symbol 30", "BadDistSymbol", fixed([A, ("dsym", 3, 30)]))
	add("unused half of a one-code distance code", "BadDistSymbol", dyn(GOOD_LIT, {0: 1}, [A, 257, ("bits", 1, 1), 256]))
	add("a distance code of the block before", "BadDistSymbol", long_then_short("dist"), data=bytes(40000))
	add("distance too far back", "TooFarBack", fixed([A, ("match", 3, 2), 256]))
	add("a literal one past ISIZE", "OutputTooLong", fixed([A, B, 99, 256]), data=b"ab")
	add("a match one past ISIZE", "OutputTooLong", fixed([A, ("match", 3, 1), 256]), data=b"aaa")
	w = BitWriter(); write_stored_block(w, b"hello")
	add("a stored block one past ISIZE", "OutputTooLong", w.bytes(), data=b"hell")
	out.append(("end-of-block code one bit short of the padding", "PastPayload", _eob_short_of_padding))
	out.append(("end-of-block code supplied by the footer", "PastPayload", _eob_from_the_footer))
	add("distance extra bits past the payload", "PastPayload", fixed([A, B, 99, ("match", 3, DIST_BASE[29] + 8191), 256])[:5])
	w = BitWriter(); write_stored_block(w, b"hello")
	add("stored LEN one more than the payload holds", "PastPayload", w.bytes()[:-1])
	add("dynamic header cut inside the code lengths", "PastPayload", dyn(GOOD_LIT, {0: 1}, [A, 256])[:30])
	add("no final block", "PastPayload", fixed([A, 256], final=False))
	add("output one byte short of ISIZE", "ShortOutput", fixed([A, B, 256]), data=b"ab", isize=3)
	add("flipped CRC", "BadCrc", fixed([A, B, 256]), data=b"ab", crc=zlib.crc32(b"ab") ^ 1)
	return out


GPU_STATUSES = [s for s in STATUS if s not in ("Ok", "BadFraming")]
