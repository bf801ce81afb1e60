"""A CPU reference for the GPU BGZF encoder (test infrastructure, pure Python + numpy).

encode_member(piece) writes the BGZF member the encoder of vcf2multialign_amd/csrc/bgzf_kernels.hpp documents for one piece of
<= 65 280 bytes, byte for byte: zlib's Z_RLE tokens (RFC 1951 matches of distance 1 only), one final dynamic block whose literal/length
code is a length-limited Huffman code (limit 15; the code-length code's limit 7) with one distance code of length 1, or a stored block
when that is not larger; the framing of the SAM/BAM specification, section 4.1.  encode(data) is the members of every piece.
inflate_tokens(raw) is a small RFC 1951 inflater that returns what each block says (its header fields, code lengths and tokens), so
that tests can compare encodings token by token as well as byte by byte.

The kernel's free choices are modelled here as the kernel makes them (its header comment and bgzf_huff_build): Huffman keys
frequency << 9 | symbol in ascending order, Moffat-Katajainen lengths, lengths over the limit folded into it and leaves taken off the
longest level below it until the Kraft sum is 1, the shortest lengths to the highest keys, dummies of frequency 1 when fewer than two
symbols are used; the end of block counted once; 16 / 17 / 18 run-length coding of the code lengths; stored iff it is not larger."""

import heapq
import zlib

import numpy as np

PIECE = 65280
HEAD = bytes([0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0])   # up to BSIZE
HEADER_BYTES = 18
FOOTER_BYTES = 8
STORED_OVERHEAD = HEADER_BYTES + 5 + FOOTER_BYTES
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)

# RFC 1951 section 3.2.5: (base, extra bits) of the length symbols 257..285 and of the distance symbols 0..29
LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
DIST_BASE = (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
	12289, 16385, 24577)
DIST_EXTRA = (0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13)


class DeflateError(ValueError):
	pass


# ---- inflater ------------------------------------------------------------------------------------------

def _decode_table(lengths, what, allow_one=False, fixed=False):
	"""{(code read LSB first, length): symbol} of a canonical code; rejects over-subscribed codes and incomplete ones (except one code
	of length 1 when allow_one, and a code with no symbols at all when allow_one: a block of literals only; and the fixed distance
	code, whose 30 codes of 5 bits RFC 1951 defines incomplete)."""
	lengths = list(lengths)
	used = [l for l in lengths if l]
	kraft = sum(1 << (15 - l) for l in used)
	if kraft > 1 << 15:
		raise DeflateError("%s code is over-subscribed" % what)
	if kraft < 1 << 15 and not fixed and not (allow_one and (used == [1] or not used)):
		raise DeflateError("%s code is incomplete" % what)
	table = {}
	for sym, code, l in _canonical(lengths):
		table[(int(bin(code)[2:].zfill(l)[::-1], 2), l)] = sym
	return table


def _canonical(lengths):
	"""(symbol, code, length) of the canonical code of `lengths` (RFC 1951 section 3.2.2), codes MSB first."""
	bl_count = [0] * 16
	for l in lengths:
		if l:
			bl_count[l] += 1
	code, next_code = 0, [0] * 16
	for b in range(1, 16):
		code = (code + bl_count[b - 1]) << 1
		next_code[b] = code
	out = []
	for sym, l in enumerate(lengths):
		if l:
			out.append((sym, next_code[l], l))
			next_code[l] += 1
	return out


class _Bits:
	def __init__(self, raw):
		bits = np.unpackbits(np.frombuffer(bytes(raw) + b"\0\0\0\0", dtype=np.uint8), bitorder="little").astype(np.uint32)
		n = len(bits) - 32
		win = np.zeros(n, dtype=np.uint32)
		for i in range(24):   # the 24 bits from every position on, LSB first
			win |= bits[i:i + n] << np.uint32(i)
		self.win = win.tolist()
		self.n = n
		self.pos = 0

	def get(self, k):
		if self.pos + k > self.n:
			raise DeflateError("input ends inside a block")
		v = self.win[self.pos] & ((1 << k) - 1) if k else 0
		self.pos += k
		return v


def _fast_table(table):
	"""A lookup of every max-length window -> (symbol, length), from a {(code, length): symbol} table."""
	max_len = max((l for _, l in table), default=1)
	lut = [None] * (1 << max_len)
	for (code, l), sym in table.items():
		for hi in range(1 << (max_len - l)):
			lut[code | (hi << l)] = (sym, l)
	return lut, max_len


def inflate_tokens(raw):
	"""Inflates a raw deflate stream: a list of one dict per block with 'btype', 'final', 'tokens' ([('lit', b)] / [('match', length,
	distance)]; a stored block's bytes as literals) and, for a dynamic block, 'hlit', 'hdist', 'hclen', 'cl_lengths' (the 19 lengths of
	the code-length code, by symbol), 'lit_lengths' (HLIT of them) and 'dist_lengths' (HDIST of them).  Raises DeflateError on a
	malformed stream (an over-subscribed or incomplete code included) and on a distance before the start of the output."""
	try:
		return _inflate(raw)
	except IndexError:
		raise DeflateError("input ends inside a block") from None


def _inflate(raw):
	br = _Bits(raw)
	blocks, produced = [], 0
	while True:
		final, btype = br.get(1), br.get(2)
		blk = {"final": final, "btype": btype}
		if btype == 0:
			br.pos = (br.pos + 7) & ~7
			n, nn = br.get(16), br.get(16)
			if n != (~nn & 0xffff):
				raise DeflateError("stored block LEN / NLEN mismatch")
			if br.pos + 8 * n > br.n:
				raise DeflateError("input ends inside a stored block")
			start = br.pos // 8
			blk["tokens"] = [("lit", b) for b in bytes(raw[start:start + n])]
			br.pos += 8 * n
		elif btype in (1, 2):
			if btype == 1:
				lit_lengths = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
				dist_lengths = [5] * 30
			else:
				hlit, hdist, hclen = br.get(5) + 257, br.get(5) + 1, br.get(4) + 4
				cl = [0] * 19
				for i in range(hclen):
					cl[CL_ORDER[i]] = br.get(3)
				cl_lut, cl_max = _fast_table(_decode_table(cl, "code-length"))
				seq = []
				while len(seq) < hlit + hdist:
					e = cl_lut[br.win[br.pos] & ((1 << cl_max) - 1)]
					if e is None:
						raise DeflateError("invalid code-length code")
					br.get(e[1])
					s = e[0]
					if s < 16:
						seq.append(s)
					elif s == 16:
						if not seq:
							raise DeflateError("repeat with no previous length")
						seq += [seq[-1]] * (3 + br.get(2))
					elif s == 17:
						seq += [0] * (3 + br.get(3))
					else:
						seq += [0] * (11 + br.get(7))
				if len(seq) > hlit + hdist:
					raise DeflateError("code lengths run past HLIT + HDIST")
				lit_lengths, dist_lengths = seq[:hlit], seq[hlit:]
				if lit_lengths[256] == 0:
					raise DeflateError("no end-of-block code")
				blk.update(hlit=hlit, hdist=hdist, hclen=hclen, cl_lengths=cl, lit_lengths=lit_lengths, dist_lengths=dist_lengths)
			lit_lut, lit_max = _fast_table(_decode_table(lit_lengths, "literal/length"))
			dist_lut, dist_max = _fast_table(_decode_table(dist_lengths, "distance", allow_one=True, fixed=btype == 1))
			toks = []
			win, n, pos = br.win, br.n, br.pos
			lit_mask, dist_mask = (1 << lit_max) - 1, (1 << dist_max) - 1
			while True:
				if pos >= n:
					raise DeflateError("input ends inside a block")
				e = lit_lut[win[pos] & lit_mask]
				if e is None:
					raise DeflateError("invalid literal/length code")
				s = e[0]
				pos += e[1]
				if s < 256:
					toks.append(("lit", s))
					produced += 1
					continue
				if s == 256:
					break
				if s > 285:
					raise DeflateError("invalid length symbol %d" % s)
				i = s - 257
				length = LEN_BASE[i] + (win[pos] & ((1 << LEN_EXTRA[i]) - 1))
				pos += LEN_EXTRA[i]
				e = dist_lut[win[pos] & dist_mask]
				if e is None or e[0] > 29:
					raise DeflateError("invalid distance code")
				pos += e[1]
				d = e[0]
				dist = DIST_BASE[d] + (win[pos] & ((1 << DIST_EXTRA[d]) - 1))
				pos += DIST_EXTRA[d]
				if dist > produced:
					raise DeflateError("distance %d before the start of the output" % dist)
				toks.append(("match", length, dist))
				produced += length
			if pos > n:
				raise DeflateError("input ends inside a block")
			br.pos = pos
			blk["tokens"] = toks
		else:
			raise DeflateError("BTYPE 11")
		if btype == 0:
			produced += len(blk["tokens"])
		blocks.append(blk)
		if final:
			break
	return blocks


def detokenize(blocks):
	"""The bytes a list of blocks from inflate_tokens stands for."""
	out = bytearray()
	for blk in blocks:
		for t in blk["tokens"]:
			if t[0] == "lit":
				out.append(t[1])
			else:
				_, length, dist = t
				for _ in range(length):
					out.append(out[-dist])
	return bytes(out)


def tokens_of(blocks):
	return [t for blk in blocks for t in blk["tokens"]]


# ---- tokens -------------------------------------------------------------------------------------------

def runs(piece):
	"""(start, length, byte) arrays of the runs of equal bytes."""
	a = np.frombuffer(bytes(piece), dtype=np.uint8)
	if len(a) == 0:
		return np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0, np.uint8)
	starts = np.flatnonzero(np.concatenate(([True], a[1:] != a[:-1])))
	lens = np.diff(np.concatenate((starts, [len(a)])))
	return starts, lens, a[starts]


def rle_tokens(piece):
	"""zlib's Z_RLE tokens of a piece: per run of n equal bytes one literal, then distance-1 matches of 258 and one of 3..257, a
	remainder < 3 as literals."""
	out = []
	_, lens, vals = runs(piece)
	for n, b in zip(lens.tolist(), vals.tolist()):
		out.append(("lit", b))
		q, r = divmod(n - 1, 258)
		out += [("match", 258, 1)] * q
		if r >= 3:
			out.append(("match", r, 1))
		else:
			out += [("lit", b)] * r
	return out


def length_code(length):
	"""(index 0..28 of the length symbol 257 + index, extra bits, their value) of a match length 3..258."""
	if length == 258:
		return 28, 0, 0
	for i in range(27, -1, -1):
		if LEN_BASE[i] <= length:
			return i, LEN_EXTRA[i], length - LEN_BASE[i]
	raise ValueError(length)


_LEN_SYM = np.zeros(259, np.int64)
_LEN_EB = np.zeros(259, np.int64)
_LEN_EV = np.zeros(259, np.int64)
for _l in range(3, 259):
	_i, _eb, _ev = length_code(_l)
	_LEN_SYM[_l], _LEN_EB[_l], _LEN_EV[_l] = 257 + _i, _eb, _ev


def _token_arrays(piece):
	"""The Z_RLE tokens as arrays: symbol (a byte, or 257 + a length index) and match length (0 for a literal), in stream order."""
	_, lens, vals = runs(piece)
	m = lens - 1
	q, r = m // 258, m % 258
	tail_match = r >= 3
	# per run: 1 literal, q matches of 258, then one match of r or r literals
	n_tok = 1 + q + np.where(tail_match, 1, r)
	run_of = np.repeat(np.arange(len(lens)), n_tok)
	k = np.arange(len(run_of)) - np.repeat(np.cumsum(n_tok) - n_tok, n_tok)   # the token's index within its run
	qr, rr, tm = q[run_of], r[run_of], tail_match[run_of]
	mlen = np.where(k == 0, 0, np.where(k <= qr, 258, np.where(tm, rr, 0)))
	sym = np.where(mlen > 0, _LEN_SYM[mlen], vals[run_of].astype(np.int64))
	return sym, mlen


# ---- Huffman codes ------------------------------------------------------------------------------------

def moffat_katajainen(freqs):
	"""Huffman code lengths of ascending frequencies (Moffat and Katajainen, 1995), the longest first, as the kernel computes them."""
	a = list(freqs)
	m = len(a)
	a[0] += a[1]
	root, leaf = 0, 2
	for nxt in range(1, m - 1):
		if leaf >= m or a[root] < a[leaf]:
			a[nxt] = a[root]
			a[root] = nxt
			root += 1
		else:
			a[nxt] = a[leaf]
			leaf += 1
		if leaf >= m or (root < nxt and a[root] < a[leaf]):
			a[nxt] += a[root]
			a[root] = nxt
			root += 1
		else:
			a[nxt] += a[leaf]
			leaf += 1
	a[m - 2] = 0
	for nxt in range(m - 3, -1, -1):
		a[nxt] = a[a[nxt]] + 1
	avail, used, depth, nxt, root = 1, 0, 0, m - 1, m - 2
	while avail > 0:
		while root >= 0 and a[root] == depth:
			used += 1
			root -= 1
		while avail > used:
			a[nxt] = depth
			nxt -= 1
			avail -= 1
		avail, depth, used = 2 * used, depth + 1, 0
	return a


def huffman_keys(freq):
	"""The kernel's sorted keys frequency << 9 | symbol of the used symbols, with dummies of frequency 1 when fewer than two are used."""
	keys = [(int(f) << 9) | s for s, f in enumerate(freq) if f]
	if not keys:
		keys = [(1 << 9) | 0, (1 << 9) | 1]
	elif len(keys) == 1:
		keys.append((1 << 9) | (0 if keys[0] & 511 else 1))
	return sorted(keys)


def unlimited_lengths(freq):
	"""{symbol: length} of the kernel's Huffman code before the limit."""
	keys = huffman_keys(freq)
	a = moffat_katajainen([k >> 9 for k in keys])
	return {k & 511: l for k, l in zip(keys, a)}


def huffman_lengths(freq, max_len):
	"""Code lengths (0: unused) of the kernel's length-limited Huffman code of freq (bgzf_huff_build)."""
	keys = huffman_keys(freq)
	a = moffat_katajainen([k >> 9 for k in keys])
	bl_count = [0] * 17
	for l in a:
		bl_count[min(l, max_len)] += 1
	total = sum(bl_count[l] << (max_len - l) for l in range(1, max_len + 1))
	while total > 1 << max_len:
		bl_count[max_len] -= 1
		for l in range(max_len - 1, 0, -1):
			if bl_count[l]:
				bl_count[l] -= 1
				bl_count[l + 1] += 2
				break
		total -= 1
	lengths = [0] * len(freq)
	j = len(keys)
	for l in range(1, max_len + 1):
		for _ in range(bl_count[l]):
			j -= 1
			lengths[keys[j] & 511] = l
	return lengths


def reversed_codes(lengths):
	"""Canonical codes bit-reversed for deflate's LSB-first packing (0 for unused symbols)."""
	codes = [0] * len(lengths)
	for sym, code, l in _canonical(lengths):
		codes[sym] = int(bin(code)[2:].zfill(l)[::-1], 2)
	return codes


def huffman_optimum(freq):
	"""The smallest total bit cost sum(freq * length) of any prefix code of the used symbols (heapq Huffman; 0 for < 2 symbols)."""
	h = [int(f) for f in freq if f]
	if len(h) < 2:
		return 0
	heapq.heapify(h)
	cost = 0
	while len(h) > 1:
		x = heapq.heappop(h) + heapq.heappop(h)
		cost += x
		heapq.heappush(h, x)
	return cost


# ---- members ------------------------------------------------------------------------------------------

def code_length_tokens(seq):
	"""The kernel's run-length coding of a code-length sequence: [(symbol, extra)]."""
	out, i, n = [], 0, len(seq)
	while i < n:
		l, run = seq[i], 1
		while i + run < n and seq[i + run] == l:
			run += 1
		i += run
		if l == 0:
			while run >= 11:
				r = min(run, 138)
				out.append((18, r - 11))
				run -= r
			if run >= 3:
				out.append((17, run - 3))
				run = 0
			out += [(0, 0)] * run
		else:
			out.append((l, 0))
			run -= 1
			while run >= 3:
				r = min(run, 6)
				out.append((16, r - 3))
				run -= r
			out += [(l, 0)] * run
	return out


class Plan:
	"""Everything the encoder decides for one piece (also what the model's own tests look at)."""

	def __init__(self, piece, tokens=None):
		"""tokens: other tokens for the piece than the Z_RLE ones (distance 1 only; for tests that need a different valid encoding)."""
		piece = bytes(piece)
		if not 0 < len(piece) <= PIECE:
			raise ValueError("a piece is 1..65280 bytes")
		self.piece = piece
		if tokens is None:
			self.sym, self.mlen = _token_arrays(piece)
		else:
			assert all(t[0] == "lit" or t[2] == 1 for t in tokens)
			self.mlen = np.array([0 if t[0] == "lit" else t[1] for t in tokens], np.int64)
			self.sym = np.array([t[1] if t[0] == "lit" else _LEN_SYM[t[1]] for t in tokens], np.int64)
		freq = np.bincount(self.sym, minlength=288)
		freq[256] += 1   # end of block
		self.freq = [int(f) for f in freq[:286]]
		self.lit_len = huffman_lengths(self.freq, 15)
		n_lit = 286
		while n_lit > 257 and self.lit_len[n_lit - 1] == 0:
			n_lit -= 1
		self.n_lit = n_lit
		self.cl_seq = self.lit_len[:n_lit] + [1]   # then the one distance code's length
		self.cl_tokens = code_length_tokens(self.cl_seq)
		self.cl_freq = [0] * 19
		for s, _ in self.cl_tokens:
			self.cl_freq[s] += 1
		self.cl_len = huffman_lengths(self.cl_freq, 7)
		n_cl = 19
		while n_cl > 4 and self.cl_len[CL_ORDER[n_cl - 1]] == 0:
			n_cl -= 1
		self.n_cl = n_cl
		self.header_bits = 3 + 5 + 5 + 4 + 3 * n_cl + sum(self.cl_len[s] + {16: 2, 17: 3, 18: 7}.get(s, 0) for s, _ in self.cl_tokens)
		lit_len = np.array(self.lit_len + [0, 0], np.int64)
		self.token_bits = int((lit_len[self.sym] + _LEN_EB[self.mlen] + (self.mlen > 0)).sum())
		self.data_bits = self.header_bits + self.token_bits + self.lit_len[256]
		self.dynamic_bytes = HEADER_BYTES + (self.data_bits + 7) // 8 + FOOTER_BYTES
		self.stored_bytes = len(piece) + STORED_OVERHEAD
		self.stored = self.stored_bytes <= self.dynamic_bytes

	def deflate(self):
		"""The raw deflate payload of the dynamic block."""
		lit_code = reversed_codes(self.lit_len)
		cl_code = reversed_codes(self.cl_len)
		vals, nbits = [1 | (2 << 1), self.n_lit - 257, 0, self.n_cl - 4], [3, 5, 5, 4]
		for i in range(self.n_cl):
			vals.append(self.cl_len[CL_ORDER[i]])
			nbits.append(3)
		for s, extra in self.cl_tokens:
			eb = {16: 2, 17: 3, 18: 7}.get(s, 0)
			vals.append(cl_code[s] | (extra << self.cl_len[s]))
			nbits.append(self.cl_len[s] + eb)
		code = np.array(lit_code + [0, 0], np.int64)
		ln = np.array(self.lit_len + [0, 0], np.int64)
		l = ln[self.sym]
		eb = _LEN_EB[self.mlen]
		# a match: its length code, the extra bits, then distance code 0 (one 0 bit)
		tv = code[self.sym] | (_LEN_EV[self.mlen] << l)
		tn = l + eb + (self.mlen > 0)
		v = np.concatenate((np.array(vals, np.int64), tv, [lit_code[256]]))
		n = np.concatenate((np.array(nbits, np.int64), tn, [self.lit_len[256]]))
		assert int(n.sum()) == self.data_bits
		bits = (v[:, None] >> np.arange(32)) & 1
		bits = bits[np.arange(32)[None, :] < n[:, None]]
		return np.packbits(bits.astype(np.uint8), bitorder="little").tobytes()

	def member(self):
		crc = zlib.crc32(self.piece).to_bytes(4, "little")
		isize = len(self.piece).to_bytes(4, "little")
		if self.stored:
			n = len(self.piece)
			body = bytes([1]) + n.to_bytes(2, "little") + (~n & 0xffff).to_bytes(2, "little") + self.piece
			size = self.stored_bytes
		else:
			body = self.deflate()
			size = self.dynamic_bytes
		out = HEAD + (size - 1).to_bytes(2, "little") + body + crc + isize
		assert len(out) == size
		return out


def encode_member(piece):
	"""The BGZF member of one piece of 1..65280 bytes."""
	return Plan(piece).member()


def encode(data):
	"""The members of every 65 280-byte piece of data, concatenated (no EOF member; b"" for b"")."""
	data = bytes(data)
	return b"".join(encode_member(data[i:i + PIECE]) for i in range(0, len(data), PIECE))


def member_payload(member):
	"""The raw deflate payload of one member."""
	return member[HEADER_BYTES:len(member) - FOOTER_BYTES]
