"""BGZF input for the tests (test infrastructure): members built with Python's zlib (a raw deflate stream per piece plus the BGZF
header and footer), hand-built deflate streams for the cases zlib refuses, and zlib's own verdict on a payload."""

import struct
import zlib

EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
STRATEGIES = {"default": zlib.Z_DEFAULT_STRATEGY, "filtered": zlib.Z_FILTERED, "huffman": zlib.Z_HUFFMAN_ONLY, "rle": zlib.Z_RLE, "fixed": zlib.Z_FIXED}


def member(payload, data=None, crc=None, isize=None, xlen=6, subfield=b"BC", slen=2, flg=4, mtime=0, xfl=0, os_=255):
	"""One BGZF member around a raw deflate `payload`; CRC and ISIZE from `data` unless given."""
	if crc is None:
		crc = zlib.crc32(data)
	if isize is None:
		isize = len(data)
	size = 18 + len(payload) + 8
	assert size <= 65536, "a BGZF member holds at most 65 536 bytes (%d)" % size
	head = b"\x1f\x8b\x08" + bytes([flg]) + struct.pack("<I", mtime) + bytes([xfl, os_]) + struct.pack("<H", xlen) + subfield + struct.pack("<HH", slen, size - 1)
	return head + payload + struct.pack("<II", crc & 0xFFFFFFFF, isize & 0xFFFFFFFF)


def deflate_raw(data, level=6, strategy="default", mem_level=8, flush_at=None, flush_mode=zlib.Z_SYNC_FLUSH):
	c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, STRATEGIES[strategy])
	if flush_at is None:
		return c.compress(data) + c.flush()
	return c.compress(data[:flush_at]) + c.flush(flush_mode) + c.compress(data[flush_at:]) + c.flush()


def bgzf(data, piece=65280, eof=True, **deflate_args):
	"""`data` as BGZF: one member per `piece` bytes (piece 0: one empty member), then the EOF member if `eof`."""
	out = []
	if piece == 0:
		out.append(member(deflate_raw(b"", **deflate_args), b""))
	else:
		for i in range(0, len(data), piece):
			chunk = data[i:i + piece]
			out.append(member(deflate_raw(chunk, **deflate_args), chunk))
	if eof:
		out.append(EOF_MEMBER)
	return b"".join(out)


def zlib_inflate(payload):
	"""What zlib's inflate makes of a raw deflate payload: the bytes, or None when it refuses it (an error, or a stream without a final
	block).  Bytes after the final block are left over, as zlib leaves them."""
	d = zlib.decompressobj(-15)
	try:
		out = d.decompress(payload)
	except zlib.error:
		return None
	return out if d.eof else None


def member_accepted(m):
	"""zlib's verdict on a whole member (framing assumed fine): its bytes if the payload inflates and CRC-32 and ISIZE match, else None."""
	out = zlib_inflate(m[18:len(m) - 8])
	crc, isize = struct.unpack_from("<II", m, len(m) - 8)
	if out is None or len(out) != isize or zlib.crc32(out) != crc:
		return None
	return out


class BitWriter:
	"""Deflate's bit order: values LSB first, Huffman codes MSB first."""

	def __init__(self):
		self.bits = []

	def put(self, value, n):
		self.bits += [(value >> i) & 1 for i in range(n)]

	def code(self, code, length):
		self.bits += [(code >> (length - 1 - i)) & 1 for i in range(length)]

	def align(self):
		while len(self.bits) % 8:
			self.bits.append(0)

	def raw(self, data):
		self.align()
		for b in data:
			self.put(b, 8)

	def bytes(self):
		bits = self.bits + [0] * (-len(self.bits) % 8)
		return bytes(sum(bits[i + k] << k for k in range(8)) for i in range(0, len(bits), 8))


def canonical(lengths):
	"""Canonical codes (RFC 1951 section 3.2.2) of a list of code lengths: code per symbol (None for length 0)."""
	bl = [0] * 16
	for L in lengths:
		if L:
			bl[L] += 1
	nxt, code = [0] * 16, 0
	for L in range(1, 16):
		code = (code + bl[L - 1]) << 1 if L > 1 else 0
		nxt[L] = code
	out = []
	for L in lengths:
		if L:
			out.append(nxt[L])
			nxt[L] += 1
		else:
			out.append(None)
	return out


CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
# a complete code-length code over all 19 symbols: 13 of length 4, 6 (lengths 10..15) of length 5
CL_LENS = [5 if 10 <= s <= 15 else 4 for s in range(19)]


def fixed_lengths():
	return [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, [5] * 32


def write_fixed_block(w, tokens, final=True):
	w.put(1 if final else 0, 1)
	w.put(1, 2)
	lit, dist = fixed_lengths()
	write_tokens(w, tokens, lit, dist)


def write_stored_block(w, data, final=True, nlen=None):
	"""A stored block (final or not): header, zero bits to the byte boundary, LEN, NLEN (~LEN unless given), the bytes."""
	w.put(1 if final else 0, 1)
	w.put(0, 2)
	w.align()
	w.put(len(data) & 0xffff, 16)
	w.put((~len(data) if nlen is None else nlen) & 0xffff, 16)
	w.raw(data)


def write_dynamic_block(w, lit_lens, dist_lens, tokens, final=True, cl_lens=None, cl_seq=None, hlit=None, hdist=None, hclen=19):
	"""A dynamic block.  cl_seq: the code-length symbols as (symbol, extra) pairs (default: the lengths one by one); hlit / hdist override
	the counts written into the header; hclen: how many of the code-length code's lengths the header lists (the rest must be 0)."""
	cl_lens = CL_LENS if cl_lens is None else cl_lens
	w.put(1 if final else 0, 1)
	w.put(2, 2)
	w.put((len(lit_lens) if hlit is None else hlit) - 257, 5)
	w.put((len(dist_lens) if hdist is None else hdist) - 1, 5)
	assert 4 <= hclen <= 19 and not any(cl_lens[s] for s in CL_ORDER[hclen:])
	w.put(hclen - 4, 4)
	for s in CL_ORDER[:hclen]:
		w.put(cl_lens[s], 3)
	cl_codes = canonical(cl_lens)
	for sym, extra in (cl_seq if cl_seq is not None else [(L, 0) for L in list(lit_lens) + list(dist_lens)]):
		w.code(cl_codes[sym], cl_lens[sym])
		if sym == 16:
			w.put(extra, 2)
		elif sym == 17:
			w.put(extra, 3)
		elif sym == 18:
			w.put(extra, 7)
	write_tokens(w, tokens, lit_lens, dist_lens)


def _length_code(n):
	for i in range(29):
		if i == 28:
			base, eb = 258, 0
		elif i < 8:
			base, eb = 3 + i, 0
		else:
			eb = (i >> 2) - 1
			base = ((4 + (i & 3)) << eb) + 3
		if base <= n < base + (1 << eb) or (i == 28 and n == 258):
			if i == 27 and n == 258:
				continue
			return 257 + i, n - base, eb
	raise ValueError(n)


def _dist_code(d):
	for i in range(30):
		eb = 0 if i < 4 else (i >> 1) - 1
		base = 1 + i if i < 4 else ((2 + (i & 1)) << eb) + 1
		if base <= d < base + (1 << eb):
			return i, d - base, eb
	raise ValueError(d)


def write_tokens(w, tokens, lit_lens, dist_lens):
	"""tokens: ints (literal / end-of-block / any raw literal-length symbol), ('match', length, distance), ('dsym', length, distance symbol),
	('bits', value, n): n raw bits."""
	lit_codes, dist_codes = canonical(lit_lens), canonical(dist_lens)
	for t in tokens:
		if isinstance(t, int):
			w.code(lit_codes[t], lit_lens[t])
			continue
		kind, length, d = t
		if kind == "bits":
			w.put(length, d)
			continue
		sym, extra, eb = _length_code(length)
		w.code(lit_codes[sym], lit_lens[sym])
		w.put(extra, eb)
		if kind == "match":
			ds, dextra, deb = _dist_code(d)
			w.code(dist_codes[ds], dist_lens[ds])
			w.put(dextra, deb)
		else:   # a raw distance symbol with no extra bits
			w.code(dist_codes[d], dist_lens[d])
