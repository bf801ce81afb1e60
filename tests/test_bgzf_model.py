"""The CPU reference of the GPU BGZF encoder (tests/deflate_ref.py), checked on its own before tests/test_gpu_bgzf.py compares the
kernel's members with it byte for byte: its inflater against zlib, its tokens against zlib's Z_RLE, its members against three decoders,
its Huffman codes against the optimum, and every edge input of the GPU table against the precondition that makes the case worth having.

The edge inputs are built here and imported by the GPU tests."""

import gzip
import random
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import deflate_ref as D
from test_bgzf_host import EOF_MEMBER, bgzf_members

PIECE = D.PIECE
SEG = 256


# ---- edge inputs (shared with tests/test_gpu_bgzf.py) -----------------------------------------------------

def a2m_like(seed, n, gap_p=0.02, mean_gap=20):
	"""Random ACGT with runs of '-' of exponential lengths: what an A2M row body looks like."""
	rng = np.random.default_rng(seed)
	out = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)]
	n_gaps = rng.binomial(max(n // 50, 0), gap_p)
	for p, l in zip(rng.integers(0, max(n, 1), n_gaps), 1 + rng.exponential(mean_gap, n_gaps).astype(np.int64)):
		out[p:p + l] = ord("-")
	return out.tobytes()


def spread(counts):
	"""A sequence with counts[b] copies of byte b and no two equal bytes adjacent (so every byte is a literal token): the copies in
	symbol order, laid on the even positions and then on the odd ones.  Needs max(counts) < sum(counts) / 2."""
	syms = np.repeat(np.arange(len(counts), dtype=np.uint8), counts)
	out = np.empty_like(syms)
	half = (len(syms) + 1) // 2
	out[0::2], out[1::2] = syms[:half], syms[half:]
	return out.tobytes()


SIZES = [1, 2, 3, 4, 15, 16, 17, 255, 256, 257, 511, 512, 513, 65024, 65025, 65279, 65280, 65281]
EDGE_RUN_LENGTHS = [1, 2, 3, 4, 258, 259, 260, 261, 515, 516, 517, 518]


def size_pieces():
	"""(name, data) per size of SIZES, A2M-like and one run of '-' (tails that leave segments empty or partly filled, and the 16-byte
	LDS load tail)."""
	out = []
	for n in SIZES:
		out.append(("a2m n=%d" % n, a2m_like(n, n)))
		out.append(("run n=%d" % n, b"-" * n))
	return out


def segment_edge_pieces():
	"""Full pieces of A2M-like background with planted runs (bytes that are not ACGT) starting at 256 k - o for every o in 0..257 and
	every length of EDGE_RUN_LENGTHS, 4 segments apart; then runs over several whole segments, from byte 0 and to the last byte.
	Returns [(name, piece, [(start, length)])]."""
	cases = [(o, l) for l in EDGE_RUN_LENGTHS for o in range(258)]
	out, i, p = [], 0, 0
	ks = list(range(2, 251, 4))
	while i < len(cases):
		piece = bytearray(a2m_like(1000 + p, PIECE, gap_p=0))
		planted = []
		for k in ks[:len(cases) - i]:
			o, l = cases[i]
			start = SEG * k - o
			piece[start:start + l] = bytes([b"N*\0\xff"[i % 4]]) * l
			planted.append((start, l))
			i += 1
		out.append(("segment edges %d" % p, bytes(piece), planted))
		p += 1
	piece = bytearray(a2m_like(2000, PIECE, gap_p=0))
	spans = [(0, 1000), (1300, 5000), (7000, 258 * 20 + 1), (20000, 3 * SEG), (20000 + 4 * SEG, 4 * SEG), (PIECE - 700, 700)]
	for n, (s, l) in enumerate(spans):
		piece[s:s + l] = bytes([b"N*"[n % 2]]) * l
	out.append(("whole segments", bytes(piece), spans))
	return out


def byte_value_pieces():
	"""Every byte value in: iid bytes (a stored block), a skewed distribution (a dynamic block), single-valued full pieces of 0x00 and
	0xff, and one-byte pieces (one literal and the end of block)."""
	rng = np.random.default_rng(77)
	out = [("iid", rng.integers(0, 256, PIECE, dtype=np.uint8).tobytes())]
	counts = np.maximum(1, (1900 * 0.97 ** np.arange(256)).astype(np.int64))
	out.append(("skewed", rng.permutation(np.repeat(np.arange(256, dtype=np.uint8), counts)).tobytes()))
	out.append(("all 0x00", b"\0" * PIECE))
	out.append(("all 0xff", b"\xff" * PIECE))
	out += [("one byte %d" % b, bytes([b])) for b in range(256)]
	return out


# 1, 2, 4, 7, 12, 20, ...: each the sum of the two before plus one.  Plain Fibonacci frequencies do not force long codes here: the
# builder's ties (a leaf before an equal internal node) balance them into 12 bits at 22 symbols.  These have no ties.
STEEP = [1, 2]
while len(STEEP) < 20:
	STEEP.append(STEEP[-1] + STEEP[-2] + 1)


def fibonacci_piece():
	"""Literals of frequencies 1, 2, 4, 7, ..., 17 710 (20 byte values, no two equal bytes adjacent): with the end of block the unlimited
	Huffman code needs 20 bits, so the literal/length code's 15-bit limit folds it."""
	counts = np.zeros(256, np.int64)
	counts[65:65 + len(STEEP)] = STEEP
	return spread(counts)


# code lengths: how many literals get each; the end of block takes one of the 15s.  Found with the model: equal lengths are not
# adjacent in byte order (no 16-repeats merge them), and the counts of the code-length symbols then need a 9-bit unlimited code.
CL_LIMIT_COUNTS = {3: 1, 4: 1, 5: 2, 6: 37, 7: 13, 8: 5, 9: 9, 10: 14, 11: 21, 13: 34, 14: 56, 15: 56}


def cl_limit_lengths():
	"""The intended literal code lengths of cl_limit_piece, by byte value."""
	lens = sorted(l for l, c in CL_LIMIT_COUNTS.items() for _ in range(c))
	lens.remove(15)
	order = list(range(0, len(lens), 2)) + list(range(1, len(lens), 2))
	out = [0] * 256
	for b, l in zip(order, lens):
		out[b] = l
	return out


def cl_limit_piece():
	"""Literals of dyadic frequencies 2^(15 - length) for cl_limit_lengths (the end of block the one of frequency 1): the Huffman code
	has exactly those lengths, and its code-length code needs the 7-bit limit."""
	return spread([1 << (15 - l) if l else 0 for l in cl_limit_lengths()])


def tie_sweep():
	"""Pieces of iid bytes whose first r bytes are one run, for r through the point where the stored block and the dynamic one have the
	same size: [(r, piece, stored_bytes - dynamic_bytes)] for a window of r around the first exact tie."""
	base = np.random.default_rng(4242).integers(0, 256, 4096, dtype=np.uint8)
	base[base == 0] = 1   # the run is of 0x00; nothing else is

	def piece(r):
		b = base.copy()
		b[:r] = 0
		return b.tobytes()

	lo, hi = 0, 4096   # stored_bytes - dynamic_bytes rises with r: < 0 at 0, > 0 at the end; bisect for the crossing
	while hi - lo > 1:
		mid = (lo + hi) // 2
		pl = D.Plan(piece(mid))
		if pl.stored_bytes - pl.dynamic_bytes < 0:
			lo = mid
		else:
			hi = mid
	out = []
	for r in range(max(0, hi - 24), hi + 24):
		pl = D.Plan(piece(r))
		out.append((r, pl.piece, pl.stored_bytes - pl.dynamic_bytes))
	return out


def random_pieces(n_seeds=64):
	"""A2M-like pieces of varied sizes, gap rates and gap lengths."""
	out = []
	for seed in range(n_seeds):
		rng = random.Random(seed)
		n = rng.choice([rng.randint(1, 4000), rng.randint(1, PIECE), PIECE])
		out.append(("random %d" % seed, a2m_like(500 + seed, n, gap_p=rng.choice([0, 0.02, 0.2, 1.0]), mean_gap=rng.choice([3, 20, 300]))))
	return out


# ---- the inflater -----------------------------------------------------------------------------------

def _zlib(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
	c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
	return c.compress(data) + c.flush()


STRATEGIES = [zlib.Z_DEFAULT_STRATEGY, zlib.Z_RLE, zlib.Z_HUFFMAN_ONLY, zlib.Z_FIXED]


@pytest.mark.parametrize("level", [1, 6, 9])
@pytest.mark.parametrize("strategy", STRATEGIES)
def test_inflater_matches_zlib(level, strategy):
	rng = np.random.default_rng(level * 10 + strategy)
	inputs = [b"", b"A", a2m_like(1, 3000), rng.integers(0, 256, 5000, dtype=np.uint8).tobytes(),
		(b"the quick brown fox jumps over the lazy dog " * 500)]
	big = a2m_like(2, 400000, gap_p=0.1, mean_gap=50) + rng.integers(0, 256, 60000, dtype=np.uint8).tobytes() + b"xy" * 30000
	inputs.append(big)
	for data in inputs:
		raw = _zlib(data, level, strategy)
		blocks = D.inflate_tokens(raw)
		assert D.detokenize(blocks) == zlib.decompress(raw, -15) == data
		assert blocks[-1]["final"] and not any(b["final"] for b in blocks[:-1])
	assert len(D.inflate_tokens(_zlib(big, level, strategy))) > 1, "a multi-block stream"


class _BitWriter:
	def __init__(self):
		self.bits = []

	def put(self, v, n):
		self.bits += [(v >> i) & 1 for i in range(n)]

	def bytes(self):
		return np.packbits(np.array(self.bits + [0] * (-len(self.bits) % 8), np.uint8), bitorder="little").tobytes()


def _dynamic_header(cl_lengths_in_order):
	w = _BitWriter()
	w.put(1 | (2 << 1), 3)
	w.put(0, 5)
	w.put(0, 5)
	w.put(len(cl_lengths_in_order) - 4, 4)
	for l in cl_lengths_in_order:
		w.put(l, 3)
	w.put(0, 64)
	return w.bytes()


def test_inflater_rejects_bad_codes():
	with pytest.raises(D.DeflateError, match="over-subscribed"):
		D.inflate_tokens(_dynamic_header([1, 1, 1, 1]))   # code-length symbols 16, 17, 18, 0 all of one bit
	with pytest.raises(D.DeflateError, match="incomplete"):
		D.inflate_tokens(_dynamic_header([2, 0, 0, 2]))   # two codes of two bits
	# a model member whose one distance code (length 1) is the code's only one is accepted, as RFC 1951 and zlib accept it
	blocks = D.inflate_tokens(D.member_payload(D.encode_member(b"A" * 1000)))
	assert blocks[0]["btype"] == 2 and blocks[0]["hdist"] == 1 and blocks[0]["dist_lengths"] == [1]
	# and a literal/length code of lengths the model made incomplete is refused
	pl = D.Plan(b"ACGT" * 300)
	good = pl.deflate()
	assert D.detokenize(D.inflate_tokens(good)) == b"ACGT" * 300
	i = pl.lit_len.index(max(pl.lit_len))
	pl.lit_len[i] += 1   # that symbol's code one bit longer: Kraft sum < 1
	pl.cl_seq = pl.lit_len[:pl.n_lit] + [1]
	pl.cl_tokens = D.code_length_tokens(pl.cl_seq)
	pl.cl_freq = [0] * 19
	for s, _ in pl.cl_tokens:
		pl.cl_freq[s] += 1
	pl.cl_len = D.huffman_lengths(pl.cl_freq, 7)
	pl.n_cl = 19
	pl.header_bits = 3 + 5 + 5 + 4 + 3 * 19 + sum(pl.cl_len[s] + {16: 2, 17: 3, 18: 7}.get(s, 0) for s, _ in pl.cl_tokens)
	lit = np.array(pl.lit_len + [0, 0])
	pl.token_bits = int((lit[pl.sym] + D._LEN_EB[pl.mlen] + (pl.mlen > 0)).sum())
	pl.data_bits = pl.header_bits + pl.token_bits + pl.lit_len[256]
	with pytest.raises(D.DeflateError, match="incomplete"):
		D.inflate_tokens(pl.deflate())


# ---- the tokenizer against zlib's Z_RLE ------------------------------------------------------------------

def _edge_inputs():
	out = [(name, d) for name, d in size_pieces()]
	out += [(name, d) for name, d, _ in segment_edge_pieces()[::7]]
	out += [(name, d) for name, d in byte_value_pieces()[1:4]]
	return out


def _assert_rle_tokens_match_zlib(name, data):
	blocks = D.inflate_tokens(_zlib(data, 6, zlib.Z_RLE))
	if any(b["btype"] == 0 for b in blocks):
		pytest.fail("%s: zlib stored it; its tokens are not visible" % name)
	assert D.tokens_of(blocks) == D.rle_tokens(data), name


def test_tokens_match_zlib_rle_at_edge_shapes():
	for name, data in _edge_inputs():
		_assert_rle_tokens_match_zlib(name, data)


def test_tokens_match_zlib_rle_on_random_pieces():
	for seed in range(200):
		rng = random.Random(seed)
		n = rng.randint(1, 8000)
		_assert_rle_tokens_match_zlib("seed %d" % seed, a2m_like(seed, n, gap_p=rng.choice([0.02, 0.3, 1.0]), mean_gap=rng.choice([2, 20, 300])))


def test_vectorized_tokens_are_the_rle_tokens():
	for name, data in _edge_inputs()[::3] + random_pieces(8):
		pl = D.Plan(data)
		toks = [("lit", int(s)) if m == 0 else ("match", int(m), 1) for s, m in zip(pl.sym, pl.mlen)]
		assert toks == D.rle_tokens(data), name


# ---- decoders accept the model's members ---------------------------------------------------------------

def _decoders_accept(data):
	out = D.encode(data)
	assert gzip.decompress(out + EOF_MEMBER) == data
	members = bgzf_members(out)
	assert b"".join(p for _, p in members) == data
	for m, p in members:
		assert D.detokenize(D.inflate_tokens(D.member_payload(m))) == p
	if shutil.which("gzip"):
		r = subprocess.run([shutil.which("gzip"), "-dc"], input=out + EOF_MEMBER, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=60)
		assert r.returncode == 0 and r.stdout == data, r.stderr
	return members


def test_decoders_accept_the_model():
	assert D.encode(b"") == b""
	for name, data in size_pieces() + byte_value_pieces()[:4] + random_pieces(8) + [("fib", fibonacci_piece()), ("cl", cl_limit_piece())]:
		_decoders_accept(data)
	_decoders_accept(b"".join(d for _, d, _ in segment_edge_pieces()[:3]))
	_decoders_accept(b"".join(d for _, d, _ in tie_sweep()))


def test_member_sizes_and_framing():
	for n in SIZES:
		members = bgzf_members(D.encode(a2m_like(n, n)))
		assert [len(p) for _, p in members] == [min(PIECE, n - i) for i in range(0, n, PIECE)]


# ---- the Huffman builder -----------------------------------------------------------------------------

def _kraft(lengths, limit):
	return sum(1 << (limit - l) for l in lengths if l)


@pytest.mark.parametrize("limit,nsym", [(15, 286), (7, 19)])
def test_huffman_lengths(limit, nsym):
	rng = np.random.default_rng(limit)
	reached = unlimited = 0
	for trial in range(400):
		kind = trial % 4
		if kind == 0:
			freq = rng.integers(0, 3, nsym) * rng.integers(1, 1000, nsym)
		elif kind == 1:
			freq = (rng.geometric(0.3, nsym) ** 3) * (rng.random(nsym) < 0.5)
		elif kind == 2:
			k = int(rng.integers(2, min(nsym, 26)))
			fib = [1, 1]
			while len(fib) < k:
				fib.append(fib[-1] + fib[-2])
			freq = np.zeros(nsym, np.int64)
			freq[rng.choice(nsym, k, replace=False)] = fib
		else:
			freq = np.zeros(nsym, np.int64)
			freq[rng.choice(nsym, int(rng.integers(0, 3)), replace=False)] = rng.integers(1, 65000)
		freq = [int(f) for f in freq]
		lens = D.huffman_lengths(freq, limit)
		assert max(lens) <= limit
		assert _kraft(lens, limit) == 1 << limit, "complete"
		assert all(l for f, l in zip(freq, lens) if f), "every used symbol has a code"
		assert sum(1 for l in lens if l) == max(2, sum(1 for f in freq if f))
		by_freq = sorted(((f, s) for s, f in enumerate(freq) if f), reverse=True)
		assert all(lens[a] <= lens[b] for (_, a), (_, b) in zip(by_freq, by_freq[1:])), "longer codes only for rarer symbols"
		if max(D.unlimited_lengths(freq).values()) <= limit:
			unlimited += 1
			if sum(1 for f in freq if f) >= 2:
				assert sum(f * l for f, l in zip(freq, lens)) == D.huffman_optimum(freq)
		else:
			reached += 1
			assert sum(f * l for f, l in zip(freq, lens)) > D.huffman_optimum(freq)
	assert reached > 10 and unlimited > 100


def test_canonical_codes_are_prefix_free():
	for freq in ([5, 0, 3, 3, 1, 1, 9] + [0] * 12, D.Plan(a2m_like(3, 20000)).freq):
		lens = D.huffman_lengths(freq, 15)
		codes = D._canonical(lens)
		words = sorted(bin(c)[2:].zfill(l) for _, c, l in codes)
		assert all(not b.startswith(a) for a, b in zip(words, words[1:]))


# ---- the edge inputs do what they are there for --------------------------------------------------------

def test_segment_edge_pieces_plant_what_they_say():
	cases = set()
	pieces = segment_edge_pieces()
	for name, piece, planted in pieces:
		assert len(piece) == PIECE
		starts, lens, _ = D.runs(piece)
		run_at = dict(zip(starts.tolist(), lens.tolist()))
		for j, (s, l) in enumerate(planted):
			assert run_at.get(s) == l, (name, s, l)
			if name.startswith("segment"):
				cases.add((SEG * (2 + 4 * j) - s, l))   # the j-th run is planted at the edge of segment 2 + 4 j
	assert cases == {(o, l) for o in range(258) for l in EDGE_RUN_LENGTHS}
	_, piece, spans = pieces[-1]
	starts, _, _ = D.runs(piece)
	assert starts[0] == 0 and starts[-1] == PIECE - 700
	no_start = set(range(PIECE // SEG)) - set((starts // SEG).tolist())
	assert len(no_start) >= 20, "segments that a run covers whole"


def test_byte_value_pieces():
	pieces = dict(byte_value_pieces())
	for name in ("iid", "skewed"):
		assert len(set(pieces[name])) == 256
	assert D.Plan(pieces["iid"]).stored and not D.Plan(pieces["skewed"]).stored
	for name in ("all 0x00", "all 0xff"):
		pl = D.Plan(pieces[name])
		assert not pl.stored and sum(1 for f in pl.freq if f) == 4, "the byte, matches of 258 and 5 (65 279 = 253 * 258 + 5), end of block"
	for b in range(256):
		pl = D.Plan(pieces["one byte %d" % b])
		assert pl.freq[b] == 1 and pl.freq[256] == 1 and sum(pl.freq) == 2 and pl.stored


def test_fibonacci_piece_needs_the_15_bit_limit():
	pl = D.Plan(fibonacci_piece())
	assert not pl.mlen.any(), "literals only"
	assert max(D.unlimited_lengths(pl.freq).values()) > 15
	assert max(pl.lit_len) == 15 and not pl.stored


def test_cl_limit_piece_needs_the_7_bit_limit():
	pl = D.Plan(cl_limit_piece())
	assert not pl.mlen.any(), "literals only"
	assert pl.lit_len[:256] == cl_limit_lengths() and pl.lit_len[256] == 15, "dyadic frequencies give exactly these lengths"
	assert max(D.unlimited_lengths(pl.cl_freq).values()) > 7
	assert max(pl.cl_len) == 7 and not pl.stored
	assert _kraft(pl.cl_len, 7) == 1 << 7


def test_tie_sweep_reaches_the_tie_from_both_sides():
	diffs = [d for _, _, d in tie_sweep()]
	assert 0 in diffs and min(diffs) < 0 < max(diffs)
	for r, piece, d in tie_sweep():
		pl = D.Plan(piece)
		assert pl.stored == (d <= 0)
		m = D.encode_member(piece)
		assert (m[18] & 7 == 1) == pl.stored and len(m) == min(pl.stored_bytes, pl.dynamic_bytes)


def test_random_pieces():
	sizes = [len(d) for _, d in random_pieces()]
	assert PIECE in sizes and min(sizes) < 4000 and len(set(sizes)) > 32


# ---- the exactness check sees what the old checks do not -----------------------------------------------

def test_a_valid_but_different_encoding_passes_the_old_checks_only():
	"""One 258-match that crosses a segment edge re-split as 257 + a literal: gzip.decompress gives the piece back and the payload
	stays within 1.02 x zlib's (the checks test_gpu_bgzf.py had), but the member is not the model's, which the exact check sees."""
	_, piece, _ = segment_edge_pieces()[50]
	toks = D.rle_tokens(piece)
	pos, alt = 0, None
	for i, t in enumerate(toks):
		n = 1 if t[0] == "lit" else t[1]
		if t[:2] == ("match", 258) and pos // SEG != (pos + n - 1) // SEG:
			b = piece[pos - 1]
			alt = toks[:i] + [("match", 257, 1), ("lit", b)] + toks[i + 1:]
			break
		pos += n
	assert alt is not None
	pl = D.Plan(piece, tokens=alt)
	assert not pl.stored
	member = pl.member()
	assert gzip.decompress(member + EOF_MEMBER) == piece
	assert len(D.member_payload(member)) <= 1.02 * len(_zlib(piece, 6, zlib.Z_RLE))
	assert member != D.encode_member(piece)
