"""BGZF input inflated on the GPU (v2m_bgzf_decompress, bgzf_inflate_kernel): a zlib corpus, hand-built streams zlib refuses, seeded bit
flips against zlib's verdict, graphs and driver runs from .vcf.gz / .fa.gz against the plain text, and the corpus on the checked build."""

import os
import random
import subprocess
import zlib

import numpy as np
import pytest

from bgzf_input_util import (EOF_MEMBER, BitWriter, bgzf, deflate_raw, fixed_lengths, member, member_accepted, write_dynamic_block,
	write_fixed_block, zlib_inflate)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")
DERIVED = os.path.join(HERE, "golden", "derived")
V2M_ERR_INVALID_ARGUMENT = 1


@pytest.fixture(scope="module")
def ctx():
	import vcf2multialign_amd as v2m
	with v2m.Context(0) as c:
		yield c


def vcf_like(n, seed=1):
	rng = random.Random(seed)
	lines, i = [], 0
	while sum(map(len, lines)) < n:
		lines.append("1\t%d\trs%d\tA\tG\t.\tPASS\t.\tGT\t%s\n" % (100 + 7 * i, i, "\t".join(rng.choice(["0|0"] * 6 + ["0|1", "1|0", "1|1"]) for _ in range(40))))
		i += 1
	return "".join(lines).encode()[:n]


def a2m_like(n, seed=2):
	rng = np.random.default_rng(seed)
	body = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)]
	body[rng.random(n) < 0.3] = ord("-")
	body[::61] = ord("\n")
	return body.tobytes()


KINDS = {
	"vcf": lambda n: vcf_like(n),
	"iid": lambda n: np.random.default_rng(3).integers(0, 256, n, dtype=np.uint8).tobytes(),
	"one byte": lambda n: b"G" * n,
	"a2m": lambda n: a2m_like(n),
	"0..255": lambda n: bytes(range(256)) * (n // 256) + bytes(range(n % 256)),
}


def check(ctx, data, **kw):
	f = bgzf(data, **kw)
	assert ctx.bgzf_decompress(f) == data


@pytest.mark.parametrize("strategy", ["default", "filtered", "huffman", "rle", "fixed"])
def test_zlib_levels_and_strategies(ctx, strategy):
	for level in range(10):
		pieces = [KINDS[k](20000 + 37 * level) for k in KINDS]
		f = b"".join(bgzf(p, eof=False, level=level, strategy=strategy) for p in pieces) + EOF_MEMBER
		assert ctx.bgzf_decompress(f) == b"".join(pieces), (strategy, level)


@pytest.mark.parametrize("piece", [0, 1, 2, 257, 258, 259, 32768, 32769, 65280, 65536])
def test_piece_sizes(ctx, piece):
	data = vcf_like(3 * max(piece, 1) + 11)
	if piece == 0:
		assert ctx.bgzf_decompress(bgzf(b"", piece=0)) == b""
		return
	check(ctx, data, piece=piece)
	if piece <= 65280:
		rnd = KINDS["iid"](2 * piece + 5)
		for level in (0, 6):
			check(ctx, rnd, piece=piece, level=level)


def test_many_blocks_and_flushes(ctx):
	data = vcf_like(65280) + a2m_like(65280)
	check(ctx, data, mem_level=1)                                   # a small buffer: many blocks per member
	for mode in (zlib.Z_SYNC_FLUSH, zlib.Z_FULL_FLUSH):             # empty stored blocks inside a member
		for at in (1, 1000, 40000):
			check(ctx, data, flush_at=at, flush_mode=mode)
			check(ctx, data, flush_at=at, flush_mode=mode, strategy="fixed")


def test_long_distances_and_matches(ctx):
	rng = np.random.default_rng(7)
	head = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
	data = head + head[:20000] + b"x" * 1000                      # a repeat exactly 32 768 bytes back, 258-byte matches
	check(ctx, data, piece=65280)
	# by hand: a match at distance 32 768 and 258-byte matches with distances 1, 2, 63, 64, 65
	w = BitWriter()
	lit, dist = fixed_lengths()
	w.put(0, 1); w.put(0, 2); w.align(); w.put(32768 & 0xffff, 16); w.put(~32768 & 0xffff, 16)
	w.raw(head[:32768])                                             # (stored LEN 32 768)
	toks = [("match", 258, 32768)] + [t for d in (1, 2, 63, 64, 65) for t in (("match", 258, d),)] + [256]
	write_fixed_block(w, toks)
	payload = w.bytes()
	out = zlib_inflate(payload)
	assert out is not None and len(out) == 32768 + 6 * 258
	assert ctx.bgzf_decompress(member(payload, out)) == out


def test_own_encoder_round_trip(ctx):
	import vcf2multialign_amd as v2m
	for data in (vcf_like(300000), a2m_like(200000), b"A" * 70000, KINDS["iid"](100000), b"Z"):
		assert ctx.bgzf_decompress(ctx.bgzf_compress(data)) == data
		assert ctx.bgzf_decompress(v2m.bgzf_frame_stored(data) + EOF_MEMBER) == data


def test_many_slices(ctx, monkeypatch):
	data = vcf_like(3_000_000) + a2m_like(1_000_000)
	f = bgzf(data, piece=40000)
	monkeypatch.setenv("V2M_RING_SLOT_BYTES", "100000")               # two or three members per slice
	assert ctx.bgzf_decompress(f) == data
	monkeypatch.setenv("V2M_RING_SLOT_BYTES", "1")                    # one member per slice
	assert ctx.bgzf_decompress(bgzf(data[:400000], piece=40000)) == data[:400000]


def test_profile_counts_launches(ctx, monkeypatch):
	import vcf2multialign_amd as v2m
	data = vcf_like(500000)
	monkeypatch.setenv("V2M_RING_SLOT_BYTES", "200000")
	ctx.profile_enable(True)
	ctx.profile_reset()
	try:
		assert ctx.bgzf_decompress(bgzf(data)) == data
		n, ms = ctx.profile_get(v2m._native.KERNEL_INFLATE)
	finally:
		ctx.profile_enable(False)
	assert n == 3 and ms > 0                                        # 9 members (8 + EOF), 3 per slice of 200 000 output bytes


# ---- hand-built streams ------------------------------------------------------------------------

def lens_of(n, pairs):
	out = [0] * n
	for s, L in pairs.items():
		out[s] = L
	return out


def dyn(lit_pairs, dist_pairs, tokens, n_lit=258, n_dist=1, **kw):
	w = BitWriter()
	write_dynamic_block(w, lens_of(n_lit, lit_pairs), lens_of(n_dist, dist_pairs), tokens, **kw)
	return w.bytes()


def fixed(tokens):
	w = BitWriter()
	write_fixed_block(w, tokens)
	return w.bytes()


A, B = ord("a"), ord("b")
GOOD_LIT = {256: 2, A: 2, B: 2, 257: 2}                             # complete
CL_REPEAT_FIRST = [(16, 0)]


def bad_streams():
	"""(name, payload, data the member claims) of streams zlib refuses."""
	c = {}
	w = BitWriter(); w.put(1, 1); w.put(3, 2); c["block type 3"] = w.bytes()
	w = BitWriter(); w.put(1, 1); w.put(0, 2); w.align(); w.put(5, 16); w.put(0, 16); w.raw(b"hello"); c["LEN != ~NLEN"] = w.bytes()
	c["HLIT > 286"] = dyn(GOOD_LIT, {0: 1}, [A, 256], n_lit=287)
	c["HDIST > 30"] = dyn(GOOD_LIT, {0: 1}, [A, 256], n_dist=31)
	c["over-subscribed literal/length code"] = dyn({256: 1, A: 1, B: 1}, {0: 1}, [])
	c["incomplete literal/length code"] = dyn({256: 2, A: 2}, {0: 1}, [])
	c["over-subscribed distance code"] = dyn(GOOD_LIT, {0: 1, 1: 1, 2: 1}, [], n_dist=3)
	c["incomplete distance code"] = dyn(GOOD_LIT, {0: 2, 1: 2}, [], n_dist=2)
	cl_inc = [0] * 19; cl_inc[1] = 1; cl_inc[2] = 2; cl_inc[0] = 3
	c["incomplete code-length code"] = dyn({256: 1}, {0: 1}, [], cl_lens=cl_inc, cl_seq=[(0, 0)] * 256 + [(1, 0), (1, 0)])
	cl_over = [0] * 19; cl_over[0] = 1; cl_over[1] = 1; cl_over[2] = 1
	c["over-subscribed code-length code"] = dyn({256: 1}, {0: 1}, [], cl_lens=cl_over, cl_seq=[(0, 0)] * 256 + [(1, 0), (1, 0)])
	c["no code-length codes"] = dyn({256: 1}, {0: 1}, [], cl_lens=[0] * 19, cl_seq=[])
	c["no end-of-block code"] = dyn({A: 1, B: 1}, {0: 1}, [], n_lit=257)
	c["repeat with no previous length"] = dyn(GOOD_LIT, {0: 1}, [], cl_seq=CL_REPEAT_FIRST)
	c["repeat past HLIT + HDIST"] = dyn({256: 1}, {0: 1}, [], cl_seq=[(18, 127), (18, 127), (1, 0), (16, 3)])
	c["literal/length symbol 286"] = fixed([A, 286])
	c["literal/length symbol 287"] = fixed([A, 287])
	c["distance symbol 30"] = fixed([A, ("dsym", 3, 30)])
	c["distance symbol 31"] = fixed([A, ("dsym", 3, 31)])
	c["distance too far back"] = fixed([A, ("match", 3, 2), 256])
	c["distance with no distance codes"] = dyn(GOOD_LIT, {}, [A, 257, ("bits", 0, 1), 256])
	c["unused half of a one-code distance code"] = dyn(GOOD_LIT, {0: 1}, [A, 257, ("bits", 1, 1), 256])
	w = BitWriter(); w.put(0, 1); w.put(1, 2); w.code(0, 7); c["no final block"] = w.bytes()   # a fixed block that is not the last, then nothing
	return c


def test_streams_zlib_refuses(ctx):
	import vcf2multialign_amd as v2m
	prefix = bgzf(vcf_like(1000), eof=False)
	for name, payload in bad_streams().items():
		assert zlib_inflate(payload) is None, name                # the construction is what it claims
		data = b"a" * 10
		f = prefix + member(payload, data) + EOF_MEMBER
		with pytest.raises(v2m.V2MError) as e:
			ctx.bgzf_decompress(f)
		assert e.value.code == V2M_ERR_INVALID_ARGUMENT, (name, str(e.value))
		assert "compressed offset %d" % len(prefix) in str(e.value), (name, str(e.value))


def test_streams_zlib_accepts(ctx):
	"""Edge cases zlib accepts: a single code of length 1 (literal/length and distance), bytes after the final block, a
	code-length sequence with all three repeat codes."""
	cases = {
		"one-code literal/length code": dyn({256: 1}, {}, [256]),
		"one-code distance code": dyn(GOOD_LIT, {0: 1}, [A, ("match", 3, 1), B, 256], n_dist=1),
		"bytes after the final block": fixed([A, B, 256]) + b"\x00\x55\xaa",
		# lengths 3 for 'a'..'f', 256 and 257: 97 zeros (18), 3 then 5 repeats (16), 153 zeros (18, 17, 17), 3, 3, then the distance code's 1
		"repeat codes": dyn({**{s: 3 for s in range(97, 103)}, 256: 3, 257: 3}, {0: 1}, [A, ("match", 3, 1), 256],
			cl_seq=[(18, 97 - 11), (3, 0), (16, 5 - 3), (18, 138 - 11), (17, 10 - 3), (17, 5 - 3), (3, 0), (3, 0), (1, 0)]),
	}
	for name, payload in cases.items():
		out = zlib_inflate(payload)
		assert out is not None, name
		assert ctx.bgzf_decompress(member(payload, out) + EOF_MEMBER) == out, name


def test_crc_and_isize_mismatches(ctx):
	import vcf2multialign_amd as v2m
	data = vcf_like(5000)
	payload = deflate_raw(data)
	for name, m in {"flipped CRC": member(payload, data, crc=zlib.crc32(data) ^ 1), "ISIZE + 1": member(payload, data, isize=len(data) + 1),
			"ISIZE - 1": member(payload, data, isize=len(data) - 1), "payload cut": member(payload[:-1], data)}.items():
		with pytest.raises(v2m.V2MError) as e:
			ctx.bgzf_decompress(bgzf(b"x" * 100, eof=False) + m)
		assert e.value.code == V2M_ERR_INVALID_ARGUMENT and "compressed offset" in str(e.value), (name, str(e.value))


def test_seeded_bit_flips_match_zlib(ctx):
	import vcf2multialign_amd as v2m
	rng = random.Random(20261016)
	sources = [vcf_like(3000, seed=5), a2m_like(2000), b"AAAACCCGGT" * 200, KINDS["0..255"](1500)]
	refused = 0
	for k in range(64):
		data = sources[k % len(sources)]
		m = bytearray(member(deflate_raw(data, level=rng.choice([1, 6, 9]), strategy=rng.choice(["default", "fixed", "huffman", "rle"])), data))
		bit = rng.randrange(8 * (len(m) - 26))
		m[18 + bit // 8] ^= 1 << (bit % 8)
		want = member_accepted(bytes(m))
		if want is None:
			refused += 1
			with pytest.raises(v2m.V2MError) as e:
				ctx.bgzf_decompress(bytes(m))
			assert e.value.code == V2M_ERR_INVALID_ARGUMENT, k
		else:
			assert ctx.bgzf_decompress(bytes(m)) == want, k
	assert refused > 32


# ---- graphs and the driver ---------------------------------------------------------------------

FIXTURES = [("test-1a", "test-1.fa"), ("test-1b", "test-1.fa"), ("test-2", "test-2.fa"), ("test-3", "test-3.fa"), ("test-4", "test-4.fa")]


def gz_copy(src, dst, piece=65280):
	with open(src, "rb") as f:
		data = f.read()
	with open(dst, "wb") as f:
		f.write(bgzf(data, piece=piece))
	return str(dst)


def graph_arrays(g):
	return dict(ref=g.ref, rp=g.reference_positions.tolist(), ap=g.aligned_positions.tolist(), tg=g.alt_edge_targets.tolist(), cs=g.alt_edge_count_csum.tolist(),
		lo=g.label_offsets.tolist(), lb=g.label_bytes, sn=g.sample_names, pc=g.ploidy_csum.tolist(), pdims=g.paths_by_edge_and_chrom_copy_dims,
		paths=g.paths_by_edge_and_chrom_copy.tobytes(), hv=g.handled_variants, cm=g.chr_id_mismatches, ov=g.overlaps)


def test_graphs_from_bgzf_equal_plain(ctx, tmp_path):
	from vcf2multialign_amd import host
	for stem, fasta in FIXTURES:
		fa, vcf = os.path.join(FIX, fasta), os.path.join(FIX, stem + ".vcf")
		fa_gz, vcf_gz = gz_copy(fa, tmp_path / (fasta + ".gz"), piece=7), gz_copy(vcf, tmp_path / (stem + ".vcf.gz"), piece=100)
		assert graph_arrays(host.HostGraph(fa_gz, vcf_gz, "1", ctx=ctx)) == graph_arrays(host.HostGraph(fa, vcf, "1")), stem
		assert graph_arrays(host.HostGraph(fa, vcf_gz, "1", ctx=ctx)) == graph_arrays(host.HostGraph(fa, vcf, "1", ctx=ctx)), stem


def test_graph_mini3_and_error_line_numbers(ctx, tmp_path):
	from vcf2multialign_amd import synth
	from vcf2multialign_amd import host
	ds = synth.dataset("mini3")
	fa, vcf = tmp_path / "m.fa", tmp_path / "m.vcf"
	ds.write_fasta_and_vcf(fa, vcf)
	fa_gz, vcf_gz = gz_copy(fa, tmp_path / "m.fa.gz"), gz_copy(vcf, tmp_path / "m.vcf.gz")
	assert graph_arrays(host.HostGraph(fa_gz, vcf_gz, "1", ctx=ctx)) == graph_arrays(host.HostGraph(str(fa), str(vcf), "1"))
	lines = open(vcf, "rb").read().split(b"\n")
	k = len(lines) * 3 // 4
	lines[k] = lines[k].replace(b"\t0|0", b"\t0|", 1)                 # an empty GT allele deep inside
	bad, bad_gz = tmp_path / "bad.vcf", tmp_path / "bad.vcf.gz"
	bad.write_bytes(b"\n".join(lines))
	gz_copy(bad, bad_gz)
	with pytest.raises(ValueError) as plain:
		host.HostGraph(str(fa), str(bad), "1")
	with pytest.raises(ValueError) as comp:
		host.HostGraph(fa_gz, str(bad_gz), "1", ctx=ctx)
	assert str(plain.value) == str(comp.value) == "VCF line %d: empty GT allele" % (k + 1)


def run(args, check=True):
	assert os.path.exists(CLI), "build the host driver first (__graft_entry__.build())"
	r = subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
	if check:
		assert r.returncode == 0, r.stderr.decode()
	return r


def test_cli_fixtures_from_bgzf(tmp_path):
	for stem, fasta in FIXTURES:
		fa_gz, vcf_gz = gz_copy(os.path.join(FIX, fasta), tmp_path / "r.fa.gz"), gz_copy(os.path.join(FIX, stem + ".vcf"), tmp_path / "v.vcf.gz", piece=64)
		out = tmp_path / "out.a2m"
		common = ["-H", "-r", fa_gz, "-a", vcf_gz, "-c", "1"]
		r = run(common + ["-s", str(out), "--verbose"])
		assert out.read_bytes() == open(os.path.join(DERIVED, stem + ".haplotypes.a2m"), "rb").read(), stem
		assert b"members" in r.stderr and b"inflated on the GPU" in r.stderr and b"WARNING" not in r.stderr
		run(common + ["-s", str(out), "--unaligned"])
		assert out.read_bytes() == open(os.path.join(DERIVED, stem + ".haplotypes.unaligned.fa"), "rb").read(), stem
		plain = ["-H", "-r", os.path.join(FIX, fasta), "-a", os.path.join(FIX, stem + ".vcf"), "-c", "1"]
		run(common + ["-s", str(out), "--output-overlaps=" + str(tmp_path / "gz.tsv")])
		run(plain + ["-s", str(tmp_path / "p.a2m"), "--output-overlaps=" + str(tmp_path / "plain.tsv")])
		assert (tmp_path / "gz.tsv").read_bytes() == (tmp_path / "plain.tsv").read_bytes(), stem


def test_cli_founders_from_bgzf(tmp_path):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	fa_gz, vcf_gz = gz_copy(fa, tmp_path / "r.fa.gz"), gz_copy(vcf, tmp_path / "v.vcf.gz", piece=50)
	run(["-F", "2", "-r", fa_gz, "-a", vcf_gz, "-c", "1", "-s", str(tmp_path / "gz.a2m")])
	run(["-F", "2", "-r", fa, "-a", vcf, "-c", "1", "-s", str(tmp_path / "plain.a2m")])
	assert (tmp_path / "gz.a2m").read_bytes() == (tmp_path / "plain.a2m").read_bytes()


def test_cli_warns_without_eof_member(tmp_path):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	vcf_gz = tmp_path / "v.vcf.gz"
	vcf_gz.write_bytes(bgzf(open(vcf, "rb").read(), eof=False))
	r = run(["-H", "-r", fa, "-a", str(vcf_gz), "-c", "1", "-s", str(tmp_path / "o.a2m")])
	assert b"does not end with the BGZF EOF member" in r.stderr
	assert (tmp_path / "o.a2m").read_bytes() == open(os.path.join(DERIVED, "test-4.haplotypes.a2m"), "rb").read()


def _compress_piece(args):
	data, = args
	return member(deflate_raw(data, level=6), data)


def bgzf_pool(path_in, path_out, processes=16):
	"""bgzip's layout (65 280-byte pieces, zlib level 6, the EOF member) by a pool of processes."""
	import multiprocessing as mp
	data = open(path_in, "rb").read()
	pieces = [(data[i:i + 65280],) for i in range(0, len(data), 65280)]
	with mp.get_context("spawn").Pool(processes) as pool, open(path_out, "wb") as f:
		for m in pool.imap(_compress_piece, pieces, chunksize=64):
			f.write(m)
		f.write(EOF_MEMBER)
	return str(path_out)


def test_cli_config2_full_size(tmp_path):
	from vcf2multialign_amd import synth
	ds = synth.dataset("config2")
	fa, vcf = tmp_path / "c2.fa", tmp_path / "c2.vcf"
	ds.write_fasta_and_vcf(fa, vcf)
	vcf_gz = bgzf_pool(vcf, tmp_path / "c2.vcf.gz")
	for src, tag in ((str(vcf), "plain"), (vcf_gz, "gz")):
		run(["-H", "-r", str(fa), "-a", src, "-c", "1", "-f", str(tmp_path / (tag + ".graph")), "--region=5000000-5001000", "-s", str(tmp_path / (tag + ".a2m"))])
	assert (tmp_path / "gz.graph").read_bytes() == (tmp_path / "plain.graph").read_bytes()
	assert (tmp_path / "gz.a2m").read_bytes() == (tmp_path / "plain.a2m").read_bytes()


# ---- the checked build -------------------------------------------------------------------------

CHECKED_CORPUS = [
	"tests/test_gpu_bgzf_input.py::test_zlib_levels_and_strategies",
	"tests/test_gpu_bgzf_input.py::test_piece_sizes",
	"tests/test_gpu_bgzf_input.py::test_many_blocks_and_flushes",
	"tests/test_gpu_bgzf_input.py::test_long_distances_and_matches",
	"tests/test_gpu_bgzf_input.py::test_many_slices",
	"tests/test_gpu_bgzf_input.py::test_streams_zlib_refuses",
	"tests/test_gpu_bgzf_input.py::test_streams_zlib_accepts",
	"tests/test_gpu_bgzf_input.py::test_crc_and_isize_mismatches",
	"tests/test_gpu_bgzf_input.py::test_seeded_bit_flips_match_zlib",
	"tests/test_gpu_bgzf_input.py::test_graphs_from_bgzf_equal_plain",
]


def test_corpus_on_the_checked_build():
	from test_gpu_checked_build import SEEDS, run_checked_corpus
	from vcf2multialign_amd import build
	assert os.path.exists(build.CHECKED_LIB_PATH) and os.path.exists(build.CHECKED_HOST_LIB_PATH), "build_native() builds them"
	for seed in SEEDS:   # the second seed only once the first has passed
		rc, out = run_checked_corpus(seed, build.CHECKED_LIB_PATH, build.CHECKED_HOST_LIB_PATH, corpus=CHECKED_CORPUS, timeout=600)
		assert rc == 0, "checked build, seed %s: exit %d\n%s" % (seed, rc, out[-6000:])
		assert " passed" in out and "libv2m_host_checked.so" in out, out[-3000:]
