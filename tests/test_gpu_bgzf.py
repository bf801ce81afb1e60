"""The GPU BGZF encoder (V2M_SPLICE_BGZF, v2m_bgzf_compress, --bgzf): every output decompresses, with Python's zlib as the
independent decoder, to exactly the bytes the same call writes without compression."""

import gzip
import os
import random
import subprocess
import zlib

import numpy as np
import pytest

import synth
from test_bgzf_host import EOF_MEMBER, bgzf_members

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")
DERIVED = os.path.join(HERE, "golden", "derived")
PIECE = 65280


@pytest.fixture(scope="module")
def v2m():
	import vcf2multialign_amd as v
	return v


@pytest.fixture(scope="module")
def ctx(v2m):
	c = v2m.Context(0)
	yield c
	c.close()


def _check(v2m, ctx, data):
	out = ctx.bgzf_compress(data)
	assert len(out) <= v2m.bgzf_bound(len(data))
	if not data:
		assert out == b""
		return out, []
	members = bgzf_members(out)
	assert [len(p) for _, p in members] == [min(PIECE, len(data) - i) for i in range(0, len(data), PIECE)]
	assert gzip.decompress(out + EOF_MEMBER) == data
	return out, members


def _zlib_rle_payload(data):
	total = 0
	for i in range(0, len(data), PIECE):
		c = zlib.compressobj(6, zlib.DEFLATED, -15, 9, zlib.Z_RLE)
		total += len(c.compress(data[i:i + PIECE]) + c.flush())
	return total


def _payload(members):
	return sum(len(m) - 26 for m, _ in members)


def _a2m_like(rng, n, gap_p=0.02, mean_gap=20):
	out = bytearray()
	while len(out) < n:
		if rng.random() < gap_p:
			out += b"-" * (1 + int(rng.expovariate(1.0 / mean_gap)))
		else:
			out += bytes(rng.choice(b"ACGT") for _ in range(50))
	return bytes(out[:n])


@pytest.mark.parametrize("n", [0, 1, 2, 3, 4, 258, 259, 65279, PIECE, PIECE + 1, 3 * PIECE + 17])
def test_sizes(v2m, ctx, n):
	rng = random.Random(n)
	_check(v2m, ctx, bytes(rng.choice(b"ACGT-") for _ in range(n)))


def test_iid_bytes_take_the_stored_block(v2m, ctx):
	data = np.random.default_rng(1).integers(0, 256, 3 * PIECE, dtype=np.uint8).tobytes()
	_, members = _check(v2m, ctx, data)
	for m, p in members:
		assert m[18] & 7 == 1 and len(m) == len(p) + 31, "stored: BFINAL, BTYPE 00, one block"


def test_one_byte_runs(v2m, ctx):
	_, members = _check(v2m, ctx, b"A" * 1000000)
	assert all(len(m) < 200 for m, _ in members), "a run of 65 280 is 253 matches of 258"
	_check(v2m, ctx, b"\0" * 70000)


def test_runs_of_every_length(v2m, ctx):
	data = bytearray()
	for n in range(1, 301):
		data += bytes([n & 1 and 0x41 or 0x43]) * n
	for n in range(300, 0, -1):
		data += bytes([(n * 7) & 255]) * n
	_check(v2m, ctx, bytes(data))
	_check(v2m, ctx, bytes(data[PIECE - 1000:]))


def test_runs_across_segment_and_block_ends(v2m, ctx):
	rng = random.Random(5)
	for _ in range(4):
		data = bytearray()
		while len(data) < 2 * PIECE + 999:
			data += bytes([rng.choice(b"AC")]) * rng.choice([1, 2, 3, 4, 255, 256, 257, 258, 259, 260, 515, 516, 517, 1000])
		_check(v2m, ctx, bytes(data))


def test_iid_acgt_ratio(v2m, ctx):
	rng = random.Random(7)
	data = bytes(rng.choice(b"ACGT") for _ in range(4 * PIECE))
	_, members = _check(v2m, ctx, data)
	assert _payload(members) <= 1.02 * _zlib_rle_payload(data)
	assert len(ctx.bgzf_compress(data)) / len(data) < 0.29


def test_a2m_like_ratio(v2m, ctx):
	data = _a2m_like(random.Random(8), 4 * PIECE)
	_, members = _check(v2m, ctx, data)
	assert _payload(members) <= 1.02 * _zlib_rle_payload(data)


def test_fibonacci_frequencies_force_the_length_limit(v2m, ctx):
	"""Symbol frequencies 1, 1, 2, 3, 5, 8, ... over 22 symbols: an unlimited Huffman code would need 21-bit codes."""
	fib = [1, 1]
	while len(fib) < 22:
		fib.append(fib[-1] + fib[-2])
	counts = [f * PIECE // sum(fib) + 1 for f in fib]   # scaled into one block, every symbol kept
	syms = bytearray()
	for i, c in enumerate(counts):
		syms += bytes([65 + i]) * c
	rng = random.Random(9)
	block = bytearray(syms[:PIECE])
	rng.shuffle(block)
	# shuffled symbols rarely repeat, so they are literals and their counts are the frequencies
	_check(v2m, ctx, bytes(block))
	# and the exact sequence 1, 1, 2, 3, ..., as isolated literals between separators
	lit = bytearray()
	for i, f in enumerate(fib[:16]):
		lit += bytes([65 + i, 10]) * f
	_check(v2m, ctx, bytes(lit[:PIECE]))


def test_a2m_rows_in_many_pieces(v2m, ctx):
	for seed in range(3):
		data = _a2m_like(random.Random(100 + seed), 5 * PIECE + seed * 12345, gap_p=0.05, mean_gap=300)
		_check(v2m, ctx, data)


def _upload(v2m, ctx, g):
	vg = v2m.VariantGraph.from_object(g)
	ctx.upload_graph(vg, g.ref)


def _rows_match(v2m, ctx, rows, unaligned):
	plain = ctx.splice_rows(rows, unaligned=unaligned)
	packed = ctx.splice_rows(rows, unaligned=unaligned, bgzf=True)
	assert len(packed) == len(plain)
	for i, (body, members) in enumerate(zip(plain, packed)):
		if not body:
			assert members == b""
			continue
		assert len(bgzf_members(members)) == -(-len(body) // PIECE)
		assert gzip.decompress(members) == body, "row %d" % i


def test_fixture_rows(v2m, ctx):
	import oracle
	for stem, fasta in [("test-1a", "test-1.fa"), ("test-2", "test-2.fa"), ("test-3", "test-3.fa"), ("test-4", "test-4.fa")]:
		g = oracle.build_variant_graph(os.path.join(FIX, fasta), os.path.join(FIX, stem + ".vcf"), "1")
		_upload(v2m, ctx, g)
		rows = [v2m.PLOIDY_MAX] + list(range(g.total_chromosome_copies))
		for unaligned in (False, True):
			_rows_match(v2m, ctx, rows, unaligned)


@pytest.mark.parametrize("small_slices", [False, True])
def test_synthetic_rows(v2m, ctx, tmp_path, monkeypatch, small_slices):
	if small_slices:
		monkeypatch.setenv("V2M_RING_SLOT_BYTES", "300000")   # a few rows per slice: many slices, both halves of the ring reused
	for seed, ref_len, n_var, n_samples, kw in [(31, 200000, 3000, 6, {}), (32, 90000, 1500, 8, {"long_every": 40}), (33, 30000, 500, 20, {"ploidy": 1})]:
		g = synth.build_case(tmp_path, seed, ref_len, n_var, n_samples, **kw)
		_upload(v2m, ctx, g)
		rows = [v2m.PLOIDY_MAX] + list(range(g.total_chromosome_copies))
		for unaligned in (False, True):
			_rows_match(v2m, ctx, rows, unaligned)


def test_flag_is_refused_where_unsupported(v2m, ctx, tmp_path):
	import ctypes as C
	from vcf2multialign_amd import _native as N
	g = synth.build_case(tmp_path, 34, 20000, 100, 2)
	_upload(v2m, ctx, g)
	rows = v2m.RowBatch([v2m.PLOIDY_MAX, 0])
	lib = v2m.load_library()
	cb = N.HOLD_SINK_FN(lambda *a: 0)
	assert lib.v2m_splice_rows_held(ctx._h, C.byref(rows.struct), N.V2M_SPLICE_BGZF, 2, cb, None) == N.V2M_ERR_UNSUPPORTED
	assert lib.v2m_splice_rows_device(ctx._h, C.byref(rows.struct), N.V2M_SPLICE_BGZF, None, 0, None) == N.V2M_ERR_INVALID_ARGUMENT
	assert lib.v2m_splice_rows(ctx._h, C.byref(rows.struct), 0x4, N.SINK_FN(lambda *a: 0), None) == N.V2M_ERR_INVALID_ARGUMENT


def test_profiled_as_one_kernel_id(v2m, ctx):
	ctx.profile_reset()
	ctx.profile_enable(True)
	try:
		ctx.bgzf_compress(b"ACGT" * 50000)
		n, ms = ctx.profile_get(v2m._native.KERNEL_BGZF)
	finally:
		ctx.profile_enable(False)
	assert n == 1 and ms > 0


def test_python_output_writes_bgzf(v2m, ctx):
	import io
	import oracle
	g = oracle.build_variant_graph(os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf"), "1")
	vg = v2m.VariantGraph.from_object(g)
	ctx.upload_graph(vg, g.ref)
	out = io.BytesIO()
	v2m.HaplotypeOutput(ctx, bgzf=True).output_a2m(vg, out)
	assert out.getvalue().endswith(EOF_MEMBER)
	assert gzip.decompress(out.getvalue()) == open(os.path.join(DERIVED, "test-4.haplotypes.a2m"), "rb").read()


def _run(args):
	return subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


@pytest.mark.parametrize("stem,fasta", [("test-1a", "test-1.fa"), ("test-1b", "test-1.fa"), ("test-2", "test-2.fa"), ("test-3", "test-3.fa"), ("test-4", "test-4.fa")])
def test_cli_on_reference_fixtures(tmp_path, stem, fasta):
	common = ["--haplotypes", "--input-reference=" + os.path.join(FIX, fasta), "--input-variants=" + os.path.join(FIX, stem + ".vcf"), "--chromosome=1", "--bgzf"]
	out = tmp_path / "out.a2m.gz"
	for extra, golden in [([], ".haplotypes.a2m"), (["--unaligned"], ".haplotypes.unaligned.fa"), (["--omit-reference", "--dst-chromosome=chrT"], ".haplotypes.chr.noref.a2m")]:
		r = _run(common + ["-s", str(out)] + extra)
		assert r.returncode == 0, r.stderr.decode()
		data = out.read_bytes()
		assert data.endswith(EOF_MEMBER)
		bgzf_members(data)
		assert gzip.decompress(data) == open(os.path.join(DERIVED, stem + golden), "rb").read(), extra


def test_cli_founders_and_two_contexts(tmp_path):
	g = synth.build_case(tmp_path, 35, 60000, 800, 12)
	fa, vcf = str(tmp_path / "synth.fa"), str(tmp_path / "synth.vcf")
	for extra in (["-F", "7"], ["-H", "--device=0,0"], ["-H", "--device=0,0", "--unaligned"]):
		plain, packed = tmp_path / "plain.a2m", tmp_path / "packed.a2m.gz"
		r = _run(["-r", fa, "-a", vcf, "-c", "1", "-s", str(plain)] + extra)
		assert r.returncode == 0, r.stderr.decode()
		r = _run(["-r", fa, "-a", vcf, "-c", "1", "-s", str(packed), "--bgzf"] + extra)
		assert r.returncode == 0, r.stderr.decode()
		data = packed.read_bytes()
		assert data.endswith(EOF_MEMBER)
		assert gzip.decompress(data) == plain.read_bytes(), extra
	assert g.total_chromosome_copies == 24


def test_config3_full_size(v2m):
	"""Config 3: REF + 31 copies of 100 Mbases through splice_rows(bgzf=True): every row's members decompress to the body the
	uncompressed path gives (by checksum), at <= 0.29 bytes per base."""
	import torch
	from vcf2multialign_amd import synth as vsynth
	ds = vsynth.dataset("config3")
	with v2m.Context(0) as ctx:
		ctx.upload_graph(ds.graph, ds.reference)
		dev = torch.device("cuda", 0)
		hp = 64
		thr = torch.from_numpy(ds.edge_thresholds.astype(np.int64)).to(torch.int32).to(dev)
		src = torch.empty(ds.path_rows // 64 * hp, dtype=torch.int64, device=dev)
		dst = torch.empty_like(src)
		torch.cuda.synchronize()
		ds.fill_paths_device(ctx.stream, src.data_ptr(), thr.data_ptr(), 0, hp)
		ctx.transpose_bits_device(src.data_ptr(), hp, ds.path_rows, dst.data_ptr())
		ctx.synchronize()
		ctx.set_paths_device(dst.data_ptr(), ds.path_rows, hp)
		rows = [v2m.PLOIDY_MAX] + list(range(31))
		plain = {}
		ctx.splice_rows(rows, sink=lambda i, body: plain.__setitem__(i, (len(body), int(v2m.checksum_rows_host([body])[0]))))
		packed, n_bytes = {}, [0]

		def sink(i, members):
			n_bytes[0] += len(members)
			body = gzip.decompress(members)
			packed[i] = (len(body), int(v2m.checksum_rows_host([body])[0]))

		ctx.splice_rows(rows, sink=sink, bgzf=True)
		assert packed == plain
		bases = sum(n for n, _ in plain.values())
		assert n_bytes[0] / bases <= 0.29, n_bytes[0] / bases
