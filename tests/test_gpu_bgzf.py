"""The GPU BGZF encoder (V2M_SPLICE_BGZF, v2m_bgzf_compress, --bgzf): every output decompresses, with Python's zlib as the
independent decoder, to exactly the bytes the same call writes without compression; and every member is byte for byte the one the CPU
reference encoder (tests/deflate_ref.py) writes for its piece, at the edge inputs of tests/test_bgzf_model.py."""

import gzip
import os
import random
import shutil
import subprocess
import zlib

import numpy as np
import pytest

import deflate_ref
import synth
import test_bgzf_model as edges
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
	"""Symbol frequencies 1, 1, 2, 3, 5, 8, ... over 22 symbols.  (The builder's tie-break balances plain Fibonacci frequencies into
	12-bit codes; test_exact_limiters has a piece that does need the 15-bit limit.)"""
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
		assert members == deflate_ref.encode(body), "row %d: the members are not the reference encoder's" % i


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


# ---- byte for byte against the CPU reference encoder (tests/deflate_ref.py) ---------------------------------

def _first_difference(got, want):
	"""Where two members first differ, and the first token where their blocks differ (when the kernel's member decodes)."""
	i = next((k for k, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want)))
	where = "%d vs %d bytes, first difference at byte %d" % (len(got), len(want), i)
	try:
		g = deflate_ref.inflate_tokens(deflate_ref.member_payload(got))
		w = deflate_ref.inflate_tokens(deflate_ref.member_payload(want))
	except deflate_ref.DeflateError as e:
		return where + " (the kernel's member does not inflate: %s)" % e
	if [b["btype"] for b in g] != [b["btype"] for b in w]:
		return where + "; BTYPE %s vs %s" % ([b["btype"] for b in g], [b["btype"] for b in w])
	tg, tw = deflate_ref.tokens_of(g), deflate_ref.tokens_of(w)
	j = next((k for k, (a, b) in enumerate(zip(tg, tw)) if a != b), min(len(tg), len(tw)))
	if j < max(len(tg), len(tw)):
		pos = sum(1 if t[0] == "lit" else t[1] for t in tw[:j])
		return where + "; token %d (input byte %d): %s vs %s" % (j, pos, tg[j:j + 3], tw[j:j + 3])
	for key in ("hlit", "hclen", "cl_lengths", "lit_lengths"):
		if g[0].get(key) != w[0].get(key):
			return where + "; same tokens, %s differ: %s vs %s" % (key, g[0].get(key), w[0].get(key))
	return where


def _exact(ctx, cases):
	"""ctx.bgzf_compress(data) == deflate_ref.encode(data) for every (name, data); one call per case."""
	bad = []
	for name, data in cases:
		got, want = ctx.bgzf_compress(data), deflate_ref.encode(data)
		if got != want:
			try:
				gm = bgzf_members(got)
			except Exception:   # (the kernel's output is not even valid BGZF)
				gm = []
			if b"".join(p for _, p in gm) != data:
				gm = []
			wm = bgzf_members(want)
			k = next((k for k, (a, b) in enumerate(zip(gm, wm)) if a[0] != b[0]), 0)
			bad.append("%s, member %d: %s" % (name, k, _first_difference(gm[k][0], wm[k][0]) if gm else "does not decompress to the input"))
	assert not bad, "%d of %d cases differ from the reference encoder:\n" % (len(bad), len(cases)) + "\n".join(bad[:20])


def test_exact_piece_sizes(ctx):
	_exact(ctx, edges.size_pieces())


def test_exact_runs_at_segment_edges(ctx):
	_exact(ctx, [(name, data) for name, data, _ in edges.segment_edge_pieces()])


def test_exact_byte_values(ctx):
	_exact(ctx, edges.byte_value_pieces())


def test_exact_limiters(ctx):
	"""The literal/length code folded into 15 bits, and the code-length code into 7 (the model's tests show both need it)."""
	_exact(ctx, [("15-bit limit", edges.fibonacci_piece()), ("7-bit code-length limit", edges.cl_limit_piece())])


def test_exact_stored_dynamic_tie(ctx):
	"""Through stored_bytes == dynamic_bytes: at the tie the stored block is the one (stored iff it is not larger)."""
	sweep = edges.tie_sweep()
	diffs = [d for _, _, d in sweep]
	assert 0 in diffs and min(diffs) < 0 < max(diffs)
	_exact(ctx, [("run of %d, stored - dynamic = %d" % (r, d), piece) for r, piece, d in sweep])
	for r, piece, d in sweep:
		if d == 0:
			assert ctx.bgzf_compress(piece)[18] & 7 == 1, "the tie takes the stored block"


def test_exact_random_pieces(ctx):
	_exact(ctx, edges.random_pieces(64))


def test_exact_in_one_call(ctx):
	"""The same pieces as the members of one multi-piece call (every piece a full one, so the pieces are the cases)."""
	cases = [d for _, d, _ in edges.segment_edge_pieces()] + [d for _, d in edges.random_pieces(64) if len(d) == PIECE]
	data = b"".join(cases)
	assert ctx.bgzf_compress(data) == b"".join(deflate_ref.encode_member(d) for d in cases)


def _distinct_pieces(n_bytes, seed):
	"""n_bytes of A2M-like pieces, each made distinct by its index in its first 8 bytes."""
	n = -(-n_bytes // PIECE)
	base = np.frombuffer(edges.a2m_like(seed, PIECE), np.uint8)
	a = np.tile(base, n)
	a.reshape(n, PIECE)[:, :8] = np.arange(n, dtype="<u8").view(np.uint8).reshape(n, 8)
	return a[:n_bytes].tobytes()


def _check_pieces(out, data):
	members = bgzf_members(out)
	assert len(members) == -(-len(data) // PIECE)
	for k, (_, p) in enumerate(members):
		assert p == data[k * PIECE:(k + 1) * PIECE], "member %d" % k
	return members


@pytest.mark.parametrize("n_pieces", [1023, 1024, 1025, 2049])
def test_many_blocks_in_one_pass(ctx, n_pieces):
	"""The member-size scan runs in rounds of 1024 blocks: every member in its place, and the members at the rounds' edges exact."""
	data = _distinct_pieces(n_pieces * PIECE - 1000, n_pieces)
	members = _check_pieces(ctx.bgzf_compress(data), data)
	for k in sorted({0, 1, 1022, 1023, 1024, 1025, 2047, 2048, n_pieces - 2, n_pieces - 1} & set(range(n_pieces))):
		assert members[k][0] == deflate_ref.encode_member(data[k * PIECE:(k + 1) * PIECE]), "member %d" % k


def test_multi_pass_compress(ctx):
	"""v2m_bgzf_compress takes 4096 pieces per pass: an input of two passes, the members either side of the boundary exact, and the
	whole output that of one call per pass."""
	chunk = 4096 * PIECE
	data = _distinct_pieces(chunk + 2 * PIECE + 77, 3)
	out = ctx.bgzf_compress(data)
	members = _check_pieces(out, data)
	assert len(members) == 4096 + 3
	for k in (4094, 4095, 4096, 4097, 4098):
		assert members[k][0] == deflate_ref.encode_member(data[k * PIECE:(k + 1) * PIECE]), "member %d" % k
	assert out == ctx.bgzf_compress(data[:chunk]) + ctx.bgzf_compress(data[chunk:])


# ---- the same file whichever way it is written -----------------------------------------------------------

def _run_env(args, **env):
	e = dict(os.environ)
	e.update(env)
	return subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=e)


def test_cli_files_are_reproducible(v2m, tmp_path):
	"""--bgzf files are byte-identical across one context and --device=0,0, across ring slice sizes, and to what the Python
	HaplotypeOutput writes, aligned and --unaligned; -F likewise across contexts and slice sizes."""
	g = synth.build_case(tmp_path, 36, 90000, 1500, 8, long_every=40)
	fa, vcf = str(tmp_path / "synth.fa"), str(tmp_path / "synth.vcf")
	files = {}
	for mode in (["-H"], ["-H", "--unaligned"], ["-F", "7"]):
		outs = []
		for extra, env in [([], {}), (["--device=0,0"], {}), ([], {"V2M_RING_SLOT_BYTES": "300000"}), (["--device=0,0"], {"V2M_RING_SLOT_BYTES": "1000000"})]:
			out = tmp_path / ("out%d.a2m.gz" % len(outs))
			r = _run_env(["-r", fa, "-a", vcf, "-c", "1", "-s", str(out), "--bgzf"] + mode + extra, **env)
			assert r.returncode == 0, r.stderr.decode()
			outs.append(out.read_bytes())
		assert all(o == outs[0] for o in outs), (mode, [len(o) for o in outs])
		files[" ".join(mode)] = outs[0]
	import io
	vg = v2m.VariantGraph.from_object(g)
	with v2m.Context(0) as c:
		c.upload_graph(vg, g.ref)
		for unaligned, key in ((False, "-H"), (True, "-H --unaligned")):
			buf = io.BytesIO()
			v2m.HaplotypeOutput(c, bgzf=True, should_output_unaligned=unaligned).output_a2m(vg, buf)
			assert buf.getvalue() == files[key], key
	gz = shutil.which("gzip")
	if gz:
		for key, data in files.items():
			r = subprocess.run([gz, "-dc"], input=data, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
			assert r.returncode == 0 and r.stdout == gzip.decompress(data), (key, r.stderr)


def test_cli_fixture_file_is_the_python_one(v2m, ctx, tmp_path):
	import io
	import oracle
	for unaligned in (False, True):
		out = tmp_path / "out.a2m.gz"
		args = ["--haplotypes", "--input-reference=" + os.path.join(FIX, "test-4.fa"), "--input-variants=" + os.path.join(FIX, "test-4.vcf"),
			"--chromosome=1", "--bgzf", "-s", str(out)] + (["--unaligned"] if unaligned else [])
		r = _run(args)
		assert r.returncode == 0, r.stderr.decode()
		g = oracle.build_variant_graph(os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf"), "1")
		vg = v2m.VariantGraph.from_object(g)
		ctx.upload_graph(vg, g.ref)
		buf = io.BytesIO()
		v2m.HaplotypeOutput(ctx, bgzf=True, should_output_unaligned=unaligned).output_a2m(vg, buf)
		assert buf.getvalue() == out.read_bytes()
