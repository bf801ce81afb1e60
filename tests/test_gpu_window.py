"""Column windows (v2m_set_column_window, --region) on the GPU: every window body against the oracle's whole rows, sliced.

Aligned bodies are the oracle's aligned rows cut at [col_begin, col_end).  Unaligned bodies are checked with a small walk kept in
this file that knows which column every emitted byte sits in and which bytes are the walk's padding (column_walk); the walk itself is
checked against the oracle's aligned and unaligned rows first."""

import ctypes as C
import gzip
import json
import os
import subprocess

import numpy as np
import pytest

import oracle
import synth

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")
FOUNDER_FIX = os.path.join(HERE, "golden", "reference-fixtures", "founder-sequences")
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
TILE = 16384
PLOIDY_MAX = 0xFFFFFFFF


@pytest.fixture(scope="module")
def v2m():
	import vcf2multialign_amd as v
	return v


@pytest.fixture(scope="module")
def ctx(v2m):
	c = v2m.Context(0)
	yield c
	c.close()


# ---- the column-tracking walk --------------------------------------------------------------------------------------------------

def column_walk(g, copy_index=PLOIDY_MAX, cuts=None):
	"""output_sequence() (sequence_writer.cc:22-85) with the column of every byte: returns (aligned row bytes, padding mask), where
	mask[c] is True when column c holds the walk's padding (not a reference or label byte).  Rows with cuts switch copy at each cut
	node and follow REF before the first one."""
	rp = [int(x) for x in g.reference_positions]
	ap = [int(x) for x in g.aligned_positions]
	csum = [int(x) for x in g.alt_edge_count_csum]
	tgt = [int(x) for x in g.alt_edge_targets]
	lo = [int(x) for x in g.label_offsets]
	lb = g.label_bytes
	ref = g.ref
	words_per_copy = g.path_rows // 64
	paths = g.paths_by_chrom_copy_and_edge
	N, L = len(rp), ap[-1]
	row = bytearray(b"-" * L)
	pad = np.ones(L, dtype=bool)
	cut_at = dict(cuts or [])
	copy = copy_index if not cuts else PLOIDY_MAX

	def is_set(c, e):
		if c == PLOIDY_MAX:
			return False
		w = int(paths[c * words_per_copy + e // 64])
		return (w >> (e % 64)) & 1 == 1

	n = 0
	while n < N - 1:
		copy = cut_at.get(n, copy)
		taken = None
		for e in range(csum[n], csum[n + 1]):
			if is_set(copy, e):
				taken = e
				break
		if taken is None:
			seg = ref[rp[n]:rp[n + 1]]
			row[ap[n]:ap[n] + len(seg)] = seg
			pad[ap[n]:ap[n] + len(seg)] = False
			n += 1
		else:
			label = lb[lo[taken]:lo[taken + 1]]
			row[ap[n]:ap[n] + len(label)] = label
			pad[ap[n]:ap[n] + len(label)] = False
			# the walk never visits the nodes the edge jumps over; a cut node there would be skipped too
			for m in range(n + 1, tgt[taken]):
				copy = cut_at.get(m, copy)
			n = tgt[taken]
	return bytes(row), pad


def window_bodies(walked, b, e):
	row, pad = walked
	aligned = row[b:e]
	unaligned = bytes(np.frombuffer(aligned, dtype=np.uint8)[~pad[b:e]])
	return aligned, unaligned


def walk_rows(g, rows):
	out = []
	for r in rows:
		out.append(column_walk(g, cuts=list(r)) if isinstance(r, list) else column_walk(g, copy_index=int(r)))
	return out


def oracle_row(g, r, unaligned=False):
	if isinstance(r, list):
		return g.output_sequence(g.ref, cuts=list(r), unaligned=unaligned)
	return g.output_sequence(g.ref, copy_index=int(r), unaligned=unaligned)


# ---- window classes ------------------------------------------------------------------------------------------------------------

def window_classes(g, rng, n_random=6):
	"""(name, col_begin, col_end) for the classes the header pins: whole row, one column, first / last column, starts and ends inside a
	label and inside padding, on and across tile boundaries, inside one long deletion's span, a window no edge reaches into."""
	L = int(g.aligned_positions[-1])
	ap = np.asarray(g.aligned_positions, dtype=np.int64)
	csum = np.asarray(g.alt_edge_count_csum, dtype=np.int64)
	src = np.repeat(np.arange(len(ap) - 1), np.diff(csum)[:len(ap) - 1]) if g.edge_count else np.zeros(0, np.int64)
	begin = ap[src] if g.edge_count else np.zeros(0, np.int64)
	end = ap[np.asarray(g.alt_edge_targets, dtype=np.int64)] if g.edge_count else np.zeros(0, np.int64)
	llen = np.diff(np.asarray(g.label_offsets, dtype=np.int64)) if g.edge_count else np.zeros(0, np.int64)
	out = [("whole", 0, L), ("first", 0, 1), ("last", L - 1, L), ("one", L // 2, L // 2 + 1)]
	for k in range(1, L // TILE + 1):
		t = k * TILE
		if t < L:
			out.append(("on_tile_%d" % k, t, min(L, t + TILE)))
			out.append(("across_tile_%d" % k, max(0, t - 37), min(L, t + 53)))
			out.append(("ends_on_tile_%d" % k, max(0, t - TILE - 5), t))
	lab = np.nonzero(llen >= 3)[0]
	if lab.size:
		e = int(lab[rng.integers(lab.size)])
		out.append(("in_label", int(begin[e]) + 1, min(L, int(begin[e]) + int(llen[e]) - 1 + 40)))
		out.append(("ends_in_label", max(0, int(begin[e]) - 30), int(begin[e]) + 1))
	padded = np.nonzero(end - begin >= llen + 3)[0]
	if padded.size:
		e = int(padded[rng.integers(padded.size)])
		out.append(("in_padding", int(begin[e]) + int(llen[e]) + 1, min(L, int(end[e]) + 25)))
		out.append(("ends_in_padding", max(0, int(begin[e]) - 11), int(begin[e]) + int(llen[e]) + 1))
	if g.edge_count:
		e = int(np.argmax(end - begin))
		if end[e] - begin[e] >= 6:
			span = int(end[e] - begin[e])
			out.append(("inside_deletion", int(begin[e]) + span // 3, int(begin[e]) + 2 * span // 3))
		order = np.argsort(begin, kind="stable")
		reach = np.maximum.accumulate(end[order])
		gaps = np.nonzero(begin[order][1:] > reach[:-1] + 2)[0]
		if gaps.size:
			i = int(gaps[rng.integers(gaps.size)])
			out.append(("no_edges", int(reach[i]) + 1, int(begin[order][i + 1]) - 1))
	else:
		out.append(("no_edges", 0, L))
	for i in range(n_random):
		b = int(rng.integers(0, L))
		out.append(("random_%d" % i, b, int(rng.integers(b + 1, L + 1))))
	return [w for w in out if 0 <= w[1] < w[2] <= L]


def check_windows(v2m, ctx, g, rows, windows, forms=("rows",)):
	vg = v2m.VariantGraph.from_object(g)
	ctx.upload_graph(vg, g.ref)
	walked = walk_rows(g, rows)
	for name, b, e in windows:
		ctx.set_column_window(b, e)
		assert ctx.window_length == e - b
		assert ctx.aligned_length == int(g.aligned_positions[-1])
		exp = [window_bodies(w, b, e) for w in walked]
		for unaligned in (False, True):
			want = [x[1] if unaligned else x[0] for x in exp]
			if "rows" in forms:
				got = ctx.splice_rows(rows, unaligned=unaligned)
				for i, (a, w) in enumerate(zip(got, want)):
					assert a == w, "%s [%d, %d) unaligned=%s row %d" % (name, b, e, unaligned, i)
			if "held" in forms:
				got = {}

				def on_row(i, ptr, n, hold):
					got[i] = C.string_at(ptr, n) if n else b""
					ctx.release_row(hold)
				ctx.splice_rows_held(rows, on_row, n_slots=3, unaligned=unaligned)
				assert [got[i] for i in range(len(rows))] == want, "%s held unaligned=%s" % (name, unaligned)
			if "device" in forms:
				import torch
				need = ctx.max_unaligned_length if unaligned else ctx.window_length
				assert need == e - b or (b, e) == (0, int(g.aligned_positions[-1]))   # the whole row: today's bound
				pitch = (need + 15) // 16 * 16 + (48 if unaligned else 0)
				assert unaligned or ctx.min_row_pitch == (e - b + 255) // 256 * 256
				buf = torch.full((len(rows) * pitch + 64,), 0x55, dtype=torch.uint8, device="cuda")
				lengths = ctx.splice_rows_device(rows, buf.data_ptr(), pitch, unaligned=unaligned, want_lengths=True)
				ctx.synchronize()
				host = buf.cpu().numpy().tobytes()
				for i, w in enumerate(want):
					assert int(lengths[i]) == len(w)
					assert host[i * pitch:i * pitch + len(w)] == w, "%s device unaligned=%s row %d" % (name, unaligned, i)
				assert host[len(rows) * pitch:] == b"\x55" * 64   # nothing past the last row's pitch
			if "bgzf" in forms:
				got = ctx.splice_rows(rows, unaligned=unaligned, bgzf=True)
				for i, (a, w) in enumerate(zip(got, want)):
					assert (gzip.decompress(a) if a else b"") == w, "%s bgzf unaligned=%s row %d" % (name, unaligned, i)
					assert (len(a) == 0) == (len(w) == 0)   # an empty body gives no member
	ctx.set_column_window(0, int(g.aligned_positions[-1]))


# ---- the walk itself -----------------------------------------------------------------------------------------------------------

FIXTURES = [("test-1a", "test-1.fa"), ("test-1b", "test-1.fa"), ("test-2", "test-2.fa"), ("test-3", "test-3.fa"), ("test-4", "test-4.fa")]


def _fixture_graph(stem, fasta):
	return oracle.build_variant_graph(os.path.join(FIX, fasta), os.path.join(FIX, stem + ".vcf"), "1")


@pytest.mark.parametrize("stem,fasta", FIXTURES)
def test_column_walk_is_the_oracle(stem, fasta):
	g = _fixture_graph(stem, fasta)
	for r in [PLOIDY_MAX] + list(range(g.total_chromosome_copies)):
		row, pad = column_walk(g, copy_index=r)
		assert row == oracle_row(g, r)
		assert bytes(np.frombuffer(row, dtype=np.uint8)[~pad]) == oracle_row(g, r, unaligned=True)


# ---- through the C ABI ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stem,fasta", FIXTURES)
def test_reference_fixtures(v2m, ctx, stem, fasta):
	g = _fixture_graph(stem, fasta)
	L = int(g.aligned_positions[-1])
	rows = [PLOIDY_MAX] + list(range(g.total_chromosome_copies))
	windows = [("all_%d_%d" % (b, e), b, e) for b in range(L) for e in range(b + 1, L + 1) if (b * 7 + e) % 5 == 0 or e - b == 1 or b == 0 or e == L]
	check_windows(v2m, ctx, g, rows, windows)
	check_windows(v2m, ctx, g, rows, windows[::9], forms=("held", "device", "bgzf"))


def test_reference_mapping_on_the_ref_row(v2m, ctx):
	"""col(p) holds ref[p] in the REF row for every p, and a reference range's window is exactly its columns."""
	for stem, fasta in FIXTURES:
		g = _fixture_graph(stem, fasta)
		vg = v2m.VariantGraph.from_object(g)
		ctx.upload_graph(vg, g.ref)
		R = len(g.ref)
		for s in range(R):
			for e in range(s + 1, R + 1):
				b, en = vg.columns_of_reference_range(s, e)
				ctx.set_column_window(b, en)
				(body,) = ctx.splice_rows([PLOIDY_MAX], unaligned=True)
				assert body == g.ref[s:e], (stem, s, e)


@pytest.mark.parametrize("seed", range(32))
def test_synthetic_random_paths(v2m, ctx, tmp_path, seed):
	rng = np.random.default_rng(900 + seed)
	ref_len = int(rng.integers(2000, 70000))
	g = synth.build_case(tmp_path, 7000 + seed, ref_len, int(rng.integers(1, max(2, ref_len // 40))), int(rng.integers(1, 4)),
		multi_allelic=float(rng.choice([0.0, 0.2])), long_every=int(rng.choice([0, 13, 50])), max_indel=int(rng.choice([8, 64])))
	g = synth.with_random_paths(g, seed, float(rng.choice([0.05, 0.3, 0.8])))
	rows = [PLOIDY_MAX] + list(range(g.total_chromosome_copies))
	forms = ("rows", "held", "device", "bgzf") if seed % 8 == 0 else ("rows",)
	check_windows(v2m, ctx, g, rows, window_classes(g, rng), forms=forms)


def _bridges(g):
	reach, bridges = 0, []
	for n in range(g.node_count - 1):
		if n >= reach and n > 0:
			bridges.append(n)
		for e in range(int(g.alt_edge_count_csum[n]), int(g.alt_edge_count_csum[n + 1])):
			reach = max(reach, int(g.alt_edge_targets[e]))
	return bridges


@pytest.mark.parametrize("max_back", [None, "0"])
def test_founder_rows_with_cuts(v2m, ctx, tmp_path, monkeypatch, max_back):
	if max_back is not None:
		monkeypatch.setenv("V2M_MAX_BACK_WORDS", max_back)   # every cross-word restart goes through the serial kernel
	g = synth.with_random_paths(synth.build_case(tmp_path, 31, 90000, 4000, 6, multi_allelic=0.2, long_every=40), 3, 0.3)
	rng = np.random.default_rng(4)
	bridges = _bridges(g)
	H = g.total_chromosome_copies
	rows = [PLOIDY_MAX] + list(range(H))
	for k in (5, 40, min(400, len(bridges))):
		cuts = [0] + sorted(int(x) for x in rng.choice(bridges, size=k, replace=False))
		copies = [int(x) for x in rng.integers(0, H, size=len(cuts))]
		copies[1] = PLOIDY_MAX
		rows.append(list(zip(cuts, copies)))
	rows.append([(bridges[len(bridges) // 2], 1)])
	for r in rows[-4:]:
		assert column_walk(g, cuts=r)[0] == oracle_row(g, r)
	check_windows(v2m, ctx, g, rows, window_classes(g, rng, n_random=10), forms=("rows", "device"))


def test_founder_golden_fixture(v2m, ctx):
	with open(os.path.join(HERE, "golden", "reference_goldens.json")) as f:
		case = next(c for c in json.load(f)["founder_sequences"] if c["vcf"] == "test-2.vcf")
	g = oracle.build_variant_graph(os.path.join(FOUNDER_FIX, case["fasta"]), os.path.join(FOUNDER_FIX, case["vcf"]), "1")
	rows = [PLOIDY_MAX] + list(range(g.total_chromosome_copies))
	bridges = _bridges(g)
	if bridges:
		rows.append([(0, 0)] + [(bridges[0], 1)])
	check_windows(v2m, ctx, g, rows, window_classes(g, np.random.default_rng(1)))


def test_serial_resolve_restart(v2m, ctx, tmp_path, monkeypatch):
	"""Long deletions (restart points far back) with V2M_MAX_BACK_WORDS=0: the serial kernel scans from the window's restart word."""
	monkeypatch.setenv("V2M_MAX_BACK_WORDS", "0")
	g = synth.with_random_paths(synth.build_case(tmp_path, 55, 200000, 12000, 4, long_every=9, max_indel=200, multi_allelic=0.3), 8, 0.5)
	rows = [PLOIDY_MAX] + list(range(g.total_chromosome_copies))
	check_windows(v2m, ctx, g, rows, window_classes(g, np.random.default_rng(2), n_random=8))


def test_whole_window_and_reupload_match_no_window(v2m, tmp_path):
	g = synth.with_random_paths(synth.build_case(tmp_path, 12, 50000, 2000, 3, long_every=30), 2, 0.3)
	rows = [PLOIDY_MAX] + list(range(g.total_chromosome_copies))
	vg = v2m.VariantGraph.from_object(g)
	L = int(g.aligned_positions[-1])
	with v2m.Context(0) as plain, v2m.Context(0) as win:
		plain.upload_graph(vg, g.ref)
		win.upload_graph(vg, g.ref)
		ref = {u: plain.splice_rows(rows, unaligned=u) for u in (False, True)}
		win.set_column_window(100, 200)
		assert win.window_length == 100 and win.min_row_pitch == 256 and win.max_unaligned_length == 100
		win.set_column_window(0, L)
		assert win.window_length == L and win.min_row_pitch == plain.min_row_pitch and win.max_unaligned_length == plain.max_unaligned_length
		for u in (False, True):
			assert win.splice_rows(rows, unaligned=u) == ref[u]
		win.set_column_window(L // 3, L // 2)
		win.splice_rows(rows, unaligned=True)
		win.upload_graph(vg, g.ref)                          # a new upload is whole rows again
		assert win.window_length == L
		for u in (False, True):
			assert win.splice_rows(rows, unaligned=u) == ref[u]
			assert [gzip.decompress(x) for x in win.splice_rows(rows, unaligned=u, bgzf=True)] == ref[u]


def test_errors(v2m):
	import vcf2multialign_amd._native as N
	g = _fixture_graph("test-4", "test-4.fa")
	with v2m.Context(0) as c:
		assert c._lib.v2m_set_column_window(c._h, 0, 1) == N.V2M_ERR_STATE
		assert c.window_length == 0
		c.upload_graph(v2m.VariantGraph.from_object(g), g.ref)
		L = c.aligned_length
		for b, e in ((0, 0), (3, 3), (4, 2), (0, L + 1), (L, L + 1)):
			assert c._lib.v2m_set_column_window(c._h, b, e) == N.V2M_ERR_INVALID_ARGUMENT, (b, e)
		assert c.window_length == L


def test_bgzf_window_longer_than_a_member(v2m, ctx, tmp_path, monkeypatch):
	"""A window of several 65 280-byte pieces, with small ring slices: each member inflates to its piece of the window body."""
	monkeypatch.setenv("V2M_RING_SLOT_BYTES", str(1 << 18))
	g = synth.with_random_paths(synth.build_case(tmp_path, 14, 400000, 9000, 3), 5, 0.2)
	rows = [PLOIDY_MAX] + list(range(g.total_chromosome_copies))
	L = int(g.aligned_positions[-1])
	check_windows(v2m, ctx, g, rows, [("multi_member", 1000, min(L, 1000 + 3 * 65280 + 77))], forms=("rows", "bgzf", "held"))


# ---- the CLI -------------------------------------------------------------------------------------------------------------------

def _run(args):
	return subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)


def _records(data):
	"""[(header, body)] of an A2M / FASTA file."""
	out = []
	for chunk in data.split(b">")[1:]:
		head, _, body = chunk.partition(b"\n")
		assert body.endswith(b"\n")
		out.append((head, body[:-1]))
	return out


def oracle_cols(g, s, e):
	from vcf2multialign_amd.variant_graph import columns_of_reference_range
	return columns_of_reference_range(g.reference_positions, g.aligned_positions, s, e)


@pytest.mark.parametrize("devices", ["0", "0,0,0"])
def test_cli_region_every_output_mode(tmp_path, devices):
	g = synth.build_case(tmp_path, 41, 60000, 1500, 5, long_every=25, multi_allelic=0.1)
	fa, vcf = str(tmp_path / "synth.fa"), str(tmp_path / "synth.vcf")
	common = ["-H", "-r", fa, "-a", vcf, "-c", "1", "--device=" + devices]
	R = len(g.ref)
	ids = ["REF"] + ["%s-%d" % (s, 1 + c) for si, s in enumerate(g.sample_names) for c in range(int(g.ploidy_csum[si + 1]) - int(g.ploidy_csum[si]))]
	rows = [PLOIDY_MAX] + list(range(g.total_chromosome_copies))
	walked = walk_rows(g, rows)
	for S, E in ((1, 1), (1, 500), (R // 2, R // 2 + 20000), (R - 300, R)):
		b, e = oracle_cols(g, S - 1, E)
		for unaligned in (False, True):
			flag = ["--unaligned"] if unaligned else []
			want = [window_bodies(w, b, e)[1 if unaligned else 0] for w in walked]
			out = tmp_path / "w.a2m"
			r = _run(common + flag + ["-s", str(out), "--region=%d-%d" % (S, E), "--verbose"])
			assert r.returncode == 0, r.stderr.decode()
			assert ("alignment columns [%d, %d)" % (b, e)).encode() in r.stderr
			assert [h for h, _ in _records(out.read_bytes())] == [i.encode() for i in ids]
			assert [x for _, x in _records(out.read_bytes())] == want, (S, E, unaligned)
			bz = tmp_path / "w.a2m.gz"
			r = _run(common + flag + ["-s", str(bz), "--bgzf", "--region=%d-%d" % (S, E)])
			assert r.returncode == 0, r.stderr.decode()
			assert gzip.decompress(bz.read_bytes()) == out.read_bytes()
			sep = tmp_path / ("sep_%d_%d_%d" % (S, E, unaligned))
			sep.mkdir()
			for fmt in ("A2M", "plain"):
				r = subprocess.run([CLI] + common + flag + ["--output-sequences-separate", "--separate-output-format=" + fmt, "--region=%d-%d" % (S, E)],
					cwd=str(sep), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
				assert r.returncode == 0, r.stderr.decode()
				files = sorted(os.listdir(sep))
				assert len(files) == len(rows)
				for name in files:
					os.remove(sep / name)


def test_cli_region_separate_and_pipe_bodies(tmp_path):
	g = synth.build_case(tmp_path, 43, 30000, 800, 3, long_every=20)
	fa, vcf = str(tmp_path / "synth.fa"), str(tmp_path / "synth.vcf")
	R = len(g.ref)
	S, E = R // 3, R // 3 + 4000
	b, e = oracle_cols(g, S - 1, E)
	rows = [PLOIDY_MAX] + list(range(g.total_chromosome_copies))
	walked = walk_rows(g, rows)
	for devices in ("0", "0,0,0"):
		for unaligned in (False, True):
			flag = ["--unaligned"] if unaligned else []
			common = ["-H", "-r", fa, "-a", vcf, "-c", "1", "--device=" + devices, "--region=%d-%d" % (S, E)] + flag
			want = sorted(window_bodies(w, b, e)[1 if unaligned else 0] for w in walked)
			sep = tmp_path / ("sep_%s_%d" % (devices, unaligned))
			sep.mkdir()
			r = subprocess.run([CLI] + common + ["--output-sequences-separate", "--separate-output-format=plain"], cwd=str(sep), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
			assert r.returncode == 0, r.stderr.decode()
			def body(data):   # one sequence per file: an optional '>'id line, the body, a newline
				return (data.split(b"\n", 1)[1] if data.startswith(b">") else data).rstrip(b"\n")
			got = sorted(body(open(sep / f, "rb").read()) for f in os.listdir(sep))
			assert got == want, (devices, unaligned)
			script = tmp_path / "to_file.sh"
			script.write_text("#!/bin/sh\ncat > \"$1.piped\"\n")
			script.chmod(0o755)
			out = tmp_path / ("p_%s_%d.a2m" % (devices, unaligned))
			r = _run(common + ["-s", str(out), "--pipe=" + str(script)])
			assert r.returncode == 0, r.stderr.decode()
			piped = open(str(out) + ".piped", "rb").read()
			assert [x for _, x in _records(piped)] == [window_bodies(w, b, e)[1 if unaligned else 0] for w in walked]


def test_cli_region_founders(tmp_path):
	g = synth.build_case(tmp_path, 44, 40000, 1200, 6)
	fa, vcf = str(tmp_path / "synth.fa"), str(tmp_path / "synth.vcf")
	full, win = tmp_path / "full.a2m", tmp_path / "win.a2m"
	common = ["-F", "3", "-d", "10", "-r", fa, "-a", vcf, "-c", "1", "--device=0,0,0"]
	r = _run(common + ["-s", str(full)])
	assert r.returncode == 0, r.stderr.decode()
	R = len(g.ref)
	S, E = 1000, R - 2000
	b, e = oracle_cols(g, S - 1, E)
	r = _run(common + ["-s", str(win), "--region=%d-%d" % (S, E)])
	assert r.returncode == 0, r.stderr.decode()
	assert [(h, x[b:e]) for h, x in _records(full.read_bytes())] == _records(win.read_bytes())


# ---- paths the small windows above do not reach ---------------------------------------------------------------------------------

@pytest.mark.parametrize("nt,unaligned_store", [("0", "plain"), ("1", "nt")])
def test_window_store_flavours_forced(v2m, ctx, tmp_path, monkeypatch, nt, unaligned_store):
	"""Both store flavours of the window kernels (splice_aligned_window_kernel<false / true>, splice_unaligned_window_kernel<false / true>):
	small launches default to nontemporal stores and only launches of 1 GiB and more calibrate, so the plain ones run only when forced."""
	monkeypatch.setenv("V2M_NT_STORES", nt)
	monkeypatch.setenv("V2M_UNALIGNED_STORE", unaligned_store)
	g = synth.with_random_paths(synth.build_case(tmp_path, 41, 60000, 1500, 3, multi_allelic=0.2, long_every=30, max_indel=64), 6, 0.3)
	rows = [PLOIDY_MAX] + list(range(g.total_chromosome_copies))
	check_windows(v2m, ctx, g, rows, window_classes(g, np.random.default_rng(41)), forms=("rows", "device"))


@pytest.mark.parametrize("rows_per_group,count_rows", [("1", "7"), ("17", None), ("256", "1")])
def test_batches_of_many_rows(v2m, ctx, tmp_path, monkeypatch, rows_per_group, count_rows):
	"""More than 300 rows in one call (copies cycled, REF and founder rows among them), whole and windowed: several count groups of
	count_unaligned[_window]_kernel, the effective-edge cache reloaded every 16 rows of a splice group, V2M_ROWS_PER_GROUP at 1, 17 and 256
	and V2M_COUNT_ROWS_PER_GROUP at 1, 7 and the default."""
	monkeypatch.setenv("V2M_ROWS_PER_GROUP", rows_per_group)
	if count_rows is not None:
		monkeypatch.setenv("V2M_COUNT_ROWS_PER_GROUP", count_rows)
	g = synth.with_random_paths(synth.build_case(tmp_path, 43, 40000, 1200, 4, multi_allelic=0.2, long_every=25), 7, 0.3)
	H = g.total_chromosome_copies
	rng = np.random.default_rng(43)
	bridges = _bridges(g)
	kinds = [PLOIDY_MAX] + list(range(H))
	for k in (4, 40):
		cuts = [0] + sorted(int(x) for x in rng.choice(bridges, size=k, replace=False))
		kinds.append(list(zip(cuts, (int(x) for x in rng.integers(0, H, size=len(cuts))))))
	rows = [kinds[i % len(kinds)] for i in range(311)]
	vg = v2m.VariantGraph.from_object(g)
	ctx.upload_graph(vg, g.ref)
	for unaligned in (False, True):
		want = [oracle_row(g, r, unaligned) for r in kinds]
		assert ctx.splice_rows(rows, unaligned=unaligned) == [want[i % len(kinds)] for i in range(len(rows))], "whole rows, unaligned=%s" % unaligned
	walked = walk_rows(g, kinds)
	L = int(g.aligned_positions[-1])
	for b, e in ((0, L), (TILE - 100, 2 * TILE + 7), (L // 3, L // 3 + 5000), (L - 3 * TILE - 1, L - 1)):
		ctx.set_column_window(b, e)
		bodies = [window_bodies(w, b, e) for w in walked]
		for unaligned in (False, True):
			got = ctx.splice_rows(rows, unaligned=unaligned)
			assert len(got) == len(rows)
			for i, a in enumerate(got):
				assert a == bodies[i % len(kinds)][1 if unaligned else 0], "[%d, %d) unaligned=%s row %d" % (b, e, unaligned, i)
	ctx.set_column_window(0, L)


def test_cache_limits_under_windows(v2m, ctx, tmp_path, monkeypatch):
	"""test_extreme_spans_and_cache_limits' graph plus a tile with more than 1024 edges beginning in it and a label longer than 1 KiB, under
	windows that start or end inside the 150-kb deletion, inside the 70-kb insertion's label and inside the dense tile: every LDS-cache
	fallback of the window kernels (candidates past kCandLds and kCandDeltaLds, labels past kLabelLds, spans >= 64 KiB, a full long-span
	queue), also with row groups larger than the cached effective-edge rows."""
	g = synth.extreme_spans_case(tmp_path, dense_tile=True)
	ap = np.asarray(g.aligned_positions, dtype=np.int64)
	csum = np.asarray(g.alt_edge_count_csum, dtype=np.int64)
	src = np.repeat(np.arange(len(ap) - 1), np.diff(csum)[:len(ap) - 1])
	begin, end = ap[src], ap[np.asarray(g.alt_edge_targets, dtype=np.int64)]
	llen = np.diff(np.asarray(g.label_offsets, dtype=np.int64))
	per_tile = np.bincount(begin // TILE)
	dense = int(np.argmax(per_tile))
	assert per_tile[dense] > 1024 and llen.max() >= 70000 and ((llen > 1024) & (llen < 2000)).any()
	d = int(np.argmax(end - begin))                                   # the 150-kb deletion
	i = int(np.argmax(llen))                                          # the 70-kb insertion
	j = int(np.nonzero((llen > 1024) & (llen < 2000))[0][0])          # the 1500-bp insertion
	L = int(ap[-1])
	db, de, ib, jb = int(begin[d]), int(end[d]), int(begin[i]), int(begin[j])
	windows = [("starts_in_deletion", db + 5000, db + 90000), ("ends_in_deletion", db - 100, db + 20000), ("inside_deletion", db + 70000, de - 70000),
		("starts_in_insertion", ib + 1000, ib + int(llen[i]) + 500), ("ends_in_insertion", ib - 50, ib + 40000),
		("starts_in_dense_tile", dense * TILE + 100, min(L, (dense + 2) * TILE + 9)), ("ends_in_dense_tile", dense * TILE - 3000, dense * TILE + 9000),
		("in_long_label", jb + 10, jb + 1400), ("whole", 0, L)]
	rows = [PLOIDY_MAX] + list(range(6)) + [[(0, 0), (g.node_count - 3, 3)]]
	check_windows(v2m, ctx, g, rows, windows)
	monkeypatch.setenv("V2M_ROWS_PER_GROUP", "40")                  # 48 rows in one group of 40: rows 16.. use the uncached path
	check_windows(v2m, ctx, g, rows * 6, windows[:1] + windows[5:7])


@pytest.mark.parametrize("capacity", ["0", "3", None])
def test_resolve_queue_capacity_windowed(v2m, ctx, tmp_path, monkeypatch, capacity):
	"""test_gpu_parity.py::test_resolve_queue_capacity under column windows: the streaming resolve pass's overflow branch on a window's words."""
	if capacity is not None:
		monkeypatch.setenv("V2M_RESOLVE_QUEUE_CAPACITY", capacity)
	g = synth.with_random_paths(synth.build_case(tmp_path, 11, 60000, 5000, 4, multi_allelic=0.2, long_every=97), 5, 0.9)
	rng = np.random.default_rng(13)
	bridges = _bridges(g)
	H = g.total_chromosome_copies
	rows = [PLOIDY_MAX] + list(range(H))
	for k in (3, 30):
		cuts = [0] + sorted(int(x) for x in rng.choice(bridges, size=k, replace=False))
		rows.append(list(zip(cuts, (int(x) for x in rng.integers(0, H, size=len(cuts))))))
	check_windows(v2m, ctx, g, rows, window_classes(g, rng, n_random=3))
