"""Distinct pieces of a window set (v2m_splice_window_set_distinct, --regions-file --distinct) on the GPU.

Every case of tests/distinct_model.py's corpus is checked in both modes against the model: class_of, the class counts, every class
body, and the order and arguments of the sink calls.  tests/test_distinct_model_host.py asserts (without a GPU) what the corpus reaches."""

import os
import subprocess

import numpy as np
import pytest

import distinct_model as M
import synth
from test_gpu_window import PLOIDY_MAX, _fixture_graph, _records, oracle_cols, walk_rows, window_bodies
from test_gpu_window_sets import _bed

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")


@pytest.fixture(scope="module")
def v2m():
	import vcf2multialign_amd as v
	return v


@pytest.fixture(scope="module")
def ctx(v2m):
	c = v2m.Context(0)
	yield c
	c.close()


def check_case(v2m, ctx, case, monkeypatch=None, modes=(False, True), upload=True, want_pieces=True):
	"""The call on `case` in each mode against the model.  Returns nothing; asserts."""
	if monkeypatch is not None:
		for k, v in case.env.items():
			monkeypatch.setenv(k, v)
	if upload:
		ctx.upload_graph(v2m.VariantGraph.from_object(case.g), case.g.ref)
		ctx.set_window_set(case.windows)
	for unaligned in modes:
		class_of, bodies, _, calls = M.classes_of(case.expected(unaligned))
		seen = []
		pieces, got = ctx.splice_window_set_distinct(case.rows, unaligned=unaligned, want_pieces=want_pieces, on_class=lambda *a: seen.append(a))
		tag = "%s unaligned=%s" % (case.name, unaligned)
		assert got.shape == class_of.shape and got.dtype == np.uint32
		if not np.array_equal(got, class_of):
			r, k = [int(x[0]) for x in np.nonzero(got != class_of)]
			assert False, "%s: class_of[%d, %d] is %d, expected %d (window [%d, %d))" % ((tag, r, k, got[r, k], class_of[r, k]) + case.windows[k])
		assert ctx.distinct_class_counts.tolist() == [len(b) for b in bodies], tag
		if want_pieces:
			for k, (a, b) in enumerate(zip(pieces, bodies)):
				assert a == b, "%s: the class bodies of window %d [%d, %d)" % ((tag, k) + case.windows[k])
			assert seen == calls, tag
		else:
			assert pieces is None and seen == []


# ---- the corpus ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stem,fasta", M.FIXTURES)
def test_reference_fixtures(v2m, ctx, stem, fasta):
	check_case(v2m, ctx, M.fixture_case(stem, fasta))


@pytest.mark.parametrize("build", [b for b in M.CASE_BUILDERS if b not in (M.small_case, M.small_ring_case)], ids=lambda b: b.__name__)
def test_corpus(v2m, ctx, tmp_path, build):
	check_case(v2m, ctx, build(tmp_path))


def test_stale_slots(v2m, ctx, tmp_path):
	"""A call on other rows first, so that the device slot holds their bytes where the tested call's pieces end."""
	case = M.lengths_case(tmp_path)
	ctx.upload_graph(v2m.VariantGraph.from_object(case.g), case.g.ref)
	ctx.set_window_set(case.windows)
	for unaligned in (False, True):
		ctx.splice_window_set_distinct(list(reversed(case.rows)) + case.rows[3:], unaligned=not unaligned)
		check_case(v2m, ctx, case, modes=(unaligned,), upload=False)


def test_small_ring_slices(v2m, ctx, tmp_path, monkeypatch):
	case = M.small_ring_case(tmp_path)
	check_case(v2m, ctx, case, monkeypatch=monkeypatch)
	check_case(v2m, ctx, case, upload=False, want_pieces=False)


def test_without_pieces(v2m, ctx, tmp_path):
	check_case(v2m, ctx, M.seam_case(tmp_path), want_pieces=False)


@pytest.mark.parametrize("bits", ["0", "1", "3", "64"])
def test_hash_bits(v2m, ctx, tmp_path, monkeypatch, bits):
	"""Fewer key bits, more collisions, the same classes; at 0 bits every piece of a window collides and the rounds show in the profile."""
	from vcf2multialign_amd import _native as N
	case = M.small_case(tmp_path)
	monkeypatch.setenv("V2M_DISTINCT_HASH_BITS", bits)
	ctx.profile_enable(True)
	try:
		for unaligned in (False, True):
			ctx.profile_reset()
			check_case(v2m, ctx, case, modes=(unaligned,), upload=not unaligned)
			hashes, _ = ctx.profile_get(N.KERNEL_DISTINCT_HASH)
			gathers, _ = ctx.profile_get(N.KERNEL_DISTINCT_GATHER)
			verifies, _ = ctx.profile_get(N.KERNEL_DISTINCT_VERIFY)
			assert hashes == 1 and gathers >= 1 and verifies >= 1          # one slice
			if bits == "0":
				# c classes of one window and one length take at least c - 1 verify rounds (the lookup is per window, key and length)
				most = max(max(np.bincount([len(x) for x in b])) for b in M.classes_of(case.expected(unaligned))[1])
				assert verifies >= most - 1, (verifies, most)
				if not unaligned:
					assert most >= 3 and verifies > 1
	finally:
		ctx.profile_enable(False)


# ---- state and errors ------------------------------------------------------------------------------------------------------------

def test_state_and_errors(v2m, tmp_path, monkeypatch):
	import ctypes as C
	import vcf2multialign_amd._native as N
	case = M.small_case(tmp_path)
	g, rows = case.g, case.rows
	vg = v2m.VariantGraph.from_object(g)
	L = int(g.aligned_positions[-1])
	with v2m.Context(0) as plain, v2m.Context(0) as c:
		with pytest.raises(v2m.V2MError) as err:                    # before an upload
			c.splice_window_set_distinct(rows)
		assert err.value.code == N.V2M_ERR_STATE
		plain.upload_graph(vg, g.ref)
		c.upload_graph(vg, g.ref)
		with pytest.raises(v2m.V2MError) as err:                    # without a set
			c.splice_window_set_distinct(rows)
		assert err.value.code == N.V2M_ERR_STATE
		c.set_window_set(case.windows)
		plain.set_window_set(case.windows)
		c.set_column_window(300, 900)
		plain.set_column_window(300, 900)
		before = {u: plain.splice_window_set(rows, unaligned=u) for u in (False, True)}
		with pytest.raises(v2m.V2MError) as err:
			c.splice_window_set_distinct(rows, bgzf=True)
		assert err.value.code == N.V2M_ERR_UNSUPPORTED
		batch = v2m.RowBatch(rows)
		counts = np.zeros(len(case.windows), dtype=np.uint32)
		null_sink = C.cast(None, N.DISTINCT_SINK_FN)
		assert c._lib.v2m_splice_window_set_distinct(c._h, C.byref(batch.struct), 0, null_sink, None, None, counts.ctypes.data) == N.V2M_ERR_INVALID_ARGUMENT
		# an empty batch: V2M_OK, the counts zeroed
		counts[:] = 7
		table = np.zeros(1, dtype=np.uint32)
		assert c._lib.v2m_splice_window_set_distinct(c._h, C.byref(v2m.RowBatch([]).struct), 0, null_sink, None, table.ctypes.data, counts.ctypes.data) == N.V2M_OK
		assert not counts.any()
		# a sink that aborts
		calls = []

		def stop(*a):
			calls.append(a)
			if len(calls) == 5:
				raise RuntimeError("enough")
		with pytest.raises(RuntimeError):
			c.splice_window_set_distinct(rows, on_class=stop)
		assert len(calls) == 5
		stop_now = N.DISTINCT_SINK_FN(lambda *a: 1)
		table = np.zeros(len(rows) * len(case.windows), dtype=np.uint32)
		assert c._lib.v2m_splice_window_set_distinct(c._h, C.byref(batch.struct), 0, stop_now, None, table.ctypes.data, None) == N.V2M_ERR_SINK
		# the pool limit: the knob named, and the context good for the next call
		monkeypatch.setenv("V2M_DISTINCT_POOL_BYTES", "4096")
		assert sum(len(x) for b in M.classes_of(case.expected(False))[1] for x in b) > 4096
		with pytest.raises(v2m.V2MError) as err:
			c.splice_window_set_distinct(rows)
		assert err.value.code == N.V2M_ERR_OUT_OF_MEMORY and "V2M_DISTINCT_POOL_BYTES" in str(err.value)
		monkeypatch.delenv("V2M_DISTINCT_POOL_BYTES")
		check_case(v2m, c, case, upload=False)
		# the set, the column window and the other calls are as before
		assert c.window_set_size == len(case.windows) and c.window_length == 600
		for u in (False, True):
			assert c.splice_window_set(rows, unaligned=u) == before[u]
			assert c.splice_rows(rows[:5], unaligned=u) == plain.splice_rows(rows[:5], unaligned=u)
		c.set_column_window(0, L)
		# bad cuts
		with pytest.raises(v2m.V2MError) as err:
			c.splice_window_set_distinct([[(5, 0), (3, 1)]])
		assert err.value.code == N.V2M_ERR_PRECONDITION


def test_unaligned_refuses_a_nul_byte(v2m):
	import vcf2multialign_amd._native as N
	g = _fixture_graph("test-4", "test-4.fa")
	ref = bytearray(g.ref)
	ref[2] = 0
	with v2m.Context(0) as c:
		c.upload_graph(v2m.VariantGraph.from_object(g), bytes(ref))
		c.set_window_set([(0, 3), (1, 5)])
		pieces, class_of = c.splice_window_set_distinct([PLOIDY_MAX, PLOIDY_MAX])
		assert [[len(x) for x in p] for p in pieces] == [[3], [4]] and class_of.tolist() == [[0, 0], [0, 0]]   # aligned mode keeps such bytes
		with pytest.raises(v2m.V2MError) as err:
			c.splice_window_set_distinct([PLOIDY_MAX], unaligned=True)
		assert err.value.code == N.V2M_ERR_UNSUPPORTED


# ---- the checked build -----------------------------------------------------------------------------------------------------------

CHECKED_CORPUS = ["tests/test_gpu_distinct.py::" + name for name in (
	"test_reference_fixtures", "test_corpus", "test_stale_slots", "test_small_ring_slices", "test_hash_bits")]


def test_distinct_on_the_checked_build():
	"""A read past a piece's defined bytes changes keys or flags under one of the seeds, and so the classes."""
	from test_gpu_checked_build import SEEDS, run_checked_corpus
	from vcf2multialign_amd import build
	assert os.path.exists(build.CHECKED_LIB_PATH) and os.path.exists(build.CHECKED_HOST_LIB_PATH), "build_native() builds them"
	for seed in SEEDS:   # the second seed only once the first has passed
		rc, out = run_checked_corpus(seed, build.CHECKED_LIB_PATH, build.CHECKED_HOST_LIB_PATH, corpus=CHECKED_CORPUS)
		assert rc == 0, "checked build, seed %s: exit %d\n%s" % (seed, rc, out[-6000:])
		assert " passed" in out, out[-3000:]


# ---- the CLI ---------------------------------------------------------------------------------------------------------------------

def _run(args, cwd, env=None):
	return subprocess.run([CLI] + args, cwd=str(cwd), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)


def _first_occurrences(records):
	seen, out = set(), []
	for header, body in records:
		if body not in seen:
			seen.add(body)
			out.append((header, body))
	return out


@pytest.mark.parametrize("founders,unaligned,omit", [(False, False, False), (False, True, True), (True, False, False), (True, True, False)],
	ids=["haplotypes_aligned", "haplotypes_unaligned_omit_reference", "founders_aligned", "founders_unaligned"])
def test_cli_regions_file_distinct(tmp_path, founders, unaligned, omit):
	g = synth.build_case(tmp_path, 41, 60000, 1500, 5, long_every=25, multi_allelic=0.1)
	fa, vcf = str(tmp_path / "synth.fa"), str(tmp_path / "synth.vcf")
	regions, bed = _bed(len(g.ref), n=5)
	assert len(regions) == 8
	bed_path = tmp_path / "regions.bed"
	bed_path.write_bytes(bed)
	mode = ["-F", "3", "-d", "10"] if founders else ["-H"]
	flags = (["--unaligned"] if unaligned else []) + (["--omit-reference"] if omit else []) + ["-m", "chrT"]
	suffix = ".fa" if unaligned else ".a2m"
	args = ["-r", fa, "-a", vcf, "-c", "1"] + mode + flags + ["--device=0", "--regions-file=" + str(bed_path), "--verbose"]
	env = dict(os.environ, V2M_REGIONS_PER_PASS="3")
	plain_dir, distinct_dir = tmp_path / "plain", tmp_path / "distinct"
	plain_dir.mkdir()
	distinct_dir.mkdir()
	p = _run(args, plain_dir, env=env)
	assert p.returncode == 0, p.stderr.decode()
	d = _run(args + ["--distinct"], distinct_dir, env=env)
	assert d.returncode == 0, d.stderr.decode()
	assert b"passes of at most 3 regions" in d.stderr and b"distinct pieces" in d.stderr and b"distinct pieces" not in p.stderr
	assert sorted(os.listdir(plain_dir)) == sorted(name + suffix for name, _, _ in regions)
	assert sorted(os.listdir(distinct_dir)) == sorted([name + suffix for name, _, _ in regions] + [name + ".classes.tsv" for name, _, _ in regions])
	walked = None
	if not founders and not omit:
		walked = walk_rows(g, [PLOIDY_MAX] + list(range(g.total_chromosome_copies)))
	for name, s, e in regions:
		plain = _records((plain_dir / (name + suffix)).read_bytes())
		got = (distinct_dir / (name + suffix)).read_bytes()
		first = _first_occurrences(plain)
		assert got == b"".join(b">" + h + b"\n" + body + b"\n" for h, body in first), name
		class_of, bodies, first_rows, _ = M.classes_of([[body] for _, body in plain])
		tsv = b"".join(b"%s\t%s\t%d\n" % (h, plain[first_rows[0][class_of[r, 0]]][0], class_of[r, 0]) for r, (h, _) in enumerate(plain))
		assert (distinct_dir / (name + ".classes.tsv")).read_bytes() == tsv, name
		if walked is not None:   # the plain file itself, against the column-tracking walk (the non-distinct output is what it was)
			b, en = oracle_cols(g, s, e)
			assert [x for _, x in plain] == [window_bodies(w, b, en)[1 if unaligned else 0] for w in walked], name
	# the plain files are those of --region runs, one region each
	for name, s, e in regions[::3]:
		single = tmp_path / ("single_" + name + suffix)
		r = _run(["-r", fa, "-a", vcf, "-c", "1"] + mode + flags + ["--device=0", "-s", str(single), "--region=%d-%d" % (s + 1, e)], tmp_path)
		assert r.returncode == 0, r.stderr.decode()
		assert single.read_bytes() == (plain_dir / (name + suffix)).read_bytes(), name
