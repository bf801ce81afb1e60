"""CPU-side tests (no GPU): the C-ABI library loads and exports every symbol include/v2m_hip.h declares, fails
loudly without a device, and the host-side logic (row batches, sharding, checksums) is right."""

import json
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def v2m():
	from vcf2multialign_amd import build
	build.build_native()
	import vcf2multialign_amd as v
	return v


def _declared_functions():
	with open(os.path.join(ROOT, "include", "v2m_hip.h")) as f:
		text = f.read()
	text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
	names = set(re.findall(r"\b(v2m_[a-z0-9_]+)\s*\(", text))
	names -= {"v2m_sink_fn"}
	return sorted(names)


def test_library_exports_every_declared_symbol(v2m):
	from vcf2multialign_amd import _native
	lib = v2m.load_library()
	declared = _declared_functions()
	assert len(declared) >= 18
	for name in declared:
		assert hasattr(lib, name), name + " is declared in include/v2m_hip.h but not exported"
	assert set(declared) == set(_native.SIGNATURES), "ctypes signatures and header disagree"
	assert lib.v2m_abi_version() == 5


def test_no_device_means_loud_failure(v2m):
	import torch
	if torch.cuda.is_available():
		pytest.skip("a GPU is present")
	with pytest.raises(v2m.V2MError) as e:
		v2m.Context(0)
	assert e.value.code == 4 and "no CPU fallback" in str(e.value)


def test_product_never_touches_the_oracle():
	"""The product tree must not import, link or mention the oracle (it is test infrastructure)."""
	pkg = os.path.join(ROOT, "vcf2multialign_amd")
	for dirpath, _, files in os.walk(pkg):
		for fn in files:
			if fn.endswith((".py", ".hip", ".cc", ".hh", ".hpp", ".h")):
				with open(os.path.join(dirpath, fn), errors="replace") as f:
					text = f.read()
				assert "v2mo_" not in text and "libv2m_oracle" not in text and "import oracle" not in text, os.path.join(dirpath, fn)


def test_row_batch_layout(v2m):
	rb = v2m.RowBatch([v2m.PLOIDY_MAX, 3, [(0, 5), (7, v2m.PLOIDY_MAX), (9, 2)], 1])
	assert rb.n_rows == 4
	assert rb.copy_index.tolist() == [v2m.PLOIDY_MAX, 3, v2m.PLOIDY_MAX, 1]
	assert rb.cut_offsets.tolist() == [0, 0, 0, 3, 3]
	assert rb.cut_nodes.tolist() == [0, 7, 9] and rb.cut_copies.tolist() == [5, v2m.PLOIDY_MAX, 2]
	assert v2m.RowBatch([0, 1]).cut_offsets is None
	assert v2m.RowBatch.haplotypes(range(3), include_reference=True).copy_index.tolist() == [v2m.PLOIDY_MAX, 0, 1, 2]


def test_checksum_reference_values(v2m):
	# the checksum definition in include/v2m_hip.h, spelled out independently for two tiny rows
	def mix(z):
		z &= 2 ** 64 - 1
		z ^= z >> 30; z = z * 0xBF58476D1CE4E5B9 % 2 ** 64
		z ^= z >> 27; z = z * 0x94D049BB133111EB % 2 ** 64
		z ^= z >> 31
		return z
	def ref(b):
		acc = mix(len(b))
		padded = b + b"\0" * ((-len(b)) % 8)
		for i in range(0, len(padded), 8):
			acc += mix(((i // 8 + 1) * 0x9E3779B97F4A7C15) % 2 ** 64 ^ int.from_bytes(padded[i:i + 8], "little"))
		return acc % 2 ** 64
	rows = [b"ACGT-ACGTACG", b"", b"A" * 8, b"ACGTACGTT"]
	assert v2m.checksum_rows_host(rows).tolist() == [ref(r) for r in rows]


@pytest.mark.parametrize("n_copies,world", [(5008, 1), (5008, 2), (5008, 4), (5008, 8), (2000, 8), (20000, 8), (100, 8), (64, 3), (1, 2)])
def test_sharding_covers_all_rows_in_order(n_copies, world):
	from vcf2multialign_amd.sharding import PLOIDY_MAX, local_rows, shard_copies
	seen = []
	for r in range(world):
		c0, c1, hp = shard_copies(n_copies, world, r)
		assert c0 % 8 == 0 or c0 == n_copies                   # whole bytes of the bit-packed source matrix
		assert hp % 64 == 0 and c1 - c0 <= hp < c1 - c0 + 64
		rows = local_rows(n_copies, world, r)
		for gi, lc in rows:
			assert lc == PLOIDY_MAX or 0 <= lc < hp
		seen.extend(gi for gi, _ in rows)
	assert seen == list(range(n_copies + 1))
	sizes = [len(local_rows(n_copies, world, r)) for r in range(world)]
	assert max(sizes) - min(sizes) <= 8                         # REF sits on rank 0, which gets no left-over block


def _free_port():
	s = socket.socket()
	s.bind(("127.0.0.1", 0))
	p = s.getsockname()[1]
	s.close()
	return p


def _gloo_worker(rank, world, port, n_copies, q):
	"""What a rank of bench.py does with the others under torch.distributed.run, through bench.py's own TorchHub: a barrier, one
	gather of figures, the maximum taken on rank 0.  No row and no tensor travels."""
	import sys
	sys.path.insert(0, ROOT)
	import bench
	from vcf2multialign_amd.sharding import local_rows
	os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
	hub = bench.TorchHub("gloo", rank, None)
	rows = local_rows(n_copies, world, rank)
	hub.barrier()
	everyone = hub.gather({"rank": rank, "elapsed_s": 1.0 + rank, "rows": [gi for gi, _ in rows]})
	hub.close()
	q.put((rank, everyone))


def test_two_rank_gloo_partition():
	"""world_size-2 rehearsal of the N>1 path on CPU: both ranks derive disjoint, ordered shards, and rank 0 ends up with every
	rank's figures (the max-over-ranks time is taken from them, as bench.py does)."""
	import torch.multiprocessing as mp
	ctx = mp.get_context("spawn")
	q = ctx.Queue()
	port = _free_port()
	procs = [ctx.Process(target=_gloo_worker, args=(r, 2, port, 300, q)) for r in range(2)]
	for p in procs:
		p.start()
	results = dict(q.get(timeout=120) for _ in procs)
	for p in procs:
		p.join(timeout=60)
		assert p.exitcode == 0
	assert results[1] is None                                     # only rank 0 holds the gathered figures
	everyone = results[0]
	assert [f["rank"] for f in everyone] == [0, 1] and max(f["elapsed_s"] for f in everyone) == 2.0
	assert everyone[0]["rows"] + everyone[1]["rows"] == list(range(301))
	assert everyone[0]["rows"][-1] == 152 and everyone[1]["rows"][0] == 153   # rank 0: REF + copies 0..151 (19 bytes of every column), rank 1: copies 152..299


def test_cpu_quota_and_threads_per_rank(tmp_path, monkeypatch):
	"""The host side of a rank is sized from the job's quota (affinity mask, cgroup cpu.max) divided by the node's ranks."""
	from vcf2multialign_amd import sharding
	cores, source = sharding.cpu_quota()
	assert 1 <= cores <= (os.cpu_count() or 1) and source
	assert sharding.host_threads_per_rank(1, cap=4) <= 4
	assert sharding.host_threads_per_rank(10 ** 6) == 1
	monkeypatch.setattr(sharding, "cpu_quota", lambda: (16, "test"))
	assert [sharding.host_threads_per_rank(n) for n in (1, 2, 4, 8, 16, 32)] == [16, 8, 4, 2, 1, 1]
	assert sharding.host_threads_per_rank(1, cap=12) == 12 and sharding.host_threads_per_rank(2, reserve=4) == 6


def test_header_is_plain_c_and_the_c_example_links(tmp_path):
	"""include/v2m_hip.h compiles as C99 (no C++ in the boundary) and examples/splice_rows.c links against the library
	with nothing but the header (it is run by the GPU suite)."""
	import shutil
	import subprocess
	from vcf2multialign_amd import build
	root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
	gcc = shutil.which("gcc")
	assert gcc, "gcc is part of the image"
	src = os.path.join(root, "examples", "splice_rows.c")
	for example in (src, os.path.join(root, "examples", "sharded_rows.c")):
		subprocess.check_call([gcc, "-std=c99", "-Wall", "-Wextra", "-pedantic", "-Werror", "-I" + os.path.join(root, "include"), "-fsyntax-only", example])
	build.build_native()
	exe = tmp_path / "splice_rows"
	subprocess.check_call([gcc, "-std=c99", "-I" + os.path.join(root, "include"), src, "-L" + build.PKG_DIR, "-lv2m_hip",
		"-Wl,-rpath," + build.PKG_DIR, "-Wl,-rpath-link,/opt/rocm/lib", "-o", str(exe)])
	assert exe.exists()


def test_cxx_and_python_sharding_agree():
	"""The command-line driver (csrc/host/gpu_path.cc) and bench.py / sharding.py cut the chromosome copies at the same places."""
	from vcf2multialign_amd import host
	from vcf2multialign_amd.sharding import shard_copies
	for n_copies in (0, 1, 7, 8, 9, 63, 64, 65, 200, 2000, 5008, 20000, 20001):
		for world in (1, 2, 3, 4, 7, 8, 16):
			covered = 0
			for rank in range(world):
				c0, c1, hp = shard_copies(n_copies, world, rank)
				assert host.shard_copies(n_copies, world, rank) == (c0, c1), (n_copies, world, rank)
				assert c0 == covered and c0 % 8 == 0 or c0 == n_copies
				assert hp % 64 == 0 and hp >= c1 - c0
				covered = c1
			assert covered == n_copies


def test_traffic_is_quoted_only_for_the_sources_it_was_measured_on():
	"""roofline.traffic comes from profiles/pmc_traffic.json and must disappear when the kernel sources have changed since."""
	import subprocess
	import sys
	ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
	sys.path.insert(0, ROOT)
	import bench
	stamp = bench.kernel_source_stamp()
	assert set(stamp) == set(bench.KERNEL_SOURCES) and all(len(h) == 40 for h in stamp.values())
	out = subprocess.run(["git", "hash-object", os.path.join(ROOT, bench.KERNEL_SOURCES[0])], stdout=subprocess.PIPE, cwd=ROOT)
	if out.returncode == 0:
		assert out.stdout.decode().strip() == stamp[bench.KERNEL_SOURCES[0]]
	# the committed record carries a stamp, and bench.py's rule is "equal stamps or no traffic figure"
	import json
	with open(os.path.join(ROOT, "profiles", "pmc_traffic.json")) as f:
		rec = json.load(f)
	for name, r in rec.items():
		if not name.startswith("_"):
			assert set(r["kernel_sources"]) == set(bench.KERNEL_SOURCES), name


def test_every_quoted_include_is_a_build_dependency_and_a_stamped_kernel_source():
	"""The library is rebuilt for -- and a PMC traffic figure is tied to -- every file v2m_hip.hip reaches through #include "...":
	the lists are read off the sources (build.include_closure), so a header cannot be forgotten again (round 3: founder_kernels.hpp)."""
	import sys
	from vcf2multialign_amd import build
	sys.path.insert(0, ROOT)
	import bench
	csrc = os.path.join(ROOT, "vcf2multialign_amd", "csrc")
	quoted = re.compile(r'^[ \t]*#[ \t]*include[ \t]*"([^"]+)"', re.M)
	def reach(path, seen):
		path = os.path.normpath(path)
		if path in seen:
			return seen
		seen.add(path)
		with open(path) as f:
			for inc in quoted.findall(f.read()):
				reach(os.path.join(os.path.dirname(path), inc), seen)
		return seen
	for sources, deps in ((build.HIP_SOURCES, build.HIP_DEPS), (build.HOST_SOURCES, build.HOST_DEPS), (build.SYNTH_SOURCES, build.SYNTH_DEPS), (build.CLI_SOURCES, build.CLI_DEPS)):
		want = set()
		for src in sources:
			reach(src, want)
		assert want <= set(deps), sorted(want - set(deps))
	hip = {os.path.relpath(p, ROOT) for p in build.HIP_DEPS}
	assert os.path.join("vcf2multialign_amd", "csrc", "founder_kernels.hpp") in hip and os.path.join("vcf2multialign_amd", "csrc", "kernels.hpp") in hip
	assert set(bench.KERNEL_SOURCES) == hip
	# every header under csrc/ belongs to some target: none is an orphan that a list could miss
	every = set(build.HIP_DEPS) | set(build.HOST_DEPS) | set(build.SYNTH_DEPS) | set(build.CLI_DEPS)
	for dirpath, _, files in os.walk(csrc):
		for fn in files:
			if fn.endswith((".hpp", ".hh", ".h")):
				assert os.path.join(dirpath, fn) in every, fn + " is included by nothing that is built"


def test_nothing_is_compiled_under_a_profiler(tmp_path, monkeypatch):
	"""A stale library in a process that runs under rocprofv3's preload is an error, not a compile: a compiler launcher started there
	would exec with the GPU already initialised by the preload (the hop that takes a node of the pool down)."""
	from vcf2multialign_amd import build
	assert not build.under_profiler()
	monkeypatch.setenv("LD_PRELOAD", "/opt/rocm/lib/librocprofiler-sdk-tool.so")
	assert build.under_profiler()
	with pytest.raises(build.StaleUnderProfiler):
		build._build(str(tmp_path / "missing.so"), build.HIP_SOURCES, build.HIP_DEPS, False, False)     # missing target: would have to compile
	build.build_native()                                                                                  # everything fresh: a no-op, no error
	monkeypatch.delenv("LD_PRELOAD")
	monkeypatch.setenv("ROCPROFILER_SOMETHING", "1")
	assert build.under_profiler()
	import oracle
	monkeypatch.setattr(oracle, "_LIB_PATH", str(tmp_path / "no_such_oracle.so"))
	with pytest.raises(RuntimeError):
		oracle.build_oracle()


def test_an_unresolved_include_makes_its_target_stale_and_nothing_else(tmp_path):
	from vcf2multialign_amd import build
	src = tmp_path / "a.cc"
	src.write_text('#include "there.hh"\n#if 0\n#include "not_there.hh"\n#endif\n')
	(tmp_path / "there.hh").write_text("// ok")
	closure = build.include_closure([str(src)])
	missing = [d for d in closure if isinstance(d, build.MissingInclude)]
	assert len(closure) == 3 and len(missing) == 1 and missing[0].endswith("not_there.hh")
	lib = tmp_path / "a.so"
	lib.write_bytes(b"")
	assert build._stale(str(lib), closure) and not build._stale(str(lib), [d for d in closure if d not in missing])
	with pytest.raises(RuntimeError):
		build.include_closure([str(src)], strict=True)
	# the tree itself has none: every quoted include of every target resolves
	for name, sources in build._SOURCES_OF.items():
		assert build.include_closure(sources, strict=True) == getattr(build, name)


def test_a_stale_library_is_noticed_through_any_header(tmp_path):
	from vcf2multialign_amd import build
	target = tmp_path / "lib.so"
	target.write_bytes(b"")
	old = os.path.getmtime(str(target)) - 1000
	for dep in build.HIP_DEPS:
		assert os.path.exists(dep)
	os.utime(str(target), (old - 10 ** 9, old - 10 ** 9))          # older than every source
	assert build._stale(str(target), build.HIP_DEPS)
	header = tmp_path / "founder_kernels.hpp"
	header.write_text("// stand-in")
	os.utime(str(target), None)
	os.utime(str(header), (old, old))
	assert not build._stale(str(target), [str(header)])
	os.utime(str(header), (os.path.getmtime(str(target)) + 5, os.path.getmtime(str(target)) + 5))
	assert build._stale(str(target), [str(header)])


def _clean_env():
	return {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "V2M_BENCH_HUB")}


@pytest.mark.parametrize("n", [2, 8])
def test_bench_hub_over_pipes(n):
	"""`python bench.py --gpus N` as typed: the parent is the ranks' hub (barriers + one gather over pipes), with no torch.distributed
	group at all.  --hub-selftest runs exactly that plumbing with no GPU work."""
	import json
	import subprocess
	import sys
	r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--hub-selftest"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=_clean_env())
	assert r.returncode == 0, r.stderr.decode()[-2000:]
	lines = [l for l in r.stdout.decode().splitlines() if l.strip()]
	assert len(lines) == 1
	d = json.loads(lines[0])
	assert [f["rank"] for f in d["hub_selftest"]] == list(range(n)) and len({f["pid"] for f in d["hub_selftest"]}) == n
	assert "no torch.distributed" in d["ranks_coordinated_by"]
	with open(os.path.join(ROOT, "bench.py")) as f:
		text = f.read()
	hub = text[text.index("class PipeHub"):text.index("class TorchHub")] + text[text.index("def launch_ranks"):text.index("class SoloHub")]
	assert "import torch" not in hub and "dist." not in hub.replace("torch.distributed.", "") and "init_process_group" not in hub


@pytest.mark.parametrize("n", [2, 8])
def test_bench_hub_under_torch_distributed_run(n):
	"""The driver's launch form (python -m torch.distributed.run --nproc-per-node N ... bench.py --gpus N), world sizes 2 and 8 on CPU: the
	same barrier / gather through a gloo group -- what the 8-GPU scaling run will use to line its ranks up."""
	import json
	import subprocess
	import sys
	r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(n), "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
		os.path.join(ROOT, "bench.py"), "--gpus", str(n), "--hub-selftest"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, env=_clean_env())
	assert r.returncode == 0, r.stderr.decode()[-2000:]
	lines = [l for l in r.stdout.decode().splitlines() if l.strip().startswith("{")]
	assert len(lines) == 1
	d = json.loads(lines[0])
	assert [f["rank"] for f in d["hub_selftest"]] == list(range(n)) and "torch.distributed (gloo)" in d["ranks_coordinated_by"]


def test_checksum_sink_of_the_end_to_end_leg(v2m):
	"""bench.py's end-to-end sink (libv2m_synth.so: v2ms_checksum_sink_fn) computes the checksum of include/v2m_hip.h for rows of
	every length class, whatever the number of threads it cuts a row over."""
	import ctypes as C
	from vcf2multialign_amd import build
	sl = C.CDLL(build.SYNTH_LIB_PATH)
	sl.v2ms_checksum_sink_create.restype = C.c_void_p
	sl.v2ms_checksum_sink_create.argtypes = [C.c_uint64, C.c_uint32]
	sl.v2ms_checksum_sink_fn.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]
	sl.v2ms_checksum_sink_fn.restype = C.c_int
	sl.v2ms_checksum_sink_checksums.restype = C.POINTER(C.c_uint64)
	sl.v2ms_checksum_sink_checksums.argtypes = [C.c_void_p]
	sl.v2ms_checksum_sink_lengths.restype = C.POINTER(C.c_uint64)
	sl.v2ms_checksum_sink_lengths.argtypes = [C.c_void_p]
	sl.v2ms_checksum_sink_rows.restype = C.c_uint64
	sl.v2ms_checksum_sink_rows.argtypes = [C.c_void_p]
	sl.v2ms_checksum_sink_destroy.argtypes = [C.c_void_p]
	sl.v2ms_checksum_sink_flavour.restype = C.c_char_p
	sl.v2ms_checksum_sink_flavour.argtypes = [C.c_void_p]
	sl.v2ms_checksum_sink_force_scalar.argtypes = [C.c_void_p]
	rng = np.random.default_rng(7)
	rows = [rng.integers(0, 256, n, dtype=np.uint8).tobytes() for n in (0, 1, 7, 8, 9, 63, 64, 65, 71, 1000, 100003, 3_000_001)]
	want = v2m.checksum_rows_host(rows).tolist()
	for threads, scalar in ((1, False), (2, False), (5, True), (16, False), (3, True)):      # the CPU's widest loop (AVX-512DQ where there is one) and the scalar one
		s = sl.v2ms_checksum_sink_create(len(rows), threads)
		assert sl.v2ms_checksum_sink_flavour(s) in (b"scalar", b"avx512dq")
		if scalar:
			sl.v2ms_checksum_sink_force_scalar(s)
			assert sl.v2ms_checksum_sink_flavour(s) == b"scalar"
		for rep in range(3):            # the pool is reused row after row
			for i, body in enumerate(rows):
				assert sl.v2ms_checksum_sink_fn(s, i, body, len(body)) == 0
		assert sl.v2ms_checksum_sink_fn(s, len(rows), b"", 0) != 0     # a row index beyond the capacity is refused
		assert [sl.v2ms_checksum_sink_checksums(s)[i] for i in range(len(rows))] == want
		assert [sl.v2ms_checksum_sink_lengths(s)[i] for i in range(len(rows))] == [len(b) for b in rows]
		assert sl.v2ms_checksum_sink_rows(s) == 3 * len(rows)
		sl.v2ms_checksum_sink_destroy(s)


def test_ring_transpose_indexing_model():
	"""tools/ring_transpose_model.py: the ring transpose kernel's slot / flush / window indexing, replayed on the CPU, writes
	every destination word exactly once with the right value on awkward shapes (the GPU suite then checks the real kernel)."""
	import subprocess
	import sys
	ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
	r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ring_transpose_model.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
	assert r.returncode == 0, r.stderr.decode()[-2000:]
	assert b"cases ok" in r.stdout


def test_lines_transpose_indexing_model():
	"""tools/lines_transpose_model.py: the whole-line transpose kernel's carried block, slab layout, span directions, store guards
	and merged column ends, replayed on the CPU: every destination word written exactly once with the right value, nothing
	outside the matrix (the GPU suite then checks the real kernel)."""
	import subprocess
	import sys
	ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
	r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "lines_transpose_model.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
	assert r.returncode == 0, r.stderr.decode()[-2000:]
	assert b"cases ok" in r.stdout and b"with merged column ends" in r.stdout


def test_rot_transpose_indexing_model():
	"""tools/rot_transpose_model.py: the rotating-line transpose kernel's register file, line ends, span bounds and guarded first / last lines,
	replayed on the CPU: every destination word written exactly once, from the right register, whole lines line-aligned."""
	import subprocess
	import sys
	r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rot_transpose_model.py")], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
	assert r.returncode == 0, r.stderr.decode()[-2000:]
	assert b"every destination word written once" in r.stdout


def test_bench_refuses_a_world_size_that_contradicts_gpus():
	import subprocess
	import sys
	env = dict(os.environ, WORLD_SIZE="3", RANK="0", LOCAL_RANK="0")
	r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"), "--gpus", "2"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)
	assert r.returncode != 0 and b"WORLD_SIZE (3) != --gpus (2)" in r.stderr and not r.stdout.strip()


def test_bench_has_full_and_dump_outputs_options():
	import subprocess
	import sys
	r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=_clean_env())
	assert r.returncode == 0, r.stderr.decode()
	assert b"--full" in r.stdout and b"--dump-outputs DIR" in r.stdout


def test_bench_dump_sample_is_fixed_and_in_bounds():
	"""--dump-outputs samples the same windows of the last batch's rows whenever the workload is the same, and never reads past a row."""
	import bench
	for n_rows, length in ((620, 100299831), (31, 2000003), (1, 5000), (3, 16384)):
		picks, width = bench.sample_windows(n_rows, length)
		again, _ = bench.sample_windows(n_rows, length)
		assert np.array_equal(picks, again) and width == min(length, bench.DUMP_WINDOW_BYTES)
		assert len(picks) == bench.DUMP_WINDOWS and (picks[:, 0] >= 0).all() and (picks[:, 0] < n_rows).all()
		assert (picks[:, 1] >= 0).all() and (picks[:, 1] + width <= length).all()
		assert tuple(picks[0]) == (0, 0) and tuple(picks[-1]) == (n_rows - 1, length - width)
	assert len(bench.sample_windows(0, 1000)[0]) == 0 and len(bench.sample_windows(5, 0)[0]) == 0
	assert bench.DUMP_WINDOWS * bench.DUMP_WINDOW_BYTES * 4 < bench.DUMP_LIMIT_BYTES      # the float32 sample alone leaves room


def test_bench_write_outputs_takes_floats_within_the_limit(tmp_path):
	import bench
	bench.write_outputs(str(tmp_path / "d"), {"a": np.arange(6, dtype=np.float32).reshape(2, 3), "b": np.ones(4, dtype=np.float64)})
	assert np.array_equal(np.load(tmp_path / "d" / "a.npy"), np.arange(6, dtype=np.float32).reshape(2, 3))
	assert np.load(tmp_path / "d" / "b.npy").dtype == np.float64
	with pytest.raises(TypeError):
		bench.write_outputs(str(tmp_path / "e"), {"a": np.zeros(4, dtype=np.uint8)})
	with pytest.raises(ValueError):
		bench.write_outputs(str(tmp_path / "e"), {"a": np.zeros((64 << 20) // 8 + 1, dtype=np.float64)})
	assert not (tmp_path / "e").exists()


def test_build_native_writes_nothing_when_fresh(monkeypatch):
	"""A checkout that build() made may be used by a user who cannot write it: with every library up to date, build_native() does not even
	take its lock file."""
	from vcf2multialign_amd import build
	assert build.stale_targets() == []

	def no_lock():
		raise AssertionError("build_native() took its lock with nothing to build")
	monkeypatch.setattr(build, "_build_lock", no_lock)
	assert build.build_native() == build.LIB_PATH


def test_bench_uses_the_libraries_of_a_checkout_it_cannot_write(monkeypatch, tmp_path):
	"""bench.py's build step where the build lock cannot be taken (another user's checkout): the libraries build() left are used; without
	them the run ends with a message."""
	import bench
	from vcf2multialign_amd import build

	def refused(*a, **k):
		raise PermissionError(13, "Permission denied", os.path.join(build.PKG_DIR, ".build.lock"))
	monkeypatch.setattr(build, "build_native", refused)
	bench.build_libraries()
	monkeypatch.setattr(build, "LIB_PATH", str(tmp_path / "libv2m_hip.so"))
	with pytest.raises(SystemExit) as e:
		bench.build_libraries()
	assert "run build() first" in str(e.value)


def test_bench_as_typed_starts_child_ranks_and_relays_their_failure():
	"""`python bench.py --gpus 2` without WORLD_SIZE starts two child ranks itself (no GPU here: both fail at the first HIP call);
	the parent must relay the failure as a non-zero exit, print nothing on stdout and never exec over itself."""
	import subprocess
	import sys
	env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
	if os.path.exists("/dev/kfd"):
		pytest.skip("a GPU is present: the working path is covered by tests/test_gpu_bench.py")
	r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--config", "mini3"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, env=env)
	assert r.returncode != 0 and not r.stdout.strip()
	assert b"rank 0 -> exit" in r.stderr and b"rank 1 -> exit" in r.stderr
	with open(os.path.join(ROOT, "bench.py")) as f:
		assert "os.exec" not in f.read().replace("Never os.exec*", "")


def test_bench_numa_binding_is_a_subset_of_what_was_allowed_and_never_fatal():
	"""bench.py at N > 1 keeps a rank's host side on its GPU's NUMA node.  In a child process (the change is the
	process's own): node 0's CPUs, cut down to what the process was allowed before, or nothing at all when the node is unknown."""
	code = ("import os, sys, json; sys.path.insert(0, %r); import bench\n"
		"before = os.sched_getaffinity(0)\n"
		"print(json.dumps([bench.bind_to_numa_node(None), bench.bind_to_numa_node(-1), bench.bind_to_numa_node(4096), sorted(os.sched_getaffinity(0) ^ before)]))\n"
		"bound = bench.bind_to_numa_node(0)\n"
		"after = os.sched_getaffinity(0)\n"
		"print(json.dumps([bound, after <= before, len(after) > 0]))\n") % ROOT
	r = subprocess.run([sys.executable, "-c", code], stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=_clean_env())
	assert r.returncode == 0, r.stderr.decode()
	lines = [json.loads(l) for l in r.stdout.decode().strip().splitlines()]
	assert lines[0] == [None, None, None, []]                                      # unknown nodes change nothing
	assert lines[1][1] is True and lines[1][2] is True                              # a subset, never empty
	if os.path.exists("/sys/devices/system/node/node0/cpulist"):
		with open("/sys/devices/system/node/node0/cpulist") as f:
			assert lines[1][0] in (None, f.read().strip())
