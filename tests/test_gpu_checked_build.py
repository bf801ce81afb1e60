"""The parity corpus on the checked build (libv2m_hip_checked.so + libv2m_host_checked.so, built by build_native() with -DV2M_CHECKED_BUILD).

Every other GPU test compares bytes with the oracle, which catches wrong logic but hardly a read of memory nobody wrote: a workgroup's LDS
holds what the previous workgroup on the CU left there, and the context's scratch, device slots and pinned slots hold what the previous
call or slice wrote -- usually data of the right shape, often the right answer.  The checked build fills all of it with a seeded pattern
before use (kernels.hpp: V2M_POISON_LDS; v2m_hip.hip: scratch_buf, V2M_POISON_HOST), so such a read changes output bytes here.

The corpus is the existing tests themselves, run by pytest in a child process per seed (the parent has the product library loaded):
reference fixtures and founder goldens, 32 fuzz seeds, dense iid path bits, the cache-limit graphs whole and windowed, window classes in
all four forms, batches of more than 300 rows, the resolve queue's overflow branch, the BGZF encoder against tests/deflate_ref.py at its
edges, founder cut positions against the host's search and the founder kernels' raw pairs and records against a plain pBWT, the
transposes, path slices and blocks, device checksums.  The second seed runs
only if the first passed; the child checks that only the checked builds are mapped."""

import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

SEEDS = ["0x2545f491", "0x9b05688c"]

CORPUS = [
	"tests/test_gpu_parity.py::test_haplotype_a2m_fixtures",
	"tests/test_gpu_parity.py::test_founder_a2m_goldens",
	"tests/test_gpu_parity.py::test_fuzz_small_graphs",                     # V2M_FUZZ_SEEDS below
	"tests/test_gpu_parity.py::test_random_path_bits_skip_rule",
	"tests/test_gpu_parity.py::test_extreme_spans_and_cache_limits",
	"tests/test_gpu_parity.py::test_resolve_queue_capacity",
	"tests/test_gpu_parity.py::test_more_rows_than_one_grid_dimension",
	"tests/test_gpu_parity.py::test_founder_rows_many_segments",
	"tests/test_gpu_parity.py::test_transpose_random",
	"tests/test_gpu_parity.py::test_bind_path_matrix_device",
	"tests/test_gpu_parity.py::test_path_slices_reproduce_every_row",
	"tests/test_gpu_parity.py::test_path_blocks_dealt_round_robin",
	"tests/test_gpu_parity.py::test_device_rows_checksums",
	"tests/test_gpu_parity.py::test_sink_slices",
	"tests/test_gpu_parity.py::test_held_rows_stay_valid_until_released",
	"tests/test_gpu_window.py::test_reference_fixtures",
	"tests/test_gpu_window.py::test_synthetic_random_paths",                # window classes; every 8th seed in all four forms
	"tests/test_gpu_window.py::test_founder_rows_with_cuts",
	"tests/test_gpu_window.py::test_serial_resolve_restart",
	"tests/test_gpu_window.py::test_window_store_flavours_forced",
	"tests/test_gpu_window.py::test_batches_of_many_rows",
	"tests/test_gpu_window.py::test_cache_limits_under_windows",
	"tests/test_gpu_window.py::test_resolve_queue_capacity_windowed",
	"tests/test_gpu_bgzf.py::test_exact_piece_sizes",
	"tests/test_gpu_bgzf.py::test_exact_runs_at_segment_edges",
	"tests/test_gpu_bgzf.py::test_exact_byte_values",
	"tests/test_gpu_bgzf.py::test_exact_limiters",
	"tests/test_gpu_bgzf.py::test_fixture_rows",
	"tests/test_gpu_bgzf.py::test_synthetic_rows",
	"tests/test_gpu_founders.py::test_reference_cut_positions",
	"tests/test_gpu_founders.py::test_random_inputs",
	"tests/test_gpu_founders.py::test_chunks_the_gpu_leaves_undone_are_walked_on_the_host",
	"tests/test_gpu_founders.py::test_streamed_and_array_form_of_the_chunk_walks_agree",
	"tests/test_gpu_founders.py::test_every_copies_per_thread_instantiation[2200_copies]",
	"tests/test_gpu_founders.py::test_every_copies_per_thread_instantiation[9400_copies]",
	# what the founder kernels write, value for value: the copy counts below 2100 and one of 16 copies per thread, the bin limit, both hash tables
	"tests/test_gpu_founder_kernels.py::test_copy_counts_at_every_seam[1]",
	"tests/test_gpu_founder_kernels.py::test_copy_counts_at_every_seam[2]",
	"tests/test_gpu_founder_kernels.py::test_copy_counts_at_every_seam[63]",
	"tests/test_gpu_founder_kernels.py::test_copy_counts_at_every_seam[64]",
	"tests/test_gpu_founder_kernels.py::test_copy_counts_at_every_seam[65]",
	"tests/test_gpu_founder_kernels.py::test_copy_counts_at_every_seam[1023]",
	"tests/test_gpu_founder_kernels.py::test_copy_counts_at_every_seam[1024]",
	"tests/test_gpu_founder_kernels.py::test_copy_counts_at_every_seam[1025]",
	"tests/test_gpu_founder_kernels.py::test_copy_counts_at_every_seam[2047]",
	"tests/test_gpu_founder_kernels.py::test_copy_counts_at_every_seam[2048]",
	"tests/test_gpu_founder_kernels.py::test_copy_counts_at_every_seam[2049]",
	"tests/test_gpu_founder_kernels.py::test_copy_counts_at_every_seam[16384]",
	"tests/test_gpu_founder_kernels.py::test_bin_limits",
	"tests/test_gpu_founder_kernels.py::test_hash_collisions_in_both_tables",
	"tests/test_gpu_founder_kernels.py::test_capacities",
	"tests/test_gpu_founder_kernels.py::test_chunkings_the_host_never_makes",
	"tests/test_gpu_founder_kernels.py::test_min_distance",
	"tests/test_gpu_founder_kernels.py::test_streamed_form",
	"tests/test_gpu_founder_kernels.py::test_cut_lists_the_search_never_produces",
]

CHILD = r"""
import os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests")]
import pytest
from vcf2multialign_amd import _native, host
assert _native.library_path() == os.environ["V2M_HIP_LIBRARY"] and host.library_path() == os.environ["V2M_HOST_LIBRARY"]
import vcf2multialign_amd as v2m
with v2m.Context(0) as ctx:
	assert "checked build: poison seed 0x%%08x" %% int(os.environ["V2M_POISON_SEED"], 0) in ctx.info, ctx.info
rc = pytest.main(["-q", "-x", "-m", "gpu", "-p", "no:cacheprovider", "--rootdir", %(root)r] + %(corpus)r)
with open("/proc/self/maps") as f:
	mapped = sorted({l.split()[-1] for l in f if "libv2m_" in l})
print("mapped:", " ".join(mapped))
assert os.environ["V2M_HIP_LIBRARY"] in mapped, mapped
assert all(m == os.environ["V2M_HOST_LIBRARY"] for m in mapped if os.path.basename(m).startswith("libv2m_host")), mapped
assert not [m for m in mapped if os.path.basename(m) in ("libv2m_hip.so", "libv2m_hip_tuning.so", "libv2m_host.so")], mapped
sys.exit(int(rc))
"""

KNOBS = ("V2M_NT_STORES", "V2M_UNALIGNED_STORE", "V2M_ROWS_PER_GROUP", "V2M_COUNT_ROWS_PER_GROUP", "V2M_MAX_BACK_WORDS", "V2M_RESOLVE_QUEUE_CAPACITY",
	"V2M_TRANSPOSE_PANEL", "V2M_RING_SLOT_BYTES")


def run_checked_corpus(seed, hip_library, host_library, corpus=CORPUS, timeout=900):
	"""Runs `corpus` (test ids relative to the repository) in a child process on the given checked libraries with V2M_POISON_SEED=seed;
	returns (exit status, output)."""
	env = dict(os.environ, V2M_HIP_LIBRARY=hip_library, V2M_HOST_LIBRARY=host_library, V2M_POISON_SEED=seed, V2M_FUZZ_SEEDS="32")
	for knob in KNOBS:
		env.pop(knob, None)
	code = CHILD % {"root": ROOT, "corpus": [os.path.join(ROOT, c) for c in corpus]}
	r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout, env=env)
	return r.returncode, r.stdout.decode(errors="replace")


def test_parity_corpus_on_the_checked_build():
	from vcf2multialign_amd import build
	assert os.path.exists(build.CHECKED_LIB_PATH) and os.path.exists(build.CHECKED_HOST_LIB_PATH), "build_native() builds them"
	for seed in SEEDS:   # the second seed only once the first has passed
		rc, out = run_checked_corpus(seed, build.CHECKED_LIB_PATH, build.CHECKED_HOST_LIB_PATH)
		assert rc == 0, "checked build, seed %s: exit %d\n%s" % (seed, rc, out[-6000:])
		assert " passed" in out and "libv2m_host_checked.so" in out, out[-3000:]   # the founder tests drove the checked host library
		print(seed, out.strip().splitlines()[-2])
