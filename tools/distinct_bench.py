"""Distinct pieces of a window set (v2m_splice_window_set_distinct) against v2m_splice_window_set on the same set: a synthetic config
with sets of windows at seeded positions, every row of the config, aligned and unaligned.  Records per set
  - the device time of hash_pieces_kernel, gather_pieces_kernel and verify_pieces_kernel per slice (v2m_profile_get_launches),
  - hash_pieces_kernel's bytes/s beside checksum_rows_kernel's on the same records (the existing kernel with the same arithmetic;
    v2m_checksum_rows_device over a buffer of the first --yardstick-rows records, wall time of the synchronous call),
  - the pieces, the distinct pieces and the bytes over the link with and without distinct,
  - the host-to-host time of both calls with sinks that only return.
The sets: --sets WINDOWSxCOLUMNS,... (default 200x50000, the BED-like set, and 2000x500, short windows in which rows do repeat).
The pool limit is raised for the measurement (V2M_DISTINCT_POOL_BYTES, 96 GiB unless set): on the synthetic configs every row of a
50-kb window is distinct, so the pool holds as much as the link would have carried.
Prints one JSON line and, with --out, writes it (profiles/r10/distinct_bench.json).

  python tools/distinct_bench.py [--config config3] [--sets 200x50000,2000x500] [--rows N] [--repeats 2] [--out profiles/r10/distinct_bench.json]
"""

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--config", default="config3")
	ap.add_argument("--sets", default="200x50000,2000x500")
	ap.add_argument("--rows", type=int, default=0, help="0 = REF and every copy")
	ap.add_argument("--yardstick-rows", type=int, default=256)
	ap.add_argument("--repeats", type=int, default=2)
	ap.add_argument("--out")
	args = ap.parse_args()
	os.environ.setdefault("V2M_DISTINCT_POOL_BYTES", str(96 << 30))
	import torch
	import vcf2multialign_amd as v2m
	from vcf2multialign_amd import _native as N, synth

	ds = synth.dataset(args.config)
	g = ds.graph
	L = g.aligned_length
	dev = torch.device("cuda", 0)
	ctx = v2m.Context(0)
	lib = ctx._lib
	ctx.upload_graph(g, ds.reference)
	thr = torch.from_numpy(ds.edge_thresholds.astype(np.int64)).to(torch.int32).to(dev)
	src = torch.empty(ds.path_rows // 64 * ds.path_cols, dtype=torch.int64, device=dev)
	torch.cuda.synchronize()
	ds.fill_paths_device(ctx.stream, src.data_ptr(), thr.data_ptr(), 0, ds.path_cols)
	ctx.bind_path_matrix_device(src.data_ptr(), ds.path_cols, ds.path_rows)
	ctx.synchronize()
	del src
	torch.cuda.empty_cache()
	rows = [v2m.PLOIDY_MAX] + list(range(ds.n_copies))
	if args.rows:
		rows = rows[:args.rows]
	batch = v2m.RowBatch(rows)
	R = len(rows)
	rng = np.random.default_rng(10)
	# sinks for the timed calls that cost nothing: libc's atoi on user = "0" returns 0 whatever else is passed
	libc = C.CDLL(None)
	zero = C.c_char_p(b"0")
	window_idle, distinct_idle = C.cast(libc.atoi, N.WINDOW_SINK_FN), C.cast(libc.atoi, N.DISTINCT_SINK_FN)
	no_sink = C.cast(None, N.DISTINCT_SINK_FN)

	def wall(fn):
		ctx.synchronize()
		t0 = time.perf_counter()
		fn()
		ctx.synchronize()
		return (time.perf_counter() - t0) * 1e3

	def measure_mode(W, unaligned):
		flags = N.V2M_SPLICE_UNALIGNED if unaligned else 0
		plain = {"bytes": 0}
		seen = {"classes": 0, "bytes": 0}

		def window_sink(_user, _row, _record, lengths):
			plain["bytes"] += int(np.ctypeslib.as_array(lengths, (W,)).sum(dtype=np.uint64))
			return 0

		def distinct_sink(_user, _window, _class, _first_row, _bytes, length):
			seen["classes"] += 1
			seen["bytes"] += length
			return 0
		class_of = np.zeros(R * W, dtype=np.uint32)
		counts = np.zeros(W, dtype=np.uint32)

		def plain_call(sink=window_idle):
			assert lib.v2m_splice_window_set(ctx._h, C.byref(batch.struct), flags, sink, zero) == 0, lib.v2m_last_error(ctx._h)

		def distinct_call(sink=distinct_idle):
			assert lib.v2m_splice_window_set_distinct(ctx._h, C.byref(batch.struct), flags, sink, zero, class_of.ctypes.data, counts.ctypes.data) == 0, lib.v2m_last_error(ctx._h)

		plain_call(N.WINDOW_SINK_FN(window_sink))        # warm-up (pinned slots, scratch growth, the unaligned template), and the bytes counted
		distinct_call(N.DISTINCT_SINK_FN(distinct_sink))
		plain_ms = min(wall(plain_call) for _ in range(args.repeats))
		ctx.profile_reset()
		ctx.profile_enable(True)
		distinct_ms = wall(distinct_call)
		per_slice = {name: [round(float(x), 4) for x in ctx.profile_launches(k)] for name, k in
			(("hash", N.KERNEL_DISTINCT_HASH), ("gather", N.KERNEL_DISTINCT_GATHER), ("verify", N.KERNEL_DISTINCT_VERIFY))}
		splice_ms = sum(ctx.profile_get(k)[1] for k in (N.KERNEL_RESOLVE, N.KERNEL_SPLICE_UNALIGNED if unaligned else N.KERNEL_SPLICE_ALIGNED, N.KERNEL_UNALIGNED_COUNT))
		ctx.profile_enable(False)
		distinct_ms = min([distinct_ms] + [wall(distinct_call) for _ in range(args.repeats - 1)])
		tables_only_ms = min(wall(lambda: distinct_call(no_sink)) for _ in range(args.repeats))
		hash_ms = sum(per_slice["hash"])
		return {"pieces": R * W, "distinct_pieces": int(counts.sum()), "max_classes_of_a_window": int(counts.max()),
			"bytes_over_the_link_plain": plain["bytes"], "bytes_over_the_link_distinct": seen["bytes"],
			"splice_window_set_wall_ms": round(plain_ms, 2), "distinct_wall_ms": round(distinct_ms, 2), "distinct_tables_only_wall_ms": round(tables_only_ms, 2),
			"slices": len(per_slice["hash"]), "device_ms_per_slice": per_slice, "splice_device_ms": round(splice_ms, 3),
			"hash_device_ms": round(hash_ms, 3), "hash_GBps": round(plain["bytes"] / hash_ms / 1e6, 1) if hash_ms else None}

	def measure_yardstick(W, columns, offsets, pitch):
		"""checksum_rows_kernel over the first records, each record's slots read as one row, beside hash_pieces_kernel on the same rows."""
		yr = min(args.yardstick_rows, R)
		slots_end = offsets[-1] + (columns + 15) // 16 * 16
		buf = torch.empty(yr * pitch, dtype=torch.uint8, device=dev)
		ctx.splice_window_set_device(rows[:yr], buf.data_ptr(), pitch)
		ctx.synchronize()
		ctx.checksum_rows_device(buf.data_ptr(), pitch, yr, length=slots_end)
		checksum_ms = min(wall(lambda: ctx.checksum_rows_device(buf.data_ptr(), pitch, yr, length=slots_end)) for _ in range(max(3, args.repeats)))
		yard_batch = v2m.RowBatch(rows[:yr])
		class_of = np.zeros(yr * W, dtype=np.uint32)
		ctx.profile_reset()
		ctx.profile_enable(True)
		assert lib.v2m_splice_window_set_distinct(ctx._h, C.byref(yard_batch.struct), 0, no_sink, None, class_of.ctypes.data, None) == 0
		hash_ms = ctx.profile_get(N.KERNEL_DISTINCT_HASH)[1]
		ctx.profile_enable(False)
		return {"rows": yr, "bytes": yr * W * columns, "checksum_rows_device_wall_ms": round(checksum_ms, 3), "checksum_GBps": round(yr * slots_end / checksum_ms / 1e6, 1),
			"hash_pieces_device_ms": round(hash_ms, 3), "hash_GBps": round(yr * W * columns / hash_ms / 1e6, 1)}

	def measure(n_windows, columns):
		windows = [(int(b), int(b) + columns) for b in rng.integers(0, L - columns, size=n_windows)]
		ctx.set_window_set(windows)
		offsets, pitch = ctx.window_set_layout
		out = {"windows": n_windows, "columns_each": columns, "record_pitch": pitch}
		for unaligned in (False, True):
			out["unaligned" if unaligned else "aligned"] = measure_mode(n_windows, unaligned)
		out["hash_against_checksum_kernel"] = measure_yardstick(n_windows, columns, offsets, pitch)
		return out

	sets = [measure(*(int(x) for x in spec.split("x"))) for spec in args.sets.split(",")]
	ctx.close()
	record = {"metric": "window set: distinct pieces found in HBM against every piece over the link", "config": args.config, "aligned_length": L, "edges": g.edge_count,
		"rows": R, "pool_limit_bytes": int(os.environ["V2M_DISTINCT_POOL_BYTES"]), "sets": sets}
	text = json.dumps(record)
	print(text)
	if args.out:
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, "w") as f:
			f.write(text + "\n")


if __name__ == "__main__":
	main()
