"""Window sets (v2m_set_window_set) against the same windows set one by one (v2m_set_column_window), on a synthetic config: sets of
many short windows at seeded positions, a batch of rows (REF + the first copies) spliced into HBM, aligned and unaligned.  Per
set: the wall time of v2m_set_window_set, the wall and device time (v2m_profile_*: resolve + splice + unaligned count) of the one
row call, the bytes written; and the wall time per window of the loop "set_column_window, splice_rows_device" over a sample of the
set's windows, scaled to the whole set.  Prints one JSON line and, with --out, writes it (profiles/r08/window_set_bench.json).

  python tools/window_set_bench.py [--config config3] [--rows 512] [--repeats 3] [--loop-sample 200] [--out profiles/r08/window_set_bench.json]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETS = ((20_000, 300), (2_000, 3_000), (200, 30_000), (20, 300_000))   # (windows, columns each): 6 MB of columns per row every time


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--config", default="config3")
	ap.add_argument("--rows", type=int, default=512)
	ap.add_argument("--repeats", type=int, default=3)
	ap.add_argument("--loop-sample", type=int, default=200)
	ap.add_argument("--out")
	args = ap.parse_args()
	import torch
	import vcf2multialign_amd as v2m
	from vcf2multialign_amd import _native as N, synth

	ds = synth.dataset(args.config)
	g = ds.graph
	L = g.aligned_length
	dev = torch.device("cuda", 0)
	ctx = v2m.Context(0)
	ctx.upload_graph(g, ds.reference)
	thr = torch.from_numpy(ds.edge_thresholds.astype(np.int64)).to(torch.int32).to(dev)
	src = torch.empty(ds.path_rows // 64 * ds.path_cols, dtype=torch.int64, device=dev)
	torch.cuda.synchronize()
	ds.fill_paths_device(ctx.stream, src.data_ptr(), thr.data_ptr(), 0, ds.path_cols)
	ctx.bind_path_matrix_device(src.data_ptr(), ds.path_cols, ds.path_rows)
	ctx.synchronize()
	del src
	torch.cuda.empty_cache()
	rows = ([v2m.PLOIDY_MAX] + list(range(ds.n_copies)))[:args.rows]
	rng = np.random.default_rng(8)

	def timed(fn):
		ctx.synchronize()
		t0 = time.perf_counter()
		fn()
		ctx.synchronize()
		return (time.perf_counter() - t0) * 1e3

	def device_ms(unaligned):
		kernels = [N.KERNEL_RESOLVE, N.KERNEL_SPLICE_UNALIGNED if unaligned else N.KERNEL_SPLICE_ALIGNED] + ([N.KERNEL_UNALIGNED_COUNT] if unaligned else [])
		return sum(ctx.profile_get(k)[1] for k in kernels)

	results = []
	for n_windows, columns in SETS:
		if columns >= L:
			continue
		begins = rng.integers(0, L - columns, size=n_windows)
		windows = [(int(b), int(b) + columns) for b in begins]
		entry = {"windows": n_windows, "columns_each": columns, "rows": len(rows)}
		entry["set_window_set_ms"] = round(min(timed(lambda: ctx.set_window_set(windows)) for _ in range(args.repeats)), 3)
		_, pitch = ctx.window_set_layout
		out = torch.empty(len(rows) * pitch, dtype=torch.uint8, device=dev)
		for unaligned in (False, True):
			call = lambda: ctx.splice_window_set_device(rows, out.data_ptr(), pitch, unaligned=unaligned)
			call()   # warm-up: scratch growth, the unaligned template
			best = None
			for _ in range(args.repeats):
				ctx.profile_reset()
				ctx.profile_enable(True)
				wall = timed(call)
				dev_ms = device_ms(unaligned)
				ctx.profile_enable(False)
				if best is None or wall < best[0]:
					best = (wall, dev_ms)
			# the same windows one by one, a sample of them, scaled to the set
			sample = windows[:min(args.loop_sample, n_windows)]
			row_pitch = (columns + 255) // 256 * 256

			def loop():
				for b, e in sample:
					ctx.set_column_window(b, e)
					ctx.splice_rows_device(rows, out.data_ptr(), row_pitch, unaligned=unaligned)
			loop()
			loop_ms = min(timed(loop) for _ in range(args.repeats)) * n_windows / len(sample)
			ctx.set_column_window(0, L)
			entry["unaligned" if unaligned else "aligned"] = {"set_call_wall_ms": round(best[0], 3), "set_call_device_ms": round(best[1], 3),
				"bytes": len(rows) * n_windows * columns if not unaligned else None, "one_by_one_wall_ms_scaled": round(loop_ms, 3),
				"one_by_one_sampled_windows": len(sample)}
		del out
		results.append(entry)
	ctx.close()
	record = {"metric": "window set: one row call over all windows against one call per window, rows into HBM", "config": args.config,
		"aligned_length": L, "edges": g.edge_count, "results": results}
	text = json.dumps(record)
	print(text)
	if args.out:
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, "w") as f:
			f.write(text + "\n")


if __name__ == "__main__":
	main()
