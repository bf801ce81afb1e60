"""Column windows (v2m_set_column_window) on the synthetic configs: for windows of 10 kb, 100 kb, 1 Mb and 10 Mb of reference at the
start, middle and end of the chromosome, every row (REF + all copies) spliced into HBM, aligned and unaligned, with the resolve and
splice device times (v2m_profile_*), the bytes written and their share of the 8 TB/s peak; next to the whole-row step (resolve +
aligned splice per row) measured in the same process.  Prints one JSON line.

  python tools/window_bench.py [--configs config3,config5] [--repeats 3]
"""

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_GBPS = 8000.0
WINDOWS = (10_000, 100_000, 1_000_000, 10_000_000)
MAX_OUT_BYTES = 24 << 30   # rows per launch are cut so that one launch writes at most this much


def run_config(name, repeats, v2m, N, synth, torch):
	ds = synth.dataset(name)
	g = ds.graph
	L, R = g.aligned_length, len(ds.reference)
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
	rows = [v2m.PLOIDY_MAX] + list(range(ds.n_copies))
	out = torch.empty(MAX_OUT_BYTES, dtype=torch.uint8, device=dev)

	def step(unaligned):
		"""All rows once; returns (resolve ms, splice ms incl. the unaligned count pass, bytes written)."""
		pitch = (ctx.max_unaligned_length + 255) // 256 * 256 if unaligned else ctx.min_row_pitch
		per = max(1, MAX_OUT_BYTES // pitch)
		ctx.profile_reset()
		ctx.profile_enable(True)
		written = 0
		for r0 in range(0, len(rows), per):
			part = rows[r0:r0 + per]
			lengths = ctx.splice_rows_device(part, out.data_ptr(), pitch, unaligned=unaligned, want_lengths=unaligned)
			written += int(lengths.sum()) if unaligned else len(part) * ctx.window_length
		ctx.synchronize()
		_, resolve = ctx.profile_get(N.KERNEL_RESOLVE)
		splice = ctx.profile_get(N.KERNEL_SPLICE_UNALIGNED if unaligned else N.KERNEL_SPLICE_ALIGNED)[1]
		count = ctx.profile_get(N.KERNEL_UNALIGNED_COUNT)[1] if unaligned else 0.0
		ctx.profile_enable(False)
		return resolve, splice, count, written

	def best(unaligned):
		step(unaligned)   # warm-up (store calibration, scratch growth)
		runs = [step(unaligned) for _ in range(repeats)]
		return min(runs, key=lambda r: r[0] + r[1] + r[2])

	def record(resolve, splice, count, written):
		return {"resolve_ms": round(resolve, 4), "splice_ms": round(splice, 4), "count_ms": round(count, 4), "device_ms": round(resolve + splice + count, 4),
			"bytes": written, "splice_GBps": round(written / splice / 1e6, 1) if splice else None,
			"splice_frac_of_peak": round(written / splice / 1e6 / PEAK_GBPS, 4) if splice else None}

	# the whole-row step on a batch of rows, scaled to all rows (a full step of config 5 writes 5 TB)
	whole_rows = rows[:min(len(rows), max(1, MAX_OUT_BYTES // ctx.min_row_pitch))]
	saved = rows
	rows = whole_rows
	whole = record(*best(False))
	rows = saved
	scale = len(rows) / len(whole_rows)
	whole_all = {"rows_measured": len(whole_rows), "device_ms_all_rows": round(whole["device_ms"] * scale, 3), **whole}

	results = []
	for size in WINDOWS:
		if size > R:
			continue
		for where, s in (("start", 0), ("middle", R // 2 - size // 2), ("end", R - size)):
			b, e = g.columns_of_reference_range(s, s + size)
			ctx.set_column_window(b, e)
			entry = {"reference_bases": size, "where": where, "range": [s, s + size], "columns": [b, e]}
			entry["aligned"] = record(*best(False))
			entry["unaligned"] = record(*best(True))
			if entry["aligned"]["splice_GBps"] and whole["splice_GBps"]:
				entry["aligned"]["splice_rate_vs_whole_row"] = round(entry["aligned"]["splice_GBps"] / whole["splice_GBps"], 3)
			results.append(entry)
			ctx.set_column_window(0, L)
	ctx.close()
	return {"config": name, "rows": len(rows), "aligned_length": L, "reference_length": R, "edges": g.edge_count, "whole_row_step": whole_all, "windows": results}


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--configs", default="config3,config5")
	ap.add_argument("--repeats", type=int, default=3)
	args = ap.parse_args()
	import torch
	import vcf2multialign_amd as v2m
	from vcf2multialign_amd import _native as N, synth
	out = {"metric": "column window resolve + splice device time, all rows, HBM-resident", "peak_GBps": PEAK_GBPS,
		"results": [run_config(c, args.repeats, v2m, N, synth, torch) for c in args.configs.split(",")]}
	print(json.dumps(out))


if __name__ == "__main__":
	main()
