"""Column counts (v2m_column_counts[_device]) on a synthetic config, all rows (REF + every copy), over the whole row and over a 100-kb
window: the device time of column_counts_kernel per slice (v2m_profile_get_launches) beside splice_aligned_kernel's for the same slices; the
select passes; the calls host to host -- the device form and both sink forms, alternated, best of --repeats with every repeat recorded --;
the records and bytes that cross the link.  The yardstick is checksum_rows_kernel (v2m_checksum_rows_device) over one slice's rows in HBM,
which reads exactly the bytes column_counts_kernel reads, timed between events on the context's stream.
With --check the window's counts, and the whole view's counts at the window's columns, are held equal to counts taken on the host from the
rows v2m_splice_rows delivers for the same window.
Prints one JSON line and, with --out, writes it (profiles/r12/column_counts_bench.json).

  python tools/column_counts_bench.py [--config config3] [--window 100000] [--repeats 3] [--check] [--out profiles/r12/column_counts_bench.json]
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
	ap.add_argument("--window", type=int, default=100000)
	ap.add_argument("--repeats", type=int, default=3)
	ap.add_argument("--views", default="whole,window")
	ap.add_argument("--check", action="store_true")
	ap.add_argument("--out")
	args = ap.parse_args()
	import torch
	import vcf2multialign_amd as v2m
	from vcf2multialign_amd import _native as N, synth

	ds = synth.dataset(args.config)
	g = ds.graph
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
	batch = v2m.RowBatch(rows)
	stream = torch.cuda.ExternalStream(ctx.stream)
	KERNELS = {"resolve": N.KERNEL_RESOLVE, "splice_aligned": N.KERNEL_SPLICE_ALIGNED, "column_counts": N.KERNEL_COLUMN_COUNTS, "column_select": N.KERNEL_COLUMN_SELECT}

	def profiled(fn):
		ctx.synchronize()
		ctx.profile_reset()
		ctx.profile_enable(True)
		t0 = time.perf_counter()
		result = fn()
		ctx.synchronize()
		wall = (time.perf_counter() - t0) * 1e3
		got = {name: ctx.profile_get(k) for name, k in KERNELS.items()}
		per_slice = {name: np.asarray(ctx.profile_launches(KERNELS[name])) for name in ("splice_aligned", "column_counts")}
		ctx.profile_enable(False)
		return {"host_to_host_ms": round(wall, 3), "device_ms": {k: round(ms, 4) for k, (_, ms) in got.items()}, "launches": {k: int(n) for k, (n, _) in got.items()},
			"per_slice_ms": {k: {"min": round(float(v.min()), 4), "median": round(float(np.median(v)), 4), "max": round(float(v.max()), 4)} for k, v in per_slice.items() if v.size}}, result

	def sink_call(flags):
		seen = [0, 0]
		def cb(_user, _records, n):
			seen[0] += n
			seen[1] += 1
			return 0
		rc = ctx._lib.v2m_column_counts(ctx._h, C.byref(batch.struct), flags, N.COLUMN_COUNTS_SINK_FN(cb), None)
		ctx._check(rc)
		return {"records": seen[0], "blocks": seen[1]}

	results = {}
	L_whole = ctx.aligned_length
	window_begin = (L_whole // 2) // 16 * 16 + 5
	whole_at_window = None          # the whole view's counts at the window's columns (the whole view takes the staged form: five rows a slice)
	for view in args.views.split(","):
		if "window" == view:
			ctx.set_column_window(window_begin, min(L_whole, window_begin + args.window))
		else:
			ctx.set_column_window(0, L_whole)
		L = ctx.window_length
		pitch = (L + 3) // 4 * 4
		table = torch.zeros(6 * pitch, dtype=torch.int32, device=dev)
		legs = {"device_form": lambda: ctx.column_counts_device(batch, table.data_ptr(), pitch), "sink_all_columns": lambda: sink_call(0),
			"sink_variable_only": lambda: sink_call(N.COUNTS_VARIABLE_ONLY)}
		warm = v2m.RowBatch(rows[:8])
		ctx.column_counts_device(warm, table.data_ptr(), pitch)          # warm-up: scratch, the device slot, the pinned slots
		ctx._check(ctx._lib.v2m_column_counts(ctx._h, C.byref(warm.struct), 0, N.COLUMN_COUNTS_SINK_FN(lambda _u, _r, _n: 0), None))
		runs = {name: [] for name in legs}
		for _ in range(args.repeats):          # alternated
			for name, fn in legs.items():
				rec, extra = profiled(fn)
				rec.update(extra or {"records": 0, "blocks": 0})
				rec["bytes_over_the_link"] = 32 * rec["records"] + 8 * rec["launches"]["column_select"]          # the records, and a range's total before them
				runs[name].append(rec)
		out = {"columns": int(L), "rows": len(rows)}
		if "whole" == view:
			whole_at_window = table.view(6, pitch)[:, window_begin:window_begin + args.window].cpu().numpy().view(np.uint32).T.copy()
		for name, recs in runs.items():
			best = min(recs, key=lambda r: r["host_to_host_ms"])
			out[name] = dict(best, host_to_host_ms_all=[r["host_to_host_ms"] for r in recs], column_counts_device_ms_all=[r["device_ms"]["column_counts"] for r in recs])
		# the yardstick on one slice: a full slice's rows in HBM (the library's rule: slots of 512 MiB for batches of 8 GiB and more, else of
		# 128 MiB), checksum_rows_kernel over them between events; column_counts_kernel's time for such a slice is the median launch above
		row_pitch = ctx.min_row_pitch
		slot = (512 << 20) if len(rows) * row_pitch >= (8 << 30) else (128 << 20)
		slice_rows = max(1, min(len(rows), slot // row_pitch))
		assert (len(rows) + slice_rows - 1) // slice_rows == out["device_form"]["launches"]["column_counts"]
		buf = torch.empty(slice_rows * row_pitch, dtype=torch.uint8, device=dev)
		ctx.splice_rows_device(v2m.RowBatch(rows[:slice_rows]), buf.data_ptr(), row_pitch)
		ctx.synchronize()
		ctx.checksum_rows_device(buf.data_ptr(), row_pitch, slice_rows, length=L)
		check_ms = []
		for _ in range(args.repeats):
			e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
			e0.record(stream)
			ctx.checksum_rows_device(buf.data_ptr(), row_pitch, slice_rows, length=L)
			e1.record(stream)
			e1.synchronize()
			check_ms.append(e0.elapsed_time(e1))
		count_ms = [r["per_slice_ms"]["column_counts"]["median"] for r in runs["device_form"]]
		splice_ms = [r["per_slice_ms"]["splice_aligned"]["median"] for r in runs["device_form"]]
		out["one_slice"] = {"rows": slice_rows, "bytes_read": int(slice_rows * L), "checksum_rows_ms": [round(x, 4) for x in check_ms], "column_counts_ms": count_ms, "splice_aligned_ms": splice_ms,
			"checksum_GBps": round(slice_rows * L / min(check_ms) / 1e6, 1), "column_counts_GBps": round(slice_rows * L / min(count_ms) / 1e6, 1),
			"column_counts_over_checksum": round(min(count_ms) / min(check_ms), 3), "column_counts_over_splice_aligned": round(min(count_ms) / min(splice_ms), 3),
			"table_bytes": int(6 * 4 * L)}
		del buf
		if args.check and "window" == view:
			b = window_begin
			want = np.zeros((L, 6), dtype=np.int64)
			def on_row(_i, body):
				a = np.frombuffer(body, dtype=np.uint8)
				low = a | 0x20
				for k, ch in enumerate(b"acgtn"):
					want[:, k] += low == ch
				want[:, 5] += a == 0x2D
			ctx.splice_rows(batch, sink=on_row)
			cols, got = ctx.column_counts(batch)
			out["spot_check"] = {"rows": len(rows), "columns": int(L), "first_column": int(cols[0]), "first_column_expected": int(b),
				"differing_counts": int((got.astype(np.int64) != want).sum()),
				"differing_counts_of_the_whole_view_at_these_columns": None if whole_at_window is None else int((whole_at_window[:L].astype(np.int64) != want).sum()), "variable_columns": int(((np.maximum(want.max(axis=1), len(rows) - want.sum(axis=1))) != len(rows)).sum())}
		results[view] = out
		del table
		torch.cuda.empty_cache()
	ctx.set_column_window(0, L_whole)
	record = {"metric": "column counts (v2m_column_counts[_device]) of all rows: device time by pass and per slice, host to host, against checksum_rows_kernel on one slice's rows",
		"config": args.config, "aligned_length": int(L_whole), "edges": g.edge_count, "repeats": args.repeats, "results": results}
	ctx.close()
	text = json.dumps(record)
	print(text)
	if args.out:
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, "w") as f:
			f.write(text + "\n")


if __name__ == "__main__":
	main()
