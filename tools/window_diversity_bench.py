"""Window diversity (v2m_window_diversity, v2m_diversity_of_counts) on a synthetic config, all rows (REF + every copy), over a window of
the alignment in 1-kb bins and over whole rows in 10-kb bins: the host form host to host with the two stream times of its info (counts,
bins), and the device form alone on a table v2m_column_counts_device made, whose bins_ms is the reduction without the counts; one
warm-up, then --repeats runs with every repeat recorded.  The floor the reduction is read against is measured in the same run: a plain
device read of the four letter planes, 16 bytes a column (torch's sum over them, between events).  With --check, a sample of the bins is
compared with the host library's plain-loop restatement (v2mh_window_diversity_cpu) on the rows spliced over that bin.
Prints one JSON line and, with --out, writes it (profiles/r19/window_diversity_bench.json).

  python tools/window_diversity_bench.py [--config config3] [--window 100000] [--repeats 2] [--check] [--out profiles/r19/window_diversity_bench.json]
"""

import argparse
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
	ap.add_argument("--repeats", type=int, default=2)
	ap.add_argument("--check", action="store_true")
	ap.add_argument("--check-bins", type=int, default=6)
	ap.add_argument("--out")
	args = ap.parse_args()
	import torch
	import vcf2multialign_amd as v2m
	from vcf2multialign_amd import _native as N
	from vcf2multialign_amd import host, synth

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
	n = len(rows)
	L_whole = ctx.aligned_length
	window_begin = (L_whole // 2) // 16 * 16 + 5
	window = (window_begin, min(L_whole, window_begin + args.window))

	def profiled(call):
		ctx.synchronize()
		ctx.profile_enable(True)
		t0 = time.perf_counter()
		out = call()
		wall = (time.perf_counter() - t0) * 1e3
		ctx.profile_enable(False)
		return out, round(wall, 3)

	def plane_read_ms(table, pitch, L):
		"""A plain read of planes 0-3 of the table over L columns: the best of five sums."""
		best = None
		for _ in range(5):
			a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
			a.record()
			total = table.view(6, pitch)[:4, :L].sum(dtype=torch.int64)
			b.record()
			torch.cuda.synchronize()
			best = a.elapsed_time(b) if best is None else min(best, a.elapsed_time(b))
		del total
		return best

	def view(name, columns, bin_width, check):
		ctx.set_column_window(*columns)
		L = columns[1] - columns[0]
		bounds = np.array(sorted(set(list(range(columns[0], columns[1], bin_width)) + [columns[1]])), dtype=np.uint64)
		ctx.window_diversity(batch, bounds)              # the warm-up: scratch, the device slot
		runs, out = [], None
		for _ in range(args.repeats):
			out, wall = profiled(lambda: ctx.window_diversity(batch, bounds, info=True))
			runs.append({"host_to_host_ms": wall, "counts_ms": round(out[2]["counts_ms"], 4), "bins_ms": round(out[2]["bins_ms"], 4)})
		bins, sfs, info = out
		# the device form on a table of its own: the reduction alone, and the floor beside it
		pitch = (L + 3) & ~3
		table = torch.zeros(6 * pitch, dtype=torch.int32, device=dev)
		d_bins = torch.zeros(len(bounds) * 8, dtype=torch.int64, device=dev)
		d_sfs = torch.zeros(n // 2 + 2, dtype=torch.int64, device=dev)
		ctx.column_counts_device(batch, table.data_ptr(), pitch)
		relative = bounds - np.uint64(columns[0])
		ctx.diversity_of_counts(table.data_ptr(), pitch, L, n, relative, d_bins.data_ptr(), d_sfs.data_ptr())
		device_runs = []
		for _ in range(args.repeats):
			rec, wall = profiled(lambda: ctx.diversity_of_counts(table.data_ptr(), pitch, L, n, relative, d_bins.data_ptr(), d_sfs.data_ptr()))
			device_runs.append({"host_to_host_ms": wall, "bins_ms": round(rec["bins_ms"], 4)})
		same = bool(d_bins.cpu().numpy()[:8 * (len(bounds) - 1)].view(np.dtype(N.DIVERSITY_BIN_DTYPE)).tobytes() == bins.tobytes()
			and d_sfs.cpu().numpy()[:n // 2 + 1].view(np.uint64).tobytes() == sfs.tobytes())
		floor = plane_read_ms(table, pitch, L)
		best_bins = min(r["bins_ms"] for r in device_runs)
		totals = {name_: int(bins[name_].sum(dtype=np.uint64)) for name_ in bins.dtype.names}
		result = {"view": name, "rows": n, "columns": int(L), "bin_width": bin_width, "n_bins": len(bounds) - 1, "multiallelic": int(info["multiallelic"]), "totals": totals,
			"host_form": runs, "device_form": device_runs, "device_form_equals_host_form_as_bytes": same,
			"plane_read": {"bytes": 16 * L, "ms_best_of_5": round(floor, 4), "what": "torch sum over planes 0-3, between events"},
			"bins_ms_over_plane_read": round(best_bins / floor, 2) if floor > 0 else None,
			"spectrum": {"entries": int(len(sfs)), "columns": int(sfs.sum(dtype=np.uint64)), "monomorphic": int(sfs[0])}}
		if check:
			rng = np.random.default_rng(1)
			picks = sorted(set(int(k) for k in rng.integers(0, len(bounds) - 1, size=args.check_bins)) | {0, len(bounds) - 2})
			equal, seconds = True, 0.0
			for k in picks:
				lo, hi = int(bounds[k]), int(bounds[k + 1])
				ctx.set_column_window(lo, hi)
				m = np.frombuffer(b"".join(ctx.splice_rows(batch)), dtype=np.uint8).reshape(n, hi - lo)
				t0 = time.perf_counter()
				cpu_bins, _, _ = host.window_diversity_cpu(m, [0, hi - lo], want_sfs=False)
				seconds += time.perf_counter() - t0
				equal = equal and cpu_bins[0:1].tobytes() == bins[k:k + 1].tobytes()
			ctx.set_column_window(*columns)
			result["cpu_restatement"] = {"bins_checked": picks, "equal_as_bytes": bool(equal), "seconds_one_core": round(seconds, 3)}
		del table, d_bins, d_sfs
		return result

	results = [view("window", window, 1000, args.check), view("whole rows", (0, L_whole), 10000, args.check)]
	ctx.set_column_window(0, L_whole)
	record = {"metric": "window diversity (v2m_window_diversity, v2m_diversity_of_counts) of all rows: host to host, stream time of the counts and of the reduction, "
		"the reduction beside a plain read of the four planes, sampled bins against the CPU restatement",
		"config": args.config, "aligned_length": int(L_whole), "window": [int(window[0]), int(window[1])], "repeats": args.repeats, "results": results}
	ctx.close()
	text = json.dumps(record)
	print(text)
	if args.out:
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, "w") as f:
			f.write(text + "\n")


if __name__ == "__main__":
	main()
