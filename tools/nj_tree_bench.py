"""The neighbour-joining tree (v2m_nj_tree) on a synthetic config, all rows (REF + every copy) over a window of the alignment: the call
host to host and the two stream times of its info (distances, tree), two warm-ups, best of --repeats with every repeat recorded; the
bytes of the working matrix nj_rowmin_kernel's launches read (the upper triangle of the live slots, every join) over the tree's stream
time beside the 8 TB/s peak -- a LOWER bound of the kernel's rate: the tree's time also holds nj_join_kernel and every kernel boundary,
which have no times of their own; v2m_nj_tree_of_distances on the leading quarter and half of the same matrix, which separates what
grows with the joins from what grows with the bytes; and, with --check, the host library's plain-loop restatement (v2mh_nj_tree_cpu) on
the same matrix, timed once on one core, with whether all its records equal the GPU's as bytes.
Prints one JSON line and, with --out, writes it (profiles/r16/nj_tree_bench.json).

  python tools/nj_tree_bench.py [--config config3] [--window 100000] [--repeats 3] [--check] [--out profiles/r16/nj_tree_bench.json]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BYTES_PER_S = 8e12


def rowmin_matrix_bytes(n, even=lambda i: (i + 1) & ~1):
	"""The bytes of the working matrix the rowmin launches of a tree of n taxa read: at r live taxa row i < r - 1 reads the slots from
	(i + 1) rounded down to even up to r rounded up to even, 8 bytes each."""
	total = 0
	for r in range(n, 3, -1):
		i = np.arange(r - 1, dtype=np.int64)
		total += int((((r + 1) & ~1) - ((i + 1) & ~1)).sum()) * 8
	return total


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--config", default="config3")
	ap.add_argument("--window", type=int, default=100000)
	ap.add_argument("--repeats", type=int, default=3)
	ap.add_argument("--check", action="store_true")
	ap.add_argument("--out")
	args = ap.parse_args()
	import torch
	import vcf2multialign_amd as v2m
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
	ctx.set_column_window(window_begin, min(L_whole, window_begin + args.window))

	def timed(call):
		ctx.synchronize()
		ctx.profile_reset()
		ctx.profile_enable(True)
		t0 = time.perf_counter()
		nodes, info = call()
		wall = (time.perf_counter() - t0) * 1e3
		ctx.profile_enable(False)
		ctx.profile_reset()
		return nodes, {"host_to_host_ms": round(wall, 3), "info": {k: (round(v, 4) if isinstance(v, float) else int(v)) for k, v in info.items()}}

	ctx.nj_tree(v2m.RowBatch(rows[:8]))          # warm-ups: scratch, the device slot,
	ctx.nj_tree(batch)                            # and the planes and the matrices at their full size
	runs, nodes = [], None
	for _ in range(args.repeats):
		nodes, rec = timed(lambda: ctx.nj_tree(batch, info=True))
		runs.append(rec)
	best = min(runs, key=lambda r: r["host_to_host_ms"])
	matrix_bytes = rowmin_matrix_bytes(n)
	tree_s = best["info"]["tree_ms"] * 1e-3
	result = dict(best, rows=n, columns=int(ctx.window_length), joins=n - 3, launches=2 * (n - 3) + 2,
		host_to_host_ms_all=[r["host_to_host_ms"] for r in runs], distances_ms_all=[r["info"]["distances_ms"] for r in runs], tree_ms_all=[r["info"]["tree_ms"] for r in runs],
		rowmin={"matrix_bytes_read": matrix_bytes, "bytes_per_s_lower_bound": round(matrix_bytes / tree_s / 1e9, 2) if tree_s > 0 else None, "unit": "1e9 bytes per second over the whole tree stage",
			"peak_bytes_per_s": PEAK_BYTES_PER_S / 1e9, "share_of_peak_lower_bound": round(matrix_bytes / tree_s / PEAK_BYTES_PER_S, 4) if tree_s > 0 else None},
		tree={"negative_branches": int((nodes["len_a"] < 0).sum() + (nodes["len_b"] < 0).sum() + (nodes["len_c"] < 0).sum()),
			"longest_branch": float(max(nodes["len_a"].max(), nodes["len_b"].max(), nodes["len_c"].max()))})

	# the same matrix on the device, and the tree of its leading parts: the time by the number of taxa
	pitch = (n + 3) // 4 * 4
	d_dist = torch.zeros(n * pitch, dtype=torch.int32, device=dev)
	ctx.pair_distances_device(batch, d_dist.data_ptr(), pitch)
	scaling = []
	for part in (n // 4, n // 2, n):
		ctx.nj_tree_of_distances(d_dist.data_ptr(), part, pitch)
		times = []
		for _ in range(args.repeats):
			part_nodes, rec = timed(lambda: ctx.nj_tree_of_distances(d_dist.data_ptr(), part, pitch, info=True))
			times.append(rec["info"]["tree_ms"])
		scaling.append({"taxa": part, "tree_ms_all": times, "tree_ms": min(times), "matrix_bytes_read": rowmin_matrix_bytes(part), "launches": 2 * (part - 3) + 2})
	result["of_distances_by_taxa"] = scaling
	result["of_distances_equals_from_rows"] = bool(part_nodes.tobytes() == nodes.tobytes())

	if args.check:
		dist = d_dist.cpu().numpy().view(np.uint32).reshape(n, pitch)[:, :n].copy()
		t0 = time.perf_counter()
		cpu_nodes = host.nj_tree_cpu(dist)
		cpu_s = time.perf_counter() - t0
		differing = int(sum(cpu_nodes[k:k + 1].tobytes() != nodes[k:k + 1].tobytes() for k in range(n - 2)))
		result["cpu_restatement"] = {"seconds_one_core": round(cpu_s, 2), "records": n - 2, "records_differing_from_the_gpu": differing,
			"all_records_equal_as_bytes": bool(cpu_nodes.tobytes() == nodes.tobytes()),
			"ratio_to_gpu_tree_stage": round(cpu_s / tree_s, 1) if tree_s > 0 else None, "ratio_to_gpu_host_to_host": round(cpu_s * 1e3 / best["host_to_host_ms"], 1)}
	ctx.set_column_window(0, L_whole)
	record = {"metric": "neighbour-joining tree (v2m_nj_tree) of all rows over a window: host to host, stream time by stage, the rowmin launches' matrix bytes over the tree stage, the CPU restatement",
		"config": args.config, "aligned_length": int(L_whole), "window": [int(window_begin), int(min(L_whole, window_begin + args.window))], "repeats": args.repeats, "result": result}
	ctx.close()
	text = json.dumps(record)
	print(text)
	if args.out:
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, "w") as f:
			f.write(text + "\n")


if __name__ == "__main__":
	main()
