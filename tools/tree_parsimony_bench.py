"""Parsimony on the tree (v2m_tree_parsimony) on a synthetic config, all rows (REF + every copy) on the neighbour-joining tree of the
same rows, over a window of the alignment and over whole rows: the call host to host and the three stream times of its info (counts,
gather, parsimony), one warm-up, then --repeats runs with every repeat recorded; the bytes the two passes move at least -- 3 n V each: a
pass reads the n leaf rows and reads or writes every one of the n - 2 sets about twice -- over the parsimony stage's stream time beside
the 8 TB/s peak (the stage also holds the scan and the kernel boundaries, so this is a lower bound of the kernels' rate); and, with
--check, the host library's plain-loop restatement (v2mh_tree_parsimony_cpu) on the same bytes of the window, timed once on one core,
with whether its site records, branch counts and mutations equal the GPU's as bytes (--check-whole: of whole rows as well, which
brings n x V bytes to the host).
Prints one JSON line and, with --out, writes it (profiles/r18/tree_parsimony_bench.json).

  python tools/tree_parsimony_bench.py [--config config3] [--window 100000] [--repeats 2] [--check] [--out profiles/r18/tree_parsimony_bench.json]
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


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--config", default="config3")
	ap.add_argument("--window", type=int, default=100000)
	ap.add_argument("--repeats", type=int, default=2)
	ap.add_argument("--check", action="store_true")
	ap.add_argument("--check-whole", action="store_true")
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
	window = (window_begin, min(L_whole, window_begin + args.window))

	def timed(call):
		ctx.synchronize()
		ctx.profile_reset()
		ctx.profile_enable(True)
		t0 = time.perf_counter()
		out = call()
		wall = (time.perf_counter() - t0) * 1e3
		ctx.profile_enable(False)
		ctx.profile_reset()
		return out, {"host_to_host_ms": round(wall, 3), "info": {k: (round(v, 4) if isinstance(v, float) else int(v)) for k, v in out[-1].items()}}

	def view(name, columns, check):
		ctx.set_column_window(*columns)
		t0 = time.perf_counter()
		nodes = ctx.nj_tree(batch)
		tree_ms = (time.perf_counter() - t0) * 1e3
		ctx.tree_parsimony(batch, nodes)              # the warm-up: scratch, the device slot, the pinned slots at their full size
		runs, out = [], None
		for _ in range(args.repeats):
			out, rec = timed(lambda: ctx.tree_parsimony(batch, nodes, info=True))
			runs.append(rec)
		sites, branch_changes, mutations, info = out
		best = min(runs, key=lambda r: r["host_to_host_ms"])
		V = int(info["n_sites"])
		pass_bytes = 3 * n * V
		stage_s = best["info"]["parsimony_ms"] * 1e-3
		popcount = np.array([bin(k).count("1") for k in range(16)])[sites["present"]]
		result = dict(best, view=name, rows=n, columns=int(ctx.window_length), n_sites=V, n_mutations=int(info["n_mutations"]), n_ranges=int(info["n_ranges"]),
			nj_tree_host_to_host_ms=round(tree_ms, 3),
			host_to_host_ms_all=[r["host_to_host_ms"] for r in runs], counts_ms_all=[r["info"]["counts_ms"] for r in runs], gather_ms_all=[r["info"]["gather_ms"] for r in runs],
			parsimony_ms_all=[r["info"]["parsimony_ms"] for r in runs],
			passes={"bytes_of_one_pass": pass_bytes, "bytes_of_both": 2 * pass_bytes, "unit": "1e9 bytes per second over the parsimony stage (up, scan and down together)",
				"bytes_per_s_lower_bound": round(2 * pass_bytes / stage_s / 1e9, 2) if stage_s > 0 else None, "peak_bytes_per_s": PEAK_BYTES_PER_S / 1e9,
				"share_of_peak_lower_bound": round(2 * pass_bytes / stage_s / PEAK_BYTES_PER_S, 4) if stage_s > 0 else None},
			tree={"homoplasic_sites": int((sites["steps"].astype(np.int64) > popcount - 1).sum()), "most_steps_of_a_site": int(sites["steps"].max(initial=0)),
				"branches_without_a_change": int((branch_changes == 0).sum()), "most_changes_of_a_branch": int(branch_changes.max(initial=0))},
			invariants={"mutations_per_site_equal_steps": bool(np.array_equal(np.bincount(mutations["site"], minlength=V), sites["steps"])),
				"branch_changes_sum_to_steps": bool(int(branch_changes.sum(dtype=np.uint64)) == int(sites["steps"].sum(dtype=np.uint64)) == len(mutations))})
		if check:
			columns_, data, _ = ctx.variable_sites(batch, snp_only=True, info=True)
			data = np.ascontiguousarray(data)
			t0 = time.perf_counter()
			cpu_sites, cpu_branches, cpu_mutations = host.tree_parsimony_cpu(data, nodes)
			cpu_s = time.perf_counter() - t0
			result["cpu_restatement"] = {"seconds_one_core": round(cpu_s, 3),
				"sites_equal_as_bytes": bool(cpu_sites["steps"].tobytes() == sites["steps"].tobytes() and cpu_sites["present"].tobytes() == sites["present"].tobytes()
					and np.array_equal(columns_, sites["column"])),
				"branch_changes_equal_as_bytes": bool(cpu_branches.tobytes() == branch_changes.tobytes()),
				"mutations_equal_as_bytes": bool(cpu_mutations.tobytes() == mutations.tobytes()),
				"ratio_to_gpu_parsimony_stage": round(cpu_s / stage_s, 1) if stage_s > 0 else None, "ratio_to_gpu_host_to_host": round(cpu_s * 1e3 / best["host_to_host_ms"], 1)}
		return result

	results = [view("window", window, args.check), view("whole rows", (0, L_whole), args.check_whole)]
	ctx.set_column_window(0, L_whole)
	record = {"metric": "parsimony on the tree (v2m_tree_parsimony) of all rows on their neighbour-joining tree: host to host, stream time by stage, the passes' bytes over the parsimony stage, the CPU restatement",
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
