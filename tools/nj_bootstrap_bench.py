"""The bootstrap of the neighbour-joining tree (v2m_nj_bootstrap) on a synthetic config, all rows (REF + every copy), over a window of
the alignment and -- with --whole-replicates > 0 -- over whole rows: the call host to host and the stream times of its info, a warm-up,
every repeat recorded; per replicate the weights, the weighted pairs and the tree; pair_distances_weighted_kernel's time per replicate
beside pair_distances_kernel's on planes of the same content in the same run (v2m_pair_distances with profiling on), as a ratio; and
the weighted kernel's 64-bit word pairs a second beside the VALU ceiling that follows from its instruction count,
--valu-base + K * --valu-per-slice vector instructions a word pair (K: the info's largest; counted in the kernel's ISA); whole rows under both flags.
Spot check over the window (--check): replicate 0's matrix equals the model's weights (tests/nj_bootstrap_model.py) applied on the host to the rows
v2m_splice_rows delivers, and its tree equals host.nj_tree_cpu's of that matrix as bytes.
Prints one JSON line and, with --out, writes it (profiles/r17/nj_bootstrap_bench.json).

  python tools/nj_bootstrap_bench.py [--config config3] [--window 100000] [--replicates 100] [--whole-replicates 10] [--repeats 2] [--check] [--out FILE]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CUS, SIMDS, CYCLES_PER_WAVE_INSTRUCTION, CLOCK_HZ = 256, 4, 2, 2.4e9


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--config", default="config3")
	ap.add_argument("--window", type=int, default=100000)
	ap.add_argument("--replicates", type=int, default=100)
	ap.add_argument("--whole-replicates", type=int, default=10)
	ap.add_argument("--repeats", type=int, default=2)
	ap.add_argument("--seed", type=int, default=1)
	ap.add_argument("--valu-base", default="8.125,10.125", help="all,acgt: vector instructions a word pair that form the mask (130 and 162 for 16 word pairs in the ISA)")
	ap.add_argument("--valu-per-slice", type=float, default=5.0625, help="vector instructions a word pair and slice (81 for 16 word pairs in the ISA)")
	ap.add_argument("--check", action="store_true", help="the spot check of replicate 0 (minutes of host time at config 3)")
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
	T, C_ = N.PAIR_TILE, N.PAIR_CHUNK_WORDS
	ceiling_lane_instructions = CUS * SIMDS * 64 / CYCLES_PER_WAVE_INSTRUCTION * CLOCK_HZ
	valu_base = dict(zip((False, True), (float(x) for x in args.valu_base.split(","))))

	def profiled(call):
		ctx.synchronize()
		ctx.profile_reset()
		ctx.profile_enable(True)
		t0 = time.perf_counter()
		out = call()
		wall = (time.perf_counter() - t0) * 1e3
		ctx.profile_enable(False)
		ctx.profile_reset()
		return out, wall

	def view(name, B, acgt=False):
		ctx.nj_bootstrap(batch, 1, seed=args.seed, acgt_only=acgt)   # warm-up: every buffer at its full size
		runs = []
		for _ in range(args.repeats):
			(nodes, support, info), wall = profiled(lambda: ctx.nj_bootstrap(batch, B, seed=args.seed, acgt_only=acgt, info=True))
			(_, plain), _ = profiled(lambda: ctx.pair_distances(batch, acgt_only=acgt, info=True))
			runs.append({"host_to_host_ms": round(wall, 3), "info": {k: (round(v, 4) if isinstance(v, float) else int(v)) for k, v in info.items()},
				"plain_pairs_ms": round(plain["pairs_ms"], 4)})
		best = min(runs, key=lambda r: r["host_to_host_ms"])
		info = best["info"]
		K = info["max_slices"]
		n_pad = (n + T - 1) // T * T
		chunks = (info["n_sites"] + 64 * C_ - 1) // (64 * C_)
		word_pairs = (n_pad // T) * (n_pad // T + 1) // 2 * T * T * chunks * C_
		weighted_ms = info["pairs_ms"] / B
		valu = valu_base[acgt] + K * args.valu_per_slice
		rec = {"view": name, "model": "acgt" if acgt else "all", "rows": n, "columns": info["n_columns"], "sites": info["n_sites"], "replicates": B, "K": K, "pack_passes": info["n_pack_passes"], "passes": info["n_passes"],
			"runs": runs, "best": best,
			"per_replicate_ms": {"weights": round(info["weights_ms"] / B, 4), "weighted_pairs": round(weighted_ms, 4), "tree": round(info["trees_ms"] / (B + 1), 4)},
			"weighted_over_plain_pair_kernel": round(weighted_ms / best["plain_pairs_ms"], 3) if best["plain_pairs_ms"] > 0 else None,
			"support": {"min": int(support.min()), "median": float(np.median(support)), "max": int(support.max()), "joins_with_all": int((support == B).sum()), "joins_with_none": int((support == 0).sum())}}
		if weighted_ms > 0:
			rate = word_pairs / (weighted_ms * 1e-3)
			ceiling = ceiling_lane_instructions / valu
			rec["weighted_pair_kernel"] = {"word_pairs_computed": int(word_pairs), "word_pairs_per_s": round(rate / 1e9, 2), "unit": "1e9 64-bit word pairs per second",
				"valu_per_word_pair": valu, "valu_ceiling_word_pairs_per_s": round(ceiling / 1e9, 2), "share_of_ceiling": round(rate / ceiling, 3)}
		return rec, nodes

	results = []
	ctx.set_column_window(*window)
	rec, nodes = view("window", args.replicates)
	if args.check:
		# the spot check: replicate 0 against the model's weights applied on the host to the spliced rows.  Columns that weigh 0 or hold
		# one class in every row add nothing and are dropped before the brute force.
		import nj_bootstrap_model as BM
		import pair_distances_model as PM
		L = window[1] - window[0]
		w = BM.weights(args.seed, 0, L)
		cls = PM.classes(np.frombuffer(b"".join(ctx.splice_rows(rows)), dtype=np.uint8).reshape(n, L))
		keep = np.flatnonzero((w > 0) & (cls != cls[0]).any(axis=0))
		want = BM.weighted_distances(np.ascontiguousarray(cls[:, keep]), w[keep])
		got = ctx.bootstrap_distances(batch, args.seed, 0)
		_, _, trees = ctx.nj_bootstrap(batch, 1, seed=args.seed, replicates=True)
		rec["spot_check"] = {"replicate_0_matrix_equals_the_model": bool(np.array_equal(got, want)),
			"replicate_0_tree_equals_nj_tree_cpu_as_bytes": bool(trees[0].tobytes() == host.nj_tree_cpu(want).tobytes())}
	results.append(rec)
	ctx.set_column_window(0, L_whole)
	if args.whole_replicates > 0:
		for acgt in (False, True):
			rec, _ = view("whole rows", args.whole_replicates, acgt)
			results.append(rec)
	record = {"metric": "bootstrap of the neighbour-joining tree (v2m_nj_bootstrap) of all rows: host to host, stream time by stage and per replicate, the weighted pair kernel beside the plain one and beside its VALU ceiling",
		"config": args.config, "aligned_length": int(L_whole), "window": [int(window[0]), int(window[1])], "repeats": args.repeats, "seed": args.seed,
		"ceiling_basis": {"cus": CUS, "simds_per_cu": SIMDS, "cycles_per_wave_instruction": CYCLES_PER_WAVE_INSTRUCTION, "clock_hz": CLOCK_HZ,
			"valu_base_all_acgt": args.valu_base, "valu_per_slice": args.valu_per_slice}, "results": results}
	ctx.close()
	text = json.dumps(record)
	print(text)
	if args.out:
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, "w") as f:
			f.write(text + "\n")


if __name__ == "__main__":
	main()
