"""Pair distances (v2m_pair_distances) on a synthetic config, all rows (REF + every copy), over the whole row and over a 100-kb window,
under both definitions: the call host to host and the three device times of its info (counts + select, pack, pairs), best of --repeats
with every repeat recorded; pack_sites_kernel per slice (the info's pack time minus the splices of the second pass, over the slices)
beside splice_aligned_kernel and column_counts_kernel on the same slices (v2m_profile_get_launches); the pair kernel's achieved 64-bit
word pairs per second beside the VALU ceiling that follows from --valu-per-word-pair, the vector instructions per word pair of its
inner loop in the cross-compiled ISA (DESIGN.md section 8.9 says how it is counted), and the figures of MI355X_MICROARCH.md: 256 CUs x 4
SIMDs, a wave instruction of 64 lanes issued over 2 cycles, 2.4 GHz.
With --check the window's matrix is held equal to one computed on the host from the rows v2m_splice_rows delivers for the window, and
the whole-row matrix minus the window's is held non-negative everywhere.
Prints one JSON line and, with --out, writes it (profiles/r13/pair_distances_bench.json).

  python tools/pair_distances_bench.py [--config config3] [--window 100000] [--repeats 3] [--check] [--out profiles/r13/pair_distances_bench.json]
"""

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CUS, SIMDS, CYCLES_PER_WAVE_INSTRUCTION, CLOCK_HZ = 256, 4, 2, 2.4e9


def host_classes(a):
	low = a | 0x20
	cls = np.full(a.shape, 6, dtype=np.uint8)
	for k, ch in enumerate(b"acgtn"):
		cls[low == ch] = k
	cls[a == 0x2D] = 5
	return cls


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--config", default="config3")
	ap.add_argument("--window", type=int, default=100000)
	ap.add_argument("--repeats", type=int, default=3)
	ap.add_argument("--views", default="window,whole")
	ap.add_argument("--valu-per-word-pair", default="10.5625,12.5625", help="all,acgt: VALU instructions per 64-bit word pair of the inner loop")
	ap.add_argument("--check", action="store_true")
	ap.add_argument("--out")
	args = ap.parse_args()
	import torch
	import vcf2multialign_amd as v2m
	from vcf2multialign_amd import _native as N, synth

	valu = dict(zip(("all", "acgt"), (float(x) for x in args.valu_per_word_pair.split(","))))
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
	KERNELS = {"resolve": N.KERNEL_RESOLVE, "splice_aligned": N.KERNEL_SPLICE_ALIGNED, "column_counts": N.KERNEL_COLUMN_COUNTS}
	T, C_ = N.PAIR_TILE, N.PAIR_CHUNK_WORDS
	ceiling_lane_instructions = CUS * SIMDS * 64 / CYCLES_PER_WAVE_INSTRUCTION * CLOCK_HZ

	def one(acgt):
		ctx.synchronize()
		ctx.profile_reset()
		ctx.profile_enable(True)
		t0 = time.perf_counter()
		dist, info = ctx.pair_distances(batch, acgt_only=acgt, info=True)
		wall = (time.perf_counter() - t0) * 1e3
		got = {name: ctx.profile_get(k) for name, k in KERNELS.items()}
		per_slice = {name: np.asarray(ctx.profile_launches(KERNELS[name])) for name in ("splice_aligned", "column_counts")}
		ctx.profile_enable(False)
		ctx.profile_reset()
		n_slices = int(got["column_counts"][0])
		# the splices of both passes over the rows are in the profile; the second pass's are those of the pack stage
		splices = per_slice["splice_aligned"]
		second = float(splices[len(splices) // 2:].sum()) if len(splices) >= 2 * n_slices and n_slices else 0.0
		chunks = -(-int(info["n_sites"]) // (64 * C_))
		n_pad = -(-n // T) * T
		word_pairs = (n_pad // T) * (n_pad // T + 1) // 2 * T * T * chunks * C_          # what the kernel computes: whole tiles of the upper triangle, padded chunks
		useful = n * (n - 1) // 2 * -(-int(info["n_sites"]) // 64)
		rec = {"host_to_host_ms": round(wall, 3), "info": {k: (round(v, 4) if isinstance(v, float) else int(v)) for k, v in info.items()},
			"launches": {k: int(c) for k, (c, _) in got.items()}, "device_ms": {k: round(ms, 4) for k, (_, ms) in got.items()},
			"per_slice_ms": {k: {"min": round(float(v.min()), 4), "median": round(float(np.median(v)), 4), "max": round(float(v.max()), 4)} for k, v in per_slice.items() if v.size},
			"pack_sites_per_slice_ms": round((info["pack_ms"] - second) / max(1, n_slices * int(info["n_passes"])), 4) if info["n_sites"] else None,
			"plane_bytes": int(3 * n_pad * chunks * C_ * 8), "word_pairs_computed": int(word_pairs), "word_pairs_of_distinct_row_pairs": int(useful)}
		if info["pairs_ms"] > 0 and info["n_sites"]:
			model = "acgt" if acgt else "all"
			rate = word_pairs / (info["pairs_ms"] * 1e-3)
			ceiling = ceiling_lane_instructions / valu[model]          # word pairs a second: a lane works on one word pair at a time
			rec["pair_kernel"] = {"word_pairs_per_s": round(rate / 1e9, 2), "unit": "1e9 64-bit word pairs per second", "valu_per_word_pair": valu[model],
				"valu_ceiling_word_pairs_per_s": round(ceiling / 1e9, 2), "share_of_ceiling": round(rate / ceiling, 3)}
		return rec, dist

	results = {}
	L_whole = ctx.aligned_length
	window_begin = (L_whole // 2) // 16 * 16 + 5
	window_dist = {}
	for view in args.views.split(","):
		if "window" == view:
			ctx.set_column_window(window_begin, min(L_whole, window_begin + args.window))
		else:
			ctx.set_column_window(0, L_whole)
		L = ctx.window_length
		ctx.pair_distances(v2m.RowBatch(rows[:8]))          # warm-up: scratch, the device slot
		ctx.pair_distances(batch)                             # and the planes and the matrix at their full size
		runs = {"all": [], "acgt": []}
		last = {}
		for _ in range(args.repeats):          # alternated
			for model in runs:
				rec, dist = one("acgt" == model)
				runs[model].append(rec)
				last[model] = dist
		out = {"columns": int(L), "rows": n}
		for model, recs in runs.items():
			best = min(recs, key=lambda r: r["host_to_host_ms"])
			out[model] = dict(best, host_to_host_ms_all=[r["host_to_host_ms"] for r in recs], pairs_ms_all=[r["info"]["pairs_ms"] for r in recs],
				pack_ms_all=[r["info"]["pack_ms"] for r in recs], counts_ms_all=[r["info"]["counts_ms"] for r in recs])
			out[model]["matrix"] = {"max": int(last[model].max()), "mean_off_diagonal": round(float(last[model].sum()) / max(1, n * (n - 1)), 3),
				"symmetric": bool(np.array_equal(last[model], last[model].T)), "zero_diagonal": bool((np.diag(last[model]) == 0).all())}
		if "window" == view:
			window_dist = dict(last)
			if args.check:
				bodies = [None] * n
				def on_row(i, body):
					bodies[i] = np.frombuffer(body, dtype=np.uint8).copy()
				ctx.splice_rows(batch, sink=on_row)
				cls = host_classes(np.stack(bodies))
				keep = (cls != cls[0]).any(axis=0)
				cls = np.ascontiguousarray(cls[:, keep])
				base = cls < 4
				differing = {"all": 0, "acgt": 0}
				for i in range(n):
					diff = cls != cls[i]
					differing["all"] += int((diff.sum(axis=1).astype(np.uint32) != last["all"][i]).sum())
					differing["acgt"] += int(((diff & base & base[i]).sum(axis=1).astype(np.uint32) != last["acgt"][i]).sum())
				out["spot_check"] = {"rows": n, "columns": int(L), "variable_columns_on_the_host": int(keep.sum()), "n_sites": out["all"]["info"]["n_sites"],
					"differing_entries": differing}
		elif window_dist:
			out["whole_minus_window_negative_entries"] = {m: int((last[m].astype(np.int64) - window_dist[m].astype(np.int64) < 0).sum()) for m in last}
		results[view] = out
	ctx.set_column_window(0, L_whole)
	record = {"metric": "pair distances (v2m_pair_distances) of all rows: host to host, device time by stage, pack_sites_kernel per slice, the pair kernel against its VALU ceiling",
		"config": args.config, "aligned_length": int(L_whole), "edges": g.edge_count, "repeats": args.repeats, "tile_rows": T, "chunk_words": C_,
		"ceiling_basis": {"cus": CUS, "simds_per_cu": SIMDS, "cycles_per_wave_instruction": CYCLES_PER_WAVE_INSTRUCTION, "clock_hz": CLOCK_HZ}, "results": results}
	ctx.close()
	text = json.dumps(record)
	print(text)
	if args.out:
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, "w") as f:
			f.write(text + "\n")


if __name__ == "__main__":
	main()
