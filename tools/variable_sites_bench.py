"""Variable sites (v2m_variable_sites) on a synthetic config, all rows (REF + every copy), over the whole row and over a 100-kb window,
under both selections: the call host to host (sinks that only count what they are given) and the two device times of its info (counts +
select, second pass + gather), best of --repeats with every repeat recorded; V per selection and the bytes over the link;
gather_sites_kernel per slice (the info's gather time minus the splices of the second pass, over the slices) beside
splice_aligned_kernel on the same slices (v2m_profile_get_launches) and beside --pack-sites-ms, pack_sites_kernel's figure per slice of
profiles/r13/pair_distances_bench.json, with both ratios; and, in the same run, v2m_splice_rows delivering the same rows whole to a sink
that does nothing -- what a user does today before a CPU tool selects the columns.
With --check the window's result is held equal to the columns selected on the host from the rows v2m_splice_rows delivers for it.
Prints one JSON line and, with --out, writes it (profiles/r14/variable_sites_bench.json).

  python tools/variable_sites_bench.py [--config config3] [--window 100000] [--repeats 3] [--check] [--out profiles/r14/variable_sites_bench.json]
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
	ap.add_argument("--pack-sites-ms", type=float, default=0.114, help="pack_sites_kernel per slice of whole rows, profiles/r13/pair_distances_bench.json")
	ap.add_argument("--whole-rows", type=int, default=1, help="repeats of v2m_splice_rows over the whole rows (0: leave it out)")
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
	n = len(rows)
	KERNELS = {"resolve": N.KERNEL_RESOLVE, "splice_aligned": N.KERNEL_SPLICE_ALIGNED, "column_counts": N.KERNEL_COLUMN_COUNTS}

	def raw_call(snp):
		"""The host form through sinks that only count: (host to host ms, info, blocks, rows, bytes over the link)."""
		seen = {"columns": 0, "blocks": 0, "rows": 0, "bytes": 0}

		def on_columns(_user, _columns, n_sites):
			seen["columns"] += 1
			seen["bytes"] += 4 * int(n_sites)
			return 0

		def on_rows(_user, _first_row, n_rows, _bytes, pitch, _n_sites):
			seen["blocks"] += 1
			seen["rows"] += int(n_rows)
			seen["bytes"] += int(n_rows) * int(pitch)
			return 0

		info = N.VariableSitesInfo()
		columns_sink, rows_sink = N.SITE_COLUMNS_SINK_FN(on_columns), N.SITE_ROWS_SINK_FN(on_rows)
		t0 = time.perf_counter()
		rc = ctx._lib.v2m_variable_sites(ctx._h, C.byref(batch.struct), N.SITES_SNP if snp else 0, columns_sink, rows_sink, None, C.byref(info))
		wall = (time.perf_counter() - t0) * 1e3
		ctx._check(rc)
		return wall, {name: getattr(info, name) for name, _ in N.VariableSitesInfo._fields_}, seen

	def one(snp):
		ctx.synchronize()
		ctx.profile_reset()
		ctx.profile_enable(True)
		wall, info, seen = raw_call(snp)
		got = {name: ctx.profile_get(k) for name, k in KERNELS.items()}
		splices = np.asarray(ctx.profile_launches(KERNELS["splice_aligned"]))
		ctx.profile_enable(False)
		ctx.profile_reset()
		n_slices = int(got["column_counts"][0])
		assert seen["rows"] == (n if info["n_sites"] else 0) and seen["blocks"] == (n_slices if info["n_sites"] else 0), (seen, n_slices)
		# the splices of both passes over the rows are in the profile; the second pass's are those of the gather stage
		second = splices[len(splices) // 2:] if len(splices) >= 2 * n_slices and n_slices and info["n_sites"] else np.zeros(0)
		rec = {"host_to_host_ms": round(wall, 3), "info": {k: (round(v, 4) if isinstance(v, float) else int(v)) for k, v in info.items()},
			"slices": n_slices, "bytes_over_the_link": seen["bytes"],
			"launches": {k: int(c) for k, (c, _) in got.items()}, "device_ms": {k: round(ms, 4) for k, (_, ms) in got.items()}}
		if second.size:
			gather = (info["gather_ms"] - float(second.sum())) / n_slices
			splice = float(np.median(second))
			rec["per_slice_ms"] = {"gather_sites": round(gather, 4), "splice_aligned_median": round(splice, 4), "splice_aligned_min": round(float(second.min()), 4),
				"splice_aligned_max": round(float(second.max()), 4), "pack_sites_r13": args.pack_sites_ms,
				"gather_over_splice": round(gather / splice, 3) if splice else None, "gather_over_pack_sites": round(gather / args.pack_sites_ms, 3)}
		return rec

	def whole_rows():
		"""v2m_splice_rows over the same rows and the view in force into a sink that does nothing: (host to host ms, bytes over the link)."""
		count = [0]

		def on_row(_user, _row, _ptr, length):
			count[0] += int(length)
			return 0

		sink = N.SINK_FN(on_row)
		ctx.synchronize()
		t0 = time.perf_counter()
		rc = ctx._lib.v2m_splice_rows(ctx._h, C.byref(batch.struct), 0, sink, None)
		wall = (time.perf_counter() - t0) * 1e3
		ctx._check(rc)
		return round(wall, 3), count[0]

	results = {}
	L_whole = ctx.aligned_length
	window_begin = (L_whole // 2) // 16 * 16 + 5
	for view in args.views.split(","):
		if "window" == view:
			ctx.set_column_window(window_begin, min(L_whole, window_begin + args.window))
		else:
			ctx.set_column_window(0, L_whole)
		L = ctx.window_length
		ctx.variable_sites(v2m.RowBatch(rows[:8]))          # warm-up: scratch, the device slot
		raw_call(False)                                      # and the site list, the gathered slices and the pinned slots at their full size
		runs = {"variable": [], "snp": []}
		for _ in range(args.repeats):          # alternated
			for selection in runs:
				runs[selection].append(one("snp" == selection))
		out = {"columns": int(L), "rows": n}
		for selection, recs in runs.items():
			best = min(recs, key=lambda r: r["host_to_host_ms"])
			out[selection] = dict(best, host_to_host_ms_all=[r["host_to_host_ms"] for r in recs], counts_ms_all=[r["info"]["counts_ms"] for r in recs],
				gather_ms_all=[r["info"]["gather_ms"] for r in recs])
		if "window" == view or args.whole_rows:
			whole = [whole_rows() for _ in range(1 + (args.repeats if "window" == view else args.whole_rows))][1:]      # (the first: warm-up of the pinned slots)
			out["splice_rows_whole"] = {"host_to_host_ms": min(w for w, _ in whole), "host_to_host_ms_all": [w for w, _ in whole], "bytes_over_the_link": whole[0][1]}
			for selection in runs:
				out[selection]["splice_rows_over_variable_sites"] = round(out["splice_rows_whole"]["host_to_host_ms"] / out[selection]["host_to_host_ms"], 2)
		if "window" == view and args.check:
			bodies = [None] * n
			def on_row(i, body):
				bodies[i] = np.frombuffer(body, dtype=np.uint8).copy()
			ctx.splice_rows(batch, sink=on_row)
			m = np.stack(bodies)
			cls = host_classes(m)
			masks = {"variable": (cls != cls[0]).any(axis=0), "snp": sum((cls == k).any(axis=0).astype(np.int64) for k in range(4)) >= 2}
			check = {"rows": n, "columns": int(L)}
			for selection, mask in masks.items():
				columns, data = ctx.variable_sites(batch, snp_only="snp" == selection)
				want_columns = np.flatnonzero(mask).astype(np.uint64) + np.uint64(window_begin)
				same_columns = bool(np.array_equal(columns, want_columns))
				check[selection] = {"sites_on_the_host": int(mask.sum()), "n_sites": int(len(columns)), "columns_equal": same_columns,
					"differing_bytes": int((data != m[:, mask]).sum()) if same_columns else None}
			out["spot_check"] = check
		results[view] = out
	ctx.set_column_window(0, L_whole)
	record = {"metric": "variable sites (v2m_variable_sites) of all rows: host to host, device time by stage, gather_sites_kernel per slice beside the splice and pack_sites_kernel, v2m_splice_rows of the same rows beside it",
		"config": args.config, "aligned_length": int(L_whole), "edges": g.edge_count, "repeats": args.repeats,
		"gather_sites": N.GATHER_SITES, "gather_threads": N.GATHER_THREADS, "results": results}
	ctx.close()
	text = json.dumps(record)
	print(text)
	if args.out:
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, "w") as f:
			f.write(text + "\n")
	if args.check:
		bad = [s for s in ("variable", "snp") if not results.get("window", {}).get("spot_check", {}).get(s, {}).get("columns_equal") or results["window"]["spot_check"][s]["differing_bytes"]]
		if "window" in results and bad:
			sys.exit("the window's result differs from the host's selection: %s" % ", ".join(bad))


if __name__ == "__main__":
	main()
