"""Row alignment ops (v2m_row_ops) on a synthetic config: per-pass device time (v2m_profile_get), host-to-host time, ops per row and bytes
returned, for one batch of rows (REF + the first copies) and for all rows; beside them, as the yardstick, the device time of
count_unaligned_kernel + splice_unaligned_kernel for the same rows in the same process (rows into HBM, batch by batch).  Best of --repeats,
the two alternated; the launches of every pass are recorded beside its time (every pass of a call covers every row exactly once: rows per
launch = rows / launches).  With --check-row N, chromosome copy N's ops are compared with the model of that row built from the CPU oracle's graph
(tests/row_ops_model.py; 0 differences expected).  Prints one JSON line and, with --out, writes it (profiles/r09/row_ops_bench.json).

With --split the two legs are v2m_row_ops with V2M_OPS_SPLIT_MATCH and without it instead (the unsplit passes of the same build are the
yardstick), on the same rows, alternated: per-pass device time and ops per row of both forms, and --check-row compares the copy's SPLIT ops
with the model of tests/row_ops_eqx_model.py (profiles/r11/row_ops_eqx_bench.json).

  python tools/row_ops_bench.py [--config config3] [--batch-rows 627] [--repeats 3] [--check-row 1234] [--out profiles/r09/row_ops_bench.json]
  python tools/row_ops_bench.py --split [--check-row 1234] [--out profiles/r11/row_ops_eqx_bench.json]
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
	ap.add_argument("--batch-rows", type=int, default=627)
	ap.add_argument("--repeats", type=int, default=3)
	ap.add_argument("--check-row", type=int, default=-1)
	ap.add_argument("--split", action="store_true")
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
	all_rows = [v2m.PLOIDY_MAX] + list(range(ds.n_copies))
	pitch = (ctx.max_unaligned_length + 255) // 256 * 256
	batch = min(args.batch_rows, len(all_rows))
	out = torch.empty(batch * pitch, dtype=torch.uint8, device=dev)
	OPS = {"resolve": N.KERNEL_RESOLVE, "count_unaligned+scan": N.KERNEL_UNALIGNED_COUNT, "count_row_ops": N.KERNEL_ROW_OPS_COUNT,
		"scan_row_ops": N.KERNEL_ROW_OPS_SCAN, "emit_row_ops": N.KERNEL_ROW_OPS_EMIT}
	SPLICE = {"resolve": N.KERNEL_RESOLVE, "count_unaligned+scan": N.KERNEL_UNALIGNED_COUNT, "splice_unaligned": N.KERNEL_SPLICE_UNALIGNED}

	def profiled(fn, kernels):
		ctx.synchronize()
		ctx.profile_reset()
		ctx.profile_enable(True)
		t0 = time.perf_counter()
		result = fn()
		ctx.synchronize()
		wall = (time.perf_counter() - t0) * 1e3
		got = {name: ctx.profile_get(k) for name, k in kernels.items()}
		ctx.profile_enable(False)
		return wall, {name: round(ms, 4) for name, (_, ms) in got.items()}, {name: int(n) for name, (n, _) in got.items()}, result

	def splice(rows):
		for r0 in range(0, len(rows), batch):
			ctx.splice_rows_device(rows[r0:r0 + batch], out.data_ptr(), pitch, unaligned=True)

	def ops_stats(got):
		n_ops = np.array([len(o) for o, _ in got])
		return {"mean": round(float(n_ops.mean()), 1), "min": int(n_ops.min()), "max": int(n_ops.max())}, int(n_ops.sum())

	results = []
	PASSES = ("count_row_ops", "scan_row_ops", "emit_row_ops")
	for rows in ((all_rows[:batch], all_rows) if args.split else ()):
		ctx.row_ops(rows[:8])          # warm-up: the 0-padded template, the tile table, scratch
		ctx.row_ops(rows[:8], split_match=True)
		best = {False: None, True: None}
		for _ in range(args.repeats):  # alternated
			for split in (False, True):
				wall, ms, launches, got = profiled(lambda: ctx.row_ops(rows, split_match=split), OPS)
				if best[split] is None or wall < best[split][0]:
					best[split] = (wall, ms, launches, ops_stats(got))
				del got
		legs = {}
		for split, name in ((False, "unsplit"), (True, "split")):
			wall, ms, launches, (per_row, total) = best[split]
			legs[name] = {"host_to_host_ms": round(wall, 3), "device_ms": ms, "launches": launches, "passes_device_ms": round(sum(ms[k] for k in PASSES), 4),
				"ops_per_row": per_row, "ops": total, "bytes_returned": total * 8}
		results.append({"rows": len(rows), "unsplit": legs["unsplit"], "split": legs["split"],
			"split_over_unsplit": dict({k: round(legs["split"]["device_ms"][k] / legs["unsplit"]["device_ms"][k], 4) for k in PASSES},
				passes=round(legs["split"]["passes_device_ms"] / legs["unsplit"]["passes_device_ms"], 4), ops=round(legs["split"]["ops"] / legs["unsplit"]["ops"], 4))})
	for rows in (() if args.split else (all_rows[:batch], all_rows)):
		ctx.row_ops(rows[:8])          # warm-up: the 0-padded template, the tile table, scratch
		splice(rows[:8])
		best_ops = best_splice = None
		for _ in range(args.repeats):  # alternated
			wall, ms, launches, got = profiled(lambda: ctx.row_ops(rows), OPS)
			if best_ops is None or wall < best_ops[0]:
				best_ops = (wall, ms, got, launches)
			wall, ms, launches, _ = profiled(lambda: splice(rows), SPLICE)
			if best_splice is None or wall < best_splice[0]:
				best_splice = (wall, ms, launches)
		n_ops = np.array([len(o) for o, _ in best_ops[2]])
		new_passes = sum(best_ops[1][k] for k in ("count_row_ops", "scan_row_ops", "emit_row_ops"))
		yardstick = best_splice[1]["count_unaligned+scan"] + best_splice[1]["splice_unaligned"]
		results.append({"rows": len(rows), "row_ops": {"host_to_host_ms": round(best_ops[0], 3), "device_ms": best_ops[1], "launches": best_ops[3], "new_passes_device_ms": round(new_passes, 4),
				"ops_per_row": {"mean": round(float(n_ops.mean()), 1), "min": int(n_ops.min()), "max": int(n_ops.max())}, "bytes_returned": int(n_ops.sum()) * 8},
			"unaligned_splice_same_rows": {"wall_ms": round(best_splice[0], 3), "device_ms": best_splice[1], "launches": best_splice[2], "count_plus_splice_device_ms": round(yardstick, 4),
				"bytes_written": int(sum(n for _, n in best_ops[2]))},
			"new_passes_over_yardstick": round(new_passes / yardstick, 4) if yardstick else None})
	metric = "row alignment ops (v2m_row_ops) against count_unaligned + splice_unaligned on the same rows, device time by pass"
	if args.split:
		metric = "row alignment ops with V2M_OPS_SPLIT_MATCH against the unsplit passes of the same build on the same rows, device time by pass"
	record = {"metric": metric, "config": args.config,
		"aligned_length": g.aligned_length, "edges": g.edge_count, "batch_rows": batch, "repeats": args.repeats, "results": results}

	if args.check_row >= 0:
		sys.path.insert(0, os.path.join(ROOT, "tests"))
		import oracle
		import row_ops_model as M
		copy = args.check_row
		words = np.zeros(ds.path_rows // 64 * 64, dtype=np.uint64)
		words[:ds.path_rows // 64] = ds.copy_column(copy)          # the copy as column 0 of a 64-copy matrix
		og = oracle.graph_from_arrays(g.reference_positions, g.aligned_positions, g.alt_edge_targets, g.alt_edge_count_csum, g.label_offsets, g.label_bytes,
			words, ds.path_rows, 64, ["S"], [0, 1])
		og.ref = ds.reference
		row, ref_is_base, row_is_base = M.column_walk(og, copy_index=0)
		assert row == og.output_sequence(og.ref, copy_index=0), "the model's walk differs from the oracle's row"
		want = M.ops_from_masks(ref_is_base, row_is_base)
		if args.split:
			import row_ops_eqx_model as E
			ref_row = M.column_walk(og)[0]
			want = E.ops_from_rows(ref_is_base, row_is_base, np.frombuffer(ref_row, np.uint8), np.frombuffer(row, np.uint8))
			assert np.array_equal(E.fold(want), M.ops_from_masks(ref_is_base, row_is_base))
		(got, length), = ctx.row_ops([copy], split_match=args.split)
		n = min(len(got), len(want))
		differing = int((got[:n] != want[:n]).any(axis=1).sum()) + abs(len(got) - len(want))
		record["spot_check"] = {"copy": copy, "ops": int(len(want)), "differing_ops": differing, "row_length_matches": bool(length == int(row_is_base.sum()))}
		if args.split:
			record["spot_check"]["X_ops"] = int((want[:, 0] == E.OP_X).sum())
			record["spot_check"]["X_bytes"] = int(want[want[:, 0] == E.OP_X, 1].sum())
	ctx.close()
	text = json.dumps(record)
	print(text)
	if args.out:
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, "w") as f:
			f.write(text + "\n")


if __name__ == "__main__":
	main()
