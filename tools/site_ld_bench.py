"""Site LD (v2m_site_ld) on a synthetic config, all rows (REF + every copy), over the whole row and over a 100-kb window, with the
default band (--ld-window 1000) and the widest (4096), at r^2 >= 1/5: the call host to host (sinks that only count what they are given)
and the three device times of its info, after two warm-up calls, best of --repeats with every repeat recorded; sites, candidates, pairs
and the planes' bytes; ld_pairs_kernel<false> on its own -- the pairs stage of a call without a pair sink, which is that kernel and the
scan of its cells -- as 64-bit word pairs per second beside the VALU ceiling that follows from --valu-per-word-pair, the vector
instructions per word pair of its inner loop counted in the compiler's output (section 8.9's derivation); and, in
the same run, v2m_variable_sites of the same rows through sinks that only count: the yardstick.
With --check the window's sites and pairs are held equal to those computed on the host from the rows v2m_splice_rows delivers for it,
at 1/5 and -- the synthetic sites are independent, so hardly a pair reaches 1/5 -- at 1/1000 and 0.
Prints one JSON line and, with --out, writes it (profiles/r15/site_ld_bench.json).

  python tools/site_ld_bench.py [--config config3] [--window 100000] [--repeats 3] [--check] [--out profiles/r15/site_ld_bench.json]
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

CUS, SIMDS, CYCLES_PER_WAVE_INSTRUCTION, CLOCK_HZ = 256, 4, 2, 2.4e9
CHECK_THRESHOLDS = ((1, 1000), (0, 1))      # the spot check's further thresholds: the synthetic sites are independent, and few pairs reach 1/5


def host_classes(a):
	low = a | 0x20
	cls = np.full(a.shape, 6, dtype=np.uint8)
	for k, ch in enumerate(b"acgtn"):
		cls[low == ch] = k
	cls[a == 0x2D] = 5
	return cls


def host_site_ld(cls, first_column, window_sites, num, den):
	"""(site columns, pair records) of the classes cls[n, L] under min_allele_count 1 and no column limit, in integers (int64 holds
	D^2 den' and num den'' for the row counts this tool runs: asserted)."""
	n = cls.shape[0]
	assert n <= 32768 and max(num, den) * (n * n // 4) ** 2 < 2 ** 62
	counts = np.stack([(cls == k).sum(axis=0) for k in range(4)])
	cols = np.flatnonzero((counts > 0).sum(axis=0) == 2)
	at = cls[:, cols]
	order = np.argsort(-(counts[:, cols] > 0).astype(np.int64), axis=0, kind="stable")      # the two present classes first, ascending
	lo, hi = order[0].astype(np.uint8), order[1].astype(np.uint8)
	carries = at == hi[None, :]
	called = carries | (at == lo[None, :])
	ca, ka = called.astype(np.int64), carries.astype(np.int64)
	N_, A, B, AB = ca.T @ ca, ka.T @ ca, ca.T @ ka, ka.T @ ka
	D = N_ * AB - A * B
	DEN = A * (N_ - A) * B * (N_ - B)
	s, t = np.triu_indices(len(cols), 1)
	keep = (t - s <= window_sites) & (DEN[s, t] != 0) & (D[s, t] * D[s, t] * den >= num * DEN[s, t])
	s, t = s[keep], t[keep]
	pairs = np.stack([s, t, N_[s, t], A[s, t], B[s, t], AB[s, t]], axis=1).astype(np.uint32)
	return cols.astype(np.uint64) + np.uint64(first_column), pairs


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--config", default="config3")
	ap.add_argument("--window", type=int, default=100000)
	ap.add_argument("--repeats", type=int, default=3)
	ap.add_argument("--views", default="window,whole")
	ap.add_argument("--ld-windows", default="1000,4096")
	ap.add_argument("--valu-per-word-pair", type=float, default=18.125, help="VALU instructions per 64-bit word pair of ld_pairs_kernel's inner loop")
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
	T, C_ = N.LD_TILE, N.LD_CHUNK_WORDS
	NUM, DEN = 1, 5
	ceiling = CUS * SIMDS * 64 / CYCLES_PER_WAVE_INSTRUCTION * CLOCK_HZ / args.valu_per_word_pair      # word pairs a second: a lane works on one word pair at a time
	null = C.cast(None, N.LD_SINK_FN)

	def raw_call(window_sites, with_pairs=True):
		"""The host form through sinks that only count: (host to host ms, info, what the sinks saw)."""
		seen = {"site_calls": 0, "blocks": 0, "pairs": 0, "bytes": 0}

		def on_sites(_user, _records, count):
			seen["site_calls"] += 1
			seen["bytes"] += 24 * int(count)
			return 0

		def on_pairs(_user, _records, count):
			seen["blocks"] += 1
			seen["pairs"] += int(count)
			seen["bytes"] += 24 * int(count)
			return 0

		params = N.SiteLdParams(window_sites, 1, NUM, DEN, 0)
		info = N.SiteLdInfo()
		sites_sink, pairs_sink = N.LD_SINK_FN(on_sites), N.LD_SINK_FN(on_pairs)
		ctx.synchronize()
		t0 = time.perf_counter()
		rc = ctx._lib.v2m_site_ld(ctx._h, C.byref(batch.struct), C.byref(params), sites_sink, pairs_sink if with_pairs else null, None, C.byref(info))
		wall = (time.perf_counter() - t0) * 1e3
		ctx._check(rc)
		return wall, {name: getattr(info, name) for name, _ in N.SiteLdInfo._fields_}, seen

	def one(window_sites):
		ctx.profile_reset()
		ctx.profile_enable(True)
		wall, info, seen = raw_call(window_sites)
		_, count_only, _ = raw_call(window_sites, with_pairs=False)
		ctx.profile_enable(False)
		ctx.profile_reset()
		assert seen["pairs"] == info["n_pairs"], (seen, info)
		V = int(info["n_sites"])
		strips, words = -(-V // T), -(-n // 64)
		blocks = min(strips, (window_sites + T - 1) // T + 1)
		tiles = sum(min(blocks, strips - ti) for ti in range(strips))
		word_pairs = tiles * T * T * -(-words // C_) * C_          # what a launch computes: whole tiles of the band, padded chunks
		rec = {"host_to_host_ms": round(wall, 3), "info": {k: (round(v, 4) if isinstance(v, float) else int(v)) for k, v in info.items()},
			"bytes_over_the_link": seen["bytes"], "pair_blocks": seen["blocks"], "plane_bytes": 16 * strips * T * words,
			"count_pass_ms": round(count_only["pairs_ms"], 4), "tiles": tiles, "word_pairs_computed": int(word_pairs)}
		if count_only["pairs_ms"] > 0 and V:
			rate = word_pairs / (count_only["pairs_ms"] * 1e-3)
			rec["count_kernel"] = {"word_pairs_per_s": round(rate / 1e9, 2), "unit": "1e9 64-bit word pairs per second", "valu_per_word_pair": args.valu_per_word_pair,
				"valu_ceiling_word_pairs_per_s": round(ceiling / 1e9, 2), "share_of_ceiling": round(rate / ceiling, 3)}
		return rec

	def variable_sites():
		seen = [0]

		def on_columns(_user, _columns, n_sites):
			seen[0] += 4 * int(n_sites)
			return 0

		def on_rows(_user, _first_row, n_rows, _bytes, pitch, _n_sites):
			seen[0] += int(n_rows) * int(pitch)
			return 0

		info = N.VariableSitesInfo()
		a, b = N.SITE_COLUMNS_SINK_FN(on_columns), N.SITE_ROWS_SINK_FN(on_rows)
		ctx.synchronize()
		t0 = time.perf_counter()
		rc = ctx._lib.v2m_variable_sites(ctx._h, C.byref(batch.struct), 0, a, b, None, C.byref(info))
		wall = (time.perf_counter() - t0) * 1e3
		ctx._check(rc)
		return round(wall, 3), int(info.n_sites), seen[0]

	ld_windows = [int(x) for x in args.ld_windows.split(",")]
	results = {}
	L_whole = ctx.aligned_length
	window_begin = (L_whole // 2) // 16 * 16 + 5
	for view in args.views.split(","):
		if "window" == view:
			ctx.set_column_window(window_begin, min(L_whole, window_begin + args.window))
		else:
			ctx.set_column_window(0, L_whole)
		L = ctx.window_length
		for _ in range(2):                                      # warm-ups: scratch, the planes, the cells and the pinned slots at their full size
			raw_call(max(ld_windows))
		variable_sites()
		runs = {w: [] for w in ld_windows}
		yardstick = []
		for _ in range(args.repeats):          # alternated
			for w in ld_windows:
				runs[w].append(one(w))
			yardstick.append(variable_sites())
		out = {"columns": int(L), "rows": n}
		for w, recs in runs.items():
			best = min(recs, key=lambda r: r["host_to_host_ms"])
			out["ld_window_%d" % w] = dict(best, host_to_host_ms_all=[r["host_to_host_ms"] for r in recs], counts_ms_all=[r["info"]["counts_ms"] for r in recs],
				pack_ms_all=[r["info"]["pack_ms"] for r in recs], pairs_ms_all=[r["info"]["pairs_ms"] for r in recs], count_pass_ms_all=[r["count_pass_ms"] for r in recs])
		out["variable_sites"] = {"host_to_host_ms": min(y[0] for y in yardstick), "host_to_host_ms_all": [y[0] for y in yardstick], "n_sites": yardstick[0][1], "bytes_over_the_link": yardstick[0][2]}
		if "window" == view and args.check:
			bodies = [None] * n
			def on_row(i, body):
				bodies[i] = np.frombuffer(body, dtype=np.uint8).copy()
			ctx.splice_rows(batch, sink=on_row)
			cls = host_classes(np.stack(bodies))
			check = {"rows": n, "columns": int(L)}
			for w, (num, den) in [(w, (NUM, DEN)) for w in ld_windows] + [(ld_windows[0], r2) for r2 in CHECK_THRESHOLDS]:
				want_columns, want_pairs = host_site_ld(cls, window_begin, w, num, den)
				sites, pairs = ctx.site_ld(batch, window_sites=w, min_r2=(num, den))
				got_pairs = np.stack([pairs[k] for k in ("site_a", "site_b", "n", "n_a", "n_b", "n_ab")], axis=1) if len(pairs) else np.zeros((0, 6), dtype=np.uint32)
				check["ld_window_%d_r2_%d_%d" % (w, num, den)] = {"sites_on_the_host": int(len(want_columns)), "n_sites": int(len(sites)), "columns_equal": bool(np.array_equal(sites["column"], want_columns)),
					"pairs_on_the_host": int(len(want_pairs)), "n_pairs": int(len(pairs)), "pairs_equal": bool(got_pairs.shape == want_pairs.shape and np.array_equal(got_pairs, want_pairs))}
			out["spot_check"] = check
		results[view] = out
	ctx.set_column_window(0, L_whole)
	record = {"metric": "site LD (v2m_site_ld) of all rows at r^2 >= 1/5: host to host, device time by stage, ld_pairs_kernel<false> against its VALU ceiling, v2m_variable_sites of the same rows beside it",
		"config": args.config, "aligned_length": int(L_whole), "edges": g.edge_count, "repeats": args.repeats, "ld_tile": T, "ld_chunk_words": C_,
		"ceiling_basis": {"cus": CUS, "simds_per_cu": SIMDS, "cycles_per_wave_instruction": CYCLES_PER_WAVE_INSTRUCTION, "clock_hz": CLOCK_HZ}, "results": results}
	ctx.close()
	text = json.dumps(record)
	print(text)
	if args.out:
		os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
		with open(args.out, "w") as f:
			f.write(text + "\n")
	if args.check and "window" in results:
		bad = [k for k, v in results["window"].get("spot_check", {}).items() if isinstance(v, dict) and not (v["columns_equal"] and v["pairs_equal"])]
		if bad or "spot_check" not in results["window"]:
			sys.exit("the window's result differs from the host's: %s" % ", ".join(bad))


if __name__ == "__main__":
	main()
