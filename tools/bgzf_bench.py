"""BGZF output on config 3: the encoder's input rate (V2M_KERNEL_BGZF device time), bytes per base, and end-to-end Gbases/s of
v2m_splice_rows into bench.py's C checksum sink with and without V2M_SPLICE_BGZF, alternated in one process.  Prints one JSON line.

  python tools/bgzf_bench.py [--copies 255] [--repeats 3] [--unaligned]
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
	ap.add_argument("--copies", type=int, default=255, help="haplotype rows after the REF row (copies 0 .. copies - 1)")
	ap.add_argument("--repeats", type=int, default=3)
	ap.add_argument("--sink-threads", type=int, default=4)
	ap.add_argument("--unaligned", action="store_true")
	args = ap.parse_args()

	import torch
	import vcf2multialign_amd as v2m
	from vcf2multialign_amd import _native as N, build as B, synth

	ds = synth.dataset("config3")
	hp = (args.copies + 63) // 64 * 64
	ctx = v2m.Context(0)
	ctx.upload_graph(ds.graph, ds.reference)
	dev = torch.device("cuda", 0)
	thr = torch.from_numpy(ds.edge_thresholds.astype(np.int64)).to(torch.int32).to(dev)
	src = torch.empty(ds.path_rows // 64 * hp, dtype=torch.int64, device=dev)
	dst = torch.empty_like(src)
	torch.cuda.synchronize()
	ds.fill_paths_device(ctx.stream, src.data_ptr(), thr.data_ptr(), 0, hp)
	ctx.transpose_bits_device(src.data_ptr(), hp, ds.path_rows, dst.data_ptr())
	ctx.synchronize()
	ctx.set_paths_device(dst.data_ptr(), ds.path_rows, hp)
	batch = v2m.RowBatch([v2m.PLOIDY_MAX] + list(range(args.copies)))

	sl = C.CDLL(B.SYNTH_LIB_PATH)
	sl.v2ms_checksum_sink_create.restype = C.c_void_p
	sl.v2ms_checksum_sink_create.argtypes = [C.c_uint64, C.c_uint32]
	sl.v2ms_checksum_sink_destroy.argtypes = [C.c_void_p]
	for name in ("rows", "bytes"):
		getattr(sl, "v2ms_checksum_sink_" + name).restype = C.c_uint64
		getattr(sl, "v2ms_checksum_sink_" + name).argtypes = [C.c_void_p]
	sink_fn = C.cast(sl.v2ms_checksum_sink_fn, N.SINK_FN)
	base_flags = N.V2M_SPLICE_UNALIGNED if args.unaligned else 0

	def run(flags):
		state = sl.v2ms_checksum_sink_create(batch.n_rows, args.sink_threads)
		try:
			t = time.perf_counter()
			rc = ctx._lib.v2m_splice_rows(ctx._h, C.byref(batch.struct), base_flags | flags, sink_fn, state)
			secs = time.perf_counter() - t
			ctx._check(rc)
			assert sl.v2ms_checksum_sink_rows(state) == batch.n_rows
			return secs, int(sl.v2ms_checksum_sink_bytes(state))
		finally:
			sl.v2ms_checksum_sink_destroy(state)

	# bases: the plain run's bytes; warm-up of both paths (buffers, pinned slots, store calibration)
	_, bases = run(0)
	_, packed = run(N.V2M_SPLICE_BGZF)
	times = {"plain": [], "bgzf": []}
	for _ in range(args.repeats):
		times["plain"].append(run(0)[0])
		times["bgzf"].append(run(N.V2M_SPLICE_BGZF)[0])

	# encoder device time, in a pass of its own (event brackets around every slice's three kernels)
	ctx.profile_reset()
	ctx.profile_enable(True)
	run(N.V2M_SPLICE_BGZF)
	launches, enc_ms = ctx.profile_get(N.KERNEL_BGZF)
	splice_kernel = N.KERNEL_SPLICE_UNALIGNED if args.unaligned else N.KERNEL_SPLICE_ALIGNED
	_, splice_ms = ctx.profile_get(splice_kernel)
	ctx.profile_enable(False)

	best_plain, best_bgzf = min(times["plain"]), min(times["bgzf"])
	print(json.dumps({
		"config": "config3", "rows": batch.n_rows, "unaligned": args.unaligned, "bases": bases, "bgzf_bytes": packed,
		"bytes_per_base": packed / bases,
		"encoder_input_GBps": bases / (enc_ms * 1e-3) / 1e9, "encoder_ms": enc_ms, "encoder_launches": launches, "splice_ms": splice_ms,
		"e2e_plain_Gbases_per_s": bases / best_plain / 1e9, "e2e_bgzf_Gbases_per_s": bases / best_bgzf / 1e9,
		"link_plain_GBps": bases / best_plain / 1e9, "link_bgzf_GBps": packed / best_bgzf / 1e9,
		"times_s": times, "sink_threads": args.sink_threads,
	}))
	ctx.close()


if __name__ == "__main__":
	main()
