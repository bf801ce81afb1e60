"""--gpu-parse on a BASELINE config (default config 3: 10 GB of VCF text, 383 MB as BGZF; put TMPDIR on /dev/shm).  The text is compressed
as tools/inflate_bench.py does it (zlib level 6, 65 280-byte pieces), then `--runs` alternated runs (default three) of
  - scan:  v2m_vcf_scan over the compressed and over the plain bytes with callbacks that only count: wall time, V2M_KERNEL_VCF and
           V2M_KERNEL_INFLATE device time and launches on the same slices, lines and declined lines, the bytes a chunk brings to the host;
  - CLI:   -H -r x.fa -c 1 -s /dev/null --region=1-1000 from x.vcf.gz and from x.vcf, each with and without --gpu-parse, and, with
           --parent-cli, the same two inputs through the parent commit's driver: whole process, up to the end of the graph build ("Done.
           Handled variants" on stderr), and the child's peak RSS (wait4's ru_maxrss); --verbose's "lines scanned, N declined" is kept;
  - merge: with V2M_READER_TIMING=1 once per --gpu-parse form, the reader's own split (stderr lines that begin with "[vcf reader]").
Every form is run once per round, the forms in turn, so that a drift of the box lands on all of them.  Writes one JSON file (--out).

usage: TMPDIR=/dev/shm python tools/gpu_parse_bench.py [--config config3] [--parent-cli PATH] [--out profiles/r07/gpu_parse_bench.json]"""

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")

from inflate_bench import compress_file, spread   # noqa: E402


def cli_run(cli, args, env=None):
	"""One driver run: (whole process s, to "graph built" s, peak RSS in MiB, stderr lines kept)."""
	t0 = time.monotonic()
	p = subprocess.Popen([cli] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, env=env)
	t_graph, err, kept = None, [], []
	for line in p.stderr:
		err.append(line)
		if t_graph is None and line.startswith(b"Done. Handled variants"):
			t_graph = time.monotonic() - t0
		if b"lines scanned" in line or line.startswith(b"[vcf reader]") or b"GPU parse not supported" in line:
			kept.append(line.decode(errors="replace").strip())
	_, status, usage = os.wait4(p.pid, 0)
	whole = time.monotonic() - t0
	p.returncode = os.waitstatus_to_exitcode(status)
	if p.returncode:
		raise RuntimeError(b"".join(err).decode(errors="replace"))
	return whole, t_graph, usage.ru_maxrss / 1024.0, kept


def scan_once(ctx, lib, N, data, chrom):
	"""v2m_vcf_scan with callbacks that only count.  The layout is the first record's, nothing excluded."""
	from vcf2multialign_amd.context import first_record_layout
	import numpy as np
	keep, tally = [], dict(chunks=0, lines=0, declined=0, bytes_to_host=0)

	def on_layout(_user, _line_index, line, length, out):
		d = first_record_layout(C.string_at(line, length))
		cb = np.ascontiguousarray(d["copy_begin"], dtype=np.uint32)
		rl = np.ascontiguousarray(d["row_lookup"] if len(d["row_lookup"]) else [0], dtype=np.int32)
		keep.extend([cb, rl])
		out[0].n_samples, out[0].n_rows, out[0].words_per_column = d["n_samples"], d["n_rows"], d["words_per_column"]
		out[0].copy_begin, out[0].row_lookup = cb.ctypes.data, rl.ctypes.data
		return 0

	def on_chunk(_user, c):
		c = c[0]
		lines = np.frombuffer(C.string_at(c.lines, c.n_lines * C.sizeof(N.VcfLine)), dtype=N.VCF_LINE_DTYPE)
		tally["chunks"] += 1
		tally["lines"] += int(c.n_lines)
		tally["declined"] += int((lines["kind"] == 3).sum())
		tally["bytes_to_host"] += int(c.n_lines) * C.sizeof(N.VcfLine) + int(c.head_bytes) + 8 * int(c.n_columns) * int(c.words_per_column)
		return 0

	lf, cf = N.VCF_LAYOUT_FN(on_layout), N.VCF_CHUNK_FN(on_chunk)
	ctx.profile_reset()
	t = time.monotonic()
	rc = lib.v2m_vcf_scan(ctx._h, C.cast(C.c_char_p(data), C.c_void_p), len(data), chrom.encode(), lf, cf, None)
	dt = time.monotonic() - t
	assert rc == 0, lib.v2m_last_error(ctx._h)
	vcf_launches, vcf_ms = ctx.profile_get(N.KERNEL_VCF)
	inf_launches, inf_ms = ctx.profile_get(N.KERNEL_INFLATE)
	return dict(tally, wall_s=dt, vcf_ms=vcf_ms, vcf_launch_groups=vcf_launches, inflate_ms=inf_ms, inflate_launches=inf_launches)


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--config", default="config3")
	ap.add_argument("--chromosome", default="1")
	ap.add_argument("--runs", type=int, default=3)
	ap.add_argument("--parent-cli", default=None, help="the parent commit's driver, built on the same box, for the runs without --gpu-parse")
	ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "gpu_parse_bench.json"))
	a = ap.parse_args()
	from vcf2multialign_amd import _native as N, synth
	import vcf2multialign_amd as v2m

	tmp = tempfile.mkdtemp(prefix="gpu_parse_bench.", dir=os.environ.get("TMPDIR", "/tmp"))
	fa, vcf, gz = (os.path.join(tmp, a.config + s) for s in (".fa", ".vcf", ".vcf.gz"))
	rec = {"config": a.config, "tool": "tools/gpu_parse_bench.py", "runs": a.runs,
		"labels": "every figure below is measured on one MI355X and its host's 16 CPUs, the forms of a kind in turn within each round"}
	try:
		print("writing the text of", a.config, flush=True)
		synth.dataset(a.config).write_fasta_and_vcf(fa, vcf)
		compress_file(vcf, gz)
		rec.update(compressed_bytes=os.path.getsize(gz), text_bytes=os.path.getsize(vcf))
		print(json.dumps(rec), flush=True)

		# ---- the scan alone: device time of the parse beside the inflate, on the same slices
		lib = N.load()
		scans = {"gz": [], "plain": []}
		with v2m.Context(0) as ctx:
			ctx.profile_enable(True)
			for tag, path in (("gz", gz), ("plain", vcf)):   # (one input in memory at a time: the plain text is 10 GB)
				with open(path, "rb") as f:
					data = f.read()
				if tag == "gz":
					scan_once(ctx, lib, N, data, a.chromosome)   # warm-up, not counted: allocations, code load
				for r in range(a.runs):
					scans[tag].append(scan_once(ctx, lib, N, data, a.chromosome))
					s = scans[tag][-1]
					print("scan", tag, r, "wall %.3f s, VCF %.1f ms in %d groups, inflate %.1f ms in %d launches, %d lines, %d declined, %.1f MB to the host"
						% (s["wall_s"], s["vcf_ms"], s["vcf_launch_groups"], s["inflate_ms"], s["inflate_launches"], s["lines"], s["declined"], s["bytes_to_host"] / 1e6), flush=True)
				del data
		rec["scan"] = {tag: {
			"wall_s": spread([s["wall_s"] for s in xs]), "kernel_vcf_s": spread([s["vcf_ms"] / 1e3 for s in xs]), "kernel_inflate_s": spread([s["inflate_ms"] / 1e3 for s in xs]),
			"vcf_launch_groups": xs[0]["vcf_launch_groups"], "inflate_launches": xs[0]["inflate_launches"], "chunks": xs[0]["chunks"], "lines": xs[0]["lines"],
			"declined": xs[0]["declined"], "bytes_to_host": xs[0]["bytes_to_host"]} for tag, xs in scans.items()}

		# ---- the driver
		common = ["-H", "-r", fa, "-c", a.chromosome, "-s", "/dev/null", "--region=1-1000", "--verbose"]
		forms = [("gz_gpu_parse", CLI, gz, ["--gpu-parse"]), ("gz", CLI, gz, []), ("plain_gpu_parse", CLI, vcf, ["--gpu-parse"]), ("plain", CLI, vcf, [])]
		if a.parent_cli:
			forms += [("parent_gz", a.parent_cli, gz, []), ("parent_plain", a.parent_cli, vcf, [])]
		cli = {tag: [] for tag, _, _, _ in forms}
		for r in range(a.runs):
			for tag, exe, src, extra in forms:
				cli[tag].append(cli_run(exe, common + ["-a", src] + extra))
				print("cli", tag, r, "whole %.3f s, graph built %.3f s, peak RSS %.0f MiB" % cli[tag][-1][:3], flush=True)
		rec["cli"] = {tag: {"whole_process_s": spread([x[0] for x in xs]), "to_graph_built_s": spread([x[1] for x in xs]), "peak_rss_MiB": spread([x[2] for x in xs]),
			"said": xs[0][3]} for tag, xs in cli.items()}
		env = dict(os.environ, V2M_READER_TIMING="1")
		rec["reader_timing"] = {tag: cli_run(exe, common + ["-a", src] + extra, env=env)[3] for tag, exe, src, extra in forms[:4]}
	finally:
		for p in (fa, vcf, gz):
			if os.path.exists(p):
				os.unlink(p)
		os.rmdir(tmp)
	os.makedirs(os.path.dirname(a.out), exist_ok=True)
	with open(a.out, "w") as f:
		json.dump(rec, f, indent=1)
	print(json.dumps(rec, indent=1))


if __name__ == "__main__":
	main()
