"""BGZF input on a BASELINE config (default config 3: 10 GB of VCF text; put TMPDIR on /dev/shm): the text is compressed into BGZF at
zlib level 6 (bgzip's default, 65 280-byte pieces) by a 16-process pool, then three alternated runs of
  - kernel:     V2M_KERNEL_INFLATE device time, as GB/s of output;
  - whole call: v2m_bgzf_decompress host to host into pageable memory, as GB/s, split by V2M_INFLATE_TIMING into scan / host staging /
                H2D / D2H / waiting / host copy out; once into a fresh malloc'd buffer (as the driver's) and once more into the same,
                pre-faulted buffer;
  - CPU:        zlib over the same members in 16 processes (started and warmed before the clock), as GB/s of output;
  - CLI:        -H -a x.vcf.gz -r x.fa -c 1 -s /dev/null --region=1-1000 against the same run with -a x.vcf, whole process and up to the
                end of the graph build ("Done. Handled variants" on stderr);
and the first-touch cost of a pageable buffer of the text's size.  Writes one JSON file (--out).

usage: TMPDIR=/dev/shm python tools/inflate_bench.py [--config config3] [--out profiles/r06/inflate_bench.json]"""

import argparse
import ctypes as C
import json
import mmap
import multiprocessing as mp
import os
import statistics
import struct
import subprocess
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")
PIECE = 65280


def _member(chunk):
	c = zlib.compressobj(6, zlib.DEFLATED, -15)
	payload = c.compress(chunk) + c.flush()
	size = 18 + len(payload) + 8
	return b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\0BC\x02\0" + struct.pack("<H", size - 1) + payload + struct.pack("<II", zlib.crc32(chunk), len(chunk))


def _compress_range(args):
	path, a, b = args
	with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as m:
		return b"".join(_member(m[i:min(i + PIECE, b)]) for i in range(a, b, PIECE))


def compress_file(src, dst, processes=16):
	n = os.path.getsize(src)
	step = PIECE * 256
	ranges = [(src, a, min(a + step, n)) for a in range(0, n, step)]
	with mp.get_context("spawn").Pool(processes) as pool, open(dst, "wb") as f:
		for blob in pool.imap(_compress_range, ranges):
			f.write(blob)
		f.write(EOF_MEMBER)


def _inflate_range(args):
	path, offsets = args
	out = 0
	with open(path, "rb") as f, mmap.mmap(f.fileno(), 0, access=mmap.ACCESS_READ) as m:
		for a, b in offsets:
			d = zlib.decompressobj(-15)
			out += len(d.decompress(m[a + 18:b - 8]))
	return out


def member_offsets(data):
	offs, pos = [], 0
	while pos < len(data):
		size = struct.unpack_from("<H", data, pos + 16)[0] + 1
		offs.append((pos, pos + size))
		pos += size
	return offs


def cli_run(args):
	t0 = time.monotonic()
	p = subprocess.Popen([CLI] + args, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
	t_graph, err = None, []
	for line in p.stderr:
		err.append(line)
		if t_graph is None and line.startswith(b"Done. Handled variants"):
			t_graph = time.monotonic() - t0
	rc = p.wait()
	if rc:
		raise RuntimeError(b"".join(err).decode(errors="replace"))
	return time.monotonic() - t0, t_graph


def spread(xs):
	return {"runs": [round(x, 4) for x in xs], "median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4)}


def main():
	ap = argparse.ArgumentParser()
	ap.add_argument("--config", default="config3")
	ap.add_argument("--runs", type=int, default=3)
	ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r06", "inflate_bench.json"))
	a = ap.parse_args()
	from vcf2multialign_amd import _native as N, synth
	import vcf2multialign_amd as v2m

	tmp = tempfile.mkdtemp(prefix="inflate_bench.", dir=os.environ.get("TMPDIR", "/tmp"))
	fa, vcf, gz = (os.path.join(tmp, a.config + s) for s in (".fa", ".vcf", ".vcf.gz"))
	rec = {"config": a.config, "tool": "tools/inflate_bench.py", "labels": "every figure below is measured on one MI355X and its host's 16 CPUs"}
	try:
		print("writing the text of", a.config, flush=True)
		t = time.time(); synth.dataset(a.config).write_fasta_and_vcf(fa, vcf); rec["write_text_s"] = round(time.time() - t, 2)
		t = time.time(); compress_file(vcf, gz); rec["compress_16_processes_s"] = round(time.time() - t, 2)
		with open(gz, "rb") as f:
			data = f.read()
		n_text = os.path.getsize(vcf)
		m, n_bytes, eof = v2m.bgzf_scan(data)
		assert n_bytes == n_text and eof
		rec.update(compressed_bytes=len(data), decompressed_bytes=n_bytes, members=m, ratio=round(n_bytes / len(data), 2))
		print(json.dumps(rec), flush=True)

		# Buffers as the driver gets them (new char[] = malloc: pages untouched until the library's copy out writes them).  First touch of
		# such a buffer of the text's size: one memset over fresh pages against a second one.
		libc = C.CDLL(None)
		libc.malloc.restype = C.c_void_p
		libc.malloc.argtypes = [C.c_size_t]
		libc.free.argtypes = [C.c_void_p]
		libc.memset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
		p = libc.malloc(n_bytes)
		t = time.time(); libc.memset(p, 1, n_bytes); first = time.time() - t
		t = time.time(); libc.memset(p, 2, n_bytes); second = time.time() - t
		libc.free(p)
		rec["first_touch"] = {"first_memset_s": round(first, 3), "second_memset_s": round(second, 3), "page_fault_cost_s": round(first - second, 3),
			"note": "one thread; the library's copy out writes the pages on up to 8"}

		lib = N.load()
		offs = member_offsets(data)
		k = (len(offs) + 15) // 16
		chunks = [(gz, offs[i:i + k]) for i in range(0, len(offs), k)]
		kernel, fresh, faulted, cpu, split = [], [], [], [], []
		with v2m.Context(0) as ctx, mp.get_context("spawn").Pool(16) as pool:
			pool.map(abs, range(64))                                     # the workers are up before any clock starts
			ctx.profile_enable(True)
			src = C.c_char_p(data)
			n_out = C.c_uint64()

			def call(dst):   # whole call (V2M_INFLATE_TIMING's line captured from fd 2): seconds, the line
				os.environ["V2M_INFLATE_TIMING"] = "1"
				log = tempfile.TemporaryFile()
				saved = os.dup(2)
				os.dup2(log.fileno(), 2)
				try:
					t = time.time()
					rc = lib.v2m_bgzf_decompress(ctx._h, src, len(data), dst, n_bytes, C.byref(n_out))
					dt = time.time() - t
				finally:
					os.dup2(saved, 2)
					os.close(saved)
					del os.environ["V2M_INFLATE_TIMING"]
				assert rc == 0 and n_out.value == n_bytes, lib.v2m_last_error(ctx._h)
				log.seek(0)
				return dt, log.read().decode().strip()

			for r in range(a.runs):
				dst = libc.malloc(n_bytes)
				try:
					ctx.profile_reset()
					dt, line = call(dst)                                 # into fresh pages, as the driver does
					launches, ms = ctx.profile_get(N.KERNEL_INFLATE)
					fresh.append(n_bytes / dt / 1e9)
					kernel.append(n_bytes / (ms / 1e3) / 1e9)
					split.append("fresh buffer: " + line)
					dt, line = call(dst)                                 # the same buffer again: every page already faulted in
					faulted.append(n_bytes / dt / 1e9)
					split.append("pre-faulted buffer: " + line)
					if r == 0:
						with open(vcf, "rb") as f:
							assert C.string_at(dst, 1 << 20) == f.read(1 << 20)
				finally:
					libc.free(dst)
				t = time.time()                                          # CPU baseline
				got = sum(pool.map(_inflate_range, chunks))
				cpu.append(n_bytes / (time.time() - t) / 1e9)
				assert got == n_bytes
				print("run", r, "kernel %.1f GB/s, call %.1f GB/s (fresh) %.1f (pre-faulted), cpu %.1f GB/s" % (kernel[-1], fresh[-1], faulted[-1], cpu[-1]), flush=True)
		rec["kernel_GBps_of_output"] = spread(kernel)
		rec["kernel_launches_per_call"] = launches
		rec["whole_call_fresh_buffer_GBps"] = spread(fresh)
		rec["whole_call_prefaulted_buffer_GBps"] = spread(faulted)
		rec["whole_call_split"] = split
		rec["cpu_zlib_16_processes_GBps"] = spread(cpu)

		common = ["-H", "-r", fa, "-c", "1", "-s", "/dev/null", "--region=1-1000"]
		cli = {"gz": [], "plain": []}
		for r in range(a.runs):
			for tag, src_path in (("gz", gz), ("plain", vcf)):
				cli[tag].append(cli_run(common + ["-a", src_path]))
		rec["cli"] = {tag: {"whole_process_s": spread([w for w, _ in xs]), "to_graph_built_s": spread([g for _, g in xs])} for tag, xs in cli.items()}
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
