"""BGZF input on the host (no GPU): v2m_bgzf_scan's members, bytes and EOF member, the framing it refuses, and the driver's refusals
of gzip that is not BGZF and of broken framing, which come before any device is opened."""

import gzip
import os
import struct
import subprocess

import pytest

from bgzf_input_util import EOF_MEMBER, bgzf, deflate_raw, member

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
FIX = os.path.join(HERE, "golden", "reference-fixtures", "variant-graph")

V2M_ERR_INVALID_ARGUMENT, V2M_ERR_UNSUPPORTED = 1, 3


@pytest.fixture(scope="module")
def v2m():
	from vcf2multialign_amd import build
	build.build_native()
	import vcf2multialign_amd as v
	return v


def text(n, seed=1):
	import random
	rng = random.Random(seed)
	return "".join("1\t%d\t.\tA\tC\t.\tPASS\t.\tGT\t%s\n" % (i, "\t".join(rng.choice(["0|0", "0|1", "1|1"]) for _ in range(20))) for i in range(n)).encode()[:n]


def test_scan_counts_members_and_bytes(v2m):
	data = text(200000)
	assert v2m.bgzf_scan(bgzf(data)) == (4 + 1, len(data), True)   # 3 full members of 65 280, one of 4 160, the EOF member
	assert v2m.bgzf_scan(bgzf(data, eof=False)) == (4, len(data), False)
	assert v2m.bgzf_scan(bgzf(data, piece=1000)) == (200 + 1, len(data), True)


def test_scan_empty_input_and_eof_member(v2m):
	assert v2m.bgzf_scan(b"") == (0, 0, False)
	assert v2m.bgzf_scan(EOF_MEMBER) == (1, 0, True)
	assert v2m.bgzf_scan(EOF_MEMBER + EOF_MEMBER) == (2, 0, True)
	assert v2m.bgzf_scan(bgzf(b"", piece=0, eof=False)) == (1, 0, True)    # zlib's empty member is the EOF member's bytes
	assert v2m.bgzf_scan(member(deflate_raw(b""), b"", mtime=1)) == (1, 0, False)   # an empty member that is not
	assert v2m.bgzf_scan(v2m.bgzf_frame_stored(b"xyz") + EOF_MEMBER) == (2, 3, True)


def scan_error(v2m, data):
	with pytest.raises(v2m.V2MError) as e:
		v2m.bgzf_scan(data)
	return e.value.code, str(e.value)


def test_scan_refuses_plain_gzip(v2m):
	code, msg = scan_error(v2m, gzip.compress(b"##fileformat=VCFv4.2\n"))
	assert code == V2M_ERR_UNSUPPORTED and "not BGZF" in msg and "bgzip" in msg


def test_scan_refuses_broken_framing(v2m):
	good = bgzf(text(70000), eof=False)
	first = struct.unpack_from("<H", good, 16)[0] + 1             # the second member's offset
	cases = {
		"wrong magic": (b"\x1f\x8c" + good[2:], 0),
		"wrong magic, second member": (good[:first] + b"\x00" + good[first + 1:], first),
		"XLEN != 6, second member": (good[:first + 10] + b"\x08" + good[first + 11:], first),
		"missing BC, second member": (good[:first + 12] + b"XY" + good[first + 14:], first),
		"BSIZE past the end": (good[:first + 16] + b"\xff\xff" + good[first + 18:], first),
		"truncated last member": (good[:-5], first),
		"truncated header": (good[:first + 7], first),
		"ISIZE > 65536": (good[:-4] + struct.pack("<I", 65537), first),
		"BSIZE below a header and footer": (good[:first + 16] + struct.pack("<H", 20) + good[first + 18:], first),
	}
	for what, (data, offset) in cases.items():
		code, msg = scan_error(v2m, data)
		assert code == V2M_ERR_INVALID_ARGUMENT, (what, msg)
		assert "compressed offset %d" % offset in msg, (what, msg)


def test_scan_first_member_without_bgzf_header_is_gzip_not_bgzf(v2m):
	data = b"x" * 1000
	for kw in (dict(xlen=8), dict(subfield=b"XY"), dict(flg=4 | 8)):
		code, msg = scan_error(v2m, member(deflate_raw(data), data, **kw))
		assert code == V2M_ERR_UNSUPPORTED and "bgzip" in msg, (kw, msg)


def test_scan_accepts_any_mtime_xfl_os(v2m):
	data = b"abc" * 1000
	m = member(deflate_raw(data), data, mtime=123456, xfl=2, os_=3)
	assert v2m.bgzf_scan(m + EOF_MEMBER) == (2, len(data), True)


def run_cli(args):
	assert os.path.exists(CLI), "build the host driver first (__graft_entry__.build())"
	env = dict(os.environ, HIP_VISIBLE_DEVICES="")   # no device, visible or not: these refusals come before one is needed
	return subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120, env=env)


def test_cli_refuses_plain_gzip_input_without_a_device(tmp_path, v2m):
	fa, vcf = os.path.join(FIX, "test-4.fa"), os.path.join(FIX, "test-4.vcf")
	vcf_gz, fa_gz = tmp_path / "x.vcf.gz", tmp_path / "x.fa.gz"
	vcf_gz.write_bytes(gzip.compress(open(vcf, "rb").read()))
	fa_gz.write_bytes(gzip.compress(open(fa, "rb").read()))
	for args in (["-r", fa, "-a", str(vcf_gz)], ["-r", str(fa_gz), "-a", vcf]):
		r = run_cli(["-H"] + args + ["-c", "1", "-s", str(tmp_path / "out.a2m")])
		err = r.stderr.decode()
		assert r.returncode != 0 and "not BGZF" in err and "bgzip" in err, err
		assert not (tmp_path / "out.a2m").exists()


def test_cli_refuses_truncated_bgzf_without_a_device(tmp_path, v2m):
	vcf = open(os.path.join(FIX, "test-4.vcf"), "rb").read()
	data = bgzf(vcf, piece=100, eof=False)
	cut = len(bgzf(vcf[:300], piece=100, eof=False))             # three whole members, then part of the fourth
	bad = tmp_path / "x.vcf.gz"
	bad.write_bytes(data[:cut + 30])
	r = run_cli(["-H", "-r", os.path.join(FIX, "test-4.fa"), "-a", str(bad), "-c", "1", "-s", str(tmp_path / "out.a2m")])
	err = r.stderr.decode()
	assert r.returncode != 0 and "compressed offset %d" % cut in err and "truncated" in err, err


def test_cli_missing_reference_message_unchanged(tmp_path, v2m):
	r = run_cli(["-H", "-r", str(tmp_path / "nope.fa"), "-a", os.path.join(FIX, "test-4.vcf"), "-c", "1", "-s", str(tmp_path / "o.a2m")])
	assert r.returncode != 0 and "Unable to read the reference" in r.stderr.decode()


def test_cli_reads_a_reference_from_a_pipe_unchanged(tmp_path, v2m):
	"""A FIFO (as -r <(samtools faidx ...) gives) is not probed for the gzip magic: the FASTA reader gets all of it, header line included.
	The reference is read before a device is needed, so its length shows up here without one."""
	import re
	import threading
	fa = os.path.join(FIX, "test-4.fa")
	common = ["-H", "-a", os.path.join(FIX, "test-4.vcf"), "-c", "1", "-s", str(tmp_path / "o.a2m")]
	want = re.search(rb"Reference length is (\d+)", run_cli(["-r", fa] + common).stderr)
	assert want, "the regular file's reference length"
	fifo = tmp_path / "ref.fifo"
	os.mkfifo(fifo)

	def feed():
		with open(fifo, "wb") as f:
			f.write(open(fa, "rb").read())
	threading.Thread(target=feed, daemon=True).start()
	r = run_cli(["-r", str(fifo)] + common)
	assert b"Reference length is %s." % want.group(1) in r.stderr, r.stderr.decode()


def test_host_graph_refuses_bgzf_without_a_context(tmp_path, v2m):
	from vcf2multialign_amd import host
	vcf = open(os.path.join(FIX, "test-4.vcf"), "rb").read()
	gz = tmp_path / "x.vcf.gz"
	gz.write_bytes(bgzf(vcf))
	with pytest.raises(ValueError, match="GPU context"):
		host.HostGraph(os.path.join(FIX, "test-4.fa"), str(gz), "1")
