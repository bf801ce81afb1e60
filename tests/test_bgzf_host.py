"""BGZF framing on the host (no GPU): v2m_bgzf_frame_stored / v2m_bgzf_bound, and the CLI's --bgzf rejections, which come before
any device is opened."""

import gzip
import os
import struct
import subprocess
import zlib

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CLI = os.path.join(ROOT, "vcf2multialign_amd", "bin", "vcf2multialign")
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


@pytest.fixture(scope="module")
def v2m():
	from vcf2multialign_amd import build
	build.build_native()
	import vcf2multialign_amd as v
	return v


def bgzf_members(data):
	"""Splits a BGZF stream into its members, checking every header field the format fixes; returns [(member, payload)]."""
	out, pos = [], 0
	while pos < len(data):
		assert data[pos:pos + 4] == b"\x1f\x8b\x08\x04", "magic, CM 8, FLG.FEXTRA"
		xlen, = struct.unpack_from("<H", data, pos + 10)
		assert xlen == 6
		assert data[pos + 12:pos + 16] == b"BC\x02\x00", "one BC subfield of SLEN 2"
		bsize, = struct.unpack_from("<H", data, pos + 16)
		size = bsize + 1
		assert size <= 65536 and pos + size <= len(data)
		member = data[pos:pos + size]
		crc, isize = struct.unpack_from("<II", member, size - 8)
		assert isize <= 65280
		payload = zlib.decompress(member[18:size - 8], -15)
		assert len(payload) == isize and zlib.crc32(payload) == crc
		out.append((member, payload))
		pos += size
	return out


@pytest.mark.parametrize("n", [0, 1, 65280, 65281, 200000])
def test_frame_stored_round_trips(v2m, n):
	data = os.urandom(n)
	framed = v2m.bgzf_frame_stored(data)
	if n == 0:
		assert framed == EOF_MEMBER
		return
	assert gzip.decompress(framed) == data
	members = bgzf_members(framed)
	assert len(members) == (n + 65279) // 65280
	assert b"".join(p for _, p in members) == data
	assert all(len(p) == 65280 for _, p in members[:-1])
	assert gzip.decompress(framed + v2m.bgzf_frame_stored(b"")) == data


def test_eof_member_is_an_empty_member(v2m):
	assert v2m.bgzf_frame_stored(b"") == EOF_MEMBER
	assert bgzf_members(EOF_MEMBER)[0][1] == b""
	assert gzip.decompress(EOF_MEMBER) == b""


@pytest.mark.parametrize("n", [0, 1, 31, 65279, 65280, 65281, 130560, 10 ** 6, 10 ** 10])
def test_bound_covers_the_stored_worst_case(v2m, n):
	pieces = -(-n // 65280)
	assert v2m.bgzf_bound(n) >= (28 if n == 0 else n + 31 * pieces)
	if 0 < n <= 200000:
		assert len(v2m.bgzf_frame_stored(b"A" * n)) <= v2m.bgzf_bound(n)


def test_frame_stored_refuses_a_short_destination(v2m):
	import ctypes as C
	lib = v2m.load_library()
	dst = C.create_string_buffer(40)
	n = C.c_uint64(99)
	assert lib.v2m_bgzf_frame_stored(b"0123456789", 10, dst, 40, C.byref(n)) == 1
	assert lib.v2m_bgzf_frame_stored(b"0123456789", 10, dst, 41, C.byref(n)) == 0 and n.value == 41


def _cli(args):
	from vcf2multialign_amd import build
	build.build_native()
	return subprocess.run([CLI] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)


@pytest.mark.parametrize("extra,message", [
	([], b"--bgzf requires -s"),
	(["-s", "out.a2m.gz", "--pipe=cat"], b"--bgzf cannot be combined with --pipe"),
	(["-s", "out.a2m.gz", "--output-sequences-separate"], b"--bgzf cannot be combined with --output-sequences-separate"),
	(["--output-sequences-separate"], b"--bgzf requires -s"),
])
def test_cli_rejects_bgzf_combinations_before_any_device(tmp_path, extra, message):
	"""The inputs do not even exist: the checks come before the reference is read and before a device is opened."""
	r = _cli(["--haplotypes", "-r", str(tmp_path / "missing.fa"), "-a", str(tmp_path / "missing.vcf"), "-c", "1", "--bgzf"] + extra)
	assert r.returncode != 0
	assert message in r.stderr, r.stderr.decode()
	assert b"Reading the reference" not in r.stderr


def test_cli_help_lists_bgzf():
	r = _cli(["--help"])
	assert b"--bgzf" in r.stderr
