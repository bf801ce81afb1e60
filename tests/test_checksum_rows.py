"""The row checksum (checksum_rows_kernel, v2m_checksum_rows_device) and its numpy twin checksum_rows_host, which between them verify every
full-size test and bench.py, against a model written here from the header's sentence:

    sum over 8-byte little-endian words w (zero padded past the row's length) of mix64((w_index + 1) * GOLDEN ^ word), plus mix64(length)

with Python integers, word by word (model()), and in numpy for the long rows (model_numpy(), held equal to model() on the short ones).
Neither imports checksum_rows_host.

The host tests need no GPU.  The GPU tests put every row into a buffer whose bytes from the row's length to its pitch are a non-zero guard,
which the kernel has to mask: lengths 0 ... 17 and either side of the kernel's block of 8192 words (65 536 bytes) with every length & 7
beside it, in the fixed-length and the per-row form; rows that end many blocks before the longest row of their call; 32 769 and 65 537
rows, where the second and third launch take their sums and lengths from an offset; the same call twice on one context.

Wall time on an MI355X: the device tests together below 1 s (65 537 rows twice: 0.24 s, most of it model())."""

import numpy as np
import pytest

MASK = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15
GUARD = 0xA5
BLOCK_BYTES = 8192 * 8          # the bytes of one workgroup of checksum_rows_kernel: 256 threads x 32 words


def mix64(z):
	z ^= z >> 30
	z = z * 0xBF58476D1CE4E5B9 & MASK
	z ^= z >> 27
	z = z * 0x94D049BB133111EB & MASK
	return z ^ (z >> 31)


def model(body):
	"""The header's sentence with Python integers."""
	body = bytes(body)
	padded = body + b"\0" * (-len(body) % 8)
	acc = mix64(len(body))
	for w in range(len(padded) // 8):
		acc += mix64(((w + 1) * GOLDEN & MASK) ^ int.from_bytes(padded[8 * w:8 * w + 8], "little"))
	return acc & MASK


def model_numpy(body):
	"""The same sum over numpy words (uint64 arithmetic wraps as the sum does)."""
	body = bytes(body)
	words = np.frombuffer(body + b"\0" * (-len(body) % 8), dtype="<u8").astype(np.uint64)
	with np.errstate(over="ignore"):
		z = np.arange(1, words.size + 1, dtype=np.uint64) * np.uint64(GOLDEN) ^ words
		z ^= z >> np.uint64(30)
		z *= np.uint64(0xBF58476D1CE4E5B9)
		z ^= z >> np.uint64(27)
		z *= np.uint64(0x94D049BB133111EB)
		z ^= z >> np.uint64(31)
		return (int(z.sum(dtype=np.uint64)) + mix64(len(body))) & MASK


def row_bytes(length, seed):
	"""`length` bytes without a zero among them (a zero byte and a byte past the end must not look alike)."""
	return np.random.default_rng(seed).integers(1, 256, size=length, dtype=np.uint8).tobytes()


SHORT = list(range(0, 18))
AROUND_A_BLOCK = list(range(BLOCK_BYTES - 8, BLOCK_BYTES + 10)) + [2 * BLOCK_BYTES - 1, 2 * BLOCK_BYTES, 2 * BLOCK_BYTES + 1]
RAGGED = [200000, 0, 7, BLOCK_BYTES, BLOCK_BYTES + 1, 1]


def test_the_lengths_are_the_ones_meant():
	assert AROUND_A_BLOCK[0] == 65528 and AROUND_A_BLOCK[17] == 65545 and AROUND_A_BLOCK[-3:] == [131071, 131072, 131073]
	assert {n & 7 for n in AROUND_A_BLOCK[:18]} == set(range(8)) and {n & 7 for n in SHORT} == set(range(8))


# ---- host --------------------------------------------------------------------------------------------------------------------------------

def test_model_spelled_out():
	assert mix64(0) == 0 and model(b"") == 0
	assert mix64(GOLDEN) == 0xE220A8397B1DCDAF                  # splitmix64's finaliser: the generator's first output from seed 0
	assert model(b"\x01") == (mix64(GOLDEN ^ 1) + mix64(1)) & MASK
	assert model(b"ABCDEFGHI") == (mix64(GOLDEN ^ 0x4847464544434241) + mix64((2 * GOLDEN & MASK) ^ 0x49) + mix64(9)) & MASK
	for n in SHORT + [63, 64, 65, 4097]:
		body = row_bytes(n, n)
		assert model_numpy(body) == model(body), n


def test_host_is_the_model():
	import vcf2multialign_amd as v2m
	bodies = [row_bytes(n, 100 + n) for n in SHORT]
	assert v2m.checksum_rows_host(bodies).tolist() == [model(b) for b in bodies]
	bodies = [row_bytes(n, n) for n in AROUND_A_BLOCK + RAGGED]
	assert v2m.checksum_rows_host(bodies).tolist() == [model_numpy(b) for b in bodies]
	bodies = [row_bytes(r % 25, 7000 + r) for r in range(300)]
	assert v2m.checksum_rows_host(bodies).tolist() == [model(b) for b in bodies]
	assert v2m.checksum_rows_host([]).tolist() == []


def test_what_the_sum_tells_apart():
	"""Word order (the index is mixed in), the last byte before the length, the length itself, and a zero byte against the end."""
	import vcf2multialign_amd as v2m
	a = row_bytes(40, 1)
	swapped = a[:8] + a[16:24] + a[8:16] + a[24:]
	last = a[:39] + bytes([a[39] ^ 1])
	rows = [a, swapped, last, a[:39], a[:39] + b"\0", a + b"\0"]
	sums = [model(r) for r in rows]
	assert len(set(sums)) == len(rows)
	assert v2m.checksum_rows_host(rows).tolist() == sums


# ---- device ------------------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
	import vcf2multialign_amd as v2m
	c = v2m.Context(0)
	yield c
	c.close()


def device_sums(ctx, bodies, pitch, per_row):
	"""The rows at `pitch` in a buffer of GUARD bytes; per_row: lengths[] (else one fixed length, which every body must have)."""
	import torch
	host = np.full(len(bodies) * pitch, GUARD, dtype=np.uint8)
	for r, body in enumerate(bodies):
		assert len(body) <= pitch
		host[r * pitch:r * pitch + len(body)] = np.frombuffer(body, dtype=np.uint8)
	buf = torch.from_numpy(host).cuda()
	assert buf.data_ptr() % 8 == 0
	if per_row:
		got = ctx.checksum_rows_device(buf.data_ptr(), pitch, len(bodies), lengths=[len(b) for b in bodies])
	else:
		assert len({len(b) for b in bodies}) == 1
		got = ctx.checksum_rows_device(buf.data_ptr(), pitch, len(bodies), length=len(bodies[0]))
	assert np.array_equal(buf.cpu().numpy(), host), "the rows are read only"
	return got.tolist()


def same_sums(got, want, lengths, what):
	bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
	assert not bad and len(got) == len(want), "%s: %d of %d sums differ, the first at row %d (length %d): got %#x, expected %#x" % (
		what, len(bad), len(want), bad[0], lengths[bad[0]], got[bad[0]], want[bad[0]])


@pytest.mark.gpu
@pytest.mark.parametrize("lengths", [SHORT, AROUND_A_BLOCK, RAGGED], ids=["short", "around_a_block", "ragged"])
def test_device_is_the_model(ctx, lengths):
	"""Per-row lengths in one call (blocks of the grid that lie wholly past a short row's end add nothing), then each length alone in the
	fixed-length form, two rows a call."""
	bodies = [row_bytes(n, 500 + i) for i, n in enumerate(lengths)]
	want = [model_numpy(b) for b in bodies]
	pitch = (max(lengths) + 7) // 8 * 8 + 24
	same_sums(device_sums(ctx, bodies, pitch, True), want, lengths, "per-row lengths")
	for body, w in zip(bodies, want):
		other = row_bytes(len(body), 900 + len(body))
		for p in sorted({(len(body) + 7) // 8 * 8, (len(body) + 7) // 8 * 8 + 8}):          # the row fills its pitch to the word; a word of guard after it
			if p:
				same_sums(device_sums(ctx, [body, other], p, False), [w, model_numpy(other)], [len(body)] * 2, "fixed length %d at pitch %d" % (len(body), p))


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows", [32769, 65537])
def test_device_many_rows(ctx, n_rows):
	"""More rows than one launch takes (32 768): the later launches' rows get their own sums and lengths.  24 bytes at pitch 32, then a
	length of its own per row."""
	rng = np.random.default_rng(n_rows)
	data = rng.integers(1, 256, size=(n_rows, 24), dtype=np.uint8)
	fixed = [data[r].tobytes() for r in range(n_rows)]
	got = device_sums(ctx, fixed, 32, False)
	same_sums(got, [model(b) for b in fixed], [24] * n_rows, "24 bytes a row")
	assert len(set(got)) == n_rows
	ragged = [data[r, :r % 25].tobytes() for r in range(n_rows)]
	same_sums(device_sums(ctx, ragged, 32, True), [model(b) for b in ragged], [r % 25 for r in range(n_rows)], "r % 25 bytes a row")


@pytest.mark.gpu
def test_device_twice_on_one_context(ctx):
	"""The sums are zeroed by every call: the same call twice, and a call of fewer, other rows after it."""
	bodies = [row_bytes(n, 40 + n) for n in (200000, 17, 65536)]
	want = [model_numpy(b) for b in bodies]
	for _ in range(2):
		same_sums(device_sums(ctx, bodies, 200008, True), want, [len(b) for b in bodies], "the same call again")
	same_sums(device_sums(ctx, bodies[1:2], 24, True), want[1:2], [17], "one row after three")


@pytest.mark.gpu
def test_device_tells_apart(ctx):
	a = row_bytes(40, 1)
	swapped = a[:8] + a[16:24] + a[8:16] + a[24:]
	last = a[:39] + bytes([a[39] ^ 1])
	got = device_sums(ctx, [a, swapped, last], 48, False)
	assert got == [model(r) for r in (a, swapped, last)] and len(set(got)) == 3
	# one byte shorter: the byte at position `length` is the guard's, not the row's
	short = device_sums(ctx, [a[:39], last[:39]], 48, False)
	assert short[0] == short[1] == model(a[:39]) and short[0] not in got
