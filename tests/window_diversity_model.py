"""The model of the window diversity (include/v2m_hip.h, "window diversity"): numpy over a counts table, a brute force over the rows that
enumerates every pair of rows per column, the doubles with np.float64 scalars in the header's order, the three texts, and the corpus
of hand-made tables tests/test_gpu_window_diversity.py runs, with the census of the seams its items reach.

from_counts() and between_from_counts() restate the header's expressions on the four letter planes; brute_within() and
brute_between() never form a count: they compare the letters of two rows.  tests/test_window_diversity_host.py holds the two to each
other and to the host library's plain loops."""

import functools
import itertools
import os
import re

import numpy as np

import column_counts_model as CM
import pair_distances_model as PM

ROOT = PM.ROOT
DIVERSITY_KERNELS_HPP = os.path.join(ROOT, "vcf2multialign_amd", "csrc", "diversity_kernels.hpp")
BIN_DTYPE = np.dtype([(name, "<u8") for name in ("columns", "called", "diffs", "pairs", "segregating", "complete", "complete_segregating", "complete_diffs")])
BETWEEN_DTYPE = np.dtype([(name, "<u8") for name in ("columns", "called", "diffs", "pairs")])
MAX_ROWS = 32768


@functools.lru_cache(maxsize=None)
def kernel_constants():
	"""(T, H): kDiversityColumns, the columns of a workgroup's tile, and kDiversitySfsLdsBins, the entries of the on-chip histogram, read
	from csrc/diversity_kernels.hpp."""
	with open(DIVERSITY_KERNELS_HPP) as f:
		text = f.read()
	out = []
	for name in ("kDiversityColumns", "kDiversitySfsLdsBins"):
		found = re.findall(r"^constexpr\s+int\s+%s\s*=\s*(\d+)\s*;" % name, text, re.M)
		assert len(found) == 1, "%s: %d definitions of the form `constexpr int %s = value;`" % (name, len(found), name)
		out.append(int(found[0]))
	return tuple(out)


# ---- from a counts table ---------------------------------------------------------------------------------------------------------------------

def letters_of(m):
	"""object-free u64[4, L]: the rows of m[n, L] that hold A, C, G, T (either case) per column -- planes 0-3 of the counts table."""
	return np.ascontiguousarray(CM.counts(np.asarray(m, dtype=np.uint8))[:, :4].T).astype(np.uint64)


def per_column(c, n):
	"""The header's per-column values of planes c[4, L] counted over n rows, all u64 / bool arrays of L."""
	a, cc, g, t = (c[k].astype(np.uint64) for k in range(4))
	m = a + cc + g + t
	diffs = a * cc + a * g + a * t + cc * g + cc * t + g * t
	pairs = m * (m - np.minimum(m, 1)) // 2
	letters = (a > 0).astype(np.int64) + (cc > 0) + (g > 0) + (t > 0)
	return dict(m=m, diffs=diffs, pairs=pairs, called=m >= 2, segregating=letters >= 2, complete=(m == n) & (n >= 2), letters=letters)


def _sum(x, lo, hi):
	return int(np.asarray(x[lo:hi], dtype=np.uint64).sum(dtype=np.uint64))


def from_counts(c, n, bounds):
	"""v2m_diversity_bin records of planes c[4, L] over the bins of bounds."""
	v = per_column(c, n)
	out = np.zeros(len(bounds) - 1, dtype=BIN_DTYPE)
	for k in range(len(out)):
		lo, hi = int(bounds[k]), int(bounds[k + 1])
		done = v["complete"]
		out[k] = (hi - lo, _sum(v["called"], lo, hi), _sum(v["diffs"], lo, hi), _sum(v["pairs"], lo, hi), _sum(v["segregating"], lo, hi), _sum(done, lo, hi),
			_sum(done & v["segregating"], lo, hi), _sum(v["diffs"] * done, lo, hi))
	return out


def between_from_counts(ca, cb, bounds):
	"""v2m_diversity_between_bin records of two tables' planes."""
	ca, cb = ca.astype(np.uint64), cb.astype(np.uint64)
	ma, mb = ca.sum(axis=0, dtype=np.uint64), cb.sum(axis=0, dtype=np.uint64)
	pairs = ma * mb
	diffs = pairs - (ca * cb).sum(axis=0, dtype=np.uint64)
	called = (ma >= 1) & (mb >= 1)
	out = np.zeros(len(bounds) - 1, dtype=BETWEEN_DTYPE)
	for k in range(len(out)):
		lo, hi = int(bounds[k]), int(bounds[k + 1])
		out[k] = (hi - lo, _sum(called, lo, hi), _sum(diffs, lo, hi), _sum(pairs, lo, hi))
	return out


def sfs_from_counts(c, n, lo, hi):
	"""(sfs u64[n // 2 + 1], multiallelic) over the columns [lo, hi)."""
	v = per_column(c, n)
	sfs = np.zeros(n // 2 + 1, dtype=np.uint64)
	many = 0
	for i in range(int(lo), int(hi)):
		if not v["complete"][i]:
			continue
		if v["letters"][i] >= 3:
			many += 1
		elif v["letters"][i] == 2:
			sfs[min(int(x) for x in c[:, i] if x)] += np.uint64(1)
		else:
			sfs[0] += np.uint64(1)
	return sfs, many


# ---- brute force from rows -------------------------------------------------------------------------------------------------------------------

def _letter(b):
	return "acgt".find(chr(b | 0x20)) if (b | 0x20) < 128 else -1


def brute_within(m, bounds, want_sfs=True):
	"""(bins, sfs, multiallelic) of the alignment m[n, L]: every pair of rows of every column is looked at."""
	m = np.asarray(m, dtype=np.uint8)
	n = m.shape[0]
	out = np.zeros(len(bounds) - 1, dtype=BIN_DTYPE)
	sfs, many = np.zeros(n // 2 + 1, dtype=np.uint64), 0
	for k in range(len(out)):
		rec = dict.fromkeys(BIN_DTYPE.names, 0)
		rec["columns"] = int(bounds[k + 1]) - int(bounds[k])
		for col in range(int(bounds[k]), int(bounds[k + 1])):
			letters = [_letter(int(b)) for b in m[:, col]]
			pairs = diffs = 0
			for i, j in itertools.combinations(range(n), 2):
				if letters[i] >= 0 and letters[j] >= 0:
					pairs += 1
					diffs += letters[i] != letters[j]
			held = [x for x in letters if x >= 0]
			kinds = sorted((held.count(x) for x in set(held)), reverse=True)
			complete = len(held) == n and n >= 2
			rec["called"] += len(held) >= 2
			rec["diffs"] += diffs
			rec["pairs"] += pairs
			rec["segregating"] += len(kinds) >= 2
			rec["complete"] += complete
			rec["complete_segregating"] += complete and len(kinds) >= 2
			rec["complete_diffs"] += diffs if complete else 0
			if complete and len(kinds) >= 3:
				many += 1
			elif complete:
				sfs[kinds[1] if len(kinds) == 2 else 0] += np.uint64(1)
		out[k] = tuple(rec[name] for name in BIN_DTYPE.names)
	return (out, sfs, many) if want_sfs else (out, None, 0)


def brute_between(ma, mb, bounds):
	ma, mb = np.asarray(ma, dtype=np.uint8), np.asarray(mb, dtype=np.uint8)
	out = np.zeros(len(bounds) - 1, dtype=BETWEEN_DTYPE)
	for k in range(len(out)):
		called = diffs = pairs = 0
		for col in range(int(bounds[k]), int(bounds[k + 1])):
			la, lb = [_letter(int(b)) for b in ma[:, col]], [_letter(int(b)) for b in mb[:, col]]
			here = 0
			for x in la:
				for y in lb:
					if x >= 0 and y >= 0:
						here += 1
						diffs += x != y
			pairs += here
			called += any(x >= 0 for x in la) and any(y >= 0 for y in lb)
		out[k] = (int(bounds[k + 1]) - int(bounds[k]), called, diffs, pairs)
	return out


# ---- the doubles -----------------------------------------------------------------------------------------------------------------------------

F = np.float64
NONE = F("nan")


@functools.lru_cache(maxsize=None)
def harmonics(n):
	a1, a2 = F(0), F(0)
	for i in range(1, n):
		d = F(i)
		a1 = a1 + F(1) / d
		a2 = a2 + F(1) / (d * d)
	return a1, a2


def values(rec, n):
	"""(pi, theta_w, tajima_d) of a window's record over n sequences, in the header's order of operations; NaN where none exists."""
	pi = theta = tajima = NONE
	if int(rec["pairs"]):
		pi = F(int(rec["diffs"])) / F(int(rec["pairs"]))
	if n < 2:
		return pi, theta, tajima
	a1, a2 = harmonics(n)
	d, S = F(n), F(int(rec["complete_segregating"]))
	theta = S / a1
	b1 = (d + F(1)) / (F(3) * (d - F(1)))
	b2 = (F(2) * ((d * d + d) + F(3))) / ((F(9) * d) * (d - F(1)))
	c1 = b1 - F(1) / a1
	c2 = (b2 - (d + F(2)) / (a1 * d)) + a2 / (a1 * a1)
	e1 = c1 / a1
	e2 = c2 / (a1 * a1 + a2)
	k = F(int(rec["complete_diffs"])) / ((d * (d - F(1))) / F(2))
	v = e1 * S + (e2 * S) * (S - F(1))
	if v > 0:
		tajima = (k - theta) / np.sqrt(v)
	return pi, theta, tajima


def tajima_of(n, S, k):
	"""The worked check: D from S segregating sites and a mean pairwise difference k given as a double."""
	a1, a2 = harmonics(n)
	d, S = F(n), F(S)
	b1 = (d + F(1)) / (F(3) * (d - F(1)))
	b2 = (F(2) * ((d * d + d) + F(3))) / ((F(9) * d) * (d - F(1)))
	c1 = b1 - F(1) / a1
	c2 = (b2 - (d + F(2)) / (a1 * d)) + a2 / (a1 * a1)
	e1, e2 = c1 / a1, c2 / (a1 * a1 + a2)
	return (F(k) - S / a1) / np.sqrt(e1 * S + (e2 * S) * (S - F(1)))


def divergence_values(between, rec_a, rec_b):
	dxy = fst = NONE
	if not int(between["pairs"]):
		return dxy, fst
	dxy = F(int(between["diffs"])) / F(int(between["pairs"]))
	if int(rec_a["pairs"]) and int(rec_b["pairs"]) and dxy > 0:
		pa = F(int(rec_a["diffs"])) / F(int(rec_a["pairs"]))
		pb = F(int(rec_b["diffs"])) / F(int(rec_b["pairs"]))
		fst = F(1) - (pa + pb) / (F(2) * dxy)
	return dxy, fst


def values_array(recs, n):
	return np.array([values(r, n) for r in recs], dtype=np.float64).reshape(len(recs), 3)


def divergence_array(between, recs_a, recs_b):
	return np.array([divergence_values(*x) for x in zip(between, recs_a, recs_b)], dtype=np.float64).reshape(len(between), 2)


def summed(bins, width):
	"""Windows of `width` consecutive bins, field by field as integers (the last one may be short)."""
	out = np.zeros(-(-len(bins) // width), dtype=bins.dtype)
	for name in bins.dtype.names:
		for w in range(len(out)):
			out[name][w] = bins[name][w * width:(w + 1) * width].sum(dtype=np.uint64)
	return out


# ---- the texts -------------------------------------------------------------------------------------------------------------------------------

def _double(x):
	return "NA" if x != x else "%.10g" % x


DIVERSITY_HEADER = "#group\tstart\tend\tcolumns\tcalled\tdiffs\tpairs\tpi\tsegregating\tcomplete\ttheta_w\ttajima_d\n"
DIVERGENCE_HEADER = "#group_a\tgroup_b\tstart\tend\tcolumns\tcalled\tdiffs\tpairs\tdxy\tfst\n"
SFS_HEADER = "#group\tn\tminor_count\tcolumns\n"


def diversity_text(group, n, windows, starts, ends, header=False):
	lines = [DIVERSITY_HEADER] if header else []
	for w, s, e in zip(windows, starts, ends):
		pi, theta, tajima = values(w, n)
		lines.append("\t".join([group] + [str(int(x)) for x in (s, e, w["columns"], w["called"], w["diffs"], w["pairs"])] + [_double(pi)]
			+ [str(int(w["segregating"])), str(int(w["complete"])), _double(theta), _double(tajima)]) + "\n")
	return "".join(lines).encode()


def divergence_text(group_a, group_b, between, windows_a, windows_b, starts, ends, header=False):
	lines = [DIVERGENCE_HEADER] if header else []
	for w, wa, wb, s, e in zip(between, windows_a, windows_b, starts, ends):
		dxy, fst = divergence_values(w, wa, wb)
		lines.append("\t".join([group_a, group_b] + [str(int(x)) for x in (s, e, w["columns"], w["called"], w["diffs"], w["pairs"])] + [_double(dxy), _double(fst)]) + "\n")
	return "".join(lines).encode()


def sfs_text(group, n, sfs, multiallelic, header=False):
	lines = [SFS_HEADER] if header else []
	lines += ["%s\t%d\t%d\t%d\n" % (group, n, k, int(x)) for k, x in enumerate(sfs)]
	lines.append("%s\t%d\tmultiallelic\t%d\n" % (group, n, multiallelic))
	return "".join(lines).encode()


# ---- small random alignments -----------------------------------------------------------------------------------------------------------------

ALPHABET = np.frombuffer(b"AACCGGTTacgtN-nR" + bytes([0, 0xC1, 0xE1, 0x0D]), dtype=np.uint8)


def random_alignment(n, L, seed):
	"""u8[n, L] of letters of both cases, N, '-' and other bytes; some columns are made complete, of one to four letters."""
	rng = np.random.default_rng(seed)
	m = ALPHABET[rng.integers(0, len(ALPHABET), size=(n, L))].copy()
	for col in range(0, L, 3):
		kinds = 1 + (col // 3) % 4
		m[:, col] = np.frombuffer(b"ACGTacgt", dtype=np.uint8)[rng.integers(0, kinds, size=n) + 4 * rng.integers(0, 2, size=n)]
	return m


def random_bounds(L, n_bins, seed):
	rng = np.random.default_rng(seed)
	return np.sort(rng.integers(0, L + 1, size=n_bins + 1)).astype(np.uint64)


# ---- the corpus of hand-made tables ----------------------------------------------------------------------------------------------------------

class Item:
	"""A counts table (and a second one: the between form) with the bins to reduce it over.  planes: u32[4, L]."""

	def __init__(self, name, n, planes, bounds, n_b=0, planes_b=None, sfs=True):
		self.name, self.n, self.planes, self.bounds = name, n, planes, np.asarray(bounds, dtype=np.uint64)
		self.n_b, self.planes_b, self.sfs = n_b, planes_b, sfs and planes_b is None
		self.L = planes.shape[1]

	def __repr__(self):
		return self.name


def random_planes(n, L, seed, hostile_outside=None):
	"""u32[4, L]: columns of every kind in turn -- m = 0, m = 1, incomplete, complete of one, two (one of them split n / 2 : n - n / 2),
	three and four letters.  hostile_outside = (lo, hi): the columns outside get counts no table could hold."""
	rng = np.random.default_rng(seed)
	p = np.zeros((4, L), dtype=np.uint32)
	for i in range(L):
		kind = int(rng.integers(0, 8))
		order = rng.permutation(4)
		if kind == 0 or n == 0:
			continue
		if kind == 1:
			p[order[0], i] = 1
		elif kind == 2:   # incomplete
			left = int(rng.integers(0, n))
			for k in order[:3]:
				x = int(rng.integers(0, left + 1))
				p[k, i], left = x, left - x
		elif kind == 3:
			p[order[0], i] = n
		elif kind == 4 or n < 3:
			x = n // 2 if i % 2 else int(rng.integers(1, max(2, n // 2 + 1))) if n >= 2 else 0
			p[order[0], i], p[order[1], i] = x, n - x
		elif kind == 5 or n < 4:
			x, y = 1 + int(rng.integers(0, n - 2)), 1
			x = min(x, n - 2)
			p[order[0], i], p[order[1], i], p[order[2], i] = x, y, n - x - y
		else:
			cuts = np.sort(rng.choice(np.arange(1, n), size=3, replace=False))
			parts = np.diff(np.concatenate([[0], cuts, [n]]))
			p[order, i] = parts
	if hostile_outside is not None:
		lo, hi = hostile_outside
		mask = np.ones(L, dtype=bool)
		mask[lo:hi] = False
		p[:, mask] = rng.integers(0x7FFF0000, 0xFFFFFFFF, size=(4, int(mask.sum())), dtype=np.uint64).astype(np.uint32)
	return p


@functools.lru_cache(maxsize=None)
def corpus():
	T, H = kernel_constants()
	items = []
	add = lambda *a, **k: items.append(Item(*a, **k))
	# the lengths, one bin over everything and a bin a column
	for L in (1, 3, 4, 5, T - 1, T, T + 1, 2 * T + 5):
		add("one_bin_L%d" % L, 7, random_planes(7, L, L), [0, L])
	L = 2 * T + 5
	add("bin_a_column", 6, random_planes(6, L, 11), np.arange(L + 1))
	add("bins_of_7", 9, random_planes(9, L, 12), sorted(set(list(range(0, L, 7)) + [L])))
	# one-column bins at each of a lane's four positions; ends at a lane, a wave and a tile seam; empty bins at 0, L and the seams
	add("lane_positions", 5, random_planes(5, T + 9, 13, (4, T + 6)), [4, 5, 6, 7, 8, 12, 256, 300, T, T + 1, T + 6])
	add("seams", 8, random_planes(8, 2 * T + 5, 14), [0, 0, 4, 4, 8, 256, 256, 512, 513, T, T, T + 3, 2 * T, 2 * T, 2 * T + 5, 2 * T + 5])
	add("empty_run", 5, random_planes(5, 40, 15), [0, 17] + [18] * 301 + [40])
	add("three_tiles", 11, random_planes(11, 3 * T + 70, 16, (50, 3 * T + 60)), [50, 3 * T + 60])
	add("inside", 4, random_planes(4, 2 * T, 17, (T - 30, T + 30)), [T - 30, T - 1, T + 2, T + 30])
	# sums that pass 2^32: the carries across lanes and waves
	p = np.zeros((4, 64), dtype=np.uint32)
	p[0], p[1] = MAX_ROWS // 2, MAX_ROWS // 2
	add("carries", MAX_ROWS, p, [0, 64])
	add("carries_split", MAX_ROWS, np.tile(p, (1, 8)), [0, 3, 259, 512])
	# the spectrum: the smallest groups, the histogram's limit, the largest group
	for n in (2, 3, 2 * (H - 1) - 2, 2 * H - 2, 2 * H, MAX_ROWS):
		add("sfs_n%d" % n, n, random_planes(n, 70, n), [3, 30, 66])
	add("no_sfs", 6, random_planes(6, 33, 18), [0, 10, 33], sfs=False)
	# between
	add("between", 5, random_planes(5, T + 9, 19), [0, 1, 5, 300, T + 9], n_b=8, planes_b=random_planes(8, T + 9, 20))
	add("between_inside", 3, random_planes(3, 2 * T + 5, 21, (7, 2 * T)), [7, 7, T + 1, 2 * T], n_b=2, planes_b=random_planes(2, 2 * T + 5, 22, (7, 2 * T)))
	pa, pb = np.zeros((4, 64), dtype=np.uint32), np.zeros((4, 64), dtype=np.uint32)
	pa[0], pb[1] = MAX_ROWS, MAX_ROWS
	add("between_carries", MAX_ROWS, pa, [0, 64], n_b=MAX_ROWS, planes_b=pb)
	names = [i.name for i in items]
	assert len(set(names)) == len(names)
	return items


def table(planes, seed=5):
	"""(u32[6, pitch], pitch) around planes[4, L]: 0 in elements L ..< (L + 3) & ~3 of planes 0-3, hostile values in everything beyond
	and in all of planes 4 and 5."""
	L = planes.shape[1]
	pad = (L + 3) & ~3
	pitch = pad + 4 * (1 + L % 3)
	rng = np.random.default_rng(seed + L)
	t = rng.integers(0x7FFF0000, 0xFFFFFFFF, size=(6, pitch), dtype=np.uint64).astype(np.uint32)
	t[:4, :pad] = 0
	t[:4, :L] = planes
	return t, pitch


@functools.lru_cache(maxsize=None)
def expected(name):
	"""(bins, sfs or None, multiallelic) of an item of corpus(): computed once, shared, read-only."""
	item = next(i for i in corpus() if i.name == name)
	if item.planes_b is not None:
		out = (between_from_counts(item.planes, item.planes_b, item.bounds), None, 0)
	else:
		sfs, many = sfs_from_counts(item.planes, item.n, item.bounds[0], item.bounds[-1]) if item.sfs else (None, 0)
		out = (from_counts(item.planes, item.n, item.bounds), sfs, many)
	for a in out[:2]:
		if a is not None:
			a.setflags(write=False)
	return out


SEAMS = ("L=1", "L=3", "L=4", "L=5", "L=T-1", "L=T", "L=T+1", "L=2T+5", "one-column bin at lane position 0", "one-column bin at lane position 1",
	"one-column bin at lane position 2", "one-column bin at lane position 3", "bin end at a lane seam", "bin end at a wave seam", "bin end at T", "bin end at 2T",
	"empty bin at 0", "empty bin at L", "empty bin at a lane seam", "empty bin at a wave seam", "empty bin at a tile seam", "300 empty bins in a row", "one bin over three tiles",
	"n_bins=1", "n_bins=L at 2T+5", "bounds[0]>0", "bounds[n_bins]<L", "a sum beyond 2^32", "m=0", "m=1", "sfs n=2", "sfs n=3", "sfs entries H-1", "sfs entries H",
	"sfs entries H+1", "sfs n=32768", "minor count n/2", "complete column", "incomplete column", "three letters", "four letters", "between n_a!=n_b", "between m=0 in one group",
	"no spectrum")


def census(item):
	"""The seams of SEAMS the item reaches, from its geometry and its counts."""
	T, H = kernel_constants()
	L, b, n = item.L, [int(x) for x in item.bounds], item.n
	got = set()
	for name, value in (("1", 1), ("3", 3), ("4", 4), ("5", 5), ("T-1", T - 1), ("T", T), ("T+1", T + 1), ("2T+5", 2 * T + 5)):
		if L == value:
			got.add("L=" + name)
	for lo, hi in zip(b, b[1:]):
		if hi - lo == 1:
			got.add("one-column bin at lane position %d" % (lo % 4))
		if hi == lo:
			got.update(s for s, ok in (("empty bin at 0", lo == 0), ("empty bin at L", lo == L), ("empty bin at a lane seam", lo % 4 == 0 and 0 < lo < L and lo % 256),
				("empty bin at a wave seam", lo % 256 == 0 and 0 < lo and lo % T), ("empty bin at a tile seam", lo % T == 0 and 0 < lo < L)) if ok)
		if hi > lo:
			got.update(s for s, ok in (("bin end at a lane seam", hi % 4 == 0 and hi % 256), ("bin end at a wave seam", hi % 256 == 0 and hi % T), ("bin end at T", hi == T),
				("bin end at 2T", hi == 2 * T), ("one bin over three tiles", hi // T - lo // T >= 2 and hi - lo > 2 * T)) if ok)
	run = longest = 0
	for lo, hi in zip(b, b[1:]):
		run = run + 1 if hi == lo else 0
		longest = max(longest, run)
	inside = slice(b[0], b[-1])
	p = item.planes[:, inside].astype(np.uint64)
	m = p.sum(axis=0)
	letters = (p > 0).sum(axis=0)
	complete = (m == n) & (n >= 2)
	flags = {"300 empty bins in a row": longest >= 300, "n_bins=1": len(b) == 2, "n_bins=L at 2T+5": len(b) - 1 == L == 2 * T + 5, "bounds[0]>0": b[0] > 0, "bounds[n_bins]<L": b[-1] < L,
		"m=0": bool((m == 0).any()), "m=1": bool((m == 1).any())}
	if item.planes_b is None:
		flags["a sum beyond 2^32"] = int(per_column(item.planes, n)["diffs"][inside].sum(dtype=np.uint64)) >= 1 << 32
		flags["no spectrum"] = not item.sfs
	if item.sfs:
		entries = n // 2 + 1
		flags.update({"sfs n=2": n == 2, "sfs n=3": n == 3, "sfs entries H-1": entries == H - 1, "sfs entries H": entries == H, "sfs entries H+1": entries == H + 1,
			"sfs n=32768": n == MAX_ROWS, "minor count n/2": bool(((letters == 2) & complete & (p.max(axis=0) * 2 == n)).any()), "complete column": bool(complete.any()),
			"incomplete column": bool((~complete).any()), "three letters": bool((complete & (letters == 3)).any()), "four letters": bool((complete & (letters == 4)).any())})
	if item.planes_b is not None:
		mb = item.planes_b[:, inside].astype(np.uint64).sum(axis=0)
		flags.update({"between n_a!=n_b": item.n != item.n_b, "between m=0 in one group": bool(((m == 0) != (mb == 0)).any())})
	got.update(s for s, ok in flags.items() if ok)
	return got


# ---- what the driver writes --------------------------------------------------------------------------------------------------------------

def driver_texts(g, ids, rows, window, step=None, groups=None, region=None):
	"""(diversity, sfs, divergence or None): the bytes of --output-diversity, --diversity-sfs and --output-divergence for the rows named
	`ids` of the oracle's graph g, from the oracle's rows.  region: the 0-based half-open reference range, None for all of it; groups:
	(id, group) pairs, None for the one group `all`.  Bins are a step wide and begin at the column of their first reference position;
	window j is the bins [j, j + window / step) summed, for every j with a whole window (one short window where there is none)."""
	from vcf2multialign_amd.variant_graph import columns_of_reference_range as columns
	step = window if step is None else step
	assert window % step == 0
	ref, aln = g.reference_positions, g.aligned_positions
	s, e = region if region is not None else (0, int(ref[-1]))
	n_bins, width = -(-(e - s) // step), window // step
	bounds = np.array([columns(ref, aln, s + k * step, e)[0] for k in range(n_bins)] + [columns(ref, aln, s, e)[1]], dtype=np.uint64)
	n_windows = n_bins - width + 1 if n_bins >= width else 1
	starts = [s + j * step + 1 for j in range(n_windows)]
	ends = [min(e, s + j * step + window) for j in range(n_windows)]
	sliding = lambda bins: np.array([tuple(int(bins[name][j:j + width].sum(dtype=np.uint64)) for name in bins.dtype.names) for j in range(n_windows)], dtype=bins.dtype)
	if groups is None:
		names, members = ["all"], [list(range(len(rows)))]
	else:
		names, members = [], []
		for i, group in groups:
			if group not in names:
				names.append(group)
				members.append([])
			members[names.index(group)].append(ids.index(i))
		members = [sorted(m) for m in members]
	m = CM.matrix(g, rows)
	planes = [letters_of(m[mem]) for mem in members]
	within = [from_counts(p, len(mem), bounds) for p, mem in zip(planes, members)]
	windows = [sliding(b) for b in within]
	diversity = b"".join(diversity_text(names[k], len(members[k]), windows[k], starts, ends, header=k == 0) for k in range(len(names)))
	spectra = b""
	for k in range(len(names)):
		sfs, many = sfs_from_counts(planes[k], len(members[k]), bounds[0], bounds[-1])
		spectra += sfs_text(names[k], len(members[k]), sfs, many, header=k == 0)
	divergence, first = None, True
	if groups is not None and len(names) >= 2:
		divergence = b""
		for a in range(len(names)):
			for b in range(a + 1, len(names)):
				divergence += divergence_text(names[a], names[b], sliding(between_from_counts(planes[a], planes[b], bounds)), windows[a], windows[b], starts, ends, header=first)
				first = False
	return diversity, spectra, divergence
