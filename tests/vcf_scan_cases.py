"""Hand-made VCFs that force every branch of the VCF scan rule (include/v2m_hip.h, "VCF scan"), for the host and the GPU tests of the
scan (test infrastructure).  A case knows which of its lines lie outside the rule: the scanner must decline exactly those."""

import numpy as np

REF = np.frombuffer(b"ACGT", np.uint8)[np.random.default_rng(7).integers(0, 4, 4000)].tobytes()
FASTA = b">1\n" + b"\n".join(REF[i:i + 70] for i in range(0, len(REF), 70)) + b"\n"
HEAD = b"##fileformat=VCFv4.2\n##FORMAT=<ID=GT,Number=1,Type=String,Description=\"Genotype\">\n"


def other(base):
	return b"ACGT"[(b"ACGT".index(base) + 1) % 4:][:1]


class Case:
	"""lines: the file's lines; declined: 0-based indices of the lines the rule declines (kind 3); exclude: (sample name, copy) or None."""

	def __init__(self, name, samples, eol=b"\n", final_eol=True):
		self.name, self.samples, self.eol, self.final_eol = name, samples, eol, final_eol
		self.lines = HEAD.split(b"\n")[:-1] + [b"#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT" + b"".join(b"\t" + s.encode() for s in samples)]
		self.declined = set()
		self.exclude = None
		self.pos = 10

	def raw(self, line, declined=False):
		if declined:
			self.declined.add(len(self.lines))
		self.lines.append(line)

	def rec(self, gts, alts=None, fmt=b"GT", chrom=b"1", declined=False, ref_len=1, step=7):
		"""A record at the next position; gts: one field per sample (bytes); alts: list of ALT strings (default: one SNV)."""
		self.pos += step + ref_len
		ref = REF[self.pos - 1:self.pos - 1 + ref_len]
		if alts is None:
			alts = [other(ref[:1])]
		elif callable(alts):
			alts = alts(ref)
		line = b"\t".join([chrom, b"%d" % self.pos, b"v%d" % len(self.lines), ref, b",".join(alts), b".", b"PASS", b".", fmt] + list(gts))
		self.raw(line, declined or (self.eol == b"\r\n" and chrom == b"1"))

	@property
	def vcf(self):
		return self.eol.join(self.lines) + (self.eol if self.final_eol else b"")

	def write(self, d):
		fa, vcf = d / (self.name + ".fa"), d / (self.name + ".vcf")
		fa.write_bytes(FASTA)
		vcf.write_bytes(self.vcf)
		return str(fa), str(vcf)

	def kwargs(self):
		return dict(exclude_sample=self.exclude[0], exclude_copy=self.exclude[1]) if self.exclude else {}

	def excluded_pairs(self):
		return {(self.samples.index(self.exclude[0]), self.exclude[1])} if self.exclude else set()


def distinct_alts(n):
	"""n distinct sequence ALTs, none equal to a single reference base."""
	return [b"AC" + b"".join(b"ACGT"[(k >> (2 * i)) & 3:][:1] for i in range(4)) for k in range(n)]


def cases():
	out = []
	S3 = ["S0", "S1", "S2"]

	c = Case("gt_not_first", S3)                     # FORMAT DP:GT: condition b fails, the host parses the line
	c.rec([b"0|1", b"1|0", b"0|0"])
	c.rec([b"3:0|1", b"4:1|1", b"5:0|0"], fmt=b"DP:GT", declined=True)
	c.rec([b"1|1", b"0|0", b"0|1"])
	out.append(c)

	c = Case("gt_dp", S3)                            # GT:DP sample fields
	c.rec([b"0|1:3", b"1|0:14", b"0|0:5"], fmt=b"GT:DP")
	c.rec([b"1|1:3:x", b"0|0", b"0|1:."], fmt=b"GT:DP:XX")
	out.append(c)

	c = Case("slash_and_dots", S3)                   # '/' separators, '.' alleles
	c.rec([b"0/1", b"1/0", b"./."])
	c.rec([b".|1", b"1|.", b"0/0"])
	out.append(c)

	c = Case("mixed_ploidy", ["H", "D", "T", "D2"])  # haploid, diploid and triploid samples
	c.rec([b"1", b"0|1", b"0|1|1", b"1|0"])
	c.rec([b"0", b"1|1", b"1|0|0", b"0|0"], alts=[b"AAC", b"<DEL>"], ref_len=2)
	c.rec([b"2", b"2|1", b"0|2|1", b"1|2"], alts=lambda ref: [other(ref), other(ref) + b"T"])
	c.rec([b".", b".|1", b"0|.|1", b"./."])
	c.rec([b"1|0", b"0|1|1", b"0|1|1|1", b"1|0|1"])  # wider than the first record's: the extra tokens are not looked at
	out.append(c)

	c = Case("excluded_copy", S3)
	c.exclude = ("S1", 1)
	c.rec([b"0|1", b"1|1", b"1|0"])
	c.rec([b"1|1", b"0|1", b"0|1"])
	c.rec([b"1|0", b"1|x", b"0|1"], declined=True)   # stricter than the text parser for an excluded copy: declined, then parsed by it
	out.append(c)

	c = Case("nine_alts", S3)
	c.rec([b"8|1", b"0|7", b"2|3"], alts=distinct_alts(8))
	c.rec([b"9|1", b"0|7", b"2|3"], alts=distinct_alts(9), declined=True)
	c.rec([b"08|1", b"0|007", b"2|3"], alts=distinct_alts(8))
	c.rec([b"0008|1", b"0|7", b"2|3"], alts=distinct_alts(8), declined=True)   # four digits
	out.append(c)

	c = Case("hundred_alts", S3)
	c.rec([b"10|100", b"0|101", b"2|3"], alts=distinct_alts(101), declined=True)
	c.rec([b"1|0", b"0|1", b"1|1"])
	out.append(c)

	c = Case("odd_alts", S3)                         # what the ALT entries are stays the host's business
	c.rec([b"1|2", b"3|4", b"0|1"], alts=[b"<DEL>", b"<CNV:X>", b"*", b"TT"], ref_len=3)
	c.rec([b"1|2", b"3|0", b"2|2"], alts=lambda ref: [other(ref), b"", b"."])
	out.append(c)

	c = Case("two_chromosomes", S3)
	for k in range(12):
		c.rec([b"0|1", b"1|0", b"1|1"], chrom=b"2" if k % 3 == 1 else b"1")
	c.rec([b"0|1", b"1|0"], chrom=b"2")            # too few columns on another chromosome: kind 1, never looked at
	c.rec([b"0|1", b"1|0", b"1|1"])
	out.append(c)

	c = Case("hash_and_blank_lines", S3)
	c.rec([b"0|1", b"1|0", b"1|1"])
	c.raw(b"")
	c.raw(b"# a comment inside the body")
	c.rec([b"1|1", b"0|0", b"0|1"])
	c.raw(b"#CHROM\tlate")
	c.raw(b"")
	c.rec([b"1|0", b"0|1", b"0|1"])
	out.append(c)

	c = Case("crlf", S3, eol=b"\r\n")                # condition a: every record declined; the text parser strips the '\r'
	c.rec([b"0|1", b"1|0", b"1|1"])
	c.rec([b"0|1", b"1|0", b"1|1"], chrom=b"2")
	c.rec([b"1|1", b"0|0", b"0|1"])
	out.append(c)

	c = Case("no_final_newline", S3, final_eol=False)
	c.rec([b"0|1", b"1|0", b"1|1"])
	c.rec([b"1|1", b"0|0", b"0|1"])
	out.append(c)

	c = Case("late_first_record", S3)                # the layout line comes after 300 lines of another chromosome
	for k in range(300):
		c.rec([b"0|1", b"1|0", b"1|1"], chrom=b"2", step=1)
	for k in range(5):
		c.rec([b"0|1", b"1|%d" % (k & 1), b"1|1"])
	out.append(c)

	c = Case("no_record", S3)
	for k in range(6):
		c.rec([b"0|1", b"1|0", b"1|1"], chrom=b"2")
	out.append(c)
	return out


def padded_case(pads, n_samples=40, sep=b"|"):
	"""Lines of a few KB whose first sample field is padded by `pad` bytes (GT:DP) for every pad of `pads`, so that over a sweep of one
	step length a two-digit allele, a separator and a tab each fall on the last and on the first byte of a step of the genotype pass."""
	c = Case("padded", ["S%d" % i for i in range(n_samples)])
	alts = distinct_alts(8)
	for pad in pads:
		for r in range(2):
			gts = [b"0" + sep + b"0:" + b"9" * pad]
			for s in range(1, n_samples):
				a, b = (s * 7 + r + pad) % 9, (s * 5 + 2 * r) % 9
				gts.append((b"0%d" % a if s % 3 == 0 else b"%d" % a) + sep + b"%d" % b + b":" + b"1" * (s % 5 + 60))
			c.rec(gts, alts=alts, fmt=b"GT:DP", step=1)
	return c


def copies_case(n_copies):
	"""n_copies chromosome copies: diploid samples and, for an odd count, one haploid sample."""
	n_dip, hap = n_copies // 2, n_copies % 2
	c = Case("copies_%d" % n_copies, ["S%d" % i for i in range(n_dip + hap)])
	for r in range(3):
		gts = [b"%d|%d" % ((s + r) % 3 == 0, (s * 3 + r) % 4 == 0) for s in range(n_dip)] + ([b"1"] if hap else [])
		if r == 2 and gts:
			gts[-1] = b"1" if hap else b"1|1"        # the last row's bit
		c.rec(gts)
	return c


def damaged(lines, k, how):
	f = lines[k].split(b"\t")
	if how == "empty GT allele":
		f[12] = f[12][:-1]                                                # "0|"
	elif how == "bad GT allele":
		f[12] = f[12][:-1] + b"x"
	elif how == "GT allele exceeds the ALT count":
		f[12] = f[12][:-1] + b"9"
	elif how == "sample column count differs from the header":
		f = f[:-1]
	elif how == "more sample columns than in the header":
		f.append(f[-1])
	elif how == "fewer than 8 columns":
		f = f[:5]
	elif how == "POS must be 1-based":
		f[1] = b"0"
	elif how == "GT has fewer alleles than in the first record":
		f[12] = f[12].split(b"|")[0]
	lines[k] = b"\t".join(f)


ERRORS = ["empty GT allele", "bad GT allele", "GT allele exceeds the ALT count", "sample column count differs from the header", "more sample columns than in the header",
	"fewer than 8 columns", "POS must be 1-based", "GT has fewer alleles than in the first record"]
