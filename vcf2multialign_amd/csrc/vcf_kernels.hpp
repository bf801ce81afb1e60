// vcf_kernels.hpp -- the VCF scan of include/v2m_hip.h ("VCF scan"): the text of a slice, already in device memory (inflated there by
// bgzf_inflate_kernel, or copied from the caller's plain text), becomes line records, a pool of record heads and bit columns in the
// layout of paths_by_edge_and_chrom_copy.  gfx950, wave64.
//
// The passes of a slice (launched by v2m_vcf_scan in v2m_hip.hip, all on the context's stream):
//   vcf_count_newlines_kernel   '\n' per 4-KiB tile, 16 bytes per thread
//   vcf_scan_u32_kernel         the tiles' counts -> offsets and the total (one workgroup)
//   vcf_line_starts_kernel      line_start[k + 1] = the byte after the k-th '\n'
//   vcf_head_kernel             one wave per line: the first nine tabs, CHROM against the wanted one, the commas of ALT, GT / GT: ->
//                               the line's kind before its genotypes are looked at (2 = a candidate)
//   vcf_alloc_scan_kernel       exclusive sums over the lines, in line order: the candidates' columns (a pool of their own, since a
//                               candidate may still be declined), then the heads and the columns of what the genotype pass accepted.
//                               Allocation is a scan, never an atomic: the chunk's layout depends on the text alone.
//   vcf_genotype_kernel         one wave per candidate: conditions d and e of the rule and the bit columns, built in LDS
//   vcf_gather_kernel           one workgroup per line: its head into the head pool, its columns into the chunk's dense column pool
//
// Every index that comes from input bytes is bounded before it is used: line starts by the slice length, tab positions by the line's
// end, the sample by n_samples, the copy by the sample's ploidy, the allele by n_alts (<= 8), the row by n_rows.  No kernel uses scratch
// memory; LDS is accessed in 32-bit words and bytes only.

#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/v2m_hip.h"
#include "kernels.hpp"

namespace v2m {

constexpr u32 kVcfTileBytes = 4096;             // bytes of text per workgroup of the line index (256 threads x 16 B)
constexpr u32 kVcfThreads = 256;
constexpr u32 kVcfScanThreads = 1024;
constexpr u32 kVcfMaxAlts = 8;                  // condition c
constexpr u32 kVcfMaxRows = 32768;              // the columns of a line fit into LDS: 8 x 4 096 B
constexpr u32 kVcfMaxWordsPerColumn = 512;
constexpr u32 kVcfLinesPerHeadBlock = kVcfThreads / 64;

// flags of a line besides its record (device only): the line is not of kind 0 and its first column is the wanted chromosome
constexpr u32 kVcfLineOnChromosome = 1;

// Inclusive sum over the wave's lanes.
__device__ __forceinline__ u32 vcf_wave_inclusive(u32 v, u32 lane)
{
#pragma unroll
	for (u32 d(1); d < 64; d <<= 1) {
		u32 const o(__shfl_up(v, d, 64));
		if (lane >= d) v += o;
	}
	return v;
}

// Exclusive sum over the workgroup's threads (blockDim.x a multiple of 64, at most 1024); `total` gets the sum.  s_waves: 17 words of
// LDS, free to be reused after the call's last barrier.
__device__ __forceinline__ u32 vcf_block_exclusive(u32 v, u32 *s_waves, u32 &total)
{
	u32 const lane(threadIdx.x & 63), wave(threadIdx.x >> 6), n_waves(blockDim.x >> 6);
	u32 const inc(vcf_wave_inclusive(v, lane));
	__syncthreads();                       // the previous call's reads of s_waves are over
	if (63 == lane) s_waves[wave] = inc;
	__syncthreads();
	u32 before(0), all(0);
	for (u32 w(0); w < n_waves; ++w) {
		u32 const t(s_waves[w]);
		if (w < wave) before += t;
		all += t;
	}
	total = all;
	return before + inc - v;
}

// Bit k of the result: byte k of the 16 bytes at text offset `at` (a multiple of 16 relative to the ALIGNED base) is '\n' and lies in
// the slice.  base16 = the text's first byte rounded down to 16 bytes, lead = text - base16, so that every load is a whole aligned
// 16 bytes inside the allocation.
__device__ __forceinline__ u32 vcf_newline_mask(unsigned char const *base16, u64 at, u32 lead, u64 end)
{
	if (at >= end) return 0;
	vec4u const v(*reinterpret_cast<vec4u const *>(base16 + at));
	u32 m(0);
#pragma unroll
	for (u32 k(0); k < 16; ++k) {
		u32 const byte((v[k >> 2] >> (8 * (k & 3))) & 255u);
		u64 const p(at + k);
		if ('\n' == byte && p >= lead && p < end) m |= 1u << k;
	}
	return m;
}

// counts[t] = the '\n' of tile t.  Tiles are cut from base16 on; end = lead + the slice's length.
__global__ void __launch_bounds__(kVcfThreads) vcf_count_newlines_kernel(unsigned char const *__restrict__ base16, u32 lead, u64 end, u32 *__restrict__ counts)
{
	__shared__ u32 vcf_lds[32];
	V2M_POISON_LDS(vcf_lds);
	u64 const at(u64(blockIdx.x) * kVcfTileBytes + 16 * threadIdx.x);
	u32 const n(__popc(vcf_newline_mask(base16, at, lead, end)));
	u32 total;
	(void) vcf_block_exclusive(n, vcf_lds, total);
	if (0 == threadIdx.x) counts[blockIdx.x] = total;
}

// out[i] = in[0] + ... + in[i - 1], out[n] = the total; one workgroup.
__global__ void __launch_bounds__(kVcfScanThreads) vcf_scan_u32_kernel(u32 const *__restrict__ in, u32 n, u32 *__restrict__ out)
{
	__shared__ u32 vcf_lds[32];
	V2M_POISON_LDS(vcf_lds);
	u32 carry(0);
	for (u32 base(0); base < n; base += kVcfScanThreads) {
		u32 const i(base + threadIdx.x);
		u32 const v(i < n ? in[i] : 0);
		u32 total;
		u32 const ex(vcf_block_exclusive(v, vcf_lds, total));
		if (i < n) out[i] = carry + ex;
		carry += total;
	}
	if (0 == threadIdx.x) out[n] = carry;
}

// line_start[0] = 0 and line_start[k + 1] = the text offset after the k-th '\n' (k < n_newlines); with a last line that has no '\n'
// (final_line: the input ends in this slice), line_start[n_newlines + 1] = length + 1, as if the '\n' were there.
__global__ void __launch_bounds__(kVcfThreads) vcf_line_starts_kernel(unsigned char const *__restrict__ base16, u32 lead, u64 end,
	u32 const *__restrict__ tile_offsets, u32 n_newlines, u32 final_line, u32 *__restrict__ line_start)
{
	__shared__ u32 vcf_lds[32];
	V2M_POISON_LDS(vcf_lds);
	u64 const at(u64(blockIdx.x) * kVcfTileBytes + 16 * threadIdx.x);
	u32 m(vcf_newline_mask(base16, at, lead, end));
	u32 total;
	u32 k(tile_offsets[blockIdx.x] + vcf_block_exclusive(__popc(m), vcf_lds, total));
	while (m) {
		u32 const b(__ffs(m) - 1);
		m &= m - 1;
		if (k < n_newlines) line_start[k + 1] = u32(at + b - lead) + 1;
		++k;
	}
	if (0 == blockIdx.x && 0 == threadIdx.x) {
		line_start[0] = 0;
		if (final_line) line_start[n_newlines + 1] = u32(end - lead) + 1;
	}
}

// The wave's lanes agree on whether text[a, a + n) equals ref[0, n).
__device__ __forceinline__ bool vcf_wave_equal(unsigned char const *text, u32 a, unsigned char const *ref, u32 n, u32 lane)
{
	bool same(true);
	for (u32 i(lane); i < n; i += 64) same = same && text[a + i] == ref[i];
	return 0 == __ballot(!same);
}

// One wave per line.  The line's record before its genotypes are looked at: kind 0, 1 or 3 with its head's length, or kind 2 for a
// candidate (conditions a, b and c hold) with n_alts, the head's length (the bytes before the 9th tab) and, in gt_off, where its sample
// columns begin (relative to the line).  head_offset and column_begin are vcf_alloc_scan_kernel's.
__global__ void __launch_bounds__(kVcfThreads) vcf_head_kernel(unsigned char const *__restrict__ text, u32 const *__restrict__ line_start, u32 n_lines,
	unsigned char const *__restrict__ wanted, u32 wanted_len, v2m_vcf_line *__restrict__ lines, u32 *__restrict__ gt_off, u32 *__restrict__ flags)
{
	u32 const lane(threadIdx.x & 63), line(blockIdx.x * kVcfLinesPerHeadBlock + (threadIdx.x >> 6));
	if (line >= n_lines) return;
	u32 const b(line_start[line]), e(line_start[line + 1] - 1), len(e - b);   // b <= e <= the slice's length: vcf_line_starts_kernel

	u32 kind(3), n_alts(0), head(len), gto(0), flag(0);
	if (0 == len || '#' == text[b]) {
		kind = 0;
		u64 const chrom(0x4D4F52484323ull);                          // "#CHROM", first byte lowest
		bool mine(true);
		if (lane < 6) mine = len >= 6 && text[b + lane] == ((chrom >> (8 * lane)) & 255u);
		head = (len >= 6 && 0 == __ballot(!mine)) ? len : 0;
	} else {
		// the first nine tabs, 64 bytes a step; the positions the rule needs: tabs 0, 3, 4, 7 and 8
		u32 n_tabs(0), t0(e), t3(e), t4(e), t7(e), t8(e);
		for (u32 p(b); p < e && n_tabs < 9; p += 64) {
			u64 m(__ballot(p + lane < e && '\t' == text[p + lane]));
			while (m && n_tabs < 9) {
				u32 const at(p + u32(__ffsll((unsigned long long) m) - 1));
				m &= m - 1;
				t0 = 0 == n_tabs ? at : t0;
				t3 = 3 == n_tabs ? at : t3;
				t4 = 4 == n_tabs ? at : t4;
				t7 = 7 == n_tabs ? at : t7;
				t8 = 8 == n_tabs ? at : t8;
				++n_tabs;
			}
		}
		// column 1: up to the first tab, or the whole line less a final '\r'
		u32 const c1_end(n_tabs ? t0 : ('\r' == text[e - 1] ? e - 1 : e));
		bool const on_chr(c1_end - b == wanted_len && vcf_wave_equal(text, b, wanted, wanted_len, lane));
		flag = on_chr ? kVcfLineOnChromosome : 0;
		if (n_tabs >= 7 && !on_chr) { kind = 1; head = 0; }
		else if (n_tabs >= 9 && '\r' != text[e - 1]) {
			u32 const f0(t7 + 1), flen(t8 - f0);                    // column 9
			bool const gt(flen >= 2 && 'G' == text[f0] && 'T' == text[f0 + 1] && (2 == flen || ':' == text[f0 + 2]));
			u32 commas(0);
			for (u32 p(t3 + 1); p < t4 && commas < kVcfMaxAlts; p += 64) commas += __popcll(__ballot(p + lane < t4 && ',' == text[p + lane]));
			if (gt && commas < kVcfMaxAlts) { kind = 2; n_alts = commas + 1; head = t8 - b; gto = t8 + 1 - b; }
		}
	}
	if (0 == lane) {
		v2m_vcf_line r;
		r.kind = kind;
		r.n_alts = n_alts;
		r.head_offset = 0;
		r.head_length = head;
		r.column_begin = 0;
		lines[line] = r;
		gt_off[line] = gto;
		flags[line] = flag;
	}
}

// Exclusive sums over the lines, one workgroup.  candidates != 0: tmp_begin[i] = the columns of the candidates (kind 2 so far) before
// line i, totals[0] = all of them.  Otherwise head_offset and column_begin of every record, totals[0] = head bytes, totals[1] = columns.
__global__ void __launch_bounds__(kVcfScanThreads) vcf_alloc_scan_kernel(v2m_vcf_line *__restrict__ lines, u32 n_lines, u32 candidates,
	u32 *__restrict__ tmp_begin, u64 *__restrict__ totals)
{
	__shared__ u32 vcf_lds[32];
	V2M_POISON_LDS(vcf_lds);
	u64 heads(0), columns(0);
	for (u32 base(0); base < n_lines; base += kVcfScanThreads) {
		u32 const i(base + threadIdx.x);
		u32 h(0), c(0);
		if (i < n_lines) {
			h = lines[i].head_length;
			c = 2 == lines[i].kind ? lines[i].n_alts : 0;
		}
		u32 total_h, total_c;
		u32 const ex_c(vcf_block_exclusive(c, vcf_lds, total_c));
		if (candidates) {
			if (i < n_lines) tmp_begin[i] = u32(columns) + ex_c;
		} else {
			u32 const ex_h(vcf_block_exclusive(h, vcf_lds, total_h));
			if (i < n_lines) {
				lines[i].head_offset = u32(heads) + ex_h;
				lines[i].column_begin = columns + ex_c;
			}
			heads += total_h;
		}
		columns += total_c;
	}
	if (0 == threadIdx.x) {
		totals[0] = candidates ? columns : heads;
		totals[1] = columns;
	}
}

// What the genotype pass needs of the layout (device pointers).
struct vcf_layout_view {
	u32 const *copy_begin;    // [n_samples + 1]
	int32_t const *row_lookup;   // [copy_begin[n_samples]], -1 = not included, else < n_rows (checked by the host)
	u32 n_samples, n_rows, words_per_column;
};

__device__ __forceinline__ bool vcf_is_digit(u32 c) { return c - u32('0') < 10u; }
__device__ __forceinline__ bool vcf_ends_token(u32 c) { return '\t' == c || '|' == c || '/' == c || ':' == c; }

// One wave per candidate line (a workgroup is one wave; the others leave at once).  Walks the sample columns 64 bytes a step.  Per byte,
// from the step's tab / separator / colon ballots and what the previous steps carry: the sample (tabs so far), the copy (separators since
// the last tab) and whether the byte is still inside the sample's GT subfield (no colon since the last tab).  The byte after a tab or a
// separator starts a token; its lane reads the token from the step's bytes staged in LDS (three bytes past the step's end are staged too)
// and sets the row's bit in the allele's column, which the wave keeps in LDS (kWordsPerColumn: the instance's capacity, so that a narrow
// matrix does not take a wide one's LDS).  The line's end counts as one more tab, so that every
// sample column ends in one.  A line that fails condition d or e becomes kind 3 with its whole text as head; otherwise its columns go to
// tmp_columns at tmp_begin[line].
template <u32 kWordsPerColumn>
__global__ void __launch_bounds__(64) vcf_genotype_kernel(unsigned char const *__restrict__ text, u32 const *__restrict__ line_start, u32 n_lines,
	v2m_vcf_line *__restrict__ lines, u32 const *__restrict__ gt_off, u32 const *__restrict__ tmp_begin, vcf_layout_view const lay, u64 *__restrict__ tmp_columns)
{
	__shared__ u32 s_cols[kVcfMaxAlts * 2 * kWordsPerColumn];      // [n_alts][col_words]
	__shared__ unsigned char s_bytes[80];                          // the step's 64 bytes and 3 of the next
	V2M_POISON_LDS(s_cols);
	V2M_POISON_LDS(s_bytes);
	u32 const lane(threadIdx.x), line(blockIdx.x);
	if (line >= n_lines || 2 != lines[line].kind) return;
	u32 const n_alts(lines[line].n_alts);
	if (0 == n_alts || n_alts > kVcfMaxAlts || lay.words_per_column > kWordsPerColumn) return;   // (never: vcf_head_kernel, v2m_vcf_scan)
	u32 const b(line_start[line]), e(line_start[line + 1] - 1);
	u32 const g0(b + gt_off[line]);                                 // <= e: the byte after the 9th tab
	u32 const col_words(2 * lay.words_per_column);                  // 32-bit words of a column
	for (u32 i(lane); i < n_alts * col_words; i += 64) s_cols[i] = 0;
	__syncthreads();

	u64 const lt((u64(1) << lane) - 1);                             // the lanes before this one
	u32 sample(0), copy(0);
	bool in_gt(true), after_start(true), bad(false);                // after_start: the byte before the step is a tab or a separator
	// [g0, e] with the byte at e read as a tab
	for (u32 p(g0); p <= e; p += 64) {
		u32 const at(p + lane);
		bool const active(at <= e);
		u32 const ch(at < e ? text[at] : u32('\t'));
		s_bytes[lane] = (unsigned char) ch;
		if (lane < 3) s_bytes[64 + lane] = (p + 64 + lane < e) ? text[p + 64 + lane] : (unsigned char) '\t';
		__syncthreads();
		u64 const tabs(__ballot(active && '\t' == ch)), seps(__ballot(active && ('|' == ch || '/' == ch))), colons(__ballot(active && ':' == ch));
		u64 const tabs_before(tabs & lt);
		// the bytes between the last tab before this lane (or the step's start) and this lane
		u64 between(lt);
		if (tabs_before) between = lt & ~((u64(2) << (63 - __clzll((long long) tabs_before))) - 1);
		u32 const my_sample(sample + __popcll(tabs_before));
		u32 const my_copy((tabs_before ? 0 : copy) + __popcll(seps & between));
		bool const my_in_gt((tabs_before ? true : in_gt) && 0 == (colons & between));
		bool const prev_starts(lane ? 0 != ((tabs | seps) >> (lane - 1) & 1) : after_start);

		if (active && my_in_gt) {
			u32 const ploidy(my_sample < lay.n_samples ? lay.copy_begin[my_sample + 1] - lay.copy_begin[my_sample] : 0);
			if (prev_starts) {
				if (my_sample >= lay.n_samples) bad = true;              // more sample columns than the header has (condition d)
				else if (my_copy < ploidy) {                             // condition e; tokens past the ploidy are not looked at
					u32 const c0(ch), c1(s_bytes[lane + 1]), c2(s_bytes[lane + 2]), c3(s_bytes[lane + 3]);
					u32 allele(0);
					bool ok(false);
					if ('.' == c0) ok = vcf_ends_token(c1);
					else if (vcf_is_digit(c0)) {
						allele = c0 - '0';
						if (vcf_ends_token(c1)) ok = true;
						else if (vcf_is_digit(c1)) {
							allele = 10 * allele + (c1 - '0');
							if (vcf_ends_token(c2)) ok = true;
							else if (vcf_is_digit(c2)) { allele = 10 * allele + (c2 - '0'); ok = vcf_ends_token(c3); }
						}
					}
					if (!ok || allele > n_alts) bad = true;
					else if (allele) {
						int32_t const row(lay.row_lookup[lay.copy_begin[my_sample] + my_copy]);
						if (row >= 0 && u32(row) < lay.n_rows && (u32(row) >> 5) < col_words)
							atomicOr(&s_cols[(allele - 1) * col_words + (u32(row) >> 5)], 1u << (u32(row) & 31));
					}
				}
			}
			// a tab or the first colon after it ends the GT subfield: it has my_copy + 1 tokens
			if (('\t' == ch || ':' == ch) && my_sample < lay.n_samples && my_copy + 1 < ploidy) bad = true;
		}

		// what the next step carries
		sample += __popcll(tabs);
		if (tabs) {
			u64 const after(~((u64(2) << (63 - __clzll((long long) tabs))) - 1));
			copy = __popcll(seps & after);
			in_gt = 0 == (colons & after);
		} else {
			copy += __popcll(seps);
			in_gt = in_gt && 0 == colons;
		}
		after_start = 0 != ((tabs | seps) >> 63);
		__syncthreads();                                              // the step's bytes have been read
	}
	bool const declined(0 != __ballot(bad) || sample != lay.n_samples);   // condition d: 8 + n_samples tabs, the line's end counted
	if (declined) {
		if (0 == lane) { lines[line].kind = 3; lines[line].n_alts = 0; lines[line].head_length = e - b; }
		return;
	}
	__syncthreads();
	u64 *const out(tmp_columns + u64(tmp_begin[line]) * lay.words_per_column);
	for (u32 i(lane); i < n_alts * lay.words_per_column; i += 64) out[i] = u64(s_cols[2 * i]) | (u64(s_cols[2 * i + 1]) << 32);
}

// One workgroup per line: the line's head into the head pool, and the columns of an accepted line from the candidates' pool into the
// chunk's.
__global__ void __launch_bounds__(kVcfThreads) vcf_gather_kernel(unsigned char const *__restrict__ text, u32 const *__restrict__ line_start, u32 n_lines,
	v2m_vcf_line const *__restrict__ lines, u32 const *__restrict__ tmp_begin, u64 const *__restrict__ tmp_columns, u32 words_per_column,
	u64 head_bytes, u64 n_columns, unsigned char *__restrict__ heads, u64 *__restrict__ columns)
{
	u32 const line(blockIdx.x);
	if (line >= n_lines) return;
	v2m_vcf_line const r(lines[line]);
	u32 const b(line_start[line]), len(line_start[line + 1] - 1 - b);
	if (r.head_length <= len && u64(r.head_offset) + r.head_length <= head_bytes)
		for (u32 i(threadIdx.x); i < r.head_length; i += kVcfThreads) heads[r.head_offset + i] = text[b + i];
	if (2 == r.kind && r.column_begin + r.n_alts <= n_columns) {
		u64 const *const src(tmp_columns + u64(tmp_begin[line]) * words_per_column);
		u64 *const dst(columns + r.column_begin * words_per_column);
		for (u32 i(threadIdx.x); i < r.n_alts * words_per_column; i += kVcfThreads) dst[i] = src[i];
	}
}

} // namespace v2m
