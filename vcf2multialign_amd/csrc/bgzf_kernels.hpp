// bgzf_kernels.hpp -- BGZF (SAM/BAM specification section 4.1) encoder for row bodies, gfx950.
//
// bgzf_deflate_kernel: one workgroup per block of <= 65 280 input bytes, one complete BGZF member per 64-KiB output slot.
//   The block is staged in LDS and cut into 256-byte segments, one per thread.  Tokens are zlib's Z_RLE ones (a run of n equal
//   bytes = one literal, then distance-1 matches of 258 and one of 3..257, a remainder < 3 as literals), so a run's tokens are a
//   closed form of its start and end: each thread finds the run starts of its segment, block scans give every thread the run
//   around its first byte and the next start after its last, and each thread emits the tokens that START in its segment.
//   Literal/length histogram in LDS -> length-limited Huffman codes (limit 15, code-length code limit 7) built by one wave ->
//   the bit cost of every thread's tokens -> a block prefix sum gives each thread its bit offset -> one final dynamic block
//   (BTYPE 10) packed into an LDS staging slot with ds_or, or a stored block when that is not larger.
//   CRC-32: every thread a table CRC of its segment in the raw register form (init 0, no final xor), moved to the block's end
//   by multiplying with x^(8 L) mod P (powers x^(2^k) precomputed, from k = 3 on for whole bytes), xor-reduced; the init and final xor
//   are applied once.
// bgzf_scan_kernel: exclusive scan of the member sizes of a slice (one workgroup), row extents + slice total into a small table.
// bgzf_compact_kernel: copies the members densely to their scanned offsets.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.hpp"   // V2M_POISON_LDS

// Tables in constant memory, outside namespace v2m: tests/test_kernel_isa.py reads every _ZN3v2m label of the ISA as a kernel.
// x^(2^k) mod P in the reflected representation (CRC-32, P = 0xEDB88320); crc_shift by n bytes starts at k = 3 (x^8: one byte)
__constant__ static uint32_t const kBgzfCrcX2n[32] = {
	0x40000000, 0x20000000, 0x08000000, 0x00800000, 0x00008000, 0xedb88320, 0xb1e6b092, 0xa06a2517, 0xed627dae, 0x88d14467, 0xd7bbfe6a,
	0xec447f11, 0x8e7ea170, 0x6427800e, 0x4d47bae0, 0x09fe548f, 0x83852d0f, 0x30362f1a, 0x7b5a9cc3, 0x31fec169, 0x9fec022a, 0x6c8dedc4,
	0x15d6874d, 0x5fde7a4e, 0xbad90e37, 0x2e4e5eef, 0x4eaba214, 0xa8a472c0, 0x429a969e, 0x148d302a, 0xc40ba6d0, 0xc4e22c3c};
// the order in which a dynamic block header lists the code-length code's lengths (RFC 1951 section 3.2.7)
__constant__ static unsigned char const kBgzfClOrder[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
// the first 16 bytes of every member: 1f 8b 08 04 | mtime 0 | xfl 0, os ff | xlen 6 | 'B' 'C' 02 00; then bsize = member length - 1
__constant__ static unsigned char const kBgzfHead[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 0x42, 0x43, 2, 0};

namespace v2m {

constexpr u32 kBgzfBlockBytes = 65280;          // uncompressed bytes per member (0xff00, htslib's block size)
constexpr u32 kBgzfSlotBytes = 65536;           // the largest member
constexpr u32 kBgzfThreads = 256;
constexpr u32 kBgzfSegBytes = 256;              // bytes per thread
constexpr u32 kBgzfSegs = kBgzfBlockBytes / kBgzfSegBytes;   // 255
constexpr u32 kBgzfSegStride = 17;              // 16-B words per staged segment: one of padding makes the threads' ds_read_b128 conflict-free
constexpr u32 kBgzfHistCopies = 8;              // literal/length histogram copies (lane % 8): fewer lanes on one address per ds_add
constexpr u32 kBgzfSyms = 288;
constexpr u32 kBgzfHeaderBytes = 18;            // gzip header with the BC extra subfield
constexpr u32 kBgzfFooterBytes = 8;             // CRC-32, ISIZE
constexpr u32 kBgzfStoredOverhead = kBgzfHeaderBytes + 5 + kBgzfFooterBytes;   // one stored block

__device__ inline void bgzf_sync()
{
	asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // every barrier waits for the LDS first (tests/test_kernel_isa.py)
	__syncthreads();
}

// a * b mod P (reflected: bit 31 = x^0)
__device__ inline u32 crc_mulmod(u32 a, u32 b)
{
	u32 p(0);
	for (u32 m(0x80000000u); m; m >>= 1) {
		if (a & m) p ^= b;
		b = (b & 1) ? (b >> 1) ^ 0xEDB88320u : b >> 1;
	}
	return p;
}

// the raw CRC register x followed by n zero bytes
__device__ inline u32 crc_shift(u32 x, u32 n)
{
	u32 p(0x80000000u);
	for (int k(3); n; n >>= 1, ++k)
		if (n & 1) p = crc_mulmod(kBgzfCrcX2n[k & 31], p);
	return crc_mulmod(p, x);
}

// Deflate's length code of a match length 3..258: index 0..28 (symbol 257 + index), extra bits and their value.
__device__ inline void deflate_length_code(u32 len, u32 &idx, u32 &eb, u32 &ev)
{
	if (258 == len) { idx = 28; eb = 0; ev = 0; return; }
	u32 const l(len - 3);
	if (l < 8) { idx = l; eb = 0; ev = 0; return; }
	eb = (31 - __builtin_clz(l)) - 2;
	idx = 4 * eb + 4 + ((l >> eb) - 4);
	ev = l & ((1u << eb) - 1);
}

// Block scans over the 256 threads (4 waves): wave scans through shuffles, the waves' totals through `tmp` (4 entries, one
// region per call site).  op must be associative; `id` its identity.  reverse: the scan runs from the last thread down.
template <typename t_op>
__device__ inline u32 bgzf_block_scan_excl(u32 v, u32 id, t_op op, bool reverse, u32 *tmp, u32 *total)
{
	int const lane(threadIdx.x & 63), wave(threadIdx.x >> 6);
	u32 incl(v);
	for (int d(1); d < 64; d <<= 1) {
		u32 const y(reverse ? __shfl_down(incl, d) : __shfl_up(incl, d));
		if (reverse ? (lane + d < 64) : (lane >= d)) incl = op(incl, y);
	}
	u32 excl(reverse ? __shfl_down(incl, 1) : __shfl_up(incl, 1));
	if (reverse ? 63 == lane : 0 == lane) excl = id;
	if (reverse ? 0 == lane : 63 == lane) tmp[wave] = incl;
	bgzf_sync();
	u32 carry(id), all(id);
	for (int w(0); w < 4; ++w) {
		u32 const tw(tmp[w]);
		all = op(all, tw);
		if (reverse ? w > wave : w < wave) carry = op(carry, tw);
	}
	if (total) *total = all;
	return op(carry, excl);
}

struct bgzf_huff_scratch {
	u32 keys[kBgzfSyms];
	u32 sorted[kBgzfSyms];
	u32 a[kBgzfSyms];
	u32 bl_count[17];
	u32 next_code[17];
	u32 m;
};

// Length-limited canonical Huffman code of freq[0, nsym) (every thread calls; wave 0 and its lane 0 do the work):
// len_out[s] = code length (0: unused), code_out[s] = the code bit-reversed for deflate's LSB-first packing.
// A code with fewer than two used symbols gets dummies of frequency 1, so that it is always complete.
__device__ inline void bgzf_huff_build(u32 const *freq, int nsym, int max_len, u32 *len_out, u32 *code_out, bgzf_huff_scratch &s)
{
	int const t(threadIdx.x), lane(t & 63);
	u64 const below((u64(1) << lane) - 1);
	if (t < 64) {   // the used symbols, as (frequency << 9 | symbol) keys
		u32 base(0);
		for (int c(0); c < nsym; c += 64) {
			int const sym(c + lane);
			u32 const f(sym < nsym ? freq[sym] : 0);
			u64 const m(__ballot(0 != f));
			if (f) s.keys[base + __popcll(m & below)] = (f << 9) | u32(sym);
			base += __popcll(m);
			if (sym < nsym) { len_out[sym] = 0; code_out[sym] = 0; }
		}
		if (0 == lane) {
			if (0 == base) { s.keys[0] = (1u << 9) | 0; s.keys[1] = (1u << 9) | 1; base = 2; }
			else if (1 == base) { s.keys[1] = (1u << 9) | ((s.keys[0] & 511) ? 0u : 1u); base = 2; }
			s.m = base;
		}
	}
	bgzf_sync();
	int const m(int(s.m));
	if (t < 64)   // rank sort (keys are distinct)
		for (int i(lane); i < m; i += 64) {
			u32 const k(s.keys[i]);
			int r(0);
			for (int j(0); j < m; ++j) r += s.keys[j] < k;
			s.sorted[r] = k;
		}
	bgzf_sync();
	if (0 == t) {
		// Huffman code lengths of the ascending frequencies, in place (Moffat and Katajainen, "In-place calculation of
		// minimum-redundancy codes", 1995)
		u32 *const a(s.a);
		for (int i(0); i < m; ++i) a[i] = s.sorted[i] >> 9;
		a[0] += a[1];
		int root(0), leaf(2);
		for (int next(1); next < m - 1; ++next) {
			if (leaf >= m || a[root] < a[leaf]) { a[next] = a[root]; a[root++] = u32(next); }
			else a[next] = a[leaf++];
			if (leaf >= m || (root < next && a[root] < a[leaf])) { a[next] += a[root]; a[root++] = u32(next); }
			else a[next] += a[leaf++];
		}
		a[m - 2] = 0;
		for (int next(m - 3); next >= 0; --next) a[next] = a[a[next]] + 1;
		int avail(1), used(0), depth(0), next(m - 1);
		root = m - 2;
		while (avail > 0) {
			while (root >= 0 && int(a[root]) == depth) { ++used; --root; }
			while (avail > used) { a[next--] = u32(depth); --avail; }
			avail = 2 * used; ++depth; used = 0;
		}
		// limit: fold the longer codes into max_len, then take leaves off the longest level until the Kraft sum is 1 again
		for (int l(0); l <= 16; ++l) s.bl_count[l] = 0;
		for (int i(0); i < m; ++i) ++s.bl_count[min(int(a[i]), max_len)];
		u32 total(0);
		for (int l(max_len); l > 0; --l) total += s.bl_count[l] << (max_len - l);
		while (total > (1u << max_len)) {
			--s.bl_count[max_len];
			for (int l(max_len - 1); l > 0; --l)
				if (s.bl_count[l]) { --s.bl_count[l]; s.bl_count[l + 1] += 2; break; }
			--total;
		}
		// the shortest codes to the most frequent symbols
		int j(m);
		for (int l(1); l <= max_len; ++l)
			for (u32 k(s.bl_count[l]); k; --k) len_out[s.sorted[--j] & 511] = u32(l);
		u32 code(0);
		s.bl_count[0] = 0;
		for (int l(1); l <= 15; ++l) {
			code = (code + (l - 1 <= max_len ? s.bl_count[l - 1] : 0)) << 1;
			s.next_code[l] = code;
		}
	}
	bgzf_sync();
	if (t < 64) {   // canonical codes: per length, in symbol order
		u32 nx[16];
#pragma unroll
		for (int l(1); l <= 15; ++l) nx[l] = s.next_code[l];
		for (int c(0); c < nsym; c += 64) {
			int const sym(c + lane);
			u32 const l(sym < nsym ? len_out[sym] : 0);
			u32 code(0);
#pragma unroll
			for (int L(1); L <= 15; ++L) {
				u64 const mk(__ballot(l == u32(L)));
				if (l == u32(L)) code = nx[L] + __popcll(mk & below);
				nx[L] += __popcll(mk);
			}
			if (l) code_out[sym] = __builtin_bitreverse32(code) >> (32 - l);
		}
	}
	bgzf_sync();
}

// Bits into the LDS staging slot, LSB first, from bit position `pos` on; whole words go out with ds_or (a neighbour owns the other
// bits of the first and last word).
struct bgzf_bit_writer {
	u32 *out;
	u64 acc;
	u32 nb, w;
	__device__ bgzf_bit_writer(u32 *o, u32 pos) : out(o), acc(0), nb(pos & 31), w(pos >> 5) {}
	__device__ void put(u32 v, u32 n)
	{
		acc |= u64(v) << nb;
		nb += n;
		if (nb >= 32) { atomicOr(&out[w], u32(acc)); ++w; acc >>= 32; nb -= 32; }
	}
	__device__ void flush() { if (nb) atomicOr(&out[w], u32(acc)); }
};

struct bgzf_lds {
	vec4u in[kBgzfSegs * kBgzfSegStride];          // the input block, segment t at [t * 17, t * 17 + 16)
	vec4u stage[kBgzfSlotBytes / 16];              // the member being packed
	u32 hist[kBgzfHistCopies][kBgzfSyms];
	u32 crc_table[256];
	u32 freq[kBgzfSyms], lit_len[kBgzfSyms], lit_code[kBgzfSyms];
	bgzf_huff_scratch huff;
	u32 cl_freq[19], cl_len[19], cl_code[19];
	u32 rle[kBgzfSyms + 2];                        // code-length tokens: symbol | extra << 8
	u32 n_rle, n_lit, n_cl, header_bits, crc;
	u32 tmp[5][4];
};

__device__ inline u32 bgzf_in_byte(bgzf_lds const &s, u32 i)
{
	return reinterpret_cast<unsigned char const *>(s.in)[(i >> 8) * (kBgzfSegStride * 16) + (i & 255)];
}

// Calls body(i, byte) for the bytes of [s0, s1) in order, from 16-B LDS reads.  (Loops kept rolled: the four walks over a segment
// inline their bodies here, and unrolled copies of them ran the kernel out of scalar registers.)
template <typename t_body>
__device__ inline void bgzf_for_bytes(bgzf_lds const &s, u32 seg, u32 s0, u32 s1, t_body &&body)
{
#pragma unroll 1
	for (u32 c(0); c < 16 && s0 + 16 * c < s1; ++c) {
		vec4u const v(s.in[seg * kBgzfSegStride + c]);
#pragma unroll 1
		for (u32 q(0); q < 4; ++q) {
			u32 const w(0 == q ? v.x : 1 == q ? v.y : 2 == q ? v.z : v.w);
#pragma unroll 1
			for (u32 b(0); b < 4; ++b) {
				u32 const i(s0 + 16 * c + 4 * q + b);
				if (i < s1) body(i, (w >> (8 * b)) & 255);
			}
		}
	}
}

// The Z_RLE tokens of the run [p, e) of byte b that start in [lo, hi): lit(b) per literal, match(len, count) per group of equal matches.
template <typename t_lit, typename t_match>
__device__ inline void bgzf_run_tokens(u32 p, u32 e, u32 b, u32 lo, u32 hi, t_lit &&lit, t_match &&match)
{
	if (p >= lo && p < hi) lit(b);
	u32 const m(e - p - 1), q(m / 258), r(m - 258 * q);
	if (q) {
		u32 const first(p + 1);
		u32 const k_lo(lo > first ? (lo - first + 257) / 258 : 0), k_hi(hi > first ? min(q, (hi - first + 257) / 258) : 0);
		if (k_hi > k_lo) match(258u, k_hi - k_lo);
	}
	u32 const tail(p + 1 + 258 * q);
	if (r >= 3) { if (tail >= lo && tail < hi) match(r, 1u); }
	else for (u32 k(0); k < r; ++k) if (tail + k >= lo && tail + k < hi) lit(b);
}

// Walks the runs that meet [s0, s1): P = the start of the run around s0, E = the first run start after s1 - 1 (or the block's end).
template <typename t_lit, typename t_match>
__device__ inline void bgzf_walk_runs(bgzf_lds const &s, u32 seg, u32 s0, u32 s1, u32 P, u32 E, t_lit &&lit, t_match &&match)
{
	if (s0 >= s1) return;
	u32 p(P), rb(bgzf_in_byte(s, s0));
	bgzf_for_bytes(s, seg, s0, s1, [&](u32 i, u32 b) {
		if (b == rb) return;
		bgzf_run_tokens(p, i, rb, s0, s1, lit, match);
		p = i;
		rb = b;
	});
	bgzf_run_tokens(p, E, rb, s0, s1, lit, match);
}

__device__ inline void bgzf_put_header(u32 *out, u32 member_bytes)
{
	atomicOr(&out[0], 0x04088b1fu);
	atomicOr(&out[2], 0xff00u | (6u << 16));
	atomicOr(&out[3], 0x42u | (0x43u << 8) | (2u << 16));
	atomicOr(&out[4], (member_bytes - 1) & 0xffffu);
}

__device__ inline void bgzf_or_byte(u32 *out, u32 pos, u32 b) { atomicOr(&out[pos >> 2], (b & 255) << (8 * (pos & 3))); }

// rows: row r at rows + r * pitch, lengths[r] bytes (or `length` for every row when lengths == NULL); blocks_per_row blocks per row in
// the grid (row = blockIdx.x / blocks_per_row).  Member of block k -> slots + k * 65536, its size -> sizes[k] (0 past a row's end).
__global__ void __launch_bounds__(kBgzfThreads) bgzf_deflate_kernel(char const *__restrict__ rows, u64 pitch, u64 const *__restrict__ lengths, u64 length,
	u32 blocks_per_row, char *__restrict__ slots, u32 *__restrict__ sizes)
{
	__shared__ bgzf_lds s;
	u32 const t(threadIdx.x), lane(t & 63);
	u64 const k(blockIdx.x), row(k / blocks_per_row), j(k % blocks_per_row);
	u64 const row_len(lengths ? lengths[row] : length);
	if (j * kBgzfBlockBytes >= row_len) { if (0 == t) sizes[k] = 0; return; }
	V2M_POISON_LDS(s);
	u32 const nb(u32(row_len - j * kBgzfBlockBytes < kBgzfBlockBytes ? row_len - j * kBgzfBlockBytes : kBgzfBlockBytes));
	char const *const src(rows + row * pitch + j * kBgzfBlockBytes);

	{   // CRC table, cleared staging slot and histograms, the block into LDS
		u32 c(t);
		for (int b(0); b < 8; ++b) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
		s.crc_table[t] = c;
		for (u32 i(t); i < kBgzfSlotBytes / 16; i += kBgzfThreads) s.stage[i] = vec4u{0, 0, 0, 0};
		for (u32 i(t); i < kBgzfHistCopies * kBgzfSyms; i += kBgzfThreads) (&s.hist[0][0])[i] = 0;
		u32 const n16(nb / 16);
		for (u32 i(t); i < n16; i += kBgzfThreads) s.in[(i >> 4) * kBgzfSegStride + (i & 15)] = reinterpret_cast<vec4u const *>(src)[i];
		for (u32 i(n16 * 16 + t); i < nb; i += kBgzfThreads)
			reinterpret_cast<unsigned char *>(s.in)[(i >> 8) * (kBgzfSegStride * 16) + (i & 255)] = static_cast<unsigned char>(src[i]);
	}
	bgzf_sync();

	u32 const s0(min(t * kBgzfSegBytes, nb)), s1(min(s0 + kBgzfSegBytes, nb));
	u32 crc(0), first(0xFFFFFFFFu), last1(0);   // last1: the last run start + 1 (0: none)
	{
		u32 prev(s0 ? bgzf_in_byte(s, s0 - 1) : 0x100u);
		bgzf_for_bytes(s, t, s0, s1, [&](u32 i, u32 b) {
			crc = s.crc_table[(crc ^ b) & 255] ^ (crc >> 8);
			if (b != prev) { if (0xFFFFFFFFu == first) first = i; last1 = i + 1; }
			prev = b;
		});
	}
	u32 const before(bgzf_block_scan_excl(last1, 0u, [](u32 a, u32 b) { return max(a, b); }, false, s.tmp[0], nullptr));
	u32 const after(bgzf_block_scan_excl(first, 0xFFFFFFFFu, [](u32 a, u32 b) { return min(a, b); }, true, s.tmp[1], nullptr));
	u32 const P(first == s0 ? s0 : before - 1), E(min(after, nb));
	{   // CRC: this segment's register moved to the block's end, xor over all segments
		u32 x(s0 < s1 ? crc_shift(crc, nb - s1) : 0);
		for (int d(32); d; d >>= 1) x ^= __shfl_xor(x, d);
		if (0 == lane) s.tmp[2][t >> 6] = x;
	}

	// literal/length histogram
	u32 *const hist(s.hist[lane & (kBgzfHistCopies - 1)]);
	bgzf_walk_runs(s, t, s0, s1, P, E,
		[&](u32 b) { atomicAdd(&hist[b], 1u); },
		[&](u32 len, u32 count) { u32 idx, eb, ev; deflate_length_code(len, idx, eb, ev); atomicAdd(&hist[257 + idx], count); });
	bgzf_sync();
	if (0 == t) s.crc = ~(crc_shift(0xFFFFFFFFu, nb) ^ s.tmp[2][0] ^ s.tmp[2][1] ^ s.tmp[2][2] ^ s.tmp[2][3]);
	for (u32 sym(t); sym < kBgzfSyms; sym += kBgzfThreads) {
		u32 f(256 == sym ? 1 : 0);   // end of block
		for (u32 c(0); c < kBgzfHistCopies; ++c) f += s.hist[c][sym];
		s.freq[sym] = sym < 286 ? f : 0;
	}
	bgzf_sync();
	bgzf_huff_build(s.freq, 286, 15, s.lit_len, s.lit_code, s.huff);

	if (0 == t) {   // the code lengths (HLIT of them, then the one distance code's 1), run-length coded with 16 / 17 / 18
		u32 n_lit(286);
		while (n_lit > 257 && 0 == s.lit_len[n_lit - 1]) --n_lit;
		s.n_lit = n_lit;
		u32 const n_all(n_lit + 1);
		for (int c(0); c < 19; ++c) s.cl_freq[c] = 0;
		u32 n_rle(0);
		auto const seq([&](u32 i) -> u32 { return i < n_lit ? s.lit_len[i] : 1u; });
		auto const tok([&](u32 sym, u32 extra) { s.rle[n_rle++] = sym | (extra << 8); ++s.cl_freq[sym]; });
		for (u32 i(0); i < n_all;) {
			u32 const l(seq(i));
			u32 run(1);
			while (i + run < n_all && seq(i + run) == l) ++run;
			i += run;
			if (0 == l) {
				while (run >= 11) { u32 const r(min(run, 138u)); tok(18, r - 11); run -= r; }
				if (run >= 3) { tok(17, run - 3); run = 0; }
				while (run) { tok(0, 0); --run; }
			} else {
				tok(l, 0);
				--run;
				while (run >= 3) { u32 const r(min(run, 6u)); tok(16, r - 3); run -= r; }
				while (run) { tok(l, 0); --run; }
			}
		}
		s.n_rle = n_rle;
	}
	bgzf_sync();
	bgzf_huff_build(s.cl_freq, 19, 7, s.cl_len, s.cl_code, s.huff);
	if (0 == t) {
		u32 n_cl(19);
		while (n_cl > 4 && 0 == s.cl_len[kBgzfClOrder[n_cl - 1]]) --n_cl;
		s.n_cl = n_cl;
		u32 h(3 + 5 + 5 + 4 + 3 * n_cl);
		for (u32 i(0); i < s.n_rle; ++i) {
			u32 const sym(s.rle[i] & 255);
			h += s.cl_len[sym] + (16 == sym ? 2 : 17 == sym ? 3 : 18 == sym ? 7 : 0);
		}
		s.header_bits = h;
	}

	// the bits of this thread's tokens, and where they go
	u32 bits(0);
	bgzf_walk_runs(s, t, s0, s1, P, E,
		[&](u32 b) { bits += s.lit_len[b]; },
		[&](u32 len, u32 count) { u32 idx, eb, ev; deflate_length_code(len, idx, eb, ev); bits += count * (s.lit_len[257 + idx] + eb + 1); });
	u32 token_bits(0);
	u32 const offset(bgzf_block_scan_excl(bits, 0u, [](u32 a, u32 b) { return a + b; }, false, s.tmp[3], &token_bits));   // (its barrier publishes header_bits)
	u32 const H(s.header_bits), data_bits(H + token_bits + s.lit_len[256]);
	u32 const dynamic_bytes(kBgzfHeaderBytes + (data_bits + 7) / 8 + kBgzfFooterBytes), stored_bytes(nb + kBgzfStoredOverhead);
	u32 const crc32(s.crc);
	char *const slot(slots + k * kBgzfSlotBytes);
	u32 *const out(reinterpret_cast<u32 *>(s.stage));

	if (stored_bytes <= dynamic_bytes) {   // stored block: every thread builds words of the member straight from the staged input
		u32 const n_words((stored_bytes + 3) / 4);
		for (u32 w(t); w < n_words; w += kBgzfThreads) {
			u32 word(0);
			for (u32 b(0); b < 4; ++b) {
				u32 const pos(4 * w + b);
				u32 v(0);
				if (pos < kBgzfHeaderBytes) {
					v = pos < 16 ? kBgzfHead[pos] : (((stored_bytes - 1) >> (8 * (pos - 16))) & 255);
				} else if (pos < kBgzfHeaderBytes + 5) {
					u32 const q(pos - kBgzfHeaderBytes);
					v = 0 == q ? 1u : q < 3 ? (nb >> (8 * (q - 1))) & 255 : (~nb >> (8 * (q - 3))) & 255;
				} else if (pos < kBgzfHeaderBytes + 5 + nb) {
					v = bgzf_in_byte(s, pos - kBgzfHeaderBytes - 5);
				} else if (pos < stored_bytes) {
					u32 const q(pos - kBgzfHeaderBytes - 5 - nb);
					v = ((q < 4 ? crc32 : nb) >> (8 * (q & 3))) & 255;
				}
				word |= v << (8 * b);
			}
			reinterpret_cast<u32 *>(slot)[w] = word;
		}
		if (0 == t) sizes[k] = stored_bytes;
		return;
	}

	{
		bgzf_bit_writer bw(out, 8 * kBgzfHeaderBytes + H + offset);
		bgzf_walk_runs(s, t, s0, s1, P, E,
			[&](u32 b) { bw.put(s.lit_code[b], s.lit_len[b]); },
			[&](u32 len, u32 count) {
				u32 idx, eb, ev;
				deflate_length_code(len, idx, eb, ev);
				u32 const l(s.lit_len[257 + idx]), v(s.lit_code[257 + idx] | (ev << l));   // then distance code 0: one 0 bit
				for (u32 c(0); c < count; ++c) bw.put(v, l + eb + 1);
			});
		bw.flush();
	}
	if (0 == t) {
		bgzf_put_header(out, dynamic_bytes);
		bgzf_bit_writer bw(out, 8 * kBgzfHeaderBytes);
		bw.put(1 | (2 << 1), 3);   // BFINAL, BTYPE = 10
		bw.put(s.n_lit - 257, 5);
		bw.put(0, 5);              // HDIST: one distance code
		bw.put(s.n_cl - 4, 4);
		for (u32 i(0); i < s.n_cl; ++i) bw.put(s.cl_len[kBgzfClOrder[i]], 3);
		for (u32 i(0); i < s.n_rle; ++i) {
			u32 const sym(s.rle[i] & 255), extra(s.rle[i] >> 8);
			bw.put(s.cl_code[sym], s.cl_len[sym]);
			if (16 == sym) bw.put(extra, 2);
			else if (17 == sym) bw.put(extra, 3);
			else if (18 == sym) bw.put(extra, 7);
		}
		bw.flush();
		bgzf_bit_writer eob(out, 8 * kBgzfHeaderBytes + H + token_bits);
		eob.put(s.lit_code[256], s.lit_len[256]);
		eob.flush();
		u32 const f(dynamic_bytes - kBgzfFooterBytes);
		for (u32 b(0); b < 4; ++b) { bgzf_or_byte(out, f + b, crc32 >> (8 * b)); bgzf_or_byte(out, f + 4 + b, nb >> (8 * b)); }
		sizes[k] = dynamic_bytes;
	}
	bgzf_sync();
	for (u32 i(t); i < (dynamic_bytes + 15) / 16; i += kBgzfThreads) reinterpret_cast<vec4u *>(slot)[i] = s.stage[i];
}

// One workgroup: offsets[k] = the sum of sizes[0, k); table[r] = offsets[r * blocks_per_row] for r < n_rows, table[n_rows] = the total.
constexpr u32 kBgzfScanThreads = 1024;
__global__ void __launch_bounds__(kBgzfScanThreads) bgzf_scan_kernel(u32 const *__restrict__ sizes, u64 n_blocks, u32 blocks_per_row, u64 n_rows,
	u64 *__restrict__ offsets, u64 *__restrict__ table)
{
	__shared__ u64 wave_sums[kBgzfScanThreads / 64];
	__shared__ u64 carry_in;
	V2M_POISON_LDS(wave_sums);
	V2M_POISON_LDS(carry_in);
	u32 const t(threadIdx.x), lane(t & 63), wave(t >> 6);
	if (0 == t) carry_in = 0;
	for (u64 base(0); base < n_blocks; base += kBgzfScanThreads) {
		u64 const k(base + t);
		u64 const v(k < n_blocks ? sizes[k] : 0);
		u64 incl(v);
		for (int d(1); d < 64; d <<= 1) {
			u64 const y(__shfl_up(incl, d));
			if (lane >= u32(d)) incl += y;
		}
		if (63 == lane) wave_sums[wave] = incl;
		bgzf_sync();
		u64 before(carry_in), all(carry_in);
		for (u32 w(0); w < kBgzfScanThreads / 64; ++w) { if (w < wave) before += wave_sums[w]; all += wave_sums[w]; }
		if (k < n_blocks) {
			offsets[k] = before + incl - v;
			if (0 == k % blocks_per_row) table[k / blocks_per_row] = before + incl - v;
		}
		bgzf_sync();
		if (0 == t) carry_in = all;
	}
	bgzf_sync();
	if (0 == t) table[n_rows] = carry_in;
}

// Block k's member from its slot to dense + offsets[k].
__global__ void __launch_bounds__(256) bgzf_compact_kernel(char const *__restrict__ slots, u32 const *__restrict__ sizes, u64 const *__restrict__ offsets,
	char *__restrict__ dense)
{
	u64 const k(blockIdx.x);
	u32 const n(sizes[k]);
	if (0 == n) return;
	unsigned char const *const src(reinterpret_cast<unsigned char const *>(slots + k * kBgzfSlotBytes));
	unsigned char *const dst(reinterpret_cast<unsigned char *>(dense + offsets[k]));
	u32 const head(min(n, u32((4 - (reinterpret_cast<uintptr_t>(dst) & 3)) & 3)));
	if (threadIdx.x < head) dst[threadIdx.x] = src[threadIdx.x];
	u32 const n_words((n - head) / 4);
	for (u32 w(threadIdx.x); w < n_words; w += 256) {
		u32 const p(head + 4 * w);
		reinterpret_cast<u32 *>(dst + head)[w] = u32(src[p]) | (u32(src[p + 1]) << 8) | (u32(src[p + 2]) << 16) | (u32(src[p + 3]) << 24);
	}
	for (u32 i(head + 4 * n_words + threadIdx.x); i < n; i += 256) dst[i] = src[i];
}

} // namespace v2m
