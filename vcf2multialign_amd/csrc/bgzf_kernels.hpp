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
//
// bgzf_inflate_kernel: the decoder of BGZF input (v2m_bgzf_decompress), one wave (a workgroup of 64) per member.  The member's whole
//   output (<= 64 KiB) stays in LDS, so back-references read LDS and never global memory the wave has just written.  Symbol decoding
//   is serial and wave-uniform: the bit buffer, the block state and every decoded symbol live in scalar registers, the compressed
//   words come in as two 64-word windows in VGPRs (lane k holds word base + k; v_readlane picks one), so one vector load serves 256
//   bytes and the next window is in flight while the current one is used.  Canonical codes with a 10-bit (literal/length), 8-bit
//   (distance) or 7-bit (code-length) root table and a per-length walk for longer codes.  The 64 lanes share the parallel work: a
//   match copy (lane k writes out[p + k] = out[p - d + (k mod d)], right for overlapping copies without rounds), stored blocks, the
//   table fills, the CRC-32 (a table CRC per lane over 1 KiB, combined with crc_shift as in the encoder) and the 16-B stores out.
//   Every index that comes from the input is bounded before use; what zlib's inflate refuses is refused (kInflate* codes below).
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


// ---- BGZF input: the decoder --------------------------------------------------------------------

constexpr u32 kInflateThreads = 64;
constexpr u32 kInflateLitRoot = 10, kInflateDistRoot = 8, kInflateClRoot = 7;
constexpr u32 kInflateNoSymbol = 0xFFFFFFFFu;

// status of a member (what was wrong with it; the host's names in v2m_hip.hip: inflate_status_text)
enum : u32 {
	kInflateOk = 0, kInflateBadBlockType, kInflateStoredLengths, kInflateTooManySymbols, kInflateBadCodeLengthCode, kInflateBadRepeat,
	kInflateBadLitLenCode, kInflateBadDistCode, kInflateNoEndOfBlock, kInflateBadLitLenSymbol, kInflateBadDistSymbol, kInflateTooFarBack,
	kInflateOutputTooLong, kInflatePastPayload, kInflateShortOutput, kInflateBadCrc, kInflateBadFraming, kInflateStatusCount
};

// A canonical Huffman code (RFC 1951 section 3.2.2): per length L, count[L] codes starting at first[L], whose symbols are
// sorted[offs[L] ...] in symbol order; max = the longest length used.
struct inflate_code {
	u32 count[16], first[16], offs[16];
	u32 max;
};

struct alignas(16) inflate_lds {
	unsigned char out[kBgzfSlotBytes + 16];    // the member's output from out[o] on, o = its global address mod 16
	u32 crc_table[256];
	u16 lit_table[1u << kInflateLitRoot], dist_table[1u << kInflateDistRoot], cl_table[1u << kInflateClRoot];   // (symbol << 4 | length), 0: none
	u16 lit_sorted[288], dist_sorted[32], cl_sorted[19];
	unsigned char lens[320], cl_lens[20];      // HLIT + HDIST code lengths (fixed blocks: 288 + 32); the code-length code's
	inflate_code lit, dist, cl;
};

__device__ inline u32 inflate_uni(u32 v) { return __builtin_amdgcn_readfirstlane(v); }

// The code of lens[0, n) into c, sorted and the root table (2^root entries).  false for a code zlib's inflate refuses: an over-subscribed
// one, an incomplete one (allowed only as a single code of length 1, never for the code-length code), a code-length code without codes.
// All 64 lanes call; all return the same.
__device__ inline bool inflate_build(unsigned char const *lens, u32 n, u32 root, bool is_cl, inflate_code &c, u16 *sorted, u16 *table)
{
	u32 const lane(threadIdx.x);
	u64 const below((u64(1) << lane) - 1);
	int left(1);
	u32 first(0), offs(0), max(0);
#pragma unroll 1
	for (u32 L(1); L <= 15; ++L) {
		u32 cnt(0);
#pragma unroll 1
		for (u32 b(0); b < n; b += 64) {
			u32 const sym(b + lane);
			bool const hit(sym < n && u32(lens[sym]) == L);
			u64 const m(__ballot(hit));
			if (hit) sorted[offs + cnt + __popcll(m & below)] = u16(sym);   // < the sum of all counts <= n
			cnt += __popcll(m);
		}
		if (0 == lane) { c.count[L] = cnt; c.first[L] = first; c.offs[L] = offs; }
		left = 2 * left - int(cnt);
		if (left < -65536) left = -65536;                                       // (stays negative: over-subscribed)
		if (cnt) max = L;
		offs += cnt;
		first = (first + cnt) << 1;
	}
	if (0 == lane) c.max = max;
	bgzf_sync();
	u32 const size(1u << root);
#pragma unroll 1
	for (u32 e(lane); e < size; e += 64) {
		u32 ent(0);
#pragma unroll 1
		for (u32 L(1); L <= root && L <= max; ++L) {
			u32 const i((__builtin_bitreverse32(e) >> (32 - L)) - c.first[L]);
			if (i < c.count[L]) { ent = (u32(sorted[c.offs[L] + i]) << 4) | L; break; }
		}
		table[e] = u16(ent);
	}
	bgzf_sync();
	if (0 == max) return !is_cl;                                               // no codes: every lookup of this code fails
	return 0 == left || (left > 0 && !is_cl && 1 == max);
}

// The symbol whose code starts the 15 bits `bits` (first bit = bit 0), its length in `len`; kInflateNoSymbol for none.
__device__ inline u32 inflate_decode(u32 bits, u16 const *table, u32 root, inflate_code const &c, u16 const *sorted, u32 &len)
{
	u32 const ent(inflate_uni(table[bits & ((1u << root) - 1)]));
	if (ent) { len = ent & 15; return ent >> 4; }
	u32 const mx(inflate_uni(c.max));
	if (mx <= root) return kInflateNoSymbol;
	u32 const rev(__builtin_bitreverse32(bits & 0x7fffu) >> 17);   // the 15 bits with the first one as the most significant
#pragma unroll 1
	for (u32 L(root + 1); L <= mx; ++L) {
		u32 const i((rev >> (15 - L)) - inflate_uni(c.first[L]));
		if (i < inflate_uni(c.count[L])) { len = L; return inflate_uni(sorted[inflate_uni(c.offs[L]) + i]); }
	}
	return kInflateNoSymbol;
}

// LSB-first bits of one member's payload.  words = the payload's address rounded down to 4 bytes, lead_bits = 8 * (address mod 4);
// words [0, n_words) cover the payload and lie inside the member (header before it, footer after it); reads past them give 0.
// Two 64-word windows in VGPRs: lane k holds words[base + k] and words[base + 64 + k].
struct inflate_bits {
	u32 const *words;
	u32 n_words, lead_bits;
	u64 bb;
	u32 nb, next, base;
	u32 cur, ahead;

	__device__ u32 load(u32 w) const { u32 const i(w + threadIdx.x); return i < n_words ? words[i] : 0u; }
	__device__ void refill()   // at least 33 bits in bb
	{
#pragma unroll 1
		while (nb <= 32) {
			if (next - base >= 64) { cur = ahead; base += 64; ahead = load(base + 64); }
			bb |= u64(inflate_uni(__builtin_amdgcn_readlane(cur, next - base))) << nb;
			nb += 32;
			++next;
		}
	}
	__device__ void seek(u32 byte)   // to payload byte `byte`
	{
		u32 const a(lead_bits / 8 + byte);
		next = base = a >> 2;
		cur = load(base);
		ahead = load(base + 64);
		bb = 0;
		nb = 0;
		refill();
		drop(8 * (a & 3));
	}
	__device__ u32 peek(u32 n) const { return u32(bb) & ((1u << n) - 1); }   // n <= 31
	__device__ void drop(u32 n) { bb >>= n; nb -= n; }
	__device__ u32 get(u32 n) { u32 const v(peek(n)); drop(n); return v; }
	__device__ u32 used() const { return 32 * next - nb - lead_bits; }        // payload bits consumed
};

// members: member m of the slice at in + in_offsets[m], in_offsets[m + 1] - in_offsets[m] bytes (framing checked by the host: v2m_bgzf_scan);
// its output to out + out_offsets[m], out_offsets[m + 1] - out_offsets[m] = ISIZE bytes (out 16-byte aligned); status[m] = kInflate*.
// A member that fails writes no output.
__global__ void __launch_bounds__(kInflateThreads) bgzf_inflate_kernel(unsigned char const *__restrict__ in, u64 const *__restrict__ in_offsets,
	u64 const *__restrict__ out_offsets, unsigned char *__restrict__ out, u32 *__restrict__ status)
{
	__shared__ inflate_lds s;
	V2M_POISON_LDS(s);
	u32 const lane(threadIdx.x), m(blockIdx.x);
	u64 const m0(in_offsets[m]), m1(in_offsets[m + 1]), o0(out_offsets[m]), o1(out_offsets[m + 1]);
	if (m1 - m0 < kBgzfHeaderBytes + kBgzfFooterBytes || m1 - m0 > kBgzfSlotBytes || o1 - o0 > kBgzfSlotBytes) {
		if (0 == lane) status[m] = kInflateBadFraming;
		return;
	}
	u32 const msize(u32(m1 - m0)), plen(msize - kBgzfHeaderBytes - kBgzfFooterBytes), isize(u32(o1 - o0)), pbits(8 * plen);
	unsigned char const *const mem(in + m0);
	unsigned char *const ob(s.out + (o0 & 15));   // ob[0, isize) fits: (o0 & 15) + 65536 <= sizeof(s.out)

	for (u32 i(lane); i < 256; i += 64) {
		u32 c(i);
		for (int b(0); b < 8; ++b) c = (c & 1) ? (c >> 1) ^ 0xEDB88320u : c >> 1;
		s.crc_table[i] = c;
	}

	inflate_bits br;
	{
		unsigned char const *const pay(mem + kBgzfHeaderBytes);
		u32 const lead(u32(reinterpret_cast<uintptr_t>(pay) & 3));
		br.words = reinterpret_cast<u32 const *>(pay - lead);   // (pointer arithmetic, not integers: the loads stay global ones)
		br.lead_bits = 8 * lead;
		br.n_words = (br.lead_bits / 8 + plen + 3) / 4;
		br.seek(0);
	}
	u32 st(kInflateOk), p(0);
	bool last(false), fixed_ready(false);
#pragma unroll 1
	while (kInflateOk == st && !last) {
		br.refill();
		u32 const hdr(br.get(3));
		last = hdr & 1;
		u32 const type(hdr >> 1);
		if (3 == type) { st = kInflateBadBlockType; break; }
		if (0 == type) {   // stored: to a byte boundary, LEN, NLEN, LEN bytes
			br.drop(br.nb & 7);
			br.refill();
			u32 const len(br.get(16)), nlen(br.get(16));
			if (br.used() > pbits) { st = kInflatePastPayload; break; }
			if (len != (~nlen & 0xffffu)) { st = kInflateStoredLengths; break; }
			u32 const pos(br.used() / 8);
			if (len > plen - pos) { st = kInflatePastPayload; break; }
			if (len > isize - p) { st = kInflateOutputTooLong; break; }
			for (u32 k(lane); k < len; k += 64) ob[p + k] = mem[kBgzfHeaderBytes + pos + k];
			p += len;
			br.seek(pos + len);
			continue;
		}
		if (1 == type) {   // fixed codes (RFC 1951 section 3.2.6), built once per member
			if (!fixed_ready) {
				for (u32 i(lane); i < 320; i += 64) s.lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
				bgzf_sync();
				(void) inflate_build(s.lens, 288, kInflateLitRoot, false, s.lit, s.lit_sorted, s.lit_table);
				(void) inflate_build(s.lens + 288, 32, kInflateDistRoot, false, s.dist, s.dist_sorted, s.dist_table);
				fixed_ready = true;
			}
		} else {           // dynamic codes (section 3.2.7)
			fixed_ready = false;
			br.refill();
			u32 const hlit(br.get(5) + 257), hdist(br.get(5) + 1), hclen(br.get(4) + 4);
			if (hlit > 286 || hdist > 30) { st = kInflateTooManySymbols; break; }
			if (lane < 20) s.cl_lens[lane] = 0;
			bgzf_sync();
#pragma unroll 1
			for (u32 i(0); i < hclen; ++i) {
				br.refill();
				u32 const v(br.get(3));
				if (0 == lane) s.cl_lens[kBgzfClOrder[i]] = v;
			}
			bgzf_sync();
			if (!inflate_build(s.cl_lens, 19, kInflateClRoot, true, s.cl, s.cl_sorted, s.cl_table)) { st = kInflateBadCodeLengthCode; break; }
			u32 const total(hlit + hdist);   // <= 316
			u32 n(0);
#pragma unroll 1
			while (n < total) {
				br.refill();
				u32 len(0);
				u32 const sym(inflate_decode(br.peek(15), s.cl_table, kInflateClRoot, s.cl, s.cl_sorted, len));
				if (kInflateNoSymbol == sym) { st = kInflateBadCodeLengthCode; break; }
				br.drop(len);
				if (sym < 16) {
					if (0 == lane) s.lens[n] = sym;
					++n;
					continue;
				}
				u32 rep, val(0);
				if (16 == sym) {
					if (0 == n) { st = kInflateBadRepeat; break; }
					val = inflate_uni(s.lens[n - 1]);
					rep = 3 + br.get(2);
				} else if (17 == sym) rep = 3 + br.get(3);
				else rep = 11 + br.get(7);
				if (rep > total - n) { st = kInflateBadRepeat; break; }
				for (u32 k(lane); k < rep; k += 64) s.lens[n + k] = val;
				n += rep;
			}
			if (kInflateOk != st) break;
			if (br.used() > pbits) { st = kInflatePastPayload; break; }
			bgzf_sync();
			if (0 == inflate_uni(s.lens[256])) { st = kInflateNoEndOfBlock; break; }
			if (!inflate_build(s.lens, hlit, kInflateLitRoot, false, s.lit, s.lit_sorted, s.lit_table)) { st = kInflateBadLitLenCode; break; }
			if (!inflate_build(s.lens + hlit, hdist, kInflateDistRoot, false, s.dist, s.dist_sorted, s.dist_table)) { st = kInflateBadDistCode; break; }
		}
#pragma unroll 1
		for (;;) {   // the block's symbols
			br.refill();
			u32 len(0);
			u32 const sym(inflate_decode(br.peek(15), s.lit_table, kInflateLitRoot, s.lit, s.lit_sorted, len));
			if (kInflateNoSymbol == sym || sym >= 286) { st = kInflateBadLitLenSymbol; break; }
			br.drop(len);
			if (sym < 256) {
				if (p >= isize) { st = kInflateOutputTooLong; break; }
				if (0 == lane) ob[p] = static_cast<unsigned char>(sym);
				++p;
			} else if (256 == sym) {
				break;
			} else {
				u32 const li(sym - 257);   // 0..28
				u32 const leb(li < 8 || 28 == li ? 0 : (li >> 2) - 1);
				u32 const mlen((li < 8 ? 3 + li : 28 == li ? 258 : ((4 + (li & 3)) << leb) + 3) + br.get(leb));
				br.refill();
				u32 dl(0);
				u32 const dsym(inflate_decode(br.peek(15), s.dist_table, kInflateDistRoot, s.dist, s.dist_sorted, dl));
				if (kInflateNoSymbol == dsym || dsym >= 30) { st = kInflateBadDistSymbol; break; }
				br.drop(dl);
				u32 const deb(dsym < 4 ? 0 : (dsym >> 1) - 1);
				u32 const dist((dsym < 4 ? 1 + dsym : ((2 + (dsym & 1)) << deb) + 1) + br.get(deb));
				if (br.used() > pbits) { st = kInflatePastPayload; break; }
				if (dist > p) { st = kInflateTooFarBack; break; }
				if (mlen > isize - p) { st = kInflateOutputTooLong; break; }
				if (dist >= 64) {   // a round's sources lie before p or in earlier rounds
#pragma unroll 1
					for (u32 k(lane); k < mlen; k += 64) ob[p + k] = ob[p - dist + k];
				} else {            // out[p + k] = out[p - dist + k mod dist]: every source lies before p
					u32 r(lane % dist);
					u32 const step(64 % dist);
#pragma unroll 1
					for (u32 k(lane); k < mlen; k += 64) {
						ob[p + k] = ob[p - dist + r];
						r += step;
						if (r >= dist) r -= dist;
					}
				}
				p += mlen;
			}
			if (br.used() > pbits) { st = kInflatePastPayload; break; }
		}
		if (kInflateOk == st && br.used() > pbits) st = kInflatePastPayload;
	}
	if (kInflateOk == st && p != isize) st = kInflateShortOutput;
	bgzf_sync();
	if (kInflateOk == st) {   // CRC-32 of ob[0, isize): a table CRC per lane over its 1 KiB, moved to the end and combined as in the encoder
		u32 const s0(min(lane * 1024u, isize)), s1(min(s0 + 1024u, isize));
		u32 crc(0);
#pragma unroll 1
		for (u32 i(s0); i < s1; ++i) crc = s.crc_table[(crc ^ ob[i]) & 255] ^ (crc >> 8);
		u32 x(s0 < s1 ? crc_shift(crc, isize - s1) : 0);
		for (int d(32); d; d >>= 1) x ^= __shfl_xor(x, d);
		unsigned char const *const f(mem + msize - kBgzfFooterBytes);
		u32 const want(u32(f[0]) | (u32(f[1]) << 8) | (u32(f[2]) << 16) | (u32(f[3]) << 24));
		if (inflate_uni(~(crc_shift(0xFFFFFFFFu, isize) ^ x)) != want) st = kInflateBadCrc;
	}
	if (0 == lane) status[m] = st;
	if (kInflateOk != st) return;
	unsigned char *const g(out + o0);
	u32 const head(min(isize, (16u - u32(o0 & 15)) & 15u));   // ob + head and g + head are both 16-byte aligned
	if (lane < head) g[lane] = ob[lane];
	u32 const n16((isize - head) / 16);
	for (u32 j(lane); j < n16; j += 64) reinterpret_cast<vec4u *>(g + head)[j] = reinterpret_cast<vec4u const *>(ob + head)[j];
	for (u32 i(head + 16 * n16 + lane); i < isize; i += 64) g[i] = ob[i];
}

} // namespace v2m
