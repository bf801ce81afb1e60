// Pair distances (v2m_pair_distances[_device], include/v2m_hip.h "pair distances"): for every two rows of a batch the number of
// columns of the view where their classes differ.  Included by v2m_hip.hip behind kernels.hpp, whose column counts name the classes.
//
// A column where one of the seven classes holds every row adds 0 to every pair under both definitions, so only the variable columns
// -- the SITES, which the column counts' selection finds -- are looked at:
//   emit_site_columns_kernel   the selection of count_variable_columns_kernel + scan_tile_counts_kernel again; a selected column's
//                              view-relative index goes to its rank: the site list, u32[V], ascending
//   pack_sites_kernel          a slice's spliced rows, gathered at the sites and classified into 3-bit codes (A, C, G, T = 0-3: bit 2
//                              clear; N = 4, gap = 5, other = 6), go into three BIT PLANES: bit s % 64 of word s / 64 of plane p of row r
//                              is bit p of the code row r holds at site s
//   pair_distances_kernel      XOR + popcount over the planes of a tile of rows i x rows j
//
// Layout of the planes, chosen for the pair kernel's loads: u64 planes[word][plane][row], row < n_pad (the rows rounded up to kPairTile).
// The words of a pass are a contiguous range; the kPairTile rows of a tile are 512 contiguous bytes per (word, plane), which a wave
// reads with one coalesced load and writes to LDS as they are (the LDS image of a chunk is that layout cut to the tile's rows), and
// pack_sites_kernel's waves write neighbouring rows of a word next to each other.  The host zeroes the planes of a pass before it
// packs: site slots from V up to the padded end, and rows from n_rows up to n_pad, hold code 0 in every row and add 0.
#pragma once

namespace v2m {

constexpr int kPairTile = 64;          // rows per side of a workgroup's tile (T)
constexpr int kPairChunkWords = 8;     // 64-bit site words per LDS chunk (C): a chunk is 64 * C sites
constexpr int kPairThreads = 256;
constexpr int kPairBlock = 4;          // a lane's block of pair accumulators is kPairBlock x kPairBlock
constexpr int kPackThreads = 256;      // pack_sites_kernel: a lane a site, a wave a site word

static_assert(kPairTile * kPairTile == kPairThreads * kPairBlock * kPairBlock, "a tile is the lanes' blocks");
static_assert(kPairTile == kWave, "a (word, plane) of a tile is one wave's load");
static_assert(kPairBlock == 4 && kPairTile == 64, "pair_row() spreads 16 lanes x 4 rows over a tile");

// The 3-bit code of an aligned byte: the class of the column counts' rule.
__device__ __forceinline__ u32 site_code(u32 b)
{
	u32 const lower = b | 0x20u;
	return lower == 'a' ? 0u : lower == 'c' ? 1u : lower == 'g' ? 2u : lower == 't' ? 3u : lower == 'n' ? 4u : b == '-' ? 5u : 6u;
}

// The site list: as emit_column_counts_kernel with variable_only, but the record is the column's index in the view.
__global__ __launch_bounds__(kSelectColumns) void emit_site_columns_kernel(
	u32 const *__restrict__ counts, u64 plane_pitch, u64 n_columns, u32 n_rows, u32 const *__restrict__ block_offsets, u32 *__restrict__ sites, u64 capacity)
{
	__shared__ u32 wave_sums[kSelectColumns / 64];
	V2M_POISON_LDS(wave_sums);
	int const t = threadIdx.x, lane = t & 63, wave = t >> 6;
	u64 const column = (u64) blockIdx.x * kSelectColumns + t;
	u32 c[kCountClasses] = {};
	u32 const mine = column < n_columns && column_selected(counts, plane_pitch, column, n_rows, 1u, c) ? 1u : 0u;
	u32 const incl = wave_inclusive_scan_u32(mine);
	if (lane == 63) wave_sums[wave] = incl;
	asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
	__syncthreads();
	u64 rank = (u64) block_offsets[blockIdx.x] + incl - mine;
#pragma unroll
	for (int wv = 0; wv < kSelectColumns / 64; ++wv) if (wv < wave) rank += wave_sums[wv];
	if (mine && rank < capacity) sites[rank] = (u32) column;
}

// blockIdx.x = kPackThreads sites of the pass (a wave: the 64 sites of word blockIdx.x * 4 + wave), blockIdx.y = a group of
// rows_per_group rows of the slice.  A lane reads its site's column once and then the byte of every row of its group there; the wave's
// three ballots are the row's word of each plane, stored by lanes 0-2.  Sites at or beyond site_end take code 0 and read nothing.
// rows: the slice's spliced rows (row r at rows + r * row_pitch); row_base: the batch row of the slice's first; planes: those of the
// pass, whose first word is site_begin / 64.
__global__ __launch_bounds__(kPackThreads) void pack_sites_kernel(
	char const *__restrict__ rows, u64 row_pitch, u32 n_rows, u32 rows_per_group, u32 row_base,
	u32 const *__restrict__ sites, u64 site_begin, u64 site_end, u64 *__restrict__ planes, u64 n_pad)
{
	int const lane = threadIdx.x & 63;
	u64 const site = site_begin + (u64) blockIdx.x * kPackThreads + threadIdx.x;
	u64 const word = ((u64) blockIdx.x * kPackThreads + threadIdx.x) >> 6;
	bool const live = site < site_end;
	u64 const column = live ? sites[site] : 0;
	u32 const row_begin = blockIdx.y * rows_per_group;
	u32 const row_end = n_rows - row_begin < rows_per_group ? n_rows : row_begin + rows_per_group;
	char const *const base = rows + column;
	u64 *const dst = planes + (word * 3 + (lane < 3 ? lane : 0)) * n_pad + row_base;
	u32 r = row_begin;
	for (; r + 4 <= row_end; r += 4) {
		u32 code[4];
#pragma unroll
		for (int k = 0; k < 4; ++k) code[k] = live ? site_code((unsigned char) base[(u64) (r + k) * row_pitch]) : 0u;
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			u64 const b0 = __ballot(code[k] & 1u), b1 = __ballot(code[k] & 2u), b2 = __ballot(code[k] & 4u);
			if (lane < 3) dst[r + k] = lane == 0 ? b0 : lane == 1 ? b1 : b2;
		}
	}
	for (; r < row_end; ++r) {
		u32 const code = live ? site_code((unsigned char) base[(u64) r * row_pitch]) : 0u;
		u64 const b0 = __ballot(code & 1u), b1 = __ballot(code & 2u), b2 = __ballot(code & 4u);
		if (lane < 3) dst[r] = lane == 0 ? b0 : lane == 1 ? b1 : b2;
	}
}

typedef u64 vec2ul __attribute__((ext_vector_type(2)));   // two neighbouring rows' words: one 16-byte LDS read

// Row k < kPairBlock of lane coordinate u < 16 within a tile.
__device__ __forceinline__ int pair_row(int u, int k) { return 2 * u + (k & 1) + 32 * (k >> 1); }

// blockIdx.x = a tile pair (ti <= tj) of the upper triangle, numbered row by row; blockIdx.z = a part of the pass's chunks
// (chunks_per_part each; the last may hold fewer).  Lane t, with ty = t / 16 and tx = t % 16, owns the pairs of rows
// ti * T + pair_row(ty, r) and tj * T + pair_row(tx, c) (r, c < 4), pair_row(u, k) = 2 u + (k & 1) + 32 (k >> 1): two neighbouring rows
// twice, so that a lane reads its rows of a (word, plane) with two 16-byte LDS reads, and the 16 lanes that an LDS cycle serves
// together read 256 contiguous bytes of the j side (all 64 banks once) while the i side's reads are broadcasts.  (Rows interleaved
// by 16 and read 8 bytes at a time, which the compiler pairs into ds_read2_b64, measured the same: the LDS reads do not bound the
// loop)  Per chunk the two sides' words, [C][3][T] each, go from the planes to LDS as they lie
// (6 coalesced 8-byte loads a lane and side, fetched into registers while the previous chunk is computed); per word a lane then
// reads its 2 x 12 words and adds the 16 popcounts.
// The sums go to dist[i][j] and dist[j][i] (a diagonal tile computes both itself and stores only [i][j]): with plain stores, or --
// use_atomics: the launch has several parts or the call several passes, on a matrix zeroed before -- with atomicAdd, exact in any order.
// Rows at and beyond n_rows are never stored.
template <bool kAcgtOnly>
__global__ __launch_bounds__(kPairThreads) void pair_distances_kernel(
	u64 const *__restrict__ planes, u64 n_pad, u32 n_chunks, u32 chunks_per_part, u32 n_tiles, u32 n_rows,
	u32 *__restrict__ dist, u64 dist_pitch, u32 use_atomics)
{
	constexpr int kSide = kPairChunkWords * 3 * kPairTile;      // words of one side's chunk
	constexpr int kLoads = kSide / kPairThreads;                // a lane's loads per side and chunk
	static_assert(kSide % kPairThreads == 0, "whole loads");
	__shared__ __attribute__((aligned(16))) u64 side_i[kSide];
	__shared__ __attribute__((aligned(16))) u64 side_j[kSide];
	V2M_POISON_LDS(side_i);
	V2M_POISON_LDS(side_j);
	int const t = threadIdx.x, ty = t >> 4, tx = t & 15;

	// the tile pair: row ti of the triangle begins at ti * n_tiles - ti * (ti - 1) / 2
	u32 const p = blockIdx.x;
	u32 ti = (u32) (((float) (2 * n_tiles + 1) - sqrtf((float) (2 * n_tiles + 1) * (float) (2 * n_tiles + 1) - 8.0f * (float) p)) * 0.5f);
	if (ti >= n_tiles) ti = n_tiles - 1;
	while (ti > 0 && ti * n_tiles - ti * (ti - 1) / 2 > p) --ti;
	while (ti + 1 < n_tiles && (ti + 1) * n_tiles - (ti + 1) * ti / 2 <= p) ++ti;
	u32 const tj = ti + (p - (ti * n_tiles - ti * (ti - 1) / 2));

	u32 const chunk_begin = blockIdx.z * chunks_per_part;
	u32 const chunk_end = n_chunks - chunk_begin < chunks_per_part ? n_chunks : chunk_begin + chunks_per_part;
	u64 const *const src_i = planes + (u64) ti * kPairTile + (t & 63);
	u64 const *const src_j = planes + (u64) tj * kPairTile + (t & 63);

	u32 acc[kPairBlock][kPairBlock] = {};
	u64 next_i[kLoads], next_j[kLoads];
	auto const fetch = [&](u32 chunk) {
		u64 const first = (u64) chunk * kPairChunkWords * 3 + (t >> 6);   // (word, plane) of the lane's first load, as one index
#pragma unroll
		for (int k = 0; k < kLoads; ++k) {
			next_i[k] = src_i[(first + 4 * k) * n_pad];
			next_j[k] = src_j[(first + 4 * k) * n_pad];
		}
	};
	if (chunk_begin < chunk_end) fetch(chunk_begin);
	for (u32 chunk = chunk_begin; chunk < chunk_end; ++chunk) {
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (the previous chunk's reads are done in every wave before it is overwritten)
		__syncthreads();
#pragma unroll
		for (int k = 0; k < kLoads; ++k) {
			side_i[t + kPairThreads * k] = next_i[k];
			side_j[t + kPairThreads * k] = next_j[k];
		}
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
		__syncthreads();
		if (chunk + 1 < chunk_end) fetch(chunk + 1);
#pragma unroll 2
		for (int w = 0; w < kPairChunkWords; ++w) {
			u64 a[3][kPairBlock], b[3][kPairBlock];
#pragma unroll
			for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
				for (int h = 0; h < kPairBlock / 2; ++h) {
					vec2ul const va = *(vec2ul const *) &side_i[(w * 3 + pl) * kPairTile + pair_row(ty, 2 * h)];
					vec2ul const vb = *(vec2ul const *) &side_j[(w * 3 + pl) * kPairTile + pair_row(tx, 2 * h)];
					a[pl][2 * h] = va.x; a[pl][2 * h + 1] = va.y;
					b[pl][2 * h] = vb.x; b[pl][2 * h + 1] = vb.y;
				}
			}
#pragma unroll
			for (int r = 0; r < kPairBlock; ++r) {
#pragma unroll
				for (int c = 0; c < kPairBlock; ++c) {
					u64 m = (a[0][r] ^ b[0][c]) | (a[1][r] ^ b[1][c]);
					if constexpr (kAcgtOnly) m &= ~(a[2][r] | b[2][c]);
					else m |= a[2][r] ^ b[2][c];
					acc[r][c] += (u32) __popcll(m);
				}
			}
		}
	}

	bool const diagonal = ti == tj;
#pragma unroll
	for (int r = 0; r < kPairBlock; ++r) {
		u32 const i = ti * kPairTile + pair_row(ty, r);
		if (i >= n_rows) continue;
#pragma unroll
		for (int c = 0; c < kPairBlock; ++c) {
			u32 const j = tj * kPairTile + pair_row(tx, c);
			if (j >= n_rows) continue;
			u32 *const upper = dist + (u64) i * dist_pitch + j;
			u32 *const lower = dist + (u64) j * dist_pitch + i;
			if (use_atomics) {
				if (acc[r][c]) {
					atomicAdd(upper, acc[r][c]);
					if (!diagonal) atomicAdd(lower, acc[r][c]);
				}
			}
			else {
				*upper = acc[r][c];
				if (!diagonal) *lower = acc[r][c];
			}
		}
	}
}

} // namespace v2m
