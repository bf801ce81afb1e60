// Site LD (v2m_site_ld[_device], include/v2m_hip.h "site LD"): for pairs of nearby biallelic sites of the view the four integer counts
// r^2 is made of, and the pairs whose r^2 reaches a threshold.  Included by v2m_hip.hip behind site_kernels.hpp.
//
// A column is a SITE when exactly two of the classes A, C, G, T have a non-zero count and both counts reach min_allele_count; lo < hi
// are those classes.  At a site a row is CALLED when its class is lo or hi and CARRIES when it is hi.
//   count_ld_columns_kernel    the sites of every block of kSelectColumns columns (scan_tile_counts_kernel makes the block offsets)
//   emit_ld_columns_kernel     the selection again; a site's view-relative column goes to its rank in the site list, u32[V], and its
//                              24-byte record (absolute column, the two classes, their counts) to the same rank
//   ld_pack_kernel             a slice's spliced rows, read at the sites, go into two BIT PLANES by site over rows: bit r % 64 of word
//                              r / 64 of plane 0 (called) or 1 (carries) of site s
//   ld_pairs_kernel            AND + popcount over the planes of a tile of sites i x sites j of the band; <false> counts the reported
//                              pairs of every (site i, tile), <true> computes the tile again and writes them at their ranks
//
// Layout of the planes, section 8.9's with rows and sites exchanged: u64 planes[row word][plane][site], site < v_pad (the sites rounded
// up to kLdTile).  The kLdTile sites of a tile are 512 contiguous bytes per (row word, plane): one coalesced load of a wave, written to
// LDS as they lie.  The host zeroes the planes before it packs; sites from V up to v_pad stay 0: no row is called there, so every
// pair with one of them has den = 0 and is never reported.
#pragma once

namespace v2m {

constexpr int kLdTile = 64;            // sites per side of a workgroup's tile (T)
constexpr int kLdChunkWords = 8;       // 64-row words per LDS chunk (C): a chunk is 64 * C rows
constexpr int kLdThreads = 256;
constexpr int kLdBlock = 4;            // a lane's block of pairs is kLdBlock x kLdBlock, four accumulators each
constexpr int kLdPackThreads = 256;    // ld_pack_kernel: a lane a site

static_assert(kLdTile * kLdTile == kLdThreads * kLdBlock * kLdBlock, "a tile is the lanes' blocks");
static_assert(kLdTile == kWave, "a (row word, plane) of a tile is one wave's load, and a site's mask of the tile one u64");
static_assert(kLdBlock == kPairBlock && kLdTile == kPairTile, "pair_row() of distance_kernels.hpp spreads the lanes' blocks over the tile");

struct ld_site_record { u64 column; u32 class_lo, class_hi, count_lo, count_hi; };    // v2m_ld_site
struct ld_pair_record { u32 site_a, site_b, n, n_a, n_b, n_ab; };                     // v2m_ld_pair
static_assert(sizeof(ld_site_record) == 24 && sizeof(ld_pair_record) == 24, "the header's records");

// Exactly two of the four classes A, C, G, T hold rows of the column, and each at least min_count of them: decided from the counts alone.
__device__ __forceinline__ bool column_is_ld_site(u32 const *__restrict__ counts, u64 plane_pitch, u64 column, u32 min_count, u32 (&cls)[2], u32 (&cnt)[2])
{
	u32 present = 0;
	cls[0] = cls[1] = 0; cnt[0] = cnt[1] = 0;
#pragma unroll
	for (int k = 0; k < 4; ++k) {
		u32 const c = counts[(u64) k * plane_pitch + column];
		if (c) {
			if (present < 2) { cls[present] = (u32) k; cnt[present] = c; }
			++present;
		}
	}
	return present == 2 && cnt[0] >= min_count && cnt[1] >= min_count;
}

// As count_snp_columns_kernel, with the site predicate.
__global__ __launch_bounds__(kSelectColumns) void count_ld_columns_kernel(
	u32 const *__restrict__ counts, u64 plane_pitch, u64 n_columns, u32 min_count, u32 *__restrict__ block_counts)
{
	__shared__ u32 wave_sums[kSelectColumns / 64];
	V2M_POISON_LDS(wave_sums);
	int const t = threadIdx.x;
	u64 const column = (u64) blockIdx.x * kSelectColumns + t;
	u32 cls[2], cnt[2];
	u32 mine = column < n_columns && column_is_ld_site(counts, plane_pitch, column, min_count, cls, cnt) ? 1u : 0u;
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) mine += __shfl_down(mine, d, kWave);
	if ((t & 63) == 0) wave_sums[t >> 6] = mine;
	__syncthreads();
	if (0 == t) {
		u32 total = 0;
#pragma unroll
		for (int wv = 0; wv < kSelectColumns / 64; ++wv) total += wave_sums[wv];
		block_counts[blockIdx.x] = total;
	}
}

// As emit_snp_columns_kernel, with the site predicate; the record of the site goes to the same rank.  column_base: the view's first
// column (the record's column is absolute).
__global__ __launch_bounds__(kSelectColumns) void emit_ld_columns_kernel(
	u32 const *__restrict__ counts, u64 plane_pitch, u64 n_columns, u32 min_count, u64 column_base, u32 const *__restrict__ block_offsets,
	u32 *__restrict__ sites, ld_site_record *__restrict__ records, u64 capacity)
{
	__shared__ u32 wave_sums[kSelectColumns / 64];
	V2M_POISON_LDS(wave_sums);
	int const t = threadIdx.x, lane = t & 63, wave = t >> 6;
	u64 const column = (u64) blockIdx.x * kSelectColumns + t;
	u32 cls[2], cnt[2];
	u32 const mine = column < n_columns && column_is_ld_site(counts, plane_pitch, column, min_count, cls, cnt) ? 1u : 0u;
	u32 const incl = wave_inclusive_scan_u32(mine);
	if (lane == 63) wave_sums[wave] = incl;
	asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
	__syncthreads();
	u64 rank = (u64) block_offsets[blockIdx.x] + incl - mine;
#pragma unroll
	for (int wv = 0; wv < kSelectColumns / 64; ++wv) if (wv < wave) rank += wave_sums[wv];
	if (mine && rank < capacity) {
		sites[rank] = (u32) column;
		records[rank] = ld_site_record{column_base + column, cls[0], cls[1], cnt[0], cnt[1]};
	}
}

// blockIdx.x = kLdPackThreads sites (a lane a site), blockIdx.y = a group of words_per_group 64-row words of the BATCH, counted from the
// word of the slice's first row: the groups of a launch are word-aligned, so that a (word, site) belongs to one lane of the launch and
// its two plane words are ORed in with a plain load and store, no atomics.  A word that two slices share is ORed by two launches,
// which the stream orders.  A lane reads its column and its two classes once, then the byte of every row of its words.
// rows: the slice's spliced rows (row r of the slice at rows + r * row_pitch); row_base: the batch row of the slice's first.
__global__ __launch_bounds__(kLdPackThreads) void ld_pack_kernel(
	char const *__restrict__ rows, u64 row_pitch, u32 n_rows, u32 words_per_group, u32 row_base,
	u32 const *__restrict__ sites, ld_site_record const *__restrict__ records, u64 n_sites, u64 *__restrict__ planes, u64 v_pad)
{
	u64 const site = (u64) blockIdx.x * kLdPackThreads + threadIdx.x;
	if (site >= n_sites) return;
	u32 const lo = records[site].class_lo, hi = records[site].class_hi;
	unsigned char const *const base = (unsigned char const *) rows + sites[site];
	u32 const row_end = row_base + n_rows;
	u32 const word_begin = row_base / 64 + blockIdx.y * words_per_group;
	u32 const word_last = (row_end - 1) / 64;      // n_rows >= 1
	u32 const word_end = word_last + 1 - word_begin < words_per_group ? word_last + 1 : word_begin + words_per_group;
	for (u32 w = word_begin; w < word_end; ++w) {
		u32 const r_begin = w * 64 < row_base ? row_base : w * 64;
		u32 const r_end = (w + 1) * 64 > row_end ? row_end : (w + 1) * 64;
		u64 called = 0, carries = 0;
		u32 r = r_begin;
		for (; r + 4 <= r_end; r += 4) {
			u32 code[4];
#pragma unroll
			for (int k = 0; k < 4; ++k) code[k] = site_code(base[(u64) (r + k - row_base) * row_pitch]);
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				u64 const bit = (u64) 1 << ((r + k) & 63);
				if (code[k] == lo || code[k] == hi) called |= bit;
				if (code[k] == hi) carries |= bit;
			}
		}
		for (; r < r_end; ++r) {
			u32 const code = site_code(base[(u64) (r - row_base) * row_pitch]);
			u64 const bit = (u64) 1 << (r & 63);
			if (code == lo || code == hi) called |= bit;
			if (code == hi) carries |= bit;
		}
		u64 *const dst = planes + (u64) w * 2 * v_pad + site;
		if (called) dst[0] |= called;
		if (carries) dst[v_pad] |= carries;
	}
}

// The pair (n, n_a, n_b, n_ab) is reported: den != 0 and D^2 * r2_den >= r2_num * den, both products 128 bits wide.
// n <= 32 768: n * n_ab and n_a * n_b are below 2^31, D^2 at most 2^60 and den at most 2^56; r2_num <= r2_den <= 10^6 < 2^20.
__device__ __forceinline__ bool ld_reported(u32 n, u32 n_a, u32 n_b, u32 n_ab, u32 r2_num, u32 r2_den)
{
	u64 const den = (u64) n_a * (n - n_a) * ((u64) n_b * (n - n_b));
	if (0 == den) return false;
	long long const d = (long long) ((u64) n * n_ab) - (long long) ((u64) n_a * n_b);
	u64 const d2 = (u64) (d * d);
	u64 const left_hi = __umul64hi(d2, (u64) r2_den), left_lo = d2 * (u64) r2_den;
	u64 const right_hi = __umul64hi(den, (u64) r2_num), right_lo = den * (u64) r2_num;
	return left_hi > right_hi || (left_hi == right_hi && left_lo >= right_lo);
}

// blockIdx.x = a strip ti of kLdTile sites (strip_first + blockIdx.x), blockIdx.y = b: the tile of sites i of strip ti x sites j of
// strip tj = ti + b, b < n_blocks = the tiles of a strip that the band of window_sites reaches.  Lane t, with ty = t / 16 and
// tx = t % 16, owns the pairs of sites ti * T + pair_row(ty, r) and tj * T + pair_row(tx, c) (r, c < 4), as pair_distances_kernel's
// lanes own rows.  Per chunk the two sides' words, [C][2][T] each, go from the planes to LDS as they lie (4 coalesced 8-byte loads a
// lane and side, fetched into registers while the previous chunk is computed; words at and beyond n_words are taken as 0 and not
// read); per row word a lane reads its 2 x 8 words and adds the 64 popcounts of the 16 pairs' four ANDs.
// Then every lane decides its pairs -- s < t < n_sites, t - s <= window_sites, the column distance within window_columns unless that
// is 0, ld_reported() -- and ORs them into the tile's 64 masks in LDS, one u64 per site i, bit j_local.
//   kEmit = false: cells[(ti * T + i_local) * n_blocks + b] = popcount(mask[i_local]), every cell of the launch written.
//   kEmit = true:  cells hold the exclusive prefix sums of those counts per strip (scan_tile_counts_kernel over the strip's T * n_blocks
//                  cells; the flattening (i_local, b) is the order (s, t)), strip_totals the strips' sums and strip_bases their
//                  exclusive prefix sums over all strips.  A tile none of whose cells counted a pair returns before it loads anything;
//                  the others compute again, and a reported pair goes to
//                  out[strip_bases[ti] - out_base + cells[i_local][b] + popcount(mask[i_local] & below(j_local))].
template <bool kEmit>
__global__ __launch_bounds__(kLdThreads) void ld_pairs_kernel(
	u64 const *__restrict__ planes, u64 v_pad, u32 n_words, u32 const *__restrict__ sites, u64 n_sites,
	u32 window_sites, u64 window_columns, u32 r2_num, u32 r2_den, u32 strip_first, u32 n_strips, u32 n_blocks,
	u32 *__restrict__ cells, u64 const *__restrict__ strip_totals, u64 const *__restrict__ strip_bases, u64 out_base, ld_pair_record *__restrict__ out)
{
	constexpr int kSide = kLdChunkWords * 2 * kLdTile;        // words of one side's chunk
	constexpr int kLoads = kSide / kLdThreads;                // a lane's loads per side and chunk
	static_assert(kSide % kLdThreads == 0, "whole loads");
	__shared__ __attribute__((aligned(16))) u64 side_i[kSide];
	__shared__ __attribute__((aligned(16))) u64 side_j[kSide];
	__shared__ u64 mask[kLdTile];
	__shared__ u32 tile_live;
	V2M_POISON_LDS(side_i);
	V2M_POISON_LDS(side_j);
	V2M_POISON_LDS(mask);
	V2M_POISON_LDS(tile_live);
	int const t = threadIdx.x, ty = t >> 4, tx = t & 15;
	u32 const ti = strip_first + blockIdx.x, b = blockIdx.y, tj = ti + b;
	u64 const cell = ((u64) ti * kLdTile + (t & 63)) * n_blocks + b;      // of lanes 0-63: site i_local = t

	if (tj >= n_strips) {                                                 // beyond the last strip: no pair
		if (!kEmit && t < kLdTile) cells[cell] = 0;
		return;
	}
	if constexpr (kEmit) {
		if (t < kLdTile) {
			u32 const prefix = cells[cell];
			bool const last = (u32) t == kLdTile - 1 && b == n_blocks - 1;
			u32 const next = last ? (u32) strip_totals[ti] : cells[cell + 1];
			u64 const any = __ballot(next != prefix);
			if (0 == t) tile_live = any ? 1u : 0u;
		}
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
		__syncthreads();
		if (!tile_live) return;
	}

	u64 const *const src_i = planes + (u64) ti * kLdTile + (t & 63);
	u64 const *const src_j = planes + (u64) tj * kLdTile + (t & 63);
	u32 const n_chunks = (n_words + kLdChunkWords - 1) / kLdChunkWords;
	u64 const n_flat = (u64) n_words * 2;                                 // (word, plane) pairs that exist

	u32 acc_n[kLdBlock][kLdBlock] = {}, acc_a[kLdBlock][kLdBlock] = {}, acc_b[kLdBlock][kLdBlock] = {}, acc_ab[kLdBlock][kLdBlock] = {};
	u64 next_i[kLoads], next_j[kLoads];
	auto const fetch = [&](u32 chunk) {
		u64 const first = (u64) chunk * kLdChunkWords * 2 + (t >> 6);     // (word, plane) of the lane's first load, as one index
#pragma unroll
		for (int k = 0; k < kLoads; ++k) {
			u64 const flat = first + 4 * k;
			next_i[k] = flat < n_flat ? src_i[flat * v_pad] : 0;
			next_j[k] = flat < n_flat ? src_j[flat * v_pad] : 0;
		}
	};
	if (n_chunks) fetch(0);
	for (u32 chunk = 0; chunk < n_chunks; ++chunk) {
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // (the previous chunk's reads are done in every wave before it is overwritten)
		__syncthreads();
#pragma unroll
		for (int k = 0; k < kLoads; ++k) {
			side_i[t + kLdThreads * k] = next_i[k];
			side_j[t + kLdThreads * k] = next_j[k];
		}
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
		__syncthreads();
		if (chunk + 1 < n_chunks) fetch(chunk + 1);
#pragma unroll 2
		for (int w = 0; w < kLdChunkWords; ++w) {
			u64 a[2][kLdBlock], c[2][kLdBlock];               // [plane: called, carries][site of the block]
#pragma unroll
			for (int pl = 0; pl < 2; ++pl) {
#pragma unroll
				for (int h = 0; h < kLdBlock / 2; ++h) {
					vec2ul const va = *(vec2ul const *) &side_i[(w * 2 + pl) * kLdTile + pair_row(ty, 2 * h)];
					vec2ul const vc = *(vec2ul const *) &side_j[(w * 2 + pl) * kLdTile + pair_row(tx, 2 * h)];
					a[pl][2 * h] = va.x; a[pl][2 * h + 1] = va.y;
					c[pl][2 * h] = vc.x; c[pl][2 * h + 1] = vc.y;
				}
			}
#pragma unroll
			for (int r = 0; r < kLdBlock; ++r) {
#pragma unroll
				for (int q = 0; q < kLdBlock; ++q) {
					acc_n[r][q] += (u32) __popcll(a[0][r] & c[0][q]);
					acc_a[r][q] += (u32) __popcll(a[1][r] & c[0][q]);
					acc_b[r][q] += (u32) __popcll(a[0][r] & c[1][q]);
					acc_ab[r][q] += (u32) __popcll(a[1][r] & c[1][q]);
				}
			}
		}
	}

	// the masks of the tile
	if (t < kLdTile) mask[t] = 0;
	asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
	__syncthreads();
	u32 mine = 0;                                             // bit r * 4 + q: the pair is reported
#pragma unroll
	for (int r = 0; r < kLdBlock; ++r) {
		u64 const s = (u64) ti * kLdTile + pair_row(ty, r);
		u64 bits = 0;
#pragma unroll
		for (int q = 0; q < kLdBlock; ++q) {
			u64 const u = (u64) tj * kLdTile + pair_row(tx, q);
			bool ok = s < u && u < n_sites && u - s <= window_sites;
			if (ok && window_columns) ok = (u64) (sites[u] - sites[s]) <= window_columns;
			if (ok && ld_reported(acc_n[r][q], acc_a[r][q], acc_b[r][q], acc_ab[r][q], r2_num, r2_den)) {
				bits |= (u64) 1 << pair_row(tx, q);
				mine |= 1u << (r * kLdBlock + q);
			}
		}
		if (bits) atomicOr((unsigned long long *) &mask[pair_row(ty, r)], (unsigned long long) bits);   // (LDS)
	}
	asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
	__syncthreads();
	if constexpr (!kEmit) {
		if (t < kLdTile) cells[cell] = (u32) __popcll(mask[t]);
	}
	else {
		if (!mine) return;
		u64 const strip_at = strip_bases[ti] - out_base;
#pragma unroll
		for (int r = 0; r < kLdBlock; ++r) {
			int const il = pair_row(ty, r);
			if (!(mine >> (r * kLdBlock) & 0xFu)) continue;
			u64 const row_mask = mask[il];
			u64 const row_at = strip_at + cells[((u64) ti * kLdTile + il) * n_blocks + b];
#pragma unroll
			for (int q = 0; q < kLdBlock; ++q) {
				if (!(mine >> (r * kLdBlock + q) & 1u)) continue;
				int const jl = pair_row(tx, q);
				u64 const at = row_at + (u64) __popcll(row_mask & (((u64) 1 << jl) - 1));
				out[at] = ld_pair_record{(u32) (ti * kLdTile + il), (u32) (tj * kLdTile + jl), acc_n[r][q], acc_a[r][q], acc_b[r][q], acc_ab[r][q]};
			}
		}
	}
}

} // namespace v2m
