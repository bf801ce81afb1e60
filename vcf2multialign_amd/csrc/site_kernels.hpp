// Variable sites (v2m_variable_sites[_device], include/v2m_hip.h "variable sites"): the rows of a batch cut down to the selected columns
// of the view, byte for byte.  Included by v2m_hip.hip behind distance_kernels.hpp, whose emit_site_columns_kernel lists the VARIABLE
// columns (flags 0); the SNP selection (V2M_SITES_SNP) has its own count and emit kernel here, on the same blocks of kSelectColumns
// columns and the same block offsets, so that scan_tile_counts_kernel serves both:
//   count_snp_columns_kernel   the columns of every block where at least two of the classes A, C, G, T have a non-zero count
//   emit_snp_columns_kernel    the selection again; a selected column's view-relative index goes to its rank: the site list, u32[V]
//   gather_sites_kernel        a slice's spliced rows, read at the sites, go to out[row][site] as they are
//
// The site list is allocated up to (V + 3) & ~3 entries: a lane of the gather reads its four sites' columns with one 16-byte load, and
// the entries from V on are never written and never used.
#pragma once

namespace v2m {

constexpr int kGatherThreads = 256;
constexpr int kGatherSites = 4;            // sites a lane owns (S): one 16-byte load of the site list, one 4-byte store per row
constexpr int kGatherMinGroupRows = 16;    // the host gives a row group at least this many rows (pack_sites_kernel's rule)

static_assert(kGatherSites == 4, "a lane's sites are one vec4u of the site list and one u32 of a row");

// At least two of the four classes A, C, G, T hold a row of the column (snp-sites' rule): decided from the counts alone.
__device__ __forceinline__ bool column_is_snp(u32 const *__restrict__ counts, u64 plane_pitch, u64 column)
{
	u32 present = 0;
#pragma unroll
	for (int k = 0; k < 4; ++k) present += counts[(u64) k * plane_pitch + column] ? 1u : 0u;
	return present >= 2;
}

// As count_variable_columns_kernel over the whole view, with the SNP predicate.
__global__ __launch_bounds__(kSelectColumns) void count_snp_columns_kernel(
	u32 const *__restrict__ counts, u64 plane_pitch, u64 n_columns, u32 *__restrict__ block_counts)
{
	__shared__ u32 wave_sums[kSelectColumns / 64];
	V2M_POISON_LDS(wave_sums);
	int const t = threadIdx.x;
	u64 const column = (u64) blockIdx.x * kSelectColumns + t;
	u32 mine = column < n_columns && column_is_snp(counts, plane_pitch, column) ? 1u : 0u;
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

// As emit_site_columns_kernel, with the SNP predicate.
__global__ __launch_bounds__(kSelectColumns) void emit_snp_columns_kernel(
	u32 const *__restrict__ counts, u64 plane_pitch, u64 n_columns, u32 const *__restrict__ block_offsets, u32 *__restrict__ sites, u64 capacity)
{
	__shared__ u32 wave_sums[kSelectColumns / 64];
	V2M_POISON_LDS(wave_sums);
	int const t = threadIdx.x, lane = t & 63, wave = t >> 6;
	u64 const column = (u64) blockIdx.x * kSelectColumns + t;
	u32 const mine = column < n_columns && column_is_snp(counts, plane_pitch, column) ? 1u : 0u;
	u32 const incl = wave_inclusive_scan_u32(mine);
	if (lane == 63) wave_sums[wave] = incl;
	asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
	__syncthreads();
	u64 rank = (u64) block_offsets[blockIdx.x] + incl - mine;
#pragma unroll
	for (int wv = 0; wv < kSelectColumns / 64; ++wv) if (wv < wave) rank += wave_sums[wv];
	if (mine && rank < capacity) sites[rank] = (u32) column;
}

// blockIdx.x = kGatherThreads * kGatherSites sites (a lane: sites 4 i .. 4 i + 3 of lane i of the grid's x), blockIdx.y = a group of
// rows_per_group rows of the slice.  A lane reads its four columns with one 16-byte load of the site list, then per row of its group
// the four bytes at those columns, and stores them as one u32 at out[(row_base + r) * out_pitch + site]: a wave stores 256 contiguous
// bytes per row.  Rows are unrolled by four: 16 byte loads in flight per lane.
// Sites at or beyond n_sites contribute a 0 byte: their lane takes the column of its first site for them (that one is always below
// n_sites, see below), so that every load of the lane is within the row, and masks the byte away.  A lane whose first site is at or
// beyond (n_sites + 3) & ~3 does nothing; for the others first site <= ((n_sites + 3) & ~3) - 4 < n_sites.
// rows: the slice's spliced rows (row r at rows + r * row_pitch, every site's column below row_pitch); sites: the list, readable up to
// (n_sites + 3) & ~3 entries, 16-byte aligned; out: 4-byte aligned with out_pitch % 4 == 0 and out_pitch >= (n_sites + 3) & ~3.
__global__ __launch_bounds__(kGatherThreads) void gather_sites_kernel(
	char const *__restrict__ rows, u64 row_pitch, u32 n_rows, u32 rows_per_group, u64 row_base,
	u32 const *__restrict__ sites, u64 n_sites, char *__restrict__ out, u64 out_pitch)
{
	u64 const site = ((u64) blockIdx.x * kGatherThreads + threadIdx.x) * kGatherSites;
	if (site >= ((n_sites + 3) & ~(u64) 3)) return;
	vec4u const listed = *(vec4u const *) (sites + site);
	u64 const left = n_sites - site;                   // >= 1
	u64 const c0 = listed.x, c1 = left > 1 ? listed.y : c0, c2 = left > 2 ? listed.z : c0, c3 = left > 3 ? listed.w : c0;
	u32 const keep = left > 3 ? 0xFFFFFFFFu : left > 2 ? 0x00FFFFFFu : left > 1 ? 0x0000FFFFu : 0x000000FFu;
	u32 const row_begin = blockIdx.y * rows_per_group;
	u32 const row_end = n_rows - row_begin < rows_per_group ? n_rows : row_begin + rows_per_group;
	unsigned char const *const src = (unsigned char const *) rows;
	char *const dst = out + row_base * out_pitch + site;
	u32 r = row_begin;
	for (; r + 4 <= row_end; r += 4) {
		u32 word[4];
#pragma unroll
		for (int k = 0; k < 4; ++k) {
			unsigned char const *const row = src + (u64) (r + k) * row_pitch;
			word[k] = (u32) row[c0] | (u32) row[c1] << 8 | (u32) row[c2] << 16 | (u32) row[c3] << 24;
		}
#pragma unroll
		for (int k = 0; k < 4; ++k) *(u32 *) (dst + (u64) (r + k) * out_pitch) = word[k] & keep;
	}
	for (; r < row_end; ++r) {
		unsigned char const *const row = src + (u64) r * row_pitch;
		u32 const word = (u32) row[c0] | (u32) row[c1] << 8 | (u32) row[c2] << 16 | (u32) row[c3] << 24;
		*(u32 *) (dst + (u64) r * out_pitch) = word & keep;
	}
}

} // namespace v2m
