// Window diversity (v2m_diversity_of_counts, v2m_window_diversity; include/v2m_hip.h "window diversity"): the counts table of the
// column counts summed over arbitrary bins of columns, and the folded site frequency spectrum.  Included by v2m_hip.hip behind
// parsimony_kernels.hpp.
//   diversity_init_kernel           every record: its `columns`, and 0 in every field the reduction adds to
//   diversity_bins_kernel<kBetween> a segmented sum over the bins, in integers, and (within form) the histogram
//
// A lane takes kDiversityLane = 4 adjacent columns: one 16-byte load per plane A, C, G, T (planes 4 and 5 are never read), a wave
// 1 KiB of every plane, a workgroup a tile of kDiversityColumns columns of the table.  A column outside [bounds[0], bounds[n_bins])
// is loaded where the table has it (elements below (L + 3) & ~3) and ignored.
//
// What a column adds is four u64: the sums diffs, pairs and complete_diffs, and the four counts (called, segregating, complete,
// complete_segregating) packed 16 bits each -- a workgroup holds kDiversityColumns = 1024 columns, so no count of a tile passes
// 2^16 and the four travel through the shuffles as one word.  They are unpacked only where an atomic is issued.
//
// Sums that share a bin meet on chip before any atomic:
//   * a tile that lies in one bin (bins wider than a tile: the common case) is a plain workgroup reduction, wave shuffles and one
//     word per wave and field through LDS, and one set of atomics per workgroup;
//   * otherwise a lane cuts its columns into runs of one bin.  A run strictly inside the lane is the whole of its bin in this wave
//     (bins are intervals and the lanes' columns ascend) and goes out at once.  A lane's first run, where the lane has more than one,
//     is handed to the lane before when that lane ends in the same bin, and goes out itself when not -- the bin then begins at this
//     lane.  The lanes' last runs have ascending bins along the wave and are summed by a segmented shuffle reduction; the first lane
//     of each segment issues the atomics.  So a bin and field receives at most one atomic per wave.
// Integer adds commute: the records have one value whatever the order.  No float anywhere.
//
// The histogram (within form): a complete column adds 1 at 0 (one letter) or at the smaller of its two counts, or to *multiallelic.
// sfs_mode 1: through kDiversitySfsLdsBins u32 counters in LDS (the spectrum's n / 2 + 1 entries fit), flushed by u64 atomics where
// non-zero; sfs_mode 2: straight to global atomics; 0: no histogram.
#pragma once

namespace v2m {

constexpr int kDiversityThreads = 256;
constexpr int kDiversityLane = 4;                 // columns a lane takes: one vec4u per plane
constexpr int kDiversityColumns = 1024;           // a workgroup's tile
constexpr int kDiversitySfsLdsBins = 4096;        // 16 KiB of u32 counters: spectra of up to 8 190 rows stay on chip

static_assert(kDiversityColumns == kDiversityThreads * kDiversityLane, "a tile is its lanes' columns");
static_assert(kDiversityColumns <= 65535, "a tile's counts travel as 16-bit fields of one word");

struct diversity_bin_record { u64 columns, called, diffs, pairs, segregating, complete, complete_segregating, complete_diffs; };   // v2m_diversity_bin
struct diversity_between_record { u64 columns, called, diffs, pairs; };                                                          // v2m_diversity_between_bin

// packed counts: called, segregating << 16, complete << 32, complete_segregating << 48
struct diversity_sums {
	u64 counts, diffs, pairs, complete_diffs;
	__device__ __forceinline__ void add(diversity_sums const &o) { counts += o.counts; diffs += o.diffs; pairs += o.pairs; complete_diffs += o.complete_diffs; }
	__device__ __forceinline__ bool any() const { return 0 != (counts | pairs); }   // (diffs > 0 needs called; complete needs called, or is no column's)
};

__device__ __forceinline__ u64 diversity_shfl_down(u64 v, int d)
{
	return (u64) __shfl_down((unsigned long long) v, d, kWave);
}

template <bool kBetween>
__device__ __forceinline__ diversity_sums diversity_shfl_down(diversity_sums const &s, int d)
{
	diversity_sums r;
	r.counts = diversity_shfl_down(s.counts, d);
	r.diffs = diversity_shfl_down(s.diffs, d);
	r.pairs = diversity_shfl_down(s.pairs, d);
	r.complete_diffs = kBetween ? 0 : diversity_shfl_down(s.complete_diffs, d);
	return r;
}

// One record's share of the sums, where non-zero.
template <bool kBetween>
__device__ __forceinline__ void diversity_flush(u64 *__restrict__ records, u32 bin, diversity_sums const &s)
{
	typedef unsigned long long ull;
	if (kBetween) {
		ull *const r = (ull *) (records + (u64) bin * 4);
		if (s.counts & 0xFFFFu) atomicAdd(r + 1, (ull) (s.counts & 0xFFFFu));
		if (s.diffs) atomicAdd(r + 2, (ull) s.diffs);
		if (s.pairs) atomicAdd(r + 3, (ull) s.pairs);
	} else {
		ull *const r = (ull *) (records + (u64) bin * 8);
		if (s.counts & 0xFFFFu) atomicAdd(r + 1, (ull) (s.counts & 0xFFFFu));
		if (s.diffs) atomicAdd(r + 2, (ull) s.diffs);
		if (s.pairs) atomicAdd(r + 3, (ull) s.pairs);
		if (s.counts >> 16 & 0xFFFFu) atomicAdd(r + 4, (ull) (s.counts >> 16 & 0xFFFFu));
		if (s.counts >> 32 & 0xFFFFu) atomicAdd(r + 5, (ull) (s.counts >> 32 & 0xFFFFu));
		if (s.counts >> 48) atomicAdd(r + 6, (ull) (s.counts >> 48));
		if (s.complete_diffs) atomicAdd(r + 7, (ull) s.complete_diffs);
	}
}

// The bin of column c among bins [lo, n_bins): the last k with bounds[k] <= c.  bounds[lo] <= c < bounds[n_bins].
__device__ __forceinline__ u32 diversity_bin_of(u64 const *__restrict__ bounds, u32 lo, u32 n_bins, u64 c)
{
	u32 hi = n_bins;                    // bounds[lo] <= c < bounds[hi]
	while (hi - lo > 1) {
		u32 const mid = lo + (hi - lo) / 2;
		if (bounds[mid] <= c) lo = mid; else hi = mid;
	}
	return lo;
}

// Record k of n_bins: columns = bounds[k + 1] - bounds[k], every other field 0.
template <bool kBetween>
__global__ __launch_bounds__(256) void diversity_init_kernel(u64 const *__restrict__ bounds, u32 n_bins, u64 *__restrict__ records)
{
	u32 const k = blockIdx.x * 256 + threadIdx.x;
	if (k >= n_bins) return;
	constexpr int kWords = kBetween ? 4 : 8;
	u64 *const r = records + (u64) k * kWords;
	r[0] = bounds[k + 1] - bounds[k];
#pragma unroll
	for (int f = 1; f < kWords; ++f) r[f] = 0;
}

// blockIdx.x + first_tile = the tile.  counts_a (and counts_b, kBetween): u32[6][plane_pitch], 16-byte aligned, plane_pitch % 4 == 0
// and >= (L + 3) & ~3 where L >= bounds[n_bins].  bounds: u64[n_bins + 1], ascending, n_bins >= 1, bounds[0] < bounds[n_bins] (the
// caller launches nothing otherwise); the grid covers the tiles of [bounds[0], bounds[n_bins]).  records: as diversity_init_kernel left
// them.  sfs (u64[n_a / 2 + 1], zeroed) and multiallelic (u64, zeroed): within form, sfs_mode != 0.
template <bool kBetween>
__global__ __launch_bounds__(kDiversityThreads) void diversity_bins_kernel(
	u32 const *__restrict__ counts_a, u32 const *__restrict__ counts_b, u64 plane_pitch,
	u64 const *__restrict__ bounds, u32 n_bins, u32 first_tile, u32 n_a, u32 n_b,
	u64 *__restrict__ records, u64 *__restrict__ sfs, u64 *__restrict__ multiallelic, u32 sfs_mode)
{
	typedef unsigned long long ull;
	(void) n_b;                        // (the between form's sums need no row count: it is the caller's limit check)
	__shared__ u64 wave_sums[kDiversityThreads / 64][4];
	__shared__ u32 histogram[kBetween ? 1 : kDiversitySfsLdsBins];
	V2M_POISON_LDS(wave_sums);
	V2M_POISON_LDS(histogram);

	u32 const t = threadIdx.x, lane = t & 63u, wave = t >> 6;
	u64 const begin = bounds[0], end = bounds[n_bins];
	u64 const tile_begin = ((u64) first_tile + blockIdx.x) * kDiversityColumns;
	u64 const lo_col = tile_begin > begin ? tile_begin : begin;                                              // the tile's columns that count:
	u64 const hi_col = tile_begin + kDiversityColumns < end ? tile_begin + kDiversityColumns : end;         // [lo_col, hi_col), not empty
	u64 const c0 = tile_begin + (u64) t * kDiversityLane;
	u32 const sfs_len = n_a / 2 + 1;

	if (!kBetween && 1 == sfs_mode) {
		for (u32 i = t; i < sfs_len; i += kDiversityThreads) histogram[i] = 0;
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
		__syncthreads();
	}

	// the lane's columns: what each adds, and which of them count
	diversity_sums col[kDiversityLane];
	bool counts_here[kDiversityLane];
	u32 many = 0;                      // complete columns of three or four letters
	{
		bool const load = c0 < hi_col && c0 + kDiversityLane > lo_col;   // (then c0 < (L + 3) & ~3: the 16 bytes are the table's)
		vec4u a = {0, 0, 0, 0}, c = a, g = a, tt = a, a2 = a, cc2 = a, g2 = a, t2 = a;
		if (load) {
			a = *(vec4u const *) (counts_a + c0);
			c = *(vec4u const *) (counts_a + plane_pitch + c0);
			g = *(vec4u const *) (counts_a + 2 * plane_pitch + c0);
			tt = *(vec4u const *) (counts_a + 3 * plane_pitch + c0);
			if (kBetween) {
				a2 = *(vec4u const *) (counts_b + c0);
				cc2 = *(vec4u const *) (counts_b + plane_pitch + c0);
				g2 = *(vec4u const *) (counts_b + 2 * plane_pitch + c0);
				t2 = *(vec4u const *) (counts_b + 3 * plane_pitch + c0);
			}
		}
#pragma unroll
		for (int j = 0; j < kDiversityLane; ++j) {
			u64 const column = c0 + j;
			bool const here = column >= lo_col && column < hi_col;
			counts_here[j] = here;
			diversity_sums s = {0, 0, 0, 0};
			if (here) {
				u64 const A = a[j], C = c[j], G = g[j], T = tt[j];
				u64 const m = A + C + G + T;
				if (kBetween) {
					u64 const A2 = a2[j], C2 = cc2[j], G2 = g2[j], T2 = t2[j];
					u64 const m2 = A2 + C2 + G2 + T2;
					s.pairs = m * m2;
					s.diffs = s.pairs - (A * A2 + C * C2 + G * G2 + T * T2);
					s.counts = (m >= 1 && m2 >= 1) ? 1 : 0;
				} else {
					u64 const diffs = A * C + A * G + A * T + C * G + C * T + G * T;
					u32 const letters = (A ? 1u : 0u) + (C ? 1u : 0u) + (G ? 1u : 0u) + (T ? 1u : 0u);
					bool const called = m >= 2, segregating = letters >= 2, complete = m == n_a && n_a >= 2;
					s.diffs = diffs;
					s.pairs = m * (m - (m ? 1 : 0)) / 2;
					s.complete_diffs = complete ? diffs : 0;
					s.counts = (called ? 1ull : 0ull) | (segregating ? 1ull << 16 : 0ull) | (complete ? 1ull << 32 : 0ull) | (complete && segregating ? 1ull << 48 : 0ull);
					if (sfs_mode && complete) {
						if (letters >= 3) ++many;
						else {
							// one letter: 0; two: the smaller count, which is m minus the largest
							u64 const top = max(max(A, C), max(G, T));
							u32 const at = 1 == letters ? 0u : (u32) min(top, m - top);
							if (1 == sfs_mode) atomicAdd(&histogram[at], 1u);
							else atomicAdd((ull *) sfs + at, 1ull);
						}
					}
				}
			}
			col[j] = s;
		}
	}

	// the bin of the tile's first column that counts, and where that bin ends
	u32 const k0 = diversity_bin_of(bounds, 0, n_bins, lo_col);
	u64 const k0_end = bounds[k0 + 1];

	if (k0_end >= hi_col) {
		// the whole tile lies in bin k0: a plain workgroup reduction
		diversity_sums mine = col[0];
#pragma unroll
		for (int j = 1; j < kDiversityLane; ++j) mine.add(col[j]);
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) mine.add(diversity_shfl_down<kBetween>(mine, d));
		if (0 == lane) { wave_sums[wave][0] = mine.counts; wave_sums[wave][1] = mine.diffs; wave_sums[wave][2] = mine.pairs; wave_sums[wave][3] = mine.complete_diffs; }
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
		__syncthreads();
		if (0 == t) {
			diversity_sums sum = {0, 0, 0, 0};
#pragma unroll
			for (int wv = 0; wv < kDiversityThreads / 64; ++wv) sum.add(diversity_sums{wave_sums[wv][0], wave_sums[wv][1], wave_sums[wv][2], wave_sums[wv][3]});
			diversity_flush<kBetween>(records, k0, sum);
		}
	} else {
		// runs of one bin within the lane
		constexpr u32 kNone = 0xFFFFFFFFu;
		u32 first_bin = kNone, last_bin = kNone;      // of the lane's first run where it has several, and of its last
		diversity_sums first = {0, 0, 0, 0}, run = {0, 0, 0, 0};
		u64 run_end = 0;                                // where last_bin ends
#pragma unroll
		for (int j = 0; j < kDiversityLane; ++j) {
			if (!counts_here[j]) continue;
			u64 const column = c0 + j;
			if (kNone == last_bin) {
				last_bin = diversity_bin_of(bounds, k0, n_bins, column);
				run_end = bounds[last_bin + 1];
			} else if (column >= run_end) {
				if (kNone == first_bin) { first_bin = last_bin; first = run; }
				else if (run.any()) diversity_flush<kBetween>(records, last_bin, run);   // strictly inside the lane: the bin's whole share
				run = diversity_sums{0, 0, 0, 0};
				last_bin = diversity_bin_of(bounds, last_bin + 1, n_bins, column);
				run_end = bounds[last_bin + 1];
			}
			run.add(col[j]);
		}
		// a first run goes to the lane before, where that lane ends in its bin
		{
			diversity_sums const next_first = diversity_shfl_down<kBetween>(first, 1);
			u32 const next_first_bin = (u32) __shfl_down(first_bin, 1, kWave);
			u32 const prev_last_bin = (u32) __shfl_up(last_bin, 1, kWave);
			if (lane < 63 && kNone != next_first_bin && next_first_bin == last_bin) run.add(next_first);
			if (kNone != first_bin && !(lane > 0 && prev_last_bin == first_bin) && first.any()) diversity_flush<kBetween>(records, first_bin, first);
		}
		// the last runs: ascending bins along the wave, equal bins adjacent
#pragma unroll
		for (int d = 1; d <= 32; d <<= 1) {
			diversity_sums const other = diversity_shfl_down<kBetween>(run, d);
			u32 const other_bin = (u32) __shfl_down(last_bin, d, kWave);
			if (lane + d < 64 && other_bin == last_bin) run.add(other);
		}
		u32 const prev_bin = (u32) __shfl_up(last_bin, 1, kWave);
		if (kNone != last_bin && (0 == lane || prev_bin != last_bin) && run.any()) diversity_flush<kBetween>(records, last_bin, run);
	}

	if (!kBetween && sfs_mode) {
#pragma unroll
		for (int d = 32; d >= 1; d >>= 1) many += __shfl_down(many, d, kWave);
		if (0 == lane && many) atomicAdd((ull *) multiallelic, (ull) many);
		if (1 == sfs_mode) {
			asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
			__syncthreads();
			for (u32 i = t; i < sfs_len; i += kDiversityThreads) {
				u32 const v = histogram[i];
				if (v) atomicAdd((ull *) sfs + i, (ull) v);
			}
		}
	}
}

} // namespace v2m
