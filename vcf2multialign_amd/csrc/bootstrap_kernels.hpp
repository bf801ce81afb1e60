// Bootstrap of the pair distances (v2m_pair_distances_weighted, v2m_bootstrap_distances, v2m_nj_bootstrap; include/v2m_hip.h
// "bootstrap"): dist_w[i][j] = the sum over the columns c of the view of w[c] * differ(i, j, c).  Included by v2m_hip.hip behind
// distance_kernels.hpp, whose site list and bit planes it reads as they are: a column that is no site adds 0 whatever it weighs, so
// the weights are kept by SITE RANK, u32 w[V], and a replicate never touches the rows.
//   bootstrap_weights_kernel         the L draws of a replicate; a draw that lands on a site adds 1 to the site's weight
//   gather_site_weights_kernel       explicit weights: w[s] = weights[sites[s]]
//   weight_slices_kernel             w cut into 32 BIT SLICES laid out as a plane is: bit s % 64 of word s / 64 of slice b is bit b
//                                    of w[s]; and the OR of all weights, whose bit length is that of the largest: K
//   pair_distances_weighted_kernel   pair_distances_kernel with acc += sum over b < K of popcount(m & slice[b][word]) << b
#pragma once

namespace v2m {

constexpr int kBootDrawThreads = 256;     // bootstrap_weights_kernel: a lane a draw
constexpr int kBootGatherThreads = 256;   // gather_site_weights_kernel: a lane a site
constexpr int kBootSliceThreads = 256;    // weight_slices_kernel: a lane a site, a wave a site word
constexpr int kBootSlices = 32;           // slices stored per site word: the bits of a u32 weight

static_assert(kPairChunkWords * kBootSlices == kPairThreads, "a chunk's slice words are one load a lane");

// key = mix(seed + G); draw k of replicate r is mix(key + ((r << 32 | k) + 1) * G) and selects column floor(x * L / 2^64).
__host__ __device__ __forceinline__ u64 bootstrap_key(u64 seed) { return mix64(seed + kGolden); }
__host__ __device__ __forceinline__ u64 bootstrap_draw(u64 key, u32 replicate, u32 k) { return mix64(key + (((u64) replicate << 32 | k) + 1) * kGolden); }

// A lane a draw.  The column's rank in the ascending site list is found by bisection; a column that is no site is dropped.  The
// adds are integer, so w does not depend on their order.  w: zeroed before.
__global__ __launch_bounds__(kBootDrawThreads) void bootstrap_weights_kernel(
	u64 key, u32 replicate, u64 n_columns, u32 const *__restrict__ sites, u64 n_sites, u32 *__restrict__ w)
{
	u64 const k = (u64) blockIdx.x * kBootDrawThreads + threadIdx.x;
	if (k >= n_columns) return;
	u32 const column = (u32) __umul64hi(bootstrap_draw(key, replicate, (u32) k), n_columns);
	u64 lo = 0, hi = n_sites;   // the first site >= column lies in [lo, hi]
	while (lo < hi) {
		u64 const mid = (lo + hi) >> 1;
		if (sites[mid] < column) lo = mid + 1; else hi = mid;
	}
	if (lo < n_sites && sites[lo] == column) atomicAdd(w + lo, 1u);
}

__global__ __launch_bounds__(kBootGatherThreads) void gather_site_weights_kernel(
	u32 const *__restrict__ weights, u32 const *__restrict__ sites, u64 n_sites, u32 *__restrict__ w)
{
	u64 const s = (u64) blockIdx.x * kBootGatherThreads + threadIdx.x;
	if (s < n_sites) w[s] = weights[sites[s]];
}

// A wave a site word of the n_words the planes' chunks hold (sites at and beyond n_sites weigh 0: the padding stays zero): 32
// ballots, lane b keeps and stores slice b's word at slices[b * n_words + word].  any: the OR of every weight (zeroed before).
__global__ __launch_bounds__(kBootSliceThreads) void weight_slices_kernel(
	u32 const *__restrict__ w, u64 n_sites, u64 n_words, u64 *__restrict__ slices, u32 *__restrict__ any)
{
	int const lane = threadIdx.x & 63;
	u64 const site = (u64) blockIdx.x * kBootSliceThreads + threadIdx.x;
	u64 const word = site >> 6;
	if (word >= n_words) return;   // (the whole wave)
	u32 const mine = site < n_sites ? w[site] : 0u;
	u64 kept = 0;
	u32 seen = 0;
#pragma unroll
	for (int b = 0; b < kBootSlices; ++b) {
		u64 const ballot = __ballot((mine >> b) & 1u);
		if (lane == b) kept = ballot;
		seen |= (ballot ? 1u : 0u) << b;
	}
	if (lane < kBootSlices) slices[(u64) lane * n_words + word] = kept;
	if (0 == lane && seen) atomicOr(any, seen);
}

// pair_distances_kernel (distance_kernels.hpp) -- its grid, tiles, LDS image, prefetch, register block and stores -- with weights:
// slices are those of weight_slices_kernel for every site word of the call (n_words a slice), the pass's first word is word_base,
// and n_slices = K >= 1 of them are read.  A chunk's K * C slice words are fetched with the planes (lane t: word t / 32, slice t % 32)
// and lie in LDS as slice_words[word][slice]; every lane reads the same one at a time: a broadcast.  Per word a lane forms its 16
// masks m as the plain kernel does and then, slice by slice, adds popcount(m & slice) << b.  No entry overflows: the weights of the
// view sum to less than 2^32.
template <bool kAcgtOnly>
__global__ __launch_bounds__(kPairThreads) void pair_distances_weighted_kernel(
	u64 const *__restrict__ planes, u64 n_pad, u32 n_chunks, u32 chunks_per_part, u32 n_tiles, u32 n_rows,
	u64 const *__restrict__ slices, u64 n_words, u64 word_base, u32 n_slices,
	u32 *__restrict__ dist, u64 dist_pitch, u32 use_atomics)
{
	constexpr int kSide = kPairChunkWords * 3 * kPairTile;      // words of one side's chunk
	constexpr int kLoads = kSide / kPairThreads;                // a lane's loads per side and chunk
	static_assert(kSide % kPairThreads == 0, "whole loads");
	__shared__ __attribute__((aligned(16))) u64 side_i[kSide];
	__shared__ __attribute__((aligned(16))) u64 side_j[kSide];
	__shared__ __attribute__((aligned(16))) u64 slice_words[kPairChunkWords * kBootSlices];
	V2M_POISON_LDS(side_i);
	V2M_POISON_LDS(side_j);
	V2M_POISON_LDS(slice_words);
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
	// the lane's slice word of a chunk: slice t % 32 of the chunk's word t / 32; slices at and beyond n_slices are never read
	bool const slice_live = (u32) (t & (kBootSlices - 1)) < n_slices;
	u64 const *const src_w = slices + (u64) (t & (kBootSlices - 1)) * n_words + word_base + (t / kBootSlices);

	u32 acc[kPairBlock][kPairBlock] = {};
	u64 next_i[kLoads], next_j[kLoads], next_w = 0;
	auto const fetch = [&](u32 chunk) {
		u64 const first = (u64) chunk * kPairChunkWords * 3 + (t >> 6);   // (word, plane) of the lane's first load, as one index
#pragma unroll
		for (int k = 0; k < kLoads; ++k) {
			next_i[k] = src_i[(first + 4 * k) * n_pad];
			next_j[k] = src_j[(first + 4 * k) * n_pad];
		}
		if (slice_live) next_w = src_w[(u64) chunk * kPairChunkWords];
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
		if (slice_live) slice_words[t] = next_w;
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
		__syncthreads();
		if (chunk + 1 < chunk_end) fetch(chunk + 1);
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
			u64 m[kPairBlock][kPairBlock];
#pragma unroll
			for (int r = 0; r < kPairBlock; ++r) {
#pragma unroll
				for (int c = 0; c < kPairBlock; ++c) {
					m[r][c] = (a[0][r] ^ b[0][c]) | (a[1][r] ^ b[1][c]);
					if constexpr (kAcgtOnly) m[r][c] &= ~(a[2][r] | b[2][c]);
					else m[r][c] |= a[2][r] ^ b[2][c];
				}
			}
			for (u32 s = 0; s < n_slices; ++s) {
				u64 const weight = slice_words[w * kBootSlices + s];
#pragma unroll
				for (int r = 0; r < kPairBlock; ++r) {
#pragma unroll
					for (int c = 0; c < kPairBlock; ++c) acc[r][c] += (u32) __popcll(m[r][c] & weight) << s;
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
