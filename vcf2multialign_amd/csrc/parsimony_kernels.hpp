// Parsimony on a tree (v2m_parsimony_of_sites, v2m_tree_parsimony; include/v2m_hip.h "parsimony"): Fitch's two passes over the join
// records of a tree, per site of the variable-sites alignment, in integers.  Included by v2m_hip.hip behind bootstrap_kernels.hpp
// (kernels.hpp's zero_bytes_mask, wave_inclusive_scan_u32 and scan_tile_counts_kernel are used here).
//   fitch_up_kernel          the sets of the internal nodes, children first; per site the steps and the present classes; per
//                            workgroup the sum of its sites' steps, and the call's total
//   scan_tile_counts_kernel  (kernels.hpp) the workgroups' sums as one "row": each workgroup's offset into the mutation list
//   fitch_down_kernel<kEmit> the states, root first, written over the sets; per branch its changes; <true>: every mutation at
//                            offset[site] + its rank within the site, the order of the header with no sort and no atomics on the list
//
// A lane owns kFitchSites = 4 adjacent sites for the whole tree: one u32 of a leaf's row (u8[row][pitch], as gather_sites_kernel
// writes it) and one u32 of every node's set, a 4-bit mask per byte, so that a wave reads and writes 256 contiguous bytes per node.
// Every byte of a set is <= 0x0F: no carry of the byte-parallel arithmetic below crosses a byte.
//
// The one hazard.  A parent's read of sets[child] follows THE SAME LANE's store to that address some iterations earlier (in a
// caterpillar: the iteration before), and the down pass reads a node's state that the same lane stored when it visited the parent.
// That is program order within a thread and needs no barrier -- as long as `sets` is read and written through this one pointer, which
// is therefore not __restrict__, and both sides are plain loads and stores.  The leaves' rows are never written: they are
// __restrict__, and the rows of a batch of kFitchBatch records are read ahead of the joins that use them.
#pragma once

namespace v2m {

constexpr int kFitchThreads = 256;
constexpr int kFitchSites = 4;             // sites a lane owns (S): one u32 of a row or of a set
constexpr int kFitchBatch = 4;             // records whose leaf rows a lane has in flight

static_assert(kFitchSites == 4, "a lane's sites are the four bytes of one u32");

struct fitch_join { u32 a, b; };                          // the children of a record; the last record's third child is an argument
struct parsimony_site_record { u32 steps, present; };     // v2m_parsimony_site
struct tree_mutation_record { u32 site, node, from, to; };   // v2m_tree_mutation

// The sets of four leaf bytes: 1 << class for A, C, G, T (either case), 0x0F for every other byte and for the bytes outside `keep`
// (0xFF in the bytes of the lane's sites below n_sites).  `called`: 0x01 in the bytes that hold one of the four.
__device__ __forceinline__ u32 fitch_leaf_sets(u32 x, u32 keep, u32 &called)
{
	u32 const lower = x | 0x20202020u;
	u32 const a = zero_bytes_mask(lower ^ 0x61616161u) >> 7;
	u32 const c = zero_bytes_mask(lower ^ 0x63636363u) >> 7;
	u32 const g = zero_bytes_mask(lower ^ 0x67676767u) >> 7;
	u32 const t = zero_bytes_mask(lower ^ 0x74747474u) >> 7;
	called = (a | c | g | t) & keep;
	return ((a | c << 1 | g << 2 | t << 3) & keep) | (called ^ 0x01010101u) * 0x0Fu;
}

// 0x01 in every byte of x (bytes <= 0x0F) that is zero.
__device__ __forceinline__ u32 fitch_empty_bytes(u32 x)
{
	return ((x | x >> 1 | x >> 2 | x >> 3) & 0x01010101u) ^ 0x01010101u;
}

// The lowest set bit of every byte of x (bytes <= 0x0F; a zero byte stays zero): x & -x per byte, where -x is 0x10 - x.
__device__ __forceinline__ u32 fitch_lowest_bits(u32 x)
{
	return x & ((x ^ 0x0F0F0F0Fu) + 0x01010101u);
}

// Fitch's rule on four sites: the intersection, or where that is empty the union and a step (0x01 in `stepped`).
__device__ __forceinline__ u32 fitch_join_sets(u32 sa, u32 sb, u32 &stepped)
{
	u32 const both = sa & sb;
	stepped = fitch_empty_bytes(both);
	return both | ((sa | sb) & stepped * 0xFFu);
}

// The class 0 ... 3 of a one-hot byte 1, 2, 4 or 8.
__device__ __forceinline__ u32 fitch_class_of(u32 one_hot)
{
	return 31u - (u32) __builtin_clz(one_hot);
}

// blockIdx.x = kFitchThreads * kFitchSites sites.  bytes: u8[n][pitch], 4-byte aligned rows, pitch % 4 == 0 and pitch >= n_sites rounded
// up to 4; the bytes of a lane's word at or beyond n_sites are read and masked to "missing".  sets: u8[n - 2][pitch].  joins: n - 2
// records, children below n + t; last_c the third child of the last.  sites[n_sites], block_steps[gridDim.x]; *total is added to.
__global__ __launch_bounds__(kFitchThreads) void fitch_up_kernel(
	unsigned char const *__restrict__ bytes, unsigned char *sets, u64 pitch, u32 n, u64 n_sites,
	fitch_join const *__restrict__ joins, u32 last_c,
	parsimony_site_record *__restrict__ sites, u32 *__restrict__ block_steps, unsigned long long *__restrict__ total)
{
	__shared__ u32 wave_sums[kFitchThreads / 64];
	V2M_POISON_LDS(wave_sums);
	u64 const site = ((u64) blockIdx.x * kFitchThreads + threadIdx.x) * kFitchSites;
	bool const active = site < n_sites;
	u32 steps[4] = {0, 0, 0, 0};
	if (active) {
		u64 const left = n_sites - site;
		u32 const keep = left > 3 ? 0xFFFFFFFFu : left > 2 ? 0x00FFFFFFu : left > 1 ? 0x0000FFFFu : 0x000000FFu;
		u32 const n_records = n - 2;
		u32 present = 0;
		// the classes present: every leaf is a child exactly once, so the leaves met as children are all the leaves
		auto const leaf([&](u32 id, u32 &called) {
			u32 const s = fitch_leaf_sets(*(u32 const *) (bytes + (u64) id * pitch + site), keep, called);
			present |= s & called * 0x0Fu;
			return s;
		});
		auto const count([&](u32 stepped) {
#pragma unroll
			for (int k = 0; k < 4; ++k) steps[k] += stepped >> (8 * k) & 1u;
		});
		u32 x = 0;
		u32 t = 0;
		// batches of kFitchBatch records: the leaf rows of the batch are loaded first (nothing writes them), the internal sets only
		// in the iteration that uses them (an earlier iteration of this lane, perhaps of this batch, stored them)
		for (; t + kFitchBatch <= n_records; t += kFitchBatch) {
			fitch_join j[kFitchBatch];
			u32 sa[kFitchBatch], sb[kFitchBatch];
#pragma unroll
			for (int k = 0; k < kFitchBatch; ++k) {
				j[k] = joins[t + k];
				u32 called;
				sa[k] = j[k].a < n ? leaf(j[k].a, called) : 0u;
				sb[k] = j[k].b < n ? leaf(j[k].b, called) : 0u;
			}
#pragma unroll
			for (int k = 0; k < kFitchBatch; ++k) {
				if (j[k].a >= n) sa[k] = *(u32 const *) (sets + (u64) (j[k].a - n) * pitch + site);
				if (j[k].b >= n) sb[k] = *(u32 const *) (sets + (u64) (j[k].b - n) * pitch + site);
				u32 stepped;
				x = fitch_join_sets(sa[k], sb[k], stepped);
				count(stepped);
				if (t + k + 1 < n_records) *(u32 *) (sets + (u64) (t + k) * pitch + site) = x;
			}
		}
		for (; t < n_records; ++t) {
			fitch_join const j = joins[t];
			u32 called;
			u32 const sa = j.a < n ? leaf(j.a, called) : *(u32 const *) (sets + (u64) (j.a - n) * pitch + site);
			u32 const sb = j.b < n ? leaf(j.b, called) : *(u32 const *) (sets + (u64) (j.b - n) * pitch + site);
			u32 stepped;
			x = fitch_join_sets(sa, sb, stepped);
			count(stepped);
			if (t + 1 < n_records) *(u32 *) (sets + (u64) t * pitch + site) = x;
		}
		// the trifurcation: x is the last record's join of a and b
		{
			u32 called;
			u32 const sc = last_c < n ? leaf(last_c, called) : *(u32 const *) (sets + (u64) (last_c - n) * pitch + site);
			u32 const y = x & sc;
			u32 const stepped = fitch_empty_bytes(y);
			count(stepped);
			x = y | (x & stepped * 0xFFu);
			*(u32 *) (sets + (u64) (n_records - 1) * pitch + site) = x;
		}
#pragma unroll
		for (int k = 0; k < 4; ++k)
			if ((u64) k < left) sites[site + k] = parsimony_site_record{steps[k], present >> (8 * k) & 0x0Fu};
	}
	// the workgroup's steps (every lane takes part; sites at or beyond n_sites hold no step: their leaves are all missing)
	u32 mine = steps[0] + steps[1] + steps[2] + steps[3];
#pragma unroll
	for (int d = 32; d >= 1; d >>= 1) mine += __shfl_down(mine, d, kWave);
	if ((threadIdx.x & 63) == 0) wave_sums[threadIdx.x >> 6] = mine;
	__syncthreads();
	if (0 == threadIdx.x) {
		u32 sum = 0;
#pragma unroll
		for (int wv = 0; wv < kFitchThreads / 64; ++wv) sum += wave_sums[wv];
		block_steps[blockIdx.x] = sum;
		if (sum) atomicAdd(total, (unsigned long long) sum);
	}
}

// The same grid and lanes.  sets holds the up pass's sets and is left holding every internal node's one-hot state.  branch_changes[x],
// x < 2 n - 3, is added to (the caller zeroes it, or keeps what earlier site ranges left): one integer atomicAdd per wave and branch,
// only where non-zero.  kEmit: sites as the up pass wrote it and block_offsets, the scanned block_steps, give every site its place in
// mutations; site_base is added to the site indices written (the range's first site).
template <bool kEmit>
__global__ __launch_bounds__(kFitchThreads) void fitch_down_kernel(
	unsigned char const *__restrict__ bytes, unsigned char *sets, u64 pitch, u32 n, u64 n_sites,
	fitch_join const *__restrict__ joins, u32 last_c, u32 *__restrict__ branch_changes,
	parsimony_site_record const *__restrict__ sites, u32 const *__restrict__ block_offsets, u32 site_base,
	tree_mutation_record *__restrict__ mutations)
{
	__shared__ u32 wave_sums[kFitchThreads / 64];
	V2M_POISON_LDS(wave_sums);
	u64 const site = ((u64) blockIdx.x * kFitchThreads + threadIdx.x) * kFitchSites;
	bool const active = site < n_sites;
	u64 const left = active ? n_sites - site : 0;
	u32 const keep = left > 3 ? 0xFFFFFFFFu : left > 2 ? 0x00FFFFFFu : left > 1 ? 0x0000FFFFu : left > 0 ? 0x000000FFu : 0u;
	u32 next[4] = {0, 0, 0, 0};                  // kEmit: where the next mutation of each of the lane's sites goes
	if (kEmit) {
		u32 own[4] = {0, 0, 0, 0};
#pragma unroll
		for (int k = 0; k < 4; ++k) if ((u64) k < left) own[k] = sites[site + k].steps;
		u32 const mine = own[0] + own[1] + own[2] + own[3];
		u32 const incl = wave_inclusive_scan_u32(mine);
		if ((threadIdx.x & 63) == 63) wave_sums[threadIdx.x >> 6] = incl;
		asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
		__syncthreads();
		u32 rank = block_offsets[blockIdx.x] + incl - mine;
#pragma unroll
		for (int wv = 0; wv < kFitchThreads / 64; ++wv) if (wv < (int) (threadIdx.x >> 6)) rank += wave_sums[wv];
		next[0] = rank; next[1] = next[0] + own[0]; next[2] = next[1] + own[1]; next[3] = next[2] + own[2];
	}
	if (0 == __ballot(active)) return;           // (a wave without a site; behind the workgroup's one barrier)
	u32 const n_records = n - 2;
	// One branch: the child's state under its parent's, the branch's changes, and with kEmit the mutations.  Wave-uniform control:
	// every lane of the wave takes part in the ballots; a lane without a site loads and stores nothing, its words are all 0 and it has
	// nothing to count.
	auto const branch([&](u32 id, u32 parent_state) {
		bool const is_leaf = id < n;
		u32 set = 0;
		if (active) {
			u32 called;
			set = is_leaf ? fitch_leaf_sets(*(u32 const *) (bytes + (u64) id * pitch + site), keep, called) : *(u32 const *) (sets + (u64) (id - n) * pitch + site);
		}
		u32 const kept = set & parent_state;
		u32 const state = kept | (fitch_lowest_bits(set) & fitch_empty_bytes(kept) * 0xFFu);
		if (!is_leaf && active) *(u32 *) (sets + (u64) (id - n) * pitch + site) = state;
		u32 const changed = (fitch_empty_bytes(state ^ parent_state) ^ 0x01010101u) & keep;   // 0x01 where the states differ
		u32 changes = 0;
#pragma unroll
		for (int k = 0; k < 4; ++k) changes += (u32) __popcll(__ballot(changed >> (8 * k) & 1u));
		if ((threadIdx.x & 63) == 0 && changes) atomicAdd(&branch_changes[id], changes);
		if (kEmit && changed) {
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				if (changed >> (8 * k) & 1u)
					mutations[next[k]++] = tree_mutation_record{site_base + (u32) site + k, id,
						fitch_class_of(parent_state >> (8 * k) & 0xFFu), fitch_class_of(state >> (8 * k) & 0xFFu)};
			}
		}
	});
	// the root's state: the lowest bit of its set
	if (active) {
		unsigned char *const root = sets + (u64) (n_records - 1) * pitch + site;
		*(u32 *) root = fitch_lowest_bits(*(u32 const *) root);
	}
	for (u32 t = n_records; t-- > 0;) {
		fitch_join const j = joins[t];
		u32 const parent_state = active ? *(u32 const *) (sets + (u64) t * pitch + site) : 0u;   // (stored by this lane: at the root above, else at its parent's record)
		branch(j.a, parent_state);
		branch(j.b, parent_state);
		if (t + 1 == n_records) branch(last_c, parent_state);
	}
}

} // namespace v2m
