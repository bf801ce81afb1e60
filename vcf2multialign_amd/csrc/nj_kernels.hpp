// Neighbour joining (v2m_nj_tree[_of_distances], include/v2m_hip.h "neighbour joining"): the canonical NJ tree of n taxa from the
// upper triangle of a u32 distance matrix, in IEEE binary64 with every operation rounded on its own.  Included by v2m_hip.hip behind
// ld_kernels.hpp.
//
// The r live taxa lie DENSE in slots 0 ... r - 1 of
//   D     double[n][pitch]   the working matrix, symmetric, zero diagonal; pitch is n rounded up to even, so that a row begins at a
//                            16-byte boundary
//   R     double[pitch]      R(slot), the row sums as the header's recurrences carry them
//   ids   u32[pitch]         the node id a slot holds: ties are broken by id, never by slot
// and a join takes three kernels' work, queued in stream order by the host, which knows r = n - t and sizes every grid:
//   nj_init_kernel     (once) the u32 triangle into D, R (sums of exact integers: any order) and ids
//   nj_rowmin_kernel   a wave a row i < r - 1: the best (Q, lower id, higher id) over the slots j > i (Q and the key are symmetric, so
//                      the upper triangle of the slots holds every pair once), 16-byte reads of the row, of R and of ids
//   nj_join_kernel     one workgroup: the best of the r - 1 row minima is the step's pair; the record; D(u, .) and the R updates.  The
//                      new node u takes the lower of the two slots and the last live slot moves into the other: their ids go along
//   nj_last_kernel     (once) the trifurcation of the three taxa left
// No kernel waits for another: a launch's results reach the next through the stream's order alone.
//
// Every function that does the header's arithmetic holds `#pragma clang fp contract(off)`: at -O3 hipcc otherwise fuses Q's product
// and difference into v_fma_f64, which rounds once where the definition rounds twice (tests/test_nj_kernel_isa.py).
#pragma once

namespace v2m {

constexpr int kNjRowsPerGroup = 8;                            // rows (waves) per workgroup of nj_rowmin_kernel (W)
constexpr int kNjJoinThreads = 256;                           // nj_join_kernel's one workgroup (B)
constexpr int kNjRowminThreads = kNjRowsPerGroup * kWave;
constexpr int kNjInitThreads = 256;
constexpr int kNjJoinBatch = 4;                               // taxa a lane of nj_join_kernel has in flight
constexpr u32 kNjNone = 0xFFFFFFFFu;                          // V2M_NJ_NONE

typedef double vec2d __attribute__((ext_vector_type(2)));
typedef u32 vec2u __attribute__((ext_vector_type(2)));

// A row's (or a lane's, or a wave's) best pair: Q, the two ids, and the slots i < j that hold them (in either order).
struct nj_best {
	double q;
	u32 lo, hi, i, j;
};
static_assert(sizeof(nj_best) == 24, "nj_best is 24 bytes");

// The three-key order: smaller Q, then smaller lower id, then smaller higher id.  A total order on distinct pairs, so a minimum does
// not depend on the order in which candidates meet.
__device__ __forceinline__ bool nj_better(double q, u32 lo, u32 hi, nj_best const &b)
{
	return q < b.q || (q == b.q && (lo < b.lo || (lo == b.lo && hi < b.hi)));
}

__device__ __forceinline__ nj_best nj_nothing()
{
	nj_best b;
	b.q = __builtin_huge_val(); b.lo = kNjNone; b.hi = kNjNone; b.i = 0; b.j = 0;
	return b;
}

// The best over the wave's lanes, in every lane.
__device__ __forceinline__ nj_best nj_wave_best(nj_best b)
{
#pragma unroll
	for (int step = 1; step < kWave; step <<= 1) {
		nj_best o;
		o.q = __shfl_xor(b.q, step); o.lo = __shfl_xor(b.lo, step); o.hi = __shfl_xor(b.hi, step); o.i = __shfl_xor(b.i, step); o.j = __shfl_xor(b.j, step);
		if (nj_better(o.q, o.lo, o.hi, b)) b = o;
	}
	return b;
}

// blockIdx.x = row i of the n.  D[i][j] = (double) dist[min(i, j)][max(i, j)] for j != i and 0 on the diagonal and in the padding
// column; R[i] = their sum (integers below 2^53: exact in any order); ids[i] = i.  Row 0's workgroup also clears the padding slot of
// R and ids.  Only the upper triangle of dist is read.
__global__ __launch_bounds__(kNjInitThreads) void nj_init_kernel(
	u32 const *__restrict__ dist, u64 dist_pitch, u32 n, double *__restrict__ D, u64 pitch, double *__restrict__ R, u32 *__restrict__ ids)
{
#pragma clang fp contract(off)
	__shared__ double wave_sums[kNjInitThreads / kWave];
	V2M_POISON_LDS(wave_sums);
	u32 const i = blockIdx.x, t = threadIdx.x;
	double sum = 0.0;
	for (u64 j = t; j < pitch; j += kNjInitThreads) {
		double v = 0.0;
		if (j < n && j != i) v = (double) (j > i ? dist[(u64) i * dist_pitch + j] : dist[j * dist_pitch + i]);
		D[(u64) i * pitch + j] = v;
		sum += v;
	}
#pragma unroll
	for (int step = 1; step < kWave; step <<= 1) sum += __shfl_xor(sum, step);
	if (0 == (t & 63)) wave_sums[t >> 6] = sum;
	asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
	__syncthreads();
	if (0 == t) {
		double total = 0.0;
#pragma unroll
		for (int w = 0; w < kNjInitThreads / kWave; ++w) total += wave_sums[w];
		R[i] = total;
		ids[i] = i;
		if (0 == i && pitch > n) { R[n] = 0.0; ids[n] = kNjNone; }
	}
}

// Wave w of workgroup g: row i = g * kNjRowsPerGroup + w, for i < r - 1.  A lane reads two neighbouring slots j, j + 1 (j even) of the
// row, of R and of ids at a time and keeps those with i < j < r; best[i] receives the row's minimum.
__global__ __launch_bounds__(kNjRowminThreads) void nj_rowmin_kernel(
	double const *__restrict__ D, u64 pitch, double const *__restrict__ R, u32 const *__restrict__ ids, u32 r, nj_best *__restrict__ best)
{
#pragma clang fp contract(off)
	int const lane = threadIdx.x & 63;
	u32 const i = blockIdx.x * kNjRowsPerGroup + (threadIdx.x >> 6);
	if (i + 1 >= r) return;
	double const factor = (double) (r - 2), r_i = R[i];
	u32 const id_i = ids[i];
	double const *const row = D + (u64) i * pitch;
	nj_best b = nj_nothing();
#pragma unroll 2
	for (u32 j = ((i + 1) & ~1u) + 2 * lane; j < r; j += 2 * kWave) {
		vec2d const d = *(vec2d const *) (row + j);
		vec2d const r_j = *(vec2d const *) (R + j);
		vec2u const id_j = *(vec2u const *) (ids + j);
#pragma unroll
		for (int e = 0; e < 2; ++e) {
			u32 const jj = j + e;
			if (jj <= i || jj >= r) continue;
			double const product = factor * (e ? d.y : d.x);
			double const sum = r_i + (e ? r_j.y : r_j.x);
			double const q = product - sum;
			u32 const other = e ? id_j.y : id_j.x;
			u32 const lo = id_i < other ? id_i : other, hi = id_i < other ? other : id_i;
			if (nj_better(q, lo, hi, b)) { b.q = q; b.lo = lo; b.hi = hi; b.i = i; b.j = jj; }
		}
	}
	b = nj_wave_best(b);
	if (0 == lane) best[i] = b;
}

// What lane 0 hands the workgroup: the slots of a (the lower id) and b, D(a, b), and the two slots that are written.
struct nj_pick {
	double d_ab;
	u32 slot_a, slot_b;
};

// One workgroup.  (1) The best of best[0 ... r - 2] by the three-key order is the pair (a, b), a the lower id.  (2) Lane 0 writes the
// join's record and R(u).  (3) With p < q the two slots and last = r - 1: every other live slot k computes D(u, k) and its new R; u
// takes slot p, and the taxon of slot `last` moves to slot q (unless q is the last), so k's new slot k' is q for k == last and k
// otherwise.  Reads in (3) are of rows slot_a, slot_b and last at column k and of R[k], by the lane that owns k; writes go to rows p
// and q at column k', to column p and q of row k', and to R[k'] -- no lane reads what another writes: rows slot_a and slot_b are
// {p, q}, read at column k only by k's own lane before it writes there; row `last` is never written (k' is never `last`); and
// D(a, b), R(a), R(b), ids are read in (1) and (2), behind a barrier.
__global__ __launch_bounds__(kNjJoinThreads) void nj_join_kernel(
	double *D, u64 pitch, double *R, u32 *ids, u32 r, u32 new_id, nj_best const *__restrict__ best, v2m_nj_node *__restrict__ node)
{
#pragma clang fp contract(off)
	__shared__ nj_best wave_best[kNjJoinThreads / kWave];
	__shared__ nj_pick pick;
	V2M_POISON_LDS(wave_best);
	V2M_POISON_LDS(pick);
	u32 const t = threadIdx.x;
	nj_best b = nj_nothing();
	for (u32 i = t; i + 1 < r; i += kNjJoinThreads) {
		nj_best const o = best[i];
		if (nj_better(o.q, o.lo, o.hi, b)) b = o;
	}
	b = nj_wave_best(b);
	if (0 == (t & 63)) wave_best[t >> 6] = b;
	asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
	__syncthreads();
	u32 const last = r - 1;
	if (0 == t) {
		b = wave_best[0];
#pragma unroll
		for (int w = 1; w < kNjJoinThreads / kWave; ++w) {
			nj_best const o = wave_best[w];
			if (nj_better(o.q, o.lo, o.hi, b)) b = o;
		}
		bool const a_first = ids[b.i] == b.lo;
		u32 const slot_a = a_first ? b.i : b.j, slot_b = a_first ? b.j : b.i;
		double const d_ab = D[(u64) slot_a * pitch + slot_b], r_a = R[slot_a], r_b = R[slot_b];
		double const delta = (r_a - r_b) / (double) (r - 2);
		double const len_a = 0.5 * (d_ab + delta);
		double const len_b = d_ab - len_a;
		v2m_nj_node out;
		out.a = b.lo; out.b = b.hi; out.c = kNjNone; out.reserved = 0;
		out.len_a = len_a; out.len_b = len_b; out.len_c = 0.0;
		*node = out;
		u32 const p = b.i, q = b.j;   // p < q
		u32 const moved = ids[last];
		double const product = (double) r * d_ab;
		R[p] = 0.5 * ((r_a + r_b) - product);
		ids[p] = new_id;
		D[(u64) p * pitch + p] = 0.0;
		if (q != last) {
			ids[q] = moved;
			D[(u64) q * pitch + q] = 0.0;
		}
		pick.d_ab = d_ab; pick.slot_a = slot_a; pick.slot_b = slot_b;
	}
	asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
	__syncthreads();
	double const d_ab = pick.d_ab;
	u32 const slot_a = pick.slot_a, slot_b = pick.slot_b;
	u32 const p = slot_a < slot_b ? slot_a : slot_b, q = slot_a < slot_b ? slot_b : slot_a;
	bool const move = q != last;
	double const *const row_a = D + (u64) slot_a * pitch, *const row_b = D + (u64) slot_b * pitch, *const row_last = D + (u64) last * pitch;
	double *const row_p = D + (u64) p * pitch, *const row_q = D + (u64) q * pitch;
	for (u32 k0 = t; k0 < r; k0 += kNjJoinBatch * kNjJoinThreads) {
		double d_ak[kNjJoinBatch], d_bk[kNjJoinBatch], d_lk[kNjJoinBatch], r_k[kNjJoinBatch];
		bool live[kNjJoinBatch];
#pragma unroll
		for (int e = 0; e < kNjJoinBatch; ++e) {
			u32 const k = k0 + e * kNjJoinThreads;
			live[e] = k < r && k != slot_a && k != slot_b;
			d_ak[e] = live[e] ? row_a[k] : 0.0;
			d_bk[e] = live[e] ? row_b[k] : 0.0;
			r_k[e] = live[e] ? R[k] : 0.0;
			d_lk[e] = live[e] && move && k != last ? row_last[k] : 0.0;
		}
#pragma unroll
		for (int e = 0; e < kNjJoinBatch; ++e) {
			if (!live[e]) continue;
			u32 const k = k0 + e * kNjJoinThreads;
			u32 const k_new = k == last ? q : k;
			double const s = d_ak[e] + d_bk[e];
			double const d_uk = 0.5 * (s - d_ab);
			row_p[k_new] = d_uk;
			D[(u64) k_new * pitch + p] = d_uk;
			R[k_new] = (r_k[e] - s) + d_uk;
			if (move && k != last) {
				row_q[k] = d_lk[e];
				D[(u64) k * pitch + q] = d_lk[e];
			}
		}
	}
}

// One wave's lane 0: the three taxa left, in slots 0, 1 and 2, ordered by id, and the trifurcation's record.
__global__ __launch_bounds__(kWave) void nj_last_kernel(double const *__restrict__ D, u64 pitch, u32 const *__restrict__ ids, v2m_nj_node *__restrict__ node)
{
#pragma clang fp contract(off)
	if (0 != threadIdx.x) return;
	u32 s0 = 0, s1 = 1, s2 = 2;
	if (ids[s1] < ids[s0]) { u32 const x = s0; s0 = s1; s1 = x; }
	if (ids[s2] < ids[s1]) { u32 const x = s1; s1 = s2; s2 = x; }
	if (ids[s1] < ids[s0]) { u32 const x = s0; s0 = s1; s1 = x; }
	double const d_ab = D[(u64) s0 * pitch + s1], d_ac = D[(u64) s0 * pitch + s2], d_bc = D[(u64) s1 * pitch + s2];
	v2m_nj_node out;
	out.a = ids[s0]; out.b = ids[s1]; out.c = ids[s2]; out.reserved = 0;
	out.len_a = 0.5 * ((d_ab + d_ac) - d_bc);
	out.len_b = 0.5 * ((d_ab + d_bc) - d_ac);
	out.len_c = 0.5 * ((d_ac + d_bc) - d_ab);
	*node = out;
}

} // namespace v2m
